/*
 * slamhip.h -- C-ABI of libslamhip.so: the MI355X-native CoreSLAM / HectorSLAM hot path.
 *
 * This is the drop-in boundary for mikkleini/slam.net.  The reference is 100 % managed C# with no
 * FFI seam of its own: its hot path is private methods of CoreSLAMProcessor and
 * ScanMatcher/OccGridMap.  The entry points below are what a P/Invoke shim behind the unchanged public
 * C# API (CoreSLAMProcessor / HoleMap / ObstacleMap / ScanMatcher / OccGridMap / MapRepMultiMap /
 * HectorSLAMProcessor) binds; each one cites the reference member it replaces
 * (paths relative to the reference repo).  INTEGRATION.md shows the C# [DllImport] stubs.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, blittable structs only; no callbacks, no exceptions.
 *   - every function returns int32 status: 0 = SLAMHIP_OK, < 0 = error; slamhip_last_error() returns
 *     a thread-local message.  Degenerate *data* (empty scan, robot outside the map, no point in
 *     bounds ...) is a silent no-op exactly as in the reference; negative status is reserved for
 *     API misuse and HIP / RCCL failures.
 *   - host pointers are only read/written during the call (pin with `fixed` / GCHandle); the
 *     library copies in/out and never retains them.  Device memory lives behind opaque handles.
 *   - a handle is single-caller (like the reference objects: ParallelWorker.Work is "blocking,
 *     non-reentrant", BaseSLAM/ParallelWorker.cs:95); different handles may be used from different
 *     threads, also handles that share one slamhip_ctx -- with per-kernel timing off
 *     (slamhip_ctx_timing_enable(ctx, 0), the default: the timers' event pool is not locked): the
 *     context's completion mailbox is guarded by a lock, so the blocking calls of such handles take
 *     turns (they share one HIP stream anyway); give each thread its own context if they should
 *     overlap or be timed.
 *   - calls block until their RESULT is on the host unless the name ends in _async.  Two calls
 *     return as soon as the result the caller reads is there while work that returns nothing is
 *     still running on the device: slamhip_cs_search_and_update / slamhip_csproc_update (back with
 *     the pose; the two map updates run on) and slamhip_hsproc_update (the grid update runs on).
 *     Every later call on the same context is ordered behind that work, so the caller sees the
 *     reference's sequential semantics.  A blocking wait polls a pinned word for up to ~300 us and
 *     then goes on polling it between 20 us sleeps, asking the stream for faults (it never waits for
 *     the stream itself: work queued behind the result is not waited for).
 *   - float poses are (x [m], y [m], theta [rad]) = System.Numerics.Vector3; points are
 *     System.Numerics.Vector2 (8 B); LogOddsCell is {int32 UpdateIndex; float Value} (8 B).
 *   - there is no CPU fallback: every compute entry point launches HIP kernels on gfx950.
 */
#ifndef SLAMHIP_H
#define SLAMHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SLAMHIP_OK            0
#define SLAMHIP_ERR_INVALID  (-1)   /* bad argument / API misuse */
#define SLAMHIP_ERR_HIP      (-2)   /* HIP runtime failure (message in slamhip_last_error) */
#define SLAMHIP_ERR_NOMEM    (-3)
#define SLAMHIP_ERR_STATE    (-4)   /* call order violated (e.g. search before set_scan) */
#define SLAMHIP_ERR_RCCL     (-5)
#define SLAMHIP_ERR_TIMEOUT  (-6)   /* a blocking wait passed its bound; the context is poisoned (slamhip_ctx_set_wait_timeout) */

typedef struct slamhip_ctx    slamhip_ctx;     /* one GPU + one HIP stream */
typedef struct slamhip_cs     slamhip_cs;      /* CoreSLAM device state: HoleMap + ObstacleMap + scan + candidates */
typedef struct slamhip_csproc slamhip_csproc;  /* CoreSLAMProcessor state machine on top of slamhip_cs */
typedef struct slamhip_hs     slamhip_hs;      /* HectorSLAM MapRepMultiMap pyramid + ScanMatcher */
typedef struct slamhip_hsproc slamhip_hsproc;  /* HectorSLAMProcessor state machine on top of slamhip_hs */
typedef struct slamhip_group  slamhip_group;   /* N GPUs in one process + RCCL communicator */
typedef struct slamhip_comm   slamhip_comm;    /* one rank (one process per GPU) of an RCCL communicator */

/* {int UpdateIndex; float Value} -- HectorSLAM/Map/LogOddsCell.cs:16-21 */
typedef struct { int32_t update_index; float value; } slamhip_cell;

/* One job of the scrolling window's backing store (slamhip_hs_set_backing; the planner, slamhip_debug_backing_plan): the
 * intersection of one world tile (tx, ty) of `level` with the cells that leave the window (kind SLAMHIP_BACKING_EVICT: wx, wy in
 * the OLD window's coordinates) or come into it (SLAMHIP_BACKING_RESTORE: in the NEW window's): nx x ny cells from window cell
 * (wx, wy), which is cell (lx, ly) of the tile; lx + nx <= tile, ly + ny <= tile. */
enum { SLAMHIP_BACKING_EVICT = 0, SLAMHIP_BACKING_RESTORE = 1 };
typedef struct slamhip_backing_job {
    int32_t level, kind, wx, wy, nx, ny;
    int64_t tx, ty;
    int32_t lx, ly;
} slamhip_backing_job;

/* One job of slamhip_hs_world_cells_upload (the planner, slamhip_debug_world_plan): nx x ny cells of the caller's rectangle from
 * rectangle cell (sx, sy), which go into the window (kind SLAMHIP_WORLD_WINDOW: (lx, ly) in window coordinates, tx = ty = 0) or
 * into world tile (tx, ty) (SLAMHIP_WORLD_TILE: (lx, ly) in the tile's local coordinates; lx + nx <= tile, ly + ny <= tile). */
enum { SLAMHIP_WORLD_WINDOW = 0, SLAMHIP_WORLD_TILE = 1 };
typedef struct slamhip_world_job { int32_t kind, sx, sy, nx, ny, lx, ly, pad; int64_t tx, ty; } slamhip_world_job;

/* ------------------------------------------------------------------------------------------------
 * Library / context
 * ---------------------------------------------------------------------------------------------- */
const char *slamhip_version(void);
const char *slamhip_last_error(void);
int32_t slamhip_device_count(int32_t *out_count);

/* Replaces `new ParallelWorker(numThreads)` (BaseSLAM/ParallelWorker.cs:34-56): the execution resource
 * the hot path runs on.  One context = one GPU ordinal + one non-blocking HIP stream, the OPERATOR's stream: everything a caller
 * can observe is ordered on it.  (The context also owns three helper streams -- plan launches, the next scan's candidate list,
 * host-mirror pushes -- created and bound to hardware queues together with it: create contexts early and keep them; a
 * process should not need more than one per GPU.) */
int32_t slamhip_ctx_create(int32_t device_ordinal, slamhip_ctx **out);
int32_t slamhip_ctx_destroy(slamhip_ctx *ctx);                     /* ParallelWorker.Dispose :122-139 */
int32_t slamhip_ctx_synchronize(slamhip_ctx *ctx);
int32_t slamhip_ctx_device(slamhip_ctx *ctx, int32_t *out_ordinal);
void   *slamhip_ctx_stream(slamhip_ctx *ctx);                      /* hipStream_t, for interop (RCCL / torch) */
/* Bound on every blocking wait of the context, in milliseconds (default: environment SLAMHIP_WAIT_TIMEOUT_MS, else 10000;
 * <= 0: unbounded).  ParallelWorker.Work waits on its AutoResetEvents without a bound (BaseSLAM/ParallelWorker.cs:106-116): a worker
 * that never signals hangs the reference's caller for ever; here a completion word that does not arrive in time ends the call with
 * SLAMHIP_ERR_TIMEOUT and POISONS the context -- the device's state is unknown, nothing is restarted or re-executed in-process, and
 * every later blocking call (every wait and every hand-over of a result to the host) on the context fails with SLAMHIP_ERR_TIMEOUT
 * at once; enqueue-only calls are not checked.  The bound counts from the start of the wait, work queued in front of the awaited
 * launch included: a caller that queues seconds of asynchronous work in front of a blocking call raises the bound first.  The caller
 * destroys its handles -- slamhip_ctx_destroy of a poisoned context waits for the stream once more, for at most the bound, and then
 * lets go of it (a kernel that never ends would otherwise move the hang into destroy); the process should then exit. */
int32_t slamhip_ctx_set_wait_timeout(slamhip_ctx *ctx, int64_t timeout_ms);
int32_t slamhip_ctx_poisoned(slamhip_ctx *ctx, int32_t *out_flag);
/* Test hook (no device involved): the wait loop of a blocking call on a caller-owned word -- returns SLAMHIP_OK once *flag has
 * reached `val` (wrap-safe), SLAMHIP_ERR_TIMEOUT after timeout_ms. */
int32_t slamhip_debug_flag_wait(volatile uint32_t *flag, uint32_t val, int64_t timeout_ms);
/* Test hook (no device involved): the device and pinned blocks that the Hector units K7 .. K27 of every
 * slamhip_hs of the process hold at this moment, and their bytes.  A unit's block counts from its allocation to its release;
 * slamhip_hs_destroy and the *_clear entry points release a unit's blocks.  The operator's own blocks (the levels, the scan, the
 * K4 / K5 tables), the world staging and the tile pool of slamhip_hs_set_backing are not counted.  Either pointer may be NULL. */
int32_t slamhip_debug_live_blocks(int64_t *out_blocks, int64_t *out_bytes);
/* Test hook (no device involved): the planner of the scrolling window's backing store (slamhip_hs_set_backing) for one shift by
 * (dx, dy) of a pyramid of `levels` levels, level 0 w0 x h0, whose window lies at (ox, oy) before the shift, with tiles of
 * `tile` x `tile` cells.  World cell of window cell (x, y) on level l: ((ox >> l) + x, (oy >> l) + y); tile index floor(X / tile),
 * local coordinate X - tile * floor(X / tile).  The jobs come in the order the shift uses them (and deals tile slots in): level 0
 * first; within a level evict jobs, then restore jobs; within each, row-major by tile (ty, tx).  The departing region (and the
 * arriving one) is the window minus the rectangle both windows share, cut into the band above it, the band below it and the strips
 * left and right of it; a tile gives one job per rectangle it meets, in that order.  *n_jobs receives the number of jobs; if it
 * exceeds `cap`, nothing is written and the call returns SLAMHIP_ERR_INVALID (jobs may be NULL when cap is 0).  levels, w0, h0 as
 * for slamhip_hs_create, tile a power of two in [8, 256]; dx and dy need not be multiples of 1 << (levels - 1) here. */
int32_t slamhip_debug_backing_plan(int32_t levels, int32_t w0, int32_t h0, int64_t ox, int64_t oy,
                                   int32_t dx, int32_t dy, int32_t tile,
                                   slamhip_backing_job *jobs, int32_t cap, int32_t *n_jobs);
/* Test hook (no device involved): the planner of slamhip_hs_world_cells_upload for the rectangle [x0, x0 + rw) x [y0, y0 + rh) in
 * WORLD cells of one level whose window is w x h cells with cell (0, 0) at world cell (OX, OY); tile: the tile side, a power of
 * two in [8, 256], or 0 for backing off.  The jobs come in the order the upload uses them (and deals tile slots in): the window
 * job first (at most one; the rectangle's intersection with the window); then, with tile > 0, the part of the rectangle outside
 * the window, cut as the backing planner cuts a region -- band above the window, band below it, left strip, right strip; the whole
 * rectangle if it misses the window -- row-major by tile (ty, tx), the jobs of one tile in that rectangle order.  With tile = 0 the
 * window job is all there is.  Every cell of the rectangle is in exactly one job with tile > 0.  *n_jobs receives the number of
 * jobs; if it exceeds `cap`, nothing is written and the call returns SLAMHIP_ERR_INVALID (jobs may be NULL when cap is 0).
 * w, h in [1, 32768]; rw, rh >= 1 with rw * rh <= 2^26; |OX|, |OY|, |x0|, |y0| < 2^60. */
int32_t slamhip_debug_world_plan(int32_t w, int32_t h, int64_t OX, int64_t OY, int64_t x0, int64_t y0, int32_t rw, int32_t rh,
                                 int32_t tile, slamhip_world_job *jobs, int32_t cap, int32_t *n_jobs);

/* Test hook (no device involved): the point-cell arithmetic of the pose-lattice search (slamhip_hs_lattice_search) for ONE heading
 * on a level of cell length `cell_length` (stm = 1.0f / cell_length, as slamhip_hs_create forms it): theta is the heading theta_k
 * itself -- (s, c) = the deterministic sine / cosine of theta -- and centre[0], centre[1] the lattice's centre in metres
 * (centre[2] is not read).  out_gxgy[2 i], out_gxgy[2 i + 1] = (gx, gy) of point i as the search's kernel forms them, or
 * INT32_MIN twice for a point the search ignores.  n >= 0; xy and out_gxgy may be NULL when n is 0. */
int32_t slamhip_debug_lattice_cells(float cell_length, const float centre[3], float theta, const float *xy, int32_t n,
                                    int32_t *out_gxgy);
/* Test hook (no device involved): the planner of the class map of slamhip_hs_world_lattice_search for one level whose window is
 * w x h cells with cell (0, 0) at world cell (OX, OY), with tiles of `tile` x `tile` cells; tiles_tytx: n_tiles pairs (ty, tx), the
 * tiles of that level that exist, distinct, in the directory's order (row-major by (ty, tx)); tile = 0 (backing off): n_tiles = 0.
 * out_rect = {x0, y0, w, h}: the rectangle R the class map covers, in WINDOW-FRAME cells -- the bounding box of the window and of
 * every tile, so x0 <= 0 and y0 <= 0.  The jobs, as slamhip_world_job: nx x ny cells that go to R from its cell (sx, sy), read
 * from the window (kind SLAMHIP_WORLD_WINDOW: always the first job, the whole window, lx = ly = tx = ty = 0) or from tile (tx, ty)
 * from its local cell (lx, ly) (SLAMHIP_WORLD_TILE).  The window wins: a tile gives the part of it that lies OUTSIDE the window,
 * cut as the backing planner cuts a region -- band above the window, band below it, left strip, right strip -- and nothing if it
 * lies wholly under the window; tiles in the order given.  Every cell of R is in at most one job; a cell in none is class 0.
 * If R has more than 2^28 cells, its rows padded to whole 16-cell words: out_rect is written, *n_jobs = 0, SLAMHIP_ERR_INVALID.
 * Otherwise *n_jobs receives the number of jobs; if it exceeds `cap`, no job is written and the call returns SLAMHIP_ERR_INVALID
 * (jobs may be NULL when cap is 0).  w, h in [1, 32768]; |OX|, |OY| < 2^60; |ty|, |tx| < 2^52. */
int32_t slamhip_debug_world_pack_plan(int32_t w, int32_t h, int64_t OX, int64_t OY, int32_t tile, const int64_t *tiles_tytx,
                                      int32_t n_tiles, int64_t out_rect[4], slamhip_world_job *jobs, int32_t cap, int32_t *n_jobs);

/* Test hooks (no device involved): the arithmetic of the beam trace (slamhip_hs_trace, THE DEFINITION at slamhip_trace_beam), the
 * text the kernel runs.  slamhip_debug_trace_lines: steps 1 and 2 for the n scan points xy under pose[3] on a level whose
 * ScaleToMap is stm, with scan origin origin[2]: out[5 i .. 5 i + 4] = {bx, by, ex, ey, da} of beam i; an ignored beam reports
 * {0, 0, 0, 0, -1}.  n >= 0; xy and out may be NULL when n is 0.
 * slamhip_debug_trace_cells: step 3 for the line from cell (bx, by) to cell (ex, ey): the walked cells in order, cell 0 first,
 * out_xy[2 j], out_xy[2 j + 1] the cell of step j; *out_n = da + 1 of them.  If that exceeds `cap` nothing is written and the
 * call returns SLAMHIP_ERR_INVALID (out_xy may be NULL when cap is 0).  SLAMHIP_ERR_INVALID, *out_n = 0: |bx|, |by|, |ex| or |ey|
 * >= 2^24, da = 0, or da > SLAMHIP_TRACE_MAX_DA -- no walked beam has such a line. */
int32_t slamhip_debug_trace_lines(float stm, const float pose[3], const float origin[2], const float *xy, int32_t n, int32_t *out);
int32_t slamhip_debug_trace_cells(int32_t bx, int32_t by, int32_t ex, int32_t ey, int32_t *out_xy, int32_t cap, int32_t *out_n);

/* Test hook (no device involved): the distance field (slamhip_hs_distance_field, THE DEFINITION there) over a caller's class array,
 * by the text the kernels run (the class-to-site test, the nearest site of a row by word, the column minimum).  cls: ch rows of cw
 * bytes of class bits (1 occupied, 2 free, 0 neither; only the low two bits are read), cell (0, 0) first; every cell outside
 * [0, cw) x [0, ch) is class 0.  out_d2: h rows of w uint16_t, the field of cells [x, x + w) x [y, y + h) -- any rectangle, the
 * constant outside E included.  SLAMHIP_ERR_INVALID: site_mask outside [1, 7], radius outside [1, 255], w or h < 1, w * h > 2^24,
 * cw or ch < 1, cw * ch > 2^26. */
int32_t slamhip_debug_distance_field(const uint8_t *cls, int32_t cw, int32_t ch, int32_t site_mask, int32_t radius,
                                     int32_t x, int32_t y, int32_t w, int32_t h, uint16_t *out_d2);

/* Kernel timing (the reference only has Stopwatch EMAs, HectorSLAMProcessor.cs:92-96,111-115).
 * When enabled, each kernel class is bracketed by HIP events on the context's stream. */
enum {
    SLAMHIP_K_CS_PREP = 0,      /* candidate transform (pose + offset -> px,py,c,s) */
    SLAMHIP_K_CS_DISTANCE = 1,  /* K1 batched distance (dominant kernel) */
    SLAMHIP_K_CS_REDUCE = 2,    /* K1r partial-sum + arg-min reduce */
    SLAMHIP_K_CS_HOLEMAP = 3,   /* K2 */
    SLAMHIP_K_CS_OBSTACLE = 4,  /* K3 */
    SLAMHIP_K_HS_MATCH = 5,     /* K4 */
    SLAMHIP_K_HS_UPDATE = 6,    /* K5 */
    SLAMHIP_K_HS_LATTICE_PACK = 7, /* K7 class-map pack */
    SLAMHIP_K_HS_LATTICE = 8,   /* K7 pose-lattice search */
    SLAMHIP_K_HS_LATTICE_PACK_WORLD = 9, /* K7 class-map pack of the world search: window and tiles */
    SLAMHIP_K_COUNT = 10
};
/* mask: bit k enables kernel class k (e.g. 1 << SLAMHIP_K_CS_DISTANCE); 0 = off; -1 = all classes */
int32_t slamhip_ctx_timing_enable(slamhip_ctx *ctx, int32_t mask);
int32_t slamhip_ctx_timing_reset(slamhip_ctx *ctx);
/* total milliseconds and launch count accumulated for one kernel class since the last reset
 * (synchronises the stream) */
int32_t slamhip_ctx_timing_get(slamhip_ctx *ctx, int32_t which, double *out_ms, int64_t *out_launches);

/* ------------------------------------------------------------------------------------------------
 * CoreSLAM, operator level
 * ---------------------------------------------------------------------------------------------- */

/* Replaces `new HoleMap(holeMapSize, physicalMapSize)`, `new ObstacleMap(obstacleMapSize, ...)` and
 * the noHitMap (CoreSLAM/CoreSLAMProcessor.cs:131-133; HoleMap.cs:17-22; ObstacleMap.cs:17-22).
 * Scale = sizePixels / sizeMeters in binary32.  Maps are created in the Reset() state. */
int32_t slamhip_cs_create(slamhip_ctx *ctx, float physical_map_size, int32_t hole_map_size,
                          int32_t obstacle_map_size, slamhip_cs **out);
int32_t slamhip_cs_destroy(slamhip_cs *cs);
int32_t slamhip_cs_info(slamhip_cs *cs, int32_t *hole_size, float *hole_scale, int32_t *obst_size, float *obst_scale);

/* CoreSLAMProcessor.Reset map part (:169-170): HoleMap := 32750, ObstacleMap := unmapped_obstacle_hits */
int32_t slamhip_cs_reset(slamhip_cs *cs, int32_t unmapped_obstacle_hits);

/* HoleMap.Pixels (HoleMap.cs:27): ushort[Size*Size] row-major.  n_pixels must equal Size*Size. */
int32_t slamhip_cs_holemap_upload(slamhip_cs *cs, const uint16_t *pixels, size_t n_pixels);
int32_t slamhip_cs_holemap_download(slamhip_cs *cs, uint16_t *pixels, size_t n_pixels);
/* Live HoleMap.Pixels (HoleMap.cs:27; callers read the array directly, Simulation/MainWindow.xaml.cs:229) at the price of what
 * changed: copies into the caller's full-size array only the bounding rectangle of the scans drawn since the previous mirror call
 * (everything on the first call and after reset / upload).  out_rect (optional) = {x0, y0, x1, y1} inclusive, or {0, 0, -1, -1}
 * when nothing changed.  `pixels` must be the array the previous mirror call filled. */
int32_t slamhip_cs_holemap_mirror(slamhip_cs *cs, uint16_t *pixels, size_t n_pixels, int32_t out_rect[4]);
/* The same without stalling the scan (the reference's callers read HoleMap.Pixels live: HoleMap.cs:27,
 * Simulation/MainWindow.xaml.cs:227-249).  From the first call on the HoleMap updates keep, per map row, the span of columns their
 * rays crossed.  _async enqueues behind everything queued so far ONE launch that copies those spans into a shadow map on the
 * device and rests them, and -- on a copy stream, behind an event -- a launch that stores the shadow's spans straight into
 * `pixels`; it returns at once, and the next search starts as soon as the snapshot is taken.  _wait blocks until the last push
 * has landed; out_rect = the bounding rectangle x0, y0, x1, y1 of what it refreshed (x1 < x0: nothing), *out_pixels = the pixels
 * of its spans.  After _wait, `pixels` equals a full download taken at the moment of the _async call.
 * Contract: `pixels` must stay alive, and must not be read, between _async and _wait (the caller passes it once; _wait uses it).
 * WHERE THE DEVICE WRITES depends on the array: one that OWNS its pages -- it starts on a 4096-byte boundary and is a whole number
 * of pages long (posix_memalign, NativeMemory.AlignedAlloc, mmap; 8 MiB at 2048^2) -- is page-locked and mapped into the device's
 * address space on its first use (hipHostRegister) and written by the device directly; it stays registered until
 * slamhip_cs_holemap_mirror_release, slamhip_cs_destroy, or a call with another array.  Any other array (a managed array on the
 * pinned object heap, a NumPy array: they share their first and last page with other objects, which the runtime pins for its own
 * copies -- registering such pages ended in device write faults in the randomised soak) is served through a pinned staging buffer
 * of the library's, and _wait copies the changed row ranges into it on the HOST (a pass over what changed; measured at 2048^2 with
 * a moving robot: 225 us per scan against 164 with a request per scan).  One push is in flight at a time: _async waits for the
 * previous one first.  The blocking slamhip_cs_holemap_mirror follows the same rule for its copies. */
int32_t slamhip_cs_holemap_mirror_async(slamhip_cs *cs, uint16_t *pixels, size_t n_pixels);
int32_t slamhip_cs_holemap_mirror_wait(slamhip_cs *cs, int32_t out_rect[4], int64_t *out_pixels);
int32_t slamhip_cs_holemap_mirror_release(slamhip_cs *cs);   /* waits, then unregisters the array (either mirror form) */
/* HoleMap.GetPackedPixels (HoleMap.cs:44-55): 4-bit packing done on the device; n_bytes = Size*Size/2 */
int32_t slamhip_cs_holemap_download_packed(slamhip_cs *cs, uint8_t *packed, size_t n_bytes);
/* ObstacleMap.Pixels (ObstacleMap.cs:31): sbyte[Size,Size], [y,x] row-major */
int32_t slamhip_cs_obstaclemap_upload(slamhip_cs *cs, const int8_t *pixels, size_t n_pixels);
int32_t slamhip_cs_obstaclemap_download(slamhip_cs *cs, int8_t *pixels, size_t n_pixels);

/* The ScanCloud of the current Update (output of ScanSegmentsToCloud, CoreSLAMProcessor.cs:187-207):
 * n_points robot-frame points (x,y).  Kept on the device for the search and both map updates.  xy may be reused as soon as the
 * call returns.  (On a device with a large BAR the call stores the scan straight into one of two alternating device blocks --
 * CPU stores, no upload launch -- whenever it knows that block idle; otherwise the first launch that reads the scan uploads it.
 * SLAMHIP_NO_DIRECT_UPLOAD=1 always takes the second way.) */
int32_t slamhip_cs_set_scan(slamhip_cs *cs, const float *xy, int32_t n_points);

/* CalculateDistance (CoreSLAMProcessor.cs:215-259) for K candidates in one batched kernel.
 * pxcs is K x 4: px = x*Scale+0.5f, py = y*Scale+0.5f, c = cos(theta)*Scale, s = sin(theta)*Scale
 * (:232-235) computed by the caller, so the CRT trig stays on the host and every distance is
 * bit-exact with the reference for the same (px,py,c,s).  out_dist (K, may be NULL) receives every
 * distance; the arg-min uses the reference tie-break (first strictly smaller, :644,:700). */
int32_t slamhip_cs_distance_pxcs(slamhip_cs *cs, const float *pxcs, int32_t K, int32_t *out_dist,
                                 int32_t *out_best_index, int32_t *out_best_dist);
/* Same from poses (K x 3: x,y,theta); (px,py,c,s) are formed on the device with the deterministic
 * correctly-rounded float sin/cos (csrc/det_trig.h). */
int32_t slamhip_cs_distance_poses(slamhip_cs *cs, const float *poses, int32_t K, int32_t *out_dist,
                                  int32_t *out_best_index, int32_t *out_best_dist);

/* The pre-drawn jitter list: replaces FillRandomQueues + the Redzen samplers
 * (CoreSLAMProcessor.cs:136-137,:599-612).  offs is n x 3 (dx, dy, dtheta) in the reference draw order
 * X, Y, theta (:635-637), flat thread-major: entry t*iterations+i is thread t's i-th draw.
 * Like the reference's background refill (:692) this is off the search's critical path. */
int32_t slamhip_cs_set_offsets(slamhip_cs *cs, const float *offs, int32_t n);
/* Device-side generation: counter-based Philox4x32-10 + Box-Muller keyed by
 * (seed, stream, index), so a shard of the list has the same values on every GPU. */
int32_t slamhip_cs_generate_offsets(slamhip_cs *cs, int32_t n, float sigma_xy, float sigma_theta,
                                    uint64_t seed, uint64_t stream);
/* The per-scan flow (CoreSLAMProcessor.Update: a fresh list per scan, :662-665) asks for (n, sigmas, seed, stream), then
 * stream + 1, + 2, ...: a slamhip_cs_search_and_update on a generated list prepares the list of stream + 1 ahead, on a stream of
 * its own, while it waits for the pose, and the next slamhip_cs_generate_offsets that asks for exactly that list finds it in
 * place (any other request simply gets what it asks for).  Diagnostics: how many requests were served that way, and how many
 * lists were prepared, since the handle was created. */
int32_t slamhip_cs_prepared_lists(slamhip_cs *cs, uint64_t *out_served, uint64_t *out_prepared);
/* Opt-in, no reference counterpart (the reference draws every candidate's heading independently, :599-612): the same generator
 * with the headings on a LATTICE -- the candidates one lane of the search kernel evaluates (2 per lane below 65 536 candidates, 4
 * from there on) share their dtheta bit for bit and differ in their translation; the headings are the strata of
 * N(0, sigma_theta), one per lane position (n / 2 or n / 4 distinct headings instead of n), the translations N(0, sigma_xy) as
 * before.  A full-range search over such a list forms the products c*X, s*Y, s*X, c*Y of a ray point once per lane instead of
 * once per candidate: 2 (3) of the ~12.75 vector operations per candidate and ray less, every candidate's distance the float
 * arithmetic of :240-241 as ever (the list can be downloaded and handed to any checker).  Same (seed, stream, index) keying.
 * Up to 12 288 candidates the search evaluates one candidate per lane (smaller groups, faster there) and the call produces the
 * plain list of slamhip_cs_generate_offsets. */
int32_t slamhip_cs_generate_offsets_lattice(slamhip_cs *cs, int32_t n, float sigma_xy, float sigma_theta,
                                            uint64_t seed, uint64_t stream);
int32_t slamhip_cs_offsets_download(slamhip_cs *cs, float *offs, int32_t n);
/* Known-answer access to the generator's integer stream (what FillRandomQueues' Redzen samplers, CoreSLAMProcessor.cs:599-612, are
 * replaced by has no reference vectors of its own, so it is pinned to its published specification instead): ONE Philox4x32-10 block
 * computed on the device -- counter[4], key[2] -> out[4] -- to be compared with Random123's kat_vectors (tests/test_gpu_coreslam.py;
 * the same vectors pin the NumPy restatement, oracle/np_oracle.py: philox4x32_10, philox_jitters).  Jitter i of a generated list uses
 * counter (i, 0, stream low, stream high) and key (seed low, seed high). */
int32_t slamhip_ctx_philox4x32_10(slamhip_ctx *ctx, const uint32_t counter[4], const uint32_t key[2], uint32_t out[4]);

/* ParallelMonteCarloSearch / SingleMonteCarloSearch (CoreSLAMProcessor.cs:624-710) over the flat
 * candidate list: candidate 0 = search_pose itself (:626-628), candidate k = search_pose + offs[k-1].
 * Returns the winning pose, its distance and its flat index. */
int32_t slamhip_cs_search(slamhip_cs *cs, const float search_pose[3], float out_pose[3],
                          int32_t *out_dist, int32_t *out_index);
/* Shard of the same search: only flat candidates [first, first+count) are evaluated.  The result is
 * the packed key (uint64(distance) << 32) | flat_index; min over shards == the full search
 * (cross-thread arg-min :695-705; cross-GPU: one RCCL min all-reduce of this key). */
int32_t slamhip_cs_search_shard(slamhip_cs *cs, const float search_pose[3], int32_t first, int32_t count,
                                uint64_t *out_key);
/* Asynchronous form: enqueues on the context's stream and writes the key to DEVICE memory d_out_key
 * (8 bytes, e.g. a torch tensor fed to an RCCL all-reduce on the same stream). */
int32_t slamhip_cs_search_shard_async(slamhip_cs *cs, const float search_pose[3], int32_t first,
                                      int32_t count, uint64_t *d_out_key);
/* Enqueue-only form with a result word owned by the handle: *d_key receives the DEVICE address of the word that holds the packed
 * key once the stream reaches that point -- one of a ring of 4 words, valid until three further RING LAUNCHES on the handle have
 * been enqueued: calls of this function, fused scans (slamhip_cs_search_and_update and its _pxcs form) and the all-reduce forms
 * (slamhip_cs_search_allreduce*, which also overwrite the slot in place with the reduced key) all advance the same ring.  A caller
 * that keeps a word across such calls copies it first (slamhip_cs_key_read).  In RING MODE (the fused scans, the all-reduce forms, SLAMHIP_K1_OVERLAP=0; for this function's default see WHICH STREAM below) no caller memory is involved, so the kernel needs no final arriver: the workgroups that complete
 * candidates min their keys straight into the word (the previous call's launch left it all ones), and the end of the launch is
 * the completion (the cross-thread arg-min of :695-705 as fire-and-forget atomics).  slamhip_cs_key_read waits for the handle's
 * stream and copies one such word to the host.
 * WHICH STREAM: consecutive calls of this function overlap on the device -- every other launch runs in a second stream of the
 * context, not in slamhip_ctx_stream, and the launch's last finisher stores the key into the word (SLAMHIP_K1_OVERLAP=0: all in
 * the operator's stream, the ring mode above).  The word is therefore NOT ordered in slamhip_ctx_stream by this call alone: it is
 * once any other call on the handle has been made (each orders the operator's stream behind the handle's searches first), after
 * slamhip_cs_key_read, and after slamhip_ctx_synchronize, which waits for both streams.  A caller's own work in
 * slamhip_ctx_stream that reads a word goes behind one of those.  The ring's size and the words' validity are unchanged; the fused
 * scans and the all-reduce forms keep their launches in the operator's stream.
 * Backpressure (round 6): every such launch is accompanied by its plan (slamhip_cs_plan_stats), whose buffers exist eight times, so
 * a caller that enqueues searches faster than the device runs them is held in this call until the search seven launches back has
 * started (the device still has six searches queued: nothing idles) -- at most 20 ms or the context's wait bound, whichever is
 * shorter; past that the search is launched without a plan. */
int32_t slamhip_cs_search_shard_enqueue(slamhip_cs *cs, const float search_pose[3], int32_t first, int32_t count,
                                        const uint64_t **d_key);
int32_t slamhip_cs_key_read(slamhip_cs *cs, const uint64_t *d_key, uint64_t *out_key);
/* Recompute the winner's pose from a (possibly all-reduced) key: search_pose + offs[index-1]. */
int32_t slamhip_cs_pose_from_key(slamhip_cs *cs, const float search_pose[3], uint64_t key,
                                 float out_pose[3], int32_t *out_dist, int32_t *out_index);

/* UpdateHoleMap + DrawLaserRayOnHoleMap + ClipRay (CoreSLAMProcessor.cs:320-443,:496-534) with the
 * current scan.  Bit-exact uint16 result including the ray-order dependence of the blend (:431). */
int32_t slamhip_cs_update_holemap(slamhip_cs *cs, const float pose[3], float hole_width, int32_t quality);
int32_t slamhip_cs_update_holemap_pxcs(slamhip_cs *cs, const float pxcs[4], float hole_width, int32_t quality);
/* UpdateObstacleMap + DrawLaserRayOnObstacleMap (:456-490,:540-593) */
int32_t slamhip_cs_update_obstaclemap(slamhip_cs *cs, const float pose[3], int32_t max_obstacle_hits);
int32_t slamhip_cs_update_obstaclemap_pxcs(slamhip_cs *cs, const float pxcs[4], int32_t max_obstacle_hits);
/* number of pixels blended by the last HoleMap update (4 algorithmic bytes each); after
 * slamhip_cs_search_and_update the figure is fetched here (this call then waits for the update) */
int32_t slamhip_cs_last_holemap_pixels(slamhip_cs *cs, int64_t *out_pixels);
/* Replica check (no reference counterpart; SURVEY.md sec.8e: on several GPUs the map updates run as replicas, kept
 * bit-identical by the integer-exact kernels): 64-bit checksums of the HoleMap (out[0]; HoleMap.cs:27 Pixels as uint16) and
 * the ObstacleMap (out[1]; ObstacleMap.cs:25 as bytes) behind everything enqueued so far:
 *     sum over i of mix64(i << 32 | element_i) mod 2^64,  mix64 = the SplitMix64 finaliser
 * (position-sensitive, order-independent; a host can recompute it from a download). */
int32_t slamhip_cs_maps_checksum(slamhip_cs *cs, uint64_t out[2]);

/* Diagnostics: with the environment variable SLAMHIP_K1_VERIFY=1 the distance kernel checks every end
 * point against the LDS tile box it derived by interval arithmetic and counts violations (always 0 when
 * the box reasoning holds; the parity tests assert it).  Returns the count accumulated so far. */
int32_t slamhip_cs_selfcheck_failures(slamhip_cs *cs, uint32_t *out_failures);

/* The whole self-check block, read-only (same copy as slamhip_cs_selfcheck_failures).  The words move only under
 * SLAMHIP_K1_VERIFY=1 and accumulate over the handle's life:
 *   [0] failures (the word slamhip_cs_selfcheck_failures returns; must stay 0)
 *   [1] ray units of SHARED tile steps    [3] ray units of GLOBAL steps    [4] ray units of BAND steps
 *       (a step of n rays adds 4 n, once per workgroup that runs it)
 *   [5] search workgroups that found their plan record, [6] that did not (searches launched with a plan only)
 *   [2], [7] unused (0). */
int32_t slamhip_cs_selfcheck_counts(slamhip_cs *cs, uint32_t out[8]);

/* Diagnostics of slamhip_cs_scan_search_and_update / slamhip_csproc_update (CoreSLAMProcessor.cs:717-752): the search launch of a scan goes
 * into the stream BEFORE the scan's tables are made and waits for them on the device (DESIGN.md sec.4 "The per-scan flow").
 * out[0] scans searched that way, out[1] such launches abandoned (the last scan's launch layout did not serve the new scan: searched
 * again in the ordinary order), out[2] scans whose layout had to be remade first, out[3] scans refused (first scans, a changed ray
 * count, a new candidate list, SLAMHIP_PRELAUNCH=0 ...).  The results do not depend on the path taken. */
int32_t slamhip_cs_prelaunch_stats(slamhip_cs *cs, uint64_t out[4]);

/* Diagnostics of the search's PLAN (round 6; replaces nothing in the reference -- it takes the per-workgroup planning of the batched
 * CalculateDistanceSISD, CoreSLAMProcessor.cs:226-259, off the search launch's critical path): every search launch of the
 * tiled kernel in its enqueue-only form is accompanied by one small launch on a stream of its own that leaves each workgroup's tile
 * steps (bounds -> boxes -> steps: what its prologue would work out in front of its first tile) in device memory, stamped; a workgroup
 * uses the record that carries its stamp and plans for itself otherwise.
 * out[0] searches launched with a plan, out[1] without (blocking searches, explicit pose lists, lattice lists, prelaunched searches,
 * SLAMHIP_K1_PLAN=0), out[2] times the host waited for a free plan slot (it was seven searches ahead of the device), out[3] plans not launched because a
 * launch that writes their inputs (candidate gather, scan upload) had not been seen to finish.  Results never depend on the path. */
int32_t slamhip_cs_plan_stats(slamhip_cs *cs, uint64_t out[4]);

/* Fused configuration C3 (device boundary at CoreSLAMProcessor.cs:732,:750,:751): search, NormalizeAngle
 * (:746) and both map updates in one call; the winning pose never leaves the device between them.
 * Completion: the call returns when the winning pose is back on the host.  The two map updates are enqueued
 * behind the search on the operator's stream and may still be running; every later call that reads or writes
 * the maps (the next search, an update, a download, an export, destroy) is ordered behind them, so a caller
 * sees the reference's sequential semantics -- it only gets the pose ~40 us earlier and can prepare its next scan
 * meanwhile.  SLAMHIP_FUSED_WAIT_UPDATES=1 restores "return after the updates". */
int32_t slamhip_cs_search_and_update(slamhip_cs *cs, const float search_pose[3], float hole_width,
                                     int32_t quality, int32_t max_obstacle_hits, float out_pose[3],
                                     int32_t *out_dist, int32_t *out_index);
/* slamhip_cs_set_scan + slamhip_cs_search_and_update in ONE call -- a scan of CoreSLAMProcessor.Update from :723 to :751 (the candidate list
 * is set or generated before it: it does not depend on the scan).  Same results as the two calls.  What the one call can do that the
 * two cannot: put the search launch into the stream BEFORE the scan's tables are made (the launch's parameters do not depend on
 * them) and let it wait for them on the device, so that the device does not idle between the previous scan's map update and this
 * search while the host sorts (DESIGN.md sec.4 "The per-scan flow" 5; slamhip_cs_prelaunch_stats counts how often; SLAMHIP_PRELAUNCH=0:
 * never).  slamhip_csproc_update is built on it.  xy: n_points (x, y) pairs in the robot frame, valid during the call. */
int32_t slamhip_cs_scan_search_and_update(slamhip_cs *cs, const float *xy, int32_t n_points, const float search_pose[3], float hole_width,
                                          int32_t quality, int32_t max_obstacle_hits, float out_pose[3], int32_t *out_dist,
                                          int32_t *out_index);
/* The same scan with the CALLER's trigonometry, end to end: the reference forms c = MathF.Cos(theta) * Scale, s = MathF.Sin(theta) * Scale
 * with the platform CRT, in CalculateDistanceSISD (:232-235) and again for the two map updates of the winner (:499-502 at the
 * HoleMap's scale, :545-548 at the ObstacleMap's -- from the pose AFTER NormalizeAngle :746, whose float arithmetic moves theta by
 * up to an ulp of 2 pi even inside (-pi, pi]), and a .NET host that wants results IDENTICAL to its own MathF -- not to this
 * library's deterministic routine -- hands in what it computed.  Two forms:
 *   slamhip_cs_search_and_update_pxcs: the K candidates as K x 4 (px, py, c, s) at the HoleMap's scale for the search (flat order:
 *     index 0 is the un-jittered search pose, then MonteCarloSearch's draws thread by thread, :626-649), and the K candidates'
 *     rows for the updates -- from the NORMALISED pose -- at the HoleMap's and the ObstacleMap's scale (NULL: no ObstacleMap update).
 *     The call evaluates every candidate, keeps the first strict minimum in flat order (:644-648, :698-705; index 0 when no point
 *     of any candidate lies in the map, :257), and draws both updates from row `index` of the caller's update arrays (only that
 *     row is read: the arrays stay on the host);
 *   slamhip_cs_distance_pxcs, then slamhip_cs_update_maps_pxcs with the winner's two rows: for a host that would rather form the
 *     update rows of ONE pose after the search than of all K before it (what the C# shim's TrigMode.Host does).
 * The pose itself never crosses the boundary: the caller knows candidate `index`.  Blocking; every integer output -- distances,
 * index, both maps -- is bit-exact with the C# on any platform BY CONSTRUCTION. */
int32_t slamhip_cs_search_and_update_pxcs(slamhip_cs *cs, const float *pxcs_search, const float *pxcs_update_hole,
                                          const float *pxcs_update_obstacle, int32_t K,
                                          float hole_width, int32_t quality, int32_t max_obstacle_hits,
                                          int32_t *out_index, int32_t *out_dist);
/* UpdateHoleMap (:750) and UpdateObstacleMap (:751) of one pose given as its (px, py, c, s) at either scale (pxcs_obstacle NULL:
 * the HoleMap only): both enqueued, one wait. */
int32_t slamhip_cs_update_maps_pxcs(slamhip_cs *cs, const float pxcs_hole[4], const float pxcs_obstacle[4], float hole_width,
                                    int32_t quality, int32_t max_obstacle_hits);

/* The search report: what a caller needs to judge a Monte-Carlo search (ParallelMonteCarloSearch, CoreSLAMProcessor.cs:624-710),
 * which itself returns only the winner.  All K = n_offs + 1 distances of the search are kept on the device, in flat order, and
 * reduced behind the search launch:
 *   dist0      the distance of flat candidate 0, the un-jittered search pose (:626-628): best_dist == dist0 with best_index == 0
 *              means that the search did not improve on the odometry prediction;
 *   runner_*   the second-smallest packed key (dist << 32 | index), n_ties the candidates at best_dist (the winner included):
 *              whether the winner stands clear of the field;
 *   the band set: the SCORED candidates (dist != INT32_MAX) with (int64)dist - best_dist <= band; band = 0 gives the ties.  Over
 *              it n_band and the sums of the jitters (dx, dy, dtheta; candidate 0 has (0, 0, 0)) and of their six products.
 *              Every product is formed in binary64 from two binary32 jitters (exact: 48 significant bits), and the terms are
 *              added in binary64 in an order that depends on K alone (per lane in index order, the lanes and wavefronts of a
 *              workgroup pairwise, the workgroups' partial sums in workgroup order; no floating-point atomics): the same call
 *              returns the same bits.  The host forms mean = sum_off / n_band and covariance = sum_off2 / n_band - mean mean^T;
 *   n_in_map   nb_points (:247) of the WINNER: CalculateDistanceSISD divides by all points (:253) but sums only those that land
 *              in the map (:244-248), so a pose that throws most of the scan off the map can score deceptively low.  It is
 *              evaluated once more for the winner alone -- (px, py, c, s) from search_pose + offs[index - 1] as the search forms
 *              them (:232-235, the library's deterministic cos / sin), :240-244 per ray.
 * If nothing is scored (best_dist == INT32_MAX; best_index = 0 as in :257): n_band = 0, the nine sums are +0.0,
 * n_ties = n_unscored = K, n_in_map = 0.  K == 1: runner_dist = INT32_MAX, runner_index = -1.
 * The library sets no threshold: what margin, spread or in-map share means "lost" depends on the map and the sensor and is the
 * host's decision.
 * Scope: full-range searches only.  The shard, all-reduce and slamhip_group_* forms have no report (a report over one shard
 * describes nothing a caller wants), and the explicit-list calls slamhip_cs_distance_pxcs / _poses return every distance already. */
typedef struct slamhip_search_report {
    double  sum_off[3];     /* over the band set: sum of dx, dy, dtheta (the jitter; candidate 0 has (0,0,0)) */
    double  sum_off2[6];    /* sum of dx*dx, dx*dy, dx*dth, dy*dy, dy*dth, dth*dth */
    int32_t best_dist, best_index;       /* exactly what the plain search returns (:644-648, :695-705) */
    int32_t runner_dist, runner_index;   /* second-smallest packed key (dist << 32 | index); K == 1: INT32_MAX, -1 */
    int32_t dist0;          /* distance of flat candidate 0, the un-jittered search pose (:626-628) */
    int32_t n_candidates;   /* K = n_offs + 1 */
    int32_t n_unscored;     /* candidates with distance int.MaxValue (:257) */
    int32_t n_ties;         /* candidates whose distance == best_dist, the winner included */
    int32_t band;           /* echo of the argument */
    int32_t n_band;         /* size of the band set */
    int32_t n_in_map;       /* nb_points (:247) of the WINNER */
    int32_t n_points;       /* cloud.Points.Count */
} slamhip_search_report;    /* 9 doubles + 12 int32, sizeof(slamhip_search_report) == 120, no padding */
/* slamhip_cs_search with the report: out_pose, best_dist and best_index are bit for bit the plain call's.  The search runs in the
 * ordinary launch order with its per-candidate distances kept, two small launches behind it on the operator's stream make the
 * report, and the call makes one wait.  band < 0 or a null out_report: SLAMHIP_ERR_INVALID. */
int32_t slamhip_cs_search_report(slamhip_cs *cs, const float search_pose[3], int32_t band, float out_pose[3],
                                 slamhip_search_report *out_report);
/* The K distances of the last report search on this handle (slamhip_cs_search_report or a fused report form), flat order.
 * SLAMHIP_ERR_STATE: there has been none, or a search without a report (any form, the explicit-list calls included) ran since;
 * SLAMHIP_ERR_INVALID: K != n_candidates of that search. */
int32_t slamhip_cs_search_distances(slamhip_cs *cs, int32_t *out_dist, int32_t K);
/* slamhip_cs_search_and_update / slamhip_cs_scan_search_and_update with the report: pose, distance, index, both maps and
 * slamhip_cs_maps_checksum are bit-identical to the plain calls.  The report describes the map that was SEARCHED: its launches
 * sit between the search and the map updates on the operator's stream.  The report forms take the ordinary launch order -- no
 * result-ring slot, no plan, no launch of the search ahead of the scan's tables, no candidate list prepared ahead
 * (slamhip_cs_prelaunch_stats, slamhip_cs_plan_stats and slamhip_cs_prepared_lists do not move); the call still returns as
 * soon as pose and report are on the host, with the map updates running on. */
int32_t slamhip_cs_search_and_update_report(slamhip_cs *cs, const float search_pose[3], int32_t band, float hole_width,
                                            int32_t quality, int32_t max_obstacle_hits, float out_pose[3],
                                            slamhip_search_report *out_report);
int32_t slamhip_cs_scan_search_and_update_report(slamhip_cs *cs, const float *xy, int32_t n_points, const float search_pose[3],
                                                 int32_t band, float hole_width, int32_t quality, int32_t max_obstacle_hits,
                                                 float out_pose[3], slamhip_search_report *out_report);

/* ------------------------------------------------------------------------------------------------
 * CoreSLAM, processor level (host-side orchestration in C++, mirrors the public C# class)
 * ---------------------------------------------------------------------------------------------- */

/* new CoreSLAMProcessor(physicalMapSize, holeMapSize, obstacleMapSize, startPose, sigmaXY, sigmaTheta,
 * iterationsPerThread, numSearchThreads)  (CoreSLAMProcessor.cs:119-162).  The candidate list has
 * max(numSearchThreads,1) * iterationsPerThread jitters; it is device-generated from (seed, scan number)
 * unless slamhip_csproc_set_offsets pins it. */
int32_t slamhip_csproc_create(slamhip_ctx *ctx, float physical_map_size, int32_t hole_map_size,
                              int32_t obstacle_map_size, const float start_pose[3], float sigma_xy,
                              float sigma_theta, int32_t iterations_per_thread, int32_t num_search_threads,
                              slamhip_csproc **out);
int32_t slamhip_csproc_destroy(slamhip_csproc *p);                 /* Dispose :757-773 */
int32_t slamhip_csproc_reset(slamhip_csproc *p);                   /* Reset :167-175 */
/* Update(List<ScanSegment>) (:717-752).  Segment i has pose seg_poses[3i..3i+2] and rays
 * [seg_start[i], seg_start[i+1]) of (angle, radius) pairs (BaseSLAM/ScanSegment.cs, Ray.cs). */
int32_t slamhip_csproc_update(slamhip_csproc *p, const float *seg_poses, const int32_t *seg_start,
                              int32_t n_segments, const float *rays);
int32_t slamhip_csproc_get_pose(slamhip_csproc *p, float out_pose[3]);                /* Pose :106 */
/* Quality :80, HoleWidth :85, PositionSearchBeginning :90, UnmappedObstacleHits :96, MaxObstacleHits :101 */
int32_t slamhip_csproc_set_params(slamhip_csproc *p, int32_t quality, float hole_width,
                                  int32_t position_search_beginning, int32_t unmapped_obstacle_hits,
                                  int32_t max_obstacle_hits);
int32_t slamhip_csproc_set_seed(slamhip_csproc *p, uint64_t seed);
/* candidates per scan from slamhip_cs_generate_offsets_lattice instead of slamhip_cs_generate_offsets (default: off) */
int32_t slamhip_csproc_set_lattice(slamhip_csproc *p, int32_t on);
/* pin the jitter list used by the next searching Update (parity tests feed the oracle the same list) */
int32_t slamhip_csproc_set_offsets(slamhip_csproc *p, const float *offs, int32_t n);
/* on = 1: every later searching slamhip_csproc_update runs slamhip_cs_scan_search_and_update_report with this band and keeps the
 * report; poses and maps do not change, the launch order does (see there: the ordinary order, nothing launched ahead).
 * on = 0 (default): Update launches exactly what it launches without this call, and the last report is dropped.  Any other
 * `on` and any negative band: SLAMHIP_ERR_INVALID, the setting unchanged.
 * Cost: two short launches per scan and the launch-ahead flow given up (DESIGN.md sec.4 "The search report");
 * tools/search_report_cost.py measures both modes at 2048^2 / 1080 rays / 16 384 candidates (not measured yet). */
int32_t slamhip_csproc_set_search_report(slamhip_csproc *p, int32_t on, int32_t band);
/* The report of the last searching slamhip_csproc_update (:732); *out_valid = 0 and *out zeroed before the first searching
 * Update (scans before PositionSearchBeginning do not search, :726; nor does a scan with an empty cloud), after
 * slamhip_csproc_reset and while reports are off. */
int32_t slamhip_csproc_get_report(slamhip_csproc *p, slamhip_search_report *out, int32_t *out_valid);
/* the underlying operator-level object (HoleMap / ObstacleMap properties :45,:50) */
int32_t slamhip_csproc_cs(slamhip_csproc *p, slamhip_cs **out_cs);
/* ScanSegmentsToCloud (CoreSLAMProcessor.cs:187-207) on its own, as slamhip_csproc_update runs it on the host: every segment's pose relative to
 * the LAST segment's (the odometry pose, :719), every ray (angle, radius) -> pose.X + radius * cos(angle + pose.Z), pose.Y + radius *
 * sin(angle + pose.Z) with the library's deterministic cos / sin (the correctly rounded float; a C# host that wants its own MathF
 * forms the cloud itself).  seg_poses: n_seg x 3, seg_start: n_seg + 1 ray offsets, rays: (angle, radius) pairs, out_xy: one (x, y)
 * per ray.  No device is involved. */
int32_t slamhip_scan_segments_to_cloud(const float *seg_poses, const int32_t *seg_start, int32_t n_seg, const float *rays, float *out_xy);

/* ------------------------------------------------------------------------------------------------
 * HectorSLAM, operator level
 * ---------------------------------------------------------------------------------------------- */

/* new MapRepMultiMap(mapResolution, mapSize, numDepth, Vector2.Zero) (HectorSLAM/Main/MapRepMultiMap.cs:40-58;
 * OccGridMap ctor Map/OccGridMap.cs:35-48; GridMap ctor Map/GridMap.cs:33-51): level i has
 * (w >> i, h >> i) cells of cell_length * 2^i metres; levels are independent maps. */
int32_t slamhip_hs_create(slamhip_ctx *ctx, float cell_length, int32_t width, int32_t height, int32_t levels,
                          slamhip_hs **out);
int32_t slamhip_hs_destroy(slamhip_hs *hs);
int32_t slamhip_hs_reset(slamhip_hs *hs);                                   /* MapRepMultiMap.Reset :63-66; also resets the probabilities and sets the cache epoch to 0 (deviation D5: slamhip_hs_probability, slamhip_hs_set_reference_cache) */
int32_t slamhip_hs_level_info(slamhip_hs *hs, int32_t level, int32_t *width, int32_t *height, float *cell_length);
/* SetUpdateFactorFree / SetUpdateFactorOccupied (:83-95; OccGridMap.cs:58-79) */
int32_t slamhip_hs_set_factors(slamhip_hs *hs, float update_free_factor, float update_occupied_factor);
/* OccGridMap.EstimateIterations per level (OccGridMap.cs:53; default 3) */
int32_t slamhip_hs_set_iterations(slamhip_hs *hs, const int32_t *iterations_per_level);
/* mapArray of one level (GridMap.cs:13): n_cells = width*height LogOddsCell structs.  An upload leaves the reference's cache
 * and its epoch as they are (slamhip_hs_set_reference_cache): the reference has no upload, and only its own events move them. */
int32_t slamhip_hs_cells_upload(slamhip_hs *hs, int32_t level, const slamhip_cell *cells, size_t n_cells);
int32_t slamhip_hs_cells_download(slamhip_hs *hs, int32_t level, slamhip_cell *cells, size_t n_cells);
/* GridMap.GetBitmapData (GridMap.cs:104-115) computed on the device */
int32_t slamhip_hs_bitmap_download(slamhip_hs *hs, int32_t level, uint8_t *out, size_t n_cells);
/* GridMap.GetMapExtends (GridMap.cs:147-207) reduced on the device: extends = {xMax, yMax, xMin, yMin} of the cells with
 * Value != 0, *found = 1; or all zeros and *found = 0 (also when a minimum never left the reference's start value 10000) */
int32_t slamhip_hs_map_extends(slamhip_hs *hs, int32_t level, int32_t extends[4], int32_t *found);
/* Replica check, as slamhip_cs_maps_checksum: out[0] over the level's log-odds (OccGridCell.Value, OccGridCell.cs, as its
 * binary32 bit pattern), out[1] over its update indices (OccGridCell.UpdateIndex as uint32) */
int32_t slamhip_hs_checksum(slamhip_hs *hs, int32_t level, uint64_t out[2]);
/* OccGridMap.GetCachedProbability (OccGridMap.cs:97-107) for a list of cell indices.  Deviation D5 -- default: the current
 * probability; opt-in: the reference's cache.  The reference's cache is not invalidated by Reset (OccGridMap.cs:244-252
 * resets currCacheIndex but not cacheArray[i].Index, which only the constructor sets to -1, :38-42), so a cell cached in
 * epoch e before a Reset is served its pre-reset probability in epoch e after it.  By default this -- and the matcher,
 * which reads the same grid -- returns exp(v)/(exp(v)+1) of each cell's CURRENT value: a probability never outlives the
 * value it was computed from.  With the reference's cache on (slamhip_hs_set_reference_cache) it answers as that cache does and
 * fills it as the reference's calls do (repeated indices in one list: as the same calls one after another). */
int32_t slamhip_hs_probability(slamhip_hs *hs, int32_t level, const int32_t *indices, int32_t n, float *out);

/* The ScanCloud handed to MatchData / UpdateByScan: points + scan.Pose.xy (ScanCloud.cs:15-20) */
int32_t slamhip_hs_set_scan(slamhip_hs *hs, const float *xy, int32_t n_points, const float scan_origin[2]);

/* ScanMatcher.MatchData(MapRepMultiMap, scan, hintPose) (HectorSLAM/Matcher/ScanMatcher.cs:41-54):
 * all levels x iterations in ONE persistent launch, 3x3 solve on the device. */
int32_t slamhip_hs_match(slamhip_hs *hs, const float hint_pose[3], float out_pose[3]);
/* ScanMatcher.MatchData(OccGridMap, scan, hintPose) (:64-84) on one level */
int32_t slamhip_hs_match_level(slamhip_hs *hs, int32_t level, const float hint_pose[3], int32_t iterations,
                               float out_pose[3]);
/* B independent hints against the same scan and maps in one launch (throughput form) */
int32_t slamhip_hs_match_batch(slamhip_hs *hs, const float *hint_poses, int32_t B, float *out_poses);
/* GetCompleteHessianDerivs (:135-204) at a map-coordinate pose: H row-major 3x3, dTr 3 */
int32_t slamhip_hs_hessian(slamhip_hs *hs, int32_t level, const float pose_map[3], float H[9], float dTr[3]);
/* ScanMatcher(numThreads) (ScanMatcher.cs:28-32,149-195): 0 = the device's own summation order (default);
 * 1..64 = the reference's: ceil(n/T)-point chunks summed sequentially in binary32, partials added in thread order.
 * (64: WaitHandle.WaitAll's limit in ParallelWorker.Work, BaseSLAM/ParallelWorker.cs:113-115.)
 * A host-side setting of this hs, read by every later slamhip_hs_match, _match_level, _match_batch and _hessian and by
 * slamhip_hsproc_update on the processor's own hs (slamhip_hsproc_hs); it survives slamhip_hs_reset.  With T >= 1, H and
 * dTr are the reference's binary32 sums bit for bit, and a batch of any size returns the single match's bits.
 * Any other value: SLAMHIP_ERR_INVALID, the setting unchanged. */
int32_t slamhip_hs_set_match_threads(slamhip_hs *hs, int32_t num_threads);
/* The reference's probability cache (deviation D5; OccGridMap.cs:16-19,38-42,97-107,147,248): on = 1 keeps cacheArray
 * {Value, Index} per cell and level on the device, and every reader of a probability goes through it as
 * GetCachedProbability does (:99-106) -- slamhip_hs_match, _match_level, _match_batch, _hessian, slamhip_hs_probability
 * and slamhip_hsproc_update on the processor's own hs.  A cell cached in epoch e before a slamhip_hs_reset is then served
 * its pre-reset probability in epoch e after it, as the reference serves it.  on = 0 (default): the current probability.
 * The epoch (currCacheIndex) is kept in either mode: every grid update that takes place adds 1, slamhip_hs_reset sets 0.
 * Every switch from off to on sets every entry to Index = -1, the state of a new OccGridMap: fills while the mode was
 * off were never recorded.  The first switch to on allocates 8 bytes per cell and level (42 MiB at 2048^2 x 3 levels);
 * if that fails the call returns SLAMHIP_ERR_NOMEM and the setting is unchanged.  A host-side setting of this hs like
 * slamhip_hs_set_match_threads; it survives slamhip_hs_reset.  Any other value: SLAMHIP_ERR_INVALID, the setting
 * unchanged. */
int32_t slamhip_hs_set_reference_cache(slamhip_hs *hs, int32_t on);

/* The match report: what a caller needs to tell a good match from a bad one, evaluated once more at the pose the match ends on.
 * The report level is level 0 (the finest, the last one matched) for a pyramid match and `level` for slamhip_hs_match_level.
 * Everything is evaluated at pose_map = GetMapCoordsPose(out_pose) on that level (GridMap.cs:133-137; out_pose the world pose
 * the call returns, angle already normalised, ScanMatcher.cs:76): H and dTr are GetCompleteHessianDerivs there
 * (ScanMatcher.cs:135-204) -- what slamhip_hs_hessian(hs, level, pose_map, ...) answers in the same summation mode; H at the
 * solution is what the original Hector matcher hands on as the pose information matrix.  residual is the sum over ALL scan
 * points of funVal * funVal, funVal = 1.0f - M (:164-166), subtract and multiply rounded separately in binary32; a point
 * outside the map has M = 0 (InterpMapValueWithDerivatives returns Vector3.Zero, :214-217) and adds exactly 1, so a pose that
 * throws the scan off the map scores n_points, and cells never observed (probability 0.5) score 0.25 each.  It is summed as H is
 * (slamhip_hs_set_match_threads: T >= 1 in ceil(n/T)-point chunks sequentially, partials in thread order; T = 0 in the device's
 * own order).  n_in_map counts the points for which IsPointOutOfMapBounds is false at pose_map (MapProperties.cs:83-87).
 * n_points == 0: out_pose is the hint (:83) and H, dTr, residual, n_in_map are zero.  With the reference's cache on
 * (slamhip_hs_set_reference_cache) the report's taps observe the cache and never fill it -- an entry of the level's epoch is
 * served, anything else is computed from the cell's current value and not recorded: the reference makes no such evaluation, so
 * it leaves no trace in state that decides later answers across slamhip_hs_reset.
 * The library sets no acceptance threshold: what residual means "lost" depends on the map and the sensor and is the host's
 * decision. */
typedef struct slamhip_match_report {
    float   pose_map[3];   /* GetMapCoordsPose(out_pose) on the report level (GridMap.cs:133-137) */
    float   H[9];          /* row-major 3x3, as slamhip_hs_hessian lays it out (ScanMatcher.cs:198-200) */
    float   dTr[3];        /* :166-172 */
    float   residual;      /* sum over all scan points of funVal * funVal, funVal = 1.0f - M (:164-166) */
    int32_t n_in_map;      /* points for which IsPointOutOfMapBounds is false at pose_map */
    int32_t n_points;
    int32_t level;         /* the report level */
} slamhip_match_report;    /* 19 four-byte fields, sizeof(slamhip_match_report) == 76, no padding */
/* slamhip_hs_match / _match_level / _match_batch with the report of every match, produced in the same launch by the workgroup
 * that ran the match; out_pose is bit for bit the plain call's.  out_reports: B of them. */
int32_t slamhip_hs_match_report(slamhip_hs *hs, const float hint_pose[3], float out_pose[3], slamhip_match_report *out_report);
int32_t slamhip_hs_match_level_report(slamhip_hs *hs, int32_t level, const float hint_pose[3], int32_t iterations,
                                      float out_pose[3], slamhip_match_report *out_report);
int32_t slamhip_hs_match_batch_report(slamhip_hs *hs, const float *hint_poses, int32_t B, float *out_poses,
                                      slamhip_match_report *out_reports);
/* Best of batch (relocalisation: many hints, one answer): the B matches of slamhip_hs_match_batch_report, and the winner picked
 * on the device by a 64-bit minimum over key = (uint64)bits(residual) << 32 | index.  A residual is >= +0, so its bit pattern
 * orders as its value does; a NaN (only from NaN cells uploaded by the caller) sorts after every number; equal residuals go to
 * the lowest index.  Only the winner's pose, its index and its report come back to the host. */
int32_t slamhip_hs_match_best(slamhip_hs *hs, const float *hint_poses, int32_t B, float out_pose[3], int32_t *out_index,
                              slamhip_match_report *out_report);

/* Relocalisation in a loaded map: the pose-lattice (correlative) search -- no reference counterpart (its HectorSLAMProcessor can
 * only Reset, Main/HectorSLAMProcessor.cs:131-138).  The scan is scored against the occupancy grid of ONE pyramid level at every
 * node of a lattice of poses: translations by whole cells of that level around `centre`, headings centre[2] + k * dtheta.  The
 * score is an exact integer correlation, orders of magnitude cheaper per pose than a Gauss-Newton match; only the best few
 * nodes then go to the matcher (slamhip_hs_relocalise).
 * THE DEFINITION (every binary32 operation rounded on its own, no fused multiply-add), with L the level, stm = 1 / cell:
 *   theta_k = centre[2] + (float)k * dtheta; (s, c) = the library's deterministic sine / cosine of theta_k (no normalisation);
 *   cxm = centre[0] * stm, cym = centre[1] * stm;
 *   for a scan point (px, py) in metres, as slamhip_hs_set_scan took it (the scan origin plays no part, as in the matcher):
 *     rx = c * px - s * py, ry = s * px + c * py; fx = rx * stm + cxm, fy = ry * stm + cym; gx = (int)floorf(fx), gy likewise;
 *   the point is ignored for this heading unless fabsf(fx) < 16777216.0f && fabsf(fy) < 16777216.0f (a NaN point is ignored);
 *   cls(x, y) = +1 if the cell's Value > 0.0f (LogOddsCell.IsOccupied), -1 if Value < 0.0f, else 0: +0, -0, NaN, or (x, y)
 *   outside [0, w) x [0, h);
 *   score(k, iy, ix) = sum over the points of cls(gx + ix, gy + iy), an int32, ix in [-nx, nx], iy in [-ny, ny]: a translation
 *   moves every point by whole cells -- this IS the definition, not an approximation of evaluating at the node's pose;
 *   flat = (iy + ny) * (2 nx + 1) + (ix + nx); key[k] = max over the nodes of
 *   ((uint64)((uint32)score ^ 0x80000000u) << 32) | (0xFFFFFFFFu - flat): the highest score, ties to the lowest flat -- the mirror
 *   image of slamhip_hs_match_best's minimum key;
 *   node pose, in the window's frame: ((cxm + (float)ix) * cell, (cym + (float)iy) * cell, theta_k).
 * The frame is the one slamhip_hs_match uses -- the WINDOW's (the contract under slamhip_hs_shift).  The search covers the window
 * only; slamhip_hs_world_lattice_search covers the world behind it.
 * THE WORLD SEARCH is this definition with ONE change: for a window-frame cell (x, y) of level L outside [0, w) x [0, h),
 * cls(x, y) is no longer 0 but the class of WORLD cell ((ox >> L) + x, (oy >> L) + y), (ox, oy) the origin (slamhip_hs_origin):
 * the tile's cell if a tile of the backing store holds it, LogOddsCell.Reset() -- class 0 -- if none does.  Inside the window
 * it is the window's cell: the window wins over a tile's older copy, as in slamhip_hs_world_cells_download and
 * slamhip_hs_world_extends.  Everything else is unchanged to the letter -- centre in the window's frame, the binary32 point-cell
 * arithmetic, the rule |f| >= 2^24, the keys and flat, the node pose -- so with backing off, or with no tile on that level, the
 * world search equals the window search bit for bit. */
typedef struct slamhip_lattice_spec {
    int32_t level;        /* pyramid level searched */
    int32_t nx, ny;       /* half-extents in cells of that level: ix in [-nx, nx], iy in [-ny, ny] */
    int32_t n_theta;      /* headings k = 0 .. n_theta-1 */
    float   centre[3];    /* pose (m, m, rad) in the window's frame: translations are centred here, heading 0 is centre[2] */
    float   dtheta;       /* heading step, rad */
} slamhip_lattice_spec;   /* 8 four-byte fields, sizeof(slamhip_lattice_spec) == 32, no padding */
/* What slamhip_hs_relocalise did: the hints it handed to the matcher and the node the winner started from. */
typedef struct slamhip_reloc_info {
    int32_t n_hints;      /* min(B, n_theta) */
    int32_t best_hint;    /* slamhip_hs_match_best's index among the hints */
    int32_t k, ix, iy;    /* the lattice node of that hint */
    int32_t score;        /* ... and its score */
    int32_t top_score;    /* the score of hint 0, the highest of the lattice */
} slamhip_reloc_info;     /* 7 four-byte fields, sizeof(slamhip_reloc_info) == 28, no padding */
/* What slamhip_hs_relocalise_world did: the fields of slamhip_reloc_info, then the shift. */
typedef struct slamhip_world_reloc_info {
    int32_t n_hints;      /* the hints handed to the matcher: min(B, n_theta) - n_far */
    int32_t best_hint;    /* slamhip_hs_match_best's index among those */
    int32_t k, ix, iy;    /* the lattice node of that hint */
    int32_t score;        /* ... and its score */
    int32_t top_score;    /* the score of the top node, the highest of the lattice */
    int32_t dx, dy;       /* the shift applied (slamhip_hs_shift), in level-0 cells */
    int32_t n_far;        /* hints dropped for lying outside the new window */
} slamhip_world_reloc_info;   /* 10 four-byte fields, sizeof(slamhip_world_reloc_info) == 40, no padding */
/* The search.  Two launches on the operator's stream, behind every grid update, shift and upload already enqueued: one packs the
 * level's cell values into a class map of 2 bits per cell (re-packed on every search; the map belongs to the hs, is allocated by
 * the first search and freed by slamhip_hs_destroy -- an hs that never searches allocates nothing), one scores the lattice and
 * reduces key[k] per heading.  out_keys: n_theta keys.  out_scores: NULL, or the whole volume,
 * n_theta * (2 ny + 1) * (2 nx + 1) scores, k-major, then iy, then ix.  Blocking, with the context's bounded wait; the results
 * come back through pinned staging that the library owns.  It reads cell values only, never probabilities or the reference's
 * cache, so it works with slamhip_hs_set_reference_cache on, and after shifts.
 * SLAMHIP_ERR_INVALID, nothing launched: level out of range, nx or ny outside [0, 4096], n_theta outside [1, 4096], more than
 * 2^26 nodes, a centre or dtheta that is not finite.  SLAMHIP_ERR_STATE: no scan (n_points == 0).  A poisoned context:
 * SLAMHIP_ERR_TIMEOUT. */
int32_t slamhip_hs_lattice_search(slamhip_hs *hs, const slamhip_lattice_spec *spec, uint64_t *out_keys, int32_t *out_scores);
/* The node pose of the definition above for heading k and flat index `flat` (pure host code: no binding restates it).
 * SLAMHIP_ERR_INVALID: a spec the search refuses, k outside [0, n_theta), flat outside [0, (2 ny + 1) * (2 nx + 1)). */
int32_t slamhip_hs_lattice_node_pose(slamhip_hs *hs, const slamhip_lattice_spec *spec, int32_t k, int32_t flat, float out_pose[3]);
/* Search, then refine: the n_theta keys are sorted descending on the host (equal keys: the lower k first) and the first
 * n_hints = min(B, n_theta) -- distinct headings, which is what gives the hints their diversity -- become node poses, in that
 * order, the hints of slamhip_hs_match_best: out_pose and out_report are exactly what that call returns for them.  1 <= B <= 64.
 * The library sets no acceptance threshold, as with the match report.  Errors as slamhip_hs_lattice_search. */
int32_t slamhip_hs_relocalise(slamhip_hs *hs, const slamhip_lattice_spec *spec, int32_t B, float out_pose[3],
                              slamhip_match_report *out_report, slamhip_reloc_info *out_info);
/* The world search (THE WORLD SEARCH above).  Arguments, results, errors, blocking behaviour and pinned staging as
 * slamhip_hs_lattice_search.  The class map covers a rectangle R of the level: the bounding box of the window and of every tile of
 * that level in the host's directory (slamhip_debug_world_pack_plan).  A memset of R's words and ONE pack launch
 * (SLAMHIP_K_HS_LATTICE_PACK_WORLD) over the window and the tiles' parts outside it take the place of the window's pack launch;
 * the search launch is the same kernel, told R's origin.  The job records reach the device in a block the library owns.  One more
 * refusal, nothing launched: SLAMHIP_ERR_INVALID if R has more than 2^28 cells (rows padded to whole 16-cell words: 64 MB of
 * packed map) -- the message gives R's size.  Works with backing off: R is the window. */
int32_t slamhip_hs_world_lattice_search(slamhip_hs *hs, const slamhip_lattice_spec *spec, uint64_t *out_keys, int32_t *out_scores);
/* Relocalise anywhere in the saved world: search the world, bring the window to the winner, refine there.
 *  1. slamhip_hs_world_lattice_search's keys, sorted as slamhip_hs_relocalise sorts them; the first min(B, n_theta) become node poses.
 *  2. With (lx, ly) the top node's pose: cx = (int)floorf(lx * stm0), cy likewise (stm0 = 1 / cell_length of level 0); per axis
 *     q = ((c - w0 / 2) / g) * g (C integer division, toward zero; g = 1 << (levels - 1)) -- slamhip_hsproc_set_scroll's rule with
 *     trigger 0; q = 0 on both axes if |floorf(.)| >= 1e9 on either.  slamhip_hs_shift(qx, qy): the backing store restores what lies there.
 *  3. Every node pose is re-based into the new frame: x - (float)qx * cell0, the product rounded first; y likewise.
 *  4. Hint 0 is kept; a later hint is kept only if fx = x * stm0 and fy = y * stm0 satisfy 0 <= fx < (float)w0 and
 *     0 <= fy < (float)h0 -- it lies in the new level-0 window; the others are counted in n_far.
 *  5. slamhip_hs_match_best over the kept hints, in their order: out_pose and out_report are exactly what that call returns.
 * out_pose is in the NEW window's frame; dx, dy tell the caller how the window moved.  1 <= B <= 64.
 * Checked before anything is launched or moved -- the map, the origin and the backing statistics stay as they were:
 * SLAMHIP_ERR_STATE if backing is off (the shift would destroy the map); SLAMHIP_ERR_INVALID if the reference's cache is on (the
 * shift refuses); the search's own errors. */
int32_t slamhip_hs_relocalise_world(slamhip_hs *hs, const slamhip_lattice_spec *spec, int32_t B, float out_pose[3],
                                    slamhip_match_report *out_report, slamhip_world_reloc_info *out_info);

/* The branch-and-bound pose-lattice search (K24; no reference counterpart): slamhip_hs_lattice_search's keys WITHOUT scoring every
 * node, for lattices far beyond K7's 2^26 nodes.  K7's score is an integer sum of cell classes in {+1, 0, -1}, and a translation
 * moves every point by whole cells; so the sum, over the points, of the HIGHEST class in the 2^h x 2^h window that starts at each
 * point's cell bounds the score of every node of a 2^h x 2^h block of translations from above -- exactly, no tolerance, no floating
 * point.  A search that prunes by that bound returns K7's keys bit for bit, the ties to the lowest flat included.
 * Everything of slamhip_lattice_spec keeps its meaning to the letter: the point-cell arithmetic, ignored points, cls, score, flat,
 * key, the node pose, the window frame, the world variant of cls.
 *  1. Refusals -- SLAMHIP_ERR_INVALID, nothing launched and nothing written: anything slamhip_hs_lattice_search refuses EXCEPT the
 *     2^26-node rule; top outside [0, 8]; world not 0 or 1; reserved != 0; max_blocks < 0 (0 means 2^26); with s = 2^top,
 *     ceil((2 nx + 1) / s) * ceil((2 ny + 1) / s) * n_theta > max_blocks; for world = 1, R of more than 2^28 cells, as
 *     slamhip_hs_world_lattice_search refuses it.  SLAMHIP_ERR_STATE without a scan.
 *  2. Pooled maps.  For h in [0, top] and ALL integer (x, y): P_h(x, y) = max over 0 <= u, v < 2^h of cls(x + u, y + v), cls being 0
 *     outside the map (outside R for the world search).  P_0 = cls.
 *  3. Blocks.  A block is (k, a, b, h), a and b multiples of 2^h, 0 <= a <= 2 nx, 0 <= b <= 2 ny.  It stands for the nodes
 *     ix = a - nx + u, iy = b - ny + v, 0 <= u, v < 2^h, that lie in the lattice.  U(block) = sum over heading k's non-ignored points
 *     of P_h(gx + a - nx, gy + b - ny); E(block) = the same sum with P_0: the exact score of the block's ORIGIN node (u = v = 0),
 *     which always lies in the lattice.  Both are int32.
 *  4. The levels, for h = top down to 0.  F_top is every block of rule 3's grid for every heading.  For every block of F_h:
 *     key[k] = max(key[k], key of (E, flat of the origin node)).  When ALL of F_h has been scored, best[k] = the score in key[k].  A
 *     block SURVIVES iff h > 0 and U >= best[k] -- equality survives, because a tie may hold a lower flat; the comparison uses the
 *     keys as they stand after the whole level, neither fresher nor staler ones, which makes the counts of rule 6 deterministic.
 *     F_(h-1) is the up to four children (k, a + {0, 2^(h-1)}, b + {0, 2^(h-1)}, h - 1) of the survivors whose origin lies in the
 *     lattice.  At h = 0, U = E: one evaluation serves.
 *  5. Capacity.  If |F_(h-1)| > max_blocks the call ends with SLAMHIP_ERR_INVALID after the launches so far; the message gives
 *     h - 1 and the count and says to raise max_blocks or top.  out_keys and out_info are not written.
 *  6. Results.  out_keys: n_theta keys; by rule 2 they equal slamhip_lattice_spec's definition for ANY lattice.  out_info:
 *     blocks[h] = |F_h|, kept[h] = the survivors of level h, entries above top 0, evaluated = the sum of blocks[h], n_levels = top + 1.
 *  7. Blocking and memory.  The call blocks with the context's bounded wait, one wait per level (slamhip_hs_nav_field's batches are
 *     the precedent for several waits in one call); results come back through pinned staging; a poisoned context returns
 *     SLAMHIP_ERR_TIMEOUT.  The unit's blocks belong to the hs: made on first use, freed by slamhip_hs_destroy; an hs that never
 *     calls this allocates nothing.
 * Why the bound holds: a node (u, v) of the block reads cls(gx + a - nx + u, gy + b - ny + v) for each point, one of the cells P_h
 * takes its maximum over; a sum of maxima bounds the sum.  A pruned block has U < best[k] <= the final key's score, so none of its
 * nodes can hold the key; a block with U == best[k] may hold a node of equal score and lower flat and is kept -- on a map where all
 * scores tie (an empty map) nothing is pruned, and the search costs top + 1 times the origin nodes on top of K7's work.
 * Launches per call: K7's pack (window or world) into K7's class map; k24_pool once per height (height 0 copies the class map into
 * the frame with its zero margin, height h doubles the window on the packed words: the maximum by value of the 2-bit codes is the OR
 * of the low bits and the AND of the high bits, a lane per 16-cell word, no unpacking); per level k24_score (a lane per block, the
 * heading's point cells in LDS chunk by chunk, P_h and P_0 gathered from global memory; a wave maximum, then one 64-bit maximum
 * per workgroup on key[k] as in K7), then for h > 0 k24_filter (survivors and children per heading), the counts to the host -- the
 * level's wait; the host forms the per-heading segments and the job table and checks rule 5 -- and k24_emit (the children into
 * their heading's segment; the order inside a segment is free, no output depends on it). */
typedef struct slamhip_bnb_spec {
    slamhip_lattice_spec lattice;      /* offset 0: K7's lattice, every field as there */
    int32_t top;                       /* offset 32: the top height, [0, 8]: top blocks are 2^top x 2^top translations */
    int32_t world;                     /* offset 36: 0 the window (slamhip_hs_lattice_search), 1 the world (slamhip_hs_world_lattice_search) */
    int32_t max_blocks;                /* offset 40: capacity of a level's frontier; 0 means 2^26 */
    int32_t reserved;                  /* offset 44: 0 */
} slamhip_bnb_spec;                    /* sizeof(slamhip_bnb_spec) == 48, no padding */
typedef struct slamhip_bnb_info {
    int32_t top;                       /* offset 0 */
    int32_t n_levels;                  /* offset 4: top + 1 */
    int64_t evaluated;                 /* offset 8: the sum of blocks[h] */
    int32_t blocks[9];                 /* offset 16: |F_h| */
    int32_t kept[9];                   /* offset 52: the survivors of level h */
} slamhip_bnb_info;                    /* sizeof(slamhip_bnb_info) == 88, no padding */
int32_t slamhip_hs_lattice_search_bnb(slamhip_hs *hs, const slamhip_bnb_spec *spec, uint64_t *out_keys, slamhip_bnb_info *out_info);
/* slamhip_hs_relocalise (world = 0: out_info is a slamhip_reloc_info) or slamhip_hs_relocalise_world (world = 1: steps 1 - 5 with
 * the same pre-checks; out_info is a slamhip_world_reloc_info), fed from the keys of slamhip_hs_lattice_search_bnb: the same host
 * text runs behind both searches, so pose, report and info are those calls' bit for bit wherever K7 accepts the lattice.
 * out_bnb: the search's info.  1 <= B <= 64. */
int32_t slamhip_hs_relocalise_bnb(slamhip_hs *hs, const slamhip_bnb_spec *spec, int32_t B, float out_pose[3],
                                  slamhip_match_report *out_report, void *out_info, slamhip_bnb_info *out_bnb);
/* Test hook (no device involved): rules 1 - 6 over a plain array of w x h cell values (row-major, as slamhip_hs_cells_download gives
 * them) of cell_length metres, the window case (world must be 0; lattice.level is not looked at), for the n points of xy.  It shares
 * the pooling step and the block arithmetic (hs_bnb.h) with the kernels. */
int32_t slamhip_debug_lattice_bnb(const float *values, int32_t w, int32_t h, float cell_length, const slamhip_bnb_spec *spec,
                                  const float *xy, int32_t n, uint64_t *out_keys, slamhip_bnb_info *out_info);

/* The beam trace (K8; no reference counterpart): what the map of ONE level holds ALONG every beam of the scan, from many poses
 * at once.  The matcher and the lattice search consult the map at beam end points only; this walks the grid update's own line
 * from the sensor cell to the beam's end cell and reads the class of every cell on it.  One operation, three uses: the check of
 * a pose that end points cannot give (a pose whose beams pass through walls the map holds: n_blocked), the expected scan (the
 * range the map predicts for a beam: first, hx, hy), and the unknown cells a pose would see (unknown_cells).
 * THE DEFINITION (every binary32 operation rounded on its own, no fused multiply-add), for level L with stm = its ScaleToMap, a
 * pose P = (x, y, theta) in the WINDOW's frame as slamhip_hs_update_by_scan takes it, and the scan and scan origin as
 * slamhip_hs_set_scan took them:
 *  1. t = Rotation(theta) * Translation(x, y) * Scale(stm), the Matrix3x2 product the grid update forms (OccGridMap.cs:120-123);
 *     (bxf, byf) = Transform(origin, t), (exf, eyf) = Transform(point, t); b = (int)rintf(.) of the former, e of the latter:
 *     banker's rounding, as the update's ToRoundPoint (:127, :134).
 *  2. The beam is IGNORED (da = -1) if any of the four floats fails fabsf(f) < 16777216.0f (a NaN fails), or if
 *     max(|ex - bx|, |ey - by|) > SLAMHIP_TRACE_MAX_DA: the cap keeps da / 2 + a * db below 2^31 and bounds the walk.  It is the
 *     SAME beam (da = 0) if b == e: the update draws nothing (:137).  Otherwise it is WALKED, da = max(|dx|, |dy|) >= 1.
 *  3. The walk: cell 0 is b; for a = 1 .. da - 1 the cell at major offset a and minor offset sign * ((da / 2 + a * db) / da), db
 *     the minor length, the major axis x iff |dx| >= |dy| (the closed form of Bresenham2D, :220-239); cell da is e.  This is
 *     exactly the list of cells the update would touch for that beam, and it is NOT cut at the window: a cell outside
 *     [0, w) x [0, h) has class 0 (the lattice search's rule).  In the WORLD variant such a cell has the class of world cell
 *     ((ox >> L) + x, (oy >> L) + y): the tile's cell if a tile of the backing store holds it, else 0 -- THE WORLD SEARCH's rule.
 *     Classes: 1 occupied (Value > 0.0f), 2 free (Value < 0.0f), 0 neither.
 *  4. Per beam, slamhip_trace_beam.  5. Per pose, slamhip_trace_summary.  The library sets no threshold and forms no score.
 * unknown_cells counts a cell once per beam that crosses it -- the cells next to the sensor hundreds of times -- so it does not
 * compare two poses; the DISTINCT cells a pose sees are slamhip_hs_view_gain's (K15). */
#define SLAMHIP_TRACE_MAX_DA 32768
typedef struct slamhip_trace_beam {
    int32_t da;           /* -1 ignored, 0 same, else the major length of the walked line */
    int32_t first;        /* the smallest a in [0, da] whose cell is occupied, or -1 */
    int32_t n_unknown;    /* the class-0 cells among a < stop, stop = first if first >= 0, else da + 1 */
    int32_t end_class;    /* the class bits of e */
    int32_t hx, hy;       /* the cell of step `first` in window-frame cells of the level; 0, 0 if there is none */
} slamhip_trace_beam;     /* 6 four-byte fields, 24 bytes, no padding; da <= 0: first = -1, every other field 0 */
typedef struct slamhip_trace_summary {
    int32_t n_walked, n_same, n_ignored;   /* the beams by status: they sum to n_points */
    int32_t n_end_hit;    /* first == da: the beam reaches its end cell and the map holds an obstacle there */
    int32_t n_blocked;    /* 0 <= first < da: the map holds an obstacle in front of the end cell */
    int32_t n_end_free;   /* first == -1 and end_class == 2: the map says free where the scan saw an obstacle */
    int64_t unknown_cells;   /* the sum of n_unknown */
} slamhip_trace_summary;  /* six int32_t, then one int64_t: 32 bytes, no padding */
/* The trace of the scan that was set, on `level`, at B poses (poses: B x 3 floats, window frame).  world: 0 the window, 1 the
 * world behind it.  out_summaries: B records.  out_beams: NULL, or B x n_points records, pose-major.
 * The launches, on the operator's stream behind every grid update, shift and upload already enqueued: the lattice search's class
 * map of the level, re-packed on every call (its pack launch and timing class for the window; the memset, the planner and the pack
 * launch of slamhip_hs_world_lattice_search for the world), a memset of the summaries, and ONE trace launch, a beam per lane.  The
 * blocks belong to the hs, are made by the first trace and freed by slamhip_hs_destroy.  Blocking, with the context's bounded
 * wait; the results come back through pinned staging that the library owns.  It reads cell values only, so it works with backing
 * off (world = window), with slamhip_hs_set_reference_cache on, and after shifts; it changes nothing of the map or of any search.
 * A pose that is not finite is no error: its beams are ignored.
 * SLAMHIP_ERR_INVALID, nothing launched: level out of range, B outside [1, 65536], out_beams given with B * n_points > 2^20, world
 * not 0 or 1, the world's rectangle over 2^28 cells.  SLAMHIP_ERR_STATE: no scan.  A poisoned context: SLAMHIP_ERR_TIMEOUT. */
int32_t slamhip_hs_trace(slamhip_hs *hs, int32_t level, const float *poses, int32_t B, int32_t world,
                         slamhip_trace_summary *out_summaries, slamhip_trace_beam *out_beams);

/* The distance field of the map and the end-point distance score (K9; no reference counterpart): how far every cell of ONE
 * level lies from the nearest mapped obstacle (or free cell, or unknown cell), as exact squared cell distances, and how far the end
 * points of the scan lie from them at many poses -- the likelihood-field (end-point) model's raw material, smooth in the pose where
 * the lattice search's exact-cell score drops to zero one cell off the wall; the same field gives clearance for obstacle inflation
 * and, with bit 0 of the site mask, the distance to the unknown.
 * THE DEFINITION, for level L, world in {0, 1}, site_mask in [1, 7] and radius r in [1, 255]:
 *  1. cls(x, y), the class of window-frame cell (x, y) of level L, is the beam trace's rule in class bits: 1 occupied (Value >
 *     0.0f), 2 free (Value < 0.0f), 0 neither.  Window variant: a cell outside [0, w) x [0, h) has class 0.  World variant: such a
 *     cell has the class of world cell ((ox >> L) + x, (oy >> L) + y): the tile's cell if a tile of the backing store holds it,
 *     else 0.
 *  2. A cell is a SITE iff bit cls(x, y) of site_mask is set: bit 0 unknown, bit 1 occupied, bit 2 free.  site_mask = 2 is "distance
 *     to obstacles", 3 "to obstacles or the unknown", 1 "to the unknown", 7 makes every cell a site.
 *  3. D2(x, y) = min over all sites (sx, sy) of (sx - x)^2 + (sy - y)^2, and the field is F(x, y) = min(D2(x, y), r^2), a uint16_t
 *     (r^2 <= 65025), defined for EVERY integer cell of the plane.  It is exact: a site with |dx| > r or |dy| > r has a squared
 *     distance above r^2 and cannot lower F, so looking only r cells each way is no approximation.
 *  4. Where it is computed.  Let M = (x0, y0, w, h) be the rectangle of the class map -- the window, or the world's rectangle R (the
 *     bounding box of the window and of every tile of the level) -- and E be M grown by r cells on every side.  Every cell outside
 *     M is class 0.  A cell outside E is more than r cells from M on one axis, so no site INSIDE M reaches it; all other cells are
 *     class 0, sites iff bit 0 of site_mask is set, and then the cell itself is one.  Hence outside E, F is the constant
 *     (site_mask & 1) ? 0 : r^2.  The device field covers E only, and both calls return that constant outside E.
 *  5. The end cell of a scan point at a pose P = (x, y, theta) in the WINDOW's frame, as slamhip_hs_update_by_scan takes it:
 *     t = Rotation(theta) * Translation(x, y) * Scale(stm) as the beam trace forms it, (exf, eyf) = Transform(point, t),
 *     e = (int)rintf(.), banker's rounding: the cell the grid update would mark.  The point is IGNORED unless both floats satisfy
 *     fabsf(f) < 16777216.0f (a NaN fails); a NaN point or pose is ignored and is no error.  The scan origin plays no part: a beam
 *     that the trace ignores for its origin, or for its length, still counts here.
 *  6. Per pose, slamhip_distance_summary over F(e) of the counted points.  The library sets no threshold. */
typedef struct slamhip_distance_summary {
    int32_t n_counted, n_ignored;      /* sum to n_points */
    int32_t n_zero;                    /* counted points whose end cell is a site (F == 0) */
    int32_t n_capped;                  /* counted points with F == r*r: no site within the radius */
    int64_t sum_d2;                    /* sum of F over the counted points */
} slamhip_distance_summary;            /* 4 int32 + 1 int64: 24 bytes, no padding */
/* The field of a rectangle: x, y, w, h in window-frame cells of the level, any position (the constant outside E); out_d2: h rows of
 * w uint16_t.  The launches, on the operator's stream behind every grid update, shift and upload already enqueued: the lattice
 * search's class map of the level, re-packed on every call (as slamhip_hs_trace packs it), the two launches of the field over E
 * (rows, then columns) and a gather of the rectangle: E itself is never downloaded.  The blocks belong to the hs, are made by the
 * first call and freed by slamhip_hs_destroy; an hs that never asks allocates nothing.  Blocking, with the context's bounded wait;
 * the result comes back through pinned staging that the library owns.  It reads cell values only, so it works with backing off
 * (world = window), with slamhip_hs_set_reference_cache on, and after shifts; it changes nothing of the map or of any search.
 * SLAMHIP_ERR_INVALID, nothing launched: level out of range, world not 0 or 1, site_mask outside [1, 7], radius outside [1, 255],
 * w or h < 1, w * h > 2^24 (32 MB of staging), E over 2^26 cells (1 + 2 bytes per cell: 192 MB; the message gives E's size, and
 * for the world this is known only once the world is planned).  A poisoned context: SLAMHIP_ERR_TIMEOUT.  The limits are design
 * conditions, not measurements. */
int32_t slamhip_hs_distance_field(slamhip_hs *hs, int32_t level, int32_t world, int32_t site_mask, int32_t radius,
                                  int32_t x, int32_t y, int32_t w, int32_t h, uint16_t *out_d2);
/* The end-point distance score of the scan that was set, at B poses (poses: B x 3 floats, window frame).  out_summaries: B records.
 * out_points: NULL, or B x n_points uint16_t, pose-major: F of the point's end cell, 0xFFFF for an ignored point.  The field is
 * built as for slamhip_hs_distance_field on every call, behind a memset of the summaries; then ONE score launch, a point per lane.
 * Everything else as slamhip_hs_distance_field.  SLAMHIP_ERR_INVALID in addition: B outside [1, 65536], out_points given with
 * B * n_points > 2^22.  SLAMHIP_ERR_STATE: no scan. */
int32_t slamhip_hs_distance_score(slamhip_hs *hs, int32_t level, int32_t world, int32_t site_mask, int32_t radius,
                                  const float *poses, int32_t B, slamhip_distance_summary *out_summaries, uint16_t *out_points);

/* The frontier cells of the map and their connected clusters (K10; no reference counterpart): where the known free space of ONE
 * level ends, and which stretches of that boundary hang together -- what an exploring robot chooses its next goal from.  The beam
 * trace's unknown_cells wants candidate viewpoints and the distance field wants goals to check for clearance: the clusters supply
 * both.
 * THE DEFINITION, for level L, world in {0, 1}, min_cells >= 1 and max_clusters in [0, 65536]:
 *  1. Class map.  cls(x, y) and the class map's rectangle M = (mx0, my0, mw, mh) are steps 1 and 4 of slamhip_hs_distance_field: M
 *     is the window, or the world's rectangle R.  Every cell outside M is class 0.
 *  2. Frontier cell.  A cell of M is a frontier cell iff cls = 2 (free) and at least one of its four edge neighbours (x +- 1, y),
 *     (x, y +- 1) has class 0.  A free cell on M's border therefore is a frontier cell, because beyond it the map knows nothing.
 *     Occupied cells and cells outside M are never frontier cells.
 *  3. Cluster.  A cluster is a connected component of frontier cells under 8-connectivity.  Its SEED is its first cell in row-major
 *     order of M; its LABEL is the seed's flat index (seed_y - my0) * mw + (seed_x - mx0).  Labels do not depend on how they are
 *     computed.
 *  4. Run.  A run is a maximal horizontal stretch of frontier cells in one row of M.
 *  5. Per-cluster record, slamhip_frontier_cluster: cells in window-frame cells of the level.  The centroid is sum / n_cells and is
 *     the caller's to form.
 *  6. Kept clusters.  A cluster is KEPT iff n_cells >= min_cells.  The kept clusters are ordered by n_cells descending, equal sizes
 *     by label ascending; the first min(n_kept, max_clusters) are returned.
 *  7. Per-call summary, slamhip_frontier_summary.
 *  8. Labels, on request.  For a caller's rectangle (lx, ly, lw, lh) in window-frame cells at any position: an int32_t per cell,
 *     the label of the cell's cluster, kept or not; -1 where the cell is not a frontier cell, and outside M.
 * The library sets no threshold beyond min_cells and ranks nothing by usefulness. */
#define SLAMHIP_FRONTIER_MAX_CLUSTERS 65536
typedef struct slamhip_frontier_cluster {
    int32_t seed_x, seed_y;            /* the cluster's first cell in row-major order of M */
    int32_t n_cells, n_runs;
    int32_t x_min, y_min, x_max, y_max;    /* the bounding box, inclusive */
    int64_t sum_x, sum_y;              /* over the cluster's cells */
} slamhip_frontier_cluster;            /* 8 int32 + 2 int64: 48 bytes, no padding */
typedef struct slamhip_frontier_summary {
    int32_t mx0, my0, mw, mh;          /* M */
    int32_t n_frontier_cells, n_runs, n_clusters;   /* over ALL components, kept or not */
    int32_t n_kept, n_returned;
    int32_t kept_cells;                /* frontier cells of the kept clusters */
} slamhip_frontier_summary;            /* 10 int32: 40 bytes */
/* The frontier clusters of `level`.  out_summary: one record.  out_clusters: room for max_clusters records (NULL allowed when
 * max_clusters is 0); the first n_returned are written.  out_labels: NULL (lx, ly, lw, lh are then ignored), or lh rows of lw
 * int32_t.
 * The launches, on the operator's stream behind every grid update, shift and upload already enqueued: the lattice search's class
 * map of the level, re-packed on every call (as slamhip_hs_trace packs it), then k10_mark (class words to frontier words, 1 bit per
 * cell; parent and count initialised at every run start), k10_merge (a lock-free union-find over run starts: each run unites itself
 * with the runs of the row above that touch it, the larger root hung under the smaller by an atomic minimum, so the final root of
 * a component is its minimum, the label), k10_count (cells per root), k10_slots (a kept root draws a slot of the record block),
 * k10_stats (one set of atomics per run into its slot), k10_emit (the counters and the drawn slots to pinned memory) and, when
 * labels are asked for, k10_gather.  Every device loop that follows parent links, retries an atomic or scans words carries a cap
 * derived from M's size; an overrun sets a flag and the call returns SLAMHIP_ERR_STATE ("frontier labelling did not converge") --
 * a labelling bug cannot hang the device.  The blocks belong to the hs, are made by the first call and freed by
 * slamhip_hs_destroy; an hs that never asks allocates nothing.  Blocking, with the context's bounded wait: ONE wait; the results
 * come back through pinned staging that the library owns, and the host sorts the at most 65536 records by the rule of step 6.  It
 * reads cell values only, so it works with backing off (world = window), with slamhip_hs_set_reference_cache on, and after shifts;
 * it changes nothing of the map or of any search.  It has no timing class.
 * SLAMHIP_ERR_INVALID, nothing launched: level out of range, world not 0 or 1, min_cells < 1, max_clusters outside [0, 65536],
 * out_clusters NULL with max_clusters > 0, and with labels asked for lw or lh < 1 or lw * lh > 2^24 (64 MB of staging); M over 2^25
 * cells (8 bytes per cell: 256 MB; the message gives M's size, and for the world this is known only once the world is planned).
 * SLAMHIP_ERR_INVALID AFTER the launches: more than 65536 clusters are kept -- the message gives n_kept and says to raise
 * min_cells; out_summary is still filled (n_returned = 0), nothing else is written.  A poisoned context: SLAMHIP_ERR_TIMEOUT.  The
 * limits are design conditions, not measurements. */
int32_t slamhip_hs_frontiers(slamhip_hs *hs, int32_t level, int32_t world, int32_t min_cells, int32_t max_clusters,
                             slamhip_frontier_summary *out_summary, slamhip_frontier_cluster *out_clusters,
                             int32_t lx, int32_t ly, int32_t lw, int32_t lh, int32_t *out_labels);
/* Test hook (no device involved): the frontier clusters of the definition over a caller's class array, M = (0, 0, cw, ch).  cls: ch
 * rows of cw bytes of class bits (only the low two bits are read), packed as the lattice search packs them; the frontier words and
 * the runs by the text the kernels run, the components by a plain sequential union-find.  out_labels: NULL, or the whole cw x ch
 * label array.  Everything else as slamhip_hs_frontiers.  SLAMHIP_ERR_INVALID: cw or ch < 1, cw * ch > 2^25, min_cells < 1,
 * max_clusters outside [0, 65536], out_clusters NULL with max_clusters > 0; more than 65536 kept clusters as there. */
int32_t slamhip_debug_frontiers(const uint8_t *cls, int32_t cw, int32_t ch, int32_t min_cells, int32_t max_clusters,
                                slamhip_frontier_summary *out_summary, slamhip_frontier_cluster *out_clusters, int32_t *out_labels);

/* The cost-to-go field of the map, goal costs and paths (K11; no reference counterpart): which of the frontier clusters an exploring
 * robot can reach, how far the drive to each is while keeping a clearance from the walls, and along which cells.  An exact integer
 * computation: every quantity below is an integer and nothing has a tolerance.
 * THE DEFINITION, for level L, world in {0, 1}, site_mask in {2, 3}, clearance c in [0, 254] and max_cost (0: no cap):
 *  1. Class map.  cls(x, y) and the class map's rectangle M = (mx0, my0, mw, mh) are steps 1 and 4 of slamhip_hs_distance_field: M
 *     is the window, or the world's rectangle R.  Every cell outside M is class 0.
 *  2. Traversable.  A cell of M is traversable iff cls = 2 (free) and, for c >= 1, no site lies within c cells: F(x, y) > c^2, F the
 *     field of slamhip_hs_distance_field with radius c + 1 and site_mask (2: obstacles, 3: obstacles or the unknown).  The test is
 *     exact, because F = min(D2, (c + 1)^2) and c^2 < (c + 1)^2.  With c = 0 no field is built.  Cells outside M are never
 *     traversable.  With site_mask = 3 and c >= 1 EVERY FRONTIER CELL IS UNTRAVERSABLE, because it touches the unknown: this is why
 *     goals are rectangles (step 6) and not cells.
 *  3. Moves.  Eight directions d = 0 .. 7: (+1, 0), (+1, +1), (0, +1), (-1, +1), (-1, 0), (-1, -1), (0, -1), (+1, -1).  The weight
 *     is 5 for even d and 7 for odd d, the 5-7 chamfer metric, an integer stand-in for 5 x the Euclidean length.  A move between two
 *     traversable cells is allowed iff, for a diagonal move, both cells that share an edge with both ends are traversable too (no
 *     corner cutting).  The relation is symmetric.
 *  4. Sources and cost.  S source cells in window-frame cells of the level.  A source that is not traversable, or lies outside M,
 *     is counted in n_sources_blocked and plays no part; the others in n_sources_used, a source given twice twice.  C(x, y) is the
 *     least total weight of a path of allowed moves from any used source, 0 at a source.  With max_cost > 0 a cell whose C exceeds
 *     max_cost is unreached (exact: every prefix of a shortest path is cheaper than the path).  An unreached cell, an untraversable
 *     cell and every cell outside M have C = SLAMHIP_NAV_UNREACHED.  C is the unique solution of the shortest-path equations and
 *     does not depend on how it is computed.
 *  5. Direction.  A reached cell that is no source has dir = the smallest d such that the move to n = (x + dx_d, y + dy_d) is
 *     allowed and C(n) + weight_d == C(x, y); a source has dir = 8; everything else 255.  Following dir from a reached cell ends at
 *     a source after finitely many steps, because C strictly decreases.
 *  6. Goals.  G rectangles {x_min, y_min, x_max, y_max}, inclusive, in window-frame cells at any position, clipped to M.  Per goal,
 *     slamhip_nav_goal_result: cost = the least C over the rectangle's cells, (bx, by) = the cell that has it, the first such cell
 *     in row-major order of M on a tie, n_reached = the reached cells of the rectangle; with no reached cell cost =
 *     SLAMHIP_NAV_UNREACHED and bx = by = 0.  A single cell is the rectangle with min == max.  A frontier cluster's box (x_min ..
 *     y_max of slamhip_frontier_cluster), grown by the caller as it sees fit, asks for "the cheapest reachable cell near that
 *     cluster": THE BOUNDING BOX, NOT THE CLUSTER'S OWN CELLS.
 *  7. Paths, for the first n_paths goals.  The path of a goal with a reached cell is (bx, by) followed by its dir steps down to a
 *     source: cell 0 is (bx, by), the last cell a source.  slamhip_nav_path: n_cells the true length (0: no reached cell), n_written
 *     = min(n_cells, max_path_cells); the first n_written cells go out as int32_t pairs at out_path_cells + 2 * i * max_path_cells.
 *  8. Per call, slamhip_nav_summary.
 *  9. On request, for a caller's rectangle (rx, ry, rw, rh) at any position: C and / or dir of its cells, the values of steps 4 and
 *     5 outside M.
 * The library ranks nothing and sets no threshold. */
#define SLAMHIP_NAV_UNREACHED 0xFFFFFFFFu
typedef struct slamhip_nav_spec {
    int32_t level, world, site_mask, clearance;
    uint32_t max_cost;                 /* 0: no cap */
} slamhip_nav_spec;                    /* 5 words: 20 bytes */
typedef struct slamhip_nav_goal_result {
    uint32_t cost;                     /* SLAMHIP_NAV_UNREACHED: no reached cell in the rectangle */
    int32_t bx, by;                    /* the cheapest reached cell, window-frame cells */
    int32_t n_reached;
} slamhip_nav_goal_result;             /* 16 bytes */
typedef struct slamhip_nav_path {
    int32_t n_cells, n_written;
} slamhip_nav_path;                    /* 8 bytes */
typedef struct slamhip_nav_summary {
    int32_t mx0, my0, mw, mh;          /* M */
    int32_t n_traversable, n_reached;
    int32_t n_sources_used, n_sources_blocked;
    uint32_t max_cost_reached;         /* 0 if nothing is reached */
    int32_t rounds;                    /* relaxation rounds the device ran up to the first that changed no tile's border: an
                                          implementation figure (the test hook returns 0) */
} slamhip_nav_summary;                 /* 10 words: 40 bytes */
/* The field of spec->level.  sources: S pairs (x, y); goals: G rectangles of four int32_t (NULL allowed when G is 0);
 * out_goal_results: G records; out_paths: n_paths records and out_path_cells: n_paths * max_path_cells pairs (both NULL allowed when
 * n_paths is 0); out_cost: NULL, or rh rows of rw uint32_t; out_dir: NULL, or rh rows of rw bytes (rx .. rh are ignored when both
 * are NULL); out_summary: one record.
 * The launches, on the operator's stream behind every grid update, shift and upload already enqueued: the lattice search's class
 * map of the level, re-packed on every call, and for c >= 1 the two launches of slamhip_hs_distance_field's field; k11_trav (class
 * words and field to traversable words, 1 bit per cell); a memset of the cost array (one uint32_t per cell of M) and k11_seed;
 * then k11_relax, ONE LAUNCH PER ROUND, a workgroup per tile of 64 x 64 cells: a tile whose flag is set relaxes its cells in LDS
 * against a one-cell halo until nothing changes, stores what got lower and flags the neighbouring tiles whose halo changed.  No
 * workgroup ever waits for another.  The host enqueues the rounds in batches of 8 (measured against 1 and 32:
 * profiles/r16_hs_nav.json), each batch followed by a one-workgroup launch that stores the round counters to pinned memory, and
 * waits once per batch with the context's bounded wait; it stops when the last round of a batch flagged no tile.  Rounds are capped
 * at n_traversable + 1 (a shortest path is simple, so it crosses tile borders fewer times than it has cells) and a tile's passes in
 * LDS by its cell count + 1; an overrun returns SLAMHIP_ERR_STATE ("navigation field did not converge") -- a relaxation bug cannot
 * hang the device.  Then k11_dirs (dir, n_reached, max_cost_reached), k11_goals (a workgroup per goal), k11_paths (a lane per
 * path), k11_gather (the rectangle) and k11_emit (summary, goal results and path heads to pinned memory).  The blocks belong to the
 * hs, are made by the first call and freed by slamhip_hs_destroy; an hs that never asks allocates nothing.  Blocking.  It reads
 * cell values only, so it works with backing off (world = window), with slamhip_hs_set_reference_cache on, and after shifts; it
 * changes nothing of the map or of any search.  It has no timing class.
 * SLAMHIP_ERR_INVALID, nothing launched, no output written: level out of range, world not 0 or 1, site_mask not 2 or 3, clearance
 * outside [0, 254], S outside [1, 4096], G outside [0, 4096], n_paths outside [0, min(G, 64)], max_path_cells outside [1, 65536],
 * n_paths * max_path_cells > 2^20, a NULL where an array is needed, a goal with x_min > x_max or y_min > y_max, with a rectangle
 * asked for rw or rh < 1 or rw * rh > 2^24; M over 2^25 cells, and for c >= 1 the field's limit on M grown by c + 1 (2^26 cells).
 * A poisoned context: SLAMHIP_ERR_TIMEOUT.  The limits are design conditions, not measurements. */
int32_t slamhip_hs_nav_field(slamhip_hs *hs, const slamhip_nav_spec *spec, const int32_t *sources, int32_t S, const int32_t *goals,
                             int32_t G, slamhip_nav_goal_result *out_goal_results, int32_t n_paths, int32_t max_path_cells,
                             slamhip_nav_path *out_paths, int32_t *out_path_cells, int32_t rx, int32_t ry, int32_t rw, int32_t rh,
                             uint32_t *out_cost, uint8_t *out_dir, slamhip_nav_summary *out_summary);
/* Test hook (no device involved): the field of the definition over a caller's class array, M = (0, 0, cw, ch).  cls: ch rows of cw
 * bytes of class bits (only the low two bits are read), packed as the lattice search packs them; the field for c >= 1 by
 * slamhip_debug_distance_field; traversable words, moves and dirs by the text the kernels run; the costs by a plain sequential
 * Dijkstra with a binary heap, not by the tiled relaxation; rounds = 0.  Everything else as slamhip_hs_nav_field.
 * SLAMHIP_ERR_INVALID: cw or ch < 1, cw * ch > 2^25, and the argument checks of slamhip_hs_nav_field. */
int32_t slamhip_debug_nav_field(const uint8_t *cls, int32_t cw, int32_t ch, int32_t site_mask, int32_t clearance, uint32_t max_cost,
                                const int32_t *sources, int32_t S, const int32_t *goals, int32_t G,
                                slamhip_nav_goal_result *out_goal_results, int32_t n_paths, int32_t max_path_cells,
                                slamhip_nav_path *out_paths, int32_t *out_path_cells, int32_t rx, int32_t ry, int32_t rw, int32_t rh,
                                uint32_t *out_cost, uint8_t *out_dir, slamhip_nav_summary *out_summary);

/* Command rollouts over the cost-to-go field (K12; no reference counterpart): B sequences of velocity commands rolled forward from
 * one pose, each cut where the robot's body first touches something, and what the field says along and at the end of each -- the
 * sampling step of a dynamic-window or sampling-MPC controller, on the map that is already resident.  Cells, counts and costs are
 * integers; the poses are binary32 with EVERY OPERATION ROUNDED ON ITS OWN (no fused multiply-add), so a result is one defined bit
 * pattern and nothing has a tolerance.
 * THE DEFINITION, for a slamhip_nav_spec, S source cells (the goal: cost-to-go 0), a start pose P_0 = (x, y, theta) in the window's
 * frame, a time step dt, P body points (bx_p, by_p) in metres in the robot's frame, B command sequences of n_cmd pairs (v, w) each,
 * and hold, the number of steps each pair is held; T = n_cmd * hold:
 *  1. Field.  M, the traversable cells, C and SLAMHIP_NAV_UNREACHED are steps 1 to 4 of slamhip_hs_nav_field for the spec and the
 *     sources given; the clearance of the spec is how the caller pads the body.  No goals, paths, dir or rectangle are formed.  No
 *     used source is no error: nothing is reached.
 *  2. Poses.  For step i = 0 .. T - 1 the pair is (v, w) = cmd[b][i / hold], (s_i, c_i) = sh_det_sincosf(theta_i), d = v * dt,
 *     x_{i+1} = x_i + d * c_i, y_{i+1} = y_i + d * s_i, theta_{i+1} = theta_i + w * dt.  Each product is rounded before its sum.
 *     There is no angle normalisation.  Explicit Euler is the definition, not an approximation of an arc.  (sh_det_sincosf is
 *     bit-reproducible for |theta| <= 65536; beyond that, and for a theta that is not finite, it is the platform's sinf / cosf.)
 *  3. Cells.  With stm the level's ScaleToMap, the centre cell of pose i is ((int)rintf(x_i * stm), (int)rintf(y_i * stm)): to
 *     nearest, ties to even -- the end-point rule of the grid update, of the trace, of the distance score and of PoseCell.  Body
 *     point p lies at wx = (c_i * bx_p - s_i * by_p) + x_i, wy = (s_i * bx_p + c_i * by_p) + y_i; its cell is (rintf(wx * stm),
 *     rintf(wy * stm)).  A coordinate f = m * stm that fails fabsf(f) < 16777216.0f has no cell; a NaN fails.
 *  4. Free pose.  Pose i is FREE iff its centre has a cell with C != SLAMHIP_NAV_UNREACHED (the cell is then traversable and
 *     connected to a source within max_cost) and every body point has a cell that is traversable.  Cells outside M never are; in
 *     the world variant M is the world's rectangle, as for the field.
 *  5. Per rollout, slamhip_rollout_result.  n_free: the number of leading free poses among P_0 .. P_T, in [0, T + 1]; the rollout is
 *     COMPLETE iff n_free == T + 1.  min_step: the first i < n_free whose centre cell has the least C; min_cost: that C.  end_cost:
 *     C at the centre of pose n_free - 1.  (x, y, theta): pose n_free - 1.  With n_free == 0: min_step = -1, both costs
 *     SLAMHIP_NAV_UNREACHED, the pose P_0.
 *  6. Per call, slamhip_rollout_summary.  nav: the field's summary (max_cost_reached and n_reached counted by a launch of this
 *     call's own).  start_cost: C at P_0's centre, or SLAMHIP_NAV_UNREACHED.  n_complete.  key_end: the minimum over the complete
 *     rollouts of ((uint64_t)end_cost << 32) | b; key_min: the same with min_cost over the rollouts with n_free >= 1; either is
 *     UINT64_MAX if no rollout qualifies.  Equal costs go to the lowest b.
 * The library weighs nothing against anything else and sets no threshold. */
typedef struct slamhip_rollout_result {
    int32_t n_free, min_step;
    uint32_t end_cost, min_cost;
    float x, y, theta;
} slamhip_rollout_result;              /* 7 words: 28 bytes, no padding */
typedef struct slamhip_rollout_summary {
    slamhip_nav_summary nav;           /* 40 bytes */
    uint32_t start_cost;
    int32_t n_complete;
    uint64_t key_end, key_min;         /* at offsets 48 and 56 */
} slamhip_rollout_summary;             /* 64 bytes, no padding */
/* The rollouts on spec->level.  sources: S pairs (x, y), window-frame cells; start_pose: 3 floats; body: P pairs (NULL allowed when P
 * is 0); cmds: B * n_cmd pairs (v, w), rollout b's at cmds + 2 * b * n_cmd; out_results: B records; out_summary: one record.
 * The launches, on the operator's stream behind everything already enqueued: what slamhip_hs_nav_field runs up to the end of its
 * relaxation, by the same internal function (that call's own launches and results are unchanged), with its batch waits; then
 * k12_count (n_reached and max_cost_reached: k11_dirs, which counts them for the field, is not run), ONE k12_rollout launch and a
 * one-workgroup k12_emit, and one bounded wait.  k12_count reads every cell of M (4 bytes each) to fill those two fields.
 * k12_rollout gives each rollout ONE lane: it integrates the state and tests the centre and then the body points of each pose
 * one after the other against the costs and the traversable words in global memory, and goes idle as soon as a pose is not free;
 * the device loop is bounded by T and ends for a wavefront once all its rollouts have.  (A sub-group of lanes per rollout and an
 * LDS copy of the words around the start were built, measured and not adopted: docs/EXPERIMENTS.md.)  The keys are reduced per
 * wavefront and merged by one 64-bit agent-scope atomic minimum per wavefront.  Commands and body points reach the device as the trace's poses do (pinned staging, one copy); the results come
 * back through pinned staging the library owns.  The blocks belong to the hs, are made by the first call and freed by
 * slamhip_hs_destroy; an hs that never asks allocates nothing.  Blocking.  It reads cell values only, so it works with backing off
 * (world = window), with slamhip_hs_set_reference_cache on, and after shifts; it changes nothing of the map or of any search.  It
 * has no timing class.
 * SLAMHIP_ERR_INVALID, nothing launched, no output written: what slamhip_hs_nav_field refuses for spec and S; B outside [1, 65536];
 * n_cmd or hold outside [1, 256]; T > 1024; B * n_cmd > 2^22; P outside [0, 32]; a start pose, dt or body point that is not
 * finite; a NULL where an array is needed.  A command that is not finite is no error: its poses have no cell.  A poisoned context:
 * SLAMHIP_ERR_TIMEOUT.  The limits are design conditions, not measurements: the sizes of the staging blocks (32 MB of commands, 1.8
 * MB of results), a sub-group that fits a wavefront, and a device loop with a small fixed bound. */
int32_t slamhip_hs_rollouts(slamhip_hs *hs, const slamhip_nav_spec *spec, const int32_t *sources, int32_t S, const float start_pose[3],
                            float dt, const float *body, int32_t P, const float *cmds, int32_t B, int32_t n_cmd, int32_t hold,
                            slamhip_rollout_result *out_results, slamhip_rollout_summary *out_summary);
/* Test hook (no device involved): the rollouts of the definition over a caller's class array, M = (0, 0, cw, ch), stm the
 * ScaleToMap (1 / cell length).  The field comes from the function slamhip_debug_nav_field builds its costs with (a sequential
 * Dijkstra), the rollouts from the header text the kernel runs (hs_rollout.h), in a plain loop; nav.rounds = 0.  Everything else as
 * slamhip_hs_rollouts.  SLAMHIP_ERR_INVALID: cw or ch < 1, cw * ch > 2^25, stm not finite or <= 0, and the argument checks of
 * slamhip_hs_rollouts. */
int32_t slamhip_debug_rollouts(const uint8_t *cls, int32_t cw, int32_t ch, int32_t site_mask, int32_t clearance, uint32_t max_cost,
                               const int32_t *sources, int32_t S, float stm, const float start_pose[3], float dt, const float *body,
                               int32_t P, const float *cmds, int32_t B, int32_t n_cmd, int32_t hold,
                               slamhip_rollout_result *out_results, slamhip_rollout_summary *out_summary);

/* One particle-filter localisation step on the distance field (K13; no reference counterpart): Monte-Carlo localisation on the
 * resident map -- a set of N pose hypotheses owned by the hs and kept in device memory is moved by odometry with noise, weighed by
 * the scan against K9's field, and resampled, without drawing into the map and without the particles crossing the bus.  Every
 * result is exact: integers, or binary32 with EVERY OPERATION ROUNDED ON ITS OWN (no fused multiply-add), so each output is one
 * defined bit pattern and nothing has a tolerance.
 * THE DEFINITION, for a slamhip_mcl_spec, r = radius, stm the level's ScaleToMap, the n points of the scan that was set, particles
 * (x_i, y_i, theta_i) in the WINDOW's frame with accumulated costs acc_i (uint64), i = 0 .. N - 1:
 *  1. Noise.  B_j = Philox4x32-10(counter = (i, j, stream lo, stream hi), key = (seed lo, seed hi)) for j = 0, 1.  The eight words,
 *     B_0's first, give sixteen 16-bit halves h_0 .. h_15: word 0's low half, word 0's high half, word 1's low half, and so on.
 *     z_m = (float)((h_4m + h_4m+1 + h_4m+2 + h_4m+3) - 131070) * ZS for m = 0, 1, 2, ZS = 0x1.bb67aep-16f, the binary32 nearest
 *     to sqrt(3 / (2^32 - 1)).  z is a four-term Irwin-Hall variate: mean 0, variance 1, tails cut at about 3.46 sigma.  It is not
 *     Box-Muller because logf is not bit-reproducible between host and device.
 *  2. Predict.  ex = dx + sx * z_0, ey = dy + sy * z_1, eth = dth + sth * z_2 (each product rounded before its sum), (s, c) =
 *     sh_det_sincosf(theta_i), x' = (x_i + fox) + (c * ex - s * ey), y' = (y_i + foy) + (s * ex + c * ey), theta' = theta_i + eth.
 *     No angle normalisation.  (sh_det_sincosf is bit-reproducible for |theta| <= 65536, the bound K12 states.)
 *  3. Cost.  cost_i = sum_d2 + r * r * n_ignored of the slamhip_distance_summary that steps 5 and 6 of slamhip_hs_distance_field
 *     define at pose (x', y', theta') for spec's level, world, site_mask and radius.  An ignored point costs as much as a point
 *     with no site within the radius, so a particle with no usable end cell is the WORST particle, not the best.
 *  4. Accumulate.  a_i = acc_i + cost_i; acc'_i = a_i - min_j a_j: bounded, and 0 for the best particle.
 *  5. Weight.  d = min(acc'_i, 2^32 - 1), e = (d * beta) >> 16 in uint64, k = e >> 6, f = e & 63, w_i = k >= 32 ? 0 : T[f] >> k with
 *     T[f] = min(2^32 - 1, floor(2^((2048 - f) / 64))) (slamhip_debug_mcl_table): beta counts, in Q16, the 1/64 halvings of the
 *     weight per unit of cost.  W = sum w_i >= 2^32 - 1.
 *  6. Summary, slamhip_mcl_summary, all exact integer sums.  h_i = w_i >> 20; A = sum h_i, Q = sum h_i^2: the effective sample
 *     size is A^2 / Q, the caller's to form.  key_best = min over i of (a_i << 16 | i) (a_i < 2^48 is the caller's to keep: with
 *     n_eff_min = 0 for ever the costs add up without bound).  sum_hx = sum h_i * (int64)rintf(x' * 1024.0f), sum_hy likewise;
 *     sum_hc = sum h_i * (int)rintf(c' * 16384.0f), sum_hs likewise, (s', c') = sh_det_sincosf(theta'); only particles whose two
 *     scaled coordinates satisfy fabsf(.) < 2147483648.0f and whose c', s' are finite contribute to the four, the others are
 *     counted in n_unplaced.  cost_min, cost_max over cost_i.  With n_unplaced == 0 the weighted-mean pose is (sum_hx / A / 1024,
 *     sum_hy / A / 1024, atan2(sum_hs, sum_hc)).  With n_unplaced > 0 the divisor A still holds the h of the unplaced particles,
 *     which the two position sums lack: x and y are then pulled towards 0 by the share of A those particles carry (none once their
 *     weight is below 2^20; an unplaced particle lies 2^21 m out and costs like a particle with no site in reach).  The summary
 *     has no sum of h over the placed particles alone; a caller who needs the exact mean then forms it from slamhip_hs_mcl_get.
 *  7. Resample iff A * A < (uint64)n_eff_min * Q (0: never; N + 1: always, because Q <= A * A <= N * Q).  If not: the particles
 *     are the predicted ones, acc = acc', the ancestors the identity, n_distinct = N.  If so, systematic resampling: C_i the
 *     inclusive uint64 prefix sum of w in index order, rr = word 0 of Philox4x32-10((0, 2, stream lo, stream hi), key),
 *     u = ((W >> 16) * rr) >> 16, T_k = k * W + u, anc_k = the least i with N * C_i > T_k (N * W < 2^64); new particle k is
 *     predicted particle anc_k, every acc becomes 0, n_distinct is the number of distinct ancestors. */
typedef struct slamhip_mcl_spec {
    int32_t level, world, site_mask, radius;   /* as slamhip_hs_distance_score */
    float delta[3];                    /* odometry increment (dx, dy, dth) in the ROBOT frame since the last step */
    float sigma[3];                    /* noise scales (sx, sy, sth); the caller scales them by the motion */
    float frame_offset[2];             /* metres, added to every particle first: the window's movement since the last step, else 0 */
    uint32_t beta;                     /* Q16 count of 1/64 halvings of weight per unit of cost; not 0 */
    int32_t n_eff_min;                 /* resample iff the effective sample size is below it: 0 never, N + 1 always */
    uint64_t seed, stream;             /* Philox key and stream; the caller advances stream per step */
} slamhip_mcl_spec;                    /* 14 words + 2 uint64 at offsets 56 and 64: 72 bytes, no padding */
typedef struct slamhip_mcl_summary {
    uint64_t W, A, Q, key_best;
    int64_t sum_hx, sum_hy, sum_hc, sum_hs;
    uint64_t cost_min, cost_max;
    int32_t resampled, n_distinct, n_unplaced, n_particles;
} slamhip_mcl_summary;                 /* 10 x 8 + 4 x 4: 96 bytes, no padding */
/* The particle set of the hs: N particles (poses: N x 3 floats, window frame), N in [1, 65536]; every acc becomes 0, the ancestors
 * the identity; it replaces any previous set.  The blocks (two particle buffers, acc, a, w, C, ancestors: 3.7 MB, and 1.5 MB of
 * pinned staging) belong to the hs, are made by the first call and freed by slamhip_hs_destroy.  Blocking.  SLAMHIP_ERR_INVALID:
 * N out of range, a value that is not finite.  A poisoned context: SLAMHIP_ERR_TIMEOUT. */
int32_t slamhip_hs_mcl_set(slamhip_hs *hs, const float *poses, int32_t N);
/* One step.  The launches, on the operator's stream behind everything already enqueued: the field of slamhip_hs_distance_score by
 * the same internal functions (the class map's pack, k9_rows, k9_cols -- REBUILT ON EVERY STEP, as K9 does, because the map may have
 * changed: at 2048^2 cells that is most of a step's time, and there is no cache); k13_score -- the scan staged in LDS once per
 * workgroup, one wavefront per particle at a time, steps 1 and 2 computed uniformly across the wavefront, lanes striding the points
 * and gathering the uint16 field, a wave reduction, 64-bit agent-scope atomic minima for min a and cost_min; k13_weigh -- a lane per
 * particle, w, acc', the sums of step 6 reduced per wavefront, one atomic per wavefront per sum; k13_scan -- ONE workgroup, the
 * inclusive uint64 scan of w in chunks of 4096, skipped when the decision read from device memory is not to resample; k13_resample
 * -- the decision read from device memory, a binary search per lane over C, the OTHER particle buffer written (the two are used in
 * turn), the distinct ancestors counted by anc_k != anc_k-1, and the last workgroup to finish stores the summary to pinned memory.
 * No host round trip inside the step; blocking, ONE bounded wait.  It changes nothing of the map or of any other call.
 * LDS: the scan's points, 8 bytes each, must fit a 64 KB allocation beside the reductions' words: n_points <= 7680 is a design
 * condition.  SLAMHIP_ERR_INVALID, nothing launched, no output written: level, world, site_mask, radius as
 * slamhip_hs_distance_score; a float of the spec that is not finite; beta == 0; n_eff_min outside [0, N + 1]; n_points > 7680; E over
 * 2^26 cells.  SLAMHIP_ERR_STATE: no particle set, or no scan.  A poisoned context: SLAMHIP_ERR_TIMEOUT.  A step that fails once its
 * first kernel is enqueued (a launch error, the wait) leaves NO particle set -- the particles are predicted in place, so they are then
 * neither the old set nor the new one: the next step and slamhip_hs_mcl_get answer SLAMHIP_ERR_STATE until slamhip_hs_mcl_set. */
int32_t slamhip_hs_mcl_step(slamhip_hs *hs, const slamhip_mcl_spec *spec, slamhip_mcl_summary *out);
/* The particles (N x 3 floats), acc (N uint64) and the ancestors of the last step (N int32; the identity before any step); any of
 * the three may be NULL.  N must be the set's.  Blocking.  SLAMHIP_ERR_STATE: no particle set. */
int32_t slamhip_hs_mcl_get(slamhip_hs *hs, float *poses, uint64_t *acc, int32_t *ancestors, int32_t N);
/* Test hook (no device involved): one step of the definition over a caller's class array, M = (0, 0, cw, ch), stm the ScaleToMap;
 * spec->level must be 0.  The field comes from slamhip_debug_distance_field, the step from the header text the kernels run
 * (hs_mcl.h), in plain loops.  points: n_points pairs; particles_in: N x 3; acc_in: N uint64, or NULL for zeros; the outputs as
 * slamhip_hs_mcl_get's, none NULL.  SLAMHIP_ERR_INVALID, no output written: cw or ch < 1, stm not finite or <= 0, n_points outside
 * [1, 7680], N outside [1, 65536], a particle that is not finite, and the spec's refusals of slamhip_hs_mcl_step. */
int32_t slamhip_debug_mcl_step(const uint8_t *cls, int32_t cw, int32_t ch, float stm, const float *points, int32_t n_points,
                               const float *particles_in, const uint64_t *acc_in, int32_t N, const slamhip_mcl_spec *spec,
                               float *particles_out, uint64_t *acc_out, int32_t *ancestors_out, slamhip_mcl_summary *summary);
/* The weight table T of step 5. */
int32_t slamhip_debug_mcl_table(uint32_t out[64]);

/* K14 -- merge a second map into the window under a rigid transform (new; no reference counterpart: a map another robot made, a map
 * an earlier session saved in another frame, or what this session mapped before slamhip_hs_relocalise_world told it where it is).
 * A SOURCE map is kept in device memory (slamhip_hs_merge_set_source); candidate alignments are RATED without touching either map
 * (slamhip_hs_merge_score); the source's evidence is FUSED into one level at the chosen alignment (slamhip_hs_merge_apply), after
 * which the matcher, the grid update and K7 - K13 go on working on the result.
 *
 * The definition, shared by score and apply, for level L with ScaleToMap stm and window wd x hd, a source array of w x h cells whose
 * first is source-frame cell (ax, ay), and a pose T = (tx, ty, theta): the origin and heading of the SOURCE frame in the destination
 * WINDOW's frame, in metres and radians as every hs pose is.  Every binary32 operation is rounded on its own, no fused multiply-add.
 *  1. txc = tx * stm, tyc = ty * stm; (c, s) = the cosine and sine the beam trace's Rotation(theta) holds (IEEERemainder by 2 pi, the
 *     four snapped angles of Matrix3x2.CreateRotation, else the deterministic sine and cosine).
 *  2. For destination cell (x, y): dxf = (float)x - txc, dyf = (float)y - tyc; u = (c * dxf) + (s * dyf), v = (c * dyf) - (s * dxf).
 *     The cell is SOURCED iff |u| < 16777216 and |v| < 16777216 (a NaN fails) and (su, sv) = ((int)rintf(u) - ax, (int)rintf(v) - ay)
 *     lies in [0, w) x [0, h); rintf rounds half to even.  Nearest neighbour, one source cell per destination cell: every destination
 *     cell has one writer and the result has no holes.  A pose that is not finite is no error: nothing is sourced.
 *  3. The report counts the destination cells: joint[3 * cd + cs] for a sourced cell, by the class of the destination cell BEFORE the
 *     call (cd) and of its source cell (cs) -- the trace's classes: 1 if Value > 0.0f, 2 if Value < 0.0f, else 0, so NaN is 0 --
 *     and n_unsourced for the others.  The library sets no threshold and forms no score.
 *  4. Apply, for a sourced cell with destination Value d and source Value sv:
 *       rule 0 ADD      if cs != 0 and d is not NaN: t = d + sv; if t > value_limit, t = value_limit; if t < -value_limit,
 *                       t = -value_limit; the cell counts in n_clamped when either cut applied.  A NaN d stays as it is.  A sum that
 *                       is NaN (an infinity met its opposite) is the quiet NaN 0x7FC00000, which no cut applies to.
 *       rule 1 FILL     if cd == 0 and cs != 0: t = sv.
 *       rule 2 REPLACE  if cs != 0: t = sv.
 *     Otherwise the cell is left alone.  UpdateIndex never changes.  The Value is written only where its bits change; such cells
 *     count in n_changed and get their probability written beside the Value, by the function every writer of the cells uses.  Tiles
 *     of the backing store and cells outside the window are not touched (the caller scrolls and merges again); the reference cache's
 *     epoch and the level's current update index are unchanged. */
typedef struct slamhip_merge_report {
    int64_t joint[9];                  /* joint[3 * cd + cs]: destination cells whose source cell lies in the source array, by the class of
                                          the destination cell BEFORE the call (cd) and of the source cell (cs): 0 neither, 1 occupied, 2 free */
    int64_t n_unsourced;               /* destination cells with no source cell; joint[] and this sum to w * h of the level */
    int64_t n_changed;                 /* apply only: cells whose Value bits changed */
    int64_t n_clamped;                 /* apply only, rule ADD: cells whose sum was cut to +-value_limit */
} slamhip_merge_report;                /* 12 int64_t, 96 bytes, no padding */
/* The source: cells[w * h], row-major, the first element source-frame cell (ax, ay) of a grid with the cell length of `level` --
 * what slamhip_hs_cells_download or slamhip_hs_world_cells_download of any hs gives.  The cells pass through staging the library
 * owns; ONE launch (k14_pack_source) leaves their Values in device memory as float[w * h] and their classes at 2 bits per cell.  The
 * source's update indices are not kept: they mean nothing in another map's epochs.  The source stays until the next
 * slamhip_hs_merge_set_source, slamhip_hs_merge_clear_source, slamhip_hs_reset or slamhip_hs_destroy; grid updates, matches and
 * shifts leave it.  The blocks (16 B of device and 8 B of pinned memory per source cell) belong to the hs, are made by the first call
 * and freed by slamhip_hs_destroy; an hs that never calls it allocates and launches nothing.  Blocking.  SLAMHIP_ERR_INVALID, nothing
 * launched, the previous source kept: level out of range; w or h below 1; w * h > 2^26; |ax| or |ay| above 2^30.  A poisoned context:
 * SLAMHIP_ERR_TIMEOUT. */
int32_t slamhip_hs_merge_set_source(slamhip_hs *hs, int32_t level, int32_t ax, int32_t ay, int32_t w, int32_t h,
                                    const slamhip_cell *cells);
/* B reports (poses: B x 3 floats, B in [1, 4096]) for the source's level, n_changed = n_clamped = 0; nothing is changed.  On the
 * operator's stream behind everything already enqueued: K7's class map of the destination level (the window's), a memset of the
 * reports, then ONE launch, k14_score -- the grid is (tiles of 64 x 16 destination cells, chunks of 16 poses); a workgroup holds its
 * tile's destination classes in registers and loops over its poses; per pose the tile box (step 2's operations on intervals) lets an
 * unsourced tile leave at once, otherwise every lane gathers its source cells' class bits from the packed source, the ten counts come
 * from wave ballots, and at the end ONE integer atomic add per workgroup, pose and non-zero counter.  Integers: every order gives the
 * same bits.  Blocking, the context's bounded wait; the reports come back through pinned staging.  SLAMHIP_ERR_INVALID: B out of
 * range.  SLAMHIP_ERR_STATE: no source.  A poisoned context: SLAMHIP_ERR_TIMEOUT.  Nothing is launched on any refusal. */
int32_t slamhip_hs_merge_score(slamhip_hs *hs, const float *poses, int32_t B, slamhip_merge_report *out_reports);
/* The source fused into its level at one pose, by ONE launch over the window (k14_apply: a workgroup per tile of 64 x 32 destination
 * cells; a tile whose box of source cells is empty leaves at once, the others gather their source Values from global memory,
 * bounds-checked -- staging the box in LDS was built and measured and does not win); the report's joint and n_unsourced equal what slamhip_hs_merge_score gives for the same pose just before.  Blocking.
 * SLAMHIP_ERR_INVALID: rule outside 0 .. 2; value_limit not finite or not above 0 (checked also for rules 1 and 2, which ignore it);
 * the reference's cache is on (slamhip_hs_set_reference_cache) -- its literal stale entries have no meaning under an operation the
 * reference lacks, as for slamhip_hs_shift.  SLAMHIP_ERR_STATE: no source.  A poisoned context: SLAMHIP_ERR_TIMEOUT.  Nothing is
 * launched on any refusal. */
int32_t slamhip_hs_merge_apply(slamhip_hs *hs, const float pose[3], int32_t rule, float value_limit,
                               slamhip_merge_report *out_report);
/* No source from here on (the blocks stay).  Never fails for an hs without one. */
int32_t slamhip_hs_merge_clear_source(slamhip_hs *hs);
/* Test hook (no device involved): steps 1 - 4 over a destination array dst[dw * dh] and a source array src[sw * sh] whose first cell
 * is source-frame cell (ax, ay), from the header text the kernels run (hs_merge.h), in plain loops.  out_cells: dw * dh merged cells;
 * out_report as slamhip_hs_merge_apply's.  SLAMHIP_ERR_INVALID: a size below 1 or above 2^26 cells, |ax| or |ay| above 2^30, and
 * the rule's and the limit's refusals of slamhip_hs_merge_apply. */
int32_t slamhip_debug_merge(const slamhip_cell *dst, int32_t dw, int32_t dh, const slamhip_cell *src, int32_t ax, int32_t ay,
                            int32_t sw, int32_t sh, const float pose[3], float stm, int32_t rule, float value_limit,
                            slamhip_cell *out_cells, slamhip_merge_report *out_report);
/* Test hook: the kernels' tile box of destination tile [x0, x1] x [y0, y1] (0 <= x0 <= x1 < 32768, likewise y) -- out_box = {u0, v0,
 * u1, v1}, inclusive, in cells of the source ARRAY: every sourced cell of the tile has its source cell in it; *out_any = 0: the box
 * is empty, no cell of the tile is sourced. */
int32_t slamhip_debug_merge_box(const float pose[3], float stm, int32_t ax, int32_t ay, int32_t sw, int32_t sh, int32_t x0, int32_t y0,
                                int32_t x1, int32_t y1, int32_t out_box[4], int32_t *out_any);

/* The view gain (K15; no reference counterpart): the DISTINCT cells of ONE level that the scan's beams would see from a pose, by
 * class and against a layer of cells already covered, for many poses at once, and the greedy choice of the few poses of a list
 * that together reveal the most -- what next-best-view exploration and a coverage run ask.  slamhip_trace_summary.unknown_cells
 * cannot answer it: that figure counts a cell once per beam that crosses it.
 * THE DEFINITION, for level L of the WINDOW only (there is no world variant), the scan and scan origin as slamhip_hs_set_scan took
 * them, a pose P in the window's frame, and `reach` in [1, 4096] cells:
 *  1. Beam.  Beam i is hs_trace_line_of under hs_trace_transform(stm, P): steps 1 - 2 of slamhip_trace_beam, unchanged -- ignored
 *     (da = -1), same (da = 0), or walked.  Its cells are step 3 there (hs_trace_walk_begin / _next).  Classes are the lattice
 *     search's: 1 occupied, 2 free, 0 neither.
 *  2. What a beam sees.  A walked beam SEES the cells of steps a = 0 .. stop, stop = min(first if first >= 0 else da, reach): the
 *     occupied cell that stops it is seen; the end cell is seen if it is reached.  Step a lies at Chebyshev distance exactly a from
 *     b, so `reach` is the sensor's range limit in cells and every seen cell lies in the square of side 2 reach + 1 around b.  A
 *     same beam sees b.  An ignored beam sees nothing.  A cell outside [0, w) x [0, h) is never seen, and the walk goes on through
 *     it (class 0), as in the trace.  A beam is CUT if it is walked, has da > reach, and has no occupied cell at a step <= reach.
 *  3. V(P) is the set of cells seen by any beam.
 *  4. The covered layer C is a set of window cells of ONE level that the slamhip_hs holds; it is empty until set or committed to.
 *     Its bitmap layout, in and out: row-major, wpr = (w + 31) / 32 uint32_t per row, cell x is bit x & 31 of word x >> 5.
 *     Padding bits are ignored on input and zero on output.
 *  5. Per pose, slamhip_view_summary.  C is the layer AS IT WAS BEFORE THE CALL for every pose of the call.  A pose that is not
 *     finite is no error: all its beams are ignored and every other field is 0.
 *  6. Greedy choice: rounds j = 1 .. k over the poses not yet chosen.  g(p) = n_new (mode 0) or n_new_unknown (mode 1), counted
 *     against the CURRENT C.  The best is the largest g, ties to the lowest pose index.  The choice stops when g(best) < min_gain.
 *     Otherwise the best is recorded with its gain, and ALL of V(best) joins C, in either mode. */
typedef struct slamhip_view_summary {
    int32_t n_walked, n_same, n_ignored;   /* the beams by status: they sum to n_points */
    int32_t n_cut;                         /* the cut beams */
    int32_t n_seen;                        /* |V| */
    int32_t n_unknown, n_free, n_occupied; /* V by class: they sum to n_seen */
    int32_t n_new;                         /* |V \ C| */
    int32_t n_new_unknown;                 /* the class-0 cells of V \ C */
} slamhip_view_summary;   /* ten int32_t, 40 bytes, no padding */
/* The covered layer.  _set_covered makes the layer for `level` from `bits` (step 4's layout; NULL: empty) and stamps it with the
 * window origin (slamhip_hs_origin); a layer of another level is replaced.  _get_covered downloads it (all zero while there is
 * none).  _view_clear frees every block of the view gain, the layer too; slamhip_hs_destroy frees them as well, slamhip_hs_reset
 * leaves the layer alone, and an hs that never asks allocates nothing.  SLAMHIP_ERR_INVALID: level out of range.
 * SLAMHIP_ERR_STATE (_get_covered): the layer belongs to another level, or the window has moved since it was made. */
int32_t slamhip_hs_view_set_covered(slamhip_hs *hs, int32_t level, const uint32_t *bits);
int32_t slamhip_hs_view_get_covered(slamhip_hs *hs, int32_t level, uint32_t *bits);
int32_t slamhip_hs_view_clear(slamhip_hs *hs);
/* Step 5 at B poses (poses: B x 3 floats, window frame; B in [1, 4096]); out_summaries: B records.  commit = -1 changes nothing;
 * -2 adds every pose's V to C after counting; 0 <= commit < B adds that pose's V.  A commit makes the layer if there is none.
 * The launches, on the operator's stream: the lattice search's class map of the level, re-packed on every call, ONE launch of
 * k15_view (a workgroup per pose: the pose's seen bitmap in LDS while the box of any pose of the call fits 8704 words -- reach 255
 * does -- else in a scratch block, zeroed by a memset), and with a commit one launch that ORs the bitmaps into C.  Blocking, with
 * the context's bounded wait; the results come back through pinned staging that the library owns.  It reads cell values only,
 * so it works with backing off, with slamhip_hs_set_reference_cache on, and after shifts (once the layer is set again); it
 * changes nothing of the map or of any search.
 * SLAMHIP_ERR_INVALID, nothing launched: level, reach, B or commit out of range; the call needs scratch (a commit, or bitmaps
 * that do not fit LDS) and B x rows x words_per_row exceeds 2^25 words (128 MB), rows = min(2 reach + 1, h), words_per_row =
 * min((2 reach + 63) / 32, (w + 31) / 32).  SLAMHIP_ERR_STATE: no scan; the layer belongs to another level; the window origin
 * differs from the layer's stamp (set the layer again; slamhip_hs_shift itself is not changed).  A poisoned context:
 * SLAMHIP_ERR_TIMEOUT. */
int32_t slamhip_hs_view_gain(slamhip_hs *hs, int32_t level, int32_t reach, const float *poses, int32_t B, int32_t commit,
                             slamhip_view_summary *out_summaries);
/* Step 6 over B poses: k in [1, 64], mode 0 or 1, min_gain >= 1.  out_order and out_gain have k entries: the chosen pose indices in
 * the order of choice and their gains; entries past *out_n are -1 and 0.  The chosen views are committed to C (the layer is made if
 * there is none).  The launches: the class map and k15_view as above (the bitmaps always go to the scratch block), then k15_gain
 * (a workgroup per pose not yet chosen) and k15_pick (one workgroup) k times back to back -- the winner's index never leaves the
 * device between rounds -- and ONE host wait at the end.  Errors as slamhip_hs_view_gain, and SLAMHIP_ERR_INVALID for k, mode or
 * min_gain out of range. */
int32_t slamhip_hs_view_select(slamhip_hs *hs, int32_t level, int32_t reach, int32_t mode, int32_t min_gain, const float *poses,
                               int32_t B, int32_t k, int32_t *out_order, int32_t *out_gain, int32_t *out_n);
/* Test hook (no device involved): steps 1 - 5 for one pose over values[w * h] (row-major cell Values), from the header text the
 * kernels run (hs_view.h), in plain loops.  covered: step 4's bitmap, or NULL (empty).  out_bits: V as a bitmap of step 4's
 * layout; out_summary as slamhip_hs_view_gain's.  SLAMHIP_ERR_INVALID: a size below 1 or above 2^26 cells, reach outside
 * [1, 4096]. */
int32_t slamhip_debug_view(const float *values, int32_t w, int32_t h, float stm, const float pose[3], const float origin[2],
                           const float *xy, int32_t n_points, int32_t reach, const uint32_t *covered, uint32_t *out_bits,
                           slamhip_view_summary *out_summary);

/* The nearest site of every cell and the scan-to-map pairs (K16; no reference counterpart): WHERE the nearest wall cell lies, not
 * only how far -- the feature transform of the map.  It gives point-to-map correspondences from up to r cells away (a closed-form
 * 2-D alignment step from one summary), a gradient of the distance field, and a direction away from the wall.
 * THE DEFINITION, for level L, world in {0, 1}, site_mask in [1, 7] and radius r in [1, 255].  Classes, sites, M and E, and the end
 * cell of a scan point are steps 1, 2, 4 and 5 of slamhip_hs_distance_field, unchanged; F is its field.
 *  1. Nearest site.  For a cell (x, y), N(x, y) is the site (sx, sy) with (sx - x)^2 + (sy - y)^2 < r^2 that minimises the key
 *     (D2, sy, sx) lexicographically: the squared distance first, then the smaller row, then the smaller column.  The result is the
 *     offset pair (dx, dy) = (sx - x, sy - y) as two int16_t, |dx|, |dy| <= 254.  If no site has D2 < r^2 the result is NONE =
 *     (INT16_MAX, INT16_MAX).  By construction dx^2 + dy^2 == F(x, y) wherever F < r^2, and NONE holds exactly where F == r^2.
 *     Outside E every cell is class 0: the result there is (0, 0) when site_mask & 1 and NONE otherwise, the distance field's
 *     constant argument.  With bit 0 set the cells outside M are sites and may be the nearest one; the key still decides: a non-site
 *     cell at M's corner (0, 0) with nothing nearer gets (0, -1), not (-1, 0).
 *  2. Separable form, exact.  Within one row the site nearest to x minimises D2 for that row, a left/right tie going to the left
 *     (the smaller sx); across rows equal D2 goes to the smaller sy.  So a row pass that keeps a SIGNED offset o with |o| < r and
 *     ties to the left, and a column pass that takes the minimum of (o^2 + dy^2, y + dy) over |dy| < r, equal the lexicographic
 *     arg-min over all sites.
 *  3. Pairs.  For the scan that was set and a pose P, every counted point (step 5 of slamhip_hs_distance_field; the scan origin
 *     plays no part) has its end cell e.  The point is MATCHED iff N(e) is not NONE, and then q = e + N(e).  The per-point record
 *     is (dx, dy): (INT16_MIN, INT16_MIN) for an ignored point, NONE for a counted point that is not matched.
 *  4. Per pose, slamhip_pair_summary.  Every sum runs over the MATCHED points only; e and q are window-frame cells of the level.
 *     The sums are accumulated modulo 2^64; nothing wraps for |coordinate| < 2^24 + 255 and at most 16 384 points (a product is
 *     below 2^49, 2^14 of them below 2^63).  Integer sums are order-free: any reduction tree and any atomic order give the same
 *     bits.  The library sets no threshold and runs no iteration: the caller's loop does. */
#define SLAMHIP_NEAREST_NONE 32767         /* INT16_MAX, both components */
#define SLAMHIP_NEAREST_IGNORED (-32768)   /* INT16_MIN, both components: the per-point record of an ignored point */
typedef struct slamhip_pair_summary {
    int32_t n_counted, n_ignored;      /* sum to n_points */
    int32_t n_matched;                 /* counted points with a site within the radius of their end cell */
    int32_t n_zero;                    /* matched points with offset (0, 0): the end cell is a site */
    int64_t sum_d2;                    /* sum of dx^2 + dy^2 over the matched points */
    int64_t sum_ex, sum_ey, sum_qx, sum_qy;
    int64_t sum_exqx, sum_eyqy, sum_exqy, sum_eyqx;
} slamhip_pair_summary;                /* 4 int32 + 9 int64: 88 bytes, no padding */
/* N of a rectangle: x, y, w, h in window-frame cells of the level, any position (the constant outside E); out_dxdy: h rows of w
 * pairs (dx, dy) of int16_t.  The launches, on the operator's stream behind every grid update, shift and upload already enqueued:
 * the lattice search's class map of the level, re-packed on every call (as slamhip_hs_trace packs it), the two launches of the
 * field over E (rows: one signed int16_t offset per cell; columns: the pair) and a gather of the rectangle: E itself is never
 * downloaded.  The blocks belong to the hs, are made by the first call and freed by slamhip_hs_destroy; an hs that never asks
 * allocates nothing, and the distance field's own blocks are not used.  Blocking, with the context's bounded wait; the result comes
 * back through pinned staging that the library owns.  It reads cell values only, so it works with backing off (world = window),
 * with slamhip_hs_set_reference_cache on, and after shifts; it changes nothing of the map or of any search.
 * SLAMHIP_ERR_INVALID, nothing launched: level out of range, world not 0 or 1, site_mask outside [1, 7], radius outside [1, 255],
 * w or h < 1, w * h > 2^24 (64 MB of staging), E over 2^26 cells (2 + 4 bytes per cell: 384 MB; the message gives E's size, and
 * for the world this is known only once the world is planned).  A poisoned context: SLAMHIP_ERR_TIMEOUT.  The limits are design
 * conditions, not measurements. */
int32_t slamhip_hs_nearest_field(slamhip_hs *hs, int32_t level, int32_t world, int32_t site_mask, int32_t radius,
                                 int32_t x, int32_t y, int32_t w, int32_t h, int16_t *out_dxdy);
/* The pairs of the scan that was set, at B poses (poses: B x 3 floats, window frame).  out_summaries: B records.  out_pairs: NULL,
 * or B x n_points pairs of int16_t, pose-major: step 3's record.  The field is built as for slamhip_hs_nearest_field on every call,
 * behind a memset of the summaries; then ONE launch, a point per lane, whose workgroups add their partial sums into the summaries
 * with 64-bit atomic adds.  Everything else as slamhip_hs_nearest_field.  SLAMHIP_ERR_INVALID in addition: B outside [1, 65536],
 * out_pairs given with B * n_points > 2^22.  SLAMHIP_ERR_STATE: no scan. */
int32_t slamhip_hs_nearest_pairs(slamhip_hs *hs, int32_t level, int32_t world, int32_t site_mask, int32_t radius,
                                 const float *poses, int32_t B, slamhip_pair_summary *out_summaries, int16_t *out_pairs);
/* Test hook (no device involved): N of the definition over cls[cw * ch] (row-major class bits, class 0 outside the array), for the
 * rectangle x, y, w, h in the array's cells, from the header text the kernels run (hs_nearest.h).  out_dxdy: h rows of w pairs.
 * SLAMHIP_ERR_INVALID as slamhip_debug_distance_field. */
int32_t slamhip_debug_nearest_field(const uint8_t *cls, int32_t cw, int32_t ch, int32_t site_mask, int32_t radius,
                                    int32_t x, int32_t y, int32_t w, int32_t h, int16_t *out_dxdy);

/* The Hough transform of a map and what a scan-free alignment of two maps takes from it (K17; no reference counterpart).  K14 fuses a
 * second map at a transform the caller has; K7 and K13 find one only from a scan taken at a known pose in the other map.  Two saved
 * worlds, or maps of two robots that never exchanged a scan, are aligned by the Hough spectrum (Carpin, "Fast and accurate map merging
 * for multi-robot systems", 2008): the circular correlation of the two maps' spectra gives the relative rotation, the correlation of
 * matching Hough rows over rho the translation along that row's direction; slamhip_hs_merge_score then rates the hypotheses.
 * THE DEFINITION.  The map M is a class map of w x h cells whose first cell is frame cell (x0, y0).  Two slots: slot 0 (destination)
 * holds level L of the window (world = 0) or of the world rectangle (world = 1), exactly as the lattice search plans it; slot 1
 * (source) holds the merge source of the hs: its packed classes, w x h, (x0, y0) = (ax, ay).  The sites: site_mask in [1, 7] and the
 * distance field's rule for which cell is a site, unchanged -- but cells outside M do not exist here: there is no grown E, and bit 0
 * of the mask makes only M's own class-0 cells sites.  The angle count T is a multiple of 4 in [4, 1024]; the bin width is b = 2^q
 * cells, q in [0, 3].
 *  1. Table.  C[0] = 16384, S[0] = 0; C[T/2] = 0, S[T/2] = 16384; for 0 < k < T/2: C[k] = (int)rint(16384 * cos(k pi / T)) and
 *     S[k] = (int)rint(16384 * sin(k pi / T)), formed in binary64 on the HOST with pi as M_PI and k pi / T as ((double)k * M_PI) /
 *     (double)T; for T/2 < k < T: C[k] = -C[T - k], S[k] = S[T - k].  The device never forms a sine: the table is an argument of
 *     the launches.
 *  2. Vote.  D = w + h, N = ((2 D) >> q) + 1.  A site at array cell (i, j), i in [0, w), j in [0, h), votes once per k into bin
 *     p = (uint32)(i C[k] + j S[k] + D 16384) >> (14 + q).  The argument is never negative and lies below 2^31 for w, h <= 16384;
 *     p < N.  H[k][p] is the number of votes, uint32; an entry is at most (2 b + 1) max(w, h) < 2^19.
 *  3. Spectrum.  HS[k] = sum_p H[k][p]^2, uint64; n_sites = sum_p H[k][p] for every k.
 *  4. Rotation scores (host arithmetic inside the library; both slots filled with equal L, T, q).  sh_d is the least shift with
 *     (max_k HS_d[k]) >> sh_d < 2^26, sh_s likewise; CC[m] = sum_k (HS_d[k] >> sh_d) (HS_s[(k - m) mod T] >> sh_s), m in [0, T),
 *     uint64 (2^52 2^10: nothing wraps).  CC peaks where the source frame is turned by m pi / T (mod pi) in the destination's.
 *  5. Row correlation of a pair (m, k), m in [0, 2T), k in [0, T).  kk = k - m; add T until kk >= 0, toggling f once per addition
 *     (0, 1 or 2 additions).  A[p] = H_d[k][p], p in [0, N_d); B[p'] = H_s[kk][f ? N_s - 1 - p' : p'], p' in [0, N_s);
 *     XC[d] = sum_p' A[p' + d] B[p'] for d in [-(N_s - 1), N_d - 1], terms with p' + d outside A being zero; uint64, nothing
 *     wraps.  The record: best_shift the arg-max, ties to the smallest d; n_ties how many d reach the maximum (an all-zero XC:
 *     -(N_s - 1), N_d + N_s - 1, 0); sum = sum_d XC[d] = n_sites_d n_sites_s.
 * Every quantity is an integer: any vote order, reduction tree or atomic order gives the same bits.  The library forms no
 * threshold and picks no peak.  From a shift d of pair (m, k), with theta = m pi / T, psi = k pi / T, n(a) = (cos a, sin a), o_d and
 * o_s the slots' (x0, y0), and the translation t of the source frame in the destination's in cells:
 *     t . n(psi) = b d + o_d . n(psi) - o_s . n(psi - theta) - D_d + D_s + (f ? b - 1 - ((2 D_s) mod b) : 0)
 * up to a bin's width (the last term: a flipped row counts its bins from the other end, where the floor of step 2 and N_s - 1 =
 * (2 D_s) >> q leave that much); two pairs with different k give t. */
typedef struct slamhip_hough_shift {
    int32_t best_shift;                /* the arg-max of XC, ties to the smallest d */
    int32_t n_ties;                    /* how many d reach the maximum */
    uint64_t best_value;               /* XC[best_shift] */
    uint64_t sum;                      /* sum_d XC[d] */
} slamhip_hough_shift;                 /* 24 bytes, no padding */
/* Fill a slot.  out_info = {w, h, x0, y0, D, N, n_sites}; out_spectrum: uint64[T]; out_H: NULL or uint32[T * N], row k at k * N.  For
 * slot 1, level must be the source's level and world 0.  On the operator's stream behind everything already enqueued: the table's
 * copy, for slot 0 the lattice search's class map of the level (re-packed on every call), a memset of H, then k17_vote -- the grid is
 * (tiles of 64 x 64 cells, chunks of 64 angles); a tile without a site leaves at once; the others list their sites in LDS and keep a
 * histogram of 96 bins per angle there (a tile's votes at one angle span at most (91 >> q) + 2 bins), a wavefront takes a site and
 * its lanes the 64 angles, so no two lanes share an address; the non-zero bins go out as 32-bit atomic adds -- and k17_spectrum, a
 * workgroup per angle.  H, the spectrum and every row's non-zero extent stay in device memory, with a host copy of the spectrum,
 * until the slot is filled again; slamhip_hs_merge_set_source, _merge_clear_source and slamhip_hs_reset empty slot 1,
 * slamhip_hs_reset slot 0 too; a refused call leaves the slot as it was.  The blocks belong to the hs, are made by the first call
 * and freed by slamhip_hs_hough_clear or slamhip_hs_destroy; an hs that never calls it allocates nothing.  Blocking, the context's
 * bounded wait; results come back through pinned staging.  SLAMHIP_ERR_INVALID, nothing launched: level, slot, world, site_mask, T or
 * q out of range; slot 1 with world != 0 or a level that is not the source's; w or h above 16384; T * N > 2^24.  SLAMHIP_ERR_STATE:
 * slot 1 without a source.  A poisoned context: SLAMHIP_ERR_TIMEOUT.  The limits are design conditions, not measurements. */
int32_t slamhip_hs_hough(slamhip_hs *hs, int32_t level, int32_t slot, int32_t world, int32_t site_mask, int32_t T, int32_t q,
                         int32_t out_info[7], uint64_t *out_spectrum, uint32_t *out_H);
/* Step 4: out_cc = uint64[T].  It launches nothing.  SLAMHIP_ERR_STATE unless both slots are filled with equal level, T, q. */
int32_t slamhip_hs_hough_rotation(slamhip_hs *hs, uint64_t *out_cc);
/* Step 5 for P pairs (pairs: P x 2 int32_t, (m, k); P in [1, 256]): out_shifts, P records; out_xc: NULL, or the P arrays XC of
 * N_d + N_s - 1 entries each, one after another, entry d + N_s - 1 the shift d.  k17_xcorr: the grid is (pair, block of 256 shifts);
 * both rows trimmed to their non-zero extents, B's through LDS in pieces (flipped on the way in), a shift per lane along A,
 * 32 x 32 -> 64-bit products, a partial record per block; k17_xcorr_finish merges them, a wavefront per pair.  Blocking, as
 * slamhip_hs_hough.  SLAMHIP_ERR_INVALID, nothing launched: P out of range; an m outside [0, 2T) or a k outside [0, T); out_xc given
 * with P * (N_d + N_s - 1) > 2^22.  SLAMHIP_ERR_STATE as slamhip_hs_hough_rotation.  A poisoned context: SLAMHIP_ERR_TIMEOUT. */
int32_t slamhip_hs_hough_shifts(slamhip_hs *hs, const int32_t *pairs, int32_t P, slamhip_hough_shift *out_shifts, uint64_t *out_xc);
/* Free the unit's blocks; both slots are empty afterwards.  Never fails for an hs that has none. */
int32_t slamhip_hs_hough_clear(slamhip_hs *hs);
/* Test hooks (no device involved), each running the header text the kernels run (hs_hough.h) in plain loops.  _table: step 1,
 * out_cs = int32[2T], C then S.  _hough: steps 1 - 3 over cls[cw * ch] (row-major class bits); out_H uint32[T * N] or NULL,
 * out_spectrum uint64[T] or NULL, not both NULL; the refusals of slamhip_hs_hough for site_mask, T, q, the size and T * N.
 * _hough_rotation: step 4 over two spectra of T entries.  _hough_xcorr: step 5 over A[Nd] and the source ROW B[Ns] (the flip is
 * applied inside); out_xc uint64[Nd + Ns - 1] or NULL; Nd, Ns in [1, 65537]. */
int32_t slamhip_debug_hough_table(int32_t T, int32_t *out_cs);
int32_t slamhip_debug_hough(const uint8_t *cls, int32_t cw, int32_t ch, int32_t site_mask, int32_t T, int32_t q, uint32_t *out_H,
                            uint64_t *out_spectrum);
int32_t slamhip_debug_hough_rotation(const uint64_t *spectrum_d, const uint64_t *spectrum_s, int32_t T, uint64_t *out_cc);
int32_t slamhip_debug_hough_xcorr(const uint32_t *A, int32_t Nd, const uint32_t *B, int32_t Ns, int32_t flip, uint64_t *out_xc,
                                  slamhip_hough_shift *out_shift);

/* Scan signatures and a keyframe store for loop candidates (K18; no reference counterpart).  Every unit above scores a scan against
 * the MAP; none compares a scan with earlier scans, and the lattice search finds a pose only near a centre the caller supplies.  A
 * signature is a rotation-invariant summary of one scan: which of n_ring x 64 polar cells round the sensor hold an end point.  A ring
 * is one 64-bit word, so a turn of the scan by one sector is a rotate of every word by one bit, and two scans are compared over all
 * 64 headings with AND, rotate and popcount alone.  The store keeps the signatures of keyframes in device memory; a query ranks the
 * keyframes against the scan that was set, the self search every keyframe against the earlier ones.  The hits are CANDIDATES: the
 * caller verifies one with slamhip_hs_relocalise round the pose guess (HectorSLAMProcessor.VerifyLoop in the mirrors).
 * THE DEFINITION.  SLAMHIP_SIG_SECTORS = 64.  The spec: Rg = n_ring in [1, 32]; rc = ring_cells >= 1 with 2 rc Rg <= 32768; scale a
 * finite binary32 > 0, in cells per metre -- the caller's choice, unrelated to any level of the map.
 *  1. Table.  For k in [0, 16): C[k] = (int)rint(16384 * cos(a)), S[k] = (int)rint(16384 * sin(a)) with a = ((double)k * M_PI) / 32.0,
 *     formed in binary64 on the HOST; for k >= 16: C[k] = -S[k - 16], S[k] = C[k - 16], so a quarter turn is exact.  The device never
 *     forms a sine: the table is an argument of the launches.
 *  2. Cell of a point.  (px, py) is the scan point slamhip_hs_set_scan took; the scan origin plays no part.  fx = px * scale,
 *     fy = py * scale, each ONE binary32 multiply rounded on its own.  A point with a NaN or |f| >= 2^14 on either axis is IGNORED.
 *     u = 2 floor(fx) + 1, v = 2 floor(fy) + 1: odd doubled coordinates -- the cell's centre, never the origin, never on an axis.
 *  3. Ring.  d2 = u^2 + v^2 (below 2^31); ring = the number of j in [1, Rg] with (2 rc j)^2 <= d2.  ring == Rg: the point is FAR --
 *     counted, not set.
 *  4. Sector.  The one k with C[k] v - S[k] u >= 0 and C[k+1 mod 64] v - S[k+1 mod 64] u < 0.  int32; the magnitudes stay below 2^30.
 *     Exactly one k exists for every odd (u, v) because cross(d_k, d_{k+1}) > 0 for all k (tests/test_hs_sig_abi.py proves it).
 *  5. Signature.  sig[r], r in [0, Rg), uint64: bit k is set iff some point has (ring r, sector k).  slamhip_sig_info: n_points,
 *     n_ignored, n_far, n_set = the total popcount (at most 2048).
 *  6. Match of query q against key k at shift s in [0, 64): inter(s) = sum_r popcount(q[r] & rotl(k[r], s)); shift = the SMALLEST s
 *     that maximises inter; uni = n_set(q) + n_set(k) - inter; score = uni ? (inter << 16) / uni : 0 -- integer division, at most
 *     65536 (the Jaccard index of the two bit sets in 16.16 fixed point).  uni falls as inter rises, so the maximal inter is the
 *     maximal score: one division per pair.  THE SIGN: q == rotl(k, s) means that the query sees everything s sectors FURTHER ROUND
 *     (counter-clockwise) than the key did, so the query's heading is theta_k - s * 2 pi / 64.
 *  7. Query over the keyframes with index in [first, last): the B <= 16 best, ordered by higher score, then lower index.  Fewer than B
 *     keyframes in the range: fewer hits; out_n holds the count.
 *  8. Self search over [first, last) with min_gap >= 1: for every keyframe i of the range ONE hit, the best j in [first, i - min_gap]
 *     by rule 7 with B = 1 (query i, key j); index = -1, score = 0 and every other field 0 if that range is empty.
 * Every quantity behind rule 2's two multiplies is an integer: any order of atomics and reductions gives the same bits.
 * The self search merges by a 64-bit atomic max on a packed key, low bits first: shift 6 bits, (2^20 - 1 - index) 20 bits, score 17
 * bits, then one bit every real pair has (an empty slot is 0): 44 bits in all. */
#define SLAMHIP_SIG_SECTORS 64
#define SLAMHIP_SIG_MAX_RINGS 32
#define SLAMHIP_SIG_MAX_HITS 16
#define SLAMHIP_SIG_MAX_KEYS (1 << 20)
typedef struct slamhip_sig_spec {
    float scale;                       /* cells per metre */
    int32_t n_ring;                    /* Rg */
    int32_t ring_cells;                /* rc: a ring is rc cells wide */
} slamhip_sig_spec;                    /* 12 bytes */
typedef struct slamhip_sig_info {
    int32_t n_points, n_ignored, n_far, n_set;
} slamhip_sig_info;                    /* 16 bytes */
typedef struct slamhip_sig_hit {
    uint32_t score;                    /* rule 6, at most 65536 */
    int32_t index;                     /* the keyframe; -1: no hit */
    int16_t shift, inter, uni, n_set_key;
} slamhip_sig_hit;                     /* 16 bytes, no padding */
/* Set the spec and EMPTY the store (signatures of another spec do not compare).  The table goes to device memory here.  The unit's
 * blocks belong to the hs, are made by this call and later ones and freed by slamhip_hs_sig_clear or slamhip_hs_destroy; an hs that
 * never calls it allocates nothing.  SLAMHIP_ERR_INVALID: a spec outside the definition's ranges.  Every other slamhip_hs_sig_* call
 * gives SLAMHIP_ERR_STATE before this one (and after slamhip_hs_sig_clear).  All of them but _sig_count are blocking with the
 * context's bounded wait (a poisoned context: SLAMHIP_ERR_TIMEOUT), run on the operator's stream behind everything already enqueued
 * and bring their results back through pinned staging. */
int32_t slamhip_hs_sig_configure(slamhip_hs *hs, const slamhip_sig_spec *spec);
/* Rules 2 - 5 over the scan slamhip_hs_set_scan took (no scan, or one of 0 points: the empty signature), appended to the store as
 * keyframe *out_index = the count before the call.  pose: three floats, opaque to the library, kept on the host and handed back by
 * slamhip_hs_sig_download.  out_index, out_sig (uint64[n_ring]) and out_info may be NULL.  k18_sig: a workgroup of 256 lanes per
 * scan, a point per lane and pass; the ring by a hardware square root with an exact integer fix-up, the sector by the quadrant of
 * the signs and four steps with exact cross products; the words in LDS, filled by 64-bit LDS atomic OR; the counts by ballot.
 * The store: blocks of 64 keyframes, ring r of a block's 64 keyframes contiguous (sig[block][r][64]), n_set as uint16 beside them;
 * it grows by whole blocks, the earlier blocks copied as they are.  SLAMHIP_ERR_INVALID: the store holds 2^20 keyframes.
 * slamhip_hs_reset empties the store and keeps the blocks and the spec; slamhip_hs_shift and the other window calls do not touch it
 * (the poses are the caller's). */
int32_t slamhip_hs_sig_add(slamhip_hs *hs, const float pose[3], int32_t *out_index, uint64_t *out_sig, slamhip_sig_info *out_info);
/* B scans of a log appended in one launch, a workgroup per scan: scan b is the points xy[2 offsets[b]] .. xy[2 offsets[b + 1]) (x, y
 * pairs), offsets = B + 1 entries, offsets[0] = 0, non-decreasing; poses = B x 3 floats; *out_first (may be NULL) = the first new
 * index.  The scan that slamhip_hs_set_scan took is not touched.  SLAMHIP_ERR_INVALID, nothing launched: B outside [1, 4096]; bad
 * offsets; more than 2^24 points; more than 2^20 keyframes afterwards. */
int32_t slamhip_hs_sig_add_scans(slamhip_hs *hs, const float *xy, const int32_t *offsets /* B + 1 */, int32_t B, const float *poses,
                                 int32_t *out_first);
/* Rule 7: the scan slamhip_hs_set_scan took against the keyframes [first, last); nothing is appended.  out_hits: room for B records;
 * *out_n of them are written.  out_sig (uint64[n_ring]) and out_info: the query's own signature, or NULL.  k18_query: a key per
 * lane; the 64 rotations of the query are formed once per workgroup in LDS (at most 16 KB) and read as broadcasts; per lane a
 * running (inter, shift) with ties to the smaller s, then one division; the workgroup's B best by repeated wavefront arg-max on
 * score << 32 | ~index.  k18_query_finish, one workgroup, merges the workgroups' lists.  SLAMHIP_ERR_INVALID, nothing launched: B
 * outside [1, 16]; not 0 <= first <= last <= count. */
int32_t slamhip_hs_sig_query(slamhip_hs *hs, int32_t first, int32_t last, int32_t B, slamhip_sig_hit *out_hits, int32_t *out_n,
                             uint64_t *out_sig, slamhip_sig_info *out_info);
/* Rule 8: out_hits = last - first records, record i - first for keyframe i.  k18_self: the grid is (tile of 64 queries, tile of 64
 * keys); tile pairs wholly above the diagonal band leave at once; the key tile is staged in LDS, a query per lane rotates its own
 * words in registers; the best per query is merged across key tiles by a 64-bit agent-scope atomic max on the packed key above;
 * k18_self_finish forms inter and uni of the winners again.  SLAMHIP_ERR_INVALID: min_gap < 1; not 0 <= first <= last <= count. */
int32_t slamhip_hs_sig_self(slamhip_hs *hs, int32_t first, int32_t last, int32_t min_gap, slamhip_sig_hit *out_hits);
/* The number of keyframes in the store.  It launches nothing. */
int32_t slamhip_hs_sig_count(slamhip_hs *hs, int32_t *out_count);
/* Keyframes [first, first + n) out of the store: sig = uint64[n * n_ring], KEY-MAJOR (keyframe i's words at (i - first) * n_ring), or
 * NULL; poses = float[n * 3] or NULL; not both NULL.  SLAMHIP_ERR_INVALID: a range outside the store. */
int32_t slamhip_hs_sig_download(slamhip_hs *hs, int32_t first, int32_t n, uint64_t *sig, float *poses);
/* n keyframes APPENDED from key-major words and poses (what slamhip_hs_sig_download gave: keyframes are saved and loaded beside a
 * saved world); the library counts the popcounts itself.  SLAMHIP_ERR_INVALID: n < 0 or more than 2^20 keyframes afterwards. */
int32_t slamhip_hs_sig_upload(slamhip_hs *hs, int32_t n, const uint64_t *sig, const float *poses);
/* Free the unit's blocks and forget the spec.  Never fails for an hs that has none. */
int32_t slamhip_hs_sig_clear(slamhip_hs *hs);
/* Test hooks (no device involved), each running the header text the kernels run (hs_sig.h) in plain loops.  _table: rule 1, C then
 * S.  _sig: rules 2 - 5 over n points (x, y pairs); out_info may be NULL; the refusals of slamhip_hs_sig_configure.  _sig_ring: rule 3
 * as the kernel forms it (square root and fix-up) for n values of d2 >= 0.  _sig_sector: rule 4 as the kernel forms it (quadrant and
 * four steps) for n pairs (u, v), both odd and within +-32767.  _sig_search: rule 7 (query_sig = uint64[n_ring]) or, with query_sig
 * NULL, rule 8 (B ignored; *out_n = last - first) over a KEY-MAJOR store of N keyframes with their popcounts n_set;
 * SLAMHIP_ERR_INVALID as the device calls, and for an n_set entry of the range that disagrees with its words. */
int32_t slamhip_debug_sig_table(int32_t out_cs[128]);
int32_t slamhip_debug_sig(const float *xy, int32_t n, const slamhip_sig_spec *spec, uint64_t *out_sig, slamhip_sig_info *out_info);
int32_t slamhip_debug_sig_ring(const int32_t *d2, int32_t n, int32_t n_ring, int32_t ring_cells, int32_t *out_ring);
int32_t slamhip_debug_sig_sector(const int32_t *uv, int32_t n, int32_t *out_sector);
int32_t slamhip_debug_sig_search(const uint64_t *query_sig, const uint64_t *store_sig, const uint16_t *n_set, int32_t N, int32_t n_ring,
                                 int32_t first, int32_t last, int32_t min_gap, int32_t B, slamhip_sig_hit *out_hits, int32_t *out_n);

/* Overwrite the poses of keyframes [first, first + n) of the store (K18): what slamhip_hs_sig_download hands back from here on.  The
 * poses live on the host: nothing is launched.  It is how a correction (slamhip_hs_pg_relax below) is taken back into the store.
 * SLAMHIP_ERR_STATE before slamhip_hs_sig_configure; SLAMHIP_ERR_INVALID: a range outside the store. */
int32_t slamhip_hs_sig_set_poses(slamhip_hs *hs, int32_t first, int32_t n, const float *poses);

/* Relaxation of a 2-D pose graph on the device (K19; no reference counterpart).  K18 finds loop candidates and K7 verifies one; a
 * verified loop says that the keyframe poses are inconsistent, and this unit spreads that error over the trajectory: Gauss-Newton
 * steps, each solved matrix-free by block-Jacobi preconditioned conjugate gradients (PCG).  slamhip_hs_update_by_scan and the
 * processor's per-scan call never enter it.
 * THE DEFINITION.  All arithmetic is binary64 + - * / and rint, ONE rounding per operation (no fused multiply-add), evaluated in the
 * order the parentheses give; there is no sqrt, no libm and no floating-point atomic.
 *  1. Graph.  N nodes (x, y, theta) as doubles, N in [1, 2^20], every value finite and |theta| <= 65536.  `fixed`: a byte per node,
 *     non-zero = the node does not move; NULL = node 0 alone is fixed; at least one node is fixed.  E edges (i, j), i != j, E in
 *     [0, 2^22], each with a measurement z = (zx, zy, zt) -- node j seen in node i's frame -- and a diagonal weight w = (wx, wy, wt),
 *     every weight finite and > 0.  Duplicate edges are allowed: they are two edges.
 *  2. Trig.  (s, c) = sh_det_sincos(theta) (det_trig.h): the binary64 Cody-Waite reduction by pi / 2 and the degree-13 / 14 kernels of
 *     sh_det_sincosf without the final rounding to binary32; contract |theta| <= 65536; at most 2 ulp from NumPy's binary64 sin / cos
 *     on 10^5 angles (measured; tests/test_hs_pg_abi.py).  wrap(a) = a - TWO_PI * rint(a / TWO_PI), TWO_PI = 6.283185307179586 (the binary64
 *     nearest 2 pi).
 *  3. Edge record, formed once per outer iteration from the poses as they stand: (s, c) of theta_i; dx = x_j - x_i, dy = y_j - y_i;
 *     ux = c * dx + s * dy, uy = c * dy - s * dx; r = (ux - zx, uy - zy, wrap((theta_j - theta_i) - zt));
 *     A = dr / d(node i) = [[-c, -s, uy], [s, -c, -ux], [0, 0, -1]], B = dr / d(node j) = [[c, s, 0], [-s, c, 0], [0, 0, 1]] (row k:
 *     residual k; column a: the node's variable a); chi2_e = (wx * (r0 * r0) + wy * (r1 * r1)) + wt * (r2 * r2).
 *  4. Sums over a node's edges run in increasing EDGE INDEX -- and for one edge the i side before the j side, which cannot occur
 *     because i != j.  J is A where the node is the edge's i, B where it is its j; the 0 and 1 entries of A and B take part in the
 *     products like any other value.  D_n starts as lambda on the diagonal and +0 elsewhere; per incident edge, for a <= b:
 *       D[a][b] = D[a][b] + (((J[0][a] * wx) * J[0][b] + (J[1][a] * wy) * J[1][b]) + (J[2][a] * wt) * J[2][b]);   D[b][a] = D[a][b].
 *     g_n starts as +0; per incident edge, with v = (wx * r0, wy * r1, wt * r2):
 *       g[a] = g[a] + ((J[0][a] * v0 + J[1][a] * v1) + J[2][a] * v2).
 *     M_n = D_n^-1 by the adjugate over the determinant: c00 = d11 * d22 - d12 * d12, c01 = d02 * d12 - d01 * d22,
 *     c02 = d01 * d12 - d02 * d11, c11 = d00 * d22 - d02 * d02, c12 = d01 * d02 - d00 * d12, c22 = d00 * d11 - d01 * d01,
 *     det = (d00 * c00 + d01 * c01) + d02 * c02, M[a][b] = M[b][a] = cab / det.  M_n = 0 unless det > 0: a free node with no edge and
 *     lambda = 0 has M = 0 and does not move.  A fixed node has M = 0 and g = 0.
 *     M v, for z = M res:  out[a] = (M[a][0] * v0 + M[a][1] * v1) + M[a][2] * v2.
 *  5. Operator q = H p.  Per edge t_e[k] = w_k * (((A[k][0] * pi0 + A[k][1] * pi1) + A[k][2] * pi2) + ((B[k][0] * pj0 + B[k][1] * pj1)
 *     + B[k][2] * pj2)), then q_n[a] starts as lambda * p_n[a] and takes, in rule 4's order, q[a] = q[a] + ((J[0][a] * t0 + J[1][a] * t1)
 *     + J[2][a] * t2).  The rows of fixed nodes are 0.  (The kernel forms t_e again at each end of an edge: the same bits.)
 *  6. Dot products -- the one reduction shape.  A field's term of a node is (u0 * v0 + u1 * v1) + u2 * v2.  The sum of a sequence of
 *     length L: pad with +0.0 to a multiple of 256 (L = 0: to 256); in every block of 256, t[k] = t[k] + t[k + h] for k < h, for
 *     h = 128, 64, .. 1; the blocks' t[0] are the next sequence; repeat while more than one value is left.  chi2 = the sum of chi2_e
 *     over the edges by the same shape.  Nothing depends on the grid, the order of workgroups or check_every.
 *  7. PCG, per outer iteration: x = 0, res = -g, z = M res, p = z, rz = res . z, rz0 = rz.  Before iteration k = 0, 1, ..: stop with
 *     `stopped` = 0 if rz <= (tol * tol) * rz0 or rz <= 0; else stop with `stopped` = 1 if k == n_cg.  One iteration: q = H p,
 *     pq = p . q; unless pq > 0 stop with `stopped` = 2 (breakdown; x stays as it was); alpha = rz / pq; x[a] = x[a] + alpha * p[a],
 *     res[a] = res[a] - alpha * q[a]; z = M res; rz' = res . z; beta = rz' / rz; p[a] = z[a] + beta * p[a]; rz = rz'.  Then, for every
 *     free node, pose[a] = pose[a] + x[a] and theta = wrap(theta); a fixed node is not touched.
 *  8. Output per outer iteration, slamhip_pg_iter: chi2 BEFORE the step, rz0, the last rz, cg_iters (the iterations completed),
 *     stopped.  chi2 after the last step comes beside the array.
 * Block-Jacobi sees one node at a time, so on chain-like graphs PCG needs a number of iterations of the order of the chain's length
 * (about 3 N for a ring closed by one loop): DESIGN.md section 4 "K19" says what that costs, and slamhip_hs_pg_relax_tri below is the
 * preconditioner for that graph. */
#define SLAMHIP_PG_MAX_NODES (1 << 20)
#define SLAMHIP_PG_MAX_EDGES (1 << 22)
#define SLAMHIP_PG_MAX_OUTER 64
#define SLAMHIP_PG_MAX_CG (1 << 20)
typedef struct slamhip_pg_spec {
    int32_t n_outer;                   /* offset 0: Gauss-Newton steps, [1, 64] */
    int32_t n_cg;                      /* offset 4: the most PCG iterations of a step, [1, 2^20] */
    int32_t check_every;               /* offset 8: >= 1, PCG iterations the host enqueues between two reads of the stop word; no result depends on it */
    int32_t reserved;                  /* offset 12: 0 */
    double lambda;                     /* offset 16: >= 0, added to every diagonal entry of H */
    double tol;                        /* offset 24: >= 0, rule 7 */
} slamhip_pg_spec;                     /* 32 bytes */
typedef struct slamhip_pg_iter {
    double chi2, rz0, rz;              /* offsets 0, 8, 16 */
    int32_t cg_iters, stopped;         /* offsets 24, 28; stopped: 0 tolerance reached, 1 n_cg reached, 2 breakdown */
} slamhip_pg_iter;                     /* 32 bytes */
/* Take a graph (rule 1), replacing any earlier one.  Everything is validated on the host before anything is launched:
 * SLAMHIP_ERR_INVALID for N or E outside their ranges, an index outside [0, N), i == j, a value that is not finite, |theta| > 65536,
 * a weight <= 0, a `fixed` array without a non-zero byte.  The host builds the node -> (edge, side) lists by a counting sort that
 * keeps the edge order; the graph goes to ONE device block through pinned staging.  poses = N x 3 doubles, ij = E x 2 int32,
 * z and w = E x 3 doubles (all three may be NULL when E == 0).  The unit's blocks belong to the hs, are made by this call and freed by
 * slamhip_hs_pg_clear or slamhip_hs_destroy; slamhip_hs_reset drops the graph and keeps the blocks.  A call that validation refuses
 * leaves the earlier graph as it was; after SLAMHIP_ERR_NOMEM or SLAMHIP_ERR_HIP the earlier graph is GONE.  Blocking, as every call below,
 * with the context's bounded wait, on the operator's stream behind everything already enqueued. */
int32_t slamhip_hs_pg_set(slamhip_hs *hs, const double *poses, const uint8_t *fixed, int32_t N, const int32_t *ij, const double *z,
                          const double *w, int32_t E);
/* Rules 3 - 8: spec->n_outer Gauss-Newton steps from the poses as they stand in device memory -- a second call continues from the
 * relaxed poses.  out_iters: n_outer records; *out_chi2_final: chi2 after the last step.  k19_linearise (a lane per edge), k19_diag
 * (a lane per node), k19_begin (one workgroup, once per step), then per PCG iteration k19_apply, k19_step, k19_dir (a lane per node
 * each; every workgroup finishes rule 6's tree itself, so alpha and beta need no launch of their own), k19_update.  Rule 7's stop is
 * decided ON THE DEVICE, by the same comparisons, into a word the later launches read: a launch enqueued behind the stop leaves at
 * once.  The host enqueues check_every iterations (at most 1024, whatever check_every says), reads the word, and goes on or not.  SLAMHIP_ERR_INVALID, nothing launched and
 * nothing written: a spec outside the ranges above, reserved != 0.  SLAMHIP_ERR_STATE: no graph. */
int32_t slamhip_hs_pg_relax(slamhip_hs *hs, const slamhip_pg_spec *spec, slamhip_pg_iter *out_iters, double *out_chi2_final);
/* The poses as they stand: N x 3 doubles; N must be the graph's.  SLAMHIP_ERR_STATE: no graph. */
int32_t slamhip_hs_pg_get(slamhip_hs *hs, double *poses, int32_t N);
/* Rule 3 at the poses as they stand: out_r = E x 3 doubles, out_chi2 = E doubles (chi2_e); either may be NULL, not both.  A caller
 * throws a bad loop edge out by its chi2 and relaxes again.  SLAMHIP_ERR_STATE: no graph. */
int32_t slamhip_hs_pg_residuals(slamhip_hs *hs, double *out_r, double *out_chi2);
/* Free the unit's blocks.  Never fails for an hs that has none. */
int32_t slamhip_hs_pg_clear(slamhip_hs *hs);
/* Test hooks (no device involved).  _pg_relax: the whole definition over the caller's arrays, from the header text the kernels run
 * (hs_pg.h) in plain loops; poses are relaxed IN PLACE; out_r (E x 3) and out_chi2 (E), rule 3 at the final poses, may be NULL; the
 * refusals of slamhip_hs_pg_set and _pg_relax, nothing written.  _pg_sum: rule 6 over L >= 0 values.  _sincos: rule 2 for n angles. */
int32_t slamhip_debug_pg_relax(double *poses, const uint8_t *fixed, int32_t N, const int32_t *ij, const double *z, const double *w,
                               int32_t E, const slamhip_pg_spec *spec, slamhip_pg_iter *out_iters, double *out_chi2_final,
                               double *out_r, double *out_chi2);
int32_t slamhip_debug_pg_sum(const double *v, int32_t L, double *out);
int32_t slamhip_debug_sincos(const double *a, int32_t n, double *out_s, double *out_c);

/* The odometry-chain preconditioner of the relaxation (K22; no reference counterpart).  The graph this library itself builds
 * (HectorSLAMProcessor.RelaxKeyframes, close_loops) has an edge (k, k + 1) for every pair of consecutive keyframes and a few loop
 * edges.  Here PCG is preconditioned by T, the BLOCK-TRIDIAGONAL part of H (the diagonal blocks and the blocks H[n][n + 1],
 * H[n + 1][n]), solved exactly by block cyclic reduction.  With L' edges that are not chain edges and join two free nodes, H - T has
 * rank <= 6 L', so PCG ends in at most 6 L' + 1 iterations in exact arithmetic, whatever N is.
 * THE DEFINITION.  Rules 1 - 3, 5, 6 and 8 of slamhip_hs_pg_relax hold unchanged; rule 4's M and the "z = M res" of rule 7 are
 * replaced by z = T^-1 res as rules T1 - T5 say.  Binary64 + - * / only, one rounding per operation, in the order the parentheses give.
 * A symmetric 3 x 3 is computed for a <= b and mirrored; U, W are general 3 x 3.
 *  T1. Live and dead nodes.  A node is LIVE if it is free and rule 4's det of D_n is > 0; else it is DEAD.  A live node's diagonal
 *      block is rule 4's D_n (lambda included) and its P_n is rule 4's M_n.  A dead node's diagonal block and P are the identity, its
 *      couplings are 0, and its z is +0 whatever the right-hand side says.
 *  T2. Coupling.  For n in [0, N - 1), U_n = H[n][n + 1] starts as +0.  If n and n + 1 are both live: for every edge that joins n and
 *      n + 1, in either direction, in increasing edge index, with Jn the edge's Jacobian (A or B) at node n and Jm its other one:
 *        U[a][b] = U[a][b] + (((Jn[0][a] * wx) * Jm[0][b] + (Jn[1][a] * wy) * Jm[1][b]) + (Jn[2][a] * wt) * Jm[2][b]).
 *      Below the diagonal stands U_n^T.  A missing chain edge or a dead neighbour leaves U_n = 0: the chain falls into segments.
 *  T3. Factorisation, once per outer iteration: block cyclic reduction.  Level 0 has n_0 = N blocks D_k, U_k and P_k (T1); level l + 1
 *      has n_{l+1} = ceil(n_l / 2) blocks, until one block is left.  Block m of level l + 1 comes from block k = 2 m of level l:
 *        D' = D_k;
 *        if k >= 1:      W = P_{k-1} U_{k-1};   D'[a][b] = D'[a][b] - ((U_{k-1}[0][a] * W[0][b] + U_{k-1}[1][a] * W[1][b]) + U_{k-1}[2][a] * W[2][b]);
 *        if k + 1 < n_l: W = P_{k+1} U_k^T;     D'[a][b] = D'[a][b] - ((U_k[a][0] * W[0][b] + U_k[a][1] * W[1][b]) + U_k[a][2] * W[2][b]);
 *        if k + 2 < n_l: W = P_{k+1} U_{k+1};   U'[a][b] = 0 - ((U_k[a][0] * W[0][b] + U_k[a][1] * W[1][b]) + U_k[a][2] * W[2][b]);  else U' = +0;
 *      where W = P X means W[a][b] = (P[a][0] * X[0][b] + P[a][1] * X[1][b]) + P[a][2] * X[2][b] (X^T: X[b][0], X[b][1], X[b][2]).
 *      A term whose `if` fails is not subtracted at all.  P' = D'^-1 by rule 4's adjugate over the determinant, P' = 0 unless
 *      det > 0: nothing ever divides by a determinant that is not positive.
 *  T4. Solve, z = T^-1 r, once per PCG iteration.  Forward, level l -> l + 1, k = 2 m, with y = P v by rule 4's "M v":
 *        r' = r_k;
 *        if k >= 1:      y = P_{k-1} r_{k-1};   r'[a] = r'[a] - ((U_{k-1}[0][a] * y0 + U_{k-1}[1][a] * y1) + U_{k-1}[2][a] * y2);
 *        if k + 1 < n_l: y = P_{k+1} r_{k+1};   r'[a] = r'[a] - ((U_k[a][0] * y0 + U_k[a][1] * y1) + U_k[a][2] * y2).
 *      At the last level z = P r.  Backward, level l + 1 -> l: an even k takes z of block k / 2 of level l + 1; an odd k
 *        t = r_k;   t[a] = t[a] - ((U_{k-1}[0][a] * zl0 + U_{k-1}[1][a] * zl1) + U_{k-1}[2][a] * zl2),            zl = z_{k-1};
 *        if k + 1 < n_l: t[a] = t[a] - ((U_k[a][0] * zr0 + U_k[a][1] * zr1) + U_k[a][2] * zr2),                  zr = z_{k+1};
 *        z_k = P_k t.
 *      At level 0 the z of a dead node is +0 (T1).
 *  T5. PCG: rule 7 with z = T^-1 res in both places, the same stop rules, the same outputs.  If T is not positive definite -- a chain
 *      segment with neither a fixed neighbour nor an edge out of it, and lambda = 0 -- pivots of T3 become 0 and PCG may stop with
 *      `stopped` = 2; block-Jacobi cannot make that graph converge either.  Where no chain edge joins two live nodes T is rule 4's
 *      block diagonal, and every value equals slamhip_hs_pg_relax's under == (a zero may differ in its sign).
 * Nothing depends on the grid, the launch shape, check_every or the developer's SLAMHIP_K22_TAIL.
 * slamhip_hs_pg_relax_tri: the spec, the outputs and the refusals of slamhip_hs_pg_relax; it continues from the poses as they stand, and
 * calls of either kind may follow one another on one graph.  The levels' blocks (D, P, U and the right-hand sides of about 2 N blocks:
 * 361 bytes per node, 379 MB at N = 2^20) are made by the first call of this or of _pg_tri_apply, grown with N, and freed by
 * slamhip_hs_pg_clear / _destroy; a caller that uses neither allocates nothing.  After SLAMHIP_ERR_NOMEM the graph is as it was and
 * slamhip_hs_pg_relax still runs.  Launches: k22_diag and k22_coupling (a lane per node), k22_reduce (one per level of more than S = 1024
 * blocks) and k22_factor_tail (ONE workgroup, the levels of at most S blocks) once per outer iteration; per PCG iteration k19_apply,
 * k19_step<false>, then k22_forward per large level, k22_solve_tail (one workgroup, the small levels in LDS) and k22_backward per large level
 * -- 2 ceil(log2(N / S)) + 1 launches, ONE for N <= S; the last of them leaves the block sums of res . z -- and k19_dir.  The stop word
 * works as in slamhip_hs_pg_relax.  SLAMHIP_K22_TAIL (developer, read at every call, [1, 1024]) sets S.
 * slamhip_hs_pg_tri_apply: T1 - T4 alone at the poses as they stand, for one right-hand side: rhs and out = N x 3 doubles.  Blocking.
 * SLAMHIP_ERR_INVALID: lambda not finite or < 0; SLAMHIP_ERR_STATE: no graph. */
int32_t slamhip_hs_pg_relax_tri(slamhip_hs *hs, const slamhip_pg_spec *spec, slamhip_pg_iter *out_iters, double *out_chi2_final);
int32_t slamhip_hs_pg_tri_apply(slamhip_hs *hs, double lambda, const double *rhs, double *out);
/* Test hooks (no device involved), from the header text the kernels run (hs_pg_tri.h) in plain loops.  _pg_relax_tri: the arguments and
 * refusals of slamhip_debug_pg_relax.  _pg_tri_apply: the graph of slamhip_hs_pg_set, then lambda, rhs and out of slamhip_hs_pg_tri_apply. */
int32_t slamhip_debug_pg_relax_tri(double *poses, const uint8_t *fixed, int32_t N, const int32_t *ij, const double *z, const double *w,
                                   int32_t E, const slamhip_pg_spec *spec, slamhip_pg_iter *out_iters, double *out_chi2_final,
                                   double *out_r, double *out_chi2);
int32_t slamhip_debug_pg_tri_apply(const double *poses, const uint8_t *fixed, int32_t N, const int32_t *ij, const double *z,
                                   const double *w, int32_t E, double lambda, const double *rhs, double *out);

/* Damped (Levenberg-Marquardt) and robust relaxation (K26; no reference counterpart).  slamhip_hs_pg_relax and _relax_tri take plain
 * Gauss-Newton steps: a step may RAISE chi2 (DESIGN.md section 4 "K22" records it), and every edge counts quadratically, so one false
 * loop edge bends the whole trajectory.  Here every step is an ATTEMPT that is taken only if it lowers the cost, lambda moves with the
 * outcome, and an edge's weight may be scaled by a robust factor.  The existing calls and their results do not change.
 * THE DEFINITION.  Rules 1 - 8 and T1 - T5 above hold as they stand; R1 - R4 say what is put around them.  Binary64 + - * / and rint, one
 * rounding per operation, in the order the parentheses give; no sqrt and no libm -- which is why the kernels are the rational ones
 * (dynamic covariance scaling, Geman-McClure) and Cauchy and Huber are not offered.
 *  R1. Edge cost and factor, at the poses being linearised.  c_e = rule 3's chi2_e with the caller's weights w.  `robust`: a byte per
 *      edge, non-zero = the edge is robust; NULL = every edge is robust.  An edge that is not robust, or kind NONE: f_e = 1,
 *      rho_e = c_e.  A robust edge, with phi the spec's:
 *        DCS:  if c_e <= phi: f_e = 1, rho_e = c_e;
 *              else s = (2 * phi) / (phi + c_e);   f_e = s * s;   rho_e = (phi * ((3 * c_e) - phi)) / (c_e + phi).
 *        GM:   s = phi / (phi + c_e);   f_e = s * s;   rho_e = (phi * c_e) / (phi + c_e).
 *      w_eff = (f_e * wx, f_e * wy, f_e * wt).  F = the sum of rho_e over the edges by rule 6.
 *  R2. One attempt.  Rules 3 - 7 with w_eff in place of w and the current lambda (precond = 1: rules 3, 5, 6 and T1 - T5) give x.
 *      trial_n[a] = pose_n[a] + x_n[a] and trial theta = wrap(trial theta) for every free node; a fixed node's trial is its pose.
 *      F_trial = R1's F at the trial poses (its own c_e, f_e are not kept).  The attempt is ACCEPTED iff F_trial < F.
 *      Accepted: poses = trial;   lambda = lambda * down;   if lambda < lambda_min: lambda = lambda_min.
 *      Rejected: the poses stay;  lambda = lambda * up;     if lambda > lambda_max: lambda = lambda_max.
 *      The first attempt uses lambda0 as it is given.  Every attempt is one outer iteration, accepted or not.
 *  R3. Stop.  After n_outer attempts; earlier, behind an ACCEPTED attempt with (F - F_trial) <= ftol * F.  *out_n = the attempts made.
 *  R4. Record per attempt, slamhip_pg_lm_iter: F, F_trial, the lambda the attempt USED, rz0, rz, cg_iters and stopped as
 *      slamhip_pg_iter has them, accepted (1 or 0), three reserved words (0).  Records behind *out_n are not written.
 * CONSEQUENCE.  With kind NONE, lambda0 = lambda_min = 0 and every attempt accepted, w_eff = w and lambda = 0 throughout: the poses and
 * the rz0, rz, cg_iters and stopped of every record equal slamhip_hs_pg_relax's (precond = 1: _relax_tri's) with lambda = 0 under ==,
 * and F is its chi2.  Behind a rejected attempt the poses, and with them R1's values and rule 3's records, are unchanged: forming them
 * again or not gives the same bits.  Nothing depends on the grid, the launch shape or check_every. */
typedef struct slamhip_pg_lm_spec {
    int32_t n_outer;                   /* offset 0: attempts, [1, 64] */
    int32_t n_cg;                      /* offset 4: the most PCG iterations of an attempt, [1, 2^20] */
    int32_t check_every;               /* offset 8: >= 1, as slamhip_pg_spec's; no result depends on it */
    int32_t precond;                   /* offset 12: 0 block-Jacobi (rule 4), 1 the odometry chain (T1 - T5) */
    int32_t kind;                      /* offset 16: 0 NONE, 1 DCS, 2 GM */
    int32_t reserved;                  /* offset 20: 0 */
    double lambda0;                    /* offset 24: >= 0, the first attempt's lambda */
    double up;                         /* offset 32: > 1 */
    double down;                       /* offset 40: in (0, 1] */
    double lambda_min;                 /* offset 48: >= 0 */
    double lambda_max;                 /* offset 56: >= lambda_min */
    double tol;                        /* offset 64: >= 0, rule 7 */
    double ftol;                       /* offset 72: >= 0, rule R3 */
    double phi;                        /* offset 80: > 0; not read for kind NONE */
} slamhip_pg_lm_spec;                  /* 88 bytes */
typedef struct slamhip_pg_lm_iter {
    double F, F_trial, lambda, rz0, rz;    /* offsets 0, 8, 16, 24, 32 */
    int32_t cg_iters, stopped, accepted;   /* offsets 40, 44, 48; stopped as slamhip_pg_iter's */
    int32_t reserved[3];                   /* offset 52: 0 */
} slamhip_pg_lm_iter;                  /* 64 bytes */
/* Rules R1 - R4 from the poses as they stand in device memory; calls of this, slamhip_hs_pg_relax and _relax_tri may follow one another
 * on one graph.  robust: E bytes or NULL (R1).  out_iters: room for n_outer records; *out_n: how many were written; *out_F_final: F at
 * the final poses; out_f: E doubles, f_e at the final poses, or NULL.  Launches per attempt: k26_weigh (a lane per edge: R1 at the
 * poses, w_eff into a second weight array) and k19_linearise -- neither behind a rejected attempt --, then the launches of
 * slamhip_hs_pg_relax (precond = 1: of _relax_tri) as they are, reading w_eff, up to but without k19_update; k26_trial (a lane per node),
 * k26_weigh at the trial poses (the cost alone), k26_decide (ONE workgroup: both sums, the comparison, the record, the accept word) and
 * k26_commit (a lane per node).  The host reads the accept word once per attempt and forms the next lambda by R2.  Its own block (32
 * bytes per edge and 24 per node) is made by the first call, grown with the graph and freed by slamhip_hs_pg_clear / _destroy; with
 * precond = 1 the levels' blocks are made as slamhip_hs_pg_relax_tri makes them; after SLAMHIP_ERR_NOMEM the graph is as it was.
 * Blocking, on the operator's stream, with the context's bounded wait.  SLAMHIP_ERR_INVALID, nothing launched and nothing written: a
 * spec outside the ranges above, a value that is not finite, reserved != 0.  SLAMHIP_ERR_STATE: no graph. */
int32_t slamhip_hs_pg_relax_lm(slamhip_hs *hs, const slamhip_pg_lm_spec *spec, const uint8_t *robust, slamhip_pg_lm_iter *out_iters,
                               int32_t *out_n, double *out_F_final, double *out_f);
/* Test hook (no device involved), from the header text the kernels run (hs_pg_lm.h, hs_pg.h, hs_pg_tri.h) in plain loops: the graph
 * arguments and refusals of slamhip_debug_pg_relax, poses relaxed IN PLACE, then the tail and the refusals of slamhip_hs_pg_relax_lm. */
int32_t slamhip_debug_pg_relax_lm(double *poses, const uint8_t *fixed, int32_t N, const int32_t *ij, const double *z, const double *w,
                                  int32_t E, const slamhip_pg_lm_spec *spec, const uint8_t *robust, slamhip_pg_lm_iter *out_iters,
                                  int32_t *out_n, double *out_F_final, double *out_f);

/* Marginal covariances of the pose graph (K27; no reference counterpart).  The relaxation moves the keyframes; this call says how well
 * they are known: blocks of Sigma = H^-1 at the poses as they stand, H rule 5's operator (lambda included) over the weights of
 * slamhip_hs_pg_set.  A column of Sigma is one more solve, H x = e, by the PCG of slamhip_hs_pg_relax / _relax_tri -- here for ALL the
 * right-hand sides of a query at once: the preconditioner is made once, and every PCG phase is ONE launch over the whole batch, each
 * right-hand side with its own scalars and its own stop word.
 * THE DEFINITION.  Binary64 + - * / only, one rounding per operation, no fused multiply-add, as in slamhip_hs_pg_relax.
 *  M1. Query.  pairs = P x 2 int32 (n, m), P in [1, 2^20], both indices in [0, N); duplicates and n == m are allowed.  The COLUMNS are
 *      the distinct m that are free nodes, in ascending node index: m_0 < m_1 < .. < m_{C-1}, C <= SLAMHIP_PG_MARG_MAX_COLS.
 *      Right-hand side 3 c + b (b = 0, 1, 2) is e(m_c, b): 1.0 at component b of node m_c and +0 elsewhere.  R = 3 C.
 *  M2. Per right-hand side: rules 3 - 7 of slamhip_hs_pg_relax, rule 7's start replaced by x = 0, res = e.  precond = 0: z = M res
 *      (rule 4); precond = 1: z = T^-1 res (T1 - T5), T factored ONCE per call.  lambda, tol, n_cg and check_every as in
 *      slamhip_pg_spec.  Rule 6's tree runs over the N nodes of that one right-hand side.  Every right-hand side stops by rule 7 on
 *      its own scalars; one that has stopped is not touched again.  No pose is updated.
 *  M3. Output.  out_blocks[p][a][b] = component a of node n_p of the x solved for e(m_p, b): P x 9 doubles; the block is +0 when n_p
 *      or m_p is fixed.  The blocks are the RAW PCG columns: Sigma[n][m] and the transpose of Sigma[m][n] agree to the solve's accuracy
 *      only, and a diagonal block is symmetric to that accuracy only.
 *  M4. Record per right-hand side, in M1's order, slamhip_pg_marg_col: rz0, the last rz, cg_iters, stopped (as slamhip_pg_iter's),
 *      node = m_c, comp = b.  *out_n_cols = R; out_cols has room for 3 * min(P, SLAMHIP_PG_MARG_MAX_COLS) records.
 *  M5. Memory.  The right-hand sides are solved in chunks of R_c = min(R, floor(budget / B)), budget = max_bytes, or 256 MiB for
 *      max_bytes = 0 (a default, not a measurement), and
 *        B = 120 N + 16 ceil(N / 256) + 40 + (precond ? 24 (tot - N) + 24 : 0),   tot = N + ceil(N / 2) + ceil(N / 4) + .. + 1
 *      the bytes of one right-hand side (five node vectors, two rows of block sums, the scalars and the stop word; the levels'
 *      right-hand sides of T4).  The query itself (12 P + 4 C bytes), the blocks and the records stand beside that.  R_c = 0:
 *      SLAMHIP_ERR_NOMEM, nothing changed.  slamhip_pg_marg_info says what was done: n_cols = C, n_rhs = R, rhs_per_chunk = R_c,
 *      n_chunks = ceil(R / R_c), group = the right-hand sides a lane keeps in registers.  With C = 0 every block is +0, nothing is
 *      launched, and rhs_per_chunk = n_chunks = 0.
 * No result depends on the chunking, the group, the grid, check_every or SLAMHIP_K22_TAIL. */
#define SLAMHIP_PG_MARG_MAX_PAIRS (1 << 20)
#define SLAMHIP_PG_MARG_MAX_COLS 4096
typedef struct slamhip_pg_marg_spec {
    int32_t n_cg;                      /* offset 0: the most PCG iterations of a right-hand side, [1, 2^20] */
    int32_t check_every;               /* offset 4: >= 1, as slamhip_pg_spec's; no result depends on it */
    int32_t precond;                   /* offset 8: 0 block-Jacobi (rule 4), 1 the odometry chain (T1 - T5) */
    int32_t reserved;                  /* offset 12: 0 */
    double lambda;                     /* offset 16: >= 0, added to every diagonal entry of H */
    double tol;                        /* offset 24: >= 0, rule 7 */
    int64_t max_bytes;                 /* offset 32: >= 0, M5; 0: 256 MiB */
} slamhip_pg_marg_spec;                /* 40 bytes */
typedef struct slamhip_pg_marg_col {
    double rz0, rz;                    /* offsets 0, 8 */
    int32_t cg_iters, stopped;         /* offsets 16, 20; stopped as slamhip_pg_iter's */
    int32_t node, comp;                /* offsets 24, 28: the right-hand side is e(node, comp) */
} slamhip_pg_marg_col;                 /* 32 bytes */
typedef struct slamhip_pg_marg_info {
    int32_t n_cols, n_rhs, rhs_per_chunk, n_chunks, group;   /* offsets 0 .. 16 */
    int32_t reserved[3];                                     /* offset 20: 0 */
} slamhip_pg_marg_info;                /* 32 bytes */
/* Rules M1 - M5 on the graph of slamhip_hs_pg_set at the poses as they stand.  It changes neither the poses nor anything a later
 * slamhip_hs_pg_relax* call reads.  Launches: k19_linearise; k19_diag (precond = 1: k22_diag, k22_coupling, k22_reduce, k22_factor_tail)
 * ONCE; per chunk k27_begin (e, x = 0; precond = 0: the first z, p and the block sums) -- precond = 1: the batched solve below --,
 * k27_begin_state (a workgroup per right-hand side: rz0, the scalars, the stop word); per PCG iteration k27_apply<G> (grid: node blocks x
 * ceil(R_c / G); a lane per node with G right-hand sides in registers; an incident edge's record and Jacobians are loaded and formed
 * once for the G), k27_step<G> and k27_dir<G> (every workgroup finishes rule 6's tree of its G scalars itself), with precond = 1 between
 * them k27_forward per large level, k27_solve_tail (a workgroup per right-hand side) and k27_backward per large level, the right-hand
 * side on grid y; per chunk k27_collect (the records and the blocks).  The host enqueues check_every iterations (at most 1024), reads the
 * chunk's stop words in ONE copy, and goes on until all are set.  No floating-point atomic; no workgroup waits on another.
 * SLAMHIP_K27_GROUP (developer, read at every call) selects G among the default 1 and 4 (at the sizes measured G = 4 does not beat G = 1:
 * DESIGN.md section 4 "K27").  The unit's work block is made by the first
 * call, grown as needed and freed by slamhip_hs_pg_clear / _destroy; a caller that never asks allocates nothing.  Blocking, on the
 * operator's stream, with the context's bounded wait.  SLAMHIP_ERR_INVALID, nothing launched and nothing written: a spec outside the
 * ranges above, a value that is not finite, reserved != 0, P or an index out of range, C above the cap.  SLAMHIP_ERR_STATE: no graph. */
int32_t slamhip_hs_pg_marginals(slamhip_hs *hs, const slamhip_pg_marg_spec *spec, const int32_t *pairs, int32_t P, double *out_blocks,
                                slamhip_pg_marg_col *out_cols, int32_t *out_n_cols, slamhip_pg_marg_info *out_info);
/* Test hook (no device involved), from the header text the kernels run (hs_pg.h, hs_pg_tri.h, hs_pg_marg.h) in plain loops, its PCG the
 * one of slamhip_debug_pg_relax: the graph arguments and refusals of slamhip_debug_pg_relax (the poses are not written), then the tail
 * and the refusals of slamhip_hs_pg_marginals.  info.group is what the device call would report. */
int32_t slamhip_debug_pg_marginals(const double *poses, const uint8_t *fixed, int32_t N, const int32_t *ij, const double *z, const double *w,
                                   int32_t E, const slamhip_pg_marg_spec *spec, const int32_t *pairs, int32_t P, double *out_blocks,
                                   slamhip_pg_marg_col *out_cols, int32_t *out_n_cols, slamhip_pg_marg_info *out_info);

/* MapRepMultiMap.UpdateByScan ->OccGridMap.UpdateByScan on every level (MapRepMultiMap.cs:73-77;
 * OccGridMap.cs:114-239), all levels in one launch sequence. */
int32_t slamhip_hs_update_by_scan(slamhip_hs *hs, const float robot_pose_world[3]);

/* The map drawn again from stored scans at poses given per scan (K20; no reference counterpart).  K18 finds loop candidates, K7
 * verifies one, K19 spreads the error over the keyframe poses; the pyramid still holds every scan at the pose it was first drawn at.
 * This unit keeps the keyframes' SCANS on the device and draws a range of them into the pyramid at corrected poses in one call.
 * slamhip_hs_update_by_scan and the processor's per-scan call never enter it.
 * THE DEFINITION.  slamhip_hs_render(hs, first, last, poses, flags) draws scans first .. last - 1 of the scan store; poses holds
 * 3 * (last - first) floats in the window's frame, the frame slamhip_hs_update_by_scan takes.  Afterwards curr_update_index and
 * curr_cache_index of every level, and on every level each cell's update_index, the bits of its value and every probability, equal
 * bit for bit what this sequence leaves:
 *  1. Unless flags & SLAMHIP_RENDER_KEEP: every cell of every level becomes LogOddsCell.Reset() {-1, 0.0f} with probability 0.5f; each
 *     level's update index and cache epoch take the values slamhip_hs_reset gives them (0, 0); the backing directory is dropped as
 *     slamhip_hs_reset drops it (the setting and the pool stay, the tiles go: a tile drawn at the old poses must not scroll back in).
 *     NOT touched: the scan store, the signature store, the pose graph, the window's origin, the factors, the iterations and the
 *     handle's current scan -- which is why this is not slamhip_hs_reset.
 *  2. For k = first .. last - 1 in order: slamhip_hs_set_scan(points_k, n_k, origin_k), then slamhip_hs_update_by_scan(pose_k).  A
 *     stored scan of 0 points still advances the update index by 3 and the epoch by 1.
 *  3. With KEEP the start state is whatever the pyramid holds.  The kernel applies the reference's literal tests update_index <
 *     mark_free and update_index < mark_occ (OccGridMap.cs:192-218): they hold for cells uploaded with indices above the marks, and
 *     for INT_MAX, as they hold in slamhip_hs_update_by_scan.
 *  4. The per-(scan, level) matrices are formed on the host exactly as slamhip_hs_update_by_scan forms them: rotation(theta) *
 *     translation(x, y) * scale(ScaleToMap) in binary32, in that order (OccGridMap.cs:120-123).
 *  5. first == last without KEEP clears (rule 1 alone); with KEEP it returns SLAMHIP_OK and launches nothing.
 *  6. Blocking: on the operator's stream behind everything already enqueued, with the context's bounded wait, no timing class.  A
 *     range is drawn in launches of at most 16384 scans (SLAMHIP_K20_CHUNK in the environment changes that; each later launch is a KEEP
 *     render of its own), and the call waits for EACH launch with the bound: the bound (default 10 s) is per 16384 scans, not per
 *     call.  A launch's time goes with the scans that reach its busiest tile; at the measured 22 us per scan (DESIGN.md section 4 "K20") 16384
 *     scans of 1080 points on one spot take about 0.36 s, far below the default bound, and a render of 2^20 scans is 64 such waits: in the worst case
 *     the call blocks for 64 times the bound before it fails with SLAMHIP_ERR_TIMEOUT.  Scans of many
 *     times 1080 points on one spot can pass it: raise the bound (slamhip_ctx_set_wait_timeout) or lower the chunk.
 *  7. SLAMHIP_ERR_INVALID with nothing changed: first < 0, last < first, last > count, flags with other bits, a pose component that is
 *     not finite, curr_update_index + 3 * (last - first) past INT_MAX on any level (0 stands for curr_update_index without KEEP), the
 *     reference's cache on (slamhip_hs_set_reference_cache), as slamhip_hs_shift refuses.  SLAMHIP_ERR_NOMEM / SLAMHIP_ERR_HIP from an
 *     allocation, a copy or a launch that did not reach the stream: the map, the indices and the directory are as they were before
 *     the launch of the chunk that failed (earlier chunks of a long range stay drawn, with their indices).  SLAMHIP_ERR_TIMEOUT
 *     poisons the context as everywhere; the map is then undefined.
 * THE SCAN STORE.  The points of all scans live in ONE device pool that grows by doubling, the front copied as it is; a record per
 * scan (on the host) holds the offset, the count and the origin.  slamhip_hs_destroy frees it; slamhip_hs_reset empties it and keeps
 * its allocation, as it does the signature store, so the indices of the two stores stay aligned; window shifts do not touch it.
 *  8. slamhip_hs_scans_add appends a scan and gives its index; xy == NULL appends the scan that is set on the handle (n_points and
 *     scan_origin are not read).  The point limits of slamhip_hs_set_scan; at most 2^20 scans (SLAMHIP_ERR_INVALID beyond).
 *  9. _scans_count: the scans held (0 without a store).  _scans_info: one scan's point count and origin.  _scans_download: one scan's
 *     points into room for `cap` points (SLAMHIP_ERR_INVALID: k outside the store, cap below the count).  _scans_clear frees the store. */
#define SLAMHIP_RENDER_KEEP 1
int32_t slamhip_hs_scans_add(slamhip_hs *hs, const float *xy, int32_t n_points, const float scan_origin[2], int32_t *out_index);
int32_t slamhip_hs_scans_count(slamhip_hs *hs, int32_t *out_count);
int32_t slamhip_hs_scans_info(slamhip_hs *hs, int32_t k, int32_t *out_n, float out_origin[2]);
int32_t slamhip_hs_scans_download(slamhip_hs *hs, int32_t k, float *out_xy, int32_t cap);
int32_t slamhip_hs_scans_clear(slamhip_hs *hs);
int32_t slamhip_hs_render(slamhip_hs *hs, int32_t first, int32_t last, const float *poses, int32_t flags);
/* Test hooks (no device involved).  _render: the definition over the caller's arrays, line by line as the reference walks
 * (UpdateLineBresenhami, Bresenham2D step by step -- not the closed form the kernel clips by), from the header text the kernels run
 * (hs_render.h).  dims: (w, h) per level; cell_length: level 0's, doubled per level as slamhip_hs_create doubles it; cells: all
 * levels' cells one behind the other, IN and OUT; update_index, cache_index: per level, IN and OUT; the factors as
 * slamhip_hs_set_factors takes them; xy: all scans' points, offsets: N + 1 entries, origins: N x 2, poses: N x 3.  Rule 7's refusals for
 * the poses, the flags and the indices.  _render_clip: for a line of major length da and minor length db, the steps i of [0, da]
 * whose cell (i, (da / 2 + i * db) / da) lies in the window of T x T offsets whose first is (a0[k], b0[k]) -- [out_i0[k], out_i1[k]],
 * empty when out_i0[k] > out_i1[k]; the interval the tile kernel walks. */
int32_t slamhip_debug_render(int32_t n_levels, const int32_t *dims, float cell_length, slamhip_cell *cells, int32_t *update_index,
                             int32_t *cache_index, float free_factor, float occ_factor, const float *xy, const int32_t *offsets,
                             const float *origins, const float *poses, int32_t N, int32_t flags);
int32_t slamhip_debug_render_clip(int32_t da, int32_t db, int32_t T, int32_t n, const int32_t *a0, const int32_t *b0, int32_t *out_i0,
                                  int32_t *out_i1);

/* The stored scans drawn into the WHOLE world behind the scrolling window (K25; no reference counterpart).  slamhip_hs_render draws
 * into the window only: a line whose begin or end cell lies outside the window's w x h is dropped, and without SLAMHIP_RENDER_KEEP the
 * backing directory goes.  For a robot whose map is larger than its window -- what slamhip_hs_set_backing and the world calls exist
 * for -- that loses the map outside the window when a loop is closed.  This call draws the same scans into the window AND the tiles.
 * THE DEFINITION.  The world of level l is an unbounded grid of cells in the window's frame at the time of the call: window cell
 * (x, y) is world cell ((ox >> l) + x, (oy >> l) + y), as in slamhip_hs_set_backing.  poses: 3 * (last - first) floats in the window's
 * frame, as slamhip_hs_render takes them.  Afterwards every world cell's update_index, the bits of its value and its probability, and
 * every level's curr_update_index and curr_cache_index, equal bit for bit what slamhip_hs_render would leave in a single pyramid
 * large enough to hold every line: the window's clipping disappears, nothing else about the arithmetic changes.
 *  1. Matrices: slamhip_hs_render's rule 4.  Lines: the arithmetic of slamhip_hs_render's lines (rintf, which is right for negative
 *     coordinates too), the inside test against w, h replaced by the WORLD BOUND: begin and end cells within +-2^20 cells of window
 *     cell (0, 0) on each axis.  For scans first .. last - 1 in order every world cell takes the two transitions with K20's marks; the
 *     indices advance as in slamhip_hs_render's rule 2 (a scan of 0 points: + 3 and + 1).
 *  2. Where the cells live.  A world cell inside the window is read from and written to the window's arrays (the window wins, as in
 *     the world download and upload); a cell outside it is read from and written to its tile's slot, cells followed by probabilities.
 *     The part of a tile under the window is neither read nor written.
 *  3. Without SLAMHIP_RENDER_KEEP: the window is cleared as in slamhip_hs_render's rule 1 and the directory is dropped; the world is
 *     then drawn into the window and into freshly taken tiles.  With it: the start state is the window plus the existing tiles; a
 *     tile that does not exist starts as Reset cells.  first == last: without KEEP the clear alone, with KEEP nothing.
 *  4. Slots.  A first device pass gives, per (scan, level), the box of the begin cell and the valid end cells and the largest line;
 *     the host reads the boxes back BEFORE anything is changed.  A slot is taken for every tile not wholly under the window that a
 *     box meets on its level and that does not exist yet, in the order (level, ty, tx) ascending: the outcome is deterministic.  A
 *     tile that ends all-Reset KEEPS its slot -- slamhip_hs_backing_stats.tiles counts it (the boxes bound the lines, they are not the
 *     lines).  evicted_cells, restored_cells and dropped_cells do not move.
 *  5. SLAMHIP_ERR_INVALID with nothing changed: slamhip_hs_render's rule 7 list; backing off (slamhip_hs_render is the call for a
 *     window alone); a begin or end cell beyond the world bound -- the begin cell of a scan of 0 points is not asked, a point that
 *     is not finite ends beyond it; a valid line of more than 32767 cells on any level (the integer clip of a line to a block is
 *     proven in 32 bits up to there).
 *  6. SLAMHIP_ERR_NOMEM with nothing changed, the directory, the pool and the stats included: the tiles to take do not fit max_bytes,
 *     or a chunk's allocation fails.  Unlike slamhip_hs_shift, which never fails for capacity and drops cells: a silently partial
 *     world after a loop closure is worse than a refusal.  Everything is planned and allocated before the directory is dropped.
 *  7. Blocking, on the operator's stream, the context's bounded wait, no timing class; chunks as slamhip_hs_render's rule 6
 *     (SLAMHIP_K20_CHUNK), the wait per chunk and once more per chunk for the boxes' pass.  An error behind the plan leaves what
 *     slamhip_hs_render's rule 7 says of a failed chunk.
 * The hook (no device involved): the definition over the caller's arrays.  rects: per level (x0, y0, w, h) in window-frame cells,
 * w * h <= 2^26; cells: the rectangles' cells one level behind the other, IN and OUT; the other arguments as slamhip_debug_render.  It
 * walks every line step by step as slamhip_debug_render does, under the world bound, and refuses (SLAMHIP_ERR_INVALID, the arrays
 * untouched) what rule 5 refuses and a scan whose box leaves its level's rectangle.  With x0 = y0 = 0 and every line inside the
 * rectangle it equals slamhip_debug_render bit for bit. */
int32_t slamhip_hs_render_world(slamhip_hs *hs, int32_t first, int32_t last, const float *poses, int32_t flags);
int32_t slamhip_debug_render_world(int32_t n_levels, const int32_t *rects, float cell_length, slamhip_cell *cells, int32_t *update_index,
                                   int32_t *cache_index, float free_factor, float occ_factor, const float *xy, const int32_t *offsets,
                                   const float *origins, const float *poses, int32_t N, int32_t flags);

/* Stored scans matched pairwise (K21; no reference counterpart).  K18 names loop CANDIDATES between keyframes, K19 spreads a loop's
 * error over the keyframe poses and asks per edge for a measurement z -- node j seen in node i's frame -- and a weight w; K20 keeps
 * the keyframes' scans in a device pool.  This unit matches scan against scan for a whole list of (reference, query) pairs of that
 * pool in ONE call, by a correlative search over a small pose lattice round a guess per pair, and returns per pair the best node, an
 * integer score and integer moments of the near-optimal nodes; a host rule turns those into (z, w).  The map takes no part: it is
 * the drifted one a loop is meant to correct.  slamhip_hs_update_by_scan and the processor's per-scan call never enter the unit.
 * THE DEFINITION.  Everything behind the few binary32 operations that place a point in a cell is an integer, so no order of atomics
 * or reductions changes a bit.  H = spec->half; a pair is (ref, query, guess), the guess being the QUERY's pose in the REFERENCE's
 * frame -- K19's direction with ref = edge end i and query = end j.  A scan's stored origin plays no part.
 *  1. Reference raster, 2H x 2H cells.  For a stored point (px, py) of scan `ref`: fx = px * scale, fy = py * scale, one binary32
 *     multiply each.  A point with a NaN or with |f| >= 2^14 on either axis is IGNORED (K18's rule 2).  Its cell is (floor(fx) + H,
 *     floor(fy) + H); a cell outside [0, 2H)^2 marks nothing.  hit(x, y): some point has that cell.  near(x, y): some cell of the
 *     3 x 3 block round (x, y), clipped to the grid, is hit.  val = 2 if hit, else 1 if near, else 0; outside the grid val = 0.
 *     n_ref = the points that were not ignored (inside the grid or not).
 *  2. Query cells: K7's arithmetic to the letter (slamhip_lattice_spec) with ScaleToMap = scale.  theta_k = guess[2] + (float)k *
 *     dtheta for k in [-nt, nt]; (s, c) = sh_det_sincosf(theta_k); cxm = guess[0] * scale, cym = guess[1] * scale; per query point
 *     rx = c * qx - s * qy, ry = s * qx + c * qy; fx = rx * scale + cxm, fy = ry * scale + cym, every operation rounded on its own.
 *     The point is IGNORED for this heading unless |fx| < 2^24 and |fy| < 2^24 (a NaN fails).  gx = (int)floorf(fx) + H, gy likewise.
 *  3. score(k, iy, ix) = the sum of val(gx + ix, gy + iy) over the points used, an int32; ix in [-nx, nx], iy in [-ny, ny].
 *     flat = ((k + nt) * (2 ny + 1) + (iy + ny)) * (2 nx + 1) + (ix + nx).  The best node has the highest score, ties to the lowest
 *     flat: the largest packed key (score ^ 0x80000000) << 32 | (0xFFFFFFFF - flat), K7's form.  n_query = the points used at the
 *     best node's heading, so score <= 2 * n_query.
 *  4. Moments.  b = the best score.  N = the nodes with score >= b - margin and score > 0.  cnt = |N|; nine int64 sums over N:
 *     ix, iy, k, ix^2, iy^2, k^2, ix * iy, ix * k, iy * k.  If b == 0: cnt = 0, the sums are 0 and the pair is INVALID (the best
 *     node is then flat 0: k = -nt, iy = -ny, ix = -nx).
 *  5. The result: slamhip_scanmatch_result below, 104 bytes, no padding.
 *  6. Edge rule (slamhip_hs_scans_edges), host code in binary64, one rounding per operation, no fused multiply-add:
 *       zx = ((double)cxm + (double)ix) / (double)scale,  zy = ((double)cym + (double)iy) / (double)scale  (cxm, cym: rule 2's binary32
 *       values),  zt = (double)theta_k  (rule 2's binary32 value).
 *     Per axis a with sums S1 = sum a, S2 = sum a^2 and n = (double)cnt:  m = (double)S1 / n;  q = (double)S2 / n;  v = q - (m * m);
 *     v = 0 unless v > 0;  u2 = u * u;  variance = (v * u2) + (u2 / 12.0);  w_a = 1.0 / variance.  u = 1.0 / (double)scale for x
 *     and y -- the near-optimal nodes' spread plus the variance of a uniform error over one cell.  For the heading u =
 *     |(double)dtheta|, EXCEPT when nt == 0 or dtheta == 0: then the lattice says nothing about the heading and u = 6.283185307179586
 *     / 64.0, K18's sector, the resolution of the candidate's shift the guess came from.  With scale and dtheta binary32 values and
 *     |a| <= 64 no u2 underflows and no variance overflows in binary64: every weight of a valid pair is finite and > 0, as
 *     slamhip_hs_pg_set demands.  valid = cnt > 0; an invalid pair gets its best node's z, w = (0, 0, 0) and valid = 0, and must
 *     not become an edge.  The three cross sums are delivered and not used: K19 takes diagonal weights.
 *  7. SLAMHIP_ERR_INVALID, nothing launched and nothing written: scale not finite or <= 0; half no multiple of 16 in [16, 192]; nx,
 *     ny or nt outside [0, 64]; dtheta not finite; margin < 0; reserved != 0; n_pairs outside [1, 4096]; more than 2^20 nodes per
 *     pair or 2^26 in the call; a guess component that is not finite; a scan index outside the store.  SLAMHIP_ERR_STATE: no scan
 *     store, or an empty one (tested behind the spec, the count and the guesses, ahead of the indices).
 * Blocking, with the context's bounded wait, on the operator's stream behind everything already enqueued; the pairs go out and the
 * results come back through pinned staging the unit owns (freed by slamhip_hs_destroy).  Two launches of one kernel: the first
 * leaves every pair's best key, the second -- which forms the scores again rather than keep a volume of up to 2^26 of them -- the
 * moments and n_query.  A workgroup of 256 lanes owns (pair, block of headings): it builds the reference raster in LDS (2 bits per
 * cell, 36 KB at H = 192; LDS atomic OR, then the dilation behind a barrier), stages a heading's query cells in chunks of 1024, and
 * a lane walks the points for one translation at a time.  The map, the signature store, the pose graph and the scan that is set
 * are neither read nor written. */
typedef struct slamhip_scanmatch_spec {
    float scale;                       /* offset 0: cells per metre, finite and > 0; the caller's choice, unrelated to any map level */
    int32_t half;                      /* offset 4: H, a multiple of 16 in [16, 192] */
    int32_t nx, ny;                    /* offsets 8, 12: each in [0, 64] */
    int32_t nt;                        /* offset 16: in [0, 64] */
    float dtheta;                      /* offset 20: finite */
    int32_t margin;                    /* offset 24: >= 0 */
    int32_t reserved;                  /* offset 28: 0 */
} slamhip_scanmatch_spec;              /* 32 bytes */
typedef struct slamhip_scan_pair {
    int32_t ref, query;                /* offsets 0, 4: indices into the scan store */
    float guess[3];                    /* offset 8: the query's pose in the reference's frame */
} slamhip_scan_pair;                   /* 20 bytes */
typedef struct slamhip_scanmatch_result {
    int32_t k, ix, iy, score;          /* offsets 0, 4, 8, 12: the best node and its score */
    int32_t n_ref, n_query, cnt;       /* offsets 16, 20, 24 */
    int32_t reserved;                  /* offset 28: 0 */
    int64_t sum_x, sum_y, sum_k;       /* offsets 32, 40, 48: sums over N of ix, iy, k */
    int64_t sum_xx, sum_yy, sum_kk;    /* offsets 56, 64, 72 */
    int64_t sum_xy, sum_xk, sum_yk;    /* offsets 80, 88, 96 */
} slamhip_scanmatch_result;            /* 104 bytes */
int32_t slamhip_hs_scans_match(slamhip_hs *hs, const slamhip_scanmatch_spec *spec, const slamhip_scan_pair *pairs, int32_t n_pairs,
                               slamhip_scanmatch_result *out_results);
/* Rule 6 for n results: out_z and out_w n x 3 doubles, out_valid n int32.  Touches no device.  SLAMHIP_ERR_INVALID, nothing written:
 * rule 7's refusals for the spec, n and the guesses; a result whose node lies outside the lattice. */
int32_t slamhip_hs_scans_edges(const slamhip_scanmatch_spec *spec, const slamhip_scan_pair *pairs, const slamhip_scanmatch_result *results,
                               int32_t n, double *out_z, double *out_w, int32_t *out_valid);
/* Test hook (no device involved): rules 1 - 5 over the caller's arrays in plain loops, from the header text the kernels run
 * (hs_scanmatch.h).  xy: all scans' points; offsets: N + 1 entries, the first 0, ascending; the scan store is those N scans (N = 0:
 * SLAMHIP_ERR_STATE).  Rule 7's refusals, nothing written. */
int32_t slamhip_debug_scans_match(const float *xy, const int32_t *offsets, int32_t N, const slamhip_scanmatch_spec *spec,
                                  const slamhip_scan_pair *pairs, int32_t n_pairs, slamhip_scanmatch_result *out_results);

/* The consistent set of loop edges (K23; no reference counterpart).  K18 names loop candidates, K21 matches them and gives (z, w),
 * K19 / K22 relax the graph, K20 draws the map again; a scan-to-scan score cannot see perceptual aliasing -- two similar corridors
 * score as well as a true revisit -- and ONE such edge bends the whole relaxed map.  This unit is pairwise consistency maximisation:
 * two loop edges are consistent if the cycle they form with the odometry chain closes within its uncertainty, and the largest
 * mutually consistent set found by a greedy search from several starts is kept.  slamhip_hs_update_by_scan and the processor's
 * per-scan call never enter it, and it reads and writes no state of the hs but its own buffers.
 * THE DEFINITION.  All floating-point arithmetic is binary64 + - * / and rint, ONE rounding per operation (no fused multiply-add),
 * in the order the parentheses give; everything behind the one comparison d2 <= gamma is an integer.  Inputs: poses = N x 3 doubles
 * (x, y, theta), the keyframe chain as it stands, node order = odometry order; L edges (ij, z, w) as slamhip_hs_pg_set takes them
 * (z: node j seen in node i's frame; w: diagonal weights); `use`, a byte per edge (NULL: every edge is used); the spec below.
 *  1. Per edge a = (i, j, z, w), with p_i, p_j its nodes' poses:  (sI, cI) = sh_det_sincos(p_i.theta) (rule 2 of slamhip_hs_pg_relax);
 *       Wx = p_i.x + (cI * z.x - sI * z.y);   Wy = p_i.y + (sI * z.x + cI * z.y);   Wtheta = p_i.theta + z.theta
 *     -- where the edge puts node j;  (sW, cW) = sh_det_sincos(Wtheta);  (sJ, cJ) = sh_det_sincos(p_j.theta);
 *       vt = 0.5 * (1 / w.x + 1 / w.y);   vtheta = 1 / w.theta.
 *  2. Per pair a < b.  The odometry from j_a to j_b, in j_a's frame:
 *       dx = p_jb.x - p_ja.x;   dy = p_jb.y - p_ja.y;   ux = cJ_a * dx + sJ_a * dy;   uy = cJ_a * dy - sJ_a * dx;   utheta = p_jb.theta - p_ja.theta.
 *     Node j_b through edge a and that odometry:
 *       Tx = Wx_a + (cW_a * ux - sW_a * uy);   Ty = Wy_a + (sW_a * ux + cW_a * uy);   Ttheta = Wtheta_a + utheta.
 *     The residual against edge b:
 *       ex = Tx - Wx_b;   ey = Ty - Wy_b;   etheta = wrap(Ttheta - Wtheta_b)      (wrap: rule 2 of slamhip_hs_pg_relax).
 *     The variances, with s = (double)(|j_a - j_b| + |i_a - i_b|) -- the odometry steps the cycle holds -- and rho2 = ux * ux + uy * uy:
 *       Vt = ((vt_a + vt_b) + s * q_t) + vtheta_a * rho2;   Vtheta = (vtheta_a + vtheta_b) + s * q_theta.
 *     The test:  d2 = (ex * ex + ey * ey) / Vt + (etheta * etheta) / Vtheta;   bit (a, b) = bit (b, a) = use[a] && use[b] && d2 <= gamma.
 *     A NaN fails (0 / 0 with every variance 0 included).  The diagonal is 0.  This is the isotropic, diagonal-weight approximation
 *     of the cycle's covariance: the translational variance is one number (the mean of the two axes, the lever arm rho of a's
 *     heading error added), no cross terms -- enough for K19's diagonal w.  The translational term being isotropic, the result does
 *     not depend on the frame of `poses` beyond rounding.
 *  3. Degrees.  adj[v] = row v of the matrix as bits; deg(v) = popcount(adj[v]).
 *  4. Starts.  The R = min(n_starts, used edges) USED edges of highest degree, ties to the lower index: start rank 0, 1, .. R - 1.
 *  5. Greedy set from start v0.  Q = {v0}, S = adj[v0].  While S is not empty: g(v) = popcount(adj[v] & S) for v in S; take the v of
 *     highest g, ties to the lower index; Q += v; S &= adj[v].  Q is a clique and it is maximal (not necessarily a maximum one).
 *  6. Result.  The largest Q wins, ties to the lower start rank.  keep[a] = 1 for the edges of the winner if its size >= min_clique,
 *     else keep is all 0 -- the size is reported all the same.  Outputs: keep = L bytes; deg = L int32; slamhip_loops_info below;
 *     and with SLAMHIP_LOOPS_ADJ in flags the matrix, L x ceil(L / 64) uint64 row-major, bit (a, b) = bit (b & 63) of word
 *     a * ceil(L / 64) + (b >> 6), the bits past L zero.  Without a used edge R = 0: size 0, start and rank -1.
 *  7. SLAMHIP_ERR_INVALID, nothing launched and nothing written: L outside [1, 4096]; N outside [1, 2^20]; an edge end outside [0, N)
 *     (i == j is allowed); a pose, z or w that is not finite; |theta| of a pose or of a z above 32768 (Wtheta stays inside
 *     sh_det_sincos's contract); a weight <= 0; gamma, q_t or q_theta not finite or < 0; n_starts outside [1, 64]; min_clique < 1;
 *     flags with other bits; reserved != 0; SLAMHIP_LOOPS_ADJ without out_adj.  There is no SLAMHIP_ERR_STATE: the unit keeps nothing
 *     between calls except its buffers.
 * Nothing depends on the grid or the launch shape.  slamhip_hs_loops_consistent blocks, with the context's bounded wait, on the
 * operator's stream behind everything already enqueued; the host gathers the two poses of every edge, and edges and results pass
 * through pinned staging the unit owns (freed by slamhip_hs_loops_clear and slamhip_hs_destroy; slamhip_hs_reset leaves them alone).
 * Launches: k23_edges (a lane per edge, rule 1), k23_pairs (a lane owns a column b, 64 row records in LDS read as broadcasts, a row's
 * word is the wavefront's ballot: one 64-bit store per word, no atomics), k23_degree (one workgroup: rule 3, rule 4's ranking by the
 * packed key (deg << 32) | (0xFFFFFFFF - v)), k23_clique (a workgroup per start: S in LDS, the matrix too where its rows fit in 144 KB
 * -- L <= 1084 -- else read from global memory; rule 5's arg-max by the same packed key), k23_finish (rule 6). */
#define SLAMHIP_LOOPS_MAX_EDGES 4096
#define SLAMHIP_LOOPS_MAX_STARTS 64
#define SLAMHIP_LOOPS_ADJ 1
typedef struct slamhip_loops_spec {
    double gamma;                      /* offset 0: finite, >= 0; d2 has 3 degrees of freedom (11.34 is chi-square's 99 %) */
    double q_t, q_theta;               /* offsets 8, 16: finite, >= 0; variance one odometry step adds, translation (m^2) and heading (rad^2) */
    int32_t n_starts;                  /* offset 24: [1, 64] */
    int32_t min_clique;                /* offset 28: >= 1 */
    int32_t flags;                     /* offset 32: 0 or SLAMHIP_LOOPS_ADJ */
    int32_t reserved;                  /* offset 36: 0 */
} slamhip_loops_spec;                  /* 40 bytes */
typedef struct slamhip_loops_info {
    int64_t n_pairs;                   /* offset 0: consistent pairs a < b */
    int32_t n_used;                    /* offset 8: edges with a non-zero use byte */
    int32_t size;                      /* offset 12: |Q| of the winner (0 without a used edge) */
    int32_t start;                     /* offset 16: the winner's start edge, -1 without one */
    int32_t rank;                      /* offset 20: its start rank, -1 without one */
    int32_t n_starts;                  /* offset 24: R */
    int32_t reserved;                  /* offset 28: 0 */
} slamhip_loops_info;                  /* 32 bytes */
int32_t slamhip_hs_loops_consistent(slamhip_hs *hs, const double *poses, int32_t N, const int32_t *ij, const double *z, const double *w,
                                    const uint8_t *use, int32_t L, const slamhip_loops_spec *spec, uint8_t *out_keep, int32_t *out_deg,
                                    slamhip_loops_info *out_info, uint64_t *out_adj);
/* Free the unit's buffers.  Never fails for an hs that has none. */
int32_t slamhip_hs_loops_clear(slamhip_hs *hs);
/* Test hook (no device involved): rules 1 - 6 over the caller's arrays in plain loops, from the header text the kernels run
 * (hs_loops.h); rule 7's refusals, nothing written.  out_adj is written whenever it is given.  out_d2 (optional): L x L doubles,
 * rule 2's d2 of the pair (min, max) at [a][b] and [b][a] whatever `use` says, 0 on the diagonal. */
int32_t slamhip_debug_loops_consistent(const double *poses, int32_t N, const int32_t *ij, const double *z, const double *w,
                                       const uint8_t *use, int32_t L, const slamhip_loops_spec *spec, uint8_t *out_keep, int32_t *out_deg,
                                       slamhip_loops_info *out_info, uint64_t *out_adj, double *out_d2);

/* The scrolling window -- something the reference lacks (its `offset`, GridMap.cs:45, is ignored by UpdateByScan,
 * OccGridMap.cs:120-123, and by the matcher, ScanMatcher.cs:139-142): the contents of the whole pyramid move by an integer
 * number of cells, on the device, in stream order, so that a robot that drives out of the window can take the window along.
 * dx, dy are level-0 cells and the window moves by (+dx, +dy): on level l, new cell (x, y) holds what old cell
 * (x + (dx >> l), y + (dy >> l)) held.  dx and dy must each be a multiple of g = 1 << (levels - 1), so that every level
 * moves by a whole number of cells (the arithmetic shift is then exact).  A new cell whose source lies outside its level becomes
 * LogOddsCell.Reset() -- Value 0.0f, UpdateIndex -1 (LogOddsCell.cs:38-42) -- with probability 0.5f; a move by a level's width
 * or height or more clears that level.  The probabilities move with the cells; update indices and the cache epoch do not
 * change.
 * The origin (ox, oy) is the sum of all shifts since slamhip_hs_create or the last slamhip_hs_reset (which sets it to 0: an
 * empty map has no frame to keep), in level-0 cells; host-side bookkeeping only.  THE CONTRACT: a world point p lies at
 * p - origin * cell_length(level 0) in the frame that slamhip_hs_match*, slamhip_hs_hessian, slamhip_hs_update_by_scan and
 * the match reports use -- those calls go on working in the window's frame, with the transforms they always had; the caller
 * (or slamhip_hsproc_set_scroll) subtracts the offset from hints and poses going in and adds it to poses coming out.
 * Enqueue-only on the operator's stream: it runs behind every grid update and match already enqueued and ahead of whatever
 * is enqueued later; no host wait.  One launch moves all levels, cells and probabilities, and writes the exposed bands.
 * The first shift allocates a second set of arrays, 12 bytes per cell and level (63 MiB at 2048^2 x 3 levels): the launch reads
 * one set and writes the other, and the two swap roles.  If that allocation fails: SLAMHIP_ERR_NOMEM, nothing changed.
 * dx == dy == 0: SLAMHIP_OK, no launch.  SLAMHIP_ERR_INVALID, maps and origin unchanged: dx or dy not a multiple of g; the
 * reference's cache is on (slamhip_hs_set_reference_cache) -- its literal stale entries have no meaning under an operation
 * the reference lacks.  A poisoned context: SLAMHIP_ERR_TIMEOUT. */
int32_t slamhip_hs_shift(slamhip_hs *hs, int32_t dx, int32_t dy);
int32_t slamhip_hs_origin(slamhip_hs *hs, int64_t *ox, int64_t *oy);

/* The backing store of the scrolling window (opt-in): what scrolls out of the window is kept in device memory and restored when the
 * window returns, so that a robot that drives a loop comes home to the map it made.  The world is cut into tiles of
 * tile_cells x tile_cells cells per level (world cell of window cell (x, y) on level l: ((ox >> l) + x, (oy >> l) + y)).  A tile
 * that holds evicted cells occupies a SLOT of a device pool: tile^2 slamhip_cell records followed by tile^2 float probabilities,
 * 12 * tile^2 bytes -- the probabilities are stored, not recomputed: they move with the cells, as in the shift itself.  The
 * directory (which tiles exist, in which slot) lives on the host, which knows the origin and every shift: the shift stays
 * enqueue-only and reads nothing back.  Slots are allocated lazily, in chunks, up to max_bytes, and start as Reset cells
 * ({-1, 0.0f}, 0.5f): restoring a part of a tile that nothing was evicted into gives exactly what the shift writes without
 * backing.
 * With backing on, slamhip_hs_shift enqueues its launch as before and ONE more behind it (none if the shift has nothing to evict
 * or restore), which copies the departing cells of the old window into their tiles and the tiles' cells into the exposed bands of
 * the new window; a launch that initialises a new chunk of slots goes ahead of it when one is allocated.  A shift NEVER fails
 * for capacity: if a departing piece needs a new tile and no slot can be had (the pool is at max_bytes, or the device allocation
 * of a chunk fails), the cells of that piece are dropped, as all of them are without backing, and counted in dropped_cells.
 * Slots are dealt in the planner's job order (slamhip_debug_backing_plan), so what is kept is deterministic.  A tile keeps its
 * copy after a restore; it is overwritten when those cells leave the window again.
 * slamhip_hs_set_backing: max_bytes == 0 (the default state): off -- every tile is dropped and the pool is freed (the call drains
 * the operator's stream first); tile_cells is then ignored.  Otherwise tile_cells must be a power of two in [8, 256] and
 * max_bytes at least one slot, 12 * tile_cells^2; anything else SLAMHIP_ERR_INVALID, the setting unchanged.  While tiles exist,
 * changing tile_cells, or lowering max_bytes below what the pool already holds, is SLAMHIP_ERR_INVALID: switch backing off first.
 * The setting survives slamhip_hs_reset; the tiles do not (the directory is dropped, the pool is kept and re-initialised).
 * slamhip_hs_cells_upload touches the window only.  slamhip_hs_destroy frees the pool.  With backing off nothing is allocated,
 * no extra launch is issued and nothing is read that is not read without this call.  While the reference's cache is on
 * (slamhip_hs_set_reference_cache) slamhip_hs_shift refuses as before, with or without backing.
 * slamhip_hs_backing_stats: tiles in the directory, bytes of the pool allocated so far, capacity_bytes = max_bytes, and the cells
 * evicted, restored and dropped since backing was switched on -- host-side sums of job areas, no device read-back; all zero
 * while backing is off. */
typedef struct slamhip_backing_stats {
    int64_t tiles, bytes, capacity_bytes;
    int64_t evicted_cells, restored_cells, dropped_cells;   /* host-side sums of job areas; no device read-back */
    int32_t tile, on;
} slamhip_backing_stats;
int32_t slamhip_hs_set_backing(slamhip_hs *hs, int32_t tile_cells, uint64_t max_bytes);
int32_t slamhip_hs_backing_stats(slamhip_hs *hs, slamhip_backing_stats *out);
/* The map of everywhere the window has been: the rectangle [x0, x0 + w) x [y0, y0 + h) of level `level` in WORLD cells, row-major
 * into out[w * h].  Cells inside the window come from the window (the window wins over a tile's older copy), evicted cells from
 * their tiles, everything else is LogOddsCell.Reset() {-1, 0.0f}.  Blocking, behind everything already on the operator's stream,
 * with the context's bounded wait.  w, h >= 1 and w * h <= 2^26 cells (512 MiB of out); anything else SLAMHIP_ERR_INVALID.  Works
 * with backing off as well: the window in a frame of Reset cells. */
int32_t slamhip_hs_world_cells_download(slamhip_hs *hs, int32_t level, int64_t x0, int64_t y0,
                                        int32_t w, int32_t h, slamhip_cell *out);
/* The inverse of the world download: load a saved world back.  cells[w * h], row-major, is the rectangle
 * [x0, x0 + w) x [y0, y0 + h) of level `level` in WORLD cells.
 * OVERWRITE: every cell of the rectangle replaces what the world holds at that place.  A cell that lies in the window (level
 * origin (win_ox >> level, win_oy >> level)) goes into the window's cells, and its probability -- formed on the device by the
 * function every writer of the cells uses, so the matcher reads the bits it reads after slamhip_hs_cells_upload -- into the
 * window's probabilities.  The part of a tile that lies under the window is NOT written: the window wins, as it does in the
 * download, and the tile's copy there is overwritten when those cells next leave the window.
 * Outside the window with backing on, the cells go into their tiles' slots, cells followed by probabilities.  If a tile does not
 * exist, a slot is taken as a shift takes one (lazy chunks, max_bytes, initialised on the stream before first use) -- but only if
 * the piece of the rectangle that falls into that tile (outside the window) holds at least one cell that is not
 * LogOddsCell.Reset() {-1, 0.0f}, compared as bits: an all-Reset piece takes no slot, so a sparse world loads sparse.  An all-Reset
 * piece over an EXISTING tile is written (overwrite).  Slots are dealt in the planner's job order (slamhip_debug_world_plan), so
 * what is kept is deterministic.
 * An upload never fails for capacity: if no slot can be had (the pool is at max_bytes, or the device allocation of a chunk fails),
 * the non-Reset cells of that piece are dropped and counted into dropped_cells of slamhip_hs_backing_stats and into *out_dropped,
 * and the call still returns SLAMHIP_OK; evicted_cells and restored_cells do not move.  With backing off the window part is
 * written, every non-Reset cell outside it is counted in *out_dropped, and nothing is allocated for tiles.  out_dropped may be NULL.
 * The level's update index follows the rule of slamhip_hs_cells_upload: with mx the largest update_index in cells[], it becomes at
 * least (mx / 3 + 1) * 3, so that the next scan's marks exceed every stored index -- a map resumed from a saved world writes the
 * marks the original writes.  The cache epoch, the reference's cache and the origin are left as they are.
 * Blocking, behind everything already on the operator's stream, with the context's bounded wait.  The caller's array reaches the
 * device through a staging buffer the library owns (kept for the next call); ONE launch scatters it.  w, h >= 1 and
 * w * h <= 2^26 cells, |x0|, |y0| < 2^60; anything else SLAMHIP_ERR_INVALID, nothing changed.  A poisoned context:
 * SLAMHIP_ERR_TIMEOUT. */
int32_t slamhip_hs_world_cells_upload(slamhip_hs *hs, int32_t level, int64_t x0, int64_t y0,
                                      int32_t w, int32_t h, const slamhip_cell *cells, int64_t *out_dropped);
/* The extents of the world: extends = {xMax, yMax, xMin, yMin} in WORLD cells of level `level`, over the cells whose Value != 0.0f
 * (a NaN counts, as in GridMap.GetMapExtends, GridMap.cs:161) in the window and in every tile of that level, EXCLUDING the part of
 * a tile that lies under the window (those copies are stale: the window wins) -- the rectangle a host downloads to save the
 * world.  If there is no such cell: *found = 0 and extends is zeroed; the reference's quirk of minima that start at 10000
 * (slamhip_hs_map_extends) does not apply here: the results are 64-bit and any cell counts.  Reduced on the device in ONE launch
 * over the window and the tiles.  Blocking, with the context's bounded wait.  Works with backing off: the window only. */
int32_t slamhip_hs_world_extends(slamhip_hs *hs, int32_t level, int64_t extends[4], int32_t *found);

/* ------------------------------------------------------------------------------------------------
 * HectorSLAM, processor level
 * ---------------------------------------------------------------------------------------------- */
/* new HectorSLAMProcessor(mapResolution, mapSize, startPose, numDepth, numThreads) (Main/HectorSLAMProcessor.cs:66-77) */
int32_t slamhip_hsproc_create(slamhip_ctx *ctx, float map_resolution, int32_t width, int32_t height,
                              const float start_pose[3], int32_t num_depth, slamhip_hsproc **out);
int32_t slamhip_hsproc_destroy(slamhip_hsproc *p);
int32_t slamhip_hsproc_reset(slamhip_hsproc *p);                                        /* :131-138 */
/* Update(scan, poseHintWorld, mapWithoutMatching) (:86-126); *out_map_updated = return value.  The match is waited
 * for (its pose gates the update); the grid update is enqueued and the call returns -- later calls that touch the
 * pyramid are ordered behind it on the operator's stream; UpdateTiming (:115) then reports the enqueue.
 * SLAMHIP_HS_WAIT_UPDATE=1 waits for the update.  While consecutive scans keep updating the map, the update is enqueued
 * behind the match BEFORE the pose is back: the kernel reads the matched pose from device memory and applies the test of
 * :107-109 itself (the same float operations the host then applies to the pose it receives); SLAMHIP_HS_NO_GATED_UPDATE=1
 * keeps the decision on the host. */
int32_t slamhip_hsproc_update(slamhip_hsproc *p, const float *xy, int32_t n_points, const float scan_origin[2],
                              const float pose_hint_world[3], int32_t map_without_matching,
                              int32_t *out_map_updated);
int32_t slamhip_hsproc_get(slamhip_hsproc *p, float match_pose[3], float last_map_update_pose[3],
                           float *match_timing_ms, float *update_timing_ms);            /* :31-46 */
/* on = 1: the match of every later slamhip_hsproc_update produces its report in the same launch (slamhip_hs_match_report);
 * the gated grid update, the launch-ahead order and what Update returns do not change.  on = 0 (default): Update launches what
 * it launches without this call.  Any other value: SLAMHIP_ERR_INVALID, the setting unchanged. */
int32_t slamhip_hsproc_set_match_report(slamhip_hsproc *p, int32_t on);
/* The report of the last slamhip_hsproc_update's match (:93); *out_valid = 0 and *out zeroed before the first match, after
 * slamhip_hsproc_reset, after an Update with mapWithoutMatching (:100) and while reports are off (switching them off drops the
 * last report). */
/* The report's pose_map stays in the WINDOW's frame (slamhip_hsproc_set_scroll, slamhip_hs_shift): map coordinates of the device's
 * level, as the match saw them. */
int32_t slamhip_hsproc_get_report(slamhip_hsproc *p, slamhip_match_report *out, int32_t *out_valid);
/* Keep the robot in the window (slamhip_hs_shift).  trigger_cells = 0 (default): off -- Update issues exactly the launches it
 * issues without this call.  trigger_cells > 0: at the end of every slamhip_hsproc_update -- the match pose on the host, this
 * scan's grid update enqueued -- with (lx, ly) the match pose in the window's frame, in binary32: cx = (int)floorf(lx * stm0),
 * cy likewise (stm0 = 1 / cell_length of level 0); per axis, if |cx - w0 / 2| > trigger_cells then q = ((cx - w0 / 2) / g) * g
 * (C integer division, toward zero; g = 1 << (levels - 1)), else q = 0; if either q is non-zero, slamhip_hs_shift(qx, qy),
 * enqueued behind the update.  Poses cross this interface in the WORLD frame whatever the window did: the hint of
 * slamhip_hsproc_update is taken as hint - (float)origin * cell0, and slamhip_hsproc_get returns the stored window-frame
 * poses + (float)origin * cell0 (float.MinValue, "never updated", absorbs both).  Valid: 0 <= trigger_cells <
 * min(w0, h0) / 2 - g; anything else SLAMHIP_ERR_INVALID, the setting unchanged.  The setting survives slamhip_hsproc_reset;
 * the origin returns to 0 there (slamhip_hs_reset).  slamhip_hsproc_get_origin: slamhip_hs_origin of the processor's own hs. */
int32_t slamhip_hsproc_set_scroll(slamhip_hsproc *p, int32_t trigger_cells);
int32_t slamhip_hsproc_get_origin(slamhip_hsproc *p, int64_t *ox, int64_t *oy);
/* slamhip_hs_shift(dx, dy) of the processor's own hs from outside an Update (resuming from a saved world: the window goes to the
 * saved origin), with the processor's MatchPose and LastMapUpdatePose -- kept in the window's frame -- re-based as the scroll
 * re-bases them, so that slamhip_hsproc_get goes on answering in the world frame.  Arguments and errors as slamhip_hs_shift. */
int32_t slamhip_hsproc_shift(slamhip_hsproc *p, int32_t dx, int32_t dy);
/* Relocalise the processor (no reference counterpart): slamhip_hs_set_scan on the processor's own hs, then slamhip_hs_relocalise
 * with spec_world->centre taken to the window's frame as slamhip_hsproc_update takes its hint (- (float)origin * cell0) and the
 * result brought back as slamhip_hsproc_get does (+ (float)origin * cell0).  adopt = 1: the result becomes both MatchPose and
 * LastMapUpdatePose -- the next Update matches from the found pose and the map is not written until the robot has moved by the
 * thresholds (a relocalisation must not immediately draw into the map); adopt = 0: the processor's state is untouched; any other
 * value SLAMHIP_ERR_INVALID.  No scroll is issued.  The search covers the window (slamhip_hs_lattice_search);
 * slamhip_hsproc_relocalise_world searches the world and moves the window. */
int32_t slamhip_hsproc_relocalise(slamhip_hsproc *p, const float *xy, int32_t n_points, const float scan_origin[2],
                                  const slamhip_lattice_spec *spec_world, int32_t B, int32_t adopt, float out_pose_world[3],
                                  slamhip_match_report *out_report, slamhip_reloc_info *out_info);
/* slamhip_hsproc_relocalise over the whole world: slamhip_hs_set_scan, then slamhip_hs_relocalise_world with spec_world->centre
 * taken to the window's frame (- (float)origin * cell0, the origin BEFORE the call).  The processor's MatchPose and
 * LastMapUpdatePose are re-based by the shift as slamhip_hsproc_shift re-bases them, whether or not adopt is set, so that
 * slamhip_hsproc_get goes on answering in the world frame; with adopt = 1 both then become the result.  out_pose_world is the
 * result + (float)origin * cell0 with the origin AFTER the call.  Errors as slamhip_hs_relocalise_world; adopt outside {0, 1}:
 * SLAMHIP_ERR_INVALID. */
int32_t slamhip_hsproc_relocalise_world(slamhip_hsproc *p, const float *xy, int32_t n_points, const float scan_origin[2],
                                        const slamhip_lattice_spec *spec_world, int32_t B, int32_t adopt,
                                        float out_pose_world[3], slamhip_match_report *out_report,
                                        slamhip_world_reloc_info *out_info);
/* slamhip_hsproc_relocalise (spec_world->world = 0: out_info is a slamhip_reloc_info) or slamhip_hsproc_relocalise_world (world = 1:
 * a slamhip_world_reloc_info) with the branch-and-bound search (slamhip_hs_relocalise_bnb) in place of the exhaustive one: frame
 * conversion, the re-basing of the stored poses and adopt exactly as in those two calls.  out_bnb: the search's info. */
int32_t slamhip_hsproc_relocalise_bnb(slamhip_hsproc *p, const float *xy, int32_t n_points, const float scan_origin[2],
                                      const slamhip_bnb_spec *spec_world, int32_t B, int32_t adopt, float out_pose_world[3],
                                      slamhip_match_report *out_report, void *out_info, slamhip_bnb_info *out_bnb);
/* The beam trace through the processor: slamhip_hs_set_scan on the processor's own hs, then slamhip_hs_trace at the B poses of
 * poses_world (B x 3, WORLD frame), each taken to the window's frame as slamhip_hsproc_relocalise takes its centre
 * (- (float)origin * cell0 per axis; the bits themselves while the origin is 0).  hx, hy stay in window-frame cells of the level:
 * slamhip_hsproc_get_origin converts them (world cell = (origin >> level) + cell).  The processor's stored poses, its update gate
 * and its match report are not touched; the scan that was set is replaced, as every call that takes a scan replaces it.
 * Errors as slamhip_hs_trace; a call refused for its level, B, world or the 2^20 records leaves the scan that was set (the world's
 * rectangle is known only once the trace plans it, behind the new scan). */
int32_t slamhip_hsproc_trace(slamhip_hsproc *p, const float *xy, int32_t n_points, const float scan_origin[2],
                             const float *poses_world, int32_t B, int32_t level, int32_t world,
                             slamhip_trace_summary *out_summaries, slamhip_trace_beam *out_beams);
/* The end-point distance score through the processor: slamhip_hs_set_scan on the processor's own hs, then
 * slamhip_hs_distance_score at the B poses of poses_world (B x 3, WORLD frame), each taken to the window's frame as
 * slamhip_hsproc_trace takes them (- (float)origin * cell0 per axis; the bits themselves while the origin is 0).  The processor's
 * stored poses, its update gate and its match report are not touched; the scan that was set is replaced.  Errors as
 * slamhip_hs_distance_score; a call refused for its level, world, site_mask, radius, B or the 2^22 records leaves the scan that was
 * set (E's size is known only once the field is planned, behind the new scan). */
int32_t slamhip_hsproc_distance_score(slamhip_hsproc *p, const float *xy, int32_t n_points, const float scan_origin[2],
                                      const float *poses_world, int32_t B, int32_t level, int32_t world, int32_t site_mask,
                                      int32_t radius, slamhip_distance_summary *out_summaries, uint16_t *out_points);
/* The frontier clusters through the processor: slamhip_hs_frontiers on the processor's own hs with every cell field in WORLD cells
 * of the level.  (lx, ly) is taken as a world cell; (origin >> level) per axis is added to the seeds, the boxes and mx0 / my0, and
 * n_cells * (origin >> level) to the sums; labels are flat indices into M and need no conversion.  No scan is needed; the
 * processor's stored poses, its update gate and the scan that was set are not touched.  Errors as slamhip_hs_frontiers. */
int32_t slamhip_hsproc_frontiers(slamhip_hsproc *p, int32_t level, int32_t world, int32_t min_cells, int32_t max_clusters,
                                 slamhip_frontier_summary *out_summary, slamhip_frontier_cluster *out_clusters,
                                 int32_t lx, int32_t ly, int32_t lw, int32_t lh, int32_t *out_labels);
/* The cost-to-go field through the processor: slamhip_hs_nav_field on the processor's own hs with every cell in WORLD cells of
 * spec->level.  Sources, goals and (rx, ry) are taken as world cells ((origin >> level) per axis is subtracted); the same is added to
 * bx / by of every goal with a reached cell, to the path cells and to mx0 / my0.  No scan is needed; the processor's stored poses,
 * its update gate and the scan that was set are not touched.  Errors as slamhip_hs_nav_field. */
int32_t slamhip_hsproc_nav_field(slamhip_hsproc *p, const slamhip_nav_spec *spec, const int32_t *sources, int32_t S, const int32_t *goals,
                                 int32_t G, slamhip_nav_goal_result *out_goal_results, int32_t n_paths, int32_t max_path_cells,
                                 slamhip_nav_path *out_paths, int32_t *out_path_cells, int32_t rx, int32_t ry, int32_t rw, int32_t rh,
                                 uint32_t *out_cost, uint8_t *out_dir, slamhip_nav_summary *out_summary);
/* The command rollouts through the processor: slamhip_hs_rollouts on the processor's own hs in WORLD cells and the WORLD pose.
 * sources are world cells of the level; start_pose_world is a world pose, or NULL for MatchPose.  The pose is taken to the window's
 * frame as slamhip_hsproc_trace takes its poses (minus (float)origin * cell0 per axis) and the results' poses taken back by the same
 * offset; nav.mx0 / nav.my0 are re-based by (origin >> level) as slamhip_hsproc_nav_field re-bases them.  With the origin at (0, 0)
 * every bit passes through.  No scan is needed; MatchPose, LastMapUpdatePose and the update gate are untouched.  Errors as
 * slamhip_hs_rollouts. */
int32_t slamhip_hsproc_rollouts(slamhip_hsproc *p, const slamhip_nav_spec *spec, const int32_t *sources, int32_t S,
                                const float *start_pose_world, float dt, const float *body, int32_t P, const float *cmds, int32_t B,
                                int32_t n_cmd, int32_t hold, slamhip_rollout_result *out_results, slamhip_rollout_summary *out_summary);
/* The localisation step through the processor: slamhip_hs_set_scan on the processor's own hs as slamhip_hsproc_relocalise sets it,
 * then slamhip_hs_mcl_step with the spec as given -- the particles live in the window's frame, and a caller whose window has scrolled
 * since the last step passes that movement in frame_offset.  MatchPose, LastMapUpdatePose, the update gate and the map are untouched;
 * the scan that was set is replaced.  Errors as slamhip_hs_mcl_step; a call refused for its spec or n_points leaves the scan that
 * was set. */
int32_t slamhip_hsproc_mcl_step(slamhip_hsproc *p, const float *xy, int32_t n_points, const float scan_origin[2],
                                const slamhip_mcl_spec *spec, slamhip_mcl_summary *out);
/* The merge through the processor.  _set_source: slamhip_hs_merge_set_source on the processor's own hs, the arguments as given (the
 * source's frame is its own).  _score and _apply: the poses are WORLD poses of the source frame's origin, taken to the window's frame
 * as slamhip_hsproc_trace takes its poses (minus (float)origin * cell0 per axis; with the origin at (0, 0) every bit passes through).
 * MatchPose, LastMapUpdatePose and the update gate are untouched.  Errors as the slamhip_hs_merge_* calls. */
int32_t slamhip_hsproc_merge_set_source(slamhip_hsproc *p, int32_t level, int32_t ax, int32_t ay, int32_t w, int32_t h,
                                        const slamhip_cell *cells);
int32_t slamhip_hsproc_merge_score(slamhip_hsproc *p, const float *poses_world, int32_t B, slamhip_merge_report *out_reports);
int32_t slamhip_hsproc_merge_apply(slamhip_hsproc *p, const float pose_world[3], int32_t rule, float value_limit,
                                   slamhip_merge_report *out_report);
/* The view gain through the processor: slamhip_hs_set_scan on the processor's own hs, then slamhip_hs_view_gain / _view_select at
 * B WORLD poses, taken to the window's frame as slamhip_hsproc_trace takes its poses (minus (float)origin * cell0 per axis; with the
 * origin at (0, 0) every bit passes through).  The covered layer is the hs's own (slamhip_hsproc_hs).  MatchPose, LastMapUpdatePose,
 * the update gate and the map are untouched; the scan that was set is replaced.  Errors as the slamhip_hs_view_* calls; a call
 * refused for its arguments alone leaves the scan that was set. */
int32_t slamhip_hsproc_view_gain(slamhip_hsproc *p, const float *xy, int32_t n_points, const float scan_origin[2],
                                 const float *poses_world, int32_t B, int32_t level, int32_t reach, int32_t commit,
                                 slamhip_view_summary *out_summaries);
int32_t slamhip_hsproc_view_select(slamhip_hsproc *p, const float *xy, int32_t n_points, const float scan_origin[2],
                                   const float *poses_world, int32_t B, int32_t level, int32_t reach, int32_t mode, int32_t min_gain,
                                   int32_t k, int32_t *out_order, int32_t *out_gain, int32_t *out_n);
/* The scan-to-map pairs through the processor: slamhip_hs_set_scan on the processor's own hs, then slamhip_hs_nearest_pairs at the B
 * poses of poses_world (B x 3, WORLD frame), each taken to the window's frame as slamhip_hsproc_trace takes them (- (float)origin *
 * cell0 per axis; the bits themselves while the origin is 0).  The summaries' cell sums stay in window-frame cells of the level.
 * The processor's stored poses, its update gate and its match report are not touched; the scan that was set is replaced.  Errors as
 * slamhip_hs_nearest_pairs; a call refused for its level, world, site_mask, radius, B or the 2^22 records leaves the scan that was
 * set (E's size is known only once the field is planned, behind the new scan). */
int32_t slamhip_hsproc_nearest_pairs(slamhip_hsproc *p, const float *xy, int32_t n_points, const float scan_origin[2],
                                     const float *poses_world, int32_t B, int32_t level, int32_t world, int32_t site_mask,
                                     int32_t radius, slamhip_pair_summary *out_summaries, int16_t *out_pairs);
/* The Hough transform through the processor: slamhip_hs_hough, _hough_rotation and _hough_shifts on the processor's own hs, the
 * arguments as given (cells and bins have no world pose to convert; out_info's x0, y0 stay window-frame cells).  The processor's
 * stored poses, its update gate, its match report and the scan that was set are not touched.  Errors as the slamhip_hs_hough* calls. */
int32_t slamhip_hsproc_hough(slamhip_hsproc *p, int32_t level, int32_t slot, int32_t world, int32_t site_mask, int32_t T, int32_t q,
                             int32_t out_info[7], uint64_t *out_spectrum, uint32_t *out_H);
int32_t slamhip_hsproc_hough_rotation(slamhip_hsproc *p, uint64_t *out_cc);
int32_t slamhip_hsproc_hough_shifts(slamhip_hsproc *p, const int32_t *pairs, int32_t P, slamhip_hough_shift *out_shifts, uint64_t *out_xc);
/* The scan signatures through the processor: the scan set as slamhip_hsproc_relocalise sets it, then slamhip_hs_sig_add /
 * _sig_query on the processor's own hs; slamhip_hs_sig_self as it is.  pose_world is stored as given (the library never reads it), so
 * keyframes keep their WORLD poses when the window moves.  What the hs call refuses for the spec's absence, B, the range or a full
 * store is refused ahead of the scan: such a call leaves the scan that was set.  The processor's stored poses, its update gate and
 * its match report are not touched.  The store is configured, read and cleared through slamhip_hsproc_hs. */
int32_t slamhip_hsproc_sig_add(slamhip_hsproc *p, const float *xy, int32_t n_points, const float scan_origin[2], const float pose_world[3],
                               int32_t *out_index, uint64_t *out_sig, slamhip_sig_info *out_info);
int32_t slamhip_hsproc_sig_query(slamhip_hsproc *p, const float *xy, int32_t n_points, const float scan_origin[2], int32_t first, int32_t last,
                                 int32_t B, slamhip_sig_hit *out_hits, int32_t *out_n, uint64_t *out_sig, slamhip_sig_info *out_info);
int32_t slamhip_hsproc_sig_self(slamhip_hsproc *p, int32_t first, int32_t last, int32_t min_gap, slamhip_sig_hit *out_hits);
/* The scan store and the render through the processor.  _scans_add appends the scan that is set on the processor's hs -- the one the
 * last slamhip_hsproc_update, _sig_add or any other call that takes a scan left -- as slamhip_hs_scans_add with xy == NULL.  _render:
 * slamhip_hs_render at WORLD poses, each taken to the window's frame as slamhip_hsproc_trace takes its poses (minus (float)origin *
 * cell0 per axis; with the origin at (0, 0) every bit passes through).  MatchPose, LastMapUpdatePose and the update gate are left
 * alone.  Errors as the slamhip_hs_* calls. */
int32_t slamhip_hsproc_scans_add(slamhip_hsproc *p, int32_t *out_index);
int32_t slamhip_hsproc_render(slamhip_hsproc *p, int32_t first, int32_t last, const float *poses_world, int32_t flags);
/* slamhip_hs_render_world at WORLD poses, taken to the window's frame exactly as slamhip_hsproc_render takes them.  MatchPose,
 * LastMapUpdatePose and the update gate are left alone. */
int32_t slamhip_hsproc_render_world(slamhip_hsproc *p, int32_t first, int32_t last, const float *poses_world, int32_t flags);
/* The scan-to-scan match through the processor: slamhip_hs_scans_match on the processor's own hs, the arguments as given -- a guess
 * and a result are RELATIVE poses and need no frame conversion.  The processor's stored poses, its update gate, its match report and
 * the scan that was set are not touched. */
int32_t slamhip_hsproc_scans_match(slamhip_hsproc *p, const slamhip_scanmatch_spec *spec, const slamhip_scan_pair *pairs, int32_t n_pairs,
                                   slamhip_scanmatch_result *out_results);
/* MinDistanceDiffForMapUpdate :51, MinAngleDiffForMapUpdate :56 */
int32_t slamhip_hsproc_set_thresholds(slamhip_hsproc *p, float min_distance_diff, float min_angle_diff);
int32_t slamhip_hsproc_hs(slamhip_hsproc *p, slamhip_hs **out_hs);                       /* MapRep :26 */

/* ------------------------------------------------------------------------------------------------
 * Multi-GPU (new; no reference counterpart: the reference's only parallelism is ParallelWorker threads)
 * ---------------------------------------------------------------------------------------------- */
/* One process, n GPUs: a context + CoreSLAM replica per device and one RCCL communicator. */
int32_t slamhip_group_create(const int32_t *device_ordinals, int32_t n, float physical_map_size,
                             int32_t hole_map_size, int32_t obstacle_map_size, slamhip_group **out);
int32_t slamhip_group_destroy(slamhip_group *g);
int32_t slamhip_group_size(slamhip_group *g, int32_t *out_n);
int32_t slamhip_group_cs(slamhip_group *g, int32_t rank, slamhip_cs **out_cs);
/* broadcast-by-replication helpers: apply the same call to every replica */
int32_t slamhip_group_reset(slamhip_group *g, int32_t unmapped_obstacle_hits);
int32_t slamhip_group_holemap_upload(slamhip_group *g, const uint16_t *pixels, size_t n_pixels);
int32_t slamhip_group_set_scan(slamhip_group *g, const float *xy, int32_t n_points);
int32_t slamhip_group_set_offsets(slamhip_group *g, const float *offs, int32_t n);
/* ... or generated on every GPU of the group (slamhip_cs_generate_offsets: the same list everywhere, keyed by seed, stream and index) */
int32_t slamhip_group_generate_offsets(slamhip_group *g, int32_t n, float sigma_xy, float sigma_theta, uint64_t seed, uint64_t stream);
/* Candidates block-sharded over the GPUs, one ncclAllReduce(min, uint64, count 1) of the packed key
 * over xGMI, winner pose recomputed locally. */
int32_t slamhip_group_search(slamhip_group *g, const float search_pose[3], float out_pose[3],
                             int32_t *out_dist, int32_t *out_index);
/* replicas apply the identical deterministic update (integer-exact kernels keep them bit-identical) */
/* One scan on every GPU of the group in one call (CoreSLAMProcessor.cs:732, :695-705, :750-751): search over the GPU's block,
 * ncclAllReduce(min), the winner decoded on each device, each replica's map updates queued behind -- as
 * slamhip_cs_search_allreduce_and_update, every rank on its own worker thread; returns with key and pose (theta normalised). */
int32_t slamhip_group_search_and_update(slamhip_group *g, const float search_pose[3], float hole_width, int32_t quality,
                                        int32_t max_obstacle_hits, float out_pose[3], int32_t *out_dist, int32_t *out_index);
int32_t slamhip_group_update_maps(slamhip_group *g, const float pose[3], float hole_width, int32_t quality,
                                  int32_t max_obstacle_hits);
/* *out_equal = 1 when slamhip_cs_maps_checksum agrees on every GPU of the group */
int32_t slamhip_group_replicas_equal(slamhip_group *g, int32_t *out_equal);


/* One process per GPU (torch.distributed.run, MPI, ...): this rank's end of an RCCL communicator.  The host framework
 * only carries the 128-byte id from rank 0 to the other ranks; the per-scan exchange -- the cross-thread arg-min of
 * CoreSLAMProcessor.cs:695-705 as ncclAllReduce(min, uint64, count 1) over xGMI -- is issued by the library on the
 * communicator's own stream, behind an event, so that the next search does not wait for the last collective. */
int32_t slamhip_comm_probe(void);                       /* every rank, before anything collective: can librccl be resolved here? */
int32_t slamhip_comm_unique_id(uint8_t out_id[128]);                                  /* rank 0 */
int32_t slamhip_comm_create(slamhip_ctx *ctx, const uint8_t id[128], int32_t rank, int32_t n_ranks, slamhip_comm **out);
int32_t slamhip_comm_destroy(slamhip_comm *comm);
int32_t slamhip_comm_info(slamhip_comm *comm, int32_t *out_rank, int32_t *out_n_ranks);
/* One sharded search step (asynchronous): flat candidates [first, first+count) on this rank; the keys of up to 16 consecutive
 * steps are min-all-reduced in one collective (every rank must issue the same steps and call slamhip_comm_wait at the same
 * places).  *d_out_key (optional) = device address where this step's reduced key will be once the collective of its batch has
 * run -- after slamhip_comm_wait, or behind a later batch on the communicator's stream -- valid for 64 further steps. */
int32_t slamhip_cs_search_allreduce_async(slamhip_cs *cs, slamhip_comm *comm, const float search_pose[3], int32_t first,
                                          int32_t count, uint64_t **d_out_key);
/* Issues the collective for the steps not yet covered by one, waits for every step issued so far; *out_key (optional) = the
 * reduced key of the last one.  (A host that needs every scan's winner before the next scan calls it after every step.) */
int32_t slamhip_comm_wait(slamhip_comm *comm, uint64_t *out_key);
/* Steps per collective of the asynchronous form (1 .. 32; default 16).  Waits for the steps issued so far; every rank calls it
 * at the same place. */
int32_t slamhip_comm_set_batch(slamhip_comm *comm, int32_t steps);
/* One sharded search step, BLOCKING -- the per-scan form: CoreSLAMProcessor.Update needs the winner (CoreSLAMProcessor.cs:732,
 * the arg-min of :695-705) before it updates the maps (:750-751).  K1 over this rank's block, ncclAllReduce(min, uint64, 1)
 * and the hand-over of the reduced key to the host sit on the operator's stream, one behind the other (no second stream, no
 * event).  *out_key = min over all ranks of (distance << 32 | flat index).  Every rank makes the same call. */
int32_t slamhip_cs_search_allreduce(slamhip_cs *cs, slamhip_comm *comm, const float search_pose[3], int32_t first,
                                    int32_t count, uint64_t *out_key);
/* One scan of the SLAM loop on every rank -- search (CoreSLAMProcessor.cs:732), exchange (:695-705 as ncclAllReduce(min, uint64, 1)),
 * both map updates from the winner's pose (:750-751) -- with NO host hop between the exchange and the updates: a one-thread launch
 * decodes the reduced key into the pose on the device (every rank holds the whole jitter list), the replicas' map updates are
 * enqueued behind it, and the call returns when key and pose have reached the host; the updates run on, and everything that touches
 * the maps afterwards is ordered behind them (as slamhip_cs_search_and_update).  out_pose: theta normalised (:746).  Every rank
 * makes the same call; a rank whose own part fails still joins the collective (with the neutral key) and reports afterwards. */
int32_t slamhip_cs_search_allreduce_and_update(slamhip_cs *cs, slamhip_comm *comm, const float search_pose[3], int32_t first,
                                               int32_t count, float hole_width, int32_t quality, int32_t max_obstacle_hits,
                                               float out_pose[3], int32_t *out_dist, int32_t *out_index);
/* Latency of the exchange step alone: `iters` 8-byte min all-reduces back to back; *out_us = device microseconds per
 * collective.  Every rank makes the same call (measurement aid for the scaling curve). */
int32_t slamhip_comm_allreduce_probe(slamhip_comm *comm, int32_t iters, float *out_us);
/* Replica check across the ranks: every rank checksums its maps (slamhip_cs_maps_checksum), one ncclAllReduce(min) and one
 * ncclAllReduce(max) of the two words; *out_equal = 1 when they agree, i.e. every rank holds bit-identical maps.  Every rank
 * makes the same call (a debug / health check: once per so many scans, not per scan). */
int32_t slamhip_comm_replicas_equal(slamhip_cs *cs, slamhip_comm *comm, int32_t *out_equal);

#ifdef __cplusplus
}
#endif
#endif /* SLAMHIP_H */
