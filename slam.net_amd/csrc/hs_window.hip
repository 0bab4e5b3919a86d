// hs_window.hip -- K6, the scrolling map window of HectorSLAM (slamhip_hs_shift), its backing store (slamhip_hs_set_backing) and
// the world behind both: download, upload and extents (slamhip_hs_world_cells_download, _world_cells_upload, _world_extends).
#include "hs_internal.h"
#include "backing_plan.h"
#include "world_plan.h"
#include <vector>
#include <map>
#include <tuple>

// ---- K6: the scrolling window (slamhip_hs_shift) -------------------------------------------------------------------------------
// Something the reference lacks (its `offset`, GridMap.cs:45, is ignored by UpdateByScan and by the matcher): the CONTENTS of every
// level move by a whole number of cells, so that K4 and K5 go on working in the window's frame with the transforms they have.  On
// level l new cell (x, y) holds what old cell (x + sx, y + sy) held, sx = dx >> l; a cell whose source lies outside the level
// becomes LogOddsCell.Reset() (LogOddsCell.cs:38-42) with probability 0.5f -- exp(0) / (exp(0) + 1), what k5_fill_cells and
// k5_refresh_prob give for Value 0.  Not in place (a workgroup would read what another has overwritten): the launch reads one set
// of arrays and writes the other, and the host swaps the pointers behind it -- every launch takes its pointers from hs->lv when it
// is enqueued (levels_arg, hs_update_enqueue's k5_arg, the downloads and reports), none is kept past a call, and the stream orders
// the launches.  ONE launch for all levels, cells and probabilities, exposed bands included.
// Lane mapping: a workgroup owns K6_BLOCK consecutive cells of a level's flat array; a lane moves 16-byte units of the DESTINATION,
// which are always aligned (two cells, four probabilities): one store each, consecutive lanes consecutive units.  A unit that lies
// in one row with all its sources inside the map is one load as wide as the source's alignment allows -- the source index differs
// from the destination's by sy * w + sx, a multiple of 4 on level 0 of a pyramid of three levels or more, of 2 on level 1, of
// anything on the coarsest (which is small); every other unit (a row's end where w is no multiple of the unit, the exposed band,
// the array's tail) goes element by element with the bounds test per element.
#define K6_BLOCK 1024
struct k6_level { int w, h, sx, sy, blk0; const slamhip_cell *src_c; slamhip_cell *dst_c; const float *src_p; float *dst_p; };
struct k6_arg { k6_level lv[HS_MAX_LEVELS]; int n; };

template <typename T, int N>                   // N elements of T are 16 bytes; i: the unit's first element, a multiple of N
__device__ static __forceinline__ void k6_unit(const T *__restrict__ src, T *__restrict__ dst, int w, int h, int sx, int sy, int i, int n, const T fill)
{
    static_assert(sizeof(T) * N == 16, "a unit is 16 bytes");
    if (i >= n) return;
    struct alignas(16) unit { T e[N]; };
    struct alignas(8) half { T e[N / 2]; };
    const int y = i / w, x = i - y * w;
    const int ys = y + sy, xs = x + sx;
    if (i + N <= n && x + N <= w && ys >= 0 && ys < h && xs >= 0 && xs + N <= w) {
        const T *s = src + ((size_t)ys * w + xs);                         // (inside the array: 0 <= ys < h, 0 <= xs, xs + N <= w)
        const unsigned mis = (unsigned)(xs + ys * w) & (N - 1);
        unit v;
        if (mis == 0) v = *(const unit *)s;
        else if (N == 4 && mis == 2) {
            const half a = *(const half *)s, b = *(const half *)(s + N / 2);
#pragma unroll
            for (int k = 0; k < N / 2; k++) { v.e[k] = a.e[k]; v.e[N / 2 + k] = b.e[k]; }
        } else {
#pragma unroll
            for (int k = 0; k < N; k++) v.e[k] = s[k];
        }
        *(unit *)(dst + i) = v;
        return;
    }
#pragma unroll
    for (int k = 0; k < N; k++) {
        const int ik = i + k;
        if (ik >= n) break;
        const int yk = ik / w, xk = ik - yk * w;
        const int yy = yk + sy, xx = xk + sx;
        const bool in = yy >= 0 && yy < h && xx >= 0 && xx < w;
        dst[ik] = in ? src[(size_t)yy * w + xx] : fill;
    }
}

__global__ void __launch_bounds__(256) k6_shift(const k6_arg A)
{
    int lvl = 0;
    for (int l = 1; l < A.n; l++) if ((int)blockIdx.x >= A.lv[l].blk0) lvl = l;
    const k6_level &L = A.lv[lvl];
    const int n = L.w * L.h;                                               // (<= 2^30: slamhip_hs_create bounds w and h by 32768)
    const int base = ((int)blockIdx.x - L.blk0) * K6_BLOCK, t = threadIdx.x;
    const slamhip_cell reset = hs_reset_cell();
    k6_unit<slamhip_cell, 2>(L.src_c, L.dst_c, L.w, L.h, L.sx, L.sy, base + 2 * t, n, reset);
    k6_unit<slamhip_cell, 2>(L.src_c, L.dst_c, L.w, L.h, L.sx, L.sy, base + K6_BLOCK / 2 + 2 * t, n, reset);
    k6_unit<float, 4>(L.src_p, L.dst_p, L.w, L.h, L.sx, L.sy, base + 4 * t, n, HS_RESET_PROB);
}

// ---- K6 page: the backing store of the scrolling window (slamhip_hs_set_backing) -------------------------------------------------
// ONE launch behind k6_shift.  Evict jobs copy pieces of the OLD set of arrays (the `_alt` names after the swap: K6 is not in
// place, so they are intact until the next shift, and the stream orders that) into tile slots; restore jobs copy pieces of tile
// slots into the exposed bands of the NEW set, over the Reset that k6_shift wrote.  The departing and the arriving cells are
// disjoint in world cells but may share a tile, and on the coarse levels dx >> l may be odd: a 16-byte unit (two cells, four
// probabilities) is used only where it lies wholly inside one job's row and is aligned on both sides; everything else goes element
// by element (probabilities also in 8-byte halves where the tile's side is aligned to 8 only) -- no lane touches an element of
// another job, so evict and restore jobs of one tile may run side by side.
// Lane mapping: jobs are thin (g cells by T for the common small shift), so a WORKGROUP owns a job piece -- at most K6P_CELLS cells
// in whole rows of one job, cut on the host -- and its lanes take the piece's 16-byte groups, laid out by the WINDOW side's
// alignment (the wide side: rows of w cells), consecutive lanes consecutive groups of a row, the next row behind the last group.
// The job table is read from a pinned host block (32 bytes per workgroup, the same for all lanes).  A slot: T * T cells, then
// T * T probabilities.
#define K6P_CELLS 2048
struct k6p_job { unsigned char *slot; int32_t wx, wy; uint16_t nx, ny, lx, ly; uint32_t level_kind, pad; };   // level_kind: level * 2 + kind
static_assert(sizeof(k6p_job) == 32, "a job piece is two 16-byte words");
struct k6p_level { int w; const slamhip_cell *old_c; const float *old_p; slamhip_cell *new_c; float *new_p; };
struct k6p_arg { k6p_level lv[HS_MAX_LEVELS]; const k6p_job *jobs; int T; };
// the slot layout, t2 = T * T: where the probabilities start, and the whole slot
__host__ __device__ static inline size_t k6p_slot_prob_offset(size_t t2) { return sizeof(slamhip_cell) * t2; }
__host__ __device__ static inline size_t k6p_slot_bytes(size_t t2) { return k6p_slot_prob_offset(t2) + sizeof(float) * t2; }

template <typename E, int N>                   // N elements of E are 16 bytes
__device__ static __forceinline__ void k6p_rows(E *__restrict__ win, E *__restrict__ tile, const bool evict, const int w, const int T,
                                                const int wx, const int wy, const int nx, const int ny, const int lx, const int ly)
{
    static_assert(sizeof(E) * N == 16, "a unit is 16 bytes");
    struct alignas(16) unit { E e[N]; };
    struct alignas(8) half { E e[N / 2]; };
    const int gpr = (nx + N - 1) / N + 1;                                  // groups per row, a row's misaligned head included
    const int items = gpr * ny;
    for (int i = threadIdx.x; i < items; i += 256) {
        const int r = i / gpr, g = i - r * gpr;
        const size_t a = (size_t)(wy + r) * w + wx;                        // the row's first element in the window's array
        const int b = (ly + r) * T + lx;                                   // ... and in the tile's
        const int e0 = g * N - (int)(a & (N - 1));                        // the group's first element in the row: a + e0 is a multiple of N
        if (e0 >= nx) continue;
        if (e0 >= 0 && e0 + N <= nx && ((b + e0) & (N / 2 - 1 + (N == 2))) == 0) {   // whole, and the tile's side aligned to 8 at least
            E *pw = win + (a + e0), *pt = tile + (b + e0);
            if (((b + e0) & (N - 1)) == 0) {
                if (evict) *(unit *)pt = *(const unit *)pw; else *(unit *)pw = *(const unit *)pt;
            } else {                                                       // (N == 4 only: the tile's side in two halves)
                if (evict) {
                    const unit v = *(const unit *)pw;
                    half lo, hi;
#pragma unroll
                    for (int k = 0; k < N / 2; k++) { lo.e[k] = v.e[k]; hi.e[k] = v.e[N / 2 + k]; }
                    *(half *)pt = lo; *(half *)(pt + N / 2) = hi;
                } else {
                    const half lo = *(const half *)pt, hi = *(const half *)(pt + N / 2);
                    unit v;
#pragma unroll
                    for (int k = 0; k < N / 2; k++) { v.e[k] = lo.e[k]; v.e[N / 2 + k] = hi.e[k]; }
                    *(unit *)pw = v;
                }
            }
            continue;
        }
#pragma unroll
        for (int k = 0; k < N; k++) {
            const int e = e0 + k;
            if (e < 0 || e >= nx) continue;
            if (evict) tile[b + e] = win[a + e]; else win[a + e] = tile[b + e];
        }
    }
}

__global__ void __launch_bounds__(256) k6_page(const k6p_arg A)
{
    const k6p_job J = A.jobs[blockIdx.x];
    const int lvl = (int)(J.level_kind >> 1);
    const bool evict = (J.level_kind & 1u) == SLAMHIP_BACKING_EVICT;
    const k6p_level &L = A.lv[lvl];
    const int T = A.T;
    slamhip_cell *tc = (slamhip_cell *)J.slot;
    float *tp = (float *)(J.slot + k6p_slot_prob_offset((size_t)T * T));
    slamhip_cell *wc = evict ? const_cast<slamhip_cell *>(L.old_c) : L.new_c;
    float *wp = evict ? const_cast<float *>(L.old_p) : L.new_p;
    k6p_rows<slamhip_cell, 2>(wc, tc, evict, L.w, T, J.wx, J.wy, J.nx, J.ny, J.lx, J.ly);
    k6p_rows<float, 4>(wp, tp, evict, L.w, T, J.wx, J.wy, J.nx, J.ny, J.lx, J.ly);
}

// a chunk of new slots: Reset cells and 0.5f (what k5_fill_cells writes), slot by slot in the slot layout
__global__ void __launch_bounds__(256) k6_fill_slots(unsigned char *base, int t2, size_t n)    // n = slots * t2
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const size_t s = i / t2, e = i - s * t2;
        unsigned char *slot = base + s * k6p_slot_bytes(t2);
        ((slamhip_cell *)slot)[e] = hs_reset_cell();
        ((float *)(slot + k6p_slot_prob_offset(t2)))[e] = HS_RESET_PROB;
    }
}

// ---- K6 world put: load a saved world back (slamhip_hs_world_cells_upload) -------------------------------------------------------
// K6's third launch kind, the inverse of the world download: the caller's rectangle, staged in device memory, is scattered into the
// window and into tile slots by ONE launch.  As in k6_page a WORKGROUP owns a job piece -- at most K6P_CELLS cells in whole rows of
// one job of the planner (world_plan.h), cut on the host -- and no lane touches an element of another job.  A lane takes groups of
// four cells laid out by the DESTINATION's alignment (consecutive lanes consecutive groups of a row, a row's misaligned head as a
// group of its own): a whole group is two 16-byte cell stores and one 16-byte store of the four probabilities formed from them
// (hs_prob_v, what k5_refresh_prob writes), its cells read with 16-byte loads where the staged row is aligned as well (the
// rectangle's x0 and width are the caller's: any parity) and with 8-byte loads otherwise; heads and tails go element by element.
// slot == nullptr: the window (rows of w cells); otherwise a tile slot (rows of T cells, probabilities behind the cells).
struct k6w_piece { unsigned char *slot; int32_t sx, sy; uint16_t nx, ny; int32_t lx, ly; uint32_t pad; };
static_assert(sizeof(k6w_piece) == 32, "a job piece is two 16-byte words");
struct k6w_arg { const slamhip_cell *src; const k6w_piece *pieces; slamhip_cell *win_c; float *win_p; int rw, w, T; };
struct alignas(8) k6w_cell1 { slamhip_cell e; };
struct alignas(16) k6w_cell2 { slamhip_cell e[2]; };

__global__ void __launch_bounds__(256) k6_world_put(const k6w_arg A)
{
    const k6w_piece J = A.pieces[blockIdx.x];
    const bool tile = J.slot != nullptr;
    const int pitch = tile ? A.T : A.w;
    slamhip_cell *dc = tile ? (slamhip_cell *)J.slot : A.win_c;
    float *dp = tile ? (float *)(J.slot + k6p_slot_prob_offset((size_t)A.T * A.T)) : A.win_p;
    const int nx = J.nx, ny = J.ny;
    const int gpr = (nx + 3) / 4 + 1;                                      // groups per row, a row's misaligned head included
    const int items = gpr * ny;
    for (int i = threadIdx.x; i < items; i += 256) {
        const int r = i / gpr, g = i - r * gpr;
        const size_t a = (size_t)(J.sy + r) * A.rw + J.sx;                 // the row's first cell in the staged rectangle
        const size_t b = (size_t)(J.ly + r) * pitch + J.lx;                // ... and in the window's or the tile's array
        const int e0 = g * 4 - (int)(b & 3);                               // the group's first cell in the row: b + e0 is a multiple of 4
        if (e0 >= nx) continue;
        if (e0 >= 0 && e0 + 4 <= nx) {
            const slamhip_cell *s = A.src + (a + e0);
            k6w_cell2 lo, hi;
            if (((a + e0) & 1) == 0) { lo = *(const k6w_cell2 *)s; hi = *(const k6w_cell2 *)(s + 2); }
            else {
                lo.e[0] = ((const k6w_cell1 *)s)[0].e; lo.e[1] = ((const k6w_cell1 *)s)[1].e;
                hi.e[0] = ((const k6w_cell1 *)s)[2].e; hi.e[1] = ((const k6w_cell1 *)s)[3].e;
            }
            float4 p;
            p.x = hs_prob_v(lo.e[0].value); p.y = hs_prob_v(lo.e[1].value); p.z = hs_prob_v(hi.e[0].value); p.w = hs_prob_v(hi.e[1].value);
            *(k6w_cell2 *)(dc + (b + e0)) = lo; *(k6w_cell2 *)(dc + (b + e0 + 2)) = hi;
            *(float4 *)(dp + (b + e0)) = p;
            continue;
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int e = e0 + k;
            if (e < 0 || e >= nx) continue;
            const k6w_cell1 c = *(const k6w_cell1 *)(A.src + (a + e));
            *(k6w_cell1 *)(dc + (b + e)) = c;
            dp[b + e] = hs_prob_v(c.e.value);
        }
    }
}

// ---- K6 world extents (slamhip_hs_world_extends) -----------------------------------------------------------------------------------
// The bounding rectangle, in world cells, of the cells whose Value != 0 (GridMap.GetMapExtends' test, GridMap.cs:161: a NaN counts)
// over the window and every tile of one level in ONE launch: a workgroup owns a job piece -- whole rows of the window or of one
// tile, (X0, Y0) the world cell of its first one -- and a tile's cell that lies under the window is skipped (its copy is stale).
// 64-bit results, ext = {xMax, yMax, xMin, yMin}, preset by the host to {INT64_MIN, INT64_MIN, INT64_MAX, INT64_MAX}.
struct k6x_job { const slamhip_cell *base; int64_t X0, Y0; uint16_t nx, ny; uint32_t pitch_kind; };   // pitch_kind: pitch * 2 + (1: a tile)
static_assert(sizeof(k6x_job) == 32, "a job piece is two 16-byte words");
struct k6x_arg { const k6x_job *jobs; long long *ext; int64_t wx0, wy0, wx1, wy1; };                  // the window: [wx0, wx1) x [wy0, wy1)

__global__ void __launch_bounds__(256) k6_world_extends(const k6x_arg A)
{
    const k6x_job J = A.jobs[blockIdx.x];
    const int pitch = (int)(J.pitch_kind >> 1), nx = J.nx, n = nx * (int)J.ny;
    const bool tile = (J.pitch_kind & 1u) != 0;
    long long xmax = INT64_MIN, ymax = INT64_MIN, xmin = INT64_MAX, ymin = INT64_MAX;
    for (int i = threadIdx.x; i < n; i += 256) {
        const int r = i / nx, x = i - r * nx;
        if (J.base[(size_t)r * pitch + x].value != 0.0f) {
            const long long X = J.X0 + x, Y = J.Y0 + r;
            if (tile && X >= A.wx0 && X < A.wx1 && Y >= A.wy0 && Y < A.wy1) continue;
            xmax = X > xmax ? X : xmax; xmin = X < xmin ? X : xmin;
            ymax = Y > ymax ? Y : ymax; ymin = Y < ymin ? Y : ymin;
        }
    }
    for (int m = 1; m < 64; m <<= 1) {
        const long long a = __shfl_xor(xmax, m), b = __shfl_xor(ymax, m), c = __shfl_xor(xmin, m), d = __shfl_xor(ymin, m);
        xmax = a > xmax ? a : xmax; ymax = b > ymax ? b : ymax; xmin = c < xmin ? c : xmin; ymin = d < ymin ? d : ymin;
    }
    if ((threadIdx.x & 63) == 0 && xmax != INT64_MIN) {
        atomicMax(A.ext + 0, xmax); atomicMax(A.ext + 1, ymax);
        atomicMin(A.ext + 2, xmin); atomicMin(A.ext + 3, ymin);
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------
// the backing store's books: the pool (chunks of slots), the directory (level, ty, tx) -> slot, and the pinned ring the job
// tables reach the device from -- a block of the ring is refilled only after the launch that read it has finished (an event per
// block, the context's bounded wait; with HS_BK_RING launches in flight at most, in steady state that costs no wait)
#define HS_BK_RING 4
#define HS_BK_CHUNK_BYTES ((size_t)4 << 20)
struct hs_bk_block { k6p_job *h; size_t cap; hipEvent_t ev; bool in_flight; };
struct hs_bk_chunk { unsigned char *base; size_t slots; };
typedef std::tuple<int, int64_t, int64_t> hs_tile_key;                     // (level, ty, tx)
struct hs_backing {
    int T; uint64_t max_bytes; size_t slot_bytes;
    std::vector<hs_bk_chunk> chunks;
    std::vector<unsigned char *> free_slots;                               // a stack: the lowest address of the newest chunk on top
    std::map<hs_tile_key, unsigned char *> dir;
    int64_t bytes, evicted, restored, dropped;
    hs_bk_block ring[HS_BK_RING]; unsigned ring_next;
    std::vector<slamhip_backing_job> plan;
    std::vector<k6p_job> pieces;
};

static void hs_bk_fill_chunk(slamhip_hs *hs, const hs_bk_chunk &c)
{
    const int t2 = hs->bk->T * hs->bk->T;
    const size_t n = c.slots * (size_t)t2, want = (n + 2047) / 2048;
    hipLaunchKernelGGL(k6_fill_slots, dim3((unsigned)(want < 1 ? 1 : want > 2048 ? 2048 : want)), dim3(256), 0, hs->ctx->stream, c.base, t2, n);
}
static void hs_bk_push_free(hs_backing *bk, const hs_bk_chunk &c)
{
    for (size_t k = c.slots; k-- > 0;) bk->free_slots.push_back(c.base + k * bk->slot_bytes);
}

// a slot for a new tile, initialised on the stream before its first use; nullptr if none can be had (the caller drops the cells)
static unsigned char *hs_bk_slot(slamhip_hs *hs)
{
    hs_backing *bk = hs->bk;
    if (bk->free_slots.empty()) {
        const uint64_t room = bk->max_bytes > (uint64_t)bk->bytes ? bk->max_bytes - (uint64_t)bk->bytes : 0;
        size_t n = HS_BK_CHUNK_BYTES / bk->slot_bytes;
        if (n < 1) n = 1;
        if ((uint64_t)n > room / bk->slot_bytes) n = (size_t)(room / bk->slot_bytes);
        if (n == 0) return nullptr;
        hs_bk_chunk c = { nullptr, n };
        if (hipMalloc(&c.base, n * bk->slot_bytes) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        bk->chunks.push_back(c);
        bk->bytes += (int64_t)(n * bk->slot_bytes);
        hs_bk_fill_chunk(hs, c);
        hs_bk_push_free(bk, c);
    }
    unsigned char *s = bk->free_slots.back();
    bk->free_slots.pop_back();
    return s;
}

// (the caller has drained the stream)
void hs_bk_free(slamhip_hs *hs)
{
    hs_backing *bk = hs->bk;
    if (!bk) return;
    for (const hs_bk_chunk &c : bk->chunks) (void)hipFree(c.base);
    for (int i = 0; i < HS_BK_RING; i++) {
        if (bk->ring[i].h) (void)hipHostFree(bk->ring[i].h);
        if (bk->ring[i].ev) (void)hipEventDestroy(bk->ring[i].ev);
    }
    delete bk;
    hs->bk = nullptr;
}

// The second launch of a shift with backing on: plan (backing_plan.h), deal slots in job order, cut the jobs into pieces of whole
// rows, put the table into the next block of the pinned ring and enqueue k6_page behind k6_shift.  (ox, oy): the origin BEFORE
// the shift; hs->lv already carries the swapped names.
static int32_t hs_bk_page(slamhip_hs *hs, int64_t ox, int64_t oy, int32_t dx, int32_t dy)
{
    hs_backing *bk = hs->bk;
    const int T = bk->T;
    bp_plan(hs->n_levels, hs->lv[0].w, hs->lv[0].h, ox, oy, dx, dy, T, bk->plan);
    bk->pieces.clear();
    for (const slamhip_backing_job &j : bk->plan) {
        const hs_level &L = hs->lv[j.level];
        // (what keeps the launch inside its arrays: a piece of the window, a piece of one tile)
        if (j.level < 0 || j.level >= hs->n_levels || j.nx < 1 || j.ny < 1 || j.wx < 0 || j.wy < 0 || j.wx + j.nx > L.w || j.wy + j.ny > L.h ||
            j.lx < 0 || j.ly < 0 || j.lx + j.nx > T || j.ly + j.ny > T)
            SH_FAIL(SLAMHIP_ERR_STATE, "slamhip_hs_shift: the backing store's planner produced a job outside its window or tile (level %d)", j.level);
        const int64_t area = (int64_t)j.nx * j.ny;
        const hs_tile_key key(j.level, j.ty, j.tx);
        auto it = bk->dir.find(key);
        unsigned char *slot = it != bk->dir.end() ? it->second : nullptr;
        if (j.kind == SLAMHIP_BACKING_EVICT) {
            if (!slot) {
                slot = hs_bk_slot(hs);
                if (!slot) { bk->dropped += area; continue; }
                bk->dir[key] = slot;
            }
            bk->evicted += area;
        } else {
            if (!slot) continue;                                           // nothing was ever evicted there: k6_shift's Reset stands
            bk->restored += area;
        }
        const int rows = K6P_CELLS / j.nx > 0 ? K6P_CELLS / j.nx : 1;
        for (int r0 = 0; r0 < j.ny; r0 += rows) {
            k6p_job p;
            p.slot = slot; p.wx = j.wx; p.wy = j.wy + r0;
            p.nx = (uint16_t)j.nx; p.ny = (uint16_t)(j.ny - r0 < rows ? j.ny - r0 : rows);
            p.lx = (uint16_t)j.lx; p.ly = (uint16_t)(j.ly + r0);
            p.level_kind = (uint32_t)(j.level * 2 + j.kind); p.pad = 0;
            bk->pieces.push_back(p);
        }
    }
    if (bk->pieces.empty()) return SLAMHIP_OK;
    if (bk->pieces.size() > (size_t)INT32_MAX) SH_FAIL(SLAMHIP_ERR_INVALID, "slamhip_hs_shift: %zu job pieces in one shift", bk->pieces.size());
    hs_bk_block &B = bk->ring[bk->ring_next++ % HS_BK_RING];
    if (!B.ev) SH_HIP(hipEventCreateWithFlags(&B.ev, hipEventDisableTiming));
    if (B.in_flight) { SH_TRY(sh_event_wait(hs->ctx, B.ev)); B.in_flight = false; }
    if (B.cap < bk->pieces.size()) {
        if (B.h) { (void)hipHostFree(B.h); B.h = nullptr; B.cap = 0; }
        const size_t cap = bk->pieces.size() + bk->pieces.size() / 2 + 256;
        SH_HIP(hipHostMalloc((void **)&B.h, sizeof(k6p_job) * cap, hipHostMallocMapped | hipHostMallocCoherent));
        B.cap = cap;
    }
    memcpy(B.h, bk->pieces.data(), sizeof(k6p_job) * bk->pieces.size());
    k6p_arg A;
    memset(&A, 0, sizeof(A));
    for (int l = 0; l < hs->n_levels; l++) {
        const hs_level &L = hs->lv[l];
        A.lv[l].w = L.w;
        A.lv[l].old_c = L.d_cells_alt; A.lv[l].old_p = L.d_prob_alt;       // (after the swap: what the window was)
        A.lv[l].new_c = L.d_cells; A.lv[l].new_p = L.d_prob;
    }
    A.jobs = B.h; A.T = T;
    hipLaunchKernelGGL(k6_page, dim3((unsigned)bk->pieces.size()), dim3(256), 0, hs->ctx->stream, A);
    SH_HIP(hipGetLastError());
    SH_HIP(hipEventRecord(B.ev, hs->ctx->stream));
    B.in_flight = true;
    return SLAMHIP_OK;
}

// slamhip_hs_reset: the directory goes, the pool stays -- every slot Reset again
void hs_bk_reset(slamhip_hs *hs)
{
    hs->bk->dir.clear();
    hs->bk->free_slots.clear();
    for (const hs_bk_chunk &c : hs->bk->chunks) { hs_bk_fill_chunk(hs, c); hs_bk_push_free(hs->bk, c); }
}


// The window moves by (+dx, +dy) level-0 cells (K6 above).  Enqueue-only: behind every update and match already on the operator's
// stream, ahead of whatever is enqueued later; no host wait.
extern "C" int32_t slamhip_hs_shift(slamhip_hs *hs, int32_t dx, int32_t dy)
{
    SH_CHECK_ARG(hs);
    if (hs->ctx->poisoned) SH_FAIL(SLAMHIP_ERR_TIMEOUT, "the context was poisoned by a blocking wait that timed out; destroy it");
    const int32_t g = 1 << (hs->n_levels - 1);
    if ((dx & (g - 1)) != 0 || (dy & (g - 1)) != 0)
        SH_FAIL(SLAMHIP_ERR_INVALID, "slamhip_hs_shift: dx = %d and dy = %d must be multiples of %d = 1 << (levels - 1), so that every level moves by whole cells",
                dx, dy, g);
    if (hs->ref_cache)
        SH_FAIL(SLAMHIP_ERR_INVALID, "slamhip_hs_shift: the reference's cache is on (slamhip_hs_set_reference_cache) -- its literal stale entries have "
                "no meaning under an operation the reference lacks; turn it off first");
    if (dx == 0 && dy == 0) return SLAMHIP_OK;
    SH_HIP(hipSetDevice(hs->ctx->device));
    if (!hs->lv[0].d_cells_alt) {                                          // the first shift: the second set, all levels or none
        for (int l = 0; l < hs->n_levels; l++) {
            hs_level &L = hs->lv[l];
            const size_t n = (size_t)L.w * L.h;
            if (hipMalloc(&L.d_cells_alt, sizeof(slamhip_cell) * n) != hipSuccess || hipMalloc(&L.d_prob_alt, sizeof(float) * n) != hipSuccess) {
                (void)hipGetLastError();
                for (int k = 0; k < hs->n_levels; k++) {
                    (void)hipFree(hs->lv[k].d_cells_alt); (void)hipFree(hs->lv[k].d_prob_alt);
                    hs->lv[k].d_cells_alt = nullptr; hs->lv[k].d_prob_alt = nullptr;
                }
                SH_FAIL(SLAMHIP_ERR_NOMEM, "device allocation of the window's second set of arrays failed (level %d)", l);
            }
        }
    }
    k6_arg A;
    memset(&A, 0, sizeof(A));
    A.n = hs->n_levels;
    int blocks = 0;
    for (int l = 0; l < hs->n_levels; l++) {
        const hs_level &L = hs->lv[l];
        k6_level &K = A.lv[l];
        K.w = L.w; K.h = L.h;
        const int sx = dx >> l, sy = dy >> l;                              // (exact: dx and dy are multiples of 1 << (levels - 1); arithmetic shift)
        // a move by the level's size or more clears the level: every source is then outside it whatever the other axis says, and
        // the clamp keeps sy * w + sx inside 32 bits
        K.sx = sx >= L.w ? L.w : sx <= -L.w ? -L.w : sx;
        K.sy = sy >= L.h ? L.h : sy <= -L.h ? -L.h : sy;
        K.blk0 = blocks;
        K.src_c = L.d_cells; K.dst_c = L.d_cells_alt; K.src_p = L.d_prob; K.dst_p = L.d_prob_alt;
        blocks += (int)(((size_t)L.w * L.h + K6_BLOCK - 1) / K6_BLOCK);
    }
    hipLaunchKernelGGL(k6_shift, dim3(blocks), dim3(256), 0, hs->ctx->stream, A);
    SH_HIP(hipGetLastError());
    for (int l = 0; l < hs->n_levels; l++) {
        hs_level &L = hs->lv[l];
        slamhip_cell *c = L.d_cells; L.d_cells = L.d_cells_alt; L.d_cells_alt = c;
        float *p = L.d_prob; L.d_prob = L.d_prob_alt; L.d_prob_alt = p;
    }
    // K5's sector records (d_k5_sec) stay: they split the NEXT scan's lines, by line index, into eight ranges of equal expected
    // work -- a balance hint only ("any partition is correct", k5_cells) that says nothing about where cells lie in memory.
    hs->win_ox += dx; hs->win_oy += dy;
    if (hs->bk) return hs_bk_page(hs, hs->win_ox - dx, hs->win_oy - dy, dx, dy);   // slamhip_hs_set_backing: ONE more launch
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_set_backing(slamhip_hs *hs, int32_t tile_cells, uint64_t max_bytes)
{
    SH_CHECK_ARG(hs);
    if (max_bytes == 0) {                                                  // off: every tile dropped, the pool freed
        if (!hs->bk) return SLAMHIP_OK;
        SH_HIP(hipSetDevice(hs->ctx->device));
        if (!hs->ctx->poisoned) SH_HIP(hipStreamSynchronize(hs->ctx->stream));   // (launches that read the pool or the ring may be in flight)
        hs_bk_free(hs);
        return SLAMHIP_OK;
    }
    if (tile_cells < 8 || tile_cells > 256 || (tile_cells & (tile_cells - 1)) != 0)
        SH_FAIL(SLAMHIP_ERR_INVALID, "slamhip_hs_set_backing: tile_cells = %d must be a power of two in [8, 256]", tile_cells);
    const size_t slot_bytes = k6p_slot_bytes((size_t)tile_cells * tile_cells);
    if (max_bytes < slot_bytes)
        SH_FAIL(SLAMHIP_ERR_INVALID, "slamhip_hs_set_backing: max_bytes = %llu is less than one slot of %zu bytes", (unsigned long long)max_bytes, slot_bytes);
    if (hs->bk) {
        hs_backing *bk = hs->bk;
        if (bk->T == tile_cells && max_bytes >= (uint64_t)bk->bytes) { bk->max_bytes = max_bytes; return SLAMHIP_OK; }
        if (!bk->dir.empty())
            SH_FAIL(SLAMHIP_ERR_INVALID, "slamhip_hs_set_backing: tiles exist -- tile_cells (%d -> %d) cannot change and max_bytes cannot fall below the pool's "
                    "%lld bytes; switch backing off first", bk->T, tile_cells, (long long)bk->bytes);
        SH_TRY(slamhip_hs_set_backing(hs, 0, 0));                          // (no tiles: a new pool under the new setting)
    }
    hs_backing *bk = new (std::nothrow) hs_backing();
    if (!bk) SH_FAIL(SLAMHIP_ERR_NOMEM, "out of host memory");
    bk->T = tile_cells; bk->max_bytes = max_bytes; bk->slot_bytes = slot_bytes;
    bk->bytes = bk->evicted = bk->restored = bk->dropped = 0;
    memset(bk->ring, 0, sizeof(bk->ring)); bk->ring_next = 0;
    hs->bk = bk;
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_backing_stats(slamhip_hs *hs, slamhip_backing_stats *out)
{
    SH_CHECK_ARG(hs && out);
    memset(out, 0, sizeof(*out));
    if (!hs->bk) return SLAMHIP_OK;
    const hs_backing *bk = hs->bk;
    out->tiles = (int64_t)bk->dir.size(); out->bytes = bk->bytes; out->capacity_bytes = (int64_t)bk->max_bytes;
    out->evicted_cells = bk->evicted; out->restored_cells = bk->restored; out->dropped_cells = bk->dropped;
    out->tile = bk->T; out->on = 1;
    return SLAMHIP_OK;
}

// Host-side assembly: `out` starts as Reset; every tile that exists and meets the rectangle is copied into its place, then the
// window over them (the same stream: the window wins), then one bounded wait.
extern "C" int32_t slamhip_hs_world_cells_download(slamhip_hs *hs, int32_t level, int64_t x0, int64_t y0, int32_t w, int32_t h, slamhip_cell *out)
{
    SH_CHECK_ARG(hs && out && level >= 0 && level < hs->n_levels);
    if (w < 1 || h < 1 || (int64_t)w * h > ((int64_t)1 << 26))
        SH_FAIL(SLAMHIP_ERR_INVALID, "slamhip_hs_world_cells_download: w = %d and h = %d must be positive with w * h <= 2^26 cells", w, h);
    SH_CHECK_ARG(x0 > -((int64_t)1 << 60) && x0 < ((int64_t)1 << 60) && y0 > -((int64_t)1 << 60) && y0 < ((int64_t)1 << 60));
    slamhip_ctx *ctx = hs->ctx;
    if (ctx->poisoned) SH_FAIL(SLAMHIP_ERR_TIMEOUT, "the context was poisoned by a blocking wait that timed out; destroy it");
    SH_HIP(hipSetDevice(ctx->device));
    const hs_level &L = hs->lv[level];
    const size_t n = (size_t)w * h;
    for (size_t i = 0; i < n; i++) out[i] = hs_reset_cell();
    const int64_t x1 = x0 + w, y1 = y0 + h;
    // [ax, bx) x [ay, by) in world cells, from a device array of `pitch` cells per row whose cell (0, 0) is world cell (sx0, sy0)
    auto copy_rect = [&](const slamhip_cell *src, int pitch, int64_t sx0, int64_t sy0, int64_t ax, int64_t ay, int64_t bx, int64_t by) -> hipError_t {
        return hipMemcpy2DAsync(out + (size_t)(ay - y0) * w + (size_t)(ax - x0), sizeof(slamhip_cell) * (size_t)w,
                                src + (size_t)(ay - sy0) * pitch + (size_t)(ax - sx0), sizeof(slamhip_cell) * (size_t)pitch,
                                sizeof(slamhip_cell) * (size_t)(bx - ax), (size_t)(by - ay), hipMemcpyDeviceToHost, ctx->stream);
    };
    if (hs->bk && !hs->bk->dir.empty()) {
        const hs_backing *bk = hs->bk;
        const int64_t T = bk->T;
        auto tile_copy = [&](int64_t ty, int64_t tx, const unsigned char *slot) -> hipError_t {
            const int64_t ax = std::max(x0, tx * T), bx = std::min(x1, tx * T + T), ay = std::max(y0, ty * T), by = std::min(y1, ty * T + T);
            if (ax >= bx || ay >= by) return hipSuccess;
            return copy_rect((const slamhip_cell *)slot, (int)T, tx * T, ty * T, ax, ay, bx, by);
        };
        const int64_t tx_a = bp_floor_div(x0, T), tx_b = bp_floor_div(x1 - 1, T), ty_a = bp_floor_div(y0, T), ty_b = bp_floor_div(y1 - 1, T);
        if ((uint64_t)(tx_b - tx_a + 1) * (uint64_t)(ty_b - ty_a + 1) <= bk->dir.size()) {
            for (int64_t ty = ty_a; ty <= ty_b; ty++)
                for (int64_t tx = tx_a; tx <= tx_b; tx++) {
                    auto it = bk->dir.find(hs_tile_key(level, ty, tx));
                    if (it != bk->dir.end()) SH_HIP(tile_copy(ty, tx, it->second));
                }
        } else {
            for (auto it = bk->dir.lower_bound(hs_tile_key(level, INT64_MIN, INT64_MIN)); it != bk->dir.end() && std::get<0>(it->first) == level; ++it)
                SH_HIP(tile_copy(std::get<1>(it->first), std::get<2>(it->first), it->second));
        }
    }
    {
        const int64_t OX = hs->win_ox >> level, OY = hs->win_oy >> level;
        const int64_t ax = std::max(x0, OX), bx = std::min(x1, OX + L.w), ay = std::max(y0, OY), by = std::min(y1, OY + L.h);
        if (ax < bx && ay < by) SH_HIP(copy_rect(L.d_cells, L.w, OX, OY, ax, ay, bx, by));
    }
    hipEvent_t ev = nullptr;
    SH_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    hipError_t e = hipEventRecord(ev, ctx->stream);
    int32_t rc = SLAMHIP_OK;
    if (e == hipSuccess) rc = sh_event_wait(ctx, ev);
    (void)hipEventDestroy(ev);
    SH_HIP(e);
    return rc;
}

// ---- the world upload and the world extents: host side ---------------------------------------------------------------------------
// Both calls block, so their staging buffer is idle whenever one of them starts: ONE device block per hs, grown when a call needs
// more and kept for the next (nothing is allocated per call that a second call of the same size allocates again), and the host
// vectors the tables are built in.  The upload lays it out as the staged cells, then the job pieces; the extents as the four
// result words, then the job pieces.  h_ext: eight pinned words the extents' presets leave the host from and its results come back
// into -- no copy of a blocking call that timed out can land in a caller's or a dead stack frame's memory.
struct hs_world {
    unsigned char *d; size_t cap; hipEvent_t ev; long long *h_ext;
    std::vector<slamhip_world_job> plan;
    std::vector<k6w_piece> pieces;
    std::vector<k6x_job> xjobs;
};

static int32_t hs_wp_stage(slamhip_hs *hs, size_t bytes)
{
    if (!hs->wp) {
        hs_world *wp = new (std::nothrow) hs_world();
        if (!wp) SH_FAIL(SLAMHIP_ERR_NOMEM, "out of host memory");
        wp->d = nullptr; wp->cap = 0; wp->ev = nullptr; wp->h_ext = nullptr;
        hs->wp = wp;
    }
    hs_world *wp = hs->wp;
    if (!wp->ev) SH_HIP(hipEventCreateWithFlags(&wp->ev, hipEventDisableTiming));
    if (!wp->h_ext) SH_HIP(hipHostMalloc((void **)&wp->h_ext, 8 * sizeof(long long), hipHostMallocDefault));
    if (wp->cap < bytes) {
        if (wp->d) { (void)hipFree(wp->d); wp->d = nullptr; wp->cap = 0; }
        if (hipMalloc(&wp->d, bytes) != hipSuccess) { (void)hipGetLastError(); SH_FAIL(SLAMHIP_ERR_NOMEM, "device allocation of a staging buffer of %zu bytes failed", bytes); }
        wp->cap = bytes;
    }
    return SLAMHIP_OK;
}

// (the caller has drained the stream)
void hs_wp_free(slamhip_hs *hs)
{
    hs_world *wp = hs->wp;
    if (!wp) return;
    if (wp->d) (void)hipFree(wp->d);
    if (wp->ev) (void)hipEventDestroy(wp->ev);
    if (wp->h_ext) (void)hipHostFree(wp->h_ext);
    delete wp;
    hs->wp = nullptr;
}

static inline bool hs_cell_is_reset(const slamhip_cell &c)                  // LogOddsCell.Reset() {-1, 0.0f}, as bits
{
    uint32_t v;
    memcpy(&v, &c.value, sizeof(v));
    return c.update_index == -1 && v == 0u;
}
// ONE walk over the nx x ny cells from (sx, sy) of the caller's array (rows of rw cells): the cells that are not Reset, and the
// largest update index into *mx.  Every cell of the rectangle is walked exactly once per upload.
static int64_t hs_wp_scan(const slamhip_cell *cells, int rw, int sx, int sy, int nx, int ny, int *mx)
{
    int64_t n = 0;
    int m = *mx;
    for (int r = 0; r < ny; r++) {
        const slamhip_cell *row = cells + (size_t)(sy + r) * rw + sx;
        for (int x = 0; x < nx; x++) {
            n += !hs_cell_is_reset(row[x]);
            if (row[x].update_index > m) m = row[x].update_index;
        }
    }
    *mx = m;
    return n;
}

extern "C" int32_t slamhip_hs_world_cells_upload(slamhip_hs *hs, int32_t level, int64_t x0, int64_t y0, int32_t w, int32_t h,
                                                 const slamhip_cell *cells, int64_t *out_dropped)
{
    SH_CHECK_ARG(hs && cells && level >= 0 && level < hs->n_levels);
    if (w < 1 || h < 1 || (int64_t)w * h > ((int64_t)1 << 26))
        SH_FAIL(SLAMHIP_ERR_INVALID, "slamhip_hs_world_cells_upload: w = %d and h = %d must be positive with w * h <= 2^26 cells", w, h);
    SH_CHECK_ARG(x0 > -((int64_t)1 << 60) && x0 < ((int64_t)1 << 60) && y0 > -((int64_t)1 << 60) && y0 < ((int64_t)1 << 60));
    slamhip_ctx *ctx = hs->ctx;
    if (ctx->poisoned) SH_FAIL(SLAMHIP_ERR_TIMEOUT, "the context was poisoned by a blocking wait that timed out; destroy it");
    SH_HIP(hipSetDevice(ctx->device));
    hs_level &L = hs->lv[level];
    hs_backing *bk = hs->bk;
    const int T = bk ? bk->T : 0;
    const size_t n = (size_t)w * h;
    const size_t pieces_at = (sizeof(slamhip_cell) * n + 15) & ~(size_t)15;
    SH_TRY(hs_wp_stage(hs, 0));
    hs_world *wp = hs->wp;
    wp_plan(L.w, L.h, hs->win_ox >> level, hs->win_oy >> level, x0, y0, w, h, T, wp->plan);
    // (what keeps the launch inside its arrays: a piece of the rectangle into a piece of the window or of one tile)
    for (const slamhip_world_job &j : wp->plan) {
        const int dw = j.kind == SLAMHIP_WORLD_WINDOW ? L.w : T, dh = j.kind == SLAMHIP_WORLD_WINDOW ? L.h : T;
        if ((j.kind != SLAMHIP_WORLD_WINDOW && j.kind != SLAMHIP_WORLD_TILE) || j.nx < 1 || j.ny < 1 || j.sx < 0 || j.sy < 0 ||
            j.sx + j.nx > w || j.sy + j.ny > h || j.lx < 0 || j.ly < 0 || j.lx + j.nx > dw || j.ly + j.ny > dh)
            SH_FAIL(SLAMHIP_ERR_STATE, "slamhip_hs_world_cells_upload: the planner produced a job outside its rectangle, window or tile (level %d)", level);
    }
    // everything that can fail for a reason of its own comes before a slot is taken: the staging block at its largest (every job
    // cut into its pieces), then the cells' copy -- an error up to here has changed nothing
    size_t max_pieces = 0;
    for (const slamhip_world_job &j : wp->plan) {
        const int rows = K6P_CELLS / j.nx > 0 ? K6P_CELLS / j.nx : 1;
        max_pieces += (size_t)((j.ny + rows - 1) / rows);
    }
    if (max_pieces > (size_t)INT32_MAX) SH_FAIL(SLAMHIP_ERR_INVALID, "slamhip_hs_world_cells_upload: %zu job pieces in one upload", max_pieces);
    if (max_pieces > 0) {
        SH_TRY(hs_wp_stage(hs, pieces_at + sizeof(k6w_piece) * max_pieces));
        SH_HIP(hipMemcpyAsync(wp->d, cells, sizeof(slamhip_cell) * n, hipMemcpyHostToDevice, ctx->stream));
    }
    int64_t dropped = 0;
    int mx = -1;
    // slots, in the planner's job order: the jobs of one tile follow one another, and the tile's piece is all of them
    wp->pieces.clear();
    auto cut = [&](const slamhip_world_job &j, unsigned char *slot) {
        const int rows = K6P_CELLS / j.nx > 0 ? K6P_CELLS / j.nx : 1;
        for (int r0 = 0; r0 < j.ny; r0 += rows) {
            k6w_piece p;
            p.slot = slot; p.sx = j.sx; p.sy = j.sy + r0;
            p.nx = (uint16_t)j.nx; p.ny = (uint16_t)(j.ny - r0 < rows ? j.ny - r0 : rows);
            p.lx = j.lx; p.ly = j.ly + r0; p.pad = 0;
            wp->pieces.push_back(p);
        }
    };
    for (size_t k = 0; k < wp->plan.size();) {
        const slamhip_world_job &j = wp->plan[k];
        if (j.kind == SLAMHIP_WORLD_WINDOW) { (void)hs_wp_scan(cells, w, j.sx, j.sy, j.nx, j.ny, &mx); cut(j, nullptr); k++; continue; }
        size_t k1 = k;
        int64_t live = 0;
        while (k1 < wp->plan.size() && wp->plan[k1].kind == SLAMHIP_WORLD_TILE && wp->plan[k1].tx == j.tx && wp->plan[k1].ty == j.ty) {
            const slamhip_world_job &q = wp->plan[k1++];
            live += hs_wp_scan(cells, w, q.sx, q.sy, q.nx, q.ny, &mx);
        }
        const hs_tile_key key(level, j.ty, j.tx);
        auto it = bk->dir.find(key);
        unsigned char *slot = it != bk->dir.end() ? it->second : nullptr;
        if (!slot && live > 0) {
            slot = hs_bk_slot(hs);
            if (slot) bk->dir[key] = slot;
            else dropped += live;
        }
        if (slot) for (size_t q = k; q < k1; q++) cut(wp->plan[q], slot);
        k = k1;
    }
    if (bk) bk->dropped += dropped;
    else {
        // backing off: the planner gave the window job alone; what lies outside it -- the band above, the band below, the strips
        // left and right -- is walked here, and every non-Reset cell of it is dropped
        int bx0 = 0, bx1 = 0, by0 = 0, by1 = 0;                            // the window job in the rectangle; empty: none
        if (!wp->plan.empty()) { bx0 = wp->plan[0].sx; bx1 = bx0 + wp->plan[0].nx; by0 = wp->plan[0].sy; by1 = by0 + wp->plan[0].ny; }
        if (bx0 >= bx1) dropped = hs_wp_scan(cells, w, 0, 0, w, h, &mx);
        else {
            dropped = hs_wp_scan(cells, w, 0, 0, w, by0, &mx) + hs_wp_scan(cells, w, 0, by1, w, h - by1, &mx) +
                      hs_wp_scan(cells, w, 0, by0, bx0, by1 - by0, &mx) + hs_wp_scan(cells, w, bx1, by0, w - bx1, by1 - by0, &mx);
        }
    }
    if (out_dropped) *out_dropped = dropped;
    if (!wp->pieces.empty()) {                                             // (at most max_pieces: the block holds them)
        SH_HIP(hipMemcpyAsync(wp->d + pieces_at, wp->pieces.data(), sizeof(k6w_piece) * wp->pieces.size(), hipMemcpyHostToDevice, ctx->stream));
        k6w_arg A;
        A.src = (const slamhip_cell *)wp->d; A.pieces = (const k6w_piece *)(wp->d + pieces_at);
        A.win_c = L.d_cells; A.win_p = L.d_prob; A.rw = w; A.w = L.w; A.T = T;
        hipLaunchKernelGGL(k6_world_put, dim3((unsigned)wp->pieces.size()), dim3(256), 0, ctx->stream, A);
        SH_HIP(hipGetLastError());
    }
    SH_HIP(hipEventRecord(wp->ev, ctx->stream));
    SH_TRY(sh_event_wait(ctx, wp->ev));
    // keep the once-per-scan guards meaningful, as slamhip_hs_cells_upload does: the next scan's marks must exceed every stored index
    if (mx >= 0) {                      // marks of scan k are 3k+1 / 3k+2 (OccGridMap.cs:116-117,:144)
        const int need = (mx / 3 + 1) * 3;
        if (need > L.curr_update_index) L.curr_update_index = need;
    }
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_world_extends(slamhip_hs *hs, int32_t level, int64_t extends[4], int32_t *found)
{
    SH_CHECK_ARG(hs && extends && found && level >= 0 && level < hs->n_levels);
    slamhip_ctx *ctx = hs->ctx;
    if (ctx->poisoned) SH_FAIL(SLAMHIP_ERR_TIMEOUT, "the context was poisoned by a blocking wait that timed out; destroy it");
    SH_HIP(hipSetDevice(ctx->device));
    const hs_level &L = hs->lv[level];
    SH_TRY(hs_wp_stage(hs, 0));
    hs_world *wp = hs->wp;
    wp->xjobs.clear();
    // pieces of whole rows, at most K6P_CELLS cells each, of an array of nx x ny cells whose cell (0, 0) is world cell (X0, Y0)
    auto cut = [&](const slamhip_cell *base, int nx, int ny, int64_t X0, int64_t Y0, unsigned kind) {
        const int rows = K6P_CELLS / nx > 0 ? K6P_CELLS / nx : 1;
        for (int r0 = 0; r0 < ny; r0 += rows) {
            k6x_job j;
            j.base = base + (size_t)r0 * nx; j.X0 = X0; j.Y0 = Y0 + r0;
            j.nx = (uint16_t)nx; j.ny = (uint16_t)(ny - r0 < rows ? ny - r0 : rows);
            j.pitch_kind = (uint32_t)nx * 2u + kind;
            wp->xjobs.push_back(j);
        }
    };
    const int64_t OX = hs->win_ox >> level, OY = hs->win_oy >> level;
    cut(L.d_cells, L.w, L.h, OX, OY, 0u);
    if (hs->bk) {
        const hs_backing *bk = hs->bk;
        const int64_t T = bk->T;
        for (auto it = bk->dir.lower_bound(hs_tile_key(level, INT64_MIN, INT64_MIN)); it != bk->dir.end() && std::get<0>(it->first) == level; ++it)
            cut((const slamhip_cell *)it->second, (int)T, (int)T, std::get<2>(it->first) * T, std::get<1>(it->first) * T, 1u);
    }
    if (wp->xjobs.size() > (size_t)INT32_MAX) SH_FAIL(SLAMHIP_ERR_INVALID, "slamhip_hs_world_extends: %zu job pieces", wp->xjobs.size());
    const size_t jobs_at = 32;
    SH_TRY(hs_wp_stage(hs, jobs_at + sizeof(k6x_job) * wp->xjobs.size()));
    long long *e4 = wp->h_ext, *r4 = wp->h_ext + 4;                        // (pinned, the library's own: see hs_world)
    e4[0] = e4[1] = INT64_MIN; e4[2] = e4[3] = INT64_MAX;
    r4[0] = r4[1] = r4[2] = r4[3] = 0;
    SH_HIP(hipMemcpyAsync(wp->d, e4, 4 * sizeof(long long), hipMemcpyHostToDevice, ctx->stream));
    SH_HIP(hipMemcpyAsync(wp->d + jobs_at, wp->xjobs.data(), sizeof(k6x_job) * wp->xjobs.size(), hipMemcpyHostToDevice, ctx->stream));
    k6x_arg A;
    A.jobs = (const k6x_job *)(wp->d + jobs_at); A.ext = (long long *)wp->d;
    A.wx0 = OX; A.wy0 = OY; A.wx1 = OX + L.w; A.wy1 = OY + L.h;
    hipLaunchKernelGGL(k6_world_extends, dim3((unsigned)wp->xjobs.size()), dim3(256), 0, ctx->stream, A);
    SH_HIP(hipGetLastError());
    SH_HIP(hipMemcpyAsync(r4, wp->d, 4 * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
    SH_HIP(hipEventRecord(wp->ev, ctx->stream));
    SH_TRY(sh_event_wait(ctx, wp->ev));
    const bool ok = r4[0] != INT64_MIN;
    for (int i = 0; i < 4; i++) extends[i] = ok ? (int64_t)r4[i] : 0;
    *found = ok ? 1 : 0;
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_origin(slamhip_hs *hs, int64_t *ox, int64_t *oy)
{
    SH_CHECK_ARG(hs && ox && oy);
    *ox = hs->win_ox; *oy = hs->win_oy;
    return SLAMHIP_OK;
}
