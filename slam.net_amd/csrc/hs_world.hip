// hs_world.hip -- the world behind the scrolling window of HectorSLAM and its backing store (hs_window.hip), the calls that block:
// download, upload and extents (slamhip_hs_world_cells_download, _world_cells_upload, _world_extends).
#include "hs_tiles.h"
#include "hs_blocks.h"
#include "world_plan.h"

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
    ~hs_world()                                                            // (the caller has drained the stream)
    {
        if (d) (void)hipFree(d);
        if (ev) (void)hipEventDestroy(ev);
        if (h_ext) (void)hipHostFree(h_ext);
    }
};

static int32_t hs_wp_stage(slamhip_hs *hs, size_t bytes)
{
    SH_TRY(hs_unit<&slamhip_hs::wp>(hs));                                  // (value-initialised: no block, no event yet)
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

// what opens every world call behind its argument checks: hs->wp exists from here on, with its event
static int32_t hs_world_enter(slamhip_hs *hs)
{
    if (hs->ctx->poisoned) SH_FAIL(SLAMHIP_ERR_TIMEOUT, "the context was poisoned by a blocking wait that timed out; destroy it");
    SH_HIP(hipSetDevice(hs->ctx->device));
    return hs_wp_stage(hs, 0);
}
// the caller's rectangle, of the download and of the upload
static int32_t hs_world_check_rect(const char *fn, int64_t x0, int64_t y0, int32_t w, int32_t h)
{
    if (w < 1 || h < 1 || (int64_t)w * h > ((int64_t)1 << 26))
        SH_FAIL(SLAMHIP_ERR_INVALID, "%s: w = %d and h = %d must be positive with w * h <= 2^26 cells", fn, w, h);
    SH_CHECK_ARG(x0 > -((int64_t)1 << 60) && x0 < ((int64_t)1 << 60) && y0 > -((int64_t)1 << 60) && y0 < ((int64_t)1 << 60));
    return SLAMHIP_OK;
}
// ... and what closes it: one bounded wait for everything the call enqueued, on the event hs_wp_stage made
static int32_t hs_world_wait(slamhip_hs *hs)
{
    SH_HIP(hipEventRecord(hs->wp->ev, hs->ctx->stream));
    return sh_event_wait(hs->ctx, hs->wp->ev);
}

// Host-side assembly: `out` starts as Reset; every tile that exists and meets the rectangle is copied into its place, then the
// window over them (the same stream: the window wins), then one bounded wait.
extern "C" int32_t slamhip_hs_world_cells_download(slamhip_hs *hs, int32_t level, int64_t x0, int64_t y0, int32_t w, int32_t h, slamhip_cell *out)
{
    SH_CHECK_ARG(hs && out && level >= 0 && level < hs->n_levels);
    SH_TRY(hs_world_check_rect("slamhip_hs_world_cells_download", x0, y0, w, h));
    SH_TRY(hs_world_enter(hs));
    slamhip_ctx *ctx = hs->ctx;
    const hs_level &L = hs->lv[level];
    std::fill_n(out, (size_t)w * h, hs_reset_cell());
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
        hipError_t e = hipSuccess;                                         // the first copy that failed: none is enqueued behind it
        auto tile_copy = [&](int64_t ty, int64_t tx, const unsigned char *slot) {
            const int64_t ax = std::max(x0, tx * T), bx = std::min(x1, tx * T + T), ay = std::max(y0, ty * T), by = std::min(y1, ty * T + T);
            if (e == hipSuccess && ax < bx && ay < by) e = copy_rect((const slamhip_cell *)slot, (int)T, tx * T, ty * T, ax, ay, bx, by);
        };
        const int64_t tx_a = bp_floor_div(x0, T), tx_b = bp_floor_div(x1 - 1, T), ty_a = bp_floor_div(y0, T), ty_b = bp_floor_div(y1 - 1, T);
        if ((uint64_t)(tx_b - tx_a + 1) * (uint64_t)(ty_b - ty_a + 1) <= bk->dir.size()) {   // fewer tiles to probe than the directory holds
            for (int64_t ty = ty_a; ty <= ty_b; ty++)
                for (int64_t tx = tx_a; tx <= tx_b; tx++)
                    if (const unsigned char *slot = bk->find(level, ty, tx)) tile_copy(ty, tx, slot);
        } else bk->for_each_tile(level, tile_copy);
        SH_HIP(e);
    }
    const int64_t OX = hs->win_ox >> level, OY = hs->win_oy >> level;
    const int64_t ax = std::max(x0, OX), bx = std::min(x1, OX + L.w), ay = std::max(y0, OY), by = std::min(y1, OY + L.h);
    if (ax < bx && ay < by) SH_HIP(copy_rect(L.d_cells, L.w, OX, OY, ax, ay, bx, by));
    return hs_world_wait(hs);
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
    SH_TRY(hs_world_check_rect("slamhip_hs_world_cells_upload", x0, y0, w, h));
    SH_TRY(hs_world_enter(hs));
    slamhip_ctx *ctx = hs->ctx;
    hs_level &L = hs->lv[level];
    hs_backing *bk = hs->bk;
    const int T = bk ? bk->T : 0;
    const size_t n = (size_t)w * h;
    const size_t pieces_at = (sizeof(slamhip_cell) * n + 15) & ~(size_t)15;
    hs_world *wp = hs->wp;
    wp_plan(L.w, L.h, hs->win_ox >> level, hs->win_oy >> level, x0, y0, w, h, T, wp->plan);
    // (what keeps the launch inside its arrays: a piece of the rectangle into a piece of the window or of one tile)
    size_t max_pieces = 0;
    for (const slamhip_world_job &j : wp->plan) {
        const int dw = j.kind == SLAMHIP_WORLD_WINDOW ? L.w : T, dh = j.kind == SLAMHIP_WORLD_WINDOW ? L.h : T;
        if ((j.kind != SLAMHIP_WORLD_WINDOW && j.kind != SLAMHIP_WORLD_TILE) || j.nx < 1 || j.ny < 1 || j.sx < 0 || j.sy < 0 ||
            j.sx + j.nx > w || j.sy + j.ny > h || j.lx < 0 || j.ly < 0 || j.lx + j.nx > dw || j.ly + j.ny > dh)
            SH_FAIL(SLAMHIP_ERR_STATE, "slamhip_hs_world_cells_upload: the planner produced a job outside its rectangle, window or tile (level %d)", level);
        max_pieces += hs_piece_count(j.nx, j.ny);
    }
    // everything that can fail for a reason of its own comes before a slot is taken: the staging block at its largest (every job
    // cut into its pieces), then the cells' copy -- an error up to here has changed nothing
    if (max_pieces > (size_t)INT32_MAX) SH_FAIL(SLAMHIP_ERR_INVALID, "slamhip_hs_world_cells_upload: %zu job pieces in one upload", max_pieces);
    if (max_pieces > 0) {
        SH_TRY(hs_wp_stage(hs, pieces_at + sizeof(k6w_piece) * max_pieces));
        SH_HIP(hipMemcpyAsync(wp->d, cells, sizeof(slamhip_cell) * n, hipMemcpyHostToDevice, ctx->stream));
    }
    int64_t dropped = 0;
    int mx = -1;                                                           // the largest update index met
    // slots, in the planner's job order: the jobs of one tile follow one another, and the tile's piece is all of them
    wp->pieces.clear();
    auto cut = [&](const slamhip_world_job &j, unsigned char *slot) {
        hs_cut_rows(j.nx, j.ny, [&](int r0, int rows) {
            k6w_piece p;
            p.slot = slot; p.sx = j.sx; p.sy = j.sy + r0;
            p.nx = (uint16_t)j.nx; p.ny = (uint16_t)rows; p.lx = j.lx; p.ly = j.ly + r0; p.pad = 0;
            wp->pieces.push_back(p);
        });
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
        unsigned char *slot = live > 0 ? bk->find_or_take(hs, level, j.ty, j.tx) : bk->find(level, j.ty, j.tx);
        if (!slot) dropped += live;
        else for (size_t q = k; q < k1; q++) cut(wp->plan[q], slot);
        k = k1;
    }
    if (bk) bk->dropped += dropped;
    else {
        // backing off: the planner gave the window job alone; what lies outside it (backing_plan.h's rectangles, the window job
        // the kept one; none: the whole rectangle) is walked here, and every non-Reset cell of it is dropped
        const slamhip_world_job kept = wp->plan.empty() ? slamhip_world_job() : wp->plan[0];
        bp_rect rects[4];
        const int nr = bp_frame_rects(w, h, kept.sx, kept.sx + kept.nx, kept.sy, kept.sy + kept.ny, rects);
        for (int r = 0; r < nr; r++) dropped += hs_wp_scan(cells, w, rects[r].x0, rects[r].y0, rects[r].x1 - rects[r].x0, rects[r].y1 - rects[r].y0, &mx);
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
    SH_TRY(hs_world_wait(hs));
    // keep the once-per-scan guards meaningful, as slamhip_hs_cells_upload does: the next scan's marks must exceed every stored index
    if (mx >= 0) {                      // marks of scan k are 3k+1 / 3k+2 (OccGridMap.cs:116-117,:144)
        const long long need = ((long long)mx / 3 + 1) * 3;                // (64-bit: an index near INT_MAX has no marks above it and moves nothing)
        if (need <= 0x7fffffffLL - 2 && need > L.curr_update_index) L.curr_update_index = (int)need;
    }
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_world_extends(slamhip_hs *hs, int32_t level, int64_t extends[4], int32_t *found)
{
    SH_CHECK_ARG(hs && extends && found && level >= 0 && level < hs->n_levels);
    SH_TRY(hs_world_enter(hs));
    slamhip_ctx *ctx = hs->ctx;
    const hs_level &L = hs->lv[level];
    hs_world *wp = hs->wp;
    wp->xjobs.clear();
    // an array of nx x ny cells whose cell (0, 0) is world cell (X0, Y0)
    auto cut = [&](const slamhip_cell *base, int nx, int ny, int64_t X0, int64_t Y0, unsigned kind) {
        hs_cut_rows(nx, ny, [&](int r0, int rows) {
            k6x_job j;
            j.base = base + (size_t)r0 * nx; j.X0 = X0; j.Y0 = Y0 + r0;
            j.nx = (uint16_t)nx; j.ny = (uint16_t)rows; j.pitch_kind = (uint32_t)nx * 2u + kind;
            wp->xjobs.push_back(j);
        });
    };
    const int64_t OX = hs->win_ox >> level, OY = hs->win_oy >> level;
    cut(L.d_cells, L.w, L.h, OX, OY, 0u);
    if (const hs_backing *bk = hs->bk)
        bk->for_each_tile(level, [&](int64_t ty, int64_t tx, const unsigned char *slot) { cut((const slamhip_cell *)slot, bk->T, bk->T, tx * bk->T, ty * bk->T, 1u); });
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
    SH_TRY(hs_world_wait(hs));
    const bool ok = r4[0] != INT64_MIN;
    for (int i = 0; i < 4; i++) extends[i] = ok ? (int64_t)r4[i] : 0;
    *found = ok ? 1 : 0;
    return SLAMHIP_OK;
}
