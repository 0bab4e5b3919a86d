// hs_render_world.hip -- K25, the stored scans drawn again into the WHOLE world behind the scrolling window: the window's arrays and the
// backing store's tiles (slamhip_hs_render_world, slamhip_debug_render_world).  Definition: include/slamhip.h; the arithmetic is
// K20's, shared through hs_render.h -- the line, its clip interval, the two transitions -- under the world bound instead of the
// window's w x h.  K20 (hs_render.hip) stays as it is: its kernels, its launch path and its hook are not touched.
//  * k25_boxes: a wavefront per (scan, level), as k20_boxes: the begin cell, the number of valid lines, the box of the begin cell and
//    the valid end cells, the largest da, and a mark for a cell beyond the world bound; 32 bytes, in window-frame cells (32 bits).
//    The host reads the boxes back BEFORE anything is changed: they say what is refused and which tiles the render needs.
//  * k25_render<B>: a workgroup of 256 lanes per block of B x B world cells of one level, all levels in one grid, the work from a job
//    table the host writes.  B = min(T, 32): a block never leaves its tile, so a job names ONE slot, and the host's check of the table
//    is a division and a directory look-up per job (DESIGN.md section 4 "K25" weighs this against 32-cell blocks over several small
//    tiles).  The window is aligned to the shift granularity, not to tiles: a block may straddle its edge, so every cell's address is
//    chosen per cell -- inside the window's rectangle the window's arrays (the window wins, as in the world download), outside it the
//    tile's slot, cells then probabilities; the part of a tile under the window is neither read nor written.  The rest is
//    k20_render: the block's cells stay in LDS while the scans pass in order, a uniform box test per scan, a lane per line, reject by
//    the line's box, hs_line_clip, an LDS atomic min on line << 1 | ends here plus the end-cell bit, the transition behind a
//    barrier, every cell stored once with its probability.  No global atomic, no wait on another workgroup.
#include "hs_blocks.h"
#include "hs_render.h"
#include "hs_scans.h"
#include "hs_tiles.h"
#include <algorithm>
#include <cmath>
#include <vector>

#define K25_LANES 256
#define K25_NONE 0xFFFFFFFFu
#define K25_BLOCK_MAX 32

struct k25_box { int x0, y0, x1, y1, bx, by, nv, da; };                    // per (scan, level); nv == 0: no valid line; nv < 0: a cell beyond the world bound; da: the largest
static_assert(sizeof(k25_box) == 32, "the record the kernels and the host read");
// a block of B x B cells whose first is window-frame cell (x0, y0) of `level`, cell (lx0, ly0) of the tile whose slot is `slot`
// (nullptr: no cell of the block outside the window is drawn)
struct k25_job { unsigned char *slot; int32_t x0, y0; int32_t level; uint16_t lx0, ly0; uint64_t pad; };
static_assert(sizeof(k25_job) == 32, "a job is two 16-byte words");
struct k25_level { int w, h; slamhip_cell *cells; float *prob; int base; int pad; };   // the window on this level: cells (0, 0) .. (w - 1, h - 1)
struct k25_arg {
    k25_level lv[HS_MAX_LEVELS]; int n_levels;
    int n_scans, keep, T; float lo_free, lo_occ;
    const float2 *pool; const k20_scan *scans; const sh_m3x2 *mats; k25_box *boxes; const k25_job *jobs;   // mats, boxes: [scan][level]
};

__global__ void __launch_bounds__(64) k25_boxes(const k25_arg A)
{
    const int k = (int)blockIdx.x / A.n_levels, lvl = (int)blockIdx.x - k * A.n_levels, lane = threadIdx.x;
    const k20_scan S = A.scans[k];
    const sh_m3x2 M = A.mats[(size_t)k * A.n_levels + lvl];
    int bx, by;
    hs_line_begin(S.ox, S.oy, M, &bx, &by);
    int x0 = 0x7fffffff, y0 = 0x7fffffff, x1 = -0x7fffffff, y1 = -0x7fffffff, nv = 0, da = 0;
    int far = (S.n > 0 && !hs_world_cell_ok(bx, by)) ? 1 : 0;             // (a scan of 0 points draws nothing: its begin cell is not asked)
    for (int i = lane; i < S.n; i += 64) {
        const float2 p = A.pool[S.off + i];
        int ex, ey;
        const hs_line ln = hs_line_make_world(p.x, p.y, M, bx, by, &ex, &ey);
        if (!hs_world_cell_ok(ex, ey)) far = 1;
        if (ln.flags & 1) { x0 = min(x0, ex); y0 = min(y0, ey); x1 = max(x1, ex); y1 = max(y1, ey); nv++; da = max(da, ln.da); }
    }
    for (int off = 32; off > 0; off >>= 1) {
        x0 = min(x0, __shfl_xor(x0, off, 64)); y0 = min(y0, __shfl_xor(y0, off, 64));
        x1 = max(x1, __shfl_xor(x1, off, 64)); y1 = max(y1, __shfl_xor(y1, off, 64));
        nv += __shfl_xor(nv, off, 64); da = max(da, __shfl_xor(da, off, 64)); far |= __shfl_xor(far, off, 64);
    }
    if (lane == 0) {
        k25_box B;
        B.nv = far ? -1 : nv; B.da = da; B.bx = bx; B.by = by;
        if (nv && !far) { B.x0 = min(x0, bx); B.y0 = min(y0, by); B.x1 = max(x1, bx); B.y1 = max(y1, by); }
        else { B.x0 = B.y0 = 1; B.x1 = B.y1 = 0; }
        A.boxes[(size_t)k * A.n_levels + lvl] = B;
    }
}

// where cell c of the job's block lives: the window's arrays inside the window's rectangle, else the tile's slot; false: nowhere
// (outside the window without a slot -- no line reaches such a cell, the host took a slot for every tile a box meets)
template <int B>
__device__ static __forceinline__ bool k25_cell_at(const k25_level &L, const k25_job &J, int T, int c, slamhip_cell **cell, float **prob)
{
    const int cx = c & (B - 1), cy = c / B;
    const int X = J.x0 + cx, Y = J.y0 + cy;
    if ((unsigned)X < (unsigned)L.w && (unsigned)Y < (unsigned)L.h) {
        const size_t g = (size_t)Y * L.w + X;
        *cell = L.cells + g; *prob = L.prob + g;
        return true;
    }
    if (!J.slot) return false;
    const size_t g = (size_t)(J.ly0 + cy) * T + (J.lx0 + cx);              // (< T * T: the host checks lx0 + B <= T and ly0 + B <= T)
    *cell = (slamhip_cell *)J.slot + g;
    *prob = (float *)(J.slot + k6p_slot_prob_offset((size_t)T * T)) + g;
    return true;
}

template <int B>
__global__ void __launch_bounds__(K25_LANES) k25_render(const k25_arg A)
{
    __shared__ float val_s[B * B];
    __shared__ int idx_s[B * B];
    __shared__ unsigned key_s[B * B];
    __shared__ unsigned end_s[(B * B + 31) / 32];
    const int tid = threadIdx.x;
    const k25_job J = A.jobs[blockIdx.x];
    const int lvl = J.level;
    const k25_level &L = A.lv[lvl];
    const int x0 = J.x0, y0 = J.y0, x1 = x0 + B - 1, y1 = y0 + B - 1;
    for (int c = tid; c < B * B; c += K25_LANES) {
        slamhip_cell cell = hs_reset_cell();
        slamhip_cell *pc; float *pp;
        if (A.keep && k25_cell_at<B>(L, J, A.T, c, &pc, &pp)) cell = *pc;
        val_s[c] = cell.value; idx_s[c] = cell.update_index; key_s[c] = K25_NONE;
    }
    if (tid < (B * B + 31) / 32) end_s[tid] = 0u;
    bool dirty = !A.keep;                                                  // (uniform: is the block to be stored?)
    __syncthreads();
    for (int k = 0; k < A.n_scans; k++) {
        const k25_box Bx = A.boxes[(size_t)k * A.n_levels + lvl];          // (uniform)
        if (Bx.nv <= 0 || Bx.x1 < x0 || Bx.x0 > x1 || Bx.y1 < y0 || Bx.y0 > y1) continue;
        const k20_scan S = A.scans[k];
        const sh_m3x2 M = A.mats[(size_t)k * A.n_levels + lvl];
        const int bx = Bx.bx, by = Bx.by;
        int touched = 0;
        for (int i = tid; i < S.n; i += K25_LANES) {
            const float2 p = A.pool[S.off + i];
            int ex, ey;
            const hs_line ln = hs_line_make_world(p.x, p.y, M, bx, by, &ex, &ey);
            if (!(ln.flags & 1) || ln.da > HS_LINE_MAX_DA) continue;       // (the host has refused a longer line: hs_line_clip's 32-bit proof)
            if (max(bx, ex) < x0 || min(bx, ex) > x1 || max(by, ey) < y0 || min(by, ey) > y1) continue;     // (the line's own box misses the block)
            const bool mx = (ln.flags & 2) != 0;
            const int smaj = ((ln.flags >> 2) & 3) - 1, smin = ln.sdb < 0 ? -1 : 1, da = ln.da, db = ln.sdb < 0 ? -ln.sdb : ln.sdb;
            const int bM = mx ? bx : by, bm = mx ? by : bx;
            const int tM0 = mx ? x0 : y0, tM1 = mx ? x1 : y1, tm0 = mx ? y0 : x0, tm1 = mx ? y1 : x1;
            const int A0 = smaj > 0 ? tM0 - bM : bM - tM1, A1 = smaj > 0 ? tM1 - bM : bM - tM0;
            const int B0 = smin > 0 ? tm0 - bm : bm - tm1, B1 = smin > 0 ? tm1 - bm : bm - tm0;
            int i0, i1;
            hs_line_clip(da, db, A0, A1, B0, B1, &i0, &i1);
            if (i0 > i1) continue;
            touched = 1;
            const int e = da / 2 + i0 * db;                                // (< 2^31: hs_line_clip)
            int m = e / da, r = e - m * da;
            for (int s = i0; s <= i1; s++) {
                const int cM = bM + smaj * s, cm = bm + smin * m;
                const int cx = (mx ? cM : cm) - x0, cy = (mx ? cm : cM) - y0;
                if ((unsigned)cx < (unsigned)B && (unsigned)cy < (unsigned)B) {    // (always, by hs_line_clip: the LDS arrays' own guard)
                    const int c = cy * B + cx;
                    if (s == da) { atomicMin(&key_s[c], ((unsigned)i << 1) | 1u); atomicOr(&end_s[c >> 5], 1u << (c & 31)); }
                    else atomicMin(&key_s[c], (unsigned)i << 1);
                }
                r += db;
                if (r >= da) { r -= da; m++; }                             // :231-235
            }
        }
        if (!__syncthreads_or(touched)) continue;                          // (uniform; no lane has written anything)
        dirty = true;
        const int mark_free = L.base + 3 * k + 1, mark_occ = L.base + 3 * k + 2;      // :116-117, :144
        for (int c = tid; c < B * B; c += K25_LANES) {
            const unsigned key = key_s[c];
            if (key == K25_NONE) continue;
            const bool ended = (end_s[c >> 5] >> (c & 31)) & 1u;
            float v = val_s[c]; int u = idx_s[c];
            const bool cross_first = !(key & 1u);                          // (k20_render's reading of the smallest key)
            hs_cell_transition(v, u, mark_free, mark_occ, cross_first ? 0 : 0x7fffffff, cross_first ? (ended ? 1 : 0x7fffffff) : 0, A.lo_free, A.lo_occ);
            val_s[c] = v; idx_s[c] = u; key_s[c] = K25_NONE;
            if (ended) atomicAnd(&end_s[c >> 5], ~(1u << (c & 31)));       // (this cell's own bit)
        }
        __syncthreads();
    }
    if (!dirty) return;
    for (int c = tid; c < B * B; c += K25_LANES) {
        slamhip_cell *pc; float *pp;
        if (!k25_cell_at<B>(L, J, A.T, c, &pc, &pp)) continue;
        slamhip_cell cell; cell.update_index = idx_s[c]; cell.value = val_s[c];
        *pc = cell;
#if HS_PROB_MODE == 0
        *pp = hs_prob_v(cell.value);
#endif
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------
// Tiles a render needs, as runs of one tile row: collected per box, then sorted and merged -- no table over the world, whose tile
// grid has up to 2^18 x 2^18 entries a level.
struct k25_run { int level; int64_t ty, tx0, tx1; };

static void k25_merge(std::vector<k25_run> &runs)
{
    std::sort(runs.begin(), runs.end(), [](const k25_run &a, const k25_run &b) {
        return a.level != b.level ? a.level < b.level : a.ty != b.ty ? a.ty < b.ty : a.tx0 < b.tx0;
    });
    size_t n = 0;
    for (const k25_run &r : runs) {
        if (n && runs[n - 1].level == r.level && runs[n - 1].ty == r.ty && r.tx0 <= runs[n - 1].tx1 + 1) runs[n - 1].tx1 = std::max(runs[n - 1].tx1, r.tx1);
        else runs[n++] = r;
    }
    runs.resize(n);
}

// the tile rows of the window-frame rectangle [x0, x1] x [y0, y1] of one level whose window cell (0, 0) is world cell (OX, OY)
static void k25_add_rect(std::vector<k25_run> &runs, int level, int64_t OX, int64_t OY, int x0, int y0, int x1, int y1, int T)
{
    const int64_t tx0 = bp_floor_div(OX + x0, T), tx1 = bp_floor_div(OX + x1, T);
    for (int64_t ty = bp_floor_div(OY + y0, T); ty <= bp_floor_div(OY + y1, T); ty++) runs.push_back({ level, ty, tx0, tx1 });
}

// What keeps the launch inside its arrays, checked against the handle and the directory, not against the code that wrote the table:
// a job's block lies in ONE tile, on the block grid; its slot is that tile's slot in the directory, or none.
static int32_t k25_check_jobs(const slamhip_hs *hs, const std::vector<k25_job> &jobs, int B)
{
    const hs_backing *bk = hs->bk;
    const int T = bk->T;
    for (const k25_job &j : jobs) {
        bool ok = j.level >= 0 && j.level < hs->n_levels && j.lx0 % B == 0 && j.ly0 % B == 0 && j.lx0 + B <= T && j.ly0 + B <= T &&
                  j.x0 >= -HS_WORLD_BOUND - 2 * T && j.x0 <= HS_WORLD_BOUND + 2 * T && j.y0 >= -HS_WORLD_BOUND - 2 * T && j.y0 <= HS_WORLD_BOUND + 2 * T;
        if (ok) {
            const int64_t X = (hs->win_ox >> j.level) + j.x0 - j.lx0, Y = (hs->win_oy >> j.level) + j.y0 - j.ly0;   // the tile's first world cell
            ok = bp_floor_div(X, T) * T == X && bp_floor_div(Y, T) * T == Y;
            if (ok && j.slot) ok = j.slot == bk->find(j.level, bp_floor_div(Y, T), bp_floor_div(X, T));
        }
        if (!ok) SH_FAIL(SLAMHIP_ERR_STATE, "slamhip_hs_render_world: the job table names a block outside its tile or a slot the directory does not hold (level %d)", j.level);
    }
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_render_world(slamhip_hs *hs, int32_t first, int32_t last, const float *poses, int32_t flags)
{
    SH_CHECK_ARG(hs);
    const int count = hs->scn ? (int)hs->scn->recs.size() : 0;
    int base[HS_MAX_LEVELS];
    for (int l = 0; l < hs->n_levels; l++) base[l] = hs->lv[l].curr_update_index;
    SH_TRY(k20_check("slamhip_hs_render_world", first, last, count, poses, flags, base, hs->n_levels));
    if (!hs->bk)
        SH_FAIL(SLAMHIP_ERR_INVALID, "slamhip_hs_render_world: backing is off (slamhip_hs_set_backing) -- there is no world behind the window; "
                "slamhip_hs_render draws the window alone");
    if (hs->ref_cache)
        SH_FAIL(SLAMHIP_ERR_INVALID, "slamhip_hs_render_world: the reference's cache is on (slamhip_hs_set_reference_cache) -- its literal stale entries have "
                "no meaning under an operation the reference lacks; turn it off first");
    const bool keep = (flags & SLAMHIP_RENDER_KEEP) != 0;
    const int N = last - first, NL = hs->n_levels;
    if (N == 0 && keep) return SLAMHIP_OK;
    slamhip_ctx *ctx = hs->ctx;
    hs_backing *bk = hs->bk;
    SH_TRY(hs_call_begin(hs));
    SH_TRY(hs_unit(&hs->scn));
    hs_scans *g = hs->scn;
    const int chunk = std::min(k20_chunk(), std::max(N, 1)), T = bk->T, B = std::min(T, K25_BLOCK_MAX), per = T / B;
    const size_t scan_bytes = sizeof(k20_scan) * (size_t)chunk, mat_bytes = sizeof(sh_m3x2) * (size_t)chunk * NL, box_bytes = sizeof(k25_box) * (size_t)chunk * NL;
    const size_t in_bytes = (scan_bytes + mat_bytes + 31) & ~(size_t)31;   // (boxes and jobs on 32-byte boundaries)
    k25_arg A;
    memset(&A, 0, sizeof(A));
    A.n_levels = NL; A.lo_free = hs->lo_free; A.lo_occ = hs->lo_occ; A.T = T;
    A.pool = g->d_pool;
    for (int l = 0; l < NL; l++) { const hs_level &L = hs->lv[l]; A.lv[l].w = L.w; A.lv[l].h = L.h; A.lv[l].cells = L.d_cells; A.lv[l].prob = L.d_prob; }
    // the blocks as they lie for `jobs` jobs: scans | matrices | boxes | jobs on the device; the same in the pinned block, the boxes
    // there being the ones read back
    auto lay = [&](size_t jobs) -> int32_t {
        const size_t all = in_bytes + box_bytes + sizeof(k25_job) * jobs;
        SH_TRY(hs_grow((void **)&g->d_in, &g->cap_in, all, HS_MEM_DEVICE, "slamhip_hs_render_world"));
        SH_TRY(hs_grow((void **)&g->h_io, &g->cap_h, all, HS_MEM_PINNED, "slamhip_hs_render_world"));
        A.scans = (const k20_scan *)g->d_in; A.mats = (const sh_m3x2 *)(g->d_in + scan_bytes);
        A.boxes = (k25_box *)(g->d_in + in_bytes); A.jobs = (const k25_job *)(g->d_in + in_bytes + box_bytes);
        return SLAMHIP_OK;
    };
    // a chunk's records and matrices to the device, and its boxes made
    auto stage = [&](int c0, int nc) -> int32_t {
        k20_scan *hr = (k20_scan *)g->h_io;
        sh_m3x2 *hm = (sh_m3x2 *)(g->h_io + scan_bytes);
        for (int k = 0; k < nc; k++) {
            hr[k] = g->recs[(size_t)(first + c0 + k)];
            for (int l = 0; l < NL; l++) hm[(size_t)k * NL + l] = k20_matrix(poses + 3 * (size_t)(c0 + k), hs->lv[l].stm);
        }
        A.n_scans = nc;
        SH_HIP(hipMemcpyAsync(g->d_in, g->h_io, scan_bytes + sizeof(sh_m3x2) * (size_t)nc * NL, hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(k25_boxes, dim3((unsigned)(nc * NL)), dim3(64), 0, ctx->stream, A);
        SH_HIP(hipGetLastError());
        return SLAMHIP_OK;
    };

    // ---- pass 1: the boxes of the whole range, read back; nothing is changed ------------------------------------------------------
    SH_TRY(lay(0));
    std::vector<k25_run> need;
    for (int c0 = 0; c0 < N; c0 += chunk) {
        const int nc = std::min(chunk, N - c0);
        SH_TRY(stage(c0, nc));
        const k25_box *hb = (const k25_box *)(g->h_io + in_bytes);
        SH_HIP(hipMemcpyAsync((void *)hb, A.boxes, sizeof(k25_box) * (size_t)nc * NL, hipMemcpyDeviceToHost, ctx->stream));
        SH_TRY(hs_call_finish(hs));
        for (int k = 0; k < nc; k++)
            for (int l = 0; l < NL; l++) {
                const k25_box &b = hb[(size_t)k * NL + l];
                if (b.nv < 0)
                    SH_FAIL(SLAMHIP_ERR_INVALID, "slamhip_hs_render_world: scan %d has a begin or end cell beyond +-2^20 cells of the window's cell (0, 0) on level %d",
                            first + c0 + k, l);
                if (b.nv > 0 && b.da > HS_LINE_MAX_DA)
                    SH_FAIL(SLAMHIP_ERR_INVALID, "slamhip_hs_render_world: scan %d has a line of %d cells on level %d, more than %d", first + c0 + k, b.da, l, HS_LINE_MAX_DA);
                if (b.nv > 0) k25_add_rect(need, l, hs->win_ox >> l, hs->win_oy >> l, b.x0, b.y0, b.x1, b.y1, T);
            }
    }
    k25_merge(need);

    // ---- the plan: the tiles to take, the jobs; still nothing is changed ------------------------------------------------------------
    // the tiles wholly under the window on a level: [wtx0, wtx1] x [wty0, wty1], empty where the window holds no whole tile
    int64_t wtx0[HS_MAX_LEVELS], wtx1[HS_MAX_LEVELS], wty0[HS_MAX_LEVELS], wty1[HS_MAX_LEVELS];
    for (int l = 0; l < NL; l++) {
        const int64_t OX = hs->win_ox >> l, OY = hs->win_oy >> l;
        wtx0[l] = bp_floor_div(OX + T - 1, T); wtx1[l] = bp_floor_div(OX + hs->lv[l].w, T) - 1;
        wty0[l] = bp_floor_div(OY + T - 1, T); wty1[l] = bp_floor_div(OY + hs->lv[l].h, T) - 1;
    }
    auto under_window = [&](int l, int64_t ty, int64_t tx) { return tx >= wtx0[l] && tx <= wtx1[l] && ty >= wty0[l] && ty <= wty1[l]; };
    uint64_t need_tiles = 0, win_tiles = 0;
    for (const k25_run &r : need) need_tiles += (uint64_t)(r.tx1 - r.tx0 + 1);
    for (int l = 0; l < NL; l++) win_tiles += (uint64_t)(sh_div_up(hs->lv[l].w, T) + 1) * (uint64_t)(sh_div_up(hs->lv[l].h, T) + 1);
    if (need_tiles > win_tiles + bk->max_bytes / bk->slot_bytes)          // (the tiles outside the window alone pass the pool's capacity: no need to name them)
        SH_FAIL(SLAMHIP_ERR_NOMEM, "slamhip_hs_render_world: the render needs about %llu tiles of %zu bytes, more than max_bytes = %llu holds",
                (unsigned long long)need_tiles, bk->slot_bytes, (unsigned long long)bk->max_bytes);
    std::vector<hs_tile_key> take;                                         // the tiles to take, (level, ty, tx) ascending: the runs' own order
    for (const k25_run &r : need)
        for (int64_t tx = r.tx0; tx <= r.tx1; tx++)
            if (!under_window(r.level, r.ty, tx) && !(keep && bk->find(r.level, r.ty, tx))) take.push_back(hs_tile_key(r.level, r.ty, tx));
    size_t at_hand = bk->free_slots.size();
    if (!keep) { at_hand = 0; for (const hs_bk_chunk &c : bk->chunks) at_hand += c.slots; }     // (the directory goes: every slot of the pool is free again)
    std::vector<k25_run> runs = need;                                      // the tiles whose blocks run: the needed ones, and without KEEP the window's (the clear)
    if (!keep) {
        for (int l = 0; l < NL; l++) k25_add_rect(runs, l, hs->win_ox >> l, hs->win_oy >> l, 0, 0, hs->lv[l].w - 1, hs->lv[l].h - 1, T);
        k25_merge(runs);
    }
    uint64_t max_jobs = 0;
    for (const k25_run &r : runs) max_jobs += (uint64_t)(r.tx1 - r.tx0 + 1) * (uint64_t)(per * per);
    if (max_jobs > (uint64_t)INT32_MAX) SH_FAIL(SLAMHIP_ERR_INVALID, "slamhip_hs_render_world: %llu blocks in one render", (unsigned long long)max_jobs);
    SH_TRY(lay((size_t)max_jobs));                                         // (the blocks' contents are gone: pass 2 stages every chunk again)
    if (take.size() > at_hand) SH_TRY(hs_bk_reserve(hs, take.size() - at_hand));      // SLAMHIP_ERR_NOMEM: max_bytes, or a chunk's allocation -- the pool as it was

    // ---- from here on the world changes --------------------------------------------------------------------------------------------
    if (!keep) hs_bk_reset(hs);                                            // rule 1: the directory goes (in stream order, ahead of the launches)
    for (const hs_tile_key &t : take)
        if (!bk->find_or_take(hs, std::get<0>(t), std::get<1>(t), std::get<2>(t)))
            SH_FAIL(SLAMHIP_ERR_STATE, "slamhip_hs_render_world: the pool gave no slot behind its own reserve");
    std::vector<k25_job> jobs;
    jobs.reserve((size_t)max_jobs);
    for (const k25_run &r : runs) {
        const hs_level &L = hs->lv[r.level];
        const int64_t OX = hs->win_ox >> r.level, OY = hs->win_oy >> r.level;
        for (int64_t tx = r.tx0; tx <= r.tx1; tx++) {
            unsigned char *slot = under_window(r.level, r.ty, tx) ? nullptr : bk->find(r.level, r.ty, tx);
            for (int by = 0; by < per; by++)
                for (int bx = 0; bx < per; bx++) {
                    k25_job j;
                    memset(&j, 0, sizeof(j));
                    j.slot = slot; j.level = r.level; j.lx0 = (uint16_t)(bx * B); j.ly0 = (uint16_t)(by * B);
                    j.x0 = (int32_t)(tx * T - OX + bx * B); j.y0 = (int32_t)(r.ty * T - OY + by * B);
                    const bool meets_window = j.x0 < L.w && j.x0 + B > 0 && j.y0 < L.h && j.y0 + B > 0;
                    if (slot || meets_window) jobs.push_back(j);            // (neither: a block of a window tile outside the window, nothing to draw or clear)
                }
        }
    }
    SH_TRY(k25_check_jobs(hs, jobs, B));
    if (!jobs.empty()) {
        unsigned char *hj = g->h_io + in_bytes + box_bytes;
        memcpy(hj, jobs.data(), sizeof(k25_job) * jobs.size());
        SH_HIP(hipMemcpyAsync((void *)A.jobs, hj, sizeof(k25_job) * jobs.size(), hipMemcpyHostToDevice, ctx->stream));
    }
    int cur_ui[HS_MAX_LEVELS], cur_ci[HS_MAX_LEVELS];
    for (int l = 0; l < NL; l++) { cur_ui[l] = keep ? hs->lv[l].curr_update_index : 0; cur_ci[l] = keep ? hs->lv[l].curr_cache_index : 0; }
    for (int c0 = 0; c0 < N || c0 == 0; c0 += chunk) {                     // (N == 0 without KEEP: one launch that clears)
        const int nc = std::min(chunk, N - c0);
        A.n_scans = nc; A.keep = (keep || c0 > 0) ? 1 : 0;                 // (a later chunk is a KEEP render of its own)
        for (int l = 0; l < NL; l++) A.lv[l].base = cur_ui[l];
        if (nc > 0) SH_TRY(stage(c0, nc));
        if (!jobs.empty()) {
            const dim3 grid((unsigned)jobs.size()), lanes(K25_LANES);
            if (B == 8) hipLaunchKernelGGL(k25_render<8>, grid, lanes, 0, ctx->stream, A);
            else if (B == 16) hipLaunchKernelGGL(k25_render<16>, grid, lanes, 0, ctx->stream, A);
            else hipLaunchKernelGGL(k25_render<32>, grid, lanes, 0, ctx->stream, A);
            SH_HIP(hipGetLastError());
        }
        for (int l = 0; l < NL; l++) {                                     // :144, :147 per scan; without KEEP from 0, as slamhip_hs_reset leaves them
            cur_ui[l] += 3 * nc; cur_ci[l] += nc;
            hs->lv[l].curr_update_index = cur_ui[l]; hs->lv[l].curr_cache_index = cur_ci[l];
        }
        SH_TRY(hs_call_finish(hs));
    }
    return SLAMHIP_OK;
}

// ---- CPU-side test hook: the definition over caller arrays, hs_render.h in plain loops ------------------------------------------------
// Line by line as the reference walks (Bresenham2D step by step), as slamhip_debug_render, under the world bound; the first walk
// only looks (what is refused leaves the arrays as they were), the second draws.
extern "C" int32_t slamhip_debug_render_world(int32_t n_levels, const int32_t *rects, float cell_length, slamhip_cell *cells, int32_t *update_index,
                                              int32_t *cache_index, float free_factor, float occ_factor, const float *xy, const int32_t *offsets,
                                              const float *origins, const float *poses, int32_t N, int32_t flags)
{
    SH_CHECK_ARG(rects && cells && update_index && cache_index && n_levels >= 1 && n_levels <= HS_MAX_LEVELS && cell_length > 0.0f && N >= 0 && N <= K20_MAX_SCANS);
    SH_CHECK_ARG(N == 0 || (offsets && origins && poses));
    for (int l = 0; l < n_levels; l++) {
        const int32_t *R = rects + 4 * l;
        SH_CHECK_ARG(R[2] >= 1 && R[3] >= 1 && (int64_t)R[2] * R[3] <= ((int64_t)1 << 26) && hs_world_cell_ok(R[0], R[1]) && hs_world_cell_ok(R[0] + R[2] - 1, R[1] + R[3] - 1));
    }
    if (N) {
        if (offsets[0] != 0) SH_FAIL(SLAMHIP_ERR_INVALID, "render world: offsets[0] = %d must be 0", offsets[0]);
        for (int k = 0; k < N; k++)
            if (offsets[k + 1] < offsets[k]) SH_FAIL(SLAMHIP_ERR_INVALID, "render world: offsets[%d] = %d below offsets[%d] = %d", k + 1, offsets[k + 1], k, offsets[k]);
        SH_CHECK_ARG(xy || offsets[N] == 0);
    }
    SH_TRY(k20_check("render world", 0, N, N, poses, flags, update_index, n_levels));
    const float lo_free = hs_prob_to_logodds(free_factor), lo_occ = hs_prob_to_logodds(occ_factor);
    for (int draw = 0; draw < 2; draw++) {
        float res = cell_length;
        slamhip_cell *C = cells;
        for (int l = 0; l < n_levels; l++) {
            const int X0 = rects[4 * l], Y0 = rects[4 * l + 1], w = rects[4 * l + 2], h = rects[4 * l + 3];
            const float stm = 1.0f / res;                                  // MapProperties.cs:32, as slamhip_hs_create forms it
            int ui = update_index[l];
            if (draw && !(flags & SLAMHIP_RENDER_KEEP)) {
                for (size_t i = 0; i < (size_t)w * h; i++) C[i] = hs_reset_cell();
                ui = 0; cache_index[l] = 0;
            }
            for (int k = 0; k < N; k++) {
                const int mark_free = ui + 1, mark_occ = ui + 2;           // :116-117
                const sh_m3x2 M = k20_matrix(poses + 3 * (size_t)k, stm);
                int bx, by;
                hs_line_begin(origins[2 * k], origins[2 * k + 1], M, &bx, &by);
                if (!draw && offsets[k + 1] > offsets[k] && !hs_world_cell_ok(bx, by))
                    SH_FAIL(SLAMHIP_ERR_INVALID, "render world: scan %d's begin cell lies beyond +-2^20 cells on level %d", k, l);
                for (int i = offsets[k]; i < offsets[k + 1]; i++) {        // :130
                    int ex, ey;
                    const hs_line ln = hs_line_make_world(xy[2 * (size_t)i], xy[2 * (size_t)i + 1], M, bx, by, &ex, &ey);
                    if (!draw) {
                        if (!hs_world_cell_ok(ex, ey)) SH_FAIL(SLAMHIP_ERR_INVALID, "render world: point %d of scan %d ends beyond +-2^20 cells on level %d", i - offsets[k], k, l);
                        if (!(ln.flags & 1)) continue;
                        if (ln.da > HS_LINE_MAX_DA) SH_FAIL(SLAMHIP_ERR_INVALID, "render world: a line of %d cells in scan %d on level %d, more than %d", ln.da, k, l, HS_LINE_MAX_DA);
                        if (bx < X0 || by < Y0 || bx >= X0 + w || by >= Y0 + h || ex < X0 || ey < Y0 || ex >= X0 + w || ey >= Y0 + h)
                            SH_FAIL(SLAMHIP_ERR_INVALID, "render world: scan %d's box leaves the rectangle of level %d", k, l);
                        continue;
                    }
                    if (!(ln.flags & 1)) continue;
                    const bool mx = (ln.flags & 2) != 0;
                    const int smaj = ((ln.flags >> 2) & 3) - 1, smin = sh_sign(ln.sdb), da = ln.da, db = ln.sdb < 0 ? -ln.sdb : ln.sdb;
                    const int step_a = mx ? smaj : smaj * w, step_b = mx ? smin * w : smin;
                    int offset = (by - Y0) * w + (bx - X0), error_b = da / 2; // :175-185
                    for (int s = 0; s < da; s++) {                         // :222-238: da free cells, the end cell excluded
                        slamhip_cell &c = C[offset];
                        if (c.update_index < mark_free) { c.value += lo_free; c.update_index = mark_free; }     // :192-199
                        offset += step_a;
                        error_b += db;
                        if (error_b >= da) { offset += step_b; error_b -= da; }                                 // :231-235
                    }
                    slamhip_cell &c = C[(ey - Y0) * w + (ex - X0)];        // :187-189
                    if (c.update_index < mark_occ) {                       // :201-218
                        if (c.update_index == mark_free) c.value -= lo_free;
                        if (c.value < 50.0f) c.value += lo_occ;
                        c.update_index = mark_occ;
                    }
                }
                ui += 3;                                                   // :144
                if (draw) cache_index[l]++;                                // :147
            }
            if (draw) update_index[l] = ui;
            C += (size_t)w * h;
            res *= 2.0f;                                                   // MapRepMultiMap.cs:56
        }
    }
    return SLAMHIP_OK;
}
