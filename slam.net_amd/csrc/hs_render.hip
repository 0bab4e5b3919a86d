// hs_render.hip -- K20, the occupancy pyramid drawn again from stored scans at poses given per scan, and the store of keyframe
// scans it draws from (slamhip_hs_scans_add, _scans_count, _scans_info, _scans_download, _scans_clear, slamhip_hs_render,
// slamhip_debug_render, slamhip_debug_render_clip).  No reference counterpart: the result is DEFINED as what the reference's
// sequential UpdateByScan calls leave (include/slamhip.h, slamhip_hs_render); the arithmetic host and device share: hs_render.h.
//
// The store: ONE device pool of points (float2), grown by doubling with the front copied as it is; the per-scan records -- offset,
// count, origin -- live on the host and travel with each launch's matrices.
//  * k20_boxes: a wavefront per (scan, level): the begin cell, the number of valid lines and the box of the begin cell and the valid
//    end cells, 16 bytes.  No line record is ever written to memory: the tile kernel makes a line again from its point and matrix.
//  * k20_render<T>: a workgroup of 256 lanes per tile of T x T cells of one level, all levels in one grid.  The tile's cells (value,
//    update index) stay in LDS for the whole launch; the scans pass over it IN ORDER.  A scan whose box misses the tile costs one
//    uniform test.  Otherwise a lane per line clips its line to the tile (hs_line_clip: one interval of steps, integers only) and
//    leaves, per step, key = line index << 1 | (1 for the line's end cell) in the cell's scratch word by an LDS atomic min, and for
//    an end cell a bit in the tile's "ended in" words by an LDS atomic or.  (The issue's other form -- two atomic mins, the smallest
//    crossing and the smallest ending index -- costs a second word per cell and a second atomic per step.  The smallest key tells
//    which kind of line touched the cell FIRST, which is all the free transition asks; the bit tells whether the occupied
//    transition takes place at all.)  Behind a barrier a lane per cell applies hs_cell_transition with that scan's marks and rests
//    the scratch; behind another the next scan follows.  At the end every cell of the tile is stored ONCE, with its probability.
//    No global atomic, no wait on another workgroup: a cell has one writer.
#include "hs_blocks.h"
#include "hs_render.h"
#include "hs_scans.h"
#include <algorithm>
#include <cmath>
#include <vector>

#define K20_LANES 256
#define K20_NONE 0xFFFFFFFFu

static_assert(SLAMHIP_RENDER_KEEP == 1, "the flag of include/slamhip.h");

struct k20_box { short x0, y0, x1, y1, bx, by; int nv; };                  // per (scan, level); nv == 0: no valid line, the rest is not read
static_assert(sizeof(k20_box) == 16, "the record the kernels read");       // (k20_scan, a stored scan's record: hs_scans.h)

struct k20_level { int w, h; slamhip_cell *cells; float *prob; int base; int tiles_x, tile0; };    // base: the level's update index in front of the launch's first scan
struct k20_arg {
    k20_level lv[HS_MAX_LEVELS]; int n_levels;
    int n_scans, keep; float lo_free, lo_occ;
    const float2 *pool; const k20_scan *scans; const sh_m3x2 *mats; k20_box *boxes;    // mats, boxes: [scan][level]
};

__global__ void __launch_bounds__(64) k20_boxes(const k20_arg A)
{
    const int k = (int)blockIdx.x / A.n_levels, lvl = (int)blockIdx.x - k * A.n_levels, lane = threadIdx.x;
    const k20_level &L = A.lv[lvl];
    const k20_scan S = A.scans[k];
    const sh_m3x2 M = A.mats[(size_t)k * A.n_levels + lvl];
    int bx, by;
    hs_line_begin(S.ox, S.oy, M, &bx, &by);
    int x0 = 0x7fffffff, y0 = 0x7fffffff, x1 = -1, y1 = -1, nv = 0;
    for (int i = lane; i < S.n; i += 64) {
        const float2 p = A.pool[S.off + i];
        int ex, ey;
        const hs_line ln = hs_line_make(p.x, p.y, M, bx, by, L.w, L.h, &ex, &ey);
        if (ln.flags & 1) { x0 = min(x0, ex); y0 = min(y0, ey); x1 = max(x1, ex); y1 = max(y1, ey); nv++; }
    }
    for (int off = 32; off > 0; off >>= 1) {
        x0 = min(x0, __shfl_xor(x0, off, 64)); y0 = min(y0, __shfl_xor(y0, off, 64));
        x1 = max(x1, __shfl_xor(x1, off, 64)); y1 = max(y1, __shfl_xor(y1, off, 64));
        nv += __shfl_xor(nv, off, 64);
    }
    if (lane == 0) {
        k20_box B;
        B.nv = nv;
        if (nv) {                                                          // (a valid line's begin cell lies inside the level: every value is below 32768)
            B.x0 = (short)min(x0, bx); B.y0 = (short)min(y0, by); B.x1 = (short)max(x1, bx); B.y1 = (short)max(y1, by);
            B.bx = (short)bx; B.by = (short)by;
        } else { B.x0 = B.y0 = 1; B.x1 = B.y1 = 0; B.bx = B.by = 0; }
        A.boxes[(size_t)k * A.n_levels + lvl] = B;
    }
}

template <int T>
__global__ void __launch_bounds__(K20_LANES) k20_render(const k20_arg A)
{
    __shared__ float val_s[T * T];
    __shared__ int idx_s[T * T];
    __shared__ unsigned key_s[T * T];
    __shared__ unsigned end_s[T * T / 32];
    const int tid = threadIdx.x;
    int lvl = 0;
    for (int l = 1; l < A.n_levels; l++) if ((int)blockIdx.x >= A.lv[l].tile0) lvl = l;
    const k20_level &L = A.lv[lvl];
    const int t = (int)blockIdx.x - L.tile0, ty = t / L.tiles_x, tx = t - ty * L.tiles_x;
    const int x0 = tx * T, y0 = ty * T, x1 = min(x0 + T, L.w) - 1, y1 = min(y0 + T, L.h) - 1;      // the tile's cells inside the level
    for (int c = tid; c < T * T; c += K20_LANES) {
        const int X = x0 + (c & (T - 1)), Y = y0 + c / T;
        slamhip_cell cell = hs_reset_cell();
        if (A.keep && X <= x1 && Y <= y1) cell = L.cells[(size_t)Y * L.w + X];
        val_s[c] = cell.value; idx_s[c] = cell.update_index; key_s[c] = K20_NONE;
    }
    if (tid < T * T / 32) end_s[tid] = 0u;
    bool dirty = !A.keep;                                                  // (uniform: is the tile to be stored?)
    __syncthreads();
    for (int k = 0; k < A.n_scans; k++) {
        const k20_box B = A.boxes[(size_t)k * A.n_levels + lvl];           // (uniform)
        if (B.nv == 0 || B.x1 < x0 || B.x0 > x1 || B.y1 < y0 || B.y0 > y1) continue;
        const k20_scan S = A.scans[k];
        const sh_m3x2 M = A.mats[(size_t)k * A.n_levels + lvl];
        const int bx = B.bx, by = B.by;
        int touched = 0;
        for (int i = tid; i < S.n; i += K20_LANES) {
            const float2 p = A.pool[S.off + i];
            int ex, ey;
            const hs_line ln = hs_line_make(p.x, p.y, M, bx, by, L.w, L.h, &ex, &ey);
            if (!(ln.flags & 1)) continue;
            if (max(bx, ex) < x0 || min(bx, ex) > x1 || max(by, ey) < y0 || min(by, ey) > y1) continue;     // (the line's own box misses the tile)
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
                if ((unsigned)cx < (unsigned)T && (unsigned)cy < (unsigned)T) {    // (always, by hs_line_clip: the LDS arrays' own guard)
                    const int c = cy * T + cx;
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
        for (int c = tid; c < T * T; c += K20_LANES) {
            const unsigned key = key_s[c];
            if (key == K20_NONE) continue;
            const bool ended = (end_s[c >> 5] >> (c & 31)) & 1u;
            float v = val_s[c]; int u = idx_s[c];
            // first touched by a crossing line: the free transition, then the occupied one if a line ends here at all;
            // first touched by an ending line: the occupied transition alone
            const bool cross_first = !(key & 1u);
            hs_cell_transition(v, u, mark_free, mark_occ, cross_first ? 0 : 0x7fffffff, cross_first ? (ended ? 1 : 0x7fffffff) : 0, A.lo_free, A.lo_occ);
            val_s[c] = v; idx_s[c] = u; key_s[c] = K20_NONE;
            if (ended) atomicAnd(&end_s[c >> 5], ~(1u << (c & 31)));       // (this cell's own bit: the word's other cells belong to other lanes)
        }
        __syncthreads();
    }
    if (!dirty) return;
    for (int c = tid; c < T * T; c += K20_LANES) {
        const int X = x0 + (c & (T - 1)), Y = y0 + c / T;
        if (X > x1 || Y > y1) continue;
        const size_t g = (size_t)Y * L.w + X;
        slamhip_cell cell; cell.update_index = idx_s[c]; cell.value = val_s[c];
        L.cells[g] = cell;
#if HS_PROB_MODE == 0
        L.prob[g] = hs_prob_v(cell.value);
#endif
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------
// What the unit keeps: struct hs_scans, hs_scans.h (K21 reads the pool and the records).

void hs_scn_free(slamhip_hs *hs)
{
    hs_scans *g = hs->scn;
    if (!g) return;
    hs_release((void **)&g->d_pool, nullptr, HS_MEM_DEVICE);
    hs_release((void **)&g->d_in, &g->cap_in, HS_MEM_DEVICE);
    hs_release((void **)&g->h_io, &g->cap_h, HS_MEM_PINNED);
    delete g;
    hs->scn = nullptr;
}

void hs_scn_reset(slamhip_hs *hs)
{
    if (!hs->scn) return;
    hs->scn->recs.clear();
    hs->scn->used_pts = 0;
}

// room for `pts` points: a larger pool is a new allocation whose front is the old one (the rule of hs_sg_reserve)
static int32_t hs_scn_reserve(slamhip_hs *hs, size_t pts)
{
    hs_scans *g = hs->scn;
    if (pts <= g->cap_pts) return SLAMHIP_OK;
    static const long long first_cap = std::max(1ll, sh_env_int("SLAMHIP_K20_POOL_POINTS", 1 << 16));     // (tests: growth within a few scans)
    const size_t cap = std::max(std::max(pts, 2 * g->cap_pts), (size_t)first_cap);
    float2 *np = nullptr;
    size_t c0 = 0;
    SH_TRY(hs_grow((void **)&np, &c0, sizeof(float2) * cap, HS_MEM_DEVICE, "scan store"));
    hipStream_t st = hs->ctx->stream;
    hipError_t e = hipSuccess;
    if (g->used_pts) e = hipMemcpyAsync(np, g->d_pool, sizeof(float2) * g->used_pts, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);                     // (the old pool is idle behind it)
    if (e != hipSuccess) { (void)hipFree(np); SH_HIP(e); }
    hs_release((void **)&g->d_pool, nullptr, HS_MEM_DEVICE);
    g->d_pool = np; g->cap_pts = cap;
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_scans_add(slamhip_hs *hs, const float *xy, int32_t n_points, const float scan_origin[2], int32_t *out_index)
{
    SH_CHECK_ARG(hs);
    const bool own = xy == nullptr;                                        // the scan that is set on the handle (n_points, scan_origin: not read)
    if (!own) SH_CHECK_ARG(n_points >= 0);
    if (hs->scn && hs->scn->recs.size() >= (size_t)K20_MAX_SCANS) SH_FAIL(SLAMHIP_ERR_INVALID, "scan store: it holds 2^20 scans");
    SH_TRY(hs_call_begin(hs));
    SH_TRY(hs_unit(&hs->scn));
    hs_scans *g = hs->scn;
    const int n = own ? hs->n_points : n_points;
    k20_scan R;
    R.off = (long long)g->used_pts; R.n = n; R.pad = 0;
    R.ox = own ? hs->origin[0] : scan_origin ? scan_origin[0] : 0.0f;
    R.oy = own ? hs->origin[1] : scan_origin ? scan_origin[1] : 0.0f;
    if (n > 0) {
        SH_TRY(hs_scn_reserve(hs, g->used_pts + (size_t)n));
        const size_t bytes = sizeof(float2) * (size_t)n;
        if (own) {
            SH_TRY(hs_flush_scan(hs));
            SH_HIP(hipMemcpyAsync(g->d_pool + g->used_pts, hs->d_pts, bytes, hipMemcpyDeviceToDevice, hs->ctx->stream));
        } else {
            SH_TRY(hs_grow((void **)&g->h_io, &g->cap_h, bytes, HS_MEM_PINNED, "scan store"));
            memcpy(g->h_io, xy, bytes);
            SH_HIP(hipMemcpyAsync(g->d_pool + g->used_pts, g->h_io, bytes, hipMemcpyHostToDevice, hs->ctx->stream));
        }
    }
    SH_TRY(hs_call_finish(hs));                                            // (a scan of 0 points too: the frame is closed as it was opened)
    if (out_index) *out_index = (int32_t)g->recs.size();
    g->recs.push_back(R);
    g->used_pts += (size_t)n;
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_scans_count(slamhip_hs *hs, int32_t *out_count)
{
    SH_CHECK_ARG(hs && out_count);
    *out_count = hs->scn ? (int32_t)hs->scn->recs.size() : 0;
    return SLAMHIP_OK;
}

static int32_t hs_scn_index(const slamhip_hs *hs, const char *who, int32_t k)
{
    const int count = hs->scn ? (int)hs->scn->recs.size() : 0;
    if (k < 0 || k >= count) SH_FAIL(SLAMHIP_ERR_INVALID, "%s: scan %d of %d", who, k, count);
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_scans_info(slamhip_hs *hs, int32_t k, int32_t *out_n, float out_origin[2])
{
    SH_CHECK_ARG(hs);
    SH_TRY(hs_scn_index(hs, "scan store info", k));
    const k20_scan &R = hs->scn->recs[(size_t)k];
    if (out_n) *out_n = R.n;
    if (out_origin) { out_origin[0] = R.ox; out_origin[1] = R.oy; }
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_scans_download(slamhip_hs *hs, int32_t k, float *out_xy, int32_t cap)
{
    SH_CHECK_ARG(hs);
    SH_TRY(hs_scn_index(hs, "scan store download", k));
    hs_scans *g = hs->scn;
    const k20_scan R = g->recs[(size_t)k];
    if (cap < R.n) SH_FAIL(SLAMHIP_ERR_INVALID, "scan store download: room for %d points, scan %d holds %d", cap, k, R.n);
    if (R.n == 0) return SLAMHIP_OK;
    SH_CHECK_ARG(out_xy);
    SH_TRY(hs_call_begin(hs));
    const size_t bytes = sizeof(float2) * (size_t)R.n;
    SH_TRY(hs_grow((void **)&g->h_io, &g->cap_h, bytes, HS_MEM_PINNED, "scan store download"));
    SH_HIP(hipMemcpyAsync(g->h_io, g->d_pool + R.off, bytes, hipMemcpyDeviceToHost, hs->ctx->stream));
    SH_TRY(hs_call_finish(hs));
    memcpy(out_xy, g->h_io, bytes);
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_scans_clear(slamhip_hs *hs)
{
    SH_CHECK_ARG(hs);
    if (!hs->scn) return SLAMHIP_OK;
    SH_TRY(hs_call_begin(hs));
    SH_TRY(hs_call_finish(hs));                                            // (the blocks are idle behind it)
    hs_scn_free(hs);
    return SLAMHIP_OK;
}

static int k20_tile()       // T: 32, or 64 by SLAMHIP_K20_TILE=64 (both are built; DESIGN.md section 4 "K20")
{
    static const int v = sh_env_int("SLAMHIP_K20_TILE", 32) == 64 ? 64 : 32;
    return v;
}
// (k20_matrix, k20_check, k20_chunk: hs_render.h -- K25 forms its matrices, refuses and cuts its range by the same text)

extern "C" int32_t slamhip_hs_render(slamhip_hs *hs, int32_t first, int32_t last, const float *poses, int32_t flags)
{
    SH_CHECK_ARG(hs);
    const int count = hs->scn ? (int)hs->scn->recs.size() : 0;
    int base[HS_MAX_LEVELS];
    for (int l = 0; l < hs->n_levels; l++) base[l] = hs->lv[l].curr_update_index;
    SH_TRY(k20_check("slamhip_hs_render", first, last, count, poses, flags, base, hs->n_levels));
    if (hs->ref_cache)
        SH_FAIL(SLAMHIP_ERR_INVALID, "slamhip_hs_render: the reference's cache is on (slamhip_hs_set_reference_cache) -- its literal stale entries have "
                "no meaning under an operation the reference lacks; turn it off first");
    const bool keep = (flags & SLAMHIP_RENDER_KEEP) != 0;
    const int N = last - first, NL = hs->n_levels;
    if (N == 0 && keep) return SLAMHIP_OK;
    slamhip_ctx *ctx = hs->ctx;
    SH_TRY(hs_call_begin(hs));
    SH_TRY(hs_unit(&hs->scn));
    hs_scans *g = hs->scn;
    const int chunk = std::min(k20_chunk(), std::max(N, 1)), T = k20_tile();
    const size_t scan_bytes = sizeof(k20_scan) * (size_t)chunk, mat_bytes = sizeof(sh_m3x2) * (size_t)chunk * NL, box_bytes = sizeof(k20_box) * (size_t)chunk * NL;
    SH_TRY(hs_grow((void **)&g->d_in, &g->cap_in, scan_bytes + mat_bytes + box_bytes, HS_MEM_DEVICE, "slamhip_hs_render"));
    SH_TRY(hs_grow((void **)&g->h_io, &g->cap_h, scan_bytes + mat_bytes, HS_MEM_PINNED, "slamhip_hs_render"));
    // The indices as they will stand, kept beside the handle's: the handle's own, and the backing directory, change only behind a
    // launch that went into the stream (a call refused or failed before that leaves everything as it was).
    int cur_ui[HS_MAX_LEVELS], cur_ci[HS_MAX_LEVELS];
    for (int l = 0; l < NL; l++) { cur_ui[l] = keep ? hs->lv[l].curr_update_index : 0; cur_ci[l] = keep ? hs->lv[l].curr_cache_index : 0; }
    k20_arg A;
    memset(&A, 0, sizeof(A));
    A.n_levels = NL; A.lo_free = hs->lo_free; A.lo_occ = hs->lo_occ;
    A.pool = g->d_pool;
    A.scans = (const k20_scan *)g->d_in; A.mats = (const sh_m3x2 *)(g->d_in + scan_bytes); A.boxes = (k20_box *)(g->d_in + scan_bytes + mat_bytes);
    int tiles = 0;
    for (int l = 0; l < NL; l++) {
        const hs_level &L = hs->lv[l];
        A.lv[l].w = L.w; A.lv[l].h = L.h; A.lv[l].cells = L.d_cells; A.lv[l].prob = L.d_prob;
        A.lv[l].tiles_x = sh_div_up(L.w, T); A.lv[l].tile0 = tiles;
        tiles += A.lv[l].tiles_x * sh_div_up(L.h, T);                      // (at most 1024 x 1024 per level)
    }
    for (int c0 = 0; c0 < N || c0 == 0; c0 += chunk) {                     // (N == 0 without KEEP: one launch that clears)
        const int nc = std::min(chunk, N - c0);
        k20_scan *hr = (k20_scan *)g->h_io;
        sh_m3x2 *hm = (sh_m3x2 *)(g->h_io + scan_bytes);
        for (int k = 0; k < nc; k++) {
            hr[k] = g->recs[(size_t)(first + c0 + k)];
            for (int l = 0; l < NL; l++) hm[(size_t)k * NL + l] = k20_matrix(poses + 3 * (size_t)(c0 + k), hs->lv[l].stm);
        }
        A.n_scans = nc; A.keep = (keep || c0 > 0) ? 1 : 0;                 // (a later chunk is a KEEP render of its own)
        for (int l = 0; l < NL; l++) A.lv[l].base = cur_ui[l];
        if (nc > 0) {
            SH_HIP(hipMemcpyAsync(g->d_in, g->h_io, scan_bytes + sizeof(sh_m3x2) * (size_t)nc * NL, hipMemcpyHostToDevice, ctx->stream));
            hipLaunchKernelGGL(k20_boxes, dim3((unsigned)(nc * NL)), dim3(64), 0, ctx->stream, A);
            SH_HIP(hipGetLastError());
        }
        if (T == 64) hipLaunchKernelGGL(k20_render<64>, dim3((unsigned)tiles), dim3(K20_LANES), 0, ctx->stream, A);
        else hipLaunchKernelGGL(k20_render<32>, dim3((unsigned)tiles), dim3(K20_LANES), 0, ctx->stream, A);
        SH_HIP(hipGetLastError());
        if (!keep && c0 == 0 && hs->bk) hs_bk_reset(hs);                   // rule 1: the directory goes with the map it belonged to (in stream order, behind the launch)
        for (int l = 0; l < NL; l++) {                                     // :144, :147 per scan; without KEEP from 0, as slamhip_hs_reset leaves them
            cur_ui[l] += 3 * nc; cur_ci[l] += nc;
            hs->lv[l].curr_update_index = cur_ui[l]; hs->lv[l].curr_cache_index = cur_ci[l];
        }
        SH_TRY(hs_call_finish(hs));                                        // (the staging block is the next chunk's; a wait that times out poisons the context)
    }
    return SLAMHIP_OK;
}

// ---- CPU-side test hooks: hs_render.h -- the text the kernels run -- in plain loops ----------------------------------------------------
extern "C" int32_t slamhip_debug_render_clip(int32_t da, int32_t db, int32_t T, int32_t n, const int32_t *a0, const int32_t *b0, int32_t *out_i0, int32_t *out_i1)
{
    SH_CHECK_ARG(a0 && b0 && out_i0 && out_i1 && n >= 0);
    if (da < 1 || da > 32767 || db < 0 || db > da || T < 1 || T > 32768)
        SH_FAIL(SLAMHIP_ERR_INVALID, "render clip: da = %d in [1, 32767], db = %d in [0, da], T = %d in [1, 32768]", da, db, T);
    for (int i = 0; i < n; i++) {
        if (a0[i] < -65536 || a0[i] > 65536 || b0[i] < -65536 || b0[i] > 65536) SH_FAIL(SLAMHIP_ERR_INVALID, "render clip: window %d lies beyond +-65536", i);
        hs_line_clip(da, db, a0[i], a0[i] + T - 1, b0[i], b0[i] + T - 1, out_i0 + i, out_i1 + i);
    }
    return SLAMHIP_OK;
}

// The definition itself, line by line as the reference walks (UpdateLineBresenhami :155-190, Bresenham2D :220-239) -- NOT the closed
// form the kernel clips by: the two are two statements of one rule.
extern "C" int32_t slamhip_debug_render(int32_t n_levels, const int32_t *dims, float cell_length, slamhip_cell *cells, int32_t *update_index, int32_t *cache_index,
                                        float free_factor, float occ_factor, const float *xy, const int32_t *offsets, const float *origins, const float *poses,
                                        int32_t N, int32_t flags)
{
    SH_CHECK_ARG(dims && cells && update_index && cache_index && n_levels >= 1 && n_levels <= HS_MAX_LEVELS && cell_length > 0.0f && N >= 0 && N <= K20_MAX_SCANS);
    SH_CHECK_ARG(N == 0 || (offsets && origins && poses));
    for (int l = 0; l < n_levels; l++) SH_CHECK_ARG(dims[2 * l] >= 1 && dims[2 * l + 1] >= 1 && dims[2 * l] <= 32768 && dims[2 * l + 1] <= 32768);
    if (N) {
        if (offsets[0] != 0) SH_FAIL(SLAMHIP_ERR_INVALID, "render: offsets[0] = %d must be 0", offsets[0]);
        for (int k = 0; k < N; k++)
            if (offsets[k + 1] < offsets[k]) SH_FAIL(SLAMHIP_ERR_INVALID, "render: offsets[%d] = %d below offsets[%d] = %d", k + 1, offsets[k + 1], k, offsets[k]);
        SH_CHECK_ARG(xy || offsets[N] == 0);
    }
    SH_TRY(k20_check("render", 0, N, N, poses, flags, update_index, n_levels));
    const float lo_free = hs_prob_to_logodds(free_factor), lo_occ = hs_prob_to_logodds(occ_factor);
    float res = cell_length;
    slamhip_cell *C = cells;
    for (int l = 0; l < n_levels; l++) {
        const int w = dims[2 * l], h = dims[2 * l + 1];
        const float stm = 1.0f / res;                                      // MapProperties.cs:32, as slamhip_hs_create forms it
        if (!(flags & SLAMHIP_RENDER_KEEP)) {
            for (size_t i = 0; i < (size_t)w * h; i++) C[i] = hs_reset_cell();
            update_index[l] = 0; cache_index[l] = 0;
        }
        for (int k = 0; k < N; k++) {
            const int mark_free = update_index[l] + 1, mark_occ = update_index[l] + 2;      // :116-117
            const sh_m3x2 M = k20_matrix(poses + 3 * (size_t)k, stm);
            int bx, by;
            hs_line_begin(origins[2 * k], origins[2 * k + 1], M, &bx, &by);
            for (int i = offsets[k]; i < offsets[k + 1]; i++) {           // :130
                int ex, ey;
                const hs_line ln = hs_line_make(xy[2 * (size_t)i], xy[2 * (size_t)i + 1], M, bx, by, w, h, &ex, &ey);
                if (!(ln.flags & 1)) continue;
                const bool mx = (ln.flags & 2) != 0;
                const int smaj = ((ln.flags >> 2) & 3) - 1, smin = sh_sign(ln.sdb), da = ln.da, db = ln.sdb < 0 ? -ln.sdb : ln.sdb;
                const int step_a = mx ? smaj : smaj * w, step_b = mx ? smin * w : smin;
                int offset = by * w + bx, error_b = da / 2;               // :175-185
                for (int s = 0; s < da; s++) {                             // :222-238: da free cells, the end cell excluded
                    slamhip_cell &c = C[offset];
                    if (c.update_index < mark_free) { c.value += lo_free; c.update_index = mark_free; }     // :192-199
                    offset += step_a;
                    error_b += db;
                    if (error_b >= da) { offset += step_b; error_b -= da; }                                 // :231-235
                }
                slamhip_cell &c = C[ey * w + ex];                          // :187-189
                if (c.update_index < mark_occ) {                           // :201-218
                    if (c.update_index == mark_free) c.value -= lo_free;
                    if (c.value < 50.0f) c.value += lo_occ;
                    c.update_index = mark_occ;
                }
            }
            update_index[l] += 3;                                          // :144
            cache_index[l]++;                                              // :147
        }
        C += (size_t)w * h;
        res *= 2.0f;                                                       // MapRepMultiMap.cs:56
    }
    return SLAMHIP_OK;
}
