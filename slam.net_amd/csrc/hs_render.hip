// hs_render.hip -- K20, the occupancy pyramid drawn again from stored scans at poses given per scan, and the store of keyframe
// scans it draws from (slamhip_hs_scans_add, _scans_count, _scans_info, _scans_download, _scans_clear, slamhip_hs_render,
// slamhip_debug_render, slamhip_debug_render_clip).  No reference counterpart: the result is DEFINED as what the reference's
// sequential UpdateByScan calls leave (include/slamhip.h, slamhip_hs_render).
//
// The store: ONE device pool of points (float2), grown by doubling with the front copied as it is; the per-scan records -- offset,
// count, origin -- live on the host and travel with each launch's matrices.
// The render is hs_render.h's, which K25 (hs_render_world.hip) shares: the line, the boxes kernel under a level's bound, the body of
// the block kernel, the chunk frame, the hook's walk.  K20's own: k20_render<T>, a workgroup per tile of T x T cells of one level, all
// levels in one grid -- the tile is found from the block index, its cells lie row-major in the level's arrays, and what of it lies
// beyond the level's w x h is nowhere; the tile count per level; and the backing directory dropped behind the first launch.
#include "hs_render.h"
#include <vector>

static_assert(SLAMHIP_RENDER_KEEP == 1, "the flag of include/slamhip.h");

struct k20_level : hs_render_level { int tiles_x, tile0; };                // (k20_scan, a stored scan's record: hs_scans.h)
struct k20_arg {
    hs_render_args<hs_box16> P; k20_level lv[HS_MAX_LEVELS];
    __device__ hs_bound_level bound(int l) const { return { lv[l].w, lv[l].h }; }
};

// cell c of the tile whose cells inside the level are [x0, x1] x [y0, y1]: row-major in the level's arrays
template <int T>
struct k20_cells {
    const k20_level &L; int x0, y0, x1, y1;
    __device__ __forceinline__ bool operator()(int c, slamhip_cell **cell, float **prob) const
    {
        const int X = x0 + (c & (T - 1)), Y = y0 + c / T;
        if (X > x1 || Y > y1) return false;
        const size_t g = (size_t)Y * L.w + X;
        *cell = L.cells + g; *prob = L.prob + g;
        return true;
    }
};

template <int T>
__global__ void __launch_bounds__(HS_RENDER_LANES) k20_render(const k20_arg A)
{
    int lvl = 0;
    for (int l = 1; l < A.P.n_levels; l++) if ((int)blockIdx.x >= A.lv[l].tile0) lvl = l;
    const k20_level &L = A.lv[lvl];
    const int t = (int)blockIdx.x - L.tile0, ty = t / L.tiles_x, tx = t - ty * L.tiles_x;
    const int x0 = tx * T, y0 = ty * T, x1 = min(x0 + T, L.w) - 1, y1 = min(y0 + T, L.h) - 1;      // the tile's cells inside the level
    hs_render_block<T>(A.P, lvl, L.base, A.bound(lvl), k20_cells<T>{ L, x0, y0, x1, y1 }, x0, y0, x1, y1);
}

// ---- host side ---------------------------------------------------------------------------------------------------
// What the unit keeps: struct hs_scans, hs_scans.h (K21 reads the pool and the records).

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
    hs_block<float2, HS_MEM_DEVICE> np;                                    // (an early return frees it)
    SH_TRY(np.grow(sizeof(float2) * cap, "scan store"));
    hipStream_t st = hs->ctx->stream;
    hipError_t e = hipSuccess;
    if (g->used_pts) e = hipMemcpyAsync(np, g->d_pool, sizeof(float2) * g->used_pts, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);                     // (the old pool is idle behind it)
    SH_HIP(e);
    g->d_pool.swap(np); g->cap_pts = cap;                                  // (the old pool goes with np)
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_scans_add(slamhip_hs *hs, const float *xy, int32_t n_points, const float scan_origin[2], int32_t *out_index)
{
    SH_CHECK_ARG(hs);
    const bool own = xy == nullptr;                                        // the scan that is set on the handle (n_points, scan_origin: not read)
    if (!own) SH_CHECK_ARG(n_points >= 0);
    if (hs->scn && hs->scn->recs.size() >= (size_t)K20_MAX_SCANS) SH_FAIL(SLAMHIP_ERR_INVALID, "scan store: it holds 2^20 scans");
    SH_TRY(hs_call_begin(hs));
    SH_TRY(hs_unit<&slamhip_hs::scn>(hs));
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
            SH_TRY(g->h_io.grow(bytes, "scan store"));
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
    SH_TRY(g->h_io.grow(bytes, "scan store download"));
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
    hs_unit_drop<&slamhip_hs::scn>(hs);
    return SLAMHIP_OK;
}

static int k20_tile()       // T: 32, or 64 by SLAMHIP_K20_TILE=64 (both are built; DESIGN.md section 4 "K20")
{
    static const int v = sh_env_int("SLAMHIP_K20_TILE", 32) == 64 ? 64 : 32;
    return v;
}

extern "C" int32_t slamhip_hs_render(slamhip_hs *hs, int32_t first, int32_t last, const float *poses, int32_t flags)
{
    SH_CHECK_ARG(hs);
    SH_TRY(hs_render_check("slamhip_hs_render", hs, first, last, poses, flags));
    SH_TRY(hs_render_check_cache("slamhip_hs_render", hs));
    if (last == first && (flags & SLAMHIP_RENDER_KEEP)) return SLAMHIP_OK;
    hs_render_frame F;
    k20_arg A;
    SH_TRY(hs_render_begin(F, A, "slamhip_hs_render", hs, first, last, poses, flags));
    SH_TRY(hs_render_lay(F, A.P, 0, false));
    const int T = k20_tile();
    int tiles = 0;
    for (int l = 0; l < F.NL; l++) {
        A.lv[l].tiles_x = sh_div_up(A.lv[l].w, T); A.lv[l].tile0 = tiles;
        tiles += A.lv[l].tiles_x * sh_div_up(A.lv[l].h, T);                // (at most 1024 x 1024 per level)
    }
    return hs_render_chunks(F, A, [&](int c0) -> int32_t {
        if (T == 64) hipLaunchKernelGGL(k20_render<64>, dim3((unsigned)tiles), dim3(HS_RENDER_LANES), 0, hs->ctx->stream, A);
        else hipLaunchKernelGGL(k20_render<32>, dim3((unsigned)tiles), dim3(HS_RENDER_LANES), 0, hs->ctx->stream, A);
        SH_HIP(hipGetLastError());
        if (!F.keep && c0 == 0 && hs->bk) hs_bk_reset(hs);                 // rule 1: the directory goes with the map it belonged to (in stream order, behind the launch)
        return SLAMHIP_OK;
    });
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

// The definition itself over caller arrays: every valid line by hs_line_walk, the levels one after another.
extern "C" int32_t slamhip_debug_render(int32_t n_levels, const int32_t *dims, float cell_length, slamhip_cell *cells, int32_t *update_index, int32_t *cache_index,
                                        float free_factor, float occ_factor, const float *xy, const int32_t *offsets, const float *origins, const float *poses,
                                        int32_t N, int32_t flags)
{
    SH_CHECK_ARG(dims && cells && update_index && cache_index && n_levels >= 1 && n_levels <= HS_MAX_LEVELS && cell_length > 0.0f && N >= 0 && N <= K20_MAX_SCANS);
    SH_CHECK_ARG(N == 0 || (offsets && origins && poses));
    for (int l = 0; l < n_levels; l++) SH_CHECK_ARG(dims[2 * l] >= 1 && dims[2 * l + 1] >= 1 && dims[2 * l] <= 32768 && dims[2 * l + 1] <= 32768);
    SH_TRY(hs_render_check_offsets("render", xy, offsets, N));
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
                const hs_line ln = hs_line_make(xy[2 * (size_t)i], xy[2 * (size_t)i + 1], M, bx, by, hs_bound_level{ w, h }, &ex, &ey);
                if (ln.flags & 1) hs_line_walk(C, w, 0, 0, ln, bx, by, ex, ey, mark_free, mark_occ, lo_free, lo_occ);
            }
            update_index[l] += 3;                                          // :144
            cache_index[l]++;                                              // :147
        }
        C += (size_t)w * h;
        res *= 2.0f;                                                       // MapRepMultiMap.cs:56
    }
    return SLAMHIP_OK;
}
