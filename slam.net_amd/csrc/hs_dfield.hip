// hs_dfield.hip -- K9, the distance field of HectorSLAM's map: for every cell of one level the squared cell distance to the nearest
// SITE (a cell whose class is selected by a mask: occupied, free, unknown), capped at r * r, and the end-point distance score of the
// scan at many poses (slamhip_hs_distance_field, slamhip_hs_distance_score, slamhip_debug_distance_field).  No reference
// counterpart.  Definition: include/slamhip.h (slamhip_hs_distance_field); the arithmetic host and device share: hs_dfield.h.
//
// The class map, E, the two-launch pass, its tiles, the gather of a field call and the host plan are hs_field.h's, shared with K16
// (hs_nearest.hip); the pose batch of the score is hs_blocks.h's, shared with K8 and K16.  This unit's own:
//  * k9_rows: g(ex, ey) = min(horizontal distance to the nearest site of row ey, 255), one byte per cell of E: every lane finds the
//    nearest set bit of four consecutive cells by word (hs_df_row_nearest) and stores the four bytes as one word.
//  * k9_cols: F = min(r * r, min over |dy| <= r of g(ex, ey + dy)^2 + dy^2) as uint16.  The tile stages the g bytes of its rows and
//    r more above and below in LDS: (128 + 510) x 64 bytes = 40 832 B at r = 255, under the 64 KB of a static allocation, three
//    workgroups per compute unit.  Rows outside E hold the constant of a class-0 row.  A wavefront takes one row of the tile at a
//    time, a column per lane (64 consecutive bytes of LDS: no bank conflict, 128 contiguous bytes stored); hs_df_col_min walks dy
//    outward and stops once dy^2 >= the best so far.
//  * k9_score: poses x chunks of K9S_LANES points as K8 lays them out, a point per lane: the end cell by hs_trace.h's
//    hs_trace_end_cell, ONE look-up of F (the constant outside E), the per-point record if asked for, ballots and a wave sum, then
//    one set of agent-scope atomic adds per workgroup into the pose's summary, zeroed in-stream ahead of the launch.
#include "hs_field.h"
#include "hs_trace.h"

#define K9_TILE_BYTES (HS_FIELD_SROWS * HS_FIELD_TX)
#define K9S_LANES 256

static_assert(sizeof(slamhip_distance_summary) == 24, "the record of include/slamhip.h");
static_assert(K9_TILE_BYTES <= 65536 && HS_FIELD_TX == 64, "a static LDS allocation; a wavefront per tile row");

__global__ void __launch_bounds__(HS_FIELD_ROW_LANES) k9_rows(const hs_field_geo A, int segs, uint8_t *__restrict__ g)
{
    __shared__ uint32_t bits_s[HS_FIELD_BITW];
    const int tid = threadIdx.x;
    const int ey = blockIdx.x / segs, seg = blockIdx.x - ey * segs;
    int bmx0, nw;
    hs_field_row_bits(A, ey, seg, bits_s, &bmx0, &nw);
    const int ex = seg * HS_FIELD_SEG + HS_FIELD_ROW_CELLS * tid;
    if (ex >= A.pitch) return;                                             // (pitch is a multiple of 4: the four cells lie in the row or none does)
    uint32_t v = 0;
#pragma unroll
    for (int c = 0; c < HS_FIELD_ROW_CELLS; c++) v |= hs_df_row_nearest(bits_s, nw, ex + c - A.r - bmx0, A.r) << (8 * c);
    *(uint32_t *)(g + (size_t)ey * A.pitch + ex) = v;
}

__global__ void __launch_bounds__(HS_FIELD_COL_LANES) k9_cols(const hs_field_geo A, int tiles_x, const uint8_t *__restrict__ g, uint16_t *__restrict__ f)
{
    __shared__ __attribute__((aligned(16))) uint8_t tile_s[K9_TILE_BYTES];
    const int tid = threadIdx.x;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int ex0 = tx * HS_FIELD_TX, ey0 = ty * HS_FIELD_TY;
    const int rows = min(HS_FIELD_TY, A.eh - ey0);
    const int srows = rows + 2 * A.r;                                      // staged rows: ey0 - r .. ey0 + rows - 1 + r
    const uint32_t gc = hs_df_outside_g(A.mask) * 0x01010101u;             // a row of E's outside: class 0 everywhere
    for (int j = tid; j < srows * (HS_FIELD_TX / 4); j += HS_FIELD_COL_LANES) {
        const int sr = j / (HS_FIELD_TX / 4), ex = ex0 + 4 * (j - sr * (HS_FIELD_TX / 4));
        const int ey = ey0 - A.r + sr;
        const bool in = ey >= 0 && ey < A.eh && ex < A.pitch;
        ((uint32_t *)tile_s)[j] = in ? *(const uint32_t *)(g + (size_t)ey * A.pitch + ex) : gc;
    }
    __syncthreads();
    const int lane = tid & 63, ex = ex0 + lane;
    if (ex >= A.ew) return;
    for (int ly = tid >> 6; ly < rows; ly += HS_FIELD_COL_LANES / 64)
        f[(size_t)(ey0 + ly) * A.pitch + ex] = (uint16_t)hs_df_col_min(tile_s + (ly + A.r) * HS_FIELD_TX + lane, HS_FIELD_TX, A.r);
}

struct k9s_arg {
    const float2 *pts; int n;
    const float *poses; int chunks;        // B x 3, window frame; workgroups per pose
    float stm;
    hs_field E;
    int r2;
    slamhip_distance_summary *sums; uint16_t *points;   // points: nullptr, or B x n
};

__global__ void __launch_bounds__(K9S_LANES) k9_score(const k9s_arg A)
{
    __shared__ sh_m3x2 t_s;
    __shared__ int red_s[K9S_LANES / 64][5];
    const int tid = threadIdx.x;
    const int pose = blockIdx.x / A.chunks, chunk = blockIdx.x - pose * A.chunks;
    if (tid == 0) t_s = hs_trace_transform(A.stm, A.poses[3 * pose], A.poses[3 * pose + 1], A.poses[3 * pose + 2]);
    __syncthreads();
    const int i = chunk * K9S_LANES + tid;
    const bool have = i < A.n;
    bool counted = false;
    uint32_t F = 0xFFFFu;
    if (have) {
        const float2 p = A.pts[i];
        int ex, ey;
        counted = hs_trace_end_cell(t_s, p.x, p.y, &ex, &ey);
        if (counted) F = hs_field_lookup(A.E, (long long)ex, (long long)ey);
        if (A.points) A.points[(size_t)pose * (size_t)A.n + (size_t)i] = (uint16_t)F;
    }
    const int cnt[4] = { (int)__popcll(__ballot(counted)), (int)__popcll(__ballot(have && !counted)),
                         (int)__popcll(__ballot(counted && F == 0u)), (int)__popcll(__ballot(counted && F == (uint32_t)A.r2)) };
    int sum = counted ? (int)F : 0;                                        // (at most 65025 per lane: a workgroup's sum stays below 2^24)
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 4; k++) red_s[tid >> 6][k] = cnt[k];
        red_s[tid >> 6][4] = sum;
    }
    __syncthreads();
    if (tid < 5) {
        int v = 0;
        for (int wv = 0; wv < K9S_LANES / 64; wv++) v += red_s[wv][tid];
        slamhip_distance_summary *S = A.sums + pose;
        if (tid < 4) { if (v) __hip_atomic_fetch_add(&S->n_counted + tid, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
        else if (v) __hip_atomic_fetch_add((unsigned long long *)&S->sum_d2, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------
// The unit's blocks are hs->dfd, a hs_field_unit (hs_field.h): g and F of E, and the pose batch's.
int32_t hs_df_check(const char *who, int n_levels, int32_t level, int32_t world, int32_t site_mask, int32_t radius)
{
    if (level < 0 || level >= n_levels) SH_FAIL(SLAMHIP_ERR_INVALID, "%s: level %d of %d", who, level, n_levels);
    if (world != 0 && world != 1) SH_FAIL(SLAMHIP_ERR_INVALID, "%s: world = %d must be 0 (the window) or 1 (the world)", who, world);
    if (site_mask < 1 || site_mask > 7) SH_FAIL(SLAMHIP_ERR_INVALID, "%s: site_mask = %d must lie in [1, 7]", who, site_mask);
    if (radius < 1 || radius > HS_DF_MAX_RADIUS) SH_FAIL(SLAMHIP_ERR_INVALID, "%s: radius = %d must lie in [1, %d]", who, radius, HS_DF_MAX_RADIUS);
    return SLAMHIP_OK;
}

int32_t hs_df_check_score(const char *who, int n_levels, int32_t level, int32_t world, int32_t site_mask, int32_t radius, int32_t B, bool want_points,
                          int n_points, bool scan_is_set)
{
    SH_TRY(hs_df_check(who, n_levels, level, world, site_mask, radius));
    return hs_pose_batch_check("distance score", B, HS_FIELD_MAX_POSES, world, "per-point", want_points, n_points, scan_is_set, HS_FIELD_LOG2_MAX_POINTS);
}

// The plan and the launches of one field, for this unit's calls and for other units' launches (K11's clearance, K13's weights):
// hs_field.h's, on this unit's blocks and kernels.
int32_t hs_df_field_prepare(slamhip_hs *hs, int level, bool world, int site_mask, int radius, hs_class_map *M, hs_field *E)
{
    return hs_field_prepare<&slamhip_hs::dfd>(hs, "distance field", sizeof(uint8_t), level, world, radius, hs_df_outside(site_mask, radius), M, E);
}

int32_t hs_df_field_enqueue(slamhip_hs *hs, int level, bool world, const hs_class_map *M, const hs_field *E, int site_mask)
{
    return hs_field_enqueue(hs, hs->dfd, k9_rows, k9_cols, level, world, M, E, site_mask);
}

extern "C" int32_t slamhip_hs_distance_field(slamhip_hs *hs, int32_t level, int32_t world, int32_t site_mask, int32_t radius,
                                             int32_t x, int32_t y, int32_t w, int32_t h, uint16_t *out_d2)
{
    SH_CHECK_ARG(hs && out_d2);
    SH_TRY(hs_df_check("distance field", hs->n_levels, level, world, site_mask, radius));
    return hs_field_call<&slamhip_hs::dfd>(hs, "distance field", k9_rows, k9_cols, level, world != 0, site_mask, radius, hs_df_outside(site_mask, radius), x, y, w, h,
                         out_d2);
}

extern "C" int32_t slamhip_hs_distance_score(slamhip_hs *hs, int32_t level, int32_t world, int32_t site_mask, int32_t radius,
                                             const float *poses, int32_t B, slamhip_distance_summary *out_summaries, uint16_t *out_points)
{
    SH_CHECK_ARG(hs && poses && out_summaries);
    SH_TRY(hs_df_check_score("distance field", hs->n_levels, level, world, site_mask, radius, B, out_points != nullptr, hs->n_points, true));
    const int n = hs->n_points;
    SH_TRY(hs_call_begin(hs));
    int chunks;
    SH_TRY(hs_pose_batch_chunks("distance score", B, n, K9S_LANES, &chunks));
    hs_class_map M; hs_field E;
    SH_TRY(hs_df_field_prepare(hs, level, world != 0, site_mask, radius, &M, &E));
    hs_pose_batch *pb = &hs->dfd->pb;
    const size_t sum_bytes = sizeof(slamhip_distance_summary) * (size_t)B;
    const size_t pts_bytes = out_points ? sizeof(uint16_t) * (size_t)B * n : 0;
    SH_TRY(hs_pose_batch_begin(hs, pb, "distance field", poses, B, sum_bytes, pts_bytes));
    SH_TRY(hs_df_field_enqueue(hs, level, world != 0, &M, &E, site_mask));
    k9s_arg A;
    A.pts = hs->d_pts; A.n = n;
    A.poses = pb->d_poses; A.chunks = chunks;
    A.stm = hs->lv[level].stm;
    A.E = E; A.r2 = radius * radius;
    A.sums = (slamhip_distance_summary *)pb->d_out.p;
    A.points = out_points ? (uint16_t *)(pb->d_out + sum_bytes) : (uint16_t *)nullptr;
    hipLaunchKernelGGL(k9_score, dim3((unsigned)(B * chunks)), dim3(K9S_LANES), 0, hs->ctx->stream, A);
    SH_HIP(hipGetLastError());
    return hs_pose_batch_finish(hs, pb, sum_bytes, pts_bytes, out_summaries, out_points);
}

// CPU-side test hook: the field of the definition over a caller's class array, by hs_dfield.h -- the text the kernels run -- in
// hs_field.h's skeleton: g by hs_df_row_nearest over r more rows above and below, then F by hs_df_col_min.
extern "C" int32_t slamhip_debug_distance_field(const uint8_t *cls, int32_t cw, int32_t ch, int32_t site_mask, int32_t radius,
                                                int32_t x, int32_t y, int32_t w, int32_t h, uint16_t *out_d2)
{
    SH_CHECK_ARG(cls && out_d2 && cw >= 1 && ch >= 1 && (int64_t)cw * ch <= HS_FIELD_MAX_E);
    const int r = radius;
    std::vector<uint8_t> g;                                                // nx x srows, sized by the first row
    return hs_field_debug<uint16_t>("distance field", cls, cw, ch, site_mask, r, x, y, w, h, out_d2,
        [&] { return (uint16_t)hs_df_outside(site_mask, r); },
        [&](int nx, int srows, int sy, const uint32_t *bits, int nw, int p0) {
            g.resize((size_t)nx * (size_t)srows);
            uint8_t *grow = g.data() + (size_t)sy * nx;
            if (!bits) { memset(grow, (int)hs_df_outside_g(site_mask), (size_t)nx); return; }
            for (int i = 0; i < nx; i++) grow[i] = (uint8_t)hs_df_row_nearest(bits, nw, p0 + i, r);
        },
        [&](int nx, int sy, int i) { return (uint16_t)hs_df_col_min(g.data() + (size_t)sy * nx + i, nx, r); });
}
