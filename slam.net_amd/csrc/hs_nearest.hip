// hs_nearest.hip -- K16, the nearest-site field of HectorSLAM's map: for every cell of one level the OFFSET (dx, dy) to the nearest
// site within r cells, ties to the smaller row and then the smaller column, and the scan-to-map pairs it gives at many poses with
// the sums a closed-form 2-D alignment step needs (slamhip_hs_nearest_field, slamhip_hs_nearest_pairs,
// slamhip_debug_nearest_field).  No reference counterpart.  Definition: include/slamhip.h (slamhip_hs_nearest_field); the arithmetic
// host and device share: hs_nearest.h, on top of hs_dfield.h's site words.
//
// The class map, E, the two-launch pass, its tiles, the gather of a field call and the host plan are hs_field.h's, shared with K9
// (hs_dfield.hip), whose blocks and kernels are not used; the pose batch of the pairs is hs_blocks.h's, shared with K8 and K9.
// This unit's own:
//  * k16_rows: o(ex, ey) = the signed offset to the nearest site of row ey with |o| < r, ties to the left, HS_NR_NONE if there is
//    none: one int16 per cell of E, four cells per lane (hs_nr_row_nearest), one 8-byte store.
//  * k16_cols: N = (o(ex, ey + dy), dy) for the dy that minimises (o^2 + dy^2, dy) below r^2.  The staged offsets are kept as a
//    MAGNITUDE BYTE per cell plus a packed SIGN PLANE, one 64-bit word per staged row: (128 + 510) x 64 + (128 + 510) x 8 =
//    45 936 B at r = 255, a static allocation, three workgroups per compute unit.  The walk (hs_nr_col_argmin) reads magnitudes
//    only, 64 consecutive bytes per wavefront and step as K9's does; the sign is read once, for the winner.  Staging: a wavefront
//    per staged row, a column per lane, the sign word by ballot.  Rows outside E hold the constant of a class-0 row.
//  * k16_pairs: poses x chunks of K16P_LANES points as K8 lays them out, a point per lane: the end cell by hs_trace.h's
//    hs_trace_end_cell, ONE look-up of N, the per-point record if asked for, then the four counts by ballot and the nine int64 sums
//    by a wavefront reduction, through LDS, and one set of agent-scope atomic adds per workgroup into the pose's summary, zeroed
//    in-stream ahead of the launch.  Integer sums: any order gives the same bits.
#include "hs_field.h"
#include "hs_nearest.h"
#include "hs_trace.h"

#define K16_STAGE 8                        // staged rows a wavefront loads before it stores any
#define K16_LDS_BYTES (HS_FIELD_SROWS * HS_FIELD_TX + HS_FIELD_SROWS * 8)
#define K16P_LANES 256
#define K16P_SUMS 9

static_assert(sizeof(slamhip_pair_summary) == 88, "the record of include/slamhip.h");
static_assert(K16_LDS_BYTES <= 65536 && HS_FIELD_TX == 64, "a static LDS allocation; a wavefront per tile row, a sign word per staged row");
static_assert(HS_NR_NONE == INT16_MAX && HS_NR_IGNORED == INT16_MIN, "the sentinels of include/slamhip.h");

__global__ void __launch_bounds__(HS_FIELD_ROW_LANES) k16_rows(const hs_field_geo A, int segs, int16_t *__restrict__ g)
{
    __shared__ uint32_t bits_s[HS_FIELD_BITW];
    const int tid = threadIdx.x;
    const int ey = blockIdx.x / segs, seg = blockIdx.x - ey * segs;
    int bmx0, nw;
    hs_field_row_bits(A, ey, seg, bits_s, &bmx0, &nw);
    const int ex = seg * HS_FIELD_SEG + HS_FIELD_ROW_CELLS * tid;
    if (ex >= A.pitch) return;                                             // (pitch is a multiple of 4: the four cells lie in the row or none does)
    uint32_t v[2] = { 0u, 0u };
#pragma unroll
    for (int c = 0; c < HS_FIELD_ROW_CELLS; c++)
        v[c >> 1] |= (uint32_t)(uint16_t)(int16_t)hs_nr_row_nearest(bits_s, nw, ex + c - A.r - bmx0, A.r) << (16 * (c & 1));
    *(uint2 *)(g + (size_t)ey * A.pitch + ex) = make_uint2(v[0], v[1]);    // (8-byte aligned: pitch and ex are multiples of 4)
}

__global__ void __launch_bounds__(HS_FIELD_COL_LANES) k16_cols(const hs_field_geo A, int tiles_x, const int16_t *__restrict__ g, uint32_t *__restrict__ n)
{
    __shared__ __attribute__((aligned(16))) uint8_t mag_s[HS_FIELD_SROWS * HS_FIELD_TX];
    __shared__ unsigned long long sign_s[HS_FIELD_SROWS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int ex0 = tx * HS_FIELD_TX, ey0 = ty * HS_FIELD_TY;
    const int rows = min(HS_FIELD_TY, A.eh - ey0);
    const int srows = rows + 2 * A.r;                                      // staged rows: ey0 - r .. ey0 + rows - 1 + r (at most HS_FIELD_SROWS)
    const int gc = hs_nr_outside_g(A.mask);                                // a row of E's outside: class 0 everywhere
    const int ex = ex0 + lane;
    // a wavefront takes K16_STAGE staged rows at a time: the loads first, all in flight together, then bytes and sign words
    for (int sb = wave * K16_STAGE; sb < srows; sb += K16_STAGE * (HS_FIELD_COL_LANES / 64)) {
        int o[K16_STAGE];
#pragma unroll
        for (int u = 0; u < K16_STAGE; u++) {
            const int ey = ey0 - A.r + sb + u;
            const bool in = sb + u < srows && ey >= 0 && ey < A.eh && ex < A.pitch;
            o[u] = in ? (int)g[(size_t)ey * A.pitch + ex] : gc;
        }
#pragma unroll
        for (int u = 0; u < K16_STAGE; u++) {
            const int sr = sb + u;
            if (sr < srows) {                                              // (the same for every lane of the wavefront; srows <= HS_FIELD_SROWS)
                mag_s[sr * HS_FIELD_TX + lane] = (uint8_t)hs_nr_mag(o[u]);
                const unsigned long long neg = __ballot(o[u] < 0);
                if (lane == 0) sign_s[sr] = neg;
            }
        }
    }
    __syncthreads();
    if (ex >= A.ew) return;
    for (int ly = wave; ly < rows; ly += HS_FIELD_COL_LANES / 64) {
        const int dy = hs_nr_col_argmin(mag_s + (ly + A.r) * HS_FIELD_TX + lane, HS_FIELD_TX, A.r);
        uint32_t pair = HS_NR_PAIR_NONE;
        if (dy != HS_NR_NONE) {                                            // (|dy| < r: the winner's row is a staged one)
            const int sr = ly + A.r + dy;
            const int m = (int)mag_s[sr * HS_FIELD_TX + lane];
            pair = hs_nr_pack(((sign_s[sr] >> lane) & 1ull) ? -m : m, dy);
        }
        n[(size_t)(ey0 + ly) * A.pitch + ex] = pair;
    }
}

struct k16p_arg {
    const float2 *pts; int n;
    const float *poses; int chunks;        // B x 3, window frame; workgroups per pose
    float stm;
    hs_nfield E;
    slamhip_pair_summary *sums; uint32_t *pairs;   // pairs: nullptr, or B x n
};

__global__ void __launch_bounds__(K16P_LANES) k16_pairs(const k16p_arg A)
{
    __shared__ sh_m3x2 t_s;
    __shared__ int cnt_s[K16P_LANES / 64][4];
    __shared__ long long sum_s[K16P_LANES / 64][K16P_SUMS];
    const int tid = threadIdx.x;
    const int pose = blockIdx.x / A.chunks, chunk = blockIdx.x - pose * A.chunks;
    if (tid == 0) t_s = hs_trace_transform(A.stm, A.poses[3 * pose], A.poses[3 * pose + 1], A.poses[3 * pose + 2]);
    __syncthreads();
    const int i = chunk * K16P_LANES + tid;
    const bool have = i < A.n;
    bool counted = false;
    uint32_t pair = HS_NR_PAIR_IGNORED;
    long long ex = 0, ey = 0;
    if (have) {
        const float2 p = A.pts[i];
        int cx, cy;
        counted = hs_trace_end_cell(t_s, p.x, p.y, &cx, &cy);
        if (counted) {
            ex = (long long)cx; ey = (long long)cy;
            pair = hs_field_lookup(A.E, ex, ey);
        }
        if (A.pairs) A.pairs[(size_t)pose * (size_t)A.n + (size_t)i] = pair;
    }
    const bool matched = counted && pair != HS_NR_PAIR_NONE;
    const int cnt[4] = { (int)__popcll(__ballot(counted)), (int)__popcll(__ballot(have && !counted)), (int)__popcll(__ballot(matched)),
                         (int)__popcll(__ballot(matched && pair == 0u)) };
    long long s[K16P_SUMS];
#pragma unroll
    for (int k = 0; k < K16P_SUMS; k++) s[k] = 0;
    if (matched) {
        const long long dx = hs_nr_dx(pair), dy = hs_nr_dy(pair);
        const long long qx = ex + dx, qy = ey + dy;                        // (|e| <= 2^24, |d| <= 254: products below 2^49)
        s[0] = dx * dx + dy * dy;
        s[1] = ex; s[2] = ey; s[3] = qx; s[4] = qy;
        s[5] = ex * qx; s[6] = ey * qy; s[7] = ex * qy; s[8] = ey * qx;
    }
#pragma unroll
    for (int k = 0; k < K16P_SUMS; k++)
        for (int off = 32; off > 0; off >>= 1) s[k] += __shfl_down(s[k], off, 64);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 4; k++) cnt_s[tid >> 6][k] = cnt[k];
#pragma unroll
        for (int k = 0; k < K16P_SUMS; k++) sum_s[tid >> 6][k] = s[k];
    }
    __syncthreads();
    slamhip_pair_summary *S = A.sums + pose;
    if (tid < 4) {
        int v = 0;
        for (int wv = 0; wv < K16P_LANES / 64; wv++) v += cnt_s[wv][tid];
        if (v) __hip_atomic_fetch_add(&S->n_counted + tid, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else if (tid < 4 + K16P_SUMS) {
        unsigned long long v = 0;                                          // (modulo 2^64, as the definition has the sums)
        for (int wv = 0; wv < K16P_LANES / 64; wv++) v += (unsigned long long)sum_s[wv][tid - 4];
        if (v) __hip_atomic_fetch_add((unsigned long long *)(&S->sum_d2 + (tid - 4)), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------
// The unit's blocks are hs->nrs, a hs_field_unit (hs_field.h): the row offsets and N of E, and the pose batch's.
int32_t hs_nr_check_pairs(int n_levels, int32_t level, int32_t world, int32_t site_mask, int32_t radius, int32_t B, bool want_pairs, int n_points,
                          bool scan_is_set)
{
    SH_TRY(hs_df_check("nearest pairs", n_levels, level, world, site_mask, radius));
    return hs_pose_batch_check("nearest pairs", B, HS_FIELD_MAX_POSES, world, "per-point", want_pairs, n_points, scan_is_set, HS_FIELD_LOG2_MAX_POINTS);
}

extern "C" int32_t slamhip_hs_nearest_field(slamhip_hs *hs, int32_t level, int32_t world, int32_t site_mask, int32_t radius,
                                            int32_t x, int32_t y, int32_t w, int32_t h, int16_t *out_dxdy)
{
    SH_CHECK_ARG(hs && out_dxdy);
    SH_TRY(hs_df_check("nearest field", hs->n_levels, level, world, site_mask, radius));
    return hs_field_call<&slamhip_hs::nrs>(hs, "nearest field", k16_rows, k16_cols, level, world != 0, site_mask, radius, hs_nr_outside(site_mask), x, y, w, h, out_dxdy);
}

extern "C" int32_t slamhip_hs_nearest_pairs(slamhip_hs *hs, int32_t level, int32_t world, int32_t site_mask, int32_t radius,
                                            const float *poses, int32_t B, slamhip_pair_summary *out_summaries, int16_t *out_pairs)
{
    SH_CHECK_ARG(hs && poses && out_summaries);
    SH_TRY(hs_nr_check_pairs(hs->n_levels, level, world, site_mask, radius, B, out_pairs != nullptr, hs->n_points, true));
    const int n = hs->n_points;
    SH_TRY(hs_call_begin(hs));
    int chunks;
    SH_TRY(hs_pose_batch_chunks("nearest pairs", B, n, K16P_LANES, &chunks));
    hs_class_map M; hs_nfield E;
    SH_TRY(hs_field_prepare<&slamhip_hs::nrs>(hs, "nearest field", sizeof(int16_t), level, world != 0, radius, hs_nr_outside(site_mask), &M, &E));
    hs_pose_batch *pb = &hs->nrs->pb;
    const size_t sum_bytes = sizeof(slamhip_pair_summary) * (size_t)B;     // (a multiple of 8: the pairs behind it stay aligned)
    const size_t pts_bytes = out_pairs ? sizeof(uint32_t) * (size_t)B * n : 0;
    SH_TRY(hs_pose_batch_begin(hs, pb, "nearest pairs", poses, B, sum_bytes, pts_bytes));
    SH_TRY(hs_field_enqueue(hs, hs->nrs, k16_rows, k16_cols, level, world != 0, &M, &E, site_mask));
    k16p_arg A;
    A.pts = hs->d_pts; A.n = n;
    A.poses = pb->d_poses; A.chunks = chunks;
    A.stm = hs->lv[level].stm;
    A.E = E;
    A.sums = (slamhip_pair_summary *)pb->d_out.p;
    A.pairs = out_pairs ? (uint32_t *)(pb->d_out + sum_bytes) : (uint32_t *)nullptr;
    hipLaunchKernelGGL(k16_pairs, dim3((unsigned)(B * chunks)), dim3(K16P_LANES), 0, hs->ctx->stream, A);
    SH_HIP(hipGetLastError());
    return hs_pose_batch_finish(hs, pb, sum_bytes, pts_bytes, out_summaries, out_pairs);
}

// CPU-side test hook: the field of the definition over a caller's class array, by hs_nearest.h -- the text the kernels run -- in
// hs_field.h's skeleton: the row offsets by hs_nr_row_nearest over r more rows above and below, kept as the column kernel keeps
// them (magnitude bytes, signs apart), then N by hs_nr_col_argmin.  (A pair is one word of the caller's int16 array.)
extern "C" int32_t slamhip_debug_nearest_field(const uint8_t *cls, int32_t cw, int32_t ch, int32_t site_mask, int32_t radius,
                                               int32_t x, int32_t y, int32_t w, int32_t h, int16_t *out_dxdy)
{
    SH_CHECK_ARG(cls && out_dxdy && cw >= 1 && ch >= 1 && (int64_t)cw * ch <= HS_FIELD_MAX_E);
    const int r = radius;
    std::vector<uint8_t> mag, neg;                                         // nx x srows each, sized by the first row
    return hs_field_debug<uint32_t>("nearest field", cls, cw, ch, site_mask, r, x, y, w, h, out_dxdy,
        [&] { return hs_nr_outside(site_mask); },
        [&](int nx, int srows, int sy, const uint32_t *bits, int nw, int p0) {
            mag.resize((size_t)nx * (size_t)srows); neg.resize((size_t)nx * (size_t)srows);
            for (int i = 0; i < nx; i++) {
                const int o = bits ? hs_nr_row_nearest(bits, nw, p0 + i, r) : hs_nr_outside_g(site_mask);
                mag[(size_t)sy * nx + i] = (uint8_t)hs_nr_mag(o); neg[(size_t)sy * nx + i] = (uint8_t)(o < 0);
            }
        },
        [&](int nx, int sy, int i) {
            const int dy = hs_nr_col_argmin(mag.data() + (size_t)sy * nx + i, nx, r);
            if (dy == HS_NR_NONE) return (uint32_t)HS_NR_PAIR_NONE;
            const size_t at = (size_t)(sy + dy) * nx + i;
            return hs_nr_pack(neg[at] ? -(int)mag[at] : (int)mag[at], dy);
        });
}
