// hs_nearest.hip -- K16, the nearest-site field of HectorSLAM's map: for every cell of one level the OFFSET (dx, dy) to the nearest
// site within r cells, ties to the smaller row and then the smaller column, and the scan-to-map pairs it gives at many poses with
// the sums a closed-form 2-D alignment step needs (slamhip_hs_nearest_field, slamhip_hs_nearest_pairs,
// slamhip_debug_nearest_field).  No reference counterpart.  Definition: include/slamhip.h (slamhip_hs_nearest_field); the arithmetic
// host and device share: hs_nearest.h, on top of hs_dfield.h's site words.
//
// The class map is K7's, re-packed on every call, and E is M grown by r cells on every side, exactly as K9 (hs_dfield.hip) has them;
// K9's own blocks and kernels are not used.  The pass is separable, two launches:
//  * k16_rows: o(ex, ey) = the signed offset to the nearest site of row ey with |o| < r, ties to the left, HS_NR_NONE if there is
//    none: one int16 per cell of E.  K9's row launch shape: a workgroup of K16_ROW_LANES lanes owns K16_SEG consecutive cells of one
//    row, the site bits the segment can see in LDS (hs_df_site_word), four cells per lane (hs_nr_row_nearest), one 8-byte store.
//  * k16_cols: N = (o(ex, ey + dy), dy) for the dy that minimises (o^2 + dy^2, dy) below r^2.  K9's tile, K16_TX columns x K16_TY
//    rows and r more rows above and below -- but the staged offsets are kept as a MAGNITUDE BYTE per cell plus a packed SIGN PLANE,
//    one 64-bit word per staged row: (128 + 510) x 64 + (128 + 510) x 8 = 45 936 B at r = 255, a static allocation, three
//    workgroups per compute unit.  The walk (hs_nr_col_argmin) reads magnitudes only, 64 consecutive bytes per wavefront and step
//    as K9's does; the sign is read once, for the winner.  Staging: a wavefront per staged row, a column per lane, the sign word by
//    ballot.  Rows outside E hold the constant of a class-0 row.
//  * k16_gather (the field call): the asked rectangle out of E, the constant outside; E is never downloaded.
//  * k16_pairs: K9's score launch shape, poses x chunks of K16P_LANES points, a point per lane: the end cell by hs_trace.h's
//    transform, ONE look-up of N, the per-point record if asked for, then the four counts by ballot and the nine int64 sums by a
//    wavefront reduction, through LDS, and one set of agent-scope atomic adds per workgroup into the pose's summary, zeroed
//    in-stream ahead of the launch.  Integer sums: any order gives the same bits.
#include "hs_blocks.h"
#include "hs_nearest.h"
#include "hs_trace.h"
#include <algorithm>
#include <vector>

#define K16_ROW_LANES 128
#define K16_ROW_CELLS 4                    // consecutive cells per lane: one 8-byte store
#define K16_SEG (K16_ROW_LANES * K16_ROW_CELLS)
#define K16_BITW (((K16_SEG + 2 * HS_DF_MAX_RADIUS + 31 + 31) >> 5) + 1)   // site words a segment can see: its first word starts up to 31 cells early
#define K16_TX 64
#define K16_TY 128
#define K16_COL_LANES 256
#define K16_STAGE 8                        // staged rows a wavefront loads before it stores any
#define K16_SROWS (K16_TY + 2 * HS_DF_MAX_RADIUS)                          // staged rows of a tile at r = 255
#define K16_LDS_BYTES (K16_SROWS * K16_TX + K16_SROWS * 8)
#define K16P_LANES 256
#define K16P_SUMS 9
#define HS_NR_MAX_E ((int64_t)1 << 26)     // cells of E: 2 + 4 bytes each, 384 MB
#define HS_NR_MAX_RECT ((int64_t)1 << 24)  // cells of a field call's rectangle: 64 MB of staging
#define HS_NR_MAX_POSES 65536
#define HS_NR_MAX_POINTS ((int64_t)1 << 22)   // B * n_points with per-point records

static_assert(sizeof(slamhip_pair_summary) == 88, "the record of include/slamhip.h");
static_assert(K16_LDS_BYTES <= 65536 && K16_TX == 64, "a static LDS allocation; a wavefront per tile row, a sign word per staged row");
static_assert(HS_NR_NONE == INT16_MAX && HS_NR_IGNORED == INT16_MIN, "the sentinels of include/slamhip.h");

// the class map M, and E = M grown by r; the offsets and N are rows of `pitch` cells (a multiple of 4)
struct k16_geo {
    const uint32_t *cls; int w, h, wpr;
    int r, mask;
    int ew, eh, pitch;
};

__global__ void __launch_bounds__(K16_ROW_LANES) k16_rows(const k16_geo A, int segs, int16_t *__restrict__ g)
{
    __shared__ uint32_t bits_s[K16_BITW];
    const int tid = threadIdx.x;
    const int ey = blockIdx.x / segs, seg = blockIdx.x - ey * segs;
    const int my = ey - A.r;
    const uint32_t *row = (my >= 0 && my < A.h) ? A.cls + (size_t)my * A.wpr : (const uint32_t *)nullptr;
    const int mx0 = seg * K16_SEG - A.r;                                   // the segment's first cell, in M's cells
    const int bmx0 = (mx0 - A.r) & ~31;                                    // the site mask's first cell: r cells further left, down to a multiple of 32
    const int nw = ((mx0 + K16_SEG - 1 + A.r - bmx0) >> 5) + 1;            // (at most K16_BITW)
    for (int j = tid; j < nw; j += K16_ROW_LANES) bits_s[j] = hs_df_site_word(row, A.w, bmx0 + 32 * j, A.mask);
    __syncthreads();
    const int ex = seg * K16_SEG + K16_ROW_CELLS * tid;
    if (ex >= A.pitch) return;                                             // (pitch is a multiple of 4: the four cells lie in the row or none does)
    uint32_t v[2] = { 0u, 0u };
#pragma unroll
    for (int c = 0; c < K16_ROW_CELLS; c++)
        v[c >> 1] |= (uint32_t)(uint16_t)(int16_t)hs_nr_row_nearest(bits_s, nw, ex + c - A.r - bmx0, A.r) << (16 * (c & 1));
    *(uint2 *)(g + (size_t)ey * A.pitch + ex) = make_uint2(v[0], v[1]);    // (8-byte aligned: pitch and ex are multiples of 4)
}

__global__ void __launch_bounds__(K16_COL_LANES) k16_cols(const k16_geo A, int tiles_x, const int16_t *__restrict__ g, uint32_t *__restrict__ n)
{
    __shared__ __attribute__((aligned(16))) uint8_t mag_s[K16_SROWS * K16_TX];
    __shared__ unsigned long long sign_s[K16_SROWS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int ex0 = tx * K16_TX, ey0 = ty * K16_TY;
    const int rows = min(K16_TY, A.eh - ey0);
    const int srows = rows + 2 * A.r;                                      // staged rows: ey0 - r .. ey0 + rows - 1 + r (at most K16_SROWS)
    const int gc = hs_nr_outside_g(A.mask);                                // a row of E's outside: class 0 everywhere
    const int ex = ex0 + lane;
    // a wavefront takes K16_STAGE staged rows at a time: the loads first, all in flight together, then bytes and sign words
    for (int sb = wave * K16_STAGE; sb < srows; sb += K16_STAGE * (K16_COL_LANES / 64)) {
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
            if (sr < srows) {                                              // (the same for every lane of the wavefront; srows <= K16_SROWS)
                mag_s[sr * K16_TX + lane] = (uint8_t)hs_nr_mag(o[u]);
                const unsigned long long neg = __ballot(o[u] < 0);
                if (lane == 0) sign_s[sr] = neg;
            }
        }
    }
    __syncthreads();
    if (ex >= A.ew) return;
    for (int ly = wave; ly < rows; ly += K16_COL_LANES / 64) {
        const int dy = hs_nr_col_argmin(mag_s + (ly + A.r) * K16_TX + lane, K16_TX, A.r);
        uint32_t pair = HS_NR_PAIR_NONE;
        if (dy != HS_NR_NONE) {                                            // (|dy| < r: the winner's row is a staged one)
            const int sr = ly + A.r + dy;
            const int m = (int)mag_s[sr * K16_TX + lane];
            pair = hs_nr_pack(((sign_s[sr] >> lane) & 1ull) ? -m : m, dy);
        }
        n[(size_t)(ey0 + ly) * A.pitch + ex] = pair;
    }
}

__global__ void __launch_bounds__(256) k16_gather(const hs_nfield E, int x, int y, int w, int n, uint32_t *__restrict__ out)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const int ry = j / w, rx = j - ry * w;
    out[j] = hs_nearest_lookup(E, (long long)x + rx, (long long)y + ry);
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
        float exf, eyf;
        sh_v2_transform(p.x, p.y, t_s, &exf, &eyf);
        counted = hs_trace_counts(exf) && hs_trace_counts(eyf);
        if (counted) {
            ex = (long long)sh_f2i(rintf(exf)); ey = (long long)sh_f2i(rintf(eyf));   // ToRoundPoint (banker's)
            pair = hs_nearest_lookup(A.E, ex, ey);
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
// What the unit needs, made by the first call and kept: the row offsets and N of E, the poses in device memory, the device block of
// the results (summaries and pairs, or a field call's rectangle), and the pinned block the poses leave and the results reach the
// host through.
struct hs_nearest {
    int16_t *d_g; size_t cap_g;
    uint32_t *d_n; size_t cap_n;
    float *d_poses; size_t cap_poses;
    unsigned char *d_out; size_t cap_out;
    unsigned char *h_io; size_t cap_h;
};

void hs_nr_free(slamhip_hs *hs)
{
    hs_nearest *nr = hs->nrs;
    if (!nr) return;
    hs_release((void **)&nr->d_g, &nr->cap_g, HS_MEM_DEVICE);
    hs_release((void **)&nr->d_n, &nr->cap_n, HS_MEM_DEVICE);
    hs_release((void **)&nr->d_poses, &nr->cap_poses, HS_MEM_DEVICE);
    hs_release((void **)&nr->d_out, &nr->cap_out, HS_MEM_DEVICE);
    hs_release((void **)&nr->h_io, &nr->cap_h, HS_MEM_PINNED);
    delete nr;
    hs->nrs = nullptr;
}

int32_t hs_nr_check_pairs(int n_levels, int32_t level, int32_t world, int32_t site_mask, int32_t radius, int32_t B, bool want_pairs, int n_points,
                          bool scan_is_set)
{
    SH_TRY(hs_df_check("nearest pairs", n_levels, level, world, site_mask, radius));
    if (B < 1 || B > HS_NR_MAX_POSES) SH_FAIL(SLAMHIP_ERR_INVALID, "nearest pairs: B = %d must lie in [1, %d]", B, HS_NR_MAX_POSES);
    if (scan_is_set && n_points <= 0) SH_FAIL(SLAMHIP_ERR_STATE, "nearest pairs: no scan (slamhip_hs_set_scan first)");
    if (want_pairs && (int64_t)B * n_points > HS_NR_MAX_POINTS)
        SH_FAIL(SLAMHIP_ERR_INVALID, "nearest pairs: per-point records of %d poses x %d points, more than 2^22", B, n_points);
    return SLAMHIP_OK;
}

// The plan of one field: the class map prepared (the world's plan refuses before anything is launched), E sized and refused if too
// large, the hs's block made if this is its first use, the offsets and N grown.  Nothing is launched.
static int32_t hs_nr_field_prepare(slamhip_hs *hs, int level, bool world, int site_mask, int radius, hs_class_map *M, hs_nfield *E)
{
    SH_TRY(hs_lat_pack_prepare(hs, level, world, M));
    const int64_t ew = (int64_t)M->w + 2 * radius, eh = (int64_t)M->h + 2 * radius;
    if (ew * eh > HS_NR_MAX_E)
        SH_FAIL(SLAMHIP_ERR_INVALID, "nearest field: E, the map of level %d grown by the radius, is %lld x %lld cells, more than 2^26", level,
                (long long)ew, (long long)eh);
    SH_TRY(hs_unit(&hs->nrs));
    hs_nearest *nr = hs->nrs;
    E->ew = (int)ew; E->eh = (int)eh; E->pitch = ((int)ew + 3) & ~3;
    E->e_x0 = M->x0 - radius; E->e_y0 = M->y0 - radius;                    // (-2^28 < x0 <= 0: no overflow)
    E->outside = hs_nr_outside(site_mask);
    const size_t cells = (size_t)E->pitch * (size_t)E->eh;
    SH_TRY(hs_grow((void **)&nr->d_g, &nr->cap_g, cells * sizeof(int16_t), HS_MEM_DEVICE, "nearest field"));
    SH_TRY(hs_grow((void **)&nr->d_n, &nr->cap_n, cells * sizeof(uint32_t), HS_MEM_DEVICE, "nearest field"));
    E->n = nr->d_n;
    return SLAMHIP_OK;
}

// the class map's pack and the two launches of the planned field, on the operator's stream (no timing class of their own)
static int32_t hs_nr_field_enqueue(slamhip_hs *hs, int level, bool world, const hs_class_map *M, const hs_nfield *E, int site_mask)
{
    hs_nearest *nr = hs->nrs;
    SH_TRY(hs_lat_pack_enqueue(hs, level, world, M));
    k16_geo G;
    G.cls = M->cls; G.w = M->w; G.h = M->h; G.wpr = M->wpr;
    G.r = M->x0 - E->e_x0; G.mask = site_mask;
    G.ew = E->ew; G.eh = E->eh; G.pitch = E->pitch;
    const int segs = sh_div_up(G.pitch, K16_SEG), tiles_x = sh_div_up(G.ew, K16_TX), tiles_y = sh_div_up(G.eh, K16_TY);
    // (at most 2^26 cells in E: neither grid reaches 2^31 workgroups)
    hipLaunchKernelGGL(k16_rows, dim3((unsigned)segs * (unsigned)G.eh), dim3(K16_ROW_LANES), 0, hs->ctx->stream, G, segs, nr->d_g);
    SH_HIP(hipGetLastError());
    hipLaunchKernelGGL(k16_cols, dim3((unsigned)tiles_x * (unsigned)tiles_y), dim3(K16_COL_LANES), 0, hs->ctx->stream, G, tiles_x, (const int16_t *)nr->d_g, nr->d_n);
    SH_HIP(hipGetLastError());
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_nearest_field(slamhip_hs *hs, int32_t level, int32_t world, int32_t site_mask, int32_t radius,
                                            int32_t x, int32_t y, int32_t w, int32_t h, int16_t *out_dxdy)
{
    SH_CHECK_ARG(hs && out_dxdy);
    SH_TRY(hs_df_check("nearest field", hs->n_levels, level, world, site_mask, radius));
    if (w < 1 || h < 1 || (int64_t)w * h > HS_NR_MAX_RECT)
        SH_FAIL(SLAMHIP_ERR_INVALID, "nearest field: a rectangle of %d x %d cells; w, h >= 1 and w * h <= 2^24", w, h);
    slamhip_ctx *ctx = hs->ctx;
    SH_TRY(hs_call_begin(hs));
    hs_class_map M; hs_nfield E;
    SH_TRY(hs_nr_field_prepare(hs, level, world != 0, site_mask, radius, &M, &E));
    hs_nearest *nr = hs->nrs;
    const int n = w * h;
    const size_t out_bytes = sizeof(uint32_t) * (size_t)n;
    SH_TRY(hs_grow((void **)&nr->d_out, &nr->cap_out, out_bytes, HS_MEM_DEVICE, "nearest field"));
    SH_TRY(hs_grow((void **)&nr->h_io, &nr->cap_h, out_bytes, HS_MEM_PINNED, "nearest field"));
    SH_TRY(hs_nr_field_enqueue(hs, level, world != 0, &M, &E, site_mask));
    hipLaunchKernelGGL(k16_gather, dim3((unsigned)sh_div_up(n, 256)), dim3(256), 0, ctx->stream, E, x, y, w, n, (uint32_t *)nr->d_out);
    SH_HIP(hipGetLastError());
    SH_HIP(hipMemcpyAsync(nr->h_io, nr->d_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    SH_TRY(hs_call_finish(hs));
    memcpy(out_dxdy, nr->h_io, out_bytes);
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_nearest_pairs(slamhip_hs *hs, int32_t level, int32_t world, int32_t site_mask, int32_t radius,
                                            const float *poses, int32_t B, slamhip_pair_summary *out_summaries, int16_t *out_pairs)
{
    SH_CHECK_ARG(hs && poses && out_summaries);
    SH_TRY(hs_nr_check_pairs(hs->n_levels, level, world, site_mask, radius, B, out_pairs != nullptr, hs->n_points, true));
    const int n = hs->n_points;
    slamhip_ctx *ctx = hs->ctx;
    SH_TRY(hs_call_begin(hs));
    const int chunks = sh_div_up(n, K16P_LANES);
    if ((int64_t)B * chunks > (int64_t)INT32_MAX) SH_FAIL(SLAMHIP_ERR_INVALID, "nearest pairs: %d poses x %d points, more workgroups than one launch takes", B, n);
    hs_class_map M; hs_nfield E;
    SH_TRY(hs_nr_field_prepare(hs, level, world != 0, site_mask, radius, &M, &E));
    hs_nearest *nr = hs->nrs;
    const size_t pose_bytes = sizeof(float) * 3 * (size_t)B;
    const size_t sum_bytes = sizeof(slamhip_pair_summary) * (size_t)B;     // (a multiple of 8: the pairs and the poses behind it stay aligned)
    const size_t pts_bytes = out_pairs ? sizeof(uint32_t) * (size_t)B * n : 0;
    const size_t out_bytes = (sum_bytes + pts_bytes + 7) & ~(size_t)7;     // (the poses follow, 8-byte aligned)
    SH_TRY(hs_grow((void **)&nr->d_poses, &nr->cap_poses, pose_bytes, HS_MEM_DEVICE, "nearest pairs"));
    SH_TRY(hs_grow((void **)&nr->d_out, &nr->cap_out, out_bytes, HS_MEM_DEVICE, "nearest pairs"));
    SH_TRY(hs_grow((void **)&nr->h_io, &nr->cap_h, out_bytes + pose_bytes, HS_MEM_PINNED, "nearest pairs"));
    float *h_poses = (float *)(nr->h_io + out_bytes);
    memcpy(h_poses, poses, pose_bytes);
    SH_TRY(hs_flush_scan(hs));
    SH_HIP(hipMemcpyAsync(nr->d_poses, h_poses, pose_bytes, hipMemcpyHostToDevice, ctx->stream));
    SH_HIP(hipMemsetAsync(nr->d_out, 0, sum_bytes, ctx->stream));
    SH_TRY(hs_nr_field_enqueue(hs, level, world != 0, &M, &E, site_mask));
    k16p_arg A;
    A.pts = hs->d_pts; A.n = n;
    A.poses = nr->d_poses; A.chunks = chunks;
    A.stm = hs->lv[level].stm;
    A.E = E;
    A.sums = (slamhip_pair_summary *)nr->d_out;
    A.pairs = out_pairs ? (uint32_t *)(nr->d_out + sum_bytes) : (uint32_t *)nullptr;
    hipLaunchKernelGGL(k16_pairs, dim3((unsigned)(B * chunks)), dim3(K16P_LANES), 0, ctx->stream, A);
    SH_HIP(hipGetLastError());
    SH_HIP(hipMemcpyAsync(nr->h_io, nr->d_out, sum_bytes + pts_bytes, hipMemcpyDeviceToHost, ctx->stream));
    SH_TRY(hs_call_finish(hs));
    memcpy(out_summaries, nr->h_io, sum_bytes);
    if (out_pairs) memcpy(out_pairs, nr->h_io + sum_bytes, pts_bytes);
    return SLAMHIP_OK;
}

// CPU-side test hook: the field of the definition over a caller's class array, by hs_nearest.h -- the text the kernels run.  The
// classes are packed as K7 packs them; for the rows and columns of E the rectangle touches, the row offsets by hs_df_site_word and
// hs_nr_row_nearest over r more rows above and below, kept as the column kernel keeps them (magnitude bytes, signs apart), then N
// by hs_nr_col_argmin.
extern "C" int32_t slamhip_debug_nearest_field(const uint8_t *cls, int32_t cw, int32_t ch, int32_t site_mask, int32_t radius,
                                               int32_t x, int32_t y, int32_t w, int32_t h, int16_t *out_dxdy)
{
    SH_CHECK_ARG(cls && out_dxdy && cw >= 1 && ch >= 1 && (int64_t)cw * ch <= HS_NR_MAX_E);
    if (site_mask < 1 || site_mask > 7) SH_FAIL(SLAMHIP_ERR_INVALID, "nearest field: site_mask = %d must lie in [1, 7]", site_mask);
    if (radius < 1 || radius > HS_DF_MAX_RADIUS) SH_FAIL(SLAMHIP_ERR_INVALID, "nearest field: radius = %d must lie in [1, %d]", radius, HS_DF_MAX_RADIUS);
    if (w < 1 || h < 1 || (int64_t)w * h > HS_NR_MAX_RECT)
        SH_FAIL(SLAMHIP_ERR_INVALID, "nearest field: a rectangle of %d x %d cells; w, h >= 1 and w * h <= 2^24", w, h);
    const int r = radius;
    uint32_t *out = (uint32_t *)out_dxdy;                                  // (a pair is one word; memcpy below keeps the caller's alignment free)
    const uint32_t outside = hs_nr_outside(site_mask);
    for (int64_t j = 0; j < (int64_t)w * h; j++) memcpy(out + j, &outside, sizeof(outside));
    // the part of the rectangle inside E, in the map's cells: [ax0, ax1) x [ay0, ay1)
    const int64_t ax0 = std::max<int64_t>(x, -r), ax1 = std::min<int64_t>((int64_t)x + w, (int64_t)cw + r);
    const int64_t ay0 = std::max<int64_t>(y, -r), ay1 = std::min<int64_t>((int64_t)y + h, (int64_t)ch + r);
    if (ax0 >= ax1 || ay0 >= ay1) return SLAMHIP_OK;
    const int wpr = (cw + 15) / 16;
    std::vector<uint32_t> packed((size_t)wpr * ch, 0u);
    for (int cy = 0; cy < ch; cy++)
        for (int cx = 0; cx < cw; cx++) packed[(size_t)cy * wpr + (cx >> 4)] |= (uint32_t)(cls[(size_t)cy * cw + cx] & 3u) << (2 * (cx & 15));
    const int nx = (int)(ax1 - ax0), ny = (int)(ay1 - ay0);
    const int bmx0 = ((int)ax0 - r) & ~31;                                 // the site mask's first cell
    const int nw = (((int)ax1 - 1 + r - bmx0) >> 5) + 1;
    std::vector<uint32_t> bits((size_t)nw);
    std::vector<uint8_t> mag((size_t)nx * (size_t)(ny + 2 * r)), neg((size_t)nx * (size_t)(ny + 2 * r));   // rows ay0 - r .. ay1 - 1 + r
    for (int gy = 0; gy < ny + 2 * r; gy++) {
        const int64_t my = ay0 - r + gy;
        uint8_t *mrow = mag.data() + (size_t)gy * nx, *nrow = neg.data() + (size_t)gy * nx;
        const bool in_e = my >= -r && my < (int64_t)ch + r;                // (a row outside E: the constant of a class-0 row)
        const uint32_t *row = (in_e && my >= 0 && my < ch) ? packed.data() + (size_t)my * wpr : (const uint32_t *)nullptr;
        if (in_e)
            for (int j = 0; j < nw; j++) bits[(size_t)j] = hs_df_site_word(row, cw, bmx0 + 32 * j, site_mask);
        for (int i = 0; i < nx; i++) {
            const int o = in_e ? hs_nr_row_nearest(bits.data(), nw, (int)ax0 + i - bmx0, r) : hs_nr_outside_g(site_mask);
            mrow[i] = (uint8_t)hs_nr_mag(o); nrow[i] = (uint8_t)(o < 0);
        }
    }
    for (int iy = 0; iy < ny; iy++)
        for (int i = 0; i < nx; i++) {
            const int dy = hs_nr_col_argmin(mag.data() + (size_t)(iy + r) * nx + i, nx, r);
            uint32_t pair = HS_NR_PAIR_NONE;
            if (dy != HS_NR_NONE) {
                const size_t at = (size_t)(iy + r + dy) * nx + i;
                pair = hs_nr_pack(neg[at] ? -(int)mag[at] : (int)mag[at], dy);
            }
            memcpy(out + (size_t)(ay0 + iy - y) * (size_t)w + (size_t)(ax0 + i - x), &pair, sizeof(pair));
        }
    return SLAMHIP_OK;
}
