// hs_dfield.hip -- K9, the distance field of HectorSLAM's map: for every cell of one level the squared cell distance to the nearest
// SITE (a cell whose class is selected by a mask: occupied, free, unknown), capped at r * r, and the end-point distance score of the
// scan at many poses (slamhip_hs_distance_field, slamhip_hs_distance_score, slamhip_debug_distance_field).  No reference
// counterpart.  Definition: include/slamhip.h (slamhip_hs_distance_field); the arithmetic host and device share: hs_dfield.h.
//
// The class map is K7's (hs_lattice.hip), re-packed on every call: M = (x0, y0, w, h) in the window's frame, the window or the
// world's rectangle R.  The field is kept for E, M grown by r cells on every side; outside E it is a constant (hs_df_outside).  E's
// cell (ex, ey) is cell (ex - r, ey - r) of M.  The pass is separable, two launches:
//  * k9_rows: g(ex, ey) = min(horizontal distance to the nearest site of row ey, 255), one byte per cell of E.  A workgroup of
//    K9_ROW_LANES lanes owns K9_SEG consecutive cells of one row.  It turns the packed 2-bit words the segment can see -- its cells
//    and r more on both sides -- into a 1-bit site mask in LDS (hs_df_site_word: at most K9_BITW words), then every lane finds the
//    nearest set bit of four consecutive cells by word (hs_df_row_nearest) and stores the four bytes as one word.  Padding cells of
//    a row's last packed word and every cell outside M are class 0 by hs_df_site_word's own test, not by what the padding holds.
//    Rows of E above and below M are rows of class 0 like any other.
//  * k9_cols: F = min(r * r, min over |dy| <= r of g(ex, ey + dy)^2 + dy^2) as uint16.  A workgroup of 256 lanes owns a tile of
//    K9_TX columns x K9_TY rows and stages the g bytes of its rows and r more above and below in LDS: (128 + 510) x 64 bytes =
//    40 832 B at r = 255, under the 64 KB of a static allocation, three workgroups per compute unit.  Rows outside E hold the
//    constant of a class-0 row.  A wavefront takes one row of the tile at a time, a column per lane (64 consecutive bytes of LDS:
//    no bank conflict, 128 contiguous bytes stored); hs_df_col_min walks dy outward and stops once dy^2 >= the best so far.
//  * k9_score: poses x chunks of K9S_LANES points as K8 lays them out, a point per lane: the end cell by hs_trace.h's transform,
//    ONE look-up of F (the constant outside E), the per-point record if asked for, ballots and a wave sum, then one set of
//    agent-scope atomic adds per workgroup into the pose's summary, zeroed in-stream ahead of the launch.
//  * k9_gather (the field call): the asked rectangle out of E, the constant outside, into the block the result leaves through; E is
//    never downloaded.
#include "hs_blocks.h"
#include "hs_dfield.h"
#include "hs_trace.h"
#include <algorithm>
#include <vector>

#define K9_ROW_LANES 128
#define K9_ROW_CELLS 4                     // consecutive cells per lane: one 4-byte store
#define K9_SEG (K9_ROW_LANES * K9_ROW_CELLS)
#define K9_BITW (((K9_SEG + 2 * HS_DF_MAX_RADIUS + 31 + 31) >> 5) + 1)   // site words a segment can see: its first word starts up to 31 cells early
#define K9_TX 64
#define K9_TY 128
#define K9_COL_LANES 256
#define K9_TILE_BYTES ((K9_TY + 2 * HS_DF_MAX_RADIUS) * K9_TX)
#define K9S_LANES 256
#define HS_DF_MAX_E ((int64_t)1 << 26)     // cells of E: 1 + 2 bytes each, 192 MB
#define HS_DF_MAX_RECT ((int64_t)1 << 24)  // cells of a field call's rectangle: 32 MB of staging
#define HS_DF_MAX_POSES 65536
#define HS_DF_MAX_POINTS ((int64_t)1 << 22)   // B * n_points with per-point records

static_assert(sizeof(slamhip_distance_summary) == 24, "the record of include/slamhip.h");
static_assert(K9_TILE_BYTES <= 65536 && K9_TX == 64, "a static LDS allocation; a wavefront per tile row");

// the class map M, and E = M grown by r; g and F are rows of `pitch` cells (a multiple of 4)
struct k9_geo {
    const uint32_t *cls; int w, h, wpr;
    int r, mask;
    int ew, eh, pitch;
};

__global__ void __launch_bounds__(K9_ROW_LANES) k9_rows(const k9_geo A, int segs, uint8_t *__restrict__ g)
{
    __shared__ uint32_t bits_s[K9_BITW];
    const int tid = threadIdx.x;
    const int ey = blockIdx.x / segs, seg = blockIdx.x - ey * segs;
    const int my = ey - A.r;
    const uint32_t *row = (my >= 0 && my < A.h) ? A.cls + (size_t)my * A.wpr : (const uint32_t *)nullptr;
    const int mx0 = seg * K9_SEG - A.r;                                    // the segment's first cell, in M's cells
    const int bmx0 = (mx0 - A.r) & ~31;                                    // the site mask's first cell: r cells further left, down to a multiple of 32
    const int nw = ((mx0 + K9_SEG - 1 + A.r - bmx0) >> 5) + 1;             // (at most K9_BITW)
    for (int j = tid; j < nw; j += K9_ROW_LANES) bits_s[j] = hs_df_site_word(row, A.w, bmx0 + 32 * j, A.mask);
    __syncthreads();
    const int ex = seg * K9_SEG + K9_ROW_CELLS * tid;
    if (ex >= A.pitch) return;                                             // (pitch is a multiple of 4: the four cells lie in the row or none does)
    uint32_t v = 0;
#pragma unroll
    for (int c = 0; c < K9_ROW_CELLS; c++) v |= hs_df_row_nearest(bits_s, nw, ex + c - A.r - bmx0, A.r) << (8 * c);
    *(uint32_t *)(g + (size_t)ey * A.pitch + ex) = v;
}

__global__ void __launch_bounds__(K9_COL_LANES) k9_cols(const k9_geo A, int tiles_x, const uint8_t *__restrict__ g, uint16_t *__restrict__ f)
{
    __shared__ __attribute__((aligned(16))) uint8_t tile_s[K9_TILE_BYTES];
    const int tid = threadIdx.x;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int ex0 = tx * K9_TX, ey0 = ty * K9_TY;
    const int rows = min(K9_TY, A.eh - ey0);
    const int srows = rows + 2 * A.r;                                      // staged rows: ey0 - r .. ey0 + rows - 1 + r
    const uint32_t gc = hs_df_outside_g(A.mask) * 0x01010101u;             // a row of E's outside: class 0 everywhere
    for (int j = tid; j < srows * (K9_TX / 4); j += K9_COL_LANES) {
        const int sr = j / (K9_TX / 4), ex = ex0 + 4 * (j - sr * (K9_TX / 4));
        const int ey = ey0 - A.r + sr;
        const bool in = ey >= 0 && ey < A.eh && ex < A.pitch;
        ((uint32_t *)tile_s)[j] = in ? *(const uint32_t *)(g + (size_t)ey * A.pitch + ex) : gc;
    }
    __syncthreads();
    const int lane = tid & 63, ex = ex0 + lane;
    if (ex >= A.ew) return;
    for (int ly = tid >> 6; ly < rows; ly += K9_COL_LANES / 64)
        f[(size_t)(ey0 + ly) * A.pitch + ex] = (uint16_t)hs_df_col_min(tile_s + (ly + A.r) * K9_TX + lane, K9_TX, A.r);
}

__global__ void __launch_bounds__(256) k9_gather(const hs_field E, int x, int y, int w, int n, uint16_t *__restrict__ out)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const int ry = j / w, rx = j - ry * w;
    out[j] = (uint16_t)hs_field_lookup(E, (long long)x + rx, (long long)y + ry);
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
        float exf, eyf;
        sh_v2_transform(p.x, p.y, t_s, &exf, &eyf);
        counted = hs_trace_counts(exf) && hs_trace_counts(eyf);
        if (counted) F = hs_field_lookup(A.E, (long long)sh_f2i(rintf(exf)), (long long)sh_f2i(rintf(eyf)));   // ToRoundPoint (banker's)
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
// What the field needs, made by the first call and kept: g and F of E, the poses in device memory, the device block of the
// results (summaries and point records, or a field call's rectangle), and the pinned block the poses leave and the results reach
// the host through.
struct hs_dfield {
    uint8_t *d_g; size_t cap_g;
    uint16_t *d_f; size_t cap_f;
    float *d_poses; size_t cap_poses;
    unsigned char *d_out; size_t cap_out;
    unsigned char *h_io; size_t cap_h;
};

void hs_df_free(slamhip_hs *hs)
{
    hs_dfield *df = hs->dfd;
    if (!df) return;
    hs_release((void **)&df->d_g, &df->cap_g, HS_MEM_DEVICE);
    hs_release((void **)&df->d_f, &df->cap_f, HS_MEM_DEVICE);
    hs_release((void **)&df->d_poses, &df->cap_poses, HS_MEM_DEVICE);
    hs_release((void **)&df->d_out, &df->cap_out, HS_MEM_DEVICE);
    hs_release((void **)&df->h_io, &df->cap_h, HS_MEM_PINNED);
    delete df;
    hs->dfd = nullptr;
}

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
    if (B < 1 || B > HS_DF_MAX_POSES) SH_FAIL(SLAMHIP_ERR_INVALID, "distance score: B = %d must lie in [1, %d]", B, HS_DF_MAX_POSES);
    if (scan_is_set && n_points <= 0) SH_FAIL(SLAMHIP_ERR_STATE, "distance score: no scan (slamhip_hs_set_scan first)");
    if (want_points && (int64_t)B * n_points > HS_DF_MAX_POINTS)
        SH_FAIL(SLAMHIP_ERR_INVALID, "distance score: per-point records of %d poses x %d points, more than 2^22", B, n_points);
    return SLAMHIP_OK;
}

// The plan of one field, for this unit's calls and for other units' launches (K11's clearance, K13's weights): the class map
// prepared (the world's plan refuses before anything is launched), E sized and refused if too large, the hs's block made if this is
// its first use, g and F grown.  Nothing is launched.
int32_t hs_df_field_prepare(slamhip_hs *hs, int level, bool world, int site_mask, int radius, hs_class_map *M, hs_field *E)
{
    SH_TRY(hs_lat_pack_prepare(hs, level, world, M));
    const int64_t ew = (int64_t)M->w + 2 * radius, eh = (int64_t)M->h + 2 * radius;
    if (ew * eh > HS_DF_MAX_E)
        SH_FAIL(SLAMHIP_ERR_INVALID, "distance field: E, the map of level %d grown by the radius, is %lld x %lld cells, more than 2^26", level,
                (long long)ew, (long long)eh);
    SH_TRY(hs_unit(&hs->dfd));
    hs_dfield *df = hs->dfd;
    E->ew = (int)ew; E->eh = (int)eh; E->pitch = ((int)ew + 3) & ~3;
    E->e_x0 = M->x0 - radius; E->e_y0 = M->y0 - radius;                    // (-2^28 < x0 <= 0: no overflow)
    E->outside = hs_df_outside(site_mask, radius);
    const size_t cells = (size_t)E->pitch * (size_t)E->eh;
    SH_TRY(hs_grow((void **)&df->d_g, &df->cap_g, cells, HS_MEM_DEVICE, "distance field"));
    SH_TRY(hs_grow((void **)&df->d_f, &df->cap_f, cells * sizeof(uint16_t), HS_MEM_DEVICE, "distance field"));
    E->f = df->d_f;
    return SLAMHIP_OK;
}

// the class map's pack and the two launches of the planned field, on the operator's stream (no timing class of their own)
int32_t hs_df_field_enqueue(slamhip_hs *hs, int level, bool world, const hs_class_map *M, const hs_field *E, int site_mask)
{
    hs_dfield *df = hs->dfd;
    SH_TRY(hs_lat_pack_enqueue(hs, level, world, M));
    k9_geo G;
    G.cls = M->cls; G.w = M->w; G.h = M->h; G.wpr = M->wpr;
    G.r = M->x0 - E->e_x0; G.mask = site_mask;
    G.ew = E->ew; G.eh = E->eh; G.pitch = E->pitch;
    const int segs = sh_div_up(G.pitch, K9_SEG), tiles_x = sh_div_up(G.ew, K9_TX), tiles_y = sh_div_up(G.eh, K9_TY);
    // (at most 2^26 cells in E: neither grid reaches 2^31 workgroups)
    hipLaunchKernelGGL(k9_rows, dim3((unsigned)segs * (unsigned)G.eh), dim3(K9_ROW_LANES), 0, hs->ctx->stream, G, segs, df->d_g);
    SH_HIP(hipGetLastError());
    hipLaunchKernelGGL(k9_cols, dim3((unsigned)tiles_x * (unsigned)tiles_y), dim3(K9_COL_LANES), 0, hs->ctx->stream, G, tiles_x, (const uint8_t *)df->d_g, df->d_f);
    SH_HIP(hipGetLastError());
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_distance_field(slamhip_hs *hs, int32_t level, int32_t world, int32_t site_mask, int32_t radius,
                                             int32_t x, int32_t y, int32_t w, int32_t h, uint16_t *out_d2)
{
    SH_CHECK_ARG(hs && out_d2);
    SH_TRY(hs_df_check("distance field", hs->n_levels, level, world, site_mask, radius));
    if (w < 1 || h < 1 || (int64_t)w * h > HS_DF_MAX_RECT)
        SH_FAIL(SLAMHIP_ERR_INVALID, "distance field: a rectangle of %d x %d cells; w, h >= 1 and w * h <= 2^24", w, h);
    slamhip_ctx *ctx = hs->ctx;
    SH_TRY(hs_call_begin(hs));
    hs_class_map M; hs_field E;
    SH_TRY(hs_df_field_prepare(hs, level, world != 0, site_mask, radius, &M, &E));
    hs_dfield *df = hs->dfd;
    const int n = w * h;
    const size_t out_bytes = sizeof(uint16_t) * (size_t)n;
    SH_TRY(hs_grow((void **)&df->d_out, &df->cap_out, out_bytes, HS_MEM_DEVICE, "distance field"));
    SH_TRY(hs_grow((void **)&df->h_io, &df->cap_h, out_bytes, HS_MEM_PINNED, "distance field"));
    SH_TRY(hs_df_field_enqueue(hs, level, world != 0, &M, &E, site_mask));
    hipLaunchKernelGGL(k9_gather, dim3((unsigned)sh_div_up(n, 256)), dim3(256), 0, ctx->stream, E, x, y, w, n, (uint16_t *)df->d_out);
    SH_HIP(hipGetLastError());
    SH_HIP(hipMemcpyAsync(df->h_io, df->d_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    SH_TRY(hs_call_finish(hs));
    memcpy(out_d2, df->h_io, out_bytes);
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_distance_score(slamhip_hs *hs, int32_t level, int32_t world, int32_t site_mask, int32_t radius,
                                             const float *poses, int32_t B, slamhip_distance_summary *out_summaries, uint16_t *out_points)
{
    SH_CHECK_ARG(hs && poses && out_summaries);
    SH_TRY(hs_df_check_score("distance field", hs->n_levels, level, world, site_mask, radius, B, out_points != nullptr, hs->n_points, true));
    const int n = hs->n_points;
    slamhip_ctx *ctx = hs->ctx;
    SH_TRY(hs_call_begin(hs));
    const int chunks = sh_div_up(n, K9S_LANES);
    if ((int64_t)B * chunks > (int64_t)INT32_MAX) SH_FAIL(SLAMHIP_ERR_INVALID, "distance score: %d poses x %d points, more workgroups than one launch takes", B, n);
    hs_class_map M; hs_field E;
    SH_TRY(hs_df_field_prepare(hs, level, world != 0, site_mask, radius, &M, &E));
    hs_dfield *df = hs->dfd;
    const size_t pose_bytes = sizeof(float) * 3 * (size_t)B;
    const size_t sum_bytes = sizeof(slamhip_distance_summary) * (size_t)B;
    const size_t pts_bytes = out_points ? sizeof(uint16_t) * (size_t)B * n : 0;
    const size_t out_bytes = (sum_bytes + pts_bytes + 7) & ~(size_t)7;     // (the poses follow, 8-byte aligned)
    SH_TRY(hs_grow((void **)&df->d_poses, &df->cap_poses, pose_bytes, HS_MEM_DEVICE, "distance field"));
    SH_TRY(hs_grow((void **)&df->d_out, &df->cap_out, out_bytes, HS_MEM_DEVICE, "distance field"));
    SH_TRY(hs_grow((void **)&df->h_io, &df->cap_h, out_bytes + pose_bytes, HS_MEM_PINNED, "distance field"));
    float *h_poses = (float *)(df->h_io + out_bytes);
    memcpy(h_poses, poses, pose_bytes);
    SH_TRY(hs_flush_scan(hs));
    SH_HIP(hipMemcpyAsync(df->d_poses, h_poses, pose_bytes, hipMemcpyHostToDevice, ctx->stream));
    SH_HIP(hipMemsetAsync(df->d_out, 0, sum_bytes, ctx->stream));
    SH_TRY(hs_df_field_enqueue(hs, level, world != 0, &M, &E, site_mask));
    k9s_arg A;
    A.pts = hs->d_pts; A.n = n;
    A.poses = df->d_poses; A.chunks = chunks;
    A.stm = hs->lv[level].stm;
    A.E = E; A.r2 = radius * radius;
    A.sums = (slamhip_distance_summary *)df->d_out;
    A.points = out_points ? (uint16_t *)(df->d_out + sum_bytes) : (uint16_t *)nullptr;
    hipLaunchKernelGGL(k9_score, dim3((unsigned)(B * chunks)), dim3(K9S_LANES), 0, ctx->stream, A);
    SH_HIP(hipGetLastError());
    SH_HIP(hipMemcpyAsync(df->h_io, df->d_out, sum_bytes + pts_bytes, hipMemcpyDeviceToHost, ctx->stream));
    SH_TRY(hs_call_finish(hs));
    memcpy(out_summaries, df->h_io, sum_bytes);
    if (out_points) memcpy(out_points, df->h_io + sum_bytes, pts_bytes);
    return SLAMHIP_OK;
}

// CPU-side test hook: the field of the definition over a caller's class array, by hs_dfield.h -- the text the kernels run.  The
// classes are packed as K7 packs them; for the rows and columns of E the rectangle touches, g by hs_df_site_word and
// hs_df_row_nearest over r more rows above and below, then F by hs_df_col_min.
extern "C" int32_t slamhip_debug_distance_field(const uint8_t *cls, int32_t cw, int32_t ch, int32_t site_mask, int32_t radius,
                                                int32_t x, int32_t y, int32_t w, int32_t h, uint16_t *out_d2)
{
    SH_CHECK_ARG(cls && out_d2 && cw >= 1 && ch >= 1 && (int64_t)cw * ch <= HS_DF_MAX_E);
    if (site_mask < 1 || site_mask > 7) SH_FAIL(SLAMHIP_ERR_INVALID, "distance field: site_mask = %d must lie in [1, 7]", site_mask);
    if (radius < 1 || radius > HS_DF_MAX_RADIUS) SH_FAIL(SLAMHIP_ERR_INVALID, "distance field: radius = %d must lie in [1, %d]", radius, HS_DF_MAX_RADIUS);
    if (w < 1 || h < 1 || (int64_t)w * h > HS_DF_MAX_RECT)
        SH_FAIL(SLAMHIP_ERR_INVALID, "distance field: a rectangle of %d x %d cells; w, h >= 1 and w * h <= 2^24", w, h);
    const int r = radius;
    const uint16_t outside = (uint16_t)hs_df_outside(site_mask, r);
    for (int64_t j = 0; j < (int64_t)w * h; j++) out_d2[j] = outside;
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
    std::vector<uint8_t> g((size_t)nx * (size_t)(ny + 2 * r));             // rows ay0 - r .. ay1 - 1 + r
    for (int gy = 0; gy < ny + 2 * r; gy++) {
        const int64_t my = ay0 - r + gy;
        uint8_t *grow = g.data() + (size_t)gy * nx;
        if (my < -r || my >= (int64_t)ch + r) { memset(grow, (int)hs_df_outside_g(site_mask), (size_t)nx); continue; }   // a row outside E
        const uint32_t *row = (my >= 0 && my < ch) ? packed.data() + (size_t)my * wpr : (const uint32_t *)nullptr;
        for (int j = 0; j < nw; j++) bits[(size_t)j] = hs_df_site_word(row, cw, bmx0 + 32 * j, site_mask);
        for (int i = 0; i < nx; i++) grow[i] = (uint8_t)hs_df_row_nearest(bits.data(), nw, (int)ax0 + i - bmx0, r);
    }
    for (int iy = 0; iy < ny; iy++)
        for (int i = 0; i < nx; i++)
            out_d2[(size_t)(ay0 + iy - y) * (size_t)w + (size_t)(ax0 + i - x)] = (uint16_t)hs_df_col_min(g.data() + (size_t)(iy + r) * nx + i, nx, r);
    return SLAMHIP_OK;
}
