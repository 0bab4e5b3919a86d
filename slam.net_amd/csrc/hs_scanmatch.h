// hs_scanmatch.h -- what K21's kernels (hs_scanmatch.hip), its host hook (slamhip_debug_scans_match) and the edge rule
// (slamhip_hs_scans_edges) share, ONE text for host and device: the raster cell of a reference point, the raster's 2-bit words, the
// dilation, val, the flat node index, the packed key and rule 6.  Definition: include/slamhip.h, slamhip_hs_scans_match.  The query's
// cells are K7's (hs_lattice.h, hs_lat_point_cell with stm = scale).  Everything behind the binary32 operations that place a point in
// a cell is an integer.
#pragma once
#include "common.h"
#include "hs_lattice.h"
#include "hs_sig.h"
#include <math.h>

#define HS_SM_MIN_HALF 16                  // H: a multiple of 16 in [16, 192]
#define HS_SM_MAX_HALF 192
#define HS_SM_MAX_N 64                     // nx, ny, nt
#define HS_SM_MAX_PAIRS 4096
#define HS_SM_MAX_NODES (1 << 20)          // per pair
#define HS_SM_MAX_CALL_NODES (1 << 26)     // per call
#define HS_SM_MAX_WORDS (2 * HS_SM_MAX_HALF * (2 * HS_SM_MAX_HALF / 16))   // 9216 words, 36 KB: the raster at H = 192
#define HS_SM_IGNORED (-(1 << 30))         // (gx, gy) of an ignored query point: with |ix|, |iy| <= 64 the sum stays negative, outside the raster

static_assert(sizeof(slamhip_scanmatch_spec) == 32 && sizeof(slamhip_scan_pair) == 20 && sizeof(slamhip_scanmatch_result) == 104,
              "the layouts of include/slamhip.h");

// what the call refuses for the spec alone
static inline bool hs_sm_spec_ok(const slamhip_scanmatch_spec &S)
{
    if (!(S.scale > 0.0f) || !(S.scale <= 3.402823466e38f)) return false;  // (NaN fails the first test, +inf the second)
    if (S.half < HS_SM_MIN_HALF || S.half > HS_SM_MAX_HALF || (S.half & 15)) return false;
    if (S.nx < 0 || S.nx > HS_SM_MAX_N || S.ny < 0 || S.ny > HS_SM_MAX_N || S.nt < 0 || S.nt > HS_SM_MAX_N) return false;
    if (!(fabsf(S.dtheta) <= 3.402823466e38f)) return false;
    return S.margin >= 0 && S.reserved == 0;
}
static inline long long hs_sm_nodes(const slamhip_scanmatch_spec &S) { return (long long)(2 * S.nt + 1) * (2 * S.ny + 1) * (2 * S.nx + 1); }

// rule 1: the raster cell of a reference point; false: the point is IGNORED (hs_sig_cell is K18's rule 2: u = 2 floor(fx) + 1).
// A cell outside [0, 2H)^2 is not ignored here: the caller tests it, and the point still counts in n_ref.
__host__ __device__ static inline bool hs_sm_ref_cell(float px, float py, float scale, int H, int *x, int *y)
{
    int u, v;
    if (!hs_sig_cell(px, py, scale, &u, &v)) return false;
    *x = ((u - 1) >> 1) + H; *y = ((v - 1) >> 1) + H;                       // (u - 1 is even: the shift is exact for negatives too)
    return true;
}

// The raster: rows of H / 8 words, 16 cells of 2 bits per word, cell x of a row in bits 2 (x & 15) and 2 (x & 15) + 1 of word x >> 4.
// Bit 1 of a cell: hit.  Bit 0: near and not hit.  So the two bits ARE val: 2 hit, 1 near, 0 neither.
__host__ __device__ static inline int hs_sm_wpr(int H) { return H >> 3; }
__host__ __device__ static inline uint32_t hs_sm_hit_bit(int x) { return 2u << (2 * (x & 15)); }
__host__ __device__ static inline int hs_sm_val(const uint32_t *ras, int H, int x, int y)
{
    if ((unsigned)x >= (unsigned)(2 * H) || (unsigned)y >= (unsigned)(2 * H)) return 0;
    return (int)((ras[y * hs_sm_wpr(H) + (x >> 4)] >> (2 * (x & 15))) & 3u);
}
// the hit bits of a word's 16 cells as 16 adjacent bits, and 16 adjacent bits back to bit 0 of 16 cells
__host__ __device__ static inline uint32_t hs_sm_hits16(uint32_t w)
{
    uint32_t x = (w >> 1) & 0x55555555u;
    x = (x | (x >> 1)) & 0x33333333u; x = (x | (x >> 2)) & 0x0F0F0F0Fu; x = (x | (x >> 4)) & 0x00FF00FFu; x = (x | (x >> 8)) & 0x0000FFFFu;
    return x;
}
__host__ __device__ static inline uint32_t hs_sm_spread16(uint32_t x)
{
    x = (x | (x << 8)) & 0x00FF00FFu; x = (x | (x << 4)) & 0x0F0F0F0Fu; x = (x | (x << 2)) & 0x33333333u; x = (x | (x << 1)) & 0x55555555u;
    return x;
}
// The dilation of one word (row r, word j) of a raster whose hit bits are final: the near bits of its 16 cells -- some cell of the
// 3 x 3 block round the cell, CLIPPED to the grid, is hit -- less the cells that are hit themselves.  Reads hit bits alone and the
// caller ORs the result into bit 0 of the word's cells, so every word may be dilated in place at the same time.
__host__ __device__ static inline uint32_t hs_sm_dilate_word(const uint32_t *ras, int H, int r, int j)
{
    const int wpr = hs_sm_wpr(H), rows = 2 * H;
    uint32_t near = 0;
    for (int rr = r - 1; rr <= r + 1; rr++) {
        if (rr < 0 || rr >= rows) continue;
        const uint32_t *row = ras + rr * wpr;
        const uint32_t h = hs_sm_hits16(row[j]);
        uint32_t m = h | (h << 1) | (h >> 1);
        if (j > 0) m |= hs_sm_hits16(row[j - 1]) >> 15;                    // the left word's last cell is cell 0's neighbour
        if (j + 1 < wpr) m |= (hs_sm_hits16(row[j + 1]) & 1u) << 15;       // the right word's first cell is cell 15's
        near |= m & 0xFFFFu;
    }
    return hs_sm_spread16(near & ~hs_sm_hits16(ras[r * wpr + j]));
}

// rule 2: heading k of a pair, K7's arithmetic
__host__ __device__ static inline float hs_sm_theta(const slamhip_scanmatch_spec &S, const float guess[3], int k) { return guess[2] + (float)k * S.dtheta; }
__host__ __device__ static inline hs_lat_heading hs_sm_heading(const slamhip_scanmatch_spec &S, const float guess[3], int k)
{
    return hs_lat_heading_of(S.scale, guess[0], guess[1], hs_sm_theta(S, guess, k));
}
// ... and the cell of a query point in raster coordinates; false: ignored for this heading
__host__ __device__ static inline bool hs_sm_query_cell(const hs_lat_heading &Hd, int H, float px, float py, int *gx, int *gy)
{
    if (!hs_lat_point_cell(Hd, px, py, gx, gy)) return false;
    *gx += H; *gy += H;                                                    // (|gx| < 2^24: no overflow)
    return true;
}

// rule 3: the flat node index (k in [-nt, nt], iy in [-ny, ny], ix in [-nx, nx]) and back; the packed key is K7's (hs_lat_key)
__host__ __device__ static inline uint32_t hs_sm_flat(const slamhip_scanmatch_spec &S, int k, int iy, int ix)
{
    return (uint32_t)(((k + S.nt) * (2 * S.ny + 1) + (iy + S.ny)) * (2 * S.nx + 1) + (ix + S.nx));
}
__host__ __device__ static inline void hs_sm_unflat(const slamhip_scanmatch_spec &S, uint32_t flat, int *k, int *iy, int *ix)
{
    const int NX = 2 * S.nx + 1, NY = 2 * S.ny + 1;
    *ix = (int)(flat % (uint32_t)NX) - S.nx;
    *iy = (int)((flat / (uint32_t)NX) % (uint32_t)NY) - S.ny;
    *k = (int)(flat / (uint32_t)(NX * NY)) - S.nt;
}
// rule 4: is a node of score s in N, b the best score
__host__ __device__ static inline bool hs_sm_in_set(int s, int b, int margin) { return s > 0 && s >= b - margin; }
// the ten integers of rule 4 in the order of slamhip_scanmatch_result: cnt, then the nine sums
#define HS_SM_SUMS 10
__host__ __device__ static inline void hs_sm_moments_add(long long m[HS_SM_SUMS], int k, int iy, int ix)
{
    m[0] += 1; m[1] += ix; m[2] += iy; m[3] += k;
    m[4] += ix * ix; m[5] += iy * iy; m[6] += k * k;
    m[7] += ix * iy; m[8] += ix * k; m[9] += iy * k;
}

// rule 6, binary64, one rounding per operation (the build's -ffp-contract=off; the pragma says it again for this function)
static inline double hs_sm_axis_weight(long long sum, long long sum2, int cnt, double u)
{
#pragma clang fp contract(off)
    const double n = (double)cnt;
    const double m = (double)sum / n;
    const double q = (double)sum2 / n;
    const double mm = m * m;
    double v = q - mm;
    if (!(v > 0.0)) v = 0.0;
    const double u2 = u * u;
    const double spread = v * u2;
    const double cell = u2 / 12.0;
    const double variance = spread + cell;
    return 1.0 / variance;
}
static inline void hs_sm_edge(const slamhip_scanmatch_spec &S, const slamhip_scan_pair &P, const slamhip_scanmatch_result &R, double z[3], double w[3], int32_t *valid)
{
#pragma clang fp contract(off)
    const float cxm = P.guess[0] * S.scale, cym = P.guess[1] * S.scale;    // binary32, as rule 2 forms them
    const double sc = (double)S.scale;
    const double ax = (double)cxm + (double)R.ix, ay = (double)cym + (double)R.iy;
    z[0] = ax / sc; z[1] = ay / sc;
    z[2] = (double)hs_sm_theta(S, P.guess, R.k);
    *valid = R.cnt > 0 ? 1 : 0;
    if (R.cnt <= 0) { w[0] = w[1] = w[2] = 0.0; return; }
    const double u = 1.0 / sc;
    const double ut = (S.nt == 0 || S.dtheta == 0.0f) ? 6.283185307179586 / 64.0 : fabs((double)S.dtheta);
    w[0] = hs_sm_axis_weight(R.sum_x, R.sum_xx, R.cnt, u);
    w[1] = hs_sm_axis_weight(R.sum_y, R.sum_yy, R.cnt, u);
    w[2] = hs_sm_axis_weight(R.sum_k, R.sum_kk, R.cnt, ut);
}
