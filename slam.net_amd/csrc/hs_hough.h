// hs_hough.h -- the arithmetic of the Hough transform of a map (K17, hs_hough.hip) that host and device share: the kernels k17_vote,
// k17_spectrum, k17_xcorr and k17_xcorr_finish and the test hooks slamhip_debug_hough_table / _hough / _hough_xcorr run this text.
// Definition: include/slamhip.h, slamhip_hs_hough.  Everything here is integer arithmetic except the table, which the HOST forms in
// binary64 and hands to every launch; the sites are hs_dfield.h's site words.
#pragma once
#include "common.h"
#include "hs_dfield.h"

#define HS_HG_MIN_T 4
#define HS_HG_MAX_T 1024                   // angles: a multiple of 4
#define HS_HG_MAX_Q 3                      // the bin width is 2^q cells
#define HS_HG_MAX_DIM 16384                // w and h of M: the bin's argument stays below 2^31
#define HS_HG_MAX_BINS ((int64_t)1 << 24)  // T * N: 64 MB of H
#define HS_HG_MAX_PAIRS 256
#define HS_HG_MAX_XC ((int64_t)1 << 22)    // P * (N_d + N_s - 1) with the XC arrays asked for: 32 MB
#define HS_HG_ONE 16384                    // the table's scale, 2^14

#include <math.h>
// step 1: cs[0 .. T) = C, cs[T .. 2T) = S.  A host function: the device never forms a sine.
static inline void hs_hough_table(int T, int32_t *cs)
{
    int32_t *C = cs, *S = cs + T;
    C[0] = HS_HG_ONE; S[0] = 0;
    C[T / 2] = 0; S[T / 2] = HS_HG_ONE;
    for (int k = 1; k < T / 2; k++) {
        const double a = ((double)k * M_PI) / (double)T;
        C[k] = (int32_t)rint(16384.0 * cos(a));
        S[k] = (int32_t)rint(16384.0 * sin(a));
    }
    for (int k = T / 2 + 1; k < T; k++) { C[k] = -C[T - k]; S[k] = S[T - k]; }
}

// step 2: D and N of a w x h map
__host__ __device__ static inline int hs_hough_D(int w, int h) { return w + h; }
__host__ __device__ static inline int hs_hough_N(int D, int q) { return ((2 * D) >> q) + 1; }
// step 2: the bin of array cell (i, j) at an angle with table entries (c, s).  The argument is never negative and lies below 2^31
// for w, h <= 16384; the bin is below N.
__host__ __device__ static inline uint32_t hs_hough_bin(int i, int j, int c, int s, int D, int q)
{
    return (uint32_t)(i * c + j * s + D * HS_HG_ONE) >> (14 + q);
}

// The site bits of the 32 cells [mx32, mx32 + 32) of one row of M, mx32 a multiple of 32 and at least 0.  K9's rule for which cell is a
// site (hs_df_site_word), but cells outside M do not exist here: a row below the map and the cells right of it have no site bit
// whatever the mask says.
__host__ __device__ static inline uint32_t hs_hough_site_word(const uint32_t *row, int w, int mx32, int site_mask)
{
    const int n = w - mx32;
    if (!row || n <= 0) return 0u;
    const uint32_t v = hs_df_site_word(row, w, mx32, site_mask);
    return n < 32 ? v & ((1u << n) - 1u) : v;
}

// step 5: the source row kk and the flip f of pair (m, k), m in [0, 2T), k in [0, T)
__host__ __device__ static inline void hs_hough_pair(int T, int m, int k, int *kk, int *f)
{
    int r = k - m, flip = 0;
    while (r < 0) { r += T; flip ^= 1; }                                   // (0, 1 or 2 additions)
    *kk = r; *f = flip;
}
// step 5: the bin of the source row that B[p'] is
__host__ __device__ static inline int hs_hough_b_index(int Ns, int f, int pp) { return f ? Ns - 1 - pp : pp; }

// step 5: the record's arg-max, kept as (best, shift, ties): `n` shifts whose smallest is d reach the value v.  Ties go to the
// smallest d; the order the candidates arrive in plays no part.
__host__ __device__ static inline void hs_hough_rec_add(unsigned long long *best, int *shift, int *ties, unsigned long long v, int d, int n)
{
    if (n == 0) return;
    if (*ties == 0 || v > *best) { *best = v; *shift = d; *ties = n; }
    else if (v == *best) { *ties += n; if (d < *shift) *shift = d; }
}
