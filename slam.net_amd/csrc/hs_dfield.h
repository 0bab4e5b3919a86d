// hs_dfield.h -- the arithmetic of the distance field (K9, hs_dfield.hip) that host and device share: the kernels k9_rows and
// k9_cols and the test hook slamhip_debug_distance_field run this text, and every reader of a field over E -- k9_score, k16_pairs,
// hs_field_gather, K13's k13_score and slamhip_debug_mcl_step -- looks it up through hs_field_lookup.  Definition: include/slamhip.h, slamhip_hs_distance_field.
// Everything here is integer arithmetic; the end cell of a scan point is hs_trace.h's transform.
#pragma once
#include "common.h"

#define HS_DF_MAX_RADIUS 255
#define HS_DF_NONE 255                     // the byte of a cell with no site within r in its row -- see hs_df_row_nearest

// the constant of the field where no site of the map can reach: every cell there is class 0, a site iff bit 0 of the mask is set
__host__ __device__ static inline uint32_t hs_df_outside(int site_mask, int r) { return (site_mask & 1) ? 0u : (uint32_t)(r * r); }
// ... and the row distance of such a cell
__host__ __device__ static inline uint32_t hs_df_outside_g(int site_mask) { return (site_mask & 1) ? 0u : (uint32_t)HS_DF_NONE; }

__host__ __device__ static inline int hs_df_ctz(uint32_t v)                // v != 0
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __ffs((int)v) - 1;
#else
    return __builtin_ctz(v);
#endif
}
__host__ __device__ static inline int hs_df_clz(uint32_t v)                // v != 0
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __clz((int)v);
#else
    return __builtin_clz(v);
#endif
}

// The class-to-site test on one packed word of K7's class map: 16 cells of 2 class bits each -> 16 site bits, bit b set iff bit
// cls(b) of site_mask is set.  Only the first `n` cells of the word are cells of the map (n in [0, 16]); the others -- a row's
// padding, or a word that lies outside the map altogether (n = 0) -- are class 0 whatever the word holds.
__host__ __device__ static inline uint32_t hs_df_site_bits16(uint32_t word, int n, int site_mask)
{
    if (n < 16) word &= (1u << (2 * n)) - 1u;                              // (n == 0: nothing of the word is kept)
    const uint32_t lo = word & 0x55555555u, hi = (word >> 1) & 0x55555555u;
    uint32_t s = 0;                                                        // the site bits on the even positions
    if (site_mask & 1) s |= ~(lo | hi) & 0x55555555u;                      // class 0
    if (site_mask & 2) s |= lo & ~hi;                                      // class 1, occupied
    if (site_mask & 4) s |= hi & ~lo;                                      // class 2, free
    s = (s | (s >> 1)) & 0x33333333u;                                      // the even bits moved together
    s = (s | (s >> 2)) & 0x0F0F0F0Fu;
    s = (s | (s >> 4)) & 0x00FF00FFu;
    s = (s | (s >> 8)) & 0x0000FFFFu;
    return s;
}

// The site bits of the 32 cells [mx32, mx32 + 32) of one row of the class map, mx32 a multiple of 32 (it may be negative: cells
// left of the map).  row: the row's packed words, or nullptr for a row above or below the map; w: the map's width in cells.
__host__ __device__ static inline uint32_t hs_df_site_word(const uint32_t *row, int w, int mx32, int site_mask)
{
    uint32_t out = 0;
    for (int half = 0; half < 2; half++) {
        const int cx = mx32 + 16 * half;                                   // a multiple of 16: the 16 cells lie in ONE packed word, or all outside
        const bool in = row && cx >= 0 && cx < w;
        const int n = in ? (w - cx < 16 ? w - cx : 16) : 0;
        out |= hs_df_site_bits16(in ? row[cx >> 4] : 0u, n, site_mask) << (16 * half);
    }
    return out;
}

// The nearest-site-in-a-row primitive.  bits: nwords words of site bits, 32 cells per word, bit p the cell asked for.  Returns the
// distance |d| <= r to the nearest set bit, or HS_DF_NONE if there is none within r (bits outside the array count as clear: the
// caller's array reaches r cells past p on both sides).  The byte 255 is EXACT although it stands for two things: a true distance
// of 255 (r = 255 only) and "none within r" both mean g >= r, so g * g >= r * r, and the field's cap min(., r * r) makes the two
// equal.  By word with ctz / clz, moving outward, never cell by cell; a side stops where it can no longer beat the other.
__host__ __device__ static inline uint32_t hs_df_row_nearest(const uint32_t *bits, int nwords, int p, int r)
{
    const int wi = p >> 5, b = p & 31;
    int best = r + 1;                                                      // nothing found yet: only d <= r counts
    const uint32_t self = bits[wi];
    const uint32_t right = self >> b;                                      // bit 0: the cell itself
    if (right) best = hs_df_ctz(right);
    else
        for (int k = 1; 32 * k - b < best; k++) {                          // (32 k - b: the distance of bit 0 of word wi + k)
            if (wi + k >= nwords) break;
            const uint32_t v = bits[wi + k];
            if (v) { const int d = 32 * k - b + hs_df_ctz(v); if (d < best) best = d; break; }
        }
    const uint32_t left = self << (31 - b);                                // bit 31: the cell itself
    if (left) { const int d = hs_df_clz(left); if (d < best) best = d; }
    else
        for (int k = 1; b + 1 + 32 * (k - 1) < best; k++) {                // (the distance of bit 31 of word wi - k)
            if (wi - k < 0) break;
            const uint32_t v = bits[wi - k];
            if (v) { const int d = b + 1 + 32 * (k - 1) + hs_df_clz(v); if (d < best) best = d; break; }
        }
    return best <= r ? (uint32_t)best : (uint32_t)HS_DF_NONE;              // (best <= r <= 255)
}

// The column minimum: min(r * r, min over |dy| <= r of g(dy)^2 + dy^2), g(dy) = g[dy * stride] the row distances of the column's
// cells (the caller's array reaches r rows up and down).  dy walks outward from 0 and stops once dy * dy alone is no better than
// the best so far; dy = r can never lower r * r.
__host__ __device__ static inline uint32_t hs_df_col_min(const uint8_t *g, int stride, int r)
{
    const uint32_t g0 = g[0], cap = (uint32_t)(r * r);
    uint32_t best = g0 * g0 < cap ? g0 * g0 : cap;
    for (int dy = 1; (uint32_t)(dy * dy) < best; dy++) {                   // (best <= r * r: dy stays below r)
        const uint32_t a = g[-dy * stride], c = g[dy * stride];
        const uint32_t m = a < c ? a : c;
        const uint32_t v = m * m + (uint32_t)(dy * dy);
        if (v < best) best = v;
    }
    return best;
}

// A field over E as a launch reads it -- K9's F (hs_field, uint16_t) or K16's N (hs_nfield, hs_nearest.h) -- E = M grown by r cells on
// every side, rows of `pitch` cells; E's first cell is (e_x0, e_y0) in the window's frame -- r = M's x0 - e_x0 -- and outside E the
// field is the constant `outside` (hs_df_outside, hs_nr_outside).  The kernels and the host plan that make one: hs_field.h.
template <typename T>
struct hs_field_of { const T *f; int ew, eh, pitch, e_x0, e_y0; uint32_t outside; };
typedef hs_field_of<uint16_t> hs_field;

// the field's value at window-frame cell (x, y)
template <typename T>
__host__ __device__ static inline uint32_t hs_field_lookup(const hs_field_of<T> &E, long long x, long long y)
{
    const long long ex = x - E.e_x0, ey = y - E.e_y0;
    const bool in = ex >= 0 && ex < E.ew && ey >= 0 && ey < E.eh;
    return in ? (uint32_t)E.f[(size_t)ey * (size_t)E.pitch + (size_t)ex] : E.outside;
}
