// hs_nearest.h -- the arithmetic of the nearest-site field (K16, hs_nearest.hip) that host and device share: the kernels k16_rows,
// k16_cols and k16_pairs and the test hook slamhip_debug_nearest_field run this text.  Definition: include/slamhip.h,
// slamhip_hs_nearest_field.  Everything here is integer arithmetic on top of hs_dfield.h's site words; the end cell of a scan point
// is hs_trace.h's transform.
#pragma once
#include "hs_dfield.h"

#define HS_NR_NONE 32767                   // INT16_MAX: a row offset, a dy or a component of the pair when there is no site
#define HS_NR_IGNORED (-32768)             // INT16_MIN: both components of the per-point record of an ignored point
#define HS_NR_MAG_NONE 255                 // the magnitude byte of HS_NR_NONE: 255^2 >= r^2 for every r, so it can never win
#define HS_NR_PAIR_NONE 0x7FFF7FFFu        // (HS_NR_NONE, HS_NR_NONE) as one word
#define HS_NR_PAIR_IGNORED 0x80008000u     // (HS_NR_IGNORED, HS_NR_IGNORED)

// a pair (dx, dy) of int16_t as the one word it is stored as: dx the low half
__host__ __device__ static inline uint32_t hs_nr_pack(int dx, int dy) { return (uint32_t)(uint16_t)(int16_t)dx | ((uint32_t)(uint16_t)(int16_t)dy << 16); }
__host__ __device__ static inline int hs_nr_dx(uint32_t pair) { return (int)(int16_t)(uint16_t)(pair & 0xFFFFu); }
__host__ __device__ static inline int hs_nr_dy(uint32_t pair) { return (int)(int16_t)(uint16_t)(pair >> 16); }

// the pair of a cell no site of the map can reach: every cell there is class 0, itself a site iff bit 0 of the mask is set
__host__ __device__ static inline uint32_t hs_nr_outside(int site_mask) { return (site_mask & 1) ? 0u : HS_NR_PAIR_NONE; }
// ... and the row offset of such a cell
__host__ __device__ static inline int hs_nr_outside_g(int site_mask) { return (site_mask & 1) ? 0 : HS_NR_NONE; }

// a row offset as the column pass keeps it: the magnitude as a byte (at most 254, HS_NR_MAG_NONE for none) and the sign apart
__host__ __device__ static inline uint32_t hs_nr_mag(int off) { return off == HS_NR_NONE ? (uint32_t)HS_NR_MAG_NONE : (uint32_t)(off < 0 ? -off : off); }

// The signed nearest-site-in-a-row primitive.  bits: nwords words of site bits, 32 cells per word, bit p the cell asked for (bits
// outside the array count as clear: the caller's array reaches r cells past p on both sides).  Returns the offset d = sx - p of the
// nearest set bit with |d| < r -- only such a site can have D2 < r^2 -- or HS_NR_NONE.  A left/right tie goes to the LEFT, the
// smaller sx: the left side is searched first and the right side wins only where it is strictly nearer.  By word with clz / ctz,
// moving outward, never cell by cell; a side stops where it can no longer win.
__host__ __device__ static inline int hs_nr_row_nearest(const uint32_t *bits, int nwords, int p, int r)
{
    const int wi = p >> 5, b = p & 31;
    int best = r;                                                          // nothing found yet: only d < r counts
    bool right_won = false;
    const uint32_t self = bits[wi];
    const uint32_t left = self << (31 - b);                                // bit 31: the cell itself
    if (left) { const int d = hs_df_clz(left); if (d < best) best = d; }
    else
        for (int k = 1; b + 1 + 32 * (k - 1) < best; k++) {                // (the distance of bit 31 of word wi - k)
            if (wi - k < 0) break;
            const uint32_t v = bits[wi - k];
            if (v) { const int d = b + 1 + 32 * (k - 1) + hs_df_clz(v); if (d < best) best = d; break; }
        }
    const uint32_t right = self >> b;                                      // bit 0: the cell itself
    if (right) { const int d = hs_df_ctz(right); if (d < best) { best = d; right_won = true; } }
    else
        for (int k = 1; 32 * k - b < best; k++) {                          // (32 k - b: the distance of bit 0 of word wi + k)
            if (wi + k >= nwords) break;
            const uint32_t v = bits[wi + k];
            if (v) { const int d = 32 * k - b + hs_df_ctz(v); if (d < best) { best = d; right_won = true; } break; }
        }
    return best < r ? (right_won ? best : -best) : HS_NR_NONE;             // (the cell itself: best == 0 from the left, offset 0)
}

// The column arg-min: the dy with |dy| < r that minimises the key (m(dy)^2 + dy^2, dy) among those whose first part is below r^2,
// m(dy) = m[dy * stride] the magnitude bytes of the column's row offsets (the caller's array reaches r rows up and down); HS_NR_NONE
// if there is none.  k = |dy| walks outward from 0 and stops once k^2 alone can neither beat nor tie the best so far; dy = -k is
// taken before +k and wins an equal D2 against everything seen before it -- all of which lies in a larger row -- while +k must be
// strictly better: the smaller row wins ties.
__host__ __device__ static inline int hs_nr_col_argmin(const uint8_t *m, int stride, int r)
{
    const int cap = r * r, m0 = (int)m[0];
    int best = cap, bdy = HS_NR_NONE;
    if (m0 * m0 < cap) { best = m0 * m0; bdy = 0; }
    for (int k = 1; k < r && k * k <= best; k++) {
        const int a = (int)m[-k * stride], c = (int)m[k * stride], kk = k * k;
        const int va = a * a + kk, vc = c * c + kk;
        if (va <= best && va < cap) { best = va; bdy = -k; }
        if (vc < best) { best = vc; bdy = k; }
    }
    return bdy;
}

// The nearest-site field as a launch reads it: N over E, a packed pair per cell, `outside` hs_nr_outside (hs_field_of, hs_dfield.h)
typedef hs_field_of<uint32_t> hs_nfield;
