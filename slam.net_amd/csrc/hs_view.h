// hs_view.h -- the arithmetic of the view gain (K15, hs_view.hip) that host and device share: the kernels k15_view, k15_gain and
// k15_pick and the test hook slamhip_debug_view run this text.  Definition: include/slamhip.h, slamhip_view_summary.  Lines and
// walks are hs_trace.h's, the 1-bit class words hs_df_site_word's (hs_dfield.h); everything here is integer arithmetic.
// A SEEN WORD holds the seen bits of 32 consecutive cells of one row of the window (bit b: cell 32 j + b), the layout of K10's
// frontier words and of the covered layer.
#pragma once
#include "hs_dfield.h"
#include "hs_lattice.h"
#include "hs_trace.h"

#define HS_VIEW_MAX_REACH 4096
#define HS_VIEW_MAX_POSES 4096
#define HS_VIEW_MAX_K 64
#define HS_VIEW_MAX_SCRATCH ((int64_t)1 << 25)   // words of the slots of one call: 128 MB
#define K15_LDS_WORDS 8704                 // words of a slot that k15_view keeps in LDS (34 KB; reach 255: 511 rows x 17 words = 8687)

// the fields of slamhip_view_summary, in their order
enum { HS_VIEW_C_WALKED, HS_VIEW_C_SAME, HS_VIEW_C_IGNORED, HS_VIEW_C_CUT, HS_VIEW_C_SEEN, HS_VIEW_C_UNKNOWN, HS_VIEW_C_FREE, HS_VIEW_C_OCCUPIED,
       HS_VIEW_C_NEW, HS_VIEW_C_NEW_UNKNOWN, HS_VIEW_CTRS };

__host__ __device__ static inline int hs_view_popc(uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __popc(v);
#else
    return __builtin_popcount(v);
#endif
}

// The box of a pose: the cells within `reach` of the sensor cell b, clipped to the window of w x h cells, its left edge aligned
// down to a seen word -- words [xw0, xw0 + nwpr) of rows [y0, y0 + rows).  Every cell a beam of the pose can see lies in it (step
// a lies at Chebyshev distance a <= reach from b).  Empty (nwpr = rows = 0): b does not count, or no cell of the window is that near.
struct hs_view_box { int32_t xw0, y0, nwpr, rows; };

__host__ __device__ static inline hs_view_box hs_view_box_of(const sh_m3x2 &t, float ox, float oy, int reach, int w, int h)
{
    hs_view_box B = { 0, 0, 0, 0 };
    const hs_trace_line l = hs_trace_line_of(t, ox, oy, ox, oy);           // the beam to the origin itself: b = e, or ignored
    if (l.da < 0) return B;
    const int x_lo = l.bx - reach > 0 ? l.bx - reach : 0, x_hi = l.bx + reach < w - 1 ? l.bx + reach : w - 1;    // (|b| <= 2^24, reach <= 4096)
    const int y_lo = l.by - reach > 0 ? l.by - reach : 0, y_hi = l.by + reach < h - 1 ? l.by + reach : h - 1;
    if (x_lo > x_hi || y_lo > y_hi) return B;
    B.xw0 = x_lo >> 5; B.nwpr = (x_hi >> 5) - B.xw0 + 1;
    B.y0 = y_lo; B.rows = y_hi - y_lo + 1;
    return B;
}

// The slot of a call: what the box of ANY pose fits -- 2 reach + 1 cells starting anywhere in a word take (2 reach + 63) / 32 words.
__host__ __device__ static inline int hs_view_slot_rows(int reach, int h) { return 2 * reach + 1 < h ? 2 * reach + 1 : h; }
__host__ __device__ static inline int hs_view_slot_wpr(int reach, int w)
{
    const int a = (2 * reach + 63) / 32, b = (w + 31) / 32;
    return a < b ? a : b;
}

// the word of cell (x, y) in the box's slot, or -1: the cell lies outside the window (it is never seen) or outside the box
__host__ __device__ static inline int hs_view_slot_word(const hs_view_box &B, int w, int h, int x, int y)
{
    if (!((unsigned)x < (unsigned)w && (unsigned)y < (unsigned)h)) return -1;
    const int r = y - B.y0, c = (x >> 5) - B.xw0;
    if (!((unsigned)r < (unsigned)B.rows && (unsigned)c < (unsigned)B.nwpr)) return -1;
    return r * B.nwpr + c;
}

// The stop rule.  A walked beam sees steps 0 .. min(first, da, reach): the walk looks no further than hs_view_last, and ends at the
// first occupied cell it sees.  hit: an occupied cell was met at a step <= hs_view_last.
__host__ __device__ static inline int hs_view_last(int da, int reach) { return da < reach ? da : reach; }
__host__ __device__ static inline bool hs_view_cut(int da, bool hit, int reach) { return da > reach && !hit; }

// the 1-bit class words of the 32 cells [mx32, mx32 + 32) of row y of K7's class map (rows of wpr16 words), y in [0, h)
__host__ __device__ static inline void hs_view_class_words(const uint32_t *cls, int wpr16, int w, int y, int mx32, uint32_t *unk, uint32_t *fre, uint32_t *occ)
{
    const uint32_t *row = cls + (size_t)y * wpr16;
    *unk = hs_df_site_word(row, w, mx32, 1);
    *occ = hs_df_site_word(row, w, mx32, 2);
    *fre = hs_df_site_word(row, w, mx32, 4);
}

// the summary's word rule: what one seen word adds to the counts, against its class words and the covered word
__host__ __device__ static inline void hs_view_word_counts(uint32_t seen, uint32_t unk, uint32_t fre, uint32_t occ, uint32_t cov, int c[HS_VIEW_CTRS])
{
    c[HS_VIEW_C_SEEN] += hs_view_popc(seen);
    c[HS_VIEW_C_UNKNOWN] += hs_view_popc(seen & unk);
    c[HS_VIEW_C_FREE] += hs_view_popc(seen & fre);
    c[HS_VIEW_C_OCCUPIED] += hs_view_popc(seen & occ);
    c[HS_VIEW_C_NEW] += hs_view_popc(seen & ~cov);
    c[HS_VIEW_C_NEW_UNKNOWN] += hs_view_popc(seen & ~cov & unk);
}

// ... and the gain's: mode 0 n_new, mode 1 n_new_unknown
__host__ __device__ static inline int hs_view_word_gain(uint32_t seen, uint32_t unk, uint32_t cov, int mode)
{
    return hs_view_popc(seen & ~cov & (mode ? unk : 0xFFFFFFFFu));
}

// The choice rule: the largest gain, ties to the lowest pose index, as the maximum of one key.  A pose already chosen carries
// gain -1, below every other; the choice stops when the best gain lies below min_gain (>= 1).
__host__ __device__ static inline unsigned long long hs_view_key(int gain, int index)
{
    return ((unsigned long long)(uint32_t)(gain + 1) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)index);
}
__host__ __device__ static inline int hs_view_key_gain(unsigned long long key) { return (int)(uint32_t)(key >> 32) - 1; }
__host__ __device__ static inline int hs_view_key_index(unsigned long long key) { return (int)(0xFFFFFFFFu - (uint32_t)key); }
__host__ __device__ static inline bool hs_view_stops(int gain, int min_gain) { return gain < min_gain; }
