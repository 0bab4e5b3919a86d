// hs_bnb.h -- the arithmetic of the branch-and-bound pose-lattice search (K24, hs_bnb.hip) that host and device share: the kernels,
// the host half of slamhip_hs_lattice_search_bnb and the test hook slamhip_debug_lattice_bnb run this text.  Definition:
// include/slamhip.h, slamhip_bnb_spec, rules 1 - 7.  Everything here is an integer; the point cells are K7's (hs_lattice.h).
#pragma once
#include "hs_lattice.h"

#define HS_BNB_MAX_TOP 8
#define HS_BNB_LEVELS (HS_BNB_MAX_TOP + 1)
#define HS_BNB_DEFAULT_BLOCKS (1 << 26)    // max_blocks = 0

// The frame of the pooled maps P_0 .. P_top of a class map of w x h cells: the map with a zero margin of mx cells (whole words) in
// front of every row and my rows in front of the first one.  mx, my >= 2^top - 1: a window that starts up to 2^top - 1 cells off the
// map still reaches into it; one that starts further off, or at or past the far edge, holds cells outside the map only -- class 0,
// which is what a cell outside the frame reads as.
struct hs_bnb_frame { int wpr, rows, mx, my; size_t words; };

__host__ __device__ static inline hs_bnb_frame hs_bnb_frame_of(int w, int h, int top)
{
    hs_bnb_frame F;
    F.my = (1 << top) - 1;
    F.mx = (F.my + 15) & ~15;
    F.wpr = (w + 15) / 16 + F.mx / 16;
    F.rows = h + F.my;
    F.words = (size_t)F.wpr * (size_t)F.rows;
    return F;
}

// rule 2, one doubling step on packed words.  The 2-bit codes are 1 occupied (+1), 0 neither, 2 free (-1); 3 never occurs.  The
// maximum BY VALUE of such codes: the low bit is the OR of the low bits, the high bit the AND of the high bits.
__host__ __device__ static inline uint32_t hs_bnb_max4(uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    return ((a | b | c | d) & 0x55555555u) | ((a & b & c & d) & 0xAAAAAAAAu);
}
// the 16 cells of a frame row from cell 16 wx + d on (row nullptr: a row past the frame); words past the row are zero
__host__ __device__ static inline uint32_t hs_bnb_shifted(const uint32_t *row, int wx, int wpr, int d)
{
    if (!row) return 0u;
    const int wo = wx + (d >> 4), sh = (d & 15) * 2;
    const uint32_t lo = wo < wpr ? row[wo] : 0u;
    if (!sh) return lo;
    const uint32_t hi = wo + 1 < wpr ? row[wo + 1] : 0u;
    return (lo >> sh) | (hi << (32 - sh));
}
// word wx of row y of P_h from P_{h-1} = prev, d = 2^(h-1): the maximum over the four offsets {0, d}^2
__host__ __device__ static inline uint32_t hs_bnb_pool_word(const uint32_t *prev, int wpr, int rows, int y, int wx, int d)
{
    const uint32_t *r0 = prev + (size_t)y * wpr;
    const uint32_t *r1 = y + d < rows ? prev + (size_t)(y + d) * wpr : (const uint32_t *)nullptr;
    return hs_bnb_max4(r0[wx], hs_bnb_shifted(r0, wx, wpr, d), hs_bnb_shifted(r1, wx, wpr, 0), hs_bnb_shifted(r1, wx, wpr, d));
}

// the value of frame cell (xx, yy) of one pooled map; a cell outside the frame is 0
__host__ __device__ static inline int hs_bnb_cell(const uint32_t *map, int wpr, int rows, int xx, int yy)
{
    const bool in = (unsigned)xx < (unsigned)(wpr * 16) && (unsigned)yy < (unsigned)rows;
    const uint32_t word = map[in ? (size_t)yy * wpr + (size_t)(xx >> 4) : (size_t)0];
    return hs_lat_class_value(in ? (word >> ((xx & 15) * 2)) & 3u : 0u);
}

// rule 3: blocks.  (a, b) <= 8192 each, one 32-bit word; the blocks of the top grid per lattice row or column
__host__ __device__ static inline uint32_t hs_bnb_pack(int a, int b) { return (uint32_t)a | ((uint32_t)b << 16); }
__host__ __device__ static inline int hs_bnb_a(uint32_t p) { return (int)(p & 0xFFFFu); }
__host__ __device__ static inline int hs_bnb_b(uint32_t p) { return (int)(p >> 16); }
__host__ __device__ static inline int hs_bnb_grid(int n, int top) { return (2 * n + (1 << top)) >> top; }   // ceil((2 n + 1) / 2^top)
__host__ __device__ static inline int hs_bnb_key_score(unsigned long long key) { return (int)((uint32_t)(key >> 32) ^ 0x80000000u); }
// rule 4: survival, and how many of a survivor's four children have their origin in the lattice
__host__ __device__ static inline bool hs_bnb_survives(int h, int U, int best) { return h > 0 && U >= best; }
__host__ __device__ static inline int hs_bnb_children(int a, int b, int h, int nx, int ny)
{
    const int d = 1 << (h - 1);
    return (1 + (a + d <= 2 * nx ? 1 : 0)) * (1 + (b + d <= 2 * ny ? 1 : 0));
}
