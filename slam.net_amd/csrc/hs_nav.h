// hs_nav.h -- the arithmetic of the cost-to-go field (K11, hs_nav.hip) that host and device share: the kernels k11_* and the test
// hook slamhip_debug_nav_field run this text.  Definition: include/slamhip.h, slamhip_hs_nav_field.
// A TRAVERSABLE WORD holds the traversable bits of 32 consecutive cells of one row of the class map M (bit b: cell 32 j + b), as
// K10's frontier words do; a row is ceil(w / 32) words, the padding bits of its last word always clear.  Everything is integer.
#pragma once
#include "hs_dfield.h"

#define HS_NAV_UNREACHED 0xFFFFFFFFu       // SLAMHIP_NAV_UNREACHED
#define HS_NAV_DIR_SOURCE 8
#define HS_NAV_DIR_NONE 255
#define HS_NAV_MAX_CLEARANCE (HS_DF_MAX_RADIUS - 1)   // the field is built with radius c + 1
#define HS_NAV_MAX_SOURCES 4096
#define HS_NAV_MAX_GOALS 4096
#define HS_NAV_MAX_PATHS 64
#define HS_NAV_MAX_PATH_CELLS 65536
#define HS_NAV_MAX_PATH_TOTAL ((int64_t)1 << 20)   // n_paths * max_path_cells: 8 MB of staging
#define HS_NAV_MAX_M ((int64_t)1 << 25)    // cells of M: 4 + 1 bytes per cell and a bit, 164 MB
#define HS_NAV_MAX_RECT ((int64_t)1 << 24) // cells of the caller's rectangle: 4 + 1 bytes each of staging
// The largest cost a cell can have is 7 * (2^25 - 1) < 2^28: cost + weight never wraps, and a neighbour that holds
// HS_NAV_UNREACHED is told apart by hs_nav_via.

// the direction table of step 3: d = 0 .. 7 counter-clockwise from (+1, 0) with y growing downwards in the array
__host__ __device__ static inline int hs_nav_dx(int d) { return (int)((0x901Au >> (2 * d)) & 3u) - 1; }   // +1 +1 0 -1 -1 -1 0 +1
__host__ __device__ static inline int hs_nav_dy(int d) { return (int)((0x01A9u >> (2 * d)) & 3u) - 1; }   // 0 +1 +1 +1 0 -1 -1 -1
__host__ __device__ static inline uint32_t hs_nav_weight(int d) { return 5u + 2u * (uint32_t)(d & 1); }    // the 5-7 chamfer metric

// The traversable bits of the cells [mx32, mx32 + 32) of row y of M, mx32 a multiple of 32 in [0, w): free cells (class 2) whose
// field value exceeds c2 = clearance^2.  row: the row's packed class words.  f: nullptr (clearance 0: no field), or K9's field
// with radius clearance + 1 AT cell (mx32, y) -- f[b] is F of cell mx32 + b; only cells of M are read (a free bit lies below w).
__host__ __device__ static inline uint32_t hs_nav_trav_word(const uint32_t *row, int w, int mx32, const uint16_t *f, uint32_t c2)
{
    uint32_t t = hs_df_site_word(row, w, mx32, 4);                         // (padding cells are never free)
    if (!f) return t;
    for (uint32_t s = t; s; s &= s - 1) {
        const int b = hs_df_ctz(s);
        if ((uint32_t)f[b] <= c2) t &= ~(1u << b);
    }
    return t;
}

// bit x of a row of nw traversable words; clear outside the row, and for a row outside M (nullptr)
__host__ __device__ static inline uint32_t hs_nav_bit(const uint32_t *bits, int nw, int x)
{
    return (bits && x >= 0 && x < 32 * nw) ? (bits[x >> 5] >> (x & 31)) & 1u : 0u;
}
// the traversable bits of cells x - 1, x, x + 1 of one row as bits 0, 1, 2
__host__ __device__ static inline uint32_t hs_nav_bits3(const uint32_t *bits, int nw, int x)
{
    return hs_nav_bit(bits, nw, x - 1) | (hs_nav_bit(bits, nw, x) << 1) | (hs_nav_bit(bits, nw, x + 1) << 2);
}

// The moves allowed from a cell: bit d set iff the move in direction d is allowed.  up / self / down: hs_nav_bits3 of rows y - 1,
// y, y + 1 around the cell.  A straight move needs both ends traversable; a diagonal one also both cells that share an edge with
// both ends (no corner cutting).  The relation is symmetric: move d from a cell is allowed iff move d ^ 4 from its target is.
__host__ __device__ static inline uint32_t hs_nav_moves(uint32_t up, uint32_t self, uint32_t down)
{
    if (!(self & 2u)) return 0u;
    const uint32_t e = (self >> 2) & 1u, w = self & 1u, s = (down >> 1) & 1u, n = (up >> 1) & 1u;
    return e | ((e & s & (down >> 2)) << 1) | (s << 2) | ((w & s & down & 1u) << 3) | (w << 4) | ((w & n & up & 1u) << 5) | (n << 6) |
           ((e & n & (up >> 2)) << 7);
}

// the cost of reaching a cell through its neighbour of cost cn in direction d, HS_NAV_UNREACHED if the neighbour is unreached or
// the sum exceeds max_cost (0: no cap)
__host__ __device__ static inline uint32_t hs_nav_via(uint32_t cn, int d, uint32_t max_cost)
{
    if (cn == HS_NAV_UNREACHED) return HS_NAV_UNREACHED;
    const uint32_t v = cn + hs_nav_weight(d);
    return (max_cost && v > max_cost) ? HS_NAV_UNREACHED : v;
}

// The dir rule of step 5 for a cell of cost c: 8 at a source (the only cells of cost 0), 255 where unreached, else the smallest
// allowed d whose neighbour's cost + weight equals c.  cn[d]: the cost of the neighbour in direction d (read only where the move
// is allowed).  255 for a reached cell means the costs are no solution of the shortest-path equations.
__host__ __device__ static inline uint32_t hs_nav_dir(uint32_t c, uint32_t moves, const uint32_t cn[8])
{
    if (c == HS_NAV_UNREACHED) return HS_NAV_DIR_NONE;
    if (c == 0u) return HS_NAV_DIR_SOURCE;
    for (int d = 0; d < 8; d++)
        if (((moves >> d) & 1u) && cn[d] != HS_NAV_UNREACHED && cn[d] + hs_nav_weight(d) == c) return (uint32_t)d;
    return HS_NAV_DIR_NONE;
}
