// hs_frontier.h -- the arithmetic of the frontier cells and their runs (K10, hs_frontier.hip) that host and device share: the
// kernels k10_* and the test hook slamhip_debug_frontiers run this text.  Definition: include/slamhip.h, slamhip_hs_frontiers.
// A FRONTIER WORD holds the frontier bits of 32 consecutive cells of one row of the class map M (bit b: cell 32 j + b); a row is
// ceil(w / 32) words, the padding bits of its last word always clear.  Everything here works by word with ctz / clz, never cell by
// cell, and every loop ends at the row's ends.
#pragma once
#include "hs_dfield.h"

#define HS_FR_MAX_CLUSTERS 65536           // SLAMHIP_FRONTIER_MAX_CLUSTERS: slots of the record block
#define HS_FR_MAX_M ((int64_t)1 << 25)     // cells of M: two int32 per cell, 256 MB
#define HS_FR_MAX_RECT ((int64_t)1 << 24)  // cells of a label rectangle: 64 MB of staging
#define HS_FR_DROPPED (-1)                 // parent of a root whose cluster is not kept; a kept root holds -2 - slot

// The frontier bits of the cells [mx32, mx32 + 32) of one row, mx32 a multiple of 32 in [0, w): free cells (class 2) with an
// unknown (class 0) cell left, right, above or below.  up / self / down: the packed class words of the three rows, nullptr for a
// row outside M.  A row outside M, a word outside M and a row's padding are all unknown: hs_df_site_word with mask 1 says so.
__host__ __device__ static inline uint32_t hs_fr_word(const uint32_t *up, const uint32_t *self, const uint32_t *down, int w, int mx32)
{
    const uint32_t f = hs_df_site_word(self, w, mx32, 4);                  // (padding cells are never free)
    if (!f) return 0u;
    const uint32_t u = hs_df_site_word(self, w, mx32, 1);
    const uint32_t ul = hs_df_site_word(self, w, mx32 - 32, 1), ur = hs_df_site_word(self, w, mx32 + 32, 1);
    const uint32_t beside = (u << 1) | (ul >> 31) | (u >> 1) | (ur << 31);
    return f & (beside | hs_df_site_word(up, w, mx32, 1) | hs_df_site_word(down, w, mx32, 1));
}

// the bits of `cur` at which a run begins; prev: the word to its left (0 for the row's first word)
__host__ __device__ static inline uint32_t hs_fr_starts(uint32_t cur, uint32_t prev) { return cur & ~((cur << 1) | (prev >> 31)); }

// The first cell of the run that the set bit p lies in; it may be several words to the left.
__host__ __device__ static inline int hs_fr_run_start(const uint32_t *bits, int p)
{
    const int wi = p >> 5, b = p & 31;
    const uint32_t inv = ~(bits[wi] << (31 - b));                          // bit 31: the cell itself; zero bits from there down: set cells
    const int n = inv ? hs_df_clz(inv) : 32;                               // set cells from p downwards in this word, at most b + 1
    if (n <= b) return p - n + 1;
    int k = wi - 1;
    while (k >= 0 && bits[k] == 0xFFFFFFFFu) k--;                          // (ends at the row's first word)
    return k < 0 ? 0 : 32 * (k + 1) - hs_df_clz(~bits[k]);
}

// The last cell of the run that the set bit p lies in; nw: words of the row (the padding of the last one is clear).
__host__ __device__ static inline int hs_fr_run_end(const uint32_t *bits, int nw, int p)
{
    const int wi = p >> 5, b = p & 31;
    const uint32_t inv = ~(bits[wi] >> b);
    const int n = inv ? hs_df_ctz(inv) : 32;                               // set cells from p upwards in this word, at most 32 - b
    if (n < 32 - b) return p + n - 1;
    int k = wi + 1;
    while (k < nw && bits[k] == 0xFFFFFFFFu) k++;                          // (ends at the row's last word)
    return k == nw ? 32 * nw - 1 : 32 * k + hs_df_ctz(~bits[k]) - 1;
}

// The first set bit at or after p, or 32 * nw if the row holds none (p >= 0, it may lie past the row).
__host__ __device__ static inline int hs_fr_next_set(const uint32_t *bits, int nw, int p)
{
    int k = p >> 5;
    if (k >= nw) return 32 * nw;
    const uint32_t v = bits[k] & (0xFFFFFFFFu << (p & 31));
    if (v) return 32 * k + hs_df_ctz(v);
    for (k++; k < nw; k++)
        if (bits[k]) return 32 * k + hs_df_ctz(bits[k]);
    return 32 * nw;
}

// the sum of the x of the cells s .. e of one run: len * (s + e) / 2, exact (one of len and s + e is even)
__host__ __device__ static inline long long hs_fr_run_sum(int s, int e) { return ((long long)(e - s + 1) * (long long)(s + e)) / 2; }
