// hs_sig.h -- the arithmetic of the scan signatures and their matches (K18, hs_sig.hip) that host and device share: the kernels k18_sig,
// k18_query, k18_query_finish, k18_self and k18_self_finish and the test hooks slamhip_debug_sig_table / _sig / _sig_ring / _sig_sector /
// _sig_search run this text.  Definition: include/slamhip.h, slamhip_hs_sig_add.  Everything here is integer arithmetic except the two
// multiplies of rule 2, each rounded on its own, and the table, which the HOST forms in binary64 and hands to every launch.
#pragma once
#include "common.h"

#define HS_SG_SECTORS 64                   // SLAMHIP_SIG_SECTORS: a ring is one 64-bit word
#define HS_SG_MAX_RING 32                  // n_ring
#define HS_SG_MAX_REACH 32768              // 2 * ring_cells * n_ring, in doubled cells: its square is 2^30
#define HS_SG_MAX_KEYS (1 << 20)           // keyframes of a store
#define HS_SG_MAX_B 16                     // hits of a query
#define HS_SG_MAX_SCANS 4096               // scans of one slamhip_hs_sig_add_scans
#define HS_SG_MAX_POINTS (1 << 24)         // points of one slamhip_hs_sig_add_scans
#define HS_SG_ONE 16384                    // the table's scale, 2^14
#define HS_SG_BLOCK 64                     // keyframes of a block of the store

// the packed key of the self search's 64-bit atomic max, low bits first: the shift, then SLAMHIP_SIG_MAX_KEYS - 1 - index (a lower
// index is a larger key), then the score, then a bit every key of a real pair has (an empty slot is 0)
#define HS_SG_PK_SHIFT_BITS 6              // shift in [0, 64)
#define HS_SG_PK_INDEX_BITS 20             // index in [0, 2^20)
#define HS_SG_PK_SCORE_BITS 17             // score in [0, 65536]
#define HS_SG_PK_VALID_BIT (HS_SG_PK_SHIFT_BITS + HS_SG_PK_INDEX_BITS + HS_SG_PK_SCORE_BITS)

#include <math.h>
// rule 1: cs[0 .. 64) = C, cs[64 .. 128) = S.  A host function: the device never forms a sine.
static inline void hs_sig_table(int32_t *cs)
{
    int32_t *C = cs, *S = cs + HS_SG_SECTORS;
    for (int k = 0; k < 16; k++) {
        const double a = ((double)k * M_PI) / 32.0;
        C[k] = (int32_t)rint(16384.0 * cos(a));
        S[k] = (int32_t)rint(16384.0 * sin(a));
    }
    for (int k = 16; k < HS_SG_SECTORS; k++) { C[k] = -S[k - 16]; S[k] = C[k - 16]; }
}

// what slamhip_hs_sig_configure refuses
__host__ __device__ static inline bool hs_sig_spec_ok(float scale, int n_ring, int ring_cells)
{
    if (!(scale > 0.0f) || !(scale <= 3.402823466e38f)) return false;      // (NaN fails the first test, +inf the second)
    if (n_ring < 1 || n_ring > HS_SG_MAX_RING || ring_cells < 1) return false;
    return (long long)2 * ring_cells * n_ring <= HS_SG_MAX_REACH;
}

// rule 2: the odd doubled coordinates of the point's cell; false: the point is IGNORED
__host__ __device__ static inline bool hs_sig_cell(float px, float py, float scale, int *u, int *v)
{
#pragma clang fp contract(off)
    const float fx = px * scale;
    const float fy = py * scale;
    if (!(fabsf(fx) < 16384.0f) || !(fabsf(fy) < 16384.0f)) return false;  // (a NaN fails either test)
    *u = 2 * (int)floorf(fx) + 1;
    *v = 2 * (int)floorf(fy) + 1;
    return true;
}

// rule 3 by a square root and an integer fix-up: whatever the root's last bits are, the two loops leave the count of the definition
__host__ __device__ static inline int hs_sig_ring(int d2, int n_ring, int ring_cells)
{
    const int step = 2 * ring_cells;
    int j = (int)(sqrtf((float)d2)) / step;
    if (j > n_ring) j = n_ring;
    while (j < n_ring && (step * (j + 1)) * (step * (j + 1)) <= d2) j++;   // (step * j <= 32768: the square is at most 2^30)
    while (j > 0 && (step * j) * (step * j) > d2) j--;
    return j;
}

// rule 4: the quadrant from the signs (u and v are odd, so neither is 0), then four steps over the quadrant's 16 directions with the
// exact cross products.  cs: the table, C then S (the host's array, or the kernel's copy in LDS).
__host__ __device__ static inline int hs_sig_cross(const int32_t *cs, int k, int u, int v) { return cs[k] * v - cs[HS_SG_SECTORS + k] * u; }
__host__ __device__ static inline int hs_sig_sector(const int32_t *cs, int u, int v)
{
    int k = v > 0 ? (u > 0 ? 0 : 16) : (u < 0 ? 32 : 48);
    for (int step = 8; step > 0; step >>= 1)
        if (hs_sig_cross(cs, k + step, u, v) >= 0) k += step;
    return k;
}

__host__ __device__ static inline unsigned long long hs_sig_rotl(unsigned long long w, int s) { return s ? (w << s) | (w >> (64 - s)) : w; }
__host__ __device__ static inline unsigned long long hs_sig_rotr(unsigned long long w, int s) { return s ? (w >> s) | (w << (64 - s)) : w; }
__host__ __device__ static inline int hs_sig_popc(unsigned long long w)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __popcll(w);
#else
    return __builtin_popcountll(w);
#endif
}

// rule 6: the score of a pair from its best inter and the two popcounts
__host__ __device__ static inline uint32_t hs_sig_score(int inter, int nq, int nk)
{
    const int uni = nq + nk - inter;
    return uni ? ((uint32_t)inter << 16) / (uint32_t)uni : 0u;
}
// rule 7's order as one word: a higher score first, then a lower index.  Never 0 for an index below 2^31.
__host__ __device__ static inline unsigned long long hs_sig_rank(uint32_t score, int index)
{
    return ((unsigned long long)score << 32) | (unsigned long long)(~(uint32_t)index);
}
// rule 8's packed key and its fields back
__host__ __device__ static inline unsigned long long hs_sig_pack(uint32_t score, int index, int shift)
{
    return (1ull << HS_SG_PK_VALID_BIT) | ((unsigned long long)score << (HS_SG_PK_SHIFT_BITS + HS_SG_PK_INDEX_BITS))
         | ((unsigned long long)(uint32_t)(HS_SG_MAX_KEYS - 1 - index) << HS_SG_PK_SHIFT_BITS) | (unsigned long long)(uint32_t)shift;
}
__host__ __device__ static inline void hs_sig_unpack(unsigned long long key, uint32_t *score, int *index, int *shift)
{
    *shift = (int)(key & ((1u << HS_SG_PK_SHIFT_BITS) - 1u));
    *index = HS_SG_MAX_KEYS - 1 - (int)((key >> HS_SG_PK_SHIFT_BITS) & ((1u << HS_SG_PK_INDEX_BITS) - 1u));
    *score = (uint32_t)((key >> (HS_SG_PK_SHIFT_BITS + HS_SG_PK_INDEX_BITS)) & ((1u << HS_SG_PK_SCORE_BITS) - 1u));
}

// where ring r of keyframe i lies in the store: blocks of 64 keyframes, ring r of a block's 64 keyframes contiguous
__host__ __device__ static inline size_t hs_sig_at(int i, int r, int n_ring)
{
    return ((size_t)(i >> 6) * (size_t)n_ring + (size_t)r) * HS_SG_BLOCK + (size_t)(i & 63);
}

// a hit from the pair's best inter and shift
__host__ __device__ static inline slamhip_sig_hit hs_sig_make_hit(int index, int shift, int inter, int nq, int nk)
{
    slamhip_sig_hit h;
    h.score = hs_sig_score(inter, nq, nk);
    h.index = index;
    h.shift = (int16_t)shift; h.inter = (int16_t)inter; h.uni = (int16_t)(nq + nk - inter); h.n_set_key = (int16_t)nk;
    return h;
}
__host__ __device__ static inline slamhip_sig_hit hs_sig_no_hit()
{
    slamhip_sig_hit h;
    h.score = 0u; h.index = -1; h.shift = 0; h.inter = 0; h.uni = 0; h.n_set_key = 0;
    return h;
}
