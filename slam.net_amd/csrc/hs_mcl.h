// hs_mcl.h -- the arithmetic of the particle-filter localisation step (K13, hs_mcl.hip) that host and device share: the kernels
// k13_score, k13_weigh and k13_resample and the test hook slamhip_debug_mcl_step run this text.  Definition: include/slamhip.h,
// slamhip_hs_mcl_step.  Every binary32 operation is rounded on its own (the build uses -ffp-contract=off: no fused multiply-add);
// everything else is integer arithmetic.  The end cells are hs_trace.h's, the field is hs_dfield.h's.
#pragma once
#include "det_trig.h"
#include "hs_dfield.h"
#include "hs_trace.h"
#include "philox.h"

#define HS_MCL_MAX_N 65536                 // particles: N * W < 2^64 with W < N * 2^32
#define HS_MCL_MAX_POINTS 7680             // scan points: 8 bytes each in LDS, 60 KB of the 64 KB a workgroup may allocate
// step 1: the binary32 nearest to sqrt(3 / (2^32 - 1)).  A sum of four 16-bit halves has variance 4 * (2^32 - 1) / 12, so z is a
// four-term Irwin-Hall variate with mean 0 and variance 1; its tails end at 131070 * ZS = 3.46 sigma.  (Not Box-Muller: logf is
// not bit-reproducible between host and device.)
#define HS_MCL_ZS 0x1.bb67aep-16f

// step 5: T[f] = min(2^32 - 1, floor(2^((2048 - f) / 64))), the integer 64th root of 2^(2048 - f)
__host__ __device__ static inline uint32_t hs_mcl_table(int f)
{
    const uint32_t T[64] = {
        0xFFFFFFFFu, 0xFD3E0C0Cu, 0xFA83B2DBu, 0xF7D0DF73u, 0xF5257D15u, 0xF281773Cu, 0xEFE4B99Bu, 0xED4F301Eu,
        0xEAC0C6E7u, 0xE8396A50u, 0xE5B906E7u, 0xE33F8972u, 0xE0CCDEECu, 0xDE60F482u, 0xDBFBB797u, 0xD99D15C2u,
        0xD744FCCAu, 0xD4F35AABu, 0xD2A81D91u, 0xD06333DAu, 0xCE248C15u, 0xCBEC14FEu, 0xC9B9BD86u, 0xC78D74C8u,
        0xC5672A11u, 0xC346CCDAu, 0xC12C4CCAu, 0xBF1799B6u, 0xBD08A39Fu, 0xBAFF5AB2u, 0xB8FBAF47u, 0xB6FD91E3u,
        0xB504F333u, 0xB311C412u, 0xB123F581u, 0xAF3B78ADu, 0xAD583EEAu, 0xAB7A39B5u, 0xA9A15AB4u, 0xA7CD93B4u,
        0xA5FED6A9u, 0xA43515AEu, 0xA2704303u, 0xA0B0510Fu, 0x9EF53260u, 0x9D3ED9A7u, 0x9B8D39B9u, 0x99E04593u,
        0x9837F051u, 0x96942D37u, 0x94F4EFA8u, 0x935A2B2Fu, 0x91C3D373u, 0x9031DC43u, 0x8EA4398Bu, 0x8D1ADF5Bu,
        0x8B95C1E3u, 0x8A14D575u, 0x88980E80u, 0x871F6196u, 0x85AAC367u, 0x843A28C3u, 0x82CD8698u, 0x8164D1F3u,
    };
    return T[f & 63];
}

struct hs_mcl_pose { float x, y, th; };
// the floats and the generator's words of a slamhip_mcl_spec, by value
struct hs_mcl_motion { float dx, dy, dth, sx, sy, sth, fox, foy; uint32_t key0, key1, str0, str1; };
// step 1: the three variates of particle i
__host__ __device__ static inline void hs_mcl_noise(const hs_mcl_motion &m, int i, float z[3])
{
    uint32_t b[8];
    for (int j = 0; j < 2; j++) {
        uint32_t c[4] = { (uint32_t)i, (uint32_t)j, m.str0, m.str1 };
        philox4x32_10(c, m.key0, m.key1);
        for (int k = 0; k < 4; k++) b[4 * j + k] = c[k];
    }
    for (int q = 0; q < 3; q++) {                                          // halves 4 q .. 4 q + 3: words 2 q and 2 q + 1
        const int sum = (int)(b[2 * q] & 0xFFFFu) + (int)(b[2 * q] >> 16) + (int)(b[2 * q + 1] & 0xFFFFu) + (int)(b[2 * q + 1] >> 16);
        z[q] = (float)(sum - 131070) * HS_MCL_ZS;                          // (|sum - 131070| < 2^17: the conversion is exact)
    }
}

// step 2
__host__ __device__ static inline hs_mcl_pose hs_mcl_predict(const hs_mcl_motion &m, const hs_mcl_pose &p, const float z[3])
{
    const float nx = m.sx * z[0], ny = m.sy * z[1], nth = m.sth * z[2];
    const float ex = m.dx + nx, ey = m.dy + ny, eth = m.dth + nth;
    float s, c;
    sh_det_sincosf(p.th, &s, &c);
    const float cx = c * ex, sy = s * ey, sx = s * ex, cy = c * ey;
    hs_mcl_pose q;
    q.x = (p.x + m.fox) + (cx - sy);
    q.y = (p.y + m.foy) + (sx + cy);
    q.th = p.th + eth;
    return q;
}

// step 3 for one scan point under t = hs_trace_transform(stm, x', y', theta'): F of its end cell; false: the point is ignored
__host__ __device__ static inline bool hs_mcl_point(const hs_field &E, const sh_m3x2 &t, float px, float py, uint32_t *F)
{
    int ex, ey;
    if (!hs_trace_end_cell(t, px, py, &ex, &ey)) return false;
    *F = hs_field_lookup(E, (long long)ex, (long long)ey);
    return true;
}

// step 5
__host__ __device__ static inline uint32_t hs_mcl_weight(unsigned long long accp, uint32_t beta)
{
    const unsigned long long d = accp < 0xFFFFFFFFull ? accp : 0xFFFFFFFFull;
    const unsigned long long e = (d * (unsigned long long)beta) >> 16;     // (below 2^64 / 2^16)
    const unsigned long long k = e >> 6;
    return k >= 32 ? 0u : hs_mcl_table((int)(e & 63)) >> (int)k;
}

// step 6: the scaled integers of a predicted pose; false: the particle is counted in n_unplaced
__host__ __device__ static inline bool hs_mcl_moments(const hs_mcl_pose &q, long long *ix, long long *iy, int *ic, int *is)
{
    const float fx = q.x * 1024.0f, fy = q.y * 1024.0f;
    float s, c;
    sh_det_sincosf(q.th, &s, &c);
    if (!(fabsf(fx) < 2147483648.0f && fabsf(fy) < 2147483648.0f && isfinite(c) && isfinite(s))) return false;
    *ix = (long long)rintf(fx); *iy = (long long)rintf(fy);
    *ic = (int)rintf(c * 16384.0f); *is = (int)rintf(s * 16384.0f);
    return true;
}

// step 7: resample?
__host__ __device__ static inline bool hs_mcl_decide(unsigned long long A, unsigned long long Q, int n_eff_min)
{
    return A * A < (unsigned long long)n_eff_min * Q;                      // (A < 2^28, Q < 2^40, n_eff_min <= 2^16 + 1)
}

// step 7: the offset u of the systematic comb
__host__ __device__ static inline unsigned long long hs_mcl_comb_offset(const hs_mcl_motion &m, unsigned long long W)
{
    uint32_t c[4] = { 0u, 2u, m.str0, m.str1 };
    philox4x32_10(c, m.key0, m.key1);
    return ((W >> 16) * (unsigned long long)c[0]) >> 16;                   // (W < 2^48: the product stays below 2^64; u < W)
}

// step 7: the least i in [0, N) with N * C[i] > T; C is non-decreasing and N * C[N - 1] = N * W > T for every tooth of the comb
__host__ __device__ static inline int hs_mcl_ancestor(const unsigned long long *C, int N, unsigned long long T)
{
    int lo = 0, hi = N - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((unsigned long long)N * C[mid] > T) hi = mid; else lo = mid + 1;
    }
    return lo;
}
