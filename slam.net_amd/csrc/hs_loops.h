// hs_loops.h -- the arithmetic of the consistent set of loop edges (K23, hs_loops.hip) that host and device share: the kernels
// k23_edges, k23_pairs, k23_degree, k23_clique and k23_finish and the test hook slamhip_debug_loops_consistent run this text.
// Definition: include/slamhip.h, slamhip_hs_loops_consistent.  The floating-point part is binary64 + - * / and rint, one rounding per
// operation (the build has -ffp-contract=off), every expression parenthesised as the definition writes it; behind the one comparison
// d2 <= gamma everything is an integer.
#pragma once
#include "common.h"
#include "det_trig.h"
#include "hs_pg.h"

#define HS_LP_MAX_EDGES 4096               // L
#define HS_LP_MAX_NODES (1 << 20)          // N
#define HS_LP_MAX_STARTS 64                // n_starts
#define HS_LP_MAX_THETA 32768.0            // |theta| of a pose and of a z: W.theta stays inside sh_det_sincos's contract
#define HS_LP_MAX_WORDS (HS_LP_MAX_EDGES / 64)
// k23_clique keeps the matrix in LDS where its rows, padded to an odd number of words, take at most this many bytes
#define HS_LP_LDS_ADJ_BYTES (144 * 1024)

typedef unsigned long long hs_lp_u64;

// an edge as it goes to the device: the two poses it joins, gathered on the host
struct hs_lp_in { double pi[3], pj[3], z[3], w[3]; int32_t i, j, use, pad; };
// rule 1's record, and what rule 2 needs of node j
struct hs_lp_rec { double Wx, Wy, Wt, sW, cW, sJ, cJ, vt, vth, jx, jy, jt; int32_t i, j, use, pad; };

__host__ __device__ static inline int hs_lp_words(int L) { return (L + 63) >> 6; }
__host__ __device__ static inline int hs_lp_stride(int L) { return hs_lp_words(L) | 1; }          // a row of the LDS copy: odd, so that lanes on consecutive rows meet different banks
__host__ __device__ static inline bool hs_lp_resident(int L) { return (size_t)L * hs_lp_stride(L) * 8 <= HS_LP_LDS_ADJ_BYTES; }

// rule 1
__host__ __device__ static inline void hs_lp_edge(const hs_lp_in &E, hs_lp_rec *R)
{
    double sI, cI;
    sh_det_sincos(E.pi[2], &sI, &cI);
    R->Wx = E.pi[0] + (cI * E.z[0] - sI * E.z[1]);
    R->Wy = E.pi[1] + (sI * E.z[0] + cI * E.z[1]);
    R->Wt = E.pi[2] + E.z[2];
    sh_det_sincos(R->Wt, &R->sW, &R->cW);
    sh_det_sincos(E.pj[2], &R->sJ, &R->cJ);
    R->vt = 0.5 * (1.0 / E.w[0] + 1.0 / E.w[1]);
    R->vth = 1.0 / E.w[2];
    R->jx = E.pj[0]; R->jy = E.pj[1]; R->jt = E.pj[2];
    R->i = E.i; R->j = E.j; R->use = E.use != 0; R->pad = 0;
}

// rule 2's d2 for the pair (a, b), a the edge of the lower index
__host__ __device__ static inline double hs_lp_d2(const hs_lp_rec &A, const hs_lp_rec &B, double q_t, double q_theta)
{
    const double dx = B.jx - A.jx, dy = B.jy - A.jy;
    const double ux = A.cJ * dx + A.sJ * dy;
    const double uy = A.cJ * dy - A.sJ * dx;
    const double ut = B.jt - A.jt;
    const double Tx = A.Wx + (A.cW * ux - A.sW * uy);
    const double Ty = A.Wy + (A.sW * ux + A.cW * uy);
    const double Tt = A.Wt + ut;
    const double ex = Tx - B.Wx;
    const double ey = Ty - B.Wy;
    const double et = hs_pg_wrap(Tt - B.Wt);
    const int dj = A.j > B.j ? A.j - B.j : B.j - A.j, di = A.i > B.i ? A.i - B.i : B.i - A.i;
    const double s = (double)(dj + di);
    const double rho2 = ux * ux + uy * uy;
    const double Vt = ((A.vt + B.vt) + s * q_t) + A.vth * rho2;
    const double Vth = (A.vth + B.vth) + s * q_theta;
    return (ex * ex + ey * ey) / Vt + (et * et) / Vth;
}

// rule 2's bit of row `row`, column `col` from the two records (row != col is the caller's)
__host__ __device__ static inline bool hs_lp_bit(const hs_lp_rec &Rrow, int row, const hs_lp_rec &Rcol, int col, double q_t, double q_theta, double gamma)
{
    if (!(Rrow.use && Rcol.use)) return false;
    const double d2 = row < col ? hs_lp_d2(Rrow, Rcol, q_t, q_theta) : hs_lp_d2(Rcol, Rrow, q_t, q_theta);
    return d2 <= gamma;                                                    // (a NaN fails)
}

// rules 4 and 5: the packed key of a candidate -- the higher count first, then the lower index.  Never 0.
__host__ __device__ static inline hs_lp_u64 hs_lp_key(int g, int v) { return ((hs_lp_u64)(uint32_t)g << 32) | (hs_lp_u64)(0xFFFFFFFFu - (uint32_t)v); }
__host__ __device__ static inline int hs_lp_key_index(hs_lp_u64 key) { return (int)(0xFFFFFFFFu - (uint32_t)key); }

__host__ __device__ static inline int hs_lp_popc(hs_lp_u64 x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __popcll(x);
#else
    return __builtin_popcountll(x);
#endif
}

// what slamhip_hs_loops_consistent refuses of its spec
static inline bool hs_lp_spec_ok(const slamhip_loops_spec *sp)
{
    return isfinite(sp->gamma) && sp->gamma >= 0.0 && isfinite(sp->q_t) && sp->q_t >= 0.0 && isfinite(sp->q_theta) && sp->q_theta >= 0.0 &&
           sp->n_starts >= 1 && sp->n_starts <= HS_LP_MAX_STARTS && sp->min_clique >= 1 && (sp->flags & ~SLAMHIP_LOOPS_ADJ) == 0 && sp->reserved == 0;
}
