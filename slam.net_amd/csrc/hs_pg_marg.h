// hs_pg_marg.h -- what host and device share of the pose graph's marginal covariances (K27, hs_pg_marg.inc) beyond hs_pg.h and
// hs_pg_tri.h: rule 5 for a GROUP of right-hand sides -- an incident edge's record and both Jacobians are loaded and formed once and
// used for every right-hand side of the group --, the limits, the spec's check and rule M5's size of one right-hand side.  The kernel
// k27_apply<G> and the test hook slamhip_debug_pg_marginals (with G = 1) run this text.  Definition: include/slamhip.h,
// slamhip_hs_pg_marginals, rules M1 - M5.  Binary64 + - * / only, one rounding per operation, parenthesised as rule 5 writes it: a
// right-hand side's q equals hs_pg_node_apply's under ==, whatever the group.
#pragma once
#include "hs_pg_tri.h"
#include <algorithm>

#define HS_MARG_MAX_PAIRS (1 << 20)        // P
#define HS_MARG_MAX_COLS 4096              // C
#define HS_MARG_GROUP 1                    // G: the right-hand sides a lane of k27_apply / _step / _dir keeps in registers (the default: DESIGN.md section 4 "K27")
#define HS_MARG_GROUP_WIDE 4               // ... and the other instantiated value, which SLAMHIP_K27_GROUP selects
#define HS_MARG_DEFAULT_BYTES ((int64_t)256 << 20)

// rule 5: t_e = W (A p_i + B p_j), A and B given (hs_pg_edge_t forms them itself: the same operations)
__host__ __device__ static inline void hs_marg_edge_t(const double A[3][3], const double B[3][3], const hs_pg_rec &R, const double pi[3], const double pj[3], double t[3])
{
    const double w[3] = { R.wx, R.wy, R.wt };
    for (int k = 0; k < 3; k++) {
        const double a = (A[k][0] * pi[0] + A[k][1] * pi[1]) + A[k][2] * pi[2];
        const double b = (B[k][0] * pj[0] + B[k][1] * pj[1]) + B[k][2] * pj[2];
        t[k] = w[k] * (a + b);
    }
}

// rule 5 for one free node and G right-hand sides: right-hand side g's p is p + g * stride, its q is q[g]; act[g] false: that one is
// skipped and its q is not written.  (In a kernel act is the same in every lane of the workgroup.)
template <int G>
__host__ __device__ static __forceinline__ void hs_marg_node_apply(double lambda, const double *p, size_t stride, const bool act[G], int n, const int32_t *off,
                                                                   const int32_t *inc, const hs_pg_rec *rec, const int32_t *ij, double q[G][3])
{
    double pn[G][3];
    for (int g = 0; g < G; g++) {
        if (!act[g]) continue;
        const double *pg = p + (size_t)g * stride + 3 * (size_t)n;
        for (int a = 0; a < 3; a++) { pn[g][a] = pg[a]; q[g][a] = lambda * pn[g][a]; }
    }
    const int m1 = off[n + 1];
    for (int m = off[n]; m < m1; m++) {
        const int e = inc[m] >> 1, side = inc[m] & 1;
        const hs_pg_rec R = rec[e];
        const int i = ij[2 * (size_t)e], j = ij[2 * (size_t)e + 1];
        const size_t o = (size_t)(side ? i : j);                           // the edge's other end
        double A[3][3], B[3][3];
        hs_pg_jac(R, 0, A);
        hs_pg_jac(R, 1, B);
        for (int g = 0; g < G; g++) {
            if (!act[g]) continue;
            const double *pg = p + (size_t)g * stride + 3 * o;
            const double po[3] = { pg[0], pg[1], pg[2] };
            double t[3];
            if (side) { hs_marg_edge_t(A, B, R, po, pn[g], t); hs_pg_add_jtv(B, t, q[g]); }
            else { hs_marg_edge_t(A, B, R, pn[g], po, t); hs_pg_add_jtv(A, t, q[g]); }
        }
    }
}

// what slamhip_hs_pg_marginals refuses of its spec
static inline bool hs_marg_spec_ok(const slamhip_pg_marg_spec *sp)
{
    return sp->n_cg >= 1 && sp->n_cg <= HS_PG_MAX_CG && sp->check_every >= 1 && (sp->precond == 0 || sp->precond == 1) && sp->reserved == 0 &&
           isfinite(sp->lambda) && sp->lambda >= 0.0 && isfinite(sp->tol) && sp->tol >= 0.0 && sp->max_bytes >= 0;
}

// rule M5: the bytes of one right-hand side in the work block -- five node vectors (x, res, z, p, q), two rows of block sums, the
// scalars and the stop word; with precond = 1 the right-hand sides of the cyclic reduction's levels above level 0
static inline int64_t hs_marg_rhs_bytes(int N, int precond)
{
    const int64_t n = N, pn = (n + HS_PG_BLOCK - 1) / HS_PG_BLOCK;
    hs_tri_plan T;
    const int64_t tot = hs_tri_levels(N, HS_TRI_TAIL, &T);
    return 120 * n + 16 * pn + 40 + (precond ? 24 * (tot - n) + 24 : 0);
}

// rule M5: R_c, and the chunks
static inline int64_t hs_marg_chunk(int64_t R, int N, const slamhip_pg_marg_spec *sp)
{
    const int64_t budget = sp->max_bytes ? sp->max_bytes : HS_MARG_DEFAULT_BYTES;
    return std::min<int64_t>(R, budget / hs_marg_rhs_bytes(N, sp->precond));
}
