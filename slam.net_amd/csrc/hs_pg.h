// hs_pg.h -- the arithmetic of the pose-graph relaxation (K19, hs_pg.hip) that host and device share: the kernels k19_linearise,
// k19_diag, k19_apply, k19_step, k19_dir and k19_update and the test hooks slamhip_debug_pg_relax / _pg_sum / _sincos run this text,
// down to the loops over a node's list of rules 4 and 5 (hs_pg_node_diag, hs_pg_node_apply: always inlined, so that a kernel's code is
// what it was with the loop written in the kernel).  Definition: include/slamhip.h, slamhip_hs_pg_relax.  Everything here is binary64 + - * / and rint, one rounding per operation (the
// build has -ffp-contract=off); every expression is parenthesised as the definition writes it.
#pragma once
#include "common.h"
#include "det_trig.h"
#include <math.h>

#define HS_PG_MAX_NODES (1 << 20)          // N
#define HS_PG_MAX_EDGES (1 << 22)          // E
#define HS_PG_MAX_OUTER 64                 // n_outer
#define HS_PG_MAX_CG (1 << 20)             // n_cg
#define HS_PG_BLOCK 256                    // rule 6: the block of the one reduction shape
#define HS_PG_TWO_PI 6.283185307179586     // the binary64 nearest 2 pi, 0x401921FB54442D18
// slamhip_pg_iter.stopped, and the device's stop word = 1 + stopped (0: running)
#define HS_PG_STOP_TOL 0
#define HS_PG_STOP_NCG 1
#define HS_PG_STOP_BREAKDOWN 2

// what an edge keeps of rule 3 for an outer iteration: (s, c) of theta_i, u, the weights and chi2_e -- A and B are formed from it
struct hs_pg_rec { double c, s, ux, uy, wx, wy, wt, chi2; };

// rule 2
__host__ __device__ static inline double hs_pg_wrap(double a) { return a - HS_PG_TWO_PI * rint(a / HS_PG_TWO_PI); }

// rule 3: the record and the residual of one edge
__host__ __device__ static inline void hs_pg_edge(const double *pi, const double *pj, const double *z, const double *w, hs_pg_rec *R, double *r)
{
    double s, c;
    sh_det_sincos(pi[2], &s, &c);
    const double dx = pj[0] - pi[0], dy = pj[1] - pi[1];
    const double ux = c * dx + s * dy, uy = c * dy - s * dx;
    r[0] = ux - z[0];
    r[1] = uy - z[1];
    r[2] = hs_pg_wrap((pj[2] - pi[2]) - z[2]);
    R->c = c; R->s = s; R->ux = ux; R->uy = uy;
    R->wx = w[0]; R->wy = w[1]; R->wt = w[2];
    R->chi2 = (w[0] * (r[0] * r[0]) + w[1] * (r[1] * r[1])) + w[2] * (r[2] * r[2]);
}

// rule 3: J[k][a] = d r_k / d (variable a of the node on `side`): A for side 0 (node i), B for side 1 (node j)
__host__ __device__ static inline void hs_pg_jac(const hs_pg_rec &R, int side, double J[3][3])
{
    if (side == 0) {
        J[0][0] = -R.c; J[0][1] = -R.s; J[0][2] = R.uy;
        J[1][0] = R.s;  J[1][1] = -R.c; J[1][2] = -R.ux;
        J[2][0] = 0.0;  J[2][1] = 0.0;  J[2][2] = -1.0;
    } else {
        J[0][0] = R.c;  J[0][1] = R.s;  J[0][2] = 0.0;
        J[1][0] = -R.s; J[1][1] = R.c;  J[1][2] = 0.0;
        J[2][0] = 0.0;  J[2][1] = 0.0;  J[2][2] = 1.0;
    }
}

// a symmetric 3 x 3 as six: (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)
// rule 4: D += J^T W J, entry (a, b) with a <= b
__host__ __device__ static inline void hs_pg_add_jtwj(const double J[3][3], const hs_pg_rec &R, double D[6])
{
    int m = 0;
    for (int a = 0; a < 3; a++)
        for (int b = a; b < 3; b++, m++)
            D[m] = D[m] + (((J[0][a] * R.wx) * J[0][b] + (J[1][a] * R.wy) * J[1][b]) + (J[2][a] * R.wt) * J[2][b]);
}

// rules 4 and 5: g += J^T v
__host__ __device__ static inline void hs_pg_add_jtv(const double J[3][3], const double v[3], double g[3])
{
    for (int a = 0; a < 3; a++) g[a] = g[a] + ((J[0][a] * v[0] + J[1][a] * v[1]) + J[2][a] * v[2]);
}

// rule 4: M = D^-1 by the adjugate over the determinant; false (M = 0) unless det > 0
__host__ __device__ static inline bool hs_pg_inv(const double D[6], double M[6])
{
    const double d00 = D[0], d01 = D[1], d02 = D[2], d11 = D[3], d12 = D[4], d22 = D[5];
    const double c00 = d11 * d22 - d12 * d12, c01 = d02 * d12 - d01 * d22, c02 = d01 * d12 - d02 * d11;
    const double c11 = d00 * d22 - d02 * d02, c12 = d01 * d02 - d00 * d12, c22 = d00 * d11 - d01 * d01;
    const double det = (d00 * c00 + d01 * c01) + d02 * c02;
    if (!(det > 0.0)) {
        for (int m = 0; m < 6; m++) M[m] = 0.0;
        return false;
    }
    M[0] = c00 / det; M[1] = c01 / det; M[2] = c02 / det; M[3] = c11 / det; M[4] = c12 / det; M[5] = c22 / det;
    return true;
}

// rule 7: z = M res
__host__ __device__ static inline void hs_pg_mul(const double M[6], const double v[3], double out[3])
{
    out[0] = (M[0] * v[0] + M[1] * v[1]) + M[2] * v[2];
    out[1] = (M[1] * v[0] + M[3] * v[1]) + M[4] * v[2];
    out[2] = (M[2] * v[0] + M[4] * v[1]) + M[5] * v[2];
}

// rule 5: t_e = W (A p_i + B p_j)
__host__ __device__ static inline void hs_pg_edge_t(const hs_pg_rec &R, const double pi[3], const double pj[3], double t[3])
{
    double A[3][3], B[3][3];
    hs_pg_jac(R, 0, A);
    hs_pg_jac(R, 1, B);
    const double w[3] = { R.wx, R.wy, R.wt };
    for (int k = 0; k < 3; k++) {
        const double a = (A[k][0] * pi[0] + A[k][1] * pi[1]) + A[k][2] * pi[2];
        const double b = (B[k][0] * pj[0] + B[k][1] * pj[1]) + B[k][2] * pj[2];
        t[k] = w[k] * (a + b);
    }
}

// The per-node loops run over the node -> (edge, side) lists: node n's entries are inc[off[n] .. off[n + 1]), an entry edge << 1 | side;
// rec and r are rule 3's records and residuals per edge, ij the edges' (i, j) pairs, a node vector three doubles per node.
// rule 4 for one free node: D_n = lambda I + sum J^T W J and g_n = sum J^T W r over the node's list
__host__ __device__ static __forceinline__ void hs_pg_node_diag(double lambda, int n, const int32_t *off, const int32_t *inc, const hs_pg_rec *rec, const double *r,
                                                                double D[6], double g[3])
{
    D[0] = lambda; D[1] = 0.0; D[2] = 0.0; D[3] = lambda; D[4] = 0.0; D[5] = lambda;
    g[0] = 0.0; g[1] = 0.0; g[2] = 0.0;
    const int m1 = off[n + 1];
    for (int m = off[n]; m < m1; m++) {
        const int e = inc[m] >> 1, side = inc[m] & 1;
        const hs_pg_rec R = rec[e];
        const double *re = r + 3 * (size_t)e;
        double J[3][3];
        hs_pg_jac(R, side, J);
        hs_pg_add_jtwj(J, R, D);
        const double v[3] = { R.wx * re[0], R.wy * re[1], R.wt * re[2] };
        hs_pg_add_jtv(J, v, g);
    }
}

// rule 5 for one free node: q_n = lambda p_n + sum J^T t_e over the node's list.  t_e is formed again at each end of an edge, from
// (p_i, p_j) in this order at either end: the same bits.  (p_n and the other end's entry are copied before use: a kernel then keeps
// p_n in registers across the loop.)
__host__ __device__ static __forceinline__ void hs_pg_node_apply(double lambda, const double *p, int n, const int32_t *off, const int32_t *inc, const hs_pg_rec *rec,
                                                                 const int32_t *ij, double q[3])
{
    const double pn[3] = { p[3 * (size_t)n], p[3 * (size_t)n + 1], p[3 * (size_t)n + 2] };
    for (int a = 0; a < 3; a++) q[a] = lambda * pn[a];
    const int m1 = off[n + 1];
    for (int m = off[n]; m < m1; m++) {
        const int e = inc[m] >> 1, side = inc[m] & 1;
        const hs_pg_rec R = rec[e];
        const int i = ij[2 * (size_t)e], j = ij[2 * (size_t)e + 1];
        const size_t o = (size_t)(side ? i : j);                           // the edge's other end
        const double po[3] = { p[3 * o], p[3 * o + 1], p[3 * o + 2] };
        double t[3], J[3][3];
        if (side) hs_pg_edge_t(R, po, pn, t); else hs_pg_edge_t(R, pn, po, t);
        hs_pg_jac(R, side, J);
        hs_pg_add_jtv(J, t, q);
    }
}

// rule 6: a field's term of one node
__host__ __device__ static inline double hs_pg_dot3(const double u[3], const double v[3]) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }

// rule 7: what is tested before iteration k and inside it
__host__ __device__ static inline bool hs_pg_converged(double rz, double rz0, double tol) { return rz <= (tol * tol) * rz0 || rz <= 0.0; }
__host__ __device__ static inline bool hs_pg_breakdown(double pq) { return !(pq > 0.0); }
// slamhip_pg_iter.stopped from the device's stop word.  No stop word after every launch the host had to enqueue: iteration n_cg was
// reached, and the tolerance is tested first.
__host__ __device__ static inline int32_t hs_pg_stopped(int32_t stop, double rz, double rz0, double tol)
{
    return stop ? stop - 1 : (hs_pg_converged(rz, rz0, tol) ? HS_PG_STOP_TOL : HS_PG_STOP_NCG);
}

// the end of an outer iteration: pose += x, theta wrapped by rule 2
__host__ __device__ static inline void hs_pg_add_pose(double pose[3], const double x[3])
{
    for (int a = 0; a < 3; a++) pose[a] = pose[a] + x[a];
    pose[2] = hs_pg_wrap(pose[2]);
}

// what slamhip_hs_pg_relax refuses of its spec
static inline bool hs_pg_spec_ok(const slamhip_pg_spec *sp)
{
    return sp->n_outer >= 1 && sp->n_outer <= HS_PG_MAX_OUTER && sp->n_cg >= 1 && sp->n_cg <= HS_PG_MAX_CG && sp->check_every >= 1 && sp->reserved == 0 &&
           isfinite(sp->lambda) && sp->lambda >= 0.0 && isfinite(sp->tol) && sp->tol >= 0.0;
}

// rule 6 on the host, in place: t holds L values and room for L rounded up to a multiple of 256
static inline double hs_pg_tree_sum(double *t, size_t L)
{
    do {
        const size_t blocks = L ? (L + HS_PG_BLOCK - 1) / HS_PG_BLOCK : 1;
        for (size_t i = L; i < blocks * HS_PG_BLOCK; i++) t[i] = 0.0;
        for (size_t b = 0; b < blocks; b++) {
            double *v = t + b * HS_PG_BLOCK;
            for (int h = HS_PG_BLOCK / 2; h >= 1; h >>= 1)
                for (int k = 0; k < h; k++) v[k] = v[k] + v[k + h];
            t[b] = v[0];                                                   // (b <= b * 256: what is overwritten has been read)
        }
        L = blocks;
    } while (L > 1);
    return t[0];
}
