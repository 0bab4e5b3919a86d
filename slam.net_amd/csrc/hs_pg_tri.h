// hs_pg_tri.h -- the arithmetic of the odometry-chain preconditioner of the pose-graph relaxation (K22, hs_pg_tri.inc) that host and
// device share: the kernels k22_* and the test hooks slamhip_debug_pg_relax_tri / _pg_tri_apply run this text, down to rule T2's loop
// over a node's list (hs_tri_node_coupling) and rule T3's block with its choice of neighbours (hs_tri_reduce_block).  Definition:
// include/slamhip.h, slamhip_hs_pg_relax_tri, rules T1 - T5.  Binary64 + - * / only, one rounding per operation (the build has
// -ffp-contract=off); every expression is parenthesised as the definition writes it.
#pragma once
#include "hs_pg.h"

#define HS_TRI_MAX_LEVELS 21               // N <= 2^20: levels of 2^20, 2^19, .. 1 blocks
#define HS_TRI_TAIL 1024                   // S: a level of at most S blocks is finished by ONE workgroup (the solve's right-hand sides in LDS)

// the levels of the block cyclic reduction: n[0] = N, n[l + 1] = ceil(n[l] / 2) down to 1; off[l] = n[0] + .. + n[l - 1].  Every
// level's blocks lie contiguously: block k of level l is entry off[l] + k of D, P (six doubles each, rule 4's order) and U (nine,
// row-major; U_k couples k and k + 1), and entry off[l] + k - N of R (three; level 0's right-hand side is the caller's vector).
struct hs_tri_plan {
    int L, lt;                             // levels; the first level with at most S blocks (the tail's)
    int n[HS_TRI_MAX_LEVELS], off[HS_TRI_MAX_LEVELS];
    double *D, *P, *U, *R;
    unsigned char *live;                   // rule T1, a byte per node
};

static inline int hs_tri_levels(int N, int S, hs_tri_plan *T)
{
    int L = 0, tot = 0;
    for (int n = N;; n = (n + 1) / 2) {
        T->n[L] = n; T->off[L] = tot; tot += n; L++;
        if (n == 1) break;
    }
    T->L = L;
    T->lt = 0;
    while (T->n[T->lt] > S) T->lt++;
    return tot;                            // blocks in all: < 2 N + 21
}

// a symmetric 3 x 3 kept as six: the place of (a, b)
__host__ __device__ static inline double hs_tri_s(const double P[6], int a, int b)
{
    return P[a == b ? (a == 0 ? 0 : (a == 1 ? 3 : 5)) : (a + b == 1 ? 1 : (a + b == 2 ? 2 : 4))];
}

// rule T2: U += Jn^T W Jm for one edge that joins n (Jacobian Jn) and n + 1 (Jm)
__host__ __device__ static inline void hs_tri_add_coupling(const double Jn[3][3], const double Jm[3][3], const hs_pg_rec &R, double U[9])
{
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++)
            U[3 * a + b] = U[3 * a + b] + (((Jn[0][a] * R.wx) * Jm[0][b] + (Jn[1][a] * R.wy) * Jm[1][b]) + (Jn[2][a] * R.wt) * Jm[2][b]);
}

// rule T2 for one node: U_n over the edges of the node's list (hs_pg.h's lists) that join n and n + 1; +0 unless both are live
__host__ __device__ static __forceinline__ void hs_tri_node_coupling(int n, int N, const unsigned char *live, const int32_t *off, const int32_t *inc,
                                                                     const hs_pg_rec *rec, const int32_t *ij, double U[9])
{
    for (int m = 0; m < 9; m++) U[m] = 0.0;
    if (!(n + 1 < N && live[n] && live[n + 1])) return;
    const int m1 = off[n + 1];
    for (int m = off[n]; m < m1; m++) {
        const int e = inc[m] >> 1, side = inc[m] & 1;
        const int i = ij[2 * (size_t)e], j = ij[2 * (size_t)e + 1];
        if ((side ? i : j) != n + 1) continue;
        const hs_pg_rec R = rec[e];
        double Jn[3][3], Jm[3][3];
        hs_pg_jac(R, side, Jn);
        hs_pg_jac(R, side ^ 1, Jm);
        hs_tri_add_coupling(Jn, Jm, R, U);
    }
}

// entry i of an array of n doubles per entry (D, P: 6; U: 9)
__host__ __device__ static inline void hs_tri_load(const double *a, size_t i, int n, double *v) { for (int m = 0; m < n; m++) v[m] = a[(size_t)n * i + m]; }
__host__ __device__ static inline void hs_tri_store(double *a, size_t i, int n, const double *v) { for (int m = 0; m < n; m++) a[(size_t)n * i + m] = v[m]; }

// rule T3: W = P X (xt false) or W = P X^T (xt true)
__host__ __device__ static inline void hs_tri_px(const double P[6], const double X[9], bool xt, double W[9])
{
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) {
            const double x0 = xt ? X[3 * b] : X[b], x1 = xt ? X[3 * b + 1] : X[3 + b], x2 = xt ? X[3 * b + 2] : X[6 + b];
            W[3 * a + b] = (hs_tri_s(P, a, 0) * x0 + hs_tri_s(P, a, 1) * x1) + hs_tri_s(P, a, 2) * x2;
        }
}

// rule T3: one block of the next level from block k = 2 m and its neighbours.  Ul, Pl: U_{k-1}, P_{k-1} (have_l); Uk, Pr: U_k,
// P_{k+1} (have_r); Un: U_{k+1} (have_n: block k + 2 exists).  D' for a <= b in rule 4's order; U' = +0 without block k + 2.
__host__ __device__ static inline void hs_tri_reduce(const double Dk[6], bool have_l, const double Ul[9], const double Pl[6], bool have_r, const double Uk[9],
                                                     const double Pr[6], bool have_n, const double Un[9], double Dn[6], double Uo[9])
{
    double W[9];
    for (int m = 0; m < 6; m++) Dn[m] = Dk[m];
    if (have_l) {
        hs_tri_px(Pl, Ul, false, W);
        int m = 0;
        for (int a = 0; a < 3; a++)
            for (int b = a; b < 3; b++, m++) Dn[m] = Dn[m] - ((Ul[a] * W[b] + Ul[3 + a] * W[3 + b]) + Ul[6 + a] * W[6 + b]);
    }
    if (have_r) {
        hs_tri_px(Pr, Uk, true, W);
        int m = 0;
        for (int a = 0; a < 3; a++)
            for (int b = a; b < 3; b++, m++) Dn[m] = Dn[m] - ((Uk[3 * a] * W[b] + Uk[3 * a + 1] * W[3 + b]) + Uk[3 * a + 2] * W[6 + b]);
    }
    if (have_n) {
        hs_tri_px(Pr, Un, false, W);
        for (int a = 0; a < 3; a++)
            for (int b = 0; b < 3; b++) Uo[3 * a + b] = 0.0 - ((Uk[3 * a] * W[b] + Uk[3 * a + 1] * W[3 + b]) + Uk[3 * a + 2] * W[6 + b]);
    } else {
        for (int m = 0; m < 9; m++) Uo[m] = 0.0;
    }
}

// rule T3 for block m of level l + 1 over the plan's arrays: the neighbours that are there, D', U' and P' = D'^-1
__host__ __device__ static inline void hs_tri_reduce_block(const hs_tri_plan &T, int l, int m)
{
    const int n = T.n[l], k = 2 * m;
    const size_t o = (size_t)T.off[l] + (size_t)k;
    const bool have_l = k >= 1, have_r = k + 1 < n, have_n = k + 2 < n;
    double Dk[6], Ul[9], Pl[6], Uk[9], Pr[6], Un[9], Dn[6], Uo[9], Pn[6];
    hs_tri_load(T.D, o, 6, Dk);
    if (have_l) { hs_tri_load(T.U, o - 1, 9, Ul); hs_tri_load(T.P, o - 1, 6, Pl); }
    if (have_r) { hs_tri_load(T.U, o, 9, Uk); hs_tri_load(T.P, o + 1, 6, Pr); }
    if (have_n) hs_tri_load(T.U, o + 1, 9, Un);
    hs_tri_reduce(Dk, have_l, Ul, Pl, have_r, Uk, Pr, have_n, Un, Dn, Uo);
    (void)hs_pg_inv(Dn, Pn);
    const size_t o1 = (size_t)T.off[l + 1] + (size_t)m;
    hs_tri_store(T.D, o1, 6, Dn); hs_tri_store(T.U, o1, 9, Uo); hs_tri_store(T.P, o1, 6, Pn);
}

// rule T4: v = v - U^T y (the neighbour below: U = U_{k-1}) and v = v - U y (the neighbour above: U = U_k)
__host__ __device__ static inline void hs_tri_sub_ut(const double U[9], const double y[3], double v[3])
{
    for (int a = 0; a < 3; a++) v[a] = v[a] - ((U[a] * y[0] + U[3 + a] * y[1]) + U[6 + a] * y[2]);
}
__host__ __device__ static inline void hs_tri_sub_u(const double U[9], const double y[3], double v[3])
{
    for (int a = 0; a < 3; a++) v[a] = v[a] - ((U[3 * a] * y[0] + U[3 * a + 1] * y[1]) + U[3 * a + 2] * y[2]);
}

// rule T4, forward: the right-hand side of block m of level l + 1 from level l's (rl: n blocks; U, P: level l's)
__host__ __device__ static inline void hs_tri_forward(const double *rl, const double *U, const double *P, int n, int m, double out[3])
{
    const int k = 2 * m;
    double y[3];
    for (int a = 0; a < 3; a++) out[a] = rl[3 * (size_t)k + a];
    if (k >= 1) {
        hs_pg_mul(P + 6 * (size_t)(k - 1), rl + 3 * (size_t)(k - 1), y);
        hs_tri_sub_ut(U + 9 * (size_t)(k - 1), y, out);
    }
    if (k + 1 < n) {
        hs_pg_mul(P + 6 * (size_t)(k + 1), rl + 3 * (size_t)(k + 1), y);
        hs_tri_sub_u(U + 9 * (size_t)k, y, out);
    }
}

// rule T4, backward: z of block k of level l (n blocks; rl, U, P: level l's) from the z of level l + 1
__host__ __device__ static inline void hs_tri_backward(const double *rl, const double *zn, const double *U, const double *P, int n, int k, double out[3])
{
    if (!(k & 1)) {
        for (int a = 0; a < 3; a++) out[a] = zn[3 * (size_t)(k >> 1) + a];
        return;
    }
    double t[3];
    for (int a = 0; a < 3; a++) t[a] = rl[3 * (size_t)k + a];
    hs_tri_sub_ut(U + 9 * (size_t)(k - 1), zn + 3 * (size_t)((k - 1) >> 1), t);
    if (k + 1 < n) hs_tri_sub_u(U + 9 * (size_t)k, zn + 3 * (size_t)((k + 1) >> 1), t);
    hs_pg_mul(P + 6 * (size_t)k, t, out);
}
