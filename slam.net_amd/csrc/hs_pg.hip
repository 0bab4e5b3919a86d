// hs_pg.hip -- K19, the relaxation of a 2-D pose graph on the device: Gauss-Newton steps, each solved matrix-free by block-Jacobi
// preconditioned conjugate gradients (slamhip_hs_pg_set, _pg_relax, _pg_get, _pg_residuals, _pg_clear, slamhip_debug_pg_relax, _pg_sum,
// _sincos).  No reference counterpart.  Definition: include/slamhip.h (slamhip_hs_pg_relax); the arithmetic host and device share:
// hs_pg.h -- the per-node loops of rules 4 and 5 included, so a kernel and the host hook differ only in who walks the nodes.
// K22 (hs_pg_tri.inc), K26 (hs_pg_lm.inc) and K27 (hs_pg_marg.inc) are the later parts of this translation unit.  They share ONE PCG
// enqueue loop (hs_pg_pcg_loop, behind hs_pg_pcg and K27's batch), ONE "n_outer steps, final chi2, read-back" (hs_pg_relax_run) and ONE
// host definition (hs_pg_host_relax, its PCG hs_pg_host_pcg), each with the preconditioner as an argument; they stand in hs_pg_tri.inc,
// behind K22's launch functions and host text, which they call.
//
// The graph lies in ONE device block: the poses, the fixed bytes, the edges (ij, z, w) and the node -> (edge, side) lists the host
// builds by a counting sort that keeps the edge order (off[N + 1], inc[2 E], an entry edge << 1 | side), then what the kernels write.
// Node vectors are arrays of three doubles per node (a gather of p_j is one 24-byte read); an edge's record is 64 bytes.
//  * k19_linearise: a lane per edge, rule 3; chi2_e's block sums.
//  * k19_diag: a lane per node, rule 4 over the node's list, M; then rule 7's start (x, res, z, p) and the block sums of res . z.
//  * k19_begin: ONE workgroup, once per outer iteration: chi2 and rz0 from the block sums, the state's reset.
//  * k19_apply: a lane per node, rule 5 fused -- t_e is formed again at each end of an edge, the same bits --; block sums of p . q.
//  * k19_step<true>: every workgroup finishes rule 6's tree of p . q itself (k19_total), so alpha needs no launch of its own; the
//    axpys, z = M res, block sums of res . z.  k19_step<false> ends behind the axpys: what K22 launches ahead of its own solve.
//  * k19_dir: every workgroup finishes the tree of res . z, beta, p = z + beta p; workgroup 0 stores rz and the count.
//  * k19_update: pose += x, wrap; workgroup 0 writes the outer iteration's slamhip_pg_iter.
// The stop word (k19_state.stop): set by workgroup 0 of k19_apply (tolerance) or k19_step (breakdown) from scalars that earlier launches
// left, so every workgroup of that launch takes the same decision on its own; every later k19_apply / _step / _dir reads it once per
// workgroup (through LDS, so a workgroup never splits on it) and leaves.  No kernel waits on another workgroup.
#include "hs_blocks.h"
#include "hs_pg.h"
#include "hs_pg_tri.h"
#include "hs_pg_lm.h"
#include "hs_pg_marg.h"
#include <algorithm>
#include <string.h>
#include <vector>

#define K19_LANES HS_PG_BLOCK
// Developer build for a timing of docs/EXPERIMENTS.md (tools/build_variant.py WORK <tag> -DK19_SCALAR_LAUNCH=1); the same bits either way.
#ifndef K19_SCALAR_LAUNCH
#define K19_SCALAR_LAUNCH 0                // 1: alpha, beta and the stop word by a one-workgroup launch behind k19_apply and behind k19_step
#endif
// the most PCG iterations enqueued between two reads of the stop word, whatever check_every says (no result depends on it)
#define K19_MAX_BATCH 1024

static_assert(sizeof(slamhip_pg_spec) == 32 && sizeof(slamhip_pg_iter) == 32 && sizeof(hs_pg_rec) == 64, "the records of include/slamhip.h");
static_assert(HS_PG_MAX_NODES == SLAMHIP_PG_MAX_NODES && HS_PG_MAX_EDGES == SLAMHIP_PG_MAX_EDGES, "the limits of include/slamhip.h");

struct k19_state { double rz[2]; double rz0, chi2; int32_t stop, iters; double alpha, beta; };

struct k19_arg {
    int N, E, PN, PE;                                      // PN, PE: workgroups over the nodes, over the edges (at least 1 each)
    double *pose; const unsigned char *fixed;
    const int2 *ij; const double *z, *w;
    const int32_t *off, *inc;
    hs_pg_rec *rec; double *r, *chi2e;
    double *M, *x, *res, *zv, *p, *q;
    double *part_e, *part_a, *part_b;
    k19_state *st; slamhip_pg_iter *iters; double *final_chi2;
};

// rule 6's block: 256 values, one per lane, t[k] += t[k + h] for h = 128 .. 1 -- the h below 64 inside wavefront 0 by shuffles (lane k
// adds lane k + h's value; the lanes k >= h hold what nothing reads).  Every lane returns the sum.
__device__ static inline double k19_block_sum(double v, double *lds)
{
    const int tid = threadIdx.x;
    lds[tid] = v;
    __syncthreads();
    if (tid < 128) lds[tid] = lds[tid] + lds[tid + 128];
    __syncthreads();
    if (tid < 64) {
        double t = lds[tid] + lds[tid + 64];
        for (int h = 32; h >= 1; h >>= 1) t = t + __shfl_down(t, h, 64);
        if (tid == 0) lds[0] = t;
    }
    __syncthreads();
    const double r = lds[0];
    __syncthreads();
    return r;
}

// the levels of rule 6's tree above the block sums: P values (at most 2^14), in every lane of the workgroup
__device__ static inline double k19_total(const double *part, int P, double *lds, double *lds2)
{
    if (P == 1) return part[0];
    const int tid = threadIdx.x, nb = (P + K19_LANES - 1) / K19_LANES;    // nb <= 64
    double r = 0.0;
    for (int b = 0; b < nb; b++) {
        const int i = b * K19_LANES + tid;
        r = k19_block_sum(i < P ? part[i] : 0.0, lds);
        if (tid == 0) lds2[b] = r;
    }
    if (nb == 1) return r;
    __syncthreads();
    return k19_block_sum(tid < nb ? lds2[tid] : 0.0, lds);
}

// the stop word, once per workgroup
__device__ static inline bool k19_stopped(const k19_state *st, int *stop_s)
{
    if (threadIdx.x == 0) *stop_s = __hip_atomic_load(&st->stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    return *stop_s != 0;
}

__device__ static inline void k19_load3(const double *a, int n, double v[3]) { v[0] = a[3 * (size_t)n]; v[1] = a[3 * (size_t)n + 1]; v[2] = a[3 * (size_t)n + 2]; }
__device__ static inline void k19_store3(double *a, int n, const double v[3]) { a[3 * (size_t)n] = v[0]; a[3 * (size_t)n + 1] = v[1]; a[3 * (size_t)n + 2] = v[2]; }

__global__ void __launch_bounds__(K19_LANES) k19_linearise(const k19_arg A)
{
    __shared__ double lds[K19_LANES];
    const int e = (int)blockIdx.x * K19_LANES + (int)threadIdx.x;
    double term = 0.0;
    if (e < A.E) {
        const int2 ij = A.ij[e];
        double pi[3], pj[3], z[3], w[3], r[3];
        k19_load3(A.pose, ij.x, pi); k19_load3(A.pose, ij.y, pj);
        k19_load3(A.z, e, z); k19_load3(A.w, e, w);
        hs_pg_rec R;
        hs_pg_edge(pi, pj, z, w, &R, r);
        A.rec[e] = R;
        k19_store3(A.r, e, r);
        A.chi2e[e] = R.chi2;
        term = R.chi2;
    }
    const double sum = k19_block_sum(term, lds);
    if (threadIdx.x == 0) A.part_e[blockIdx.x] = sum;
}

__global__ void __launch_bounds__(K19_LANES) k19_diag(const k19_arg A, double lambda)
{
    __shared__ double lds[K19_LANES];
    const int n = (int)blockIdx.x * K19_LANES + (int)threadIdx.x;
    double term = 0.0;
    if (n < A.N) {
        double D[6], g[3] = { 0.0, 0.0, 0.0 }, M[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
        if (!A.fixed[n]) {
            hs_pg_node_diag(lambda, n, A.off, A.inc, A.rec, A.r, D, g);
            (void)hs_pg_inv(D, M);
        }
        for (int m = 0; m < 6; m++) A.M[6 * (size_t)n + m] = M[m];
        const double x[3] = { 0.0, 0.0, 0.0 }, res[3] = { -g[0], -g[1], -g[2] };
        double zv[3];
        hs_pg_mul(M, res, zv);
        k19_store3(A.x, n, x); k19_store3(A.res, n, res); k19_store3(A.zv, n, zv); k19_store3(A.p, n, zv);
        term = hs_pg_dot3(res, zv);
    }
    const double sum = k19_block_sum(term, lds);
    if (threadIdx.x == 0) A.part_b[blockIdx.x] = sum;
}

// one workgroup.  final_only: chi2 at the poses as they stand, beside the array; else the start of an outer iteration's PCG
__global__ void __launch_bounds__(K19_LANES) k19_begin(const k19_arg A, int final_only)
{
    __shared__ double lds[K19_LANES], lds2[64];
    const double chi2 = k19_total(A.part_e, A.PE, lds, lds2);
    if (final_only) {
        if (threadIdx.x == 0) *A.final_chi2 = chi2;
        return;
    }
    __syncthreads();
    const double rz0 = k19_total(A.part_b, A.PN, lds, lds2);
    if (threadIdx.x == 0) {
        A.st->chi2 = chi2; A.st->rz0 = rz0; A.st->rz[0] = rz0; A.st->rz[1] = rz0;
        A.st->iters = 0;
        __hip_atomic_store(&A.st->stop, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ void __launch_bounds__(K19_LANES) k19_apply(const k19_arg A, int k, double lambda, double tol)
{
    __shared__ double lds[K19_LANES];
    __shared__ int stop_s;
    if (k19_stopped(A.st, &stop_s)) return;
    if (hs_pg_converged(A.st->rz[k & 1], A.st->rz0, tol)) {                // (scalars of earlier launches: the same in every workgroup)
        if (blockIdx.x == 0 && threadIdx.x == 0) __hip_atomic_store(&A.st->stop, 1 + HS_PG_STOP_TOL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    const int n = (int)blockIdx.x * K19_LANES + (int)threadIdx.x;
    double term = 0.0;
    if (n < A.N) {
        double pn[3], q[3] = { 0.0, 0.0, 0.0 };
        k19_load3(A.p, n, pn);
        if (!A.fixed[n]) hs_pg_node_apply(lambda, A.p, n, A.off, A.inc, A.rec, (const int32_t *)A.ij, q);
        k19_store3(A.q, n, q);
        term = hs_pg_dot3(pn, q);
    }
    const double sum = k19_block_sum(term, lds);
    if (threadIdx.x == 0) A.part_a[blockIdx.x] = sum;
}

// JACOBI: with rule 7's z = M res and the block sums of res . z; without, another preconditioner's launches form them (K22's solve)
template <bool JACOBI>
__global__ void __launch_bounds__(K19_LANES) k19_step(const k19_arg A, int k)
{
    __shared__ double lds[K19_LANES], lds2[64];
    __shared__ int stop_s;
    if (k19_stopped(A.st, &stop_s)) return;
#if K19_SCALAR_LAUNCH
    const double alpha = A.st->alpha;                                      // (k19_scal_a; a breakdown has set the stop word)
#else
    const double pq = k19_total(A.part_a, A.PN, lds, lds2);
    if (hs_pg_breakdown(pq)) {                                             // (the same in every workgroup)
        if (blockIdx.x == 0 && threadIdx.x == 0) __hip_atomic_store(&A.st->stop, 1 + HS_PG_STOP_BREAKDOWN, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    const double alpha = A.st->rz[k & 1] / pq;
#endif
    const int n = (int)blockIdx.x * K19_LANES + (int)threadIdx.x;
    double term = 0.0;
    if (n < A.N) {
        double x[3], res[3], p[3], q[3], M[6], zv[3];
        k19_load3(A.x, n, x); k19_load3(A.res, n, res); k19_load3(A.p, n, p); k19_load3(A.q, n, q);
        if (JACOBI) for (int m = 0; m < 6; m++) M[m] = A.M[6 * (size_t)n + m];
        for (int a = 0; a < 3; a++) { x[a] = x[a] + alpha * p[a]; res[a] = res[a] - alpha * q[a]; }
        if (JACOBI) hs_pg_mul(M, res, zv);
        k19_store3(A.x, n, x); k19_store3(A.res, n, res);
        if (JACOBI) {
            k19_store3(A.zv, n, zv);
            term = hs_pg_dot3(res, zv);
        }
    }
    if (!JACOBI) return;
    const double sum = k19_block_sum(term, lds);
    if (threadIdx.x == 0) A.part_b[blockIdx.x] = sum;
}

__global__ void __launch_bounds__(K19_LANES) k19_dir(const k19_arg A, int k)
{
    __shared__ double lds[K19_LANES], lds2[64];
    __shared__ int stop_s;
    if (k19_stopped(A.st, &stop_s)) return;
#if K19_SCALAR_LAUNCH
    const double beta = A.st->beta;                                        // (k19_scal_b, which has stored rz and the count too)
#else
    const double rzn = k19_total(A.part_b, A.PN, lds, lds2);
    const double beta = rzn / A.st->rz[k & 1];
#endif
    const int n = (int)blockIdx.x * K19_LANES + (int)threadIdx.x;
    if (n < A.N) {
        double p[3], zv[3];
        k19_load3(A.p, n, p); k19_load3(A.zv, n, zv);
        for (int a = 0; a < 3; a++) p[a] = zv[a] + beta * p[a];
        k19_store3(A.p, n, p);
    }
#if !K19_SCALAR_LAUNCH
    if (blockIdx.x == 0 && threadIdx.x == 0) { A.st->rz[(k + 1) & 1] = rzn; A.st->iters = k + 1; }   // (this launch reads rz[k & 1] alone)
#endif
}

#if K19_SCALAR_LAUNCH
// one workgroup behind k19_apply: p . q, the breakdown test, alpha
__global__ void __launch_bounds__(K19_LANES) k19_scal_a(const k19_arg A, int k)
{
    __shared__ double lds[K19_LANES], lds2[64];
    __shared__ int stop_s;
    if (k19_stopped(A.st, &stop_s)) return;
    const double pq = k19_total(A.part_a, A.PN, lds, lds2);
    if (threadIdx.x != 0) return;
    if (hs_pg_breakdown(pq)) __hip_atomic_store(&A.st->stop, 1 + HS_PG_STOP_BREAKDOWN, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else A.st->alpha = A.st->rz[k & 1] / pq;
}
// one workgroup behind k19_step: res . z, beta, rz and the count
__global__ void __launch_bounds__(K19_LANES) k19_scal_b(const k19_arg A, int k)
{
    __shared__ double lds[K19_LANES], lds2[64];
    __shared__ int stop_s;
    if (k19_stopped(A.st, &stop_s)) return;
    const double rzn = k19_total(A.part_b, A.PN, lds, lds2);
    if (threadIdx.x != 0) return;
    A.st->beta = rzn / A.st->rz[k & 1];
    A.st->rz[(k + 1) & 1] = rzn; A.st->iters = k + 1;
}
#endif

__global__ void __launch_bounds__(K19_LANES) k19_update(const k19_arg A, double tol, int outer)
{
    const int n = (int)blockIdx.x * K19_LANES + (int)threadIdx.x;
    if (n < A.N && !A.fixed[n]) {
        double pose[3], x[3];
        k19_load3(A.pose, n, pose); k19_load3(A.x, n, x);
        hs_pg_add_pose(pose, x);
        k19_store3(A.pose, n, pose);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const k19_state *S = A.st;                                         // (read in place: a copy indexed by iters would be put into LDS)
        slamhip_pg_iter I;
        I.chi2 = S->chi2; I.rz0 = S->rz0; I.cg_iters = S->iters; I.rz = S->rz[I.cg_iters & 1];
        I.stopped = hs_pg_stopped(S->stop, I.rz, I.rz0, tol);
        A.iters[outer] = I;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------
// What the unit keeps, made by slamhip_hs_pg_set: the sizes, the one device block and the places in it, the pinned block the graph
// leaves the host through and the results come back in.
struct hs_pg {
    bool have;
    k19_arg A;
    hs_block<unsigned char, HS_MEM_DEVICE> d_blob;
    hs_block<unsigned char, HS_MEM_PINNED> h_io;
    hs_block<unsigned char, HS_MEM_DEVICE> d_tri;                  // K22 (hs_pg_tri.inc): the levels' blocks, made by the first _pg_relax_tri / _pg_tri_apply
    hs_tri_plan T;
    hs_block<unsigned char, HS_MEM_DEVICE> d_lm;                    // K26 (hs_pg_lm.inc): the weights, the trial poses and the records, made by the first _pg_relax_lm
    hs_block<unsigned char, HS_MEM_DEVICE> d_marg;                // K27 (hs_pg_marg.inc): the query and the batch's work block, made by the first _pg_marginals
    std::vector<unsigned char> fx;                         // the fixed bytes as the device has them: K27 forms its columns on the host
};

void hs_pg_reset(slamhip_hs *hs)
{
    if (hs->pg) hs->pg->have = false;
}

// rule 1: what slamhip_hs_pg_set and slamhip_debug_pg_relax refuse
static int32_t hs_pg_check_graph(const double *poses, const uint8_t *fixed, int32_t N, const int32_t *ij, const double *z, const double *w, int32_t E)
{
    if (N < 1 || N > HS_PG_MAX_NODES) SH_FAIL(SLAMHIP_ERR_INVALID, "pose graph: N = %d must lie in [1, 2^20]", N);
    if (E < 0 || E > HS_PG_MAX_EDGES) SH_FAIL(SLAMHIP_ERR_INVALID, "pose graph: E = %d must lie in [0, 2^22]", E);
    SH_CHECK_ARG(poses && (E == 0 || (ij && z && w)));
    for (int n = 0; n < N; n++) {
        const double *p = poses + 3 * (size_t)n;
        if (!isfinite(p[0]) || !isfinite(p[1]) || !(fabs(p[2]) <= 65536.0))
            SH_FAIL(SLAMHIP_ERR_INVALID, "pose graph: node %d = (%g, %g, %g) must be finite with |theta| <= 65536", n, p[0], p[1], p[2]);
    }
    if (fixed) {
        bool any = false;
        for (int n = 0; n < N && !any; n++) any = fixed[n] != 0;
        if (!any) SH_FAIL(SLAMHIP_ERR_INVALID, "pose graph: no node is fixed");
    }
    for (int e = 0; e < E; e++) {
        const int i = ij[2 * (size_t)e], j = ij[2 * (size_t)e + 1];
        if (i < 0 || i >= N || j < 0 || j >= N || i == j) SH_FAIL(SLAMHIP_ERR_INVALID, "pose graph: edge %d = (%d, %d) of %d nodes", e, i, j, N);
        for (int a = 0; a < 3; a++) {
            const double zz = z[3 * (size_t)e + a], ww = w[3 * (size_t)e + a];
            if (!isfinite(zz)) SH_FAIL(SLAMHIP_ERR_INVALID, "pose graph: edge %d has a measurement that is not finite", e);
            if (!isfinite(ww) || !(ww > 0.0)) SH_FAIL(SLAMHIP_ERR_INVALID, "pose graph: edge %d has the weight %g: it must be finite and > 0", e, ww);
        }
    }
    return SLAMHIP_OK;
}

static int32_t hs_pg_check_spec(const slamhip_pg_spec *sp)
{
    if (!hs_pg_spec_ok(sp))
        SH_FAIL(SLAMHIP_ERR_INVALID, "pose graph: n_outer = %d in [1, 64], n_cg = %d in [1, 2^20], check_every = %d >= 1, reserved = %d == 0, lambda = %g and tol = %g finite and >= 0",
                sp->n_outer, sp->n_cg, sp->check_every, sp->reserved, sp->lambda, sp->tol);
    return SLAMHIP_OK;
}

// the node -> (edge, side) lists: a counting sort that keeps the edge order, the i side of an edge before its j side
static void hs_pg_lists(int N, const int32_t *ij, int E, int32_t *off, int32_t *inc)
{
    for (int n = 0; n <= N; n++) off[n] = 0;
    for (size_t m = 0; m < 2 * (size_t)E; m++) off[ij[m] + 1]++;
    for (int n = 0; n < N; n++) off[n + 1] += off[n];
    std::vector<int32_t> at(off, off + N);
    for (int e = 0; e < E; e++)
        for (int side = 0; side < 2; side++) inc[at[(size_t)ij[2 * (size_t)e + side]]++] = (e << 1) | side;
}

// the fixed bytes, N of them: the caller's as 0 / 1, or node 0 alone
static void hs_pg_fixed_bytes(const uint8_t *fixed, int N, unsigned char *out)
{
    if (fixed) for (int n = 0; n < N; n++) out[n] = fixed[n] ? 1 : 0;
    else { memset(out, 0, (size_t)N); out[0] = 1; }
}

static inline size_t hs_pg_al(size_t b) { return (b + 255) & ~(size_t)255; }

static int32_t hs_pg_need(const slamhip_hs *hs, const char *who)
{
    if (!hs->pg || !hs->pg->have) SH_FAIL(SLAMHIP_ERR_STATE, "%s: no pose graph (slamhip_hs_pg_set first)", who);
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_pg_set(slamhip_hs *hs, const double *poses, const uint8_t *fixed, int32_t N, const int32_t *ij, const double *z, const double *w,
                                     int32_t E)
{
    SH_CHECK_ARG(hs);
    SH_TRY(hs_pg_check_graph(poses, fixed, N, ij, z, w, E));
    slamhip_ctx *ctx = hs->ctx;
    SH_TRY(hs_call_begin(hs));
    SH_TRY(hs_unit<&slamhip_hs::pg>(hs));
    hs_pg *g = hs->pg;
    g->have = false;
    const size_t n = (size_t)N, e = (size_t)E;
    const int PN = sh_div_up(N, K19_LANES), PE = E ? sh_div_up(E, K19_LANES) : 1;
    // what the host fills, in this order, then what the kernels write
    size_t o = 0;
    const size_t o_pose = o; o += hs_pg_al(24 * n);
    const size_t o_fixed = o; o += hs_pg_al(n);
    const size_t o_ij = o; o += hs_pg_al(8 * e);
    const size_t o_z = o; o += hs_pg_al(24 * e);
    const size_t o_w = o; o += hs_pg_al(24 * e);
    const size_t o_off = o; o += hs_pg_al(4 * (n + 1));
    const size_t o_inc = o; o += hs_pg_al(8 * e);
    const size_t in_bytes = o;
    const size_t o_rec = o; o += hs_pg_al(sizeof(hs_pg_rec) * e);
    const size_t o_r = o; o += hs_pg_al(24 * e);
    const size_t o_chi2e = o; o += hs_pg_al(8 * e);
    const size_t o_M = o; o += hs_pg_al(48 * n);
    size_t o_vec[5];
    for (int v = 0; v < 5; v++) { o_vec[v] = o; o += hs_pg_al(24 * n); }
    const size_t o_pe = o; o += hs_pg_al(8 * (size_t)PE);
    const size_t o_pa = o; o += hs_pg_al(8 * (size_t)PN);
    const size_t o_pb = o; o += hs_pg_al(8 * (size_t)PN);
    const size_t o_st = o; o += hs_pg_al(sizeof(k19_state));
    const size_t o_it = o; o += hs_pg_al(sizeof(slamhip_pg_iter) * HS_PG_MAX_OUTER);
    const size_t o_fin = o; o += hs_pg_al(8);
    SH_TRY(g->d_blob.grow(o, "pose graph"));
    SH_TRY(g->h_io.grow(std::max(in_bytes, 32 * e), "pose graph"));
    unsigned char *h = g->h_io, *d = g->d_blob;
    memcpy(h + o_pose, poses, 24 * n);
    hs_pg_fixed_bytes(fixed, N, h + o_fixed);
    g->fx.assign(h + o_fixed, h + o_fixed + n);
    if (E) { memcpy(h + o_ij, ij, 8 * e); memcpy(h + o_z, z, 24 * e); memcpy(h + o_w, w, 24 * e); }
    hs_pg_lists(N, ij, E, (int32_t *)(h + o_off), (int32_t *)(h + o_inc));
    SH_HIP(hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    SH_TRY(hs_call_finish(hs));
    k19_arg &A = g->A;
    A.N = N; A.E = E; A.PN = PN; A.PE = PE;
    A.pose = (double *)(d + o_pose); A.fixed = d + o_fixed;
    A.ij = (const int2 *)(d + o_ij); A.z = (const double *)(d + o_z); A.w = (const double *)(d + o_w);
    A.off = (const int32_t *)(d + o_off); A.inc = (const int32_t *)(d + o_inc);
    A.rec = (hs_pg_rec *)(d + o_rec); A.r = (double *)(d + o_r); A.chi2e = (double *)(d + o_chi2e);
    A.M = (double *)(d + o_M);
    A.x = (double *)(d + o_vec[0]); A.res = (double *)(d + o_vec[1]); A.zv = (double *)(d + o_vec[2]); A.p = (double *)(d + o_vec[3]); A.q = (double *)(d + o_vec[4]);
    A.part_e = (double *)(d + o_pe); A.part_a = (double *)(d + o_pa); A.part_b = (double *)(d + o_pb);
    A.st = (k19_state *)(d + o_st); A.iters = (slamhip_pg_iter *)(d + o_it); A.final_chi2 = (double *)(d + o_fin);
    g->have = true;
    return SLAMHIP_OK;
}

#define K19_LAUNCH(kernel, wgs, ...) do { hipLaunchKernelGGL(kernel, dim3((unsigned)(wgs)), dim3(K19_LANES), 0, st, __VA_ARGS__); SH_HIP(hipGetLastError()); } while (0)

// n_outer Gauss-Newton steps, the final chi2, the read-back: behind K22's launch functions in hs_pg_tri.inc, which it calls with tri
static int32_t hs_pg_relax_run(slamhip_hs *hs, const slamhip_pg_spec *spec, bool tri, const char *who, slamhip_pg_iter *out_iters, double *out_chi2_final);

extern "C" int32_t slamhip_hs_pg_relax(slamhip_hs *hs, const slamhip_pg_spec *spec, slamhip_pg_iter *out_iters, double *out_chi2_final)
{
    SH_CHECK_ARG(hs && spec && out_iters && out_chi2_final);
    return hs_pg_relax_run(hs, spec, false, "pose graph relax", out_iters, out_chi2_final);
}

extern "C" int32_t slamhip_hs_pg_get(slamhip_hs *hs, double *poses, int32_t N)
{
    SH_CHECK_ARG(hs && poses);
    SH_TRY(hs_pg_need(hs, "pose graph get"));
    hs_pg *g = hs->pg;
    if (N != g->A.N) SH_FAIL(SLAMHIP_ERR_INVALID, "pose graph get: N = %d, but the graph has %d nodes", N, g->A.N);
    SH_TRY(hs_call_begin(hs));
    const size_t bytes = 24 * (size_t)N;
    SH_TRY(g->h_io.grow(bytes, "pose graph get"));
    SH_HIP(hipMemcpyAsync(g->h_io, g->A.pose, bytes, hipMemcpyDeviceToHost, hs->ctx->stream));
    SH_TRY(hs_call_finish(hs));
    memcpy(poses, g->h_io, bytes);
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_pg_residuals(slamhip_hs *hs, double *out_r, double *out_chi2)
{
    SH_CHECK_ARG(hs && (out_r || out_chi2));
    SH_TRY(hs_pg_need(hs, "pose graph residuals"));
    hs_pg *g = hs->pg;
    const k19_arg &A = g->A;
    if (A.E == 0) return SLAMHIP_OK;
    hipStream_t st = hs->ctx->stream;
    SH_TRY(hs_call_begin(hs));
    const size_t e = (size_t)A.E;
    SH_TRY(g->h_io.grow(32 * e, "pose graph residuals"));
    K19_LAUNCH(k19_linearise, A.PE, A);
    SH_HIP(hipMemcpyAsync(g->h_io, A.r, 24 * e, hipMemcpyDeviceToHost, st));
    SH_HIP(hipMemcpyAsync(g->h_io + 24 * e, A.chi2e, 8 * e, hipMemcpyDeviceToHost, st));
    SH_TRY(hs_call_finish(hs));
    if (out_r) memcpy(out_r, g->h_io, 24 * e);
    if (out_chi2) memcpy(out_chi2, g->h_io + 24 * e, 8 * e);
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_pg_clear(slamhip_hs *hs)
{
    SH_CHECK_ARG(hs);
    if (!hs->pg) return SLAMHIP_OK;
    SH_TRY(hs_call_begin(hs));
    SH_TRY(hs_call_finish(hs));                                            // (the block is idle behind it)
    hs_unit_drop<&slamhip_hs::pg>(hs);
    return SLAMHIP_OK;
}

// ---- CPU-side test hooks: hs_pg.h -- the text the kernels run -- in plain loops ------------------------------------------------------
// what slamhip_hs_pg_set makes of a graph beside its arrays: the node -> (edge, side) lists and the fixed bytes
struct hs_pg_host_lists { std::vector<int32_t> off, inc; std::vector<unsigned char> fx; };

static void hs_pg_host_lists_init(hs_pg_host_lists &G, const uint8_t *fixed, int N, const int32_t *ij, int E)
{
    G.off.resize((size_t)N + 1); G.inc.resize(2 * (size_t)E + 1); G.fx.resize((size_t)N);
    hs_pg_lists(N, ij, E, G.off.data(), G.inc.data());
    hs_pg_fixed_bytes(fixed, N, G.fx.data());
}

// rule 3 over every edge -> chi2 by rule 6
static double hs_pg_host_linearise(const double *pose, const int32_t *ij, const double *z, const double *w, int E, hs_pg_rec *rec, double *r, double *tmp)
{
    for (int e = 0; e < E; e++) {
        hs_pg_edge(pose + 3 * (size_t)ij[2 * (size_t)e], pose + 3 * (size_t)ij[2 * (size_t)e + 1], z + 3 * (size_t)e, w + 3 * (size_t)e, &rec[e], r + 3 * (size_t)e);
        tmp[e] = rec[e].chi2;
    }
    return hs_pg_tree_sum(tmp, (size_t)E);
}

static double hs_pg_host_dot(const double *u, const double *v, int N, double *tmp)
{
    for (int n = 0; n < N; n++) tmp[n] = hs_pg_dot3(u + 3 * (size_t)n, v + 3 * (size_t)n);
    return hs_pg_tree_sum(tmp, (size_t)N);
}

// the definition of K19 and of K22 over a graph and a spec that have been checked: behind K22's host text in hs_pg_tri.inc, which it
// runs with tri
static void hs_pg_host_relax(bool tri, double *poses, const uint8_t *fixed, int32_t N, const int32_t *ij, const double *z, const double *w, int32_t E,
                             const slamhip_pg_spec *spec, slamhip_pg_iter *out_iters, double *out_chi2_final, double *out_r, double *out_chi2);

extern "C" int32_t slamhip_debug_pg_relax(double *poses, const uint8_t *fixed, int32_t N, const int32_t *ij, const double *z, const double *w, int32_t E,
                                          const slamhip_pg_spec *spec, slamhip_pg_iter *out_iters, double *out_chi2_final, double *out_r, double *out_chi2)
{
    SH_CHECK_ARG(spec && out_iters && out_chi2_final);
    SH_TRY(hs_pg_check_spec(spec));
    SH_TRY(hs_pg_check_graph(poses, fixed, N, ij, z, w, E));
    hs_pg_host_relax(false, poses, fixed, N, ij, z, w, E, spec, out_iters, out_chi2_final, out_r, out_chi2);
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_debug_pg_sum(const double *v, int32_t L, double *out)
{
    SH_CHECK_ARG(out && L >= 0 && (v || L == 0));
    std::vector<double> t((size_t)L + HS_PG_BLOCK);
    if (L) memcpy(t.data(), v, 8 * (size_t)L);
    *out = hs_pg_tree_sum(t.data(), (size_t)L);
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_debug_sincos(const double *a, int32_t n, double *out_s, double *out_c)
{
    SH_CHECK_ARG(n >= 0 && (n == 0 || (a && out_s && out_c)));
    for (int i = 0; i < n; i++) sh_det_sincos(a[i], &out_s[i], &out_c[i]);
    return SLAMHIP_OK;
}

#include "hs_pg_tri.inc"
#include "hs_pg_lm.inc"
#include "hs_pg_marg.inc"
