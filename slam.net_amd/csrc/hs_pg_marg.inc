// hs_pg_marg.inc -- K27, marginal covariances of the pose graph: blocks of Sigma = H^-1 at the poses as they stand, every column one
// solve H x = e by the unit's PCG, all the columns of a query in ONE batch (slamhip_hs_pg_marginals, slamhip_debug_pg_marginals).  The
// last part of hs_pg.hip's translation unit: k19_linearise, k19_diag, k22_diag, k22_coupling, k22_reduce and k22_factor_tail are launched
// as they are, ONCE per call; the batch's enqueue loop is the unit's (hs_pg_pcg_loop, hs_pg_tri.inc), the hook's PCG the unit's host
// definition (hs_pg_host_pcg).  Definition: include/slamhip.h, rules M1 - M5; shared host / device text: hs_pg_marg.h, hs_pg.h, hs_pg_tri.h.
// A chunk's right-hand side j keeps its node vectors at j * 3 N doubles in x, res, zv, p and q, its block sums in row j of part_a and
// part_b, its scalars in st[j] and its stop word in stop[j].
//  * k27_begin<JACOBI>: grid (node blocks, R_c): res = e, x = 0; JACOBI: z = M res, p = z and the block sums of res . z.
//  * k27_begin_state: a workgroup per right-hand side: rz0 by rule 6's tree, the scalars, the stop word's reset.
//  * k27_apply<G>: grid (node blocks, ceil(R_c / G)), a lane per node with G right-hand sides in registers: an incident edge's record
//    and Jacobians are loaded and formed once and used for the G (hs_marg_node_apply); the block sums of p . q go to each one's row.
//  * k27_step<JACOBI, G>, k27_dir<G>: K19's two kernels over the batch; every workgroup finishes rule 6's tree for its G scalars itself.
//  * k27_forward, k27_solve_tail, k27_backward: K22's solve with the right-hand side on grid y (the tail: a workgroup per right-hand
//    side), D, P and U from the call's single factorisation, the hs_tri_* device functions as they are.
//  * k27_collect: a chunk's records and its share of the blocks.
// A right-hand side's stop word is set by the workgroups x = 0 of k27_apply (tolerance) or k27_step (breakdown) from scalars that
// earlier launches left, so every workgroup takes the same decision on its own; which of a group's right-hand sides are still running
// is read once per workgroup, through LDS.  No kernel waits on another workgroup; no floating-point atomic.

static_assert(sizeof(slamhip_pg_marg_spec) == 40 && sizeof(slamhip_pg_marg_col) == 32 && sizeof(slamhip_pg_marg_info) == 32, "the records of include/slamhip.h");
static_assert(HS_MARG_MAX_PAIRS == SLAMHIP_PG_MARG_MAX_PAIRS && HS_MARG_MAX_COLS == SLAMHIP_PG_MARG_MAX_COLS, "the limits of include/slamhip.h");

struct k27_state { double rz[2]; double rz0; int32_t iters, pad; };

struct k27_arg {
    int Rc, r0, P;                                         // the chunk: its right-hand sides, the first one's place in M1's order; the pairs
    size_t vs, rs;                                         // doubles per right-hand side: of a node vector (3 N), of the levels' right-hand sides
    const int32_t *cols, *pn, *prhs;                       // M1's columns (a node each); per pair its n and its first right-hand side (-1: a +0 block)
    double *x, *res, *zv, *p, *q;
    double *part_a, *part_b;
    double *R;                                             // rule T4's right-hand sides above level 0 (precond = 1)
    k27_state *st; int32_t *stop;
    double *blocks; slamhip_pg_marg_col *recs;
};

// which of the group's right-hand sides are still running: once per workgroup, the same in every lane
template <int G>
__device__ static inline bool k27_running(const k27_arg &B, int j0, int *act_s, bool act[G])
{
    if ((int)threadIdx.x < G) {
        const int j = j0 + (int)threadIdx.x;
        act_s[threadIdx.x] = j < B.Rc && __hip_atomic_load(&B.stop[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0;
    }
    __syncthreads();
    bool any = false;
    for (int g = 0; g < G; g++) { act[g] = __builtin_amdgcn_readfirstlane(act_s[g]) != 0; any = any || act[g]; }
    return any;
}

template <bool JACOBI>
__global__ void __launch_bounds__(K19_LANES) k27_begin(const k19_arg A, const k27_arg B)
{
    __shared__ double lds[K19_LANES];
    const int j = (int)blockIdx.y, n = (int)blockIdx.x * K19_LANES + (int)threadIdx.x;
    const int rhs = B.r0 + j, node = B.cols[rhs / 3], comp = rhs % 3;
    double term = 0.0;
    if (n < A.N) {
        const bool at = n == node;
        const double x[3] = { 0.0, 0.0, 0.0 }, res[3] = { at && comp == 0 ? 1.0 : 0.0, at && comp == 1 ? 1.0 : 0.0, at && comp == 2 ? 1.0 : 0.0 };
        const size_t o = (size_t)j * B.vs;
        k19_store3(B.x + o, n, x); k19_store3(B.res + o, n, res);
        if (JACOBI) {
            double M[6], zv[3];
            for (int m = 0; m < 6; m++) M[m] = A.M[6 * (size_t)n + m];
            hs_pg_mul(M, res, zv);
            k19_store3(B.zv + o, n, zv); k19_store3(B.p + o, n, zv);
            term = hs_pg_dot3(res, zv);
        }
    }
    if (!JACOBI) return;
    const double sum = k19_block_sum(term, lds);
    if (threadIdx.x == 0) B.part_b[(size_t)j * A.PN + blockIdx.x] = sum;
}

__global__ void __launch_bounds__(K19_LANES) k27_begin_state(const k19_arg A, const k27_arg B)
{
    __shared__ double lds[K19_LANES], lds2[64];
    const int j = (int)blockIdx.x;
    const double rz0 = k19_total(B.part_b + (size_t)j * A.PN, A.PN, lds, lds2);
    if (threadIdx.x == 0) {
        k27_state S;
        S.rz[0] = rz0; S.rz[1] = rz0; S.rz0 = rz0; S.iters = 0; S.pad = 0;
        B.st[j] = S;
        __hip_atomic_store(&B.stop[j], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

template <int G>
__global__ void __launch_bounds__(K19_LANES) k27_apply(const k19_arg A, const k27_arg B, int k, double lambda, double tol)
{
    __shared__ double lds[K19_LANES];
    __shared__ int act_s[G];
    const int j0 = (int)blockIdx.y * G;
    if ((int)threadIdx.x < G) {
        const int j = j0 + (int)threadIdx.x;
        int a = 0;
        if (j < B.Rc && __hip_atomic_load(&B.stop[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) {
            if (!hs_pg_converged(B.st[j].rz[k & 1], B.st[j].rz0, tol)) a = 1;   // (scalars of earlier launches: the same in every workgroup)
            else if (blockIdx.x == 0) __hip_atomic_store(&B.stop[j], 1 + HS_PG_STOP_TOL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        act_s[threadIdx.x] = a;
    }
    __syncthreads();
    bool act[G], any = false;
    for (int g = 0; g < G; g++) { act[g] = __builtin_amdgcn_readfirstlane(act_s[g]) != 0; any = any || act[g]; }
    if (!any) return;
    const int n = (int)blockIdx.x * K19_LANES + (int)threadIdx.x;
    const double *p = B.p + (size_t)j0 * B.vs;
    double term[G];
    for (int g = 0; g < G; g++) term[g] = 0.0;
    if (n < A.N) {
        double q[G][3];
        for (int g = 0; g < G; g++) q[g][0] = q[g][1] = q[g][2] = 0.0;
        if (!A.fixed[n]) hs_marg_node_apply<G>(lambda, p, B.vs, act, n, A.off, A.inc, A.rec, (const int32_t *)A.ij, q);
        for (int g = 0; g < G; g++) {
            if (!act[g]) continue;
            double pn[3];
            k19_load3(p + (size_t)g * B.vs, n, pn);
            k19_store3(B.q + (size_t)(j0 + g) * B.vs, n, q[g]);
            term[g] = hs_pg_dot3(pn, q[g]);
        }
    }
    for (int g = 0; g < G; g++) {
        if (!act[g]) continue;
        const double sum = k19_block_sum(term[g], lds);
        if (threadIdx.x == 0) B.part_a[(size_t)(j0 + g) * A.PN + blockIdx.x] = sum;
    }
}

// JACOBI: with rule 7's z = M res and the block sums of res . z; without, the batched solve's launches form them
template <bool JACOBI, int G>
__global__ void __launch_bounds__(K19_LANES) k27_step(const k19_arg A, const k27_arg B, int k)
{
    __shared__ double lds[K19_LANES], lds2[64];
    __shared__ int act_s[G];
    const int j0 = (int)blockIdx.y * G;
    bool act[G];
    if (!k27_running<G>(B, j0, act_s, act)) return;
    const int n = (int)blockIdx.x * K19_LANES + (int)threadIdx.x;
    double M[6];
    if (JACOBI && n < A.N) for (int m = 0; m < 6; m++) M[m] = A.M[6 * (size_t)n + m];
    for (int g = 0; g < G; g++) {
        if (!act[g]) continue;
        const int j = j0 + g;
        const double pq = k19_total(B.part_a + (size_t)j * A.PN, A.PN, lds, lds2);
        if (hs_pg_breakdown(pq)) {                                         // (the same in every workgroup)
            if (blockIdx.x == 0 && threadIdx.x == 0) __hip_atomic_store(&B.stop[j], 1 + HS_PG_STOP_BREAKDOWN, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            continue;
        }
        const double alpha = B.st[j].rz[k & 1] / pq;
        const size_t o = (size_t)j * B.vs;
        double term = 0.0;
        if (n < A.N) {
            double x[3], res[3], p[3], q[3], zv[3];
            k19_load3(B.x + o, n, x); k19_load3(B.res + o, n, res); k19_load3(B.p + o, n, p); k19_load3(B.q + o, n, q);
            for (int a = 0; a < 3; a++) { x[a] = x[a] + alpha * p[a]; res[a] = res[a] - alpha * q[a]; }
            k19_store3(B.x + o, n, x); k19_store3(B.res + o, n, res);
            if (JACOBI) {
                hs_pg_mul(M, res, zv);
                k19_store3(B.zv + o, n, zv);
                term = hs_pg_dot3(res, zv);
            }
        }
        if (JACOBI) {
            const double sum = k19_block_sum(term, lds);
            if (threadIdx.x == 0) B.part_b[(size_t)j * A.PN + blockIdx.x] = sum;
        }
    }
}

template <int G>
__global__ void __launch_bounds__(K19_LANES) k27_dir(const k19_arg A, const k27_arg B, int k)
{
    __shared__ double lds[K19_LANES], lds2[64];
    __shared__ int act_s[G];
    const int j0 = (int)blockIdx.y * G;
    bool act[G];
    if (!k27_running<G>(B, j0, act_s, act)) return;
    const int n = (int)blockIdx.x * K19_LANES + (int)threadIdx.x;
    for (int g = 0; g < G; g++) {
        if (!act[g]) continue;
        const int j = j0 + g;
        const double rzn = k19_total(B.part_b + (size_t)j * A.PN, A.PN, lds, lds2);
        const double beta = rzn / B.st[j].rz[k & 1];
        const size_t o = (size_t)j * B.vs;
        if (n < A.N) {
            double p[3], zv[3];
            k19_load3(B.p + o, n, p); k19_load3(B.zv + o, n, zv);
            for (int a = 0; a < 3; a++) p[a] = zv[a] + beta * p[a];
            k19_store3(B.p + o, n, p);
        }
        if (blockIdx.x == 0 && threadIdx.x == 0) { B.st[j].rz[(k + 1) & 1] = rzn; B.st[j].iters = k + 1; }   // (this launch reads rz[k & 1] alone)
    }
}

// ---- K22's solve over the batch: right-hand side j = grid y (the tail: grid x) --------------------------------------------------------
// first: rule 7's start (no stop word yet; z goes into p too)
__device__ static inline bool k27_stopped(const k27_arg &B, int j, int first, int *stop_s)
{
    if (first) return false;
    if (threadIdx.x == 0) *stop_s = __hip_atomic_load(&B.stop[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    return *stop_s != 0;
}

// right-hand side j's rule T4 right-hand side of level l
__device__ static inline double *k27_rhs(const hs_tri_plan &T, const k27_arg &B, int j, int l)
{
    return l ? B.R + (size_t)j * B.rs + 3 * ((size_t)T.off[l] - (size_t)T.n[0]) : B.res + (size_t)j * B.vs;
}

// level 0's z of node k (rule T1: 0 for a dead node), stored; its term of res . z
__device__ static inline double k27_finish(const hs_tri_plan &T, const k27_arg &B, int j, int first, int k, double z[3])
{
    const size_t o = (size_t)j * B.vs;
    if (!T.live[k]) z[0] = z[1] = z[2] = 0.0;
    k19_store3(B.zv + o, k, z);
    if (first) k19_store3(B.p + o, k, z);
    double r[3];
    k19_load3(B.res + o, k, r);
    return hs_pg_dot3(r, z);
}

__global__ void __launch_bounds__(K19_LANES) k27_forward(const hs_tri_plan T, const k27_arg B, int l, int first)
{
    __shared__ int stop_s;
    const int j = (int)blockIdx.y;
    if (k27_stopped(B, j, first, &stop_s)) return;
    const int m = (int)blockIdx.x * K19_LANES + (int)threadIdx.x;
    if (m >= T.n[l + 1]) return;
    double out[3];
    hs_tri_forward(k27_rhs(T, B, j, l), T.U + 9 * (size_t)T.off[l], T.P + 6 * (size_t)T.off[l], T.n[l], m, out);
    k19_store3(k27_rhs(T, B, j, l + 1), m, out);
}

__global__ void __launch_bounds__(K19_LANES) k27_backward(const hs_tri_plan T, const k27_arg B, int PN, int l, int first)
{
    __shared__ double lds[K19_LANES];
    __shared__ int stop_s;
    const int j = (int)blockIdx.y;
    if (k27_stopped(B, j, first, &stop_s)) return;
    const int k = (int)blockIdx.x * K19_LANES + (int)threadIdx.x;
    double term = 0.0;
    if (k < T.n[l]) {
        double z[3];
        double *rl = k27_rhs(T, B, j, l);
        hs_tri_backward(rl, k27_rhs(T, B, j, l + 1), T.U + 9 * (size_t)T.off[l], T.P + 6 * (size_t)T.off[l], T.n[l], k, z);
        if (l) k19_store3(rl, k, z);                                       // (in place: a lane reads its own block's right-hand side alone)
        else term = k27_finish(T, B, j, first, k, z);
    }
    if (l == 0) {
        const double sum = k19_block_sum(term, lds);
        if (threadIdx.x == 0) B.part_b[(size_t)j * PN + blockIdx.x] = sum;
    }
}

// a workgroup per right-hand side: levels lt .. L - 1 of its application
__global__ void __launch_bounds__(K19_LANES) k27_solve_tail(const hs_tri_plan T, const k27_arg B, int PN, int first)
{
    __shared__ double sr[3 * (2 * HS_TRI_TAIL + 32)];
    __shared__ double lds[K19_LANES];
    __shared__ int stop_s;
    const int j = (int)blockIdx.x;
    if (k27_stopped(B, j, first, &stop_s)) return;
    const int tid = (int)threadIdx.x, lt = T.lt, base = T.off[lt];
    double *r = k27_rhs(T, B, j, lt);
    for (int i = tid; i < 3 * T.n[lt]; i += K19_LANES) sr[i] = r[i];
    __syncthreads();
    for (int l = lt; l + 1 < T.L; l++) {
        double *rl = sr + 3 * (T.off[l] - base), *rn = sr + 3 * (T.off[l + 1] - base);
        for (int m = tid; m < T.n[l + 1]; m += K19_LANES) {
            double out[3];
            hs_tri_forward(rl, T.U + 9 * (size_t)T.off[l], T.P + 6 * (size_t)T.off[l], T.n[l], m, out);
            rn[3 * m] = out[0]; rn[3 * m + 1] = out[1]; rn[3 * m + 2] = out[2];
        }
        __syncthreads();
    }
    if (tid == 0) {                                                        // the last level: z = P r
        double *rl = sr + 3 * (T.off[T.L - 1] - base), z[3];
        hs_pg_mul(T.P + 6 * (size_t)T.off[T.L - 1], rl, z);
        rl[0] = z[0]; rl[1] = z[1]; rl[2] = z[2];
    }
    __syncthreads();
    for (int l = T.L - 2; l >= lt; l--) {
        double *rl = sr + 3 * (T.off[l] - base);
        const double *zn = sr + 3 * (T.off[l + 1] - base);
        for (int k = tid; k < T.n[l]; k += K19_LANES) {
            double z[3];
            hs_tri_backward(rl, zn, T.U + 9 * (size_t)T.off[l], T.P + 6 * (size_t)T.off[l], T.n[l], k, z);
            rl[3 * k] = z[0]; rl[3 * k + 1] = z[1]; rl[3 * k + 2] = z[2];  // (in place: a lane reads its own block's right-hand side alone)
        }
        __syncthreads();
    }
    if (lt) {
        for (int i = tid; i < 3 * T.n[lt]; i += K19_LANES) r[i] = sr[i];
        return;
    }
    const int chunks = (T.n[0] + K19_LANES - 1) / K19_LANES;               // level 0: z, and rule 6's blocks of 256 nodes
    for (int c = 0; c < chunks; c++) {
        const int k = c * K19_LANES + tid;
        double term = 0.0;
        if (k < T.n[0]) {
            double z[3] = { sr[3 * k], sr[3 * k + 1], sr[3 * k + 2] };
            term = k27_finish(T, B, j, first, k, z);
        }
        const double sum = k19_block_sum(term, lds);
        if (tid == 0) B.part_b[(size_t)j * PN + c] = sum;
    }
}

// a lane per right-hand side of the chunk: rule M4's record; a lane per entry of a block: rule M3, for the right-hand sides of the chunk
__global__ void __launch_bounds__(K19_LANES) k27_collect(const k27_arg B, double tol)
{
    const size_t idx = (size_t)blockIdx.x * K19_LANES + threadIdx.x;
    if (idx < (size_t)B.Rc) {
        const int j = (int)idx, rhs = B.r0 + j;
        const k27_state *S = B.st + j;                                     // (read in place: a copy indexed by iters would be put into LDS)
        slamhip_pg_marg_col I;
        I.rz0 = S->rz0; I.cg_iters = S->iters; I.rz = S->rz[I.cg_iters & 1];
        I.stopped = hs_pg_stopped(B.stop[j], I.rz, I.rz0, tol);
        I.node = B.cols[rhs / 3]; I.comp = rhs % 3;
        B.recs[rhs] = I;
    }
    if (idx < 9 * (size_t)B.P) {
        const size_t pr = idx / 9;
        const int ab = (int)(idx % 9), a = ab / 3, b = ab % 3, first = B.prhs[pr];
        const int j = first + b - B.r0;
        if (first >= 0 && j >= 0 && j < B.Rc) B.blocks[idx] = B.x[(size_t)j * B.vs + 3 * (size_t)B.pn[pr] + a];
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------
// the developer's G, among the instantiated ones; no result depends on it
static int hs_marg_group()
{
    return sh_env_int("SLAMHIP_K27_GROUP", HS_MARG_GROUP) == HS_MARG_GROUP_WIDE ? HS_MARG_GROUP_WIDE : HS_MARG_GROUP;
}

static int32_t hs_marg_check_spec(const slamhip_pg_marg_spec *sp)
{
    if (!hs_marg_spec_ok(sp))
        SH_FAIL(SLAMHIP_ERR_INVALID, "pose graph marginals: n_cg = %d in [1, 2^20], check_every = %d >= 1, precond = %d in {0, 1}, reserved = %d == 0, lambda = %g and tol = %g "
                "finite and >= 0, max_bytes = %lld >= 0", sp->n_cg, sp->check_every, sp->precond, sp->reserved, sp->lambda, sp->tol, (long long)sp->max_bytes);
    return SLAMHIP_OK;
}

// rule M1: the columns, and per pair its n and its first right-hand side (-1: n or m is fixed)
struct hs_marg_query { std::vector<int32_t> cols, pn, prhs; };

static int32_t hs_marg_plan(const unsigned char *fx, int N, const int32_t *pairs, int32_t P, hs_marg_query &Q)
{
    if (P < 1 || P > HS_MARG_MAX_PAIRS) SH_FAIL(SLAMHIP_ERR_INVALID, "pose graph marginals: P = %d must lie in [1, 2^20]", P);
    std::vector<int32_t> col_of((size_t)N, -1);
    for (int p = 0; p < P; p++) {
        const int n = pairs[2 * (size_t)p], m = pairs[2 * (size_t)p + 1];
        if (n < 0 || n >= N || m < 0 || m >= N) SH_FAIL(SLAMHIP_ERR_INVALID, "pose graph marginals: pair %d = (%d, %d) of %d nodes", p, n, m, N);
        if (!fx[m]) col_of[(size_t)m] = 0;
    }
    Q.cols.clear();
    for (int n = 0; n < N; n++)
        if (col_of[(size_t)n] == 0) { col_of[(size_t)n] = (int32_t)Q.cols.size(); Q.cols.push_back(n); }
    if (Q.cols.size() > HS_MARG_MAX_COLS) SH_FAIL(SLAMHIP_ERR_INVALID, "pose graph marginals: %zu columns, more than %d", Q.cols.size(), HS_MARG_MAX_COLS);
    Q.pn.resize((size_t)P); Q.prhs.resize((size_t)P);
    for (int p = 0; p < P; p++) {
        const int n = pairs[2 * (size_t)p], m = pairs[2 * (size_t)p + 1];
        Q.pn[(size_t)p] = n;
        Q.prhs[(size_t)p] = fx[n] || fx[m] ? -1 : 3 * col_of[(size_t)m];
    }
    return SLAMHIP_OK;
}

// rule M5's report; false: not one right-hand side fits
static bool hs_marg_info(int C, int N, const slamhip_pg_marg_spec *sp, slamhip_pg_marg_info *I)
{
    const int64_t R = 3 * (int64_t)C, Rc = hs_marg_chunk(R, N, sp);
    memset(I, 0, sizeof(*I));
    I->n_cols = C; I->n_rhs = (int32_t)R; I->rhs_per_chunk = (int32_t)Rc; I->n_chunks = Rc ? (int32_t)((R + Rc - 1) / Rc) : 0;
    I->group = hs_marg_group();
    return R == 0 || Rc > 0;
}

#define K27_LAUNCH(kernel, gx, gy, ...) do { hipLaunchKernelGGL(kernel, dim3((unsigned)(gx), (unsigned)(gy)), dim3(K19_LANES), 0, st, __VA_ARGS__); SH_HIP(hipGetLastError()); } while (0)

// rule T4 for every right-hand side of the chunk: 2 lt + 1 launches
static int32_t hs_marg_solve(const hs_tri_plan &T, const k27_arg &B, int PN, hipStream_t st, int first)
{
    for (int l = 0; l < T.lt; l++) K27_LAUNCH(k27_forward, sh_div_up(T.n[l + 1], K19_LANES), B.Rc, T, B, l, first);
    K27_LAUNCH(k27_solve_tail, B.Rc, 1, T, B, PN, first);
    for (int l = T.lt - 1; l >= 0; l--) K27_LAUNCH(k27_backward, sh_div_up(T.n[l], K19_LANES), B.Rc, T, B, PN, l, first);
    return SLAMHIP_OK;
}

// one PCG iteration of the chunk
template <int G>
static int32_t hs_marg_iteration(const k19_arg &A, const hs_tri_plan &T, const k27_arg &B, hipStream_t st, bool tri, int k, double lambda, double tol)
{
    const int groups = sh_div_up(B.Rc, G);
    K27_LAUNCH(k27_apply<G>, A.PN, groups, A, B, k, lambda, tol);
    if (tri) {
        K27_LAUNCH((k27_step<false, G>), A.PN, groups, A, B, k);
        SH_TRY(hs_marg_solve(T, B, A.PN, st, 0));
    } else {
        K27_LAUNCH((k27_step<true, G>), A.PN, groups, A, B, k);
    }
    K27_LAUNCH(k27_dir<G>, A.PN, groups, A, B, k);
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_pg_marginals(slamhip_hs *hs, const slamhip_pg_marg_spec *spec, const int32_t *pairs, int32_t P, double *out_blocks,
                                           slamhip_pg_marg_col *out_cols, int32_t *out_n_cols, slamhip_pg_marg_info *out_info)
{
    SH_CHECK_ARG(hs && spec && pairs && out_blocks && out_cols && out_n_cols && out_info);
#if K19_SCALAR_LAUNCH
    SH_FAIL(SLAMHIP_ERR_STATE, "K27 is not part of the K19_SCALAR_LAUNCH developer build");
#endif
    SH_TRY(hs_marg_check_spec(spec));
    SH_TRY(hs_pg_need(hs, "pose graph marginals"));
    hs_pg *g = hs->pg;
    const k19_arg &A = g->A;
    hs_marg_query Q;
    SH_TRY(hs_marg_plan(g->fx.data(), A.N, pairs, P, Q));
    const int C = (int)Q.cols.size(), R = 3 * C, G = hs_marg_group();
    const bool tri = spec->precond == 1;
    slamhip_pg_marg_info info;
    if (!hs_marg_info(C, A.N, spec, &info))
        SH_FAIL(SLAMHIP_ERR_NOMEM, "pose graph marginals: max_bytes = %lld holds no right-hand side of %lld bytes", (long long)spec->max_bytes, (long long)hs_marg_rhs_bytes(A.N, spec->precond));
    const size_t np = (size_t)P, blk_bytes = 72 * np, rec_bytes = sizeof(slamhip_pg_marg_col) * (size_t)R;
    if (R == 0) {
        memset(out_blocks, 0, blk_bytes);
        *out_n_cols = 0; *out_info = info;
        return SLAMHIP_OK;
    }
    hipStream_t st = hs->ctx->stream;
    SH_TRY(hs_call_begin(hs));
    if (tri) SH_TRY(hs_tri_blocks(g, "pose graph marginals"));
    // the unit's block: the query, the blocks and the records, then rule M5's work block of R_c right-hand sides
    const size_t Rc = (size_t)info.rhs_per_chunk, n = (size_t)A.N, pn = (size_t)A.PN;
    hs_tri_plan lv;
    const size_t vs = 3 * n, rs = tri ? 3 * ((size_t)hs_tri_levels(A.N, HS_TRI_TAIL, &lv) - n) + 3 : 0;
    size_t o = 0;
    const size_t o_cols = o; o += hs_pg_al(4 * (size_t)C);
    const size_t o_pn = o; o += hs_pg_al(4 * np);
    const size_t o_prhs = o; o += hs_pg_al(4 * np);
    const size_t in_bytes = o;
    const size_t o_blk = o; o += hs_pg_al(blk_bytes);
    const size_t o_rec = o; o += hs_pg_al(rec_bytes);
    size_t o_vec[5];
    for (int v = 0; v < 5; v++) { o_vec[v] = o; o += 8 * vs * Rc; }
    const size_t o_pa = o; o += 8 * pn * Rc;
    const size_t o_pb = o; o += 8 * pn * Rc;
    const size_t o_R = o; o += 8 * rs * Rc;
    const size_t o_st = o; o += sizeof(k27_state) * Rc;
    const size_t o_stop = o; o += 8 * Rc;
    SH_TRY(g->d_marg.grow(o, "pose graph marginals"));
    // the pinned block: the query on its way in; the blocks, the records and the stop words' copy on their way out
    const size_t h_stop_at = hs_pg_al(std::max(in_bytes, blk_bytes + rec_bytes));
    SH_TRY(g->h_io.grow(h_stop_at + 4 * Rc, "pose graph marginals"));
    unsigned char *h = g->h_io, *d = g->d_marg;
    memcpy(h + o_cols, Q.cols.data(), 4 * (size_t)C);
    memcpy(h + o_pn, Q.pn.data(), 4 * np);
    memcpy(h + o_prhs, Q.prhs.data(), 4 * np);
    SH_HIP(hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, st));
    SH_HIP(hipMemsetAsync(d + o_blk, 0, blk_bytes, st));                   // (rule M3's +0 blocks)
    k27_arg B;
    B.P = P; B.vs = vs; B.rs = rs;
    B.cols = (const int32_t *)(d + o_cols); B.pn = (const int32_t *)(d + o_pn); B.prhs = (const int32_t *)(d + o_prhs);
    B.x = (double *)(d + o_vec[0]); B.res = (double *)(d + o_vec[1]); B.zv = (double *)(d + o_vec[2]); B.p = (double *)(d + o_vec[3]); B.q = (double *)(d + o_vec[4]);
    B.part_a = (double *)(d + o_pa); B.part_b = (double *)(d + o_pb); B.R = (double *)(d + o_R);
    B.st = (k27_state *)(d + o_st); B.stop = (int32_t *)(d + o_stop);
    B.blocks = (double *)(d + o_blk); B.recs = (slamhip_pg_marg_col *)(d + o_rec);
    // the linearisation and the preconditioner, once
    K19_LAUNCH(k19_linearise, A.PE, A);
    if (tri) SH_TRY(hs_tri_factor(A, g->T, st, spec->lambda, 0));
    else K19_LAUNCH(k19_diag, A.PN, A, spec->lambda);
    const int32_t *h_stop = (const int32_t *)(h + h_stop_at);
    for (int r0 = 0; r0 < R; r0 += (int)Rc) {
        B.r0 = r0; B.Rc = std::min((int)Rc, R - r0);
        if (tri) {
            K27_LAUNCH(k27_begin<false>, A.PN, B.Rc, A, B);
            SH_TRY(hs_marg_solve(g->T, B, A.PN, st, 1));                   // rule 7's start: z = T^-1 e, p = z, the block sums of res . z
        } else {
            K27_LAUNCH(k27_begin<true>, A.PN, B.Rc, A, B);
        }
        K27_LAUNCH(k27_begin_state, B.Rc, 1, A, B);
        auto iteration = [&](int k) -> int32_t {
            return G == HS_MARG_GROUP ? hs_marg_iteration<HS_MARG_GROUP>(A, g->T, B, st, tri, k, spec->lambda, spec->tol)
                                      : hs_marg_iteration<HS_MARG_GROUP_WIDE>(A, g->T, B, st, tri, k, spec->lambda, spec->tol);
        };
        auto all_stopped = [&]() {
            for (int j = 0; j < B.Rc; j++) if (!h_stop[j]) return false;
            return true;
        };
        SH_TRY(hs_pg_pcg_loop(hs, spec->n_cg, spec->check_every, B.stop, h + h_stop_at, 4 * (size_t)B.Rc, iteration, all_stopped));
        K27_LAUNCH(k27_collect, sh_div_up((int)std::max<size_t>(9 * np, (size_t)B.Rc), K19_LANES), 1, B, spec->tol);
    }
    SH_HIP(hipMemcpyAsync(h, d + o_blk, blk_bytes, hipMemcpyDeviceToHost, st));
    SH_HIP(hipMemcpyAsync(h + blk_bytes, d + o_rec, rec_bytes, hipMemcpyDeviceToHost, st));
    SH_TRY(hs_call_finish(hs));
    memcpy(out_blocks, h, blk_bytes);
    memcpy(out_cols, h + blk_bytes, rec_bytes);
    *out_n_cols = R; *out_info = info;
    return SLAMHIP_OK;
}

// ---- CPU-side test hook: the unit's host definition (hs_pg_host_sys, hs_pg_host_pcg) with rule 7's start replaced ------------------------
extern "C" int32_t slamhip_debug_pg_marginals(const double *poses, const uint8_t *fixed, int32_t N, const int32_t *ij, const double *z, const double *w, int32_t E,
                                              const slamhip_pg_marg_spec *spec, const int32_t *pairs, int32_t P, double *out_blocks,
                                              slamhip_pg_marg_col *out_cols, int32_t *out_n_cols, slamhip_pg_marg_info *out_info)
{
    SH_CHECK_ARG(spec && pairs && out_blocks && out_cols && out_n_cols && out_info);
    SH_TRY(hs_marg_check_spec(spec));
    SH_TRY(hs_pg_check_graph(poses, fixed, N, ij, z, w, E));
    hs_pg_host_sys S;
    hs_pg_host_sys_init(S, spec->precond == 1, fixed, N, ij, E);
    const hs_pg_host_lists &G = S.G;
    hs_marg_query Q;
    SH_TRY(hs_marg_plan(G.fx.data(), N, pairs, P, Q));
    const int C = (int)Q.cols.size(), R = 3 * C;
    slamhip_pg_marg_info info;
    if (!hs_marg_info(C, N, spec, &info))
        SH_FAIL(SLAMHIP_ERR_NOMEM, "pose graph marginals: max_bytes = %lld holds no right-hand side of %lld bytes", (long long)spec->max_bytes, (long long)hs_marg_rhs_bytes(N, spec->precond));
    memset(out_blocks, 0, 72 * (size_t)P);
    std::vector<std::vector<int32_t>> of_col((size_t)C);                   // the pairs that read a column
    for (int p = 0; p < P; p++)
        if (Q.prhs[(size_t)p] >= 0) of_col[(size_t)(Q.prhs[(size_t)p] / 3)].push_back(p);
    if (R) (void)hs_pg_host_sys_linearise(S, poses, z, w, spec->lambda);
    const bool one[1] = { true };
    auto apply = [&](int n, const double *p, double *qn) {
        hs_marg_node_apply<1>(S.lambda, p, 0, one, n, G.off.data(), G.inc.data(), S.rec.data(), ij, (double (*)[3])qn);
    };
    for (int rhs = 0; rhs < R; rhs++) {
        const int c = rhs / 3, b = rhs % 3, m = Q.cols[(size_t)c];
        for (double &v : S.res) v = 0.0;
        S.res[3 * (size_t)m + b] = 1.0;
        slamhip_pg_iter I;
        hs_pg_host_pcg(S, spec->n_cg, spec->tol, apply, &I);
        slamhip_pg_marg_col K;
        K.rz0 = I.rz0; K.rz = I.rz; K.cg_iters = I.cg_iters; K.stopped = I.stopped; K.node = m; K.comp = b;
        out_cols[rhs] = K;
        for (int32_t p : of_col[(size_t)c])
            for (int a = 0; a < 3; a++) out_blocks[9 * (size_t)p + 3 * a + b] = S.x[3 * (size_t)Q.pn[(size_t)p] + a];
    }
    *out_n_cols = R; *out_info = info;
    return SLAMHIP_OK;
}
