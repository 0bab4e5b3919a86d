// hs_pg_tri.inc -- K22, the odometry-chain preconditioner of the pose-graph relaxation: PCG with z = T^-1 res, T the block-tridiagonal
// part of H, factorised and solved by block cyclic reduction (slamhip_hs_pg_relax_tri, _pg_tri_apply, slamhip_debug_pg_relax_tri,
// _pg_tri_apply).  The second part of hs_pg.hip's translation unit: it launches k19_linearise, k19_begin, k19_apply, k19_step<false>,
// k19_dir and k19_update as they are and shares their device helpers.  Definition: include/slamhip.h, rules T1 - T5; the arithmetic
// host and device share: hs_pg_tri.h, the per-node loop of rule T2 and rule T3's choice of neighbours included.  Behind K22's launch
// functions stand the unit's enqueue loop, PCG driver and relax call (hs_pg_pcg_loop, hs_pg_pcg, hs_pg_relax_run), behind its host text
// the unit's host definition (hs_pg_host_sys, hs_pg_host_pcg, hs_pg_host_relax): K19, K22 and K26 all go through them, with the
// preconditioner as an argument, and K27 (hs_pg_marg.inc) through the loop and the host PCG.
//  * k22_diag: a lane per node, rule 4's D_n and g_n over the node's list, rule T1, P = D^-1; for PCG x = 0 and res = -g.
//  * k22_coupling: a lane per node, rule T2 over the same list.
//  * k22_reduce: one launch per level with more than S blocks, a lane per block of the NEXT level, rule T3.
//  * k22_factor_tail: ONE workgroup, every level from the first with at most S blocks on, a barrier between levels.
//  * k22_forward / k22_backward: one launch per level with more than S blocks, rule T4; level 0's k22_backward stores z and the block
//    sums of res . z.
//  * k22_solve_tail: ONE workgroup: forward, last level and backward of every level with at most S blocks, the right-hand sides in LDS;
//    with N <= S it is the whole application, z and the block sums included.
// In PCG every k22 launch reads the stop word once per workgroup and leaves behind a stop, as K19's do.  No kernel waits on another
// workgroup.

static_assert(3 * (2 * HS_TRI_TAIL + 32) * sizeof(double) + (K19_LANES + 64) * sizeof(double) + 64 <= 65536, "the tail's LDS");

__global__ void __launch_bounds__(K19_LANES) k22_diag(const k19_arg A, const hs_tri_plan T, double lambda, int start)
{
    const int n = (int)blockIdx.x * K19_LANES + (int)threadIdx.x;
    if (n >= A.N) return;
    double D[6], g[3] = { 0.0, 0.0, 0.0 }, P[6];
    bool live = false;
    if (!A.fixed[n]) {
        hs_pg_node_diag(lambda, n, A.off, A.inc, A.rec, A.r, D, g);
        live = hs_pg_inv(D, P);
    }
    if (!live) {                                                           // rule T1: the identity, and g = 0 (fixed, or no edge at all)
        D[0] = D[3] = D[5] = 1.0; D[1] = D[2] = D[4] = 0.0;
        for (int m = 0; m < 6; m++) P[m] = D[m];
    }
    hs_tri_store(T.D, (size_t)n, 6, D); hs_tri_store(T.P, (size_t)n, 6, P);
    T.live[n] = live ? 1 : 0;
    if (start) {
        const double x[3] = { 0.0, 0.0, 0.0 }, res[3] = { -g[0], -g[1], -g[2] };
        k19_store3(A.x, n, x); k19_store3(A.res, n, res);
    }
}

__global__ void __launch_bounds__(K19_LANES) k22_coupling(const k19_arg A, const hs_tri_plan T)
{
    const int n = (int)blockIdx.x * K19_LANES + (int)threadIdx.x;
    if (n >= A.N) return;
    double U[9];
    hs_tri_node_coupling(n, A.N, T.live, A.off, A.inc, A.rec, (const int32_t *)A.ij, U);
    hs_tri_store(T.U, (size_t)n, 9, U);
}

__global__ void __launch_bounds__(K19_LANES) k22_reduce(const hs_tri_plan T, int l)
{
    const int m = (int)blockIdx.x * K19_LANES + (int)threadIdx.x;
    if (m < T.n[l + 1]) hs_tri_reduce_block(T, l, m);
}

// one workgroup: levels lt + 1 .. L - 1 (what a level reads, the level before has stored ahead of the barrier)
__global__ void __launch_bounds__(K19_LANES) k22_factor_tail(const hs_tri_plan T)
{
    for (int l = T.lt; l + 1 < T.L; l++) {
        for (int m = (int)threadIdx.x; m < T.n[l + 1]; m += K19_LANES) hs_tri_reduce_block(T, l, m);
        __threadfence_block();
        __syncthreads();
    }
}

// what one application reads and writes at level 0: the right-hand side r0, z into z0 (and z1, if given: rule 7's p = z); part:
// the block sums of r0 . z (nullptr: none); st: the stop word to leave behind (nullptr: not inside PCG)
struct k22_io { const double *r0; double *z0, *z1, *part; const k19_state *st; };

__device__ static inline const double *k22_rhs(const hs_tri_plan &T, const k22_io &io, int l) { return l ? T.R + 3 * ((size_t)T.off[l] - (size_t)T.n[0]) : io.r0; }

__global__ void __launch_bounds__(K19_LANES) k22_forward(const hs_tri_plan T, const k22_io io, int l)
{
    __shared__ int stop_s;
    if (io.st && k19_stopped(io.st, &stop_s)) return;
    const int m = (int)blockIdx.x * K19_LANES + (int)threadIdx.x;
    if (m >= T.n[l + 1]) return;
    double out[3];
    hs_tri_forward(k22_rhs(T, io, l), T.U + 9 * (size_t)T.off[l], T.P + 6 * (size_t)T.off[l], T.n[l], m, out);
    k19_store3(T.R + 3 * ((size_t)T.off[l + 1] - (size_t)T.n[0]), m, out);
}

// level 0's z of node k (rule T1: 0 for a dead node), stored; its term of res . z
__device__ static inline double k22_finish(const hs_tri_plan &T, const k22_io &io, int k, double z[3])
{
    if (!T.live[k]) z[0] = z[1] = z[2] = 0.0;
    k19_store3(io.z0, k, z);
    if (io.z1) k19_store3(io.z1, k, z);
    double r[3];
    k19_load3(io.r0, k, r);
    return hs_pg_dot3(r, z);
}

__global__ void __launch_bounds__(K19_LANES) k22_backward(const hs_tri_plan T, const k22_io io, int l)
{
    __shared__ double lds[K19_LANES];
    __shared__ int stop_s;
    if (io.st && k19_stopped(io.st, &stop_s)) return;
    const int k = (int)blockIdx.x * K19_LANES + (int)threadIdx.x;
    double term = 0.0;
    if (k < T.n[l]) {
        double z[3];
        const double *rl = k22_rhs(T, io, l);
        hs_tri_backward(rl, k22_rhs(T, io, l + 1), T.U + 9 * (size_t)T.off[l], T.P + 6 * (size_t)T.off[l], T.n[l], k, z);
        if (l) k19_store3(const_cast<double *>(rl), k, z);                 // (in place: a lane reads its own block's right-hand side alone)
        else term = k22_finish(T, io, k, z);
    }
    if (l == 0 && io.part) {
        const double sum = k19_block_sum(term, lds);
        if (threadIdx.x == 0) io.part[blockIdx.x] = sum;
    }
}

// one workgroup: levels lt .. L - 1 of one application
__global__ void __launch_bounds__(K19_LANES) k22_solve_tail(const hs_tri_plan T, const k22_io io)
{
    __shared__ double sr[3 * (2 * HS_TRI_TAIL + 32)];
    __shared__ double lds[K19_LANES];
    __shared__ int stop_s;
    if (io.st && k19_stopped(io.st, &stop_s)) return;
    const int tid = (int)threadIdx.x, lt = T.lt, base = T.off[lt];
    const double *r = k22_rhs(T, io, lt);
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
        double *zl = const_cast<double *>(r);
        for (int i = tid; i < 3 * T.n[lt]; i += K19_LANES) zl[i] = sr[i];
        return;
    }
    const int chunks = (T.n[0] + K19_LANES - 1) / K19_LANES;               // level 0: z, and rule 6's blocks of 256 nodes
    for (int c = 0; c < chunks; c++) {
        const int k = c * K19_LANES + tid;
        double term = 0.0;
        if (k < T.n[0]) {
            double z[3] = { sr[3 * k], sr[3 * k + 1], sr[3 * k + 2] };
            term = k22_finish(T, io, k, z);
        }
        if (io.part) {
            const double sum = k19_block_sum(term, lds);
            if (tid == 0) io.part[c] = sum;
        }
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------
// the developer's S (tests drive small graphs through several global levels with it); no result depends on it
static int hs_tri_tail_blocks()
{
    return (int)std::min<long long>(std::max<long long>(sh_env_int("SLAMHIP_K22_TAIL", HS_TRI_TAIL), 1), HS_TRI_TAIL);
}

// the levels' blocks, made on first use and grown with N; after SLAMHIP_ERR_NOMEM the graph is as it was
static int32_t hs_tri_blocks(hs_pg *g, const char *who)
{
    hs_tri_plan &T = g->T;
    const size_t tot = (size_t)hs_tri_levels(g->A.N, hs_tri_tail_blocks(), &T), n = (size_t)g->A.N;
    size_t o = 0;
    const size_t o_D = o; o += hs_pg_al(48 * tot);
    const size_t o_P = o; o += hs_pg_al(48 * tot);
    const size_t o_U = o; o += hs_pg_al(72 * tot);
    const size_t o_R = o; o += hs_pg_al(24 * (tot - n) + 24);
    const size_t o_live = o; o += hs_pg_al(n);
    SH_TRY(g->d_tri.grow(o, who));
    unsigned char *d = g->d_tri;
    T.D = (double *)(d + o_D); T.P = (double *)(d + o_P); T.U = (double *)(d + o_U); T.R = (double *)(d + o_R); T.live = d + o_live;
    return SLAMHIP_OK;
}

// rules T1 - T3 at the poses as they stand (k19_linearise has run)
static int32_t hs_tri_factor(const k19_arg &A, const hs_tri_plan &T, hipStream_t st, double lambda, int start)
{
    K19_LAUNCH(k22_diag, A.PN, A, T, lambda, start);
    K19_LAUNCH(k22_coupling, A.PN, A, T);
    for (int l = 0; l < T.lt; l++) K19_LAUNCH(k22_reduce, sh_div_up(T.n[l + 1], K19_LANES), T, l);
    if (T.lt + 1 < T.L) K19_LAUNCH(k22_factor_tail, 1, T);
    return SLAMHIP_OK;
}

// rule T4: 2 lt + 1 launches
static int32_t hs_tri_solve(hs_pg *g, hipStream_t st, const k22_io &io)
{
    const hs_tri_plan &T = g->T;
    for (int l = 0; l < T.lt; l++) K19_LAUNCH(k22_forward, sh_div_up(T.n[l + 1], K19_LANES), T, io, l);
    K19_LAUNCH(k22_solve_tail, 1, T, io);
    for (int l = T.lt - 1; l >= 0; l--) K19_LAUNCH(k22_backward, sh_div_up(T.n[l], K19_LANES), T, io, l);
    return SLAMHIP_OK;
}

// The unit's ONE enqueue loop: batches of check_every PCG iterations (iteration(k) enqueues one), the stop words -- stop_bytes at
// d_stop -- read back into h_stop (pinned) in one copy between them, until all_stopped() says so or n_cg is reached.  K19, K22 and K26
// run it over one right-hand side (hs_pg_pcg), K27 over a chunk of them (hs_pg_marg.inc).
template <class Iteration, class AllStopped>
static int32_t hs_pg_pcg_loop(slamhip_hs *hs, int n_cg, int check_every, const void *d_stop, void *h_stop, size_t stop_bytes, Iteration iteration, AllStopped all_stopped)
{
    for (int k = 0; k < n_cg;) {
        const int k1 = (int)std::min<int64_t>((int64_t)k + std::min(check_every, K19_MAX_BATCH), n_cg);
        for (; k < k1; k++) SH_TRY(iteration(k));
        SH_HIP(hipMemcpyAsync(h_stop, d_stop, stop_bytes, hipMemcpyDeviceToHost, hs->ctx->stream));
        SH_TRY(hs_call_finish(hs));                                        // (the stop words, between batches)
        if (all_stopped()) break;
    }
    return SLAMHIP_OK;
}

// The unit's PCG driver for one right-hand side: rules 4 - 7 (tri: T1 - T5) up to the pose update, over A's weights at the
// linearisation k19_linearise has left.
static int32_t hs_pg_pcg(slamhip_hs *hs, hs_pg *g, const k19_arg &A, bool tri, double lambda, int n_cg, int check_every, double tol, k19_state *h_st)
{
    hipStream_t st = hs->ctx->stream;
    const k22_io first = { A.res, A.zv, A.p, A.part_b, nullptr }, io = { A.res, A.zv, nullptr, A.part_b, A.st };
    if (tri) {
        SH_TRY(hs_tri_factor(A, g->T, st, lambda, 1));
        SH_TRY(hs_tri_solve(g, st, first));                                // rule 7's start: z = T^-1 res, p = z, the block sums of res . z
    } else {
        K19_LAUNCH(k19_diag, A.PN, A, lambda);
    }
    K19_LAUNCH(k19_begin, 1, A, 0);
    auto iteration = [&](int k) -> int32_t {
        K19_LAUNCH(k19_apply, A.PN, A, k, lambda, tol);
#if K19_SCALAR_LAUNCH
        K19_LAUNCH(k19_scal_a, 1, A, k);
#endif
        if (tri) {
            K19_LAUNCH(k19_step<false>, A.PN, A, k);
            SH_TRY(hs_tri_solve(g, st, io));
        } else {
            K19_LAUNCH(k19_step<true>, A.PN, A, k);
        }
#if K19_SCALAR_LAUNCH
        K19_LAUNCH(k19_scal_b, 1, A, k);
#endif
        K19_LAUNCH(k19_dir, A.PN, A, k);
        return SLAMHIP_OK;
    };
    return hs_pg_pcg_loop(hs, n_cg, check_every, A.st, h_st, sizeof(k19_state), iteration, [&]() { return h_st->stop != 0; });
}

static int32_t hs_pg_relax_run(slamhip_hs *hs, const slamhip_pg_spec *spec, bool tri, const char *who, slamhip_pg_iter *out_iters, double *out_chi2_final)
{
    SH_TRY(hs_pg_check_spec(spec));
    SH_TRY(hs_pg_need(hs, who));
    hs_pg *g = hs->pg;
    const k19_arg &A = g->A;
    hipStream_t st = hs->ctx->stream;
    SH_TRY(hs_call_begin(hs));
    if (tri) SH_TRY(hs_tri_blocks(g, who));
    // the pinned block: the records, the final chi2, the stop word's copy
    const size_t out_bytes = sizeof(slamhip_pg_iter) * (size_t)spec->n_outer;
    SH_TRY(g->h_io.grow(out_bytes + 8 + sizeof(k19_state), who));
    k19_state *h_st = (k19_state *)(g->h_io + out_bytes + 8);
    for (int outer = 0; outer < spec->n_outer; outer++) {
        K19_LAUNCH(k19_linearise, A.PE, A);
        SH_TRY(hs_pg_pcg(hs, g, A, tri, spec->lambda, spec->n_cg, spec->check_every, spec->tol, h_st));
        K19_LAUNCH(k19_update, A.PN, A, spec->tol, outer);
    }
    K19_LAUNCH(k19_linearise, A.PE, A);
    K19_LAUNCH(k19_begin, 1, A, 1);
    SH_HIP(hipMemcpyAsync(g->h_io, A.iters, out_bytes, hipMemcpyDeviceToHost, st));
    SH_HIP(hipMemcpyAsync(g->h_io + out_bytes, A.final_chi2, 8, hipMemcpyDeviceToHost, st));
    SH_TRY(hs_call_finish(hs));
    memcpy(out_iters, g->h_io, out_bytes);
    memcpy(out_chi2_final, g->h_io + out_bytes, 8);
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_pg_relax_tri(slamhip_hs *hs, const slamhip_pg_spec *spec, slamhip_pg_iter *out_iters, double *out_chi2_final)
{
    SH_CHECK_ARG(hs && spec && out_iters && out_chi2_final);
#if K19_SCALAR_LAUNCH
    SH_FAIL(SLAMHIP_ERR_STATE, "K22 is not part of the K19_SCALAR_LAUNCH developer build");
#endif
    return hs_pg_relax_run(hs, spec, true, "pose graph relax (tri)", out_iters, out_chi2_final);
}

extern "C" int32_t slamhip_hs_pg_tri_apply(slamhip_hs *hs, double lambda, const double *rhs, double *out)
{
    SH_CHECK_ARG(hs && rhs && out);
#if K19_SCALAR_LAUNCH
    SH_FAIL(SLAMHIP_ERR_STATE, "K22 is not part of the K19_SCALAR_LAUNCH developer build");
#endif
    if (!isfinite(lambda) || !(lambda >= 0.0)) SH_FAIL(SLAMHIP_ERR_INVALID, "pose graph tri apply: lambda = %g must be finite and >= 0", lambda);
    SH_TRY(hs_pg_need(hs, "pose graph tri apply"));
    hs_pg *g = hs->pg;
    const k19_arg &A = g->A;
    hipStream_t st = hs->ctx->stream;
    SH_TRY(hs_call_begin(hs));
    SH_TRY(hs_tri_blocks(g, "pose graph tri apply"));
    const size_t bytes = 24 * (size_t)A.N;
    SH_TRY(g->h_io.grow(bytes, "pose graph tri apply"));
    memcpy(g->h_io, rhs, bytes);
    SH_HIP(hipMemcpyAsync(A.res, g->h_io, bytes, hipMemcpyHostToDevice, st));   // (the PCG vectors are free between two calls)
    K19_LAUNCH(k19_linearise, A.PE, A);
    SH_TRY(hs_tri_factor(A, g->T, st, lambda, 0));
    const k22_io io = { A.res, A.zv, nullptr, nullptr, nullptr };
    SH_TRY(hs_tri_solve(g, st, io));
    SH_HIP(hipMemcpyAsync(g->h_io, A.zv, bytes, hipMemcpyDeviceToHost, st));
    SH_TRY(hs_call_finish(hs));
    memcpy(out, g->h_io, bytes);
    return SLAMHIP_OK;
}

// ---- CPU-side test hooks: hs_pg_tri.h -- the text the kernels run -- in plain loops ----------------------------------------------------
struct hs_tri_host {
    hs_tri_plan T;
    std::vector<double> D, P, U, R;
    std::vector<unsigned char> live;
};

static void hs_tri_host_init(hs_tri_host &H, int N)
{
    const size_t tot = (size_t)hs_tri_levels(N, HS_TRI_TAIL, &H.T);
    H.D.assign(6 * tot, 0.0); H.P.assign(6 * tot, 0.0); H.U.assign(9 * tot, 0.0); H.R.assign(3 * (tot - (size_t)N) + 3, 0.0);
    H.live.assign((size_t)N, 0);
    H.T.D = H.D.data(); H.T.P = H.P.data(); H.T.U = H.U.data(); H.T.R = H.R.data(); H.T.live = H.live.data();
}

// rules T1 - T3; g (N x 3, or nullptr): rule 4's g_n beside them
static void hs_tri_host_factor(hs_tri_host &H, const hs_pg_host_lists &G, int N, const int32_t *ij, const hs_pg_rec *rec, const double *r, double lambda, double *g_out)
{
    const hs_tri_plan &T = H.T;
    for (int n = 0; n < N; n++) {
        double D[6], g[3] = { 0.0, 0.0, 0.0 }, P[6];
        bool live = false;
        if (!G.fx[(size_t)n]) {
            hs_pg_node_diag(lambda, n, G.off.data(), G.inc.data(), rec, r, D, g);
            live = hs_pg_inv(D, P);
        }
        if (!live) {
            D[0] = D[3] = D[5] = 1.0; D[1] = D[2] = D[4] = 0.0;
            for (int m = 0; m < 6; m++) P[m] = D[m];
        }
        hs_tri_store(T.D, (size_t)n, 6, D); hs_tri_store(T.P, (size_t)n, 6, P);
        T.live[n] = live ? 1 : 0;
        if (g_out) for (int a = 0; a < 3; a++) g_out[3 * (size_t)n + a] = g[a];
    }
    for (int n = 0; n < N; n++) hs_tri_node_coupling(n, N, T.live, G.off.data(), G.inc.data(), rec, ij, T.U + 9 * (size_t)n);
    for (int l = 0; l + 1 < T.L; l++)
        for (int m = 0; m < T.n[l + 1]; m++) hs_tri_reduce_block(T, l, m);
}

// rule T4: z = T^-1 r0
static void hs_tri_host_solve(hs_tri_host &H, const double *r0, double *z0)
{
    const hs_tri_plan &T = H.T;
    const size_t N = (size_t)T.n[0];
    auto rhs = [&](int l) -> double * { return l ? T.R + 3 * ((size_t)T.off[l] - N) : const_cast<double *>(r0); };
    for (int l = 0; l + 1 < T.L; l++)
        for (int m = 0; m < T.n[l + 1]; m++) hs_tri_forward(rhs(l), T.U + 9 * (size_t)T.off[l], T.P + 6 * (size_t)T.off[l], T.n[l], m, rhs(l + 1) + 3 * (size_t)m);
    {
        double z[3], *rl = T.L > 1 ? rhs(T.L - 1) : z0;
        hs_pg_mul(T.P + 6 * (size_t)T.off[T.L - 1], rhs(T.L - 1), z);
        for (int a = 0; a < 3; a++) rl[a] = z[a];
    }
    for (int l = T.L - 2; l >= 0; l--)
        for (int k = 0; k < T.n[l]; k++) {
            double z[3], *out = l ? rhs(l) + 3 * (size_t)k : z0 + 3 * (size_t)k;
            hs_tri_backward(rhs(l), rhs(l + 1), T.U + 9 * (size_t)T.off[l], T.P + 6 * (size_t)T.off[l], T.n[l], k, z);
            for (int a = 0; a < 3; a++) out[a] = z[a];
        }
    for (size_t n = 0; n < N; n++)
        if (!T.live[n]) z0[3 * n] = z0[3 * n + 1] = z0[3 * n + 2] = 0.0;
}

// The definition of K19 (block-Jacobi) and of K22 (tri) over a graph and a spec that have been checked; K26's hook takes single steps
// through it, with its own weights.  tri is read where the preconditioner is made and where z is formed from res, nowhere else.
// what the host definition keeps of a graph: the lists, one linearisation with its preconditioner, and PCG's vectors
struct hs_pg_host_sys {
    bool tri; int N, E; const int32_t *ij; double lambda;
    hs_pg_host_lists G;
    hs_tri_host H;
    std::vector<hs_pg_rec> rec;
    std::vector<double> r, tmp, M, g, x, res, zv, p, q;
};

static void hs_pg_host_sys_init(hs_pg_host_sys &S, bool tri, const uint8_t *fixed, int N, const int32_t *ij, int E)
{
    const size_t n3 = 3 * (size_t)N;
    S.tri = tri; S.N = N; S.E = E; S.ij = ij; S.lambda = 0.0;
    hs_pg_host_lists_init(S.G, fixed, N, ij, E);
    if (tri) hs_tri_host_init(S.H, N);
    S.rec.resize((size_t)E + 1);
    S.r.resize(3 * (size_t)E + 3); S.tmp.resize((size_t)std::max(N, E) + HS_PG_BLOCK); S.M.resize(tri ? 0 : 6 * (size_t)N);
    for (std::vector<double> *v : { &S.g, &S.x, &S.res, &S.zv, &S.p, &S.q }) v->resize(n3);
}

// rules 3 and 4 (tri: T1 - T3) at the poses: the records, chi2 (returned), g and the preconditioner for this lambda
static double hs_pg_host_sys_linearise(hs_pg_host_sys &S, const double *poses, const double *z, const double *w, double lambda)
{
    const hs_pg_host_lists &G = S.G;
    S.lambda = lambda;
    const double chi2 = hs_pg_host_linearise(poses, S.ij, z, w, S.E, S.rec.data(), S.r.data(), S.tmp.data());
    if (S.tri) hs_tri_host_factor(S.H, G, S.N, S.ij, S.rec.data(), S.r.data(), lambda, S.g.data());
    else for (int n = 0; n < S.N; n++) {                                   // rule 4: M = 0 and g = 0 for a fixed node
        double D[6], *gn = S.g.data() + 3 * (size_t)n, *Mn = S.M.data() + 6 * (size_t)n;
        gn[0] = gn[1] = gn[2] = 0.0;
        for (int m = 0; m < 6; m++) Mn[m] = 0.0;
        if (G.fx[(size_t)n]) continue;
        hs_pg_node_diag(lambda, n, G.off.data(), G.inc.data(), S.rec.data(), S.r.data(), D, gn);
        (void)hs_pg_inv(D, Mn);
    }
    return chi2;
}

// THE PCG of the host definition, rule 7 from "z = M res" on: the caller has put rule 7's right-hand side into S.res; x is left in
// S.x and rz0, rz, cg_iters and stopped in *I.  apply(n, p, q_n) is rule 5 for the free node n.  S.tri is read where z is formed from
// res, nowhere else.
template <class Apply>
static void hs_pg_host_pcg(hs_pg_host_sys &S, int n_cg, double tol, Apply apply, slamhip_pg_iter *I)
{
    const int N = S.N;
    const size_t n3 = 3 * (size_t)N;
    std::vector<double> &x = S.x, &res = S.res, &zv = S.zv, &p = S.p, &q = S.q, &tmp = S.tmp;
    auto precondition = [&]() {                                            // z from res
        if (S.tri) hs_tri_host_solve(S.H, res.data(), zv.data());
        else for (int n = 0; n < N; n++) hs_pg_mul(S.M.data() + 6 * (size_t)n, res.data() + 3 * (size_t)n, zv.data() + 3 * (size_t)n);
    };
    for (size_t i = 0; i < n3; i++) x[i] = 0.0;
    precondition();
    p = zv;
    double rz = hs_pg_host_dot(res.data(), zv.data(), N, tmp.data());
    I->rz0 = rz;
    int k = 0, stopped;
    for (;; k++) {
        if (hs_pg_converged(rz, I->rz0, tol)) { stopped = HS_PG_STOP_TOL; break; }
        if (k == n_cg) { stopped = HS_PG_STOP_NCG; break; }
        for (int n = 0; n < N; n++) {                                      // rule 5: q = 0 for a fixed node
            double *qn = q.data() + 3 * (size_t)n;
            qn[0] = qn[1] = qn[2] = 0.0;
            if (!S.G.fx[(size_t)n]) apply(n, p.data(), qn);
        }
        const double pq = hs_pg_host_dot(p.data(), q.data(), N, tmp.data());
        if (hs_pg_breakdown(pq)) { stopped = HS_PG_STOP_BREAKDOWN; break; }
        const double alpha = rz / pq;
        for (size_t i = 0; i < n3; i++) { x[i] = x[i] + alpha * p[i]; res[i] = res[i] - alpha * q[i]; }
        precondition();
        const double rzn = hs_pg_host_dot(res.data(), zv.data(), N, tmp.data());
        const double beta = rzn / rz;
        for (size_t i = 0; i < n3; i++) p[i] = zv[i] + beta * p[i];
        rz = rzn;
    }
    I->rz = rz; I->cg_iters = k; I->stopped = stopped;
}

static void hs_pg_host_relax(bool tri, double *poses, const uint8_t *fixed, int32_t N, const int32_t *ij, const double *z, const double *w, int32_t E,
                             const slamhip_pg_spec *spec, slamhip_pg_iter *out_iters, double *out_chi2_final, double *out_r, double *out_chi2)
{
    const size_t n3 = 3 * (size_t)N;
    hs_pg_host_sys S;
    hs_pg_host_sys_init(S, tri, fixed, N, ij, E);
    const hs_pg_host_lists &G = S.G;
    auto apply = [&](int n, const double *p, double *qn) { hs_pg_node_apply(S.lambda, p, n, G.off.data(), G.inc.data(), S.rec.data(), ij, qn); };
    for (int outer = 0; outer < spec->n_outer; outer++) {
        slamhip_pg_iter I;
        I.chi2 = hs_pg_host_sys_linearise(S, poses, z, w, spec->lambda);
        for (size_t i = 0; i < n3; i++) S.res[i] = -S.g[i];                // rule 7's start
        hs_pg_host_pcg(S, spec->n_cg, spec->tol, apply, &I);
        out_iters[outer] = I;
        for (int n = 0; n < N; n++)
            if (!G.fx[(size_t)n]) hs_pg_add_pose(poses + 3 * (size_t)n, S.x.data() + 3 * (size_t)n);
    }
    *out_chi2_final = hs_pg_host_linearise(poses, ij, z, w, E, S.rec.data(), S.r.data(), S.tmp.data());
    if (out_r && E) memcpy(out_r, S.r.data(), 24 * (size_t)E);
    if (out_chi2) for (int e = 0; e < E; e++) out_chi2[e] = S.rec[(size_t)e].chi2;
}

extern "C" int32_t slamhip_debug_pg_relax_tri(double *poses, const uint8_t *fixed, int32_t N, const int32_t *ij, const double *z, const double *w, int32_t E,
                                              const slamhip_pg_spec *spec, slamhip_pg_iter *out_iters, double *out_chi2_final, double *out_r, double *out_chi2)
{
    SH_CHECK_ARG(spec && out_iters && out_chi2_final);
    SH_TRY(hs_pg_check_spec(spec));
    SH_TRY(hs_pg_check_graph(poses, fixed, N, ij, z, w, E));
    hs_pg_host_relax(true, poses, fixed, N, ij, z, w, E, spec, out_iters, out_chi2_final, out_r, out_chi2);
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_debug_pg_tri_apply(const double *poses, const uint8_t *fixed, int32_t N, const int32_t *ij, const double *z, const double *w, int32_t E,
                                              double lambda, const double *rhs, double *out)
{
    SH_CHECK_ARG(rhs && out);
    if (!isfinite(lambda) || !(lambda >= 0.0)) SH_FAIL(SLAMHIP_ERR_INVALID, "pose graph tri apply: lambda = %g must be finite and >= 0", lambda);
    SH_TRY(hs_pg_check_graph(poses, fixed, N, ij, z, w, E));
    hs_pg_host_lists G;
    hs_pg_host_lists_init(G, fixed, N, ij, E);
    hs_tri_host H;
    hs_tri_host_init(H, N);
    std::vector<hs_pg_rec> rec((size_t)E + 1);
    std::vector<double> r(3 * (size_t)E + 3), tmp((size_t)E + HS_PG_BLOCK);
    (void)hs_pg_host_linearise(poses, ij, z, w, E, rec.data(), r.data(), tmp.data());
    hs_tri_host_factor(H, G, N, ij, rec.data(), r.data(), lambda, nullptr);
    hs_tri_host_solve(H, rhs, out);
    return SLAMHIP_OK;
}
