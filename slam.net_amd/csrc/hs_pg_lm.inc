// hs_pg_lm.inc -- K26, the damped (Levenberg-Marquardt) and robust relaxation of the pose graph: every step of K19 / K22 becomes an
// ATTEMPT that is taken only if it lowers the cost, lambda moves with the outcome, and an edge's weight is scaled by a rational robust
// factor (slamhip_hs_pg_relax_lm, slamhip_debug_pg_relax_lm).  The last part of hs_pg.hip's translation unit: an attempt's PCG is the
// unit's driver (hs_pg_pcg, hs_pg_tri.inc) over a k19_arg whose w points at the scaled weights, the hook's is a single step of the
// unit's host definition (hs_pg_host_relax) over the same weights.  Definition: include/slamhip.h, rules R1 - R4; the arithmetic host
// and device share: hs_pg_lm.h, and hs_pg.h for the stopped code and the "pose + x" that k26_decide and k26_trial need.
//  * k26_weigh<0>: a lane per edge, rule R1 at the poses: c_e, f_e, w_eff into the second weight array, the block sums of rho_e.
//  * k26_weigh<1>: the same lane at the trial poses, the cost alone.
//  * k26_trial: a lane per node, trial = pose + x, theta wrapped; a fixed node's trial is its pose.
//  * k26_decide: ONE workgroup, once per attempt: F and F_trial from the block sums (k19_total), rule R2's comparison, rule R3's
//    test, the attempt's slamhip_pg_lm_iter and the accept word.
//  * k26_commit: a lane per node, pose = trial behind an accepted attempt.
// The host reads the accept word once per attempt and forms the next lambda by rule R2 (lambda travels as a kernel argument).  Behind
// a rejected attempt the poses have not moved, so k26_weigh<0> and k19_linearise are not launched again: they would store the same bits.

struct k26_state { double F, F_trial; int32_t accept, done; };

struct k26_arg {
    const unsigned char *robust;                           // a byte per edge; nullptr: every edge is robust
    double *w_eff, *f, *trial;
    double *part_f, *part_t;                               // the block sums of rho_e at the poses, at the trial poses (PE each)
    k26_state *st; slamhip_pg_lm_iter *iters; double *final_F;
    int kind; double phi;
};

static_assert(sizeof(slamhip_pg_lm_spec) == 88 && sizeof(slamhip_pg_lm_iter) == 64, "the records of include/slamhip.h");

template <int TRIAL>
__global__ void __launch_bounds__(K19_LANES) k26_weigh(const k19_arg A, const k26_arg L)
{
    __shared__ double lds[K19_LANES];
    const int e = (int)blockIdx.x * K19_LANES + (int)threadIdx.x;
    double term = 0.0;
    if (e < A.E) {
        const int2 ij = A.ij[e];
        const double *pose = TRIAL ? L.trial : A.pose;
        double pi[3], pj[3], z[3], w[3], f, rho;
        k19_load3(pose, ij.x, pi); k19_load3(pose, ij.y, pj);
        k19_load3(A.z, e, z); k19_load3(A.w, e, w);
        hs_lm_edge(pi, pj, z, w, L.kind, L.robust ? L.robust[e] != 0 : true, L.phi, &f, &rho);
        if (!TRIAL) {
            const double we[3] = { f * w[0], f * w[1], f * w[2] };
            k19_store3(L.w_eff, e, we);
            L.f[e] = f;
        }
        term = rho;
    }
    const double sum = k19_block_sum(term, lds);
    if (threadIdx.x == 0) (TRIAL ? L.part_t : L.part_f)[blockIdx.x] = sum;
}

__global__ void __launch_bounds__(K19_LANES) k26_trial(const k19_arg A, const k26_arg L)
{
    const int n = (int)blockIdx.x * K19_LANES + (int)threadIdx.x;
    if (n >= A.N) return;
    double pose[3];
    k19_load3(A.pose, n, pose);
    if (!A.fixed[n]) {
        double x[3];
        k19_load3(A.x, n, x);
        hs_pg_add_pose(pose, x);
    }
    k19_store3(L.trial, n, pose);
}

// one workgroup.  final_only: F at the poses as they stand, beside the array; else the end of attempt `outer`
__global__ void __launch_bounds__(K19_LANES) k26_decide(const k19_arg A, const k26_arg L, double lambda, double tol, double ftol, int outer, int final_only)
{
    __shared__ double lds[K19_LANES], lds2[64];
    const double F = k19_total(L.part_f, A.PE, lds, lds2);
    if (final_only) {
        if (threadIdx.x == 0) *L.final_F = F;
        return;
    }
    __syncthreads();
    const double Ft = k19_total(L.part_t, A.PE, lds, lds2);
    if (threadIdx.x == 0) {
        const k19_state *S = A.st;
        slamhip_pg_lm_iter I;
        I.F = F; I.F_trial = Ft; I.lambda = lambda;
        I.rz0 = S->rz0; I.cg_iters = S->iters; I.rz = S->rz[I.cg_iters & 1];
        I.stopped = hs_pg_stopped(S->stop, I.rz, I.rz0, tol);
        I.accepted = hs_lm_accept(F, Ft) ? 1 : 0;
        I.reserved[0] = I.reserved[1] = I.reserved[2] = 0;
        L.iters[outer] = I;
        k26_state D;
        D.F = F; D.F_trial = Ft; D.accept = I.accepted; D.done = I.accepted && hs_lm_done(F, Ft, ftol) ? 1 : 0;
        *L.st = D;
    }
}

__global__ void __launch_bounds__(K19_LANES) k26_commit(const k19_arg A, const k26_arg L)
{
    if (!L.st->accept) return;                                             // (k26_decide's word: the same in every workgroup)
    const int n = (int)blockIdx.x * K19_LANES + (int)threadIdx.x;
    if (n < A.N && !A.fixed[n]) {
        double pose[3];
        k19_load3(L.trial, n, pose);
        k19_store3(A.pose, n, pose);
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------
static int32_t hs_lm_check_spec(const slamhip_pg_lm_spec *sp)
{
    if (!hs_lm_spec_ok(sp))
        SH_FAIL(SLAMHIP_ERR_INVALID, "pose graph relax (lm): n_outer = %d in [1, 64], n_cg = %d in [1, 2^20], check_every = %d >= 1, precond = %d in {0, 1}, kind = %d in {0, 1, 2}, "
                "reserved = %d == 0, lambda0 = %g >= 0, up = %g > 1, down = %g in (0, 1], 0 <= lambda_min = %g <= lambda_max = %g, tol = %g and ftol = %g >= 0, all finite, phi = %g finite and > 0",
                sp->n_outer, sp->n_cg, sp->check_every, sp->precond, sp->kind, sp->reserved, sp->lambda0, sp->up, sp->down, sp->lambda_min, sp->lambda_max, sp->tol, sp->ftol, sp->phi);
    return SLAMHIP_OK;
}

// the unit's own block, made on first use and grown with the graph; after SLAMHIP_ERR_NOMEM the graph is as it was
static int32_t hs_lm_blocks(hs_pg *g, const char *who, k26_arg *L)
{
    const size_t n = (size_t)g->A.N, e = (size_t)g->A.E, pe = (size_t)g->A.PE;
    size_t o = 0;
    const size_t o_w = o; o += hs_pg_al(24 * e);
    const size_t o_f = o; o += hs_pg_al(8 * e);
    const size_t o_trial = o; o += hs_pg_al(24 * n);
    const size_t o_robust = o; o += hs_pg_al(e);
    const size_t o_pf = o; o += hs_pg_al(8 * pe);
    const size_t o_pt = o; o += hs_pg_al(8 * pe);
    const size_t o_st = o; o += hs_pg_al(sizeof(k26_state));
    const size_t o_it = o; o += hs_pg_al(sizeof(slamhip_pg_lm_iter) * HS_PG_MAX_OUTER);
    const size_t o_fin = o; o += hs_pg_al(8);
    SH_TRY(g->d_lm.grow(o, who));
    unsigned char *d = g->d_lm;
    L->robust = d + o_robust;
    L->w_eff = (double *)(d + o_w); L->f = (double *)(d + o_f); L->trial = (double *)(d + o_trial);
    L->part_f = (double *)(d + o_pf); L->part_t = (double *)(d + o_pt);
    L->st = (k26_state *)(d + o_st); L->iters = (slamhip_pg_lm_iter *)(d + o_it); L->final_F = (double *)(d + o_fin);
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_pg_relax_lm(slamhip_hs *hs, const slamhip_pg_lm_spec *spec, const uint8_t *robust, slamhip_pg_lm_iter *out_iters, int32_t *out_n,
                                          double *out_F_final, double *out_f)
{
    SH_CHECK_ARG(hs && spec && out_iters && out_n && out_F_final);
#if K19_SCALAR_LAUNCH
    SH_FAIL(SLAMHIP_ERR_STATE, "K26 is not part of the K19_SCALAR_LAUNCH developer build");
#endif
    SH_TRY(hs_lm_check_spec(spec));
    SH_TRY(hs_pg_need(hs, "pose graph relax (lm)"));
    hs_pg *g = hs->pg;
    const k19_arg &A = g->A;
    hipStream_t st = hs->ctx->stream;
    SH_TRY(hs_call_begin(hs));
    if (spec->precond == HS_LM_TRI) SH_TRY(hs_tri_blocks(g, "pose graph relax (lm)"));
    k26_arg L;
    SH_TRY(hs_lm_blocks(g, "pose graph relax (lm)", &L));
    L.kind = spec->kind; L.phi = spec->phi;
    // the pinned block: the records, F, f, the two state words' copies, the robust bytes on their way in
    const size_t e = (size_t)A.E, rec_bytes = sizeof(slamhip_pg_lm_iter) * (size_t)spec->n_outer;
    const size_t o_fin = rec_bytes, o_f = o_fin + 8, o_st = o_f + 8 * e, o_lst = o_st + hs_pg_al(sizeof(k19_state)), o_rob = o_lst + hs_pg_al(sizeof(k26_state));
    SH_TRY(g->h_io.grow(o_rob + e, "pose graph relax (lm)"));
    k19_state *h_st = (k19_state *)(g->h_io + o_st);
    k26_state *h_lst = (k26_state *)(g->h_io + o_lst);
    if (robust && e) {
        for (size_t i = 0; i < e; i++) g->h_io[o_rob + i] = robust[i] ? 1 : 0;
        SH_HIP(hipMemcpyAsync(const_cast<unsigned char *>(L.robust), g->h_io + o_rob, e, hipMemcpyHostToDevice, st));
    } else {
        L.robust = nullptr;
    }
    k19_arg AL = A;                                                        // the K19 / K22 kernels over the scaled weights
    AL.w = L.w_eff;
    double lambda = spec->lambda0;
    bool moved = true;                                                     // the poses are not the ones last weighed and linearised
    int n = 0;
    while (n < spec->n_outer) {
        if (moved) {
            K19_LAUNCH(k26_weigh<0>, A.PE, A, L);
            K19_LAUNCH(k19_linearise, A.PE, AL);
        }
        SH_TRY(hs_pg_pcg(hs, g, AL, spec->precond == HS_LM_TRI, lambda, spec->n_cg, spec->check_every, spec->tol, h_st));
        K19_LAUNCH(k26_trial, A.PN, A, L);
        K19_LAUNCH(k26_weigh<1>, A.PE, A, L);
        K19_LAUNCH(k26_decide, 1, A, L, lambda, spec->tol, spec->ftol, n, 0);
        K19_LAUNCH(k26_commit, A.PN, A, L);
        SH_HIP(hipMemcpyAsync(h_lst, L.st, sizeof(k26_state), hipMemcpyDeviceToHost, st));
        SH_TRY(hs_call_finish(hs));                                        // (the accept word: rule R2's lambda is the host's)
        n++;
        moved = h_lst->accept != 0;
        lambda = hs_lm_next_lambda(spec, lambda, moved);
        if (h_lst->done) break;
    }
    if (moved) K19_LAUNCH(k26_weigh<0>, A.PE, A, L);
    K19_LAUNCH(k26_decide, 1, A, L, 0.0, 0.0, 0.0, 0, 1);
    SH_HIP(hipMemcpyAsync(g->h_io, L.iters, sizeof(slamhip_pg_lm_iter) * (size_t)n, hipMemcpyDeviceToHost, st));
    SH_HIP(hipMemcpyAsync(g->h_io + o_fin, L.final_F, 8, hipMemcpyDeviceToHost, st));
    if (out_f && e) SH_HIP(hipMemcpyAsync(g->h_io + o_f, L.f, 8 * e, hipMemcpyDeviceToHost, st));
    SH_TRY(hs_call_finish(hs));
    memcpy(out_iters, g->h_io, sizeof(slamhip_pg_lm_iter) * (size_t)n);
    *out_n = n;
    memcpy(out_F_final, g->h_io + o_fin, 8);
    if (out_f && e) memcpy(out_f, g->h_io + o_f, 8 * e);
    return SLAMHIP_OK;
}

// ---- CPU-side test hook: hs_pg_lm.h -- the text the kernels run -- in plain loops ------------------------------------------------------
// rule R1 over every edge -> F by rule 6; w_eff and f may be nullptr (the cost alone)
static double hs_lm_host_weigh(const double *pose, const int32_t *ij, const double *z, const double *w, int E, const uint8_t *robust, int kind, double phi,
                               double *w_eff, double *f_out, double *tmp)
{
    for (int e = 0; e < E; e++) {
        const double *we = w + 3 * (size_t)e;
        double f, rho;
        hs_lm_edge(pose + 3 * (size_t)ij[2 * (size_t)e], pose + 3 * (size_t)ij[2 * (size_t)e + 1], z + 3 * (size_t)e, we, kind, robust ? robust[e] != 0 : true, phi, &f, &rho);
        if (w_eff) for (int a = 0; a < 3; a++) w_eff[3 * (size_t)e + a] = f * we[a];
        if (f_out) f_out[e] = f;
        tmp[e] = rho;
    }
    return hs_pg_tree_sum(tmp, (size_t)E);
}

extern "C" int32_t slamhip_debug_pg_relax_lm(double *poses, const uint8_t *fixed, int32_t N, const int32_t *ij, const double *z, const double *w, int32_t E,
                                             const slamhip_pg_lm_spec *spec, const uint8_t *robust, slamhip_pg_lm_iter *out_iters, int32_t *out_n,
                                             double *out_F_final, double *out_f)
{
    SH_CHECK_ARG(spec && out_iters && out_n && out_F_final);
    SH_TRY(hs_lm_check_spec(spec));
    SH_TRY(hs_pg_check_graph(poses, fixed, N, ij, z, w, E));
    const size_t n3 = 3 * (size_t)N;
    std::vector<double> w_eff(3 * (size_t)E + 3), f((size_t)E + 1), tmp((size_t)E + HS_PG_BLOCK), trial(n3);
    slamhip_pg_spec one;                                                   // a single step of the K19 / K22 definition
    one.n_outer = 1; one.n_cg = spec->n_cg; one.check_every = spec->check_every; one.reserved = 0; one.tol = spec->tol;
    double lambda = spec->lambda0, F = 0.0;
    bool moved = true;
    int n = 0;
    while (n < spec->n_outer) {
        if (moved) F = hs_lm_host_weigh(poses, ij, z, w, E, robust, spec->kind, spec->phi, w_eff.data(), f.data(), tmp.data());
        memcpy(trial.data(), poses, 8 * n3);
        slamhip_pg_iter step;
        double chi2_w;
        one.lambda = lambda;
        hs_pg_host_relax(spec->precond == HS_LM_TRI, trial.data(), fixed, N, ij, z, w_eff.data(), E, &one, &step, &chi2_w, nullptr, nullptr);
        const double Ft = hs_lm_host_weigh(trial.data(), ij, z, w, E, robust, spec->kind, spec->phi, nullptr, nullptr, tmp.data());
        slamhip_pg_lm_iter I;
        I.F = F; I.F_trial = Ft; I.lambda = lambda;
        I.rz0 = step.rz0; I.rz = step.rz; I.cg_iters = step.cg_iters; I.stopped = step.stopped;
        I.accepted = hs_lm_accept(F, Ft) ? 1 : 0;
        I.reserved[0] = I.reserved[1] = I.reserved[2] = 0;
        out_iters[n++] = I;
        moved = I.accepted != 0;
        lambda = hs_lm_next_lambda(spec, lambda, moved);
        if (moved) {
            memcpy(poses, trial.data(), 8 * n3);
            if (hs_lm_done(F, Ft, spec->ftol)) break;
        }
    }
    if (moved) F = hs_lm_host_weigh(poses, ij, z, w, E, robust, spec->kind, spec->phi, w_eff.data(), f.data(), tmp.data());
    *out_n = n;
    *out_F_final = F;
    if (out_f && E) memcpy(out_f, f.data(), 8 * (size_t)E);
    return SLAMHIP_OK;
}
