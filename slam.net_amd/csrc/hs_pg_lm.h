// hs_pg_lm.h -- the arithmetic of the damped and robust pose-graph relaxation (K26, hs_pg_lm.inc) that host and device share: the
// kernels k26_weigh and k26_decide and the test hook slamhip_debug_pg_relax_lm run this text.  Definition: include/slamhip.h,
// slamhip_hs_pg_relax_lm, rules R1 - R4.  Binary64 + - * / only, one rounding per operation (the build has -ffp-contract=off); every
// expression is parenthesised as the definition writes it.
#pragma once
#include "hs_pg.h"

// slamhip_pg_lm_spec.kind and .precond
#define HS_LM_NONE 0
#define HS_LM_DCS 1
#define HS_LM_GM 2
#define HS_LM_JACOBI 0
#define HS_LM_TRI 1

// rule R1: the factor f_e and the cost rho_e of an edge whose quadratic cost is c
__host__ __device__ static inline void hs_lm_factor(int kind, bool robust, double phi, double c, double *f, double *rho)
{
    *f = 1.0; *rho = c;
    if (!robust || kind == HS_LM_NONE) return;
    if (kind == HS_LM_DCS) {
        if (c <= phi) return;
        const double s = (2.0 * phi) / (phi + c);
        *f = s * s;
        *rho = (phi * ((3.0 * c) - phi)) / (c + phi);
    } else {
        const double s = phi / (phi + c);
        *f = s * s;
        *rho = (phi * c) / (phi + c);
    }
}

// rule R1 for one edge at the poses (pi, pj): c_e is rule 3's chi2_e with the caller's weights
__host__ __device__ static inline void hs_lm_edge(const double *pi, const double *pj, const double *z, const double *w, int kind, bool robust, double phi,
                                                  double *f, double *rho)
{
    hs_pg_rec R;
    double r[3];
    hs_pg_edge(pi, pj, z, w, &R, r);
    hs_lm_factor(kind, robust, phi, R.chi2, f, rho);
}

// rule R2: the comparison, and the lambda of the next attempt
__host__ __device__ static inline bool hs_lm_accept(double F, double F_trial) { return F_trial < F; }
static inline double hs_lm_next_lambda(const slamhip_pg_lm_spec *sp, double lambda, bool accepted)
{
    if (accepted) {
        lambda = lambda * sp->down;
        return lambda < sp->lambda_min ? sp->lambda_min : lambda;
    }
    lambda = lambda * sp->up;
    return lambda > sp->lambda_max ? sp->lambda_max : lambda;
}

// rule R3: what ends the run behind an accepted attempt
__host__ __device__ static inline bool hs_lm_done(double F, double F_trial, double ftol) { return (F - F_trial) <= ftol * F; }

// what slamhip_hs_pg_relax_lm refuses of its spec
static inline bool hs_lm_spec_ok(const slamhip_pg_lm_spec *sp)
{
    return sp->n_outer >= 1 && sp->n_outer <= HS_PG_MAX_OUTER && sp->n_cg >= 1 && sp->n_cg <= HS_PG_MAX_CG && sp->check_every >= 1 &&
           (sp->precond == HS_LM_JACOBI || sp->precond == HS_LM_TRI) && sp->kind >= HS_LM_NONE && sp->kind <= HS_LM_GM && sp->reserved == 0 &&
           isfinite(sp->lambda0) && sp->lambda0 >= 0.0 && isfinite(sp->up) && sp->up > 1.0 && sp->down > 0.0 && sp->down <= 1.0 &&
           isfinite(sp->lambda_min) && isfinite(sp->lambda_max) && sp->lambda_min >= 0.0 && sp->lambda_min <= sp->lambda_max &&
           isfinite(sp->tol) && sp->tol >= 0.0 && isfinite(sp->ftol) && sp->ftol >= 0.0 && (sp->kind == HS_LM_NONE || (isfinite(sp->phi) && sp->phi > 0.0));
}
