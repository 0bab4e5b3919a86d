"""The graphs of the damped and robust relaxation's tests (K26: tests/test_hs_pg_lm_abi.py, tests/test_gpu_hector_pg_lm.py) and the NumPy
restatement of its definition (include/slamhip.h, slamhip_hs_pg_relax_lm, rules R1 - R4).

The restatement (np_cost, np_relax_lm) shares no text with hs_pg_lm.h.  An attempt's step is ONE outer iteration of the restatements it
builds on -- np_relax of tests/test_hs_pg_abi.py, np_relax_tri of tests/pg_tri_cases.py -- over the scaled weights; R1 is elementwise
NumPy with the header's parentheses.  `wrong` names a wrong copy of a rule; each must fail its case of WRONG_CASES."""
import numpy as np

import pg_tri_cases as tc
import test_hs_pg_abi as A

D = np.float64
NONE, DCS, GM = 0, 1, 2
W_RING = (400.0, 400.0, 2500.0)
FIELDS = ("F", "F_trial", "lambda", "rz0", "rz", "cg_iters", "stopped", "accepted")


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def np_cost(poses, ij, z, w, rb, kind, phi, wrong=None):
    """Rule R1 at `poses` -> (F, f (E,), w_eff (E, 3))."""
    c = A.np_edges(poses, ij, z, w)[3]
    f = np.ones_like(c); rho = c.copy()
    phi = D(phi)
    if kind == DCS:
        m = rb & ~((c < phi) if wrong == "lt" else (c <= phi))
        s = (D(2.0) * phi) / (phi + c[m])
        f[m] = s if wrong == "s" else s * s
        rho[m] = (phi * ((D(3.0) * c[m]) - phi)) / (c[m] + phi)
    elif kind == GM:
        s = phi / (phi + c[rb])
        f[rb] = s if wrong == "s" else s * s
        rho[rb] = (phi * c[rb]) / (phi + c[rb])
    w_eff = f[:, None] * w
    if wrong == "F_weff":
        return A.np_sum(A.np_edges(poses, ij, z, w_eff)[3]), f, w_eff
    return A.np_sum(rho), f, w_eff


def np_next_lambda(lam, accepted, sp):
    if accepted:
        lam = lam * D(sp["down"])
        return D(sp["lambda_min"]) if lam < D(sp["lambda_min"]) else lam
    lam = lam * D(sp["up"])
    return D(sp["lambda_max"]) if lam > D(sp["lambda_max"]) else lam


def np_relax_lm(poses, fixed, ij, z, w, sp, robust=None, wrong=None):
    """Rules R1 - R4; sp: a capi.pg_lm_spec record -> (poses, iters as a list of dicts, F_final, f)."""
    sp = {n: sp[n][0] for n in sp.dtype.names}
    poses, fx, ij, z, w = tc.np_graph(poses, fixed, ij, z, w)
    rb = np.ones(ij.shape[0], bool) if robust is None else np.asarray(robust).astype(bool)
    kind, phi = int(sp["kind"]), sp["phi"]
    step = tc.np_relax_tri if int(sp["precond"]) == 1 else A.np_relax
    lam = D(sp["lambda0"])
    iters = []
    accepted = True
    while len(iters) < int(sp["n_outer"]):
        if wrong == "lambda_early":
            lam = np_next_lambda(lam, accepted, sp)
        F, f, w_eff = np_cost(poses, ij, z, w, rb, kind, phi, wrong)
        trial, it = step(poses, fx, ij, z, w_eff, 1, int(sp["n_cg"]), lam, sp["tol"])[:2]
        Ft = np_cost(trial, ij, z, w, rb, kind, phi, wrong)[0]
        accepted = bool(Ft <= F) if wrong == "accept_le" else bool(Ft < F)
        iters.append({"F": F, "F_trial": Ft, "lambda": lam, "rz0": it[0]["rz0"], "rz": it[0]["rz"], "cg_iters": it[0]["cg_iters"],
                      "stopped": it[0]["stopped"], "accepted": int(accepted)})
        if wrong != "lambda_early":
            lam = np_next_lambda(lam, accepted, sp)
        if accepted:
            poses = trial
            if (F - Ft) <= D(sp["ftol"]) * F:
                break
    F, f, _ = np_cost(poses, ij, z, w, rb, kind, phi, wrong)
    return poses, iters, F, f


def same_as_hook(capi, poses, fixed, ij, z, w, sp, robust=None, wrong=None):
    """hook == restatement on every output -> the hook's outputs (with wrong: whether they are all equal)."""
    hp, hit, hF, hf = capi.debug_pg_relax_lm(poses, fixed, ij, z, w, sp, robust)
    wp, wit, wF, wf = np_relax_lm(poses, fixed, ij, z, w, sp, robust, wrong)
    eq = np.array_equal(hp, wp) and hF == wF and np.array_equal(hf, wf) and len(hit) == len(wit)
    eq = eq and all(hit[o][n] == wit[o][n] for o in range(min(len(hit), len(wit))) for n in FIELDS) and not hit["reserved"].any()
    if wrong is not None:
        return eq
    assert eq, (hp - wp, hit, wit, hF, wF)
    return hp, hit, hF, hf


# ---- graphs ----------------------------------------------------------------------------------------------------------------------
def true_ring(N):
    """Node k at angle 2 pi k / N on the radius N / (2 pi), heading along the tangent."""
    a = 2.0 * np.pi * np.arange(N) / N
    R = N / (2.0 * np.pi)
    return np.stack([R * np.cos(a), R * np.sin(a), A.np_wrap(a + np.pi / 2)], axis=1)


def dead_reckoning(true, bias):
    """The chain's exact measurements composed from node 0, `bias` added to the heading at every step."""
    N = true.shape[0]
    poses = [true[0].copy()]
    for k in range(N - 1):
        p = A.compose(poses[-1], A.rel(true[k], true[k + 1]))
        p[2] = A.np_wrap(p[2] + bias)
        poses.append(p)
    return np.stack(poses)


def ring_graph(N, bias, loops):
    """-> (start, ij, z, w, true): the chain (k, k + 1), then `loops`; every z exact, w = W_RING, node 0 fixed (fixed = None)."""
    true = true_ring(N)
    ij = np.array([(k, k + 1) for k in range(N - 1)] + [tuple(l) for l in loops], np.int32).reshape(-1, 2)
    z = np.stack([A.rel(true[i], true[j]) for i, j in ij]) if len(ij) else np.zeros((0, 3))
    w = np.tile(np.array(W_RING), (ij.shape[0], 1))
    return dead_reckoning(true, bias), ij, z, w, true


def ring_a(N, bias):
    """Ring A of the issue: the chain closed by (N - 1, 0); N * bias stays below pi."""
    assert N * bias < np.pi
    return ring_graph(N, bias, [(N - 1, 0)])


RING_A = ((64, 0.03), (257, 0.01))
B_LOOPS = ((63, 0), (40, 8), (50, 20))
B_CORRUPTION = np.array([1.5, -1.0, 0.4])


def graph_b(false_edge=True):
    """Graph B of the issue: a ring of 64 from a start with bias 0.005, three loops, the last one's measurement corrupted
    -> (start, ij, z, w, true, robust): the loops are the robust edges."""
    start, ij, z, w, true = ring_graph(64, 0.005, B_LOOPS)
    if false_edge:
        z[-1] = z[-1] + B_CORRUPTION
    robust = np.arange(ij.shape[0]) >= 63
    return start, ij, z, w, true, robust


def pose_error(poses, true):
    """-> (largest position error in metres, largest heading error in radians)."""
    d = np.asarray(poses, D) - true
    return float(np.hypot(d[:, 0], d[:, 1]).max()), float(np.abs(A.np_wrap(d[:, 2])).max())


def noisy_ring(N, n_edges=None, seed=0):
    """A size case for device == hook: tc.chain_ring's noisy ring with two loops, padded with further loops (or cut) to n_edges edges."""
    loops = [(N - 2, 1), (N // 2, 2)] if N >= 8 else []
    poses, ij, z, w = tc.chain_ring(N, loops, seed=200 + N + seed)
    if n_edges is not None:
        g = np.random.Generator(np.random.Philox(300 + n_edges))
        true = tc.ring_true(N)
        while ij.shape[0] < n_edges:
            i, j = (int(v) for v in g.choice(N, 2, replace=False))
            ij = np.concatenate([ij, [(i, j)]]).astype(np.int32)
            z = np.concatenate([z, tc.rel_many(true, np.array([i]), np.array([j])) + g.standard_normal((1, 3)) * A.SIGMA])
            w = np.concatenate([w, w[:1]])
        ij, z, w = ij[:n_edges], z[:n_edges], w[:n_edges]
    return poses, ij, z, w


def one_edge(c_over_phi_ulps=0, phi=1.0):
    """Two nodes, one edge with r = (0.5, 0, 0) and wx = 4 phi: c_e == phi exactly, or that many ulps of wx beside it."""
    poses = np.array([[0.0, 0.0, 0.0], [1.5, 0.0, 0.0]])
    wx = D(4.0 * phi)
    for _ in range(abs(c_over_phi_ulps)):
        wx = np.nextafter(wx, D(np.inf) if c_over_phi_ulps > 0 else D(0.0))
    return poses, np.array([[0, 1]], np.int32), np.array([[1.0, 0.0, 0.0]]), np.array([[wx, 4.0, 4.0]])
