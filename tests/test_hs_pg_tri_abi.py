"""CPU-side checks of the odometry-chain preconditioner of the pose-graph relaxation (K22: slamhip_hs_pg_relax_tri, _pg_tri_apply and
the hooks slamhip_debug_pg_relax_tri / _pg_tri_apply; include/slamhip.h, rules T1 - T5).  tests/test_gpu_hector_pg_tri.py compares the
device with the hooks; here the hooks are tied to the NumPy restatement of tests/pg_tri_cases.py with == on every output, to
numpy.linalg.solve on the dense T by backward errors, and to slamhip_debug_pg_relax by iteration counts and results.  No compute calls
on a device."""
import math

import numpy as np
import pytest

import pg_tri_cases as tc
import test_hs_pg_abi as A

D = np.float64
FIELDS = ("chi2", "rz0", "rz", "cg_iters", "stopped")
SYMBOLS = ("slamhip_hs_pg_relax_tri", "slamhip_hs_pg_tri_apply", "slamhip_debug_pg_relax_tri", "slamhip_debug_pg_tri_apply")


@pytest.fixture(scope="module")
def capi():
    import slam.net_amd.build as b
    b.build()
    import slam.net_amd.capi as capi
    return capi


def hook_equals_restatement(capi, poses, fixed, ij, z, w, lam, n_outer=2, n_cg=40, tol=1e-6, seed=1):
    g = np.random.Generator(np.random.Philox(seed))
    rhs = g.standard_normal((np.asarray(poses).reshape(-1, 3).shape[0], 3))
    got = capi.debug_pg_tri_apply(poses, fixed, ij, z, w, lam, rhs)
    want = tc.np_tri_apply(poses, fixed, ij, z, w, lam, rhs)
    assert np.array_equal(got, want), np.abs(got - want).max()
    hp, hit, hfin, hr, hc = capi.debug_pg_relax_tri(poses, fixed, ij, z, w, capi.pg_spec(n_outer, n_cg, lam=lam, tol=tol))
    wp, wit, wfin, wr, wc = tc.np_relax_tri(poses, fixed, ij, z, w, n_outer, n_cg, lam, tol)
    assert np.array_equal(hp, wp) and hfin == wfin and np.array_equal(hr, wr) and np.array_equal(hc, wc), (np.abs(hp - wp).max(), hfin, wfin)
    for o in range(n_outer):
        assert all(hit[o][f] == wit[o][f] for f in FIELDS), (o, hit[o], wit[o])
    return hp, hit, hfin, got


# ---- 1. hook == restatement -----------------------------------------------------------------------------------------------------------
def test_symbols(capi):
    L = capi.lib()
    declared = set(capi.declared_symbols())
    for name in SYMBOLS:
        assert name in declared and hasattr(L, name) and name in L._signatures, name
    assert capi.PG_SPEC.itemsize == 32 and [capi.PG_SPEC.fields[n][1] for n in ("n_outer", "n_cg", "check_every", "reserved", "lambda", "tol")] == [0, 4, 8, 12, 16, 24]


@pytest.mark.parametrize("N", [n for n in tc.LEVEL_SIZES if n <= 257] + [tc.TAIL + 1])
def test_restatement_at_level_edges(capi, N):
    poses, ij, z, w = tc.level_case(N)
    hook_equals_restatement(capi, poses, None, ij, z, w, 0.0, n_outer=2, n_cg=30)


@pytest.mark.parametrize("name", sorted(tc.structure_cases()))
def test_restatement_on_structures(capi, name):
    poses, fixed, ij, z, w, lam = tc.structure_cases()[name]
    hp, hit, hfin, zz = hook_equals_restatement(capi, poses, fixed, ij, z, w, lam, n_outer=3, n_cg=60)
    assert np.isfinite(hp).all() and np.isfinite(zz).all() and math.isfinite(hfin)
    fx = np.zeros(40, bool) if fixed is None else np.asarray(fixed).astype(bool)
    if name == "dead_node":
        assert np.array_equal(zz[10], [0.0, 0.0, 0.0]) and np.array_equal(hp[10], poses[10])
    if name == "lone_node_lambda":
        assert zz[10].any() and np.array_equal(hp[10], poses[10])          # z = rhs / lambda there; g = 0, so the node stays
    if name in ("fixed_mid", "fixed_ends"):
        assert np.array_equal(hp[fx], poses[fx]) and not zz[fx].any()
    if name == "floating_segment":
        print("floating segment: stopped", hit["stopped"].tolist(), "cg_iters", hit["cg_iters"].tolist())


def test_star_equals_block_jacobi(capi):
    """No chain edge joins two live nodes: T is rule 4's block diagonal, so PCG is slamhip_debug_pg_relax's -- the iteration counts are
    equal, and every value is equal under == (what the header states: a zero may differ in its sign, no more)."""
    poses, fixed, ij, z, w, lam = tc.structure_cases()["star"]
    spec = capi.pg_spec(3, 40)
    tp, tit, tfin, tr, tchi = capi.debug_pg_relax_tri(poses, fixed, ij, z, w, spec)
    jp, jit, jfin, jr, jchi = capi.debug_pg_relax(poses, fixed, ij, z, w, spec)
    assert tit["cg_iters"].tolist() == jit["cg_iters"].tolist() and (jit["cg_iters"] > 0).all()
    assert np.array_equal(tp, jp) and tfin == jfin and np.array_equal(tr, jr) and all(np.array_equal(tit[f], jit[f]) for f in FIELDS)


# ---- 2. against LAPACK on the dense T ---------------------------------------------------------------------------------------------
def dense_T(poses, fixed, ij, z, w, lam, want_H=False):
    """T from rule 3's A and B: H = sum of J^T W J over the edges + lambda I on the free nodes, its block-tridiagonal part, identity
    rows for the fixed nodes (every free node of the graphs used here is live)."""
    poses, fx, ij, z, w = tc.np_graph(poses, fixed, ij, z, w)
    N = poses.shape[0]
    Aj, Bj, _, _ = A.np_edges(poses, ij, z, w)
    H = np.zeros((N, N, 3, 3))
    for e, (i, j) in enumerate(ij):
        W = np.diag(w[e])
        for a, Ja in ((i, Aj[e]), (j, Bj[e])):
            for b, Jb in ((i, Aj[e]), (j, Bj[e])):
                H[a, b] += Ja.T @ W @ Jb
    T = np.zeros((3 * N, 3 * N))
    for n in range(N):
        for m in (n - 1, n, n + 1):
            if 0 <= m < N and not fx[n] and not fx[m]:
                T[3 * n:3 * n + 3, 3 * m:3 * m + 3] = H[n, m]
        T[3 * n:3 * n + 3, 3 * n:3 * n + 3] += np.eye(3) * (1.0 if fx[n] else lam)
    if want_H:                                                             # H itself, the rows and columns of the fixed nodes the identity's
        Hd = np.zeros((3 * N, 3 * N))
        for n in range(N):
            for m in range(N):
                if not fx[n] and not fx[m]:
                    Hd[3 * n:3 * n + 3, 3 * m:3 * m + 3] = H[n, m]
            Hd[3 * n:3 * n + 3, 3 * n:3 * n + 3] += np.eye(3) * (1.0 if fx[n] else lam)
        return T, fx, Hd
    return T, fx


def backward_error(T, zz, r):
    return np.linalg.norm(T @ zz - r) / (np.linalg.norm(T, 2) * np.linalg.norm(zz) + np.linalg.norm(r))


@pytest.mark.parametrize("N", [2, 9, 40, 257, 300])
def test_apply_against_lapack(capi, N):
    """Backward errors ||T z - r|| / (||T|| ||z|| + ||r||) of the hook and of numpy.linalg.solve on the same dense system.  Measured
    here (N: hook, LAPACK): 2: 6.1e-17, 3.1e-17; 9: 2.4e-17, 2.0e-17; 40: 2.0e-17, 1.6e-17; 257: 8.4e-19, 8.7e-19; 300: 5.9e-19,
    6.3e-19 -- the hook within 2.0 x LAPACK's.  Allowed: 8 x LAPACK's (both are a fraction of 2^-53; cyclic reduction has log2 N levels
    of 3 x 3 inverses where LAPACK pivots once, hence a margin of a few times)."""
    poses, ij, z, w = tc.level_case(N)
    T, fx = dense_T(poses, None, ij, z, w, 0.0)
    g = np.random.Generator(np.random.Philox(N))
    rhs = g.standard_normal((N, 3)); rhs[fx] = 0.0
    r = rhs.reshape(-1)
    hook = capi.debug_pg_tri_apply(poses, None, ij, z, w, 0.0, rhs).reshape(-1)
    lap = np.linalg.solve(T, r)
    eh, el = backward_error(T, hook, r), backward_error(T, lap, r)
    print("N = %d: backward error hook %.2e, LAPACK %.2e, ratio %.2f; smallest eigenvalue of T %.2e" % (N, eh, el, eh / el, np.linalg.eigvalsh(T).min()))
    assert eh <= 8.0 * el


# ---- 3. iteration counts -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ring257_runs(capi):
    out = {}
    for name, loops in (("three", [(200, 10), (130, 3)]), ("one", [])):    # the closing edge (256, 0) is chain_ring's own
        poses, ij, z, w = tc.chain_ring(257, loops, seed=7)
        spec = capi.pg_spec(6, 8 * 257, tol=1e-6)
        out[name] = (poses, capi.debug_pg_relax_tri(poses, None, ij, z, w, spec), capi.debug_pg_relax(poses, None, ij, z, w, spec), tc.ring_true(257))
    return out


def test_iterations_on_the_ring_of_257(ring257_runs):
    """Loops (256, 0), (200, 10), (130, 3): L' = 2 edges join two free nodes off the chain, so 6 L' + 1 = 13 iterations in exact
    arithmetic, and at most twice that here; the loop (256, 0) alone: T = H, 1 or 2.  Both below a tenth of block-Jacobi's count."""
    _, tri, jac, _ = ring257_runs["three"]
    print("three loops: tri %s, block-Jacobi %s" % (tri[1]["cg_iters"].tolist(), jac[1]["cg_iters"].tolist()))
    assert 1 <= tri[1][0]["cg_iters"] <= 26 and tri[1][0]["stopped"] == 0
    assert 10 * tri[1][0]["cg_iters"] < jac[1][0]["cg_iters"]
    _, tri1, jac1, _ = ring257_runs["one"]
    print("one loop: tri %s, block-Jacobi %s" % (tri1[1]["cg_iters"].tolist(), jac1[1]["cg_iters"].tolist()))
    assert tri1[1][0]["cg_iters"] in (1, 2) and tri1[1][0]["stopped"] == 0
    assert 10 * tri1[1][0]["cg_iters"] < jac1[1][0]["cg_iters"]


@pytest.mark.parametrize("name", ["three", "one"])
def test_both_solvers_reach_the_same_minimum(ring257_runs, name):
    """chi2 falls for both solvers and they end at the same poses.  The bound on the difference: a PCG that stops at
    rz <= tol^2 rz0 with the preconditioner P leaves the step wrong by e = H^-1 res with |e| <= |res| / min eig(H) and
    |res|^2 <= max eig(P) rz, so |e| <= tol sqrt(max eig(P) rz0) / min eig(H).  Taken with the rz0 of the FIRST step (the largest: every
    later step's is smaller, and after six steps Gauss-Newton's own remainder is far below it), for both solvers, the eigenvalues
    measured on the dense H, T and block diagonal at the starting poses."""
    poses, tri, jac, _ = ring257_runs[name]
    for run in (tri, jac):
        assert run[2] < run[1][0]["chi2"] and run[1][-1]["stopped"] == 0
    p, ij, z, w = tc.chain_ring(257, [(200, 10), (130, 3)] if name == "three" else [], seed=7)
    T, fx, H = dense_T(p, None, ij, z, w, 0.0, want_H=True)
    Dg = np.zeros_like(H)
    for n in range(257):
        Dg[3 * n:3 * n + 3, 3 * n:3 * n + 3] = H[3 * n:3 * n + 3, 3 * n:3 * n + 3]
    lo = np.linalg.eigvalsh(H).min()
    bound = 1e-6 * (math.sqrt(np.linalg.eigvalsh(T).max() * tri[1][0]["rz0"]) + math.sqrt(np.linalg.eigvalsh(Dg).max() * jac[1][0]["rz0"])) / lo
    diff = np.abs(tri[0] - jac[0]).max()
    print("%s: chi2 %.6f -> tri %.12f, block-Jacobi %.12f; smallest eigenvalue of H %.3e; poses differ by %.3e, bound %.3e" %
          (name, tri[1][0]["chi2"], tri[2], jac[2], lo, diff, bound))
    assert diff <= bound
    assert abs(tri[2] - jac[2]) <= np.linalg.eigvalsh(H).max() * bound * bound * 3 * 257   # chi2 is quadratic about its minimum: |d chi2| <= max eig(H) |d pose|^2


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_equal_pg_relax(capi):
    poses, ij, z, w = A.tiny_graph(3, 4, [(0, 1), (1, 2), (2, 3), (3, 0)])
    bad_specs = [dict(n_outer=0), dict(n_outer=65), dict(n_cg=0), dict(check_every=0), dict(reserved=1), dict(tol=-1.0), dict(lam=-1.0), dict(lam=float("nan"))]
    for kw in bad_specs:
        a = dict(n_outer=1, n_cg=4); a.update(kw)
        codes = []
        for hook in (capi.debug_pg_relax, capi.debug_pg_relax_tri):
            with pytest.raises(capi.SlamhipError) as e:
                hook(poses, None, ij, z, w, capi.pg_spec(**a))
            codes.append(e.value.code)
        assert codes == [capi.ERR_INVALID, capi.ERR_INVALID], kw
    bad_w = w.copy(); bad_w[1, 1] = 0.0
    bad_ij = ij.copy(); bad_ij[2] = (2, 2)
    for args in ((poses, None, ij, z, bad_w), (poses, None, bad_ij, z, w), (poses, [0, 0, 0, 0], ij, z, w)):
        codes = []
        for hook in (capi.debug_pg_relax, capi.debug_pg_relax_tri):
            with pytest.raises(capi.SlamhipError) as e:
                hook(*args, capi.pg_spec(1, 4))
            codes.append(e.value.code)
        assert codes == [capi.ERR_INVALID, capi.ERR_INVALID]
        with pytest.raises(capi.SlamhipError) as e:
            capi.debug_pg_tri_apply(*args, 0.0, np.zeros((4, 3)))
        assert e.value.code == capi.ERR_INVALID
    with pytest.raises(capi.SlamhipError) as e:
        capi.debug_pg_tri_apply(poses, None, ij, z, w, -0.5, np.zeros((4, 3)))
    assert e.value.code == capi.ERR_INVALID


# ---- 5. the lap ----------------------------------------------------------------------------------------------------------------------
def test_lap_on_the_cpu_with_tri(capi):
    """The lap of tests/test_hs_scanmatch_abi.py::test_lap_on_the_cpu, its loop edges relaxed by both hooks.  Measured here: 3 loop
    edges; the largest keyframe position error 1.361 m drifted, 0.074358671 m relaxed by either (equal to the nanometre); PCG
    iterations per step: tri 7, block-Jacobi 132 to 137.  Asserted: tri's error is no worse than block-Jacobi's (beyond the 1e-6 m that the
    binary32 store of the poses resolves at this size), and it takes fewer than a fifth of the iterations."""
    import render_cases as rc
    import test_hs_scanmatch_abi as SM
    L = rc.lap()
    true = L["true"].astype(D)
    _, _, _, loops = SM.lap_edges(capi, L, lambda sp, pr: capi.debug_scans_match(L["scans"], sp, pr))
    p0 = np.asarray(L["drifted"], np.float32).astype(D)
    N = p0.shape[0]
    ij = [(k, k + 1) for k in range(N - 1)] + [(int(l[0]), int(l[1])) for l in loops]
    z = [capi.pg_edge_between(p0[k], p0[k + 1]) for k in range(N - 1)] + [tuple(float(v) for v in l[2]) for l in loops]
    w = [rc.LAP_ODOM_W] * (N - 1) + [tuple(float(v) for v in l[3]) for l in loops]
    spec = capi.pg_spec(5, 4 * N, tol=1e-8)
    g = (p0, None, np.array(ij, np.int32), np.array(z, D), np.array(w, D))
    tri = capi.debug_pg_relax_tri(*g, spec)
    jac = capi.debug_pg_relax(*g, spec)
    e_drift, e_tri, e_jac = (SM.max_position_error(p, true) for p in (L["drifted"], tri[0], jac[0]))
    print("%d loop edges; largest keyframe error: drifted %.3f m, tri %.9f m, block-Jacobi %.9f m; PCG iterations tri %s, block-Jacobi %s" %
          (len(loops), e_drift, e_tri, e_jac, tri[1]["cg_iters"].tolist(), jac[1]["cg_iters"].tolist()))
    assert e_tri < e_drift and e_tri <= e_jac + 1e-6
    assert 5 * int(tri[1]["cg_iters"].sum()) < int(jac[1]["cg_iters"].sum())
