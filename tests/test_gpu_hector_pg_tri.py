"""The odometry-chain preconditioner of the pose-graph relaxation (K22: slamhip_hs_pg_relax_tri, slamhip_hs_pg_tri_apply,
MapRepMultiMap.PgRelax(precond="tri"), PgTriApply, close_loops(precond="tri")) on the device, against the host hooks
slamhip_debug_pg_relax_tri / _pg_tri_apply, which tests/test_hs_pg_tri_abi.py ties to the NumPy restatement of rules T1 - T5.  Everything
is compared with == on the poses, every slamhip_pg_iter field, the final chi2, the residuals and the preconditioner's output; there is
no tolerance anywhere but in the end-to-end case's ordering.

Shapes are the smallest at which each path can go wrong (tests/pg_tri_cases.py): the level edges 1 .. 9, rule 6's blocks 255 .. 257, the
tail's S - 1, S, S + 1 and 2 S + 1 blocks (S = 1024: levels of more than S blocks take a launch each, the others ONE workgroup), 40 and
257 nodes with the developer's SLAMHIP_K22_TAIL at 4 and 16 (several global levels, then the tail), one chain of 65537, and the chain's
structures: a missing edge, fixed nodes, a reversed edge, duplicates, dead and lone nodes, a star, a floating segment."""
import contextlib
import os

import numpy as np
import pytest

import pg_tri_cases as tc
import test_hs_pg_abi as A
from test_gpu_hector_shift import hs_mod, ctx                              # noqa: F401 (fixtures)

gpu = pytest.mark.gpu
D = np.float64
FIELDS = ("chi2", "rz0", "rz", "cg_iters", "stopped")


def new_rep(hs_mod, ctx):
    return hs_mod.MapRepMultiMap(0.1, (64, 64), 2, ctx=ctx)


@contextlib.contextmanager
def tail_blocks(S):
    """The developer's S (read at every call; no result depends on it)."""
    old = os.environ.get("SLAMHIP_K22_TAIL")
    if S is not None:
        os.environ["SLAMHIP_K22_TAIL"] = str(S)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("SLAMHIP_K22_TAIL", None)
        else:
            os.environ["SLAMHIP_K22_TAIL"] = old


def same_iters(got, want):
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (got, want)


def device_equals_hook(hs_mod, rep, poses, fixed, ij, z, w, spec, seed=1):
    """_pg_set, _pg_tri_apply at the starting poses, _pg_relax_tri, _pg_get, _pg_residuals, _pg_tri_apply at the relaxed poses."""
    capi = hs_mod.capi
    lam = float(spec["lambda"][0])
    rhs = np.random.Generator(np.random.Philox(seed)).standard_normal((np.asarray(poses).reshape(-1, 3).shape[0], 3))
    hp, hit, hfin, hr, hc = capi.debug_pg_relax_tri(poses, fixed, ij, z, w, spec)
    rep.PgSet(poses, fixed, ij, z, w)
    z0 = rep.PgTriApply(lam, rhs)
    want0 = capi.debug_pg_tri_apply(poses, fixed, ij, z, w, lam, rhs)
    assert np.array_equal(z0, want0), np.abs(z0 - want0).max()
    it, fin = rep.PgRelax(spec, precond="tri")
    got = rep.PgGet()
    r, c2 = rep.PgResiduals()
    assert np.array_equal(got, hp), np.abs(got - hp).max()
    same_iters(it, hit)
    assert fin == hfin and np.array_equal(r, hr) and np.array_equal(c2, hc)
    assert np.array_equal(rep.PgTriApply(lam, rhs), capi.debug_pg_tri_apply(hp, fixed, ij, z, w, lam, rhs))
    return got, it, fin


# ---- 1. level edges --------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("N", tc.LEVEL_SIZES)
def test_level_edges(hs_mod, ctx, N):
    poses, ij, z, w = tc.level_case(N)
    rep = new_rep(hs_mod, ctx)
    got, it, fin = device_equals_hook(hs_mod, rep, poses, None, ij, z, w, hs_mod.capi.pg_spec(2, 30, check_every=4))
    if N >= 8:
        assert it[0]["stopped"] == 0 and 1 <= it[0]["cg_iters"] <= 26 and fin < it[0]["chi2"]      # L' = 2
    rep.close()


@gpu
@pytest.mark.parametrize("N,S", [(40, 4), (40, 16), (257, 4), (257, 16), (9, 1)])
def test_small_graphs_through_global_levels(hs_mod, ctx, N, S):
    poses, ij, z, w = tc.level_case(N)
    rep = new_rep(hs_mod, ctx)
    with tail_blocks(S):
        device_equals_hook(hs_mod, rep, poses, None, ij, z, w, hs_mod.capi.pg_spec(2, 30, check_every=3))
    rep.close()


@gpu
def test_chain_of_65537_with_three_loops(hs_mod, ctx):
    """One loop to node 0 (the closing edge) and two between free nodes: 13 iterations in exact arithmetic."""
    poses, ij, z, w = tc.chain_ring(65537, [(60000, 10), (30000, 3)], seed=5)
    rep = new_rep(hs_mod, ctx)
    got, it, fin = device_equals_hook(hs_mod, rep, poses, None, ij, z, w, hs_mod.capi.pg_spec(1, 40, check_every=7, tol=1e-6))
    print("65537 nodes: cg_iters %s, stopped %s, chi2 %.3f -> %.3f" % (it["cg_iters"].tolist(), it["stopped"].tolist(), it[0]["chi2"], fin))
    assert it[0]["stopped"] == 0 and 1 <= it[0]["cg_iters"] <= 26 and fin < it[0]["chi2"]
    rep.close()


# ---- 2. structure --------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", sorted(tc.structure_cases()))
def test_structures(hs_mod, ctx, name):
    poses, fixed, ij, z, w, lam = tc.structure_cases()[name]
    rep = new_rep(hs_mod, ctx)
    got, it, fin = device_equals_hook(hs_mod, rep, poses, fixed, ij, z, w, hs_mod.capi.pg_spec(3, 60, lam=lam))
    assert np.isfinite(got).all() and np.isfinite(fin) and all(np.isfinite(it[f]).all() for f in FIELDS)
    if name == "star":                                                     # T is block diagonal: slamhip_hs_pg_relax's counts and values (== ; a zero's sign may differ)
        rep.PgSet(poses, fixed, ij, z, w)
        jit, jfin = rep.PgRelax(hs_mod.capi.pg_spec(3, 60, lam=lam))
        assert it["cg_iters"].tolist() == jit["cg_iters"].tolist() and (jit["cg_iters"] > 0).all()
        assert np.array_equal(rep.PgGet(), got) and jfin == fin and all(np.array_equal(it[f], jit[f]) for f in FIELDS)
    rep.close()


# ---- 3. the call's life ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ring257():
    return tc.chain_ring(257, [(200, 10), (130, 3)], seed=7)


@gpu
def test_check_every_and_two_calls(hs_mod, ctx, ring257):
    capi = hs_mod.capi
    poses, ij, z, w = ring257
    rep = new_rep(hs_mod, ctx)
    ck = [rep.Maps[l].checksum() for l in range(2)]
    runs = []
    for every in (1, 3, 1024):
        rep.PgSet(poses, None, ij, z, w)
        it, fin = rep.PgRelax(capi.pg_spec(2, 1024, check_every=every), precond="tri")
        runs.append((rep.PgGet().tobytes(), it.tobytes(), fin))
    assert runs[0] == runs[1] == runs[2]
    rep.PgSet(poses, None, ij, z, w)
    six, fin6 = rep.PgRelax(capi.pg_spec(6, 64), precond="tri")
    p6 = rep.PgGet()
    rep.PgSet(poses, None, ij, z, w)
    a, _ = rep.PgRelax(capi.pg_spec(3, 64), precond="tri")
    b, fin33 = rep.PgRelax(capi.pg_spec(3, 64), precond="tri")             # a second call continues from the relaxed poses
    same_iters(np.concatenate([a, b]), six)
    assert fin33 == fin6 and np.array_equal(rep.PgGet(), p6)
    assert [rep.Maps[l].checksum() for l in range(2)] == ck                # the grids are not touched
    rep.close()


@gpu
def test_jacobi_then_tri_and_regrow(hs_mod, ctx, ring257):
    capi = hs_mod.capi
    poses, ij, z, w = ring257
    rep = new_rep(hs_mod, ctx)
    spec = capi.pg_spec(2, 40)
    rep.PgSet(poses, None, ij, z, w)
    jit, _ = rep.PgRelax(capi.pg_spec(1, 50))                              # block-Jacobi first: n_cg reached, the stop word left set
    mid = rep.PgGet()
    it, fin = rep.PgRelax(spec, precond="tri")
    hj = capi.debug_pg_relax(poses, None, ij, z, w, capi.pg_spec(1, 50))
    assert np.array_equal(mid, hj[0]) and jit.tobytes() == hj[1].tobytes()
    ht = capi.debug_pg_relax_tri(mid, None, ij, z, w, spec)
    assert np.array_equal(rep.PgGet(), ht[0]) and fin == ht[2]
    same_iters(it, ht[1])
    jit2, _ = rep.PgRelax(capi.pg_spec(1, 50))                             # ... and block-Jacobi behind tri is its own self
    assert jit2.tobytes() == capi.debug_pg_relax(ht[0], None, ij, z, w, capi.pg_spec(1, 50))[1].tobytes()
    # _pg_set twice with another N between tri calls: the levels' blocks regrow, and shrink in use
    for N in (40, 2 * tc.TAIL + 1, 9):
        g = tc.level_case(N)
        device_equals_hook(hs_mod, rep, g[0], None, g[1], g[2], g[3], spec)
    rep.close()


@gpu
def test_clear_reset_and_state(hs_mod, ctx):
    capi = hs_mod.capi
    rep = new_rep(hs_mod, ctx)
    spec = capi.pg_spec(1, 4)
    g = tc.level_case(9)
    for call in (lambda: rep.PgRelax(spec, precond="tri"), lambda: rep.PgTriApply(0.0, np.zeros((1, 3)))):
        with pytest.raises(capi.SlamhipError) as e:                        # before slamhip_hs_pg_set
            call()
        assert e.value.code == capi.ERR_STATE
    rep.PgSet(g[0], None, g[1], g[2], g[3])
    for kw in (dict(n_outer=0), dict(n_cg=0), dict(check_every=0), dict(reserved=1), dict(tol=-1.0), dict(lam=-1.0)):
        a = dict(n_outer=1, n_cg=4); a.update(kw)
        for precond in ("jacobi", "tri"):                                  # the refusals of slamhip_hs_pg_relax
            with pytest.raises(capi.SlamhipError) as e:
                rep.PgRelax(capi.pg_spec(**a), precond=precond)
            assert e.value.code == capi.ERR_INVALID, (kw, precond)
    with pytest.raises(capi.SlamhipError) as e:
        rep.PgTriApply(-1.0, np.zeros((9, 3)))
    assert e.value.code == capi.ERR_INVALID
    with pytest.raises(ValueError):
        rep.PgRelax(spec, precond="cholesky")
    device_equals_hook(hs_mod, rep, g[0], None, g[1], g[2], g[3], spec)
    rep.PgClear()
    with pytest.raises(capi.SlamhipError) as e:
        rep.PgRelax(spec, precond="tri")
    assert e.value.code == capi.ERR_STATE
    device_equals_hook(hs_mod, rep, g[0], None, g[1], g[2], g[3], spec)    # the blocks are made again
    rep.Reset()                                                            # slamhip_hs_reset drops the graph
    with pytest.raises(capi.SlamhipError) as e:
        rep.PgTriApply(0.0, np.zeros((9, 3)))
    assert e.value.code == capi.ERR_STATE
    rep.close()


# ---- 4. end to end -------------------------------------------------------------------------------------------------------------------
@gpu
def test_close_loops_with_tri(hs_mod, ctx):
    """K21's lap (tests/test_gpu_hector_scanmatch.py::test_end_to_end_lap): close_loops with precond="tri" accepts the loops that
    precond="jacobi" accepts from the same drifted store, and its largest keyframe position error is no worse -- an ordering, both
    numbers printed; the two solvers stop at the same minimum to far below the 1e-6 m allowed here (tol = 1e-8)."""
    import render_cases as rc
    import scanmatch_cases as sc
    import test_hs_scanmatch_abi as SM
    capi = hs_mod.capi
    L = rc.lap()
    N = len(L["scans"])
    true = L["true"].astype(D)
    proc = hs_mod.HectorSLAMProcessor(rc.LAP_CELL, rc.LAP_SIZE, (0.0, 0.0, 0.0), rc.LAP_LEVELS, ctx=ctx)
    try:
        proc.MapRep.SigConfigure(*rc.LAP_SIG)
        for i in range(N):
            proc.AddKeyframe(hs_mod.ScanCloud(L["scans"][i], (0.0, 0.0, 0.0)), L["drifted"][i], keep_scan=True)
        sp = capi.scanmatch_spec(**sc.LAP_SPEC)
        out = {}
        for precond in ("jacobi", "tri"):
            proc.MapRep.SigSetPoses(np.asarray(L["drifted"], np.float32))
            out[precond] = proc.close_loops(sc.LAP_MIN_GAP, sp, sc.accept, odom_w=rc.LAP_ODOM_W, precond=precond)
        closed = {k: [(o["pairs"][n][0], o["pairs"][n][1]) for n in range(len(o["pairs"])) if o["accepted"][n]] for k, o in out.items()}
        assert closed["tri"] == closed["jacobi"] and len(closed["tri"]) >= 1
        e_drift = SM.max_position_error(L["drifted"], true)
        e_jac, e_tri = SM.max_position_error(out["jacobi"]["poses"], true), SM.max_position_error(out["tri"]["poses"], true)
        print("loops %s; largest keyframe error: drifted %.3f m, block-Jacobi %.9f m, tri %.9f m; PCG iterations block-Jacobi %s, tri %s" %
              (closed["tri"], e_drift, e_jac, e_tri, out["jacobi"]["iters"]["cg_iters"].tolist(), out["tri"]["iters"]["cg_iters"].tolist()))
        assert e_tri < e_drift and e_tri <= e_jac + 1e-6
        assert int(out["tri"]["iters"]["cg_iters"].sum()) < int(out["jacobi"]["iters"]["cg_iters"].sum())
    finally:
        proc.Dispose()
