"""The damped and robust relaxation of the pose graph (K26: slamhip_hs_pg_relax_lm, MapRepMultiMap.PgRelaxLM,
HectorSLAMProcessor.RelaxKeyframes(lm=...)) on the device, against the host hook slamhip_debug_pg_relax_lm, which
tests/test_hs_pg_lm_abi.py ties to the NumPy restatement of rules R1 - R4.  Everything is compared with == on the poses, every
slamhip_pg_lm_iter field, F_final and f; there is no tolerance anywhere but in the end-to-end case's bound on the false edge's factor.

Shapes are the smallest at which each path can go wrong (tests/pg_lm_cases.py): 1, 2 and 3 nodes, rule 6's and the lane-per-node
kernels' blocks at 255 .. 257 and 513 nodes, the lane-per-edge kernels' at 255 .. 257 edges, one edge with c_e == phi and one ulp
beside it, and the run's life: a first attempt rejected, lambda pinned at either bound, rule R3's stop, the three relax calls in turn."""
import ctypes as C

import numpy as np
import pytest

import pg_lm_cases as lc
from test_gpu_hector_pg_tri import new_rep, tail_blocks
from test_gpu_hector_shift import hs_mod, ctx                              # noqa: F401 (fixtures)

gpu = pytest.mark.gpu
D = np.float64
COMBOS = [(kind, precond) for kind in ("none", "dcs", "gm") for precond in ("jacobi", "tri")]


def same_iters(got, want):
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (got, want)


def device_equals_hook(hs_mod, rep, poses, fixed, ij, z, w, spec, robust=None, set_graph=True):
    """_pg_set (unless the graph stands: `poses` are then the ones it stands at), _pg_relax_lm, _pg_get against the hook."""
    hp, hit, hF, hf = hs_mod.capi.debug_pg_relax_lm(poses, fixed, ij, z, w, spec, robust)
    if set_graph:
        rep.PgSet(poses, fixed, ij, z, w)
    it, F, f = rep.PgRelaxLM(spec, robust)
    got = rep.PgGet()
    assert np.array_equal(got, hp), np.abs(got - hp).max()
    same_iters(it, hit)
    assert F == hF and np.array_equal(f, hf)
    return got, it, F, f


def robust_forms(E, n_chain):
    """NULL, all zero, the loops only, every second edge."""
    return {"null": None, "zero": np.zeros(E, bool), "loops": np.arange(E) >= n_chain, "second": np.arange(E) % 2 == 0}


# ---- 1. sizes ------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("N", [1, 2, 3, 255, 256, 257, 513])
def test_node_counts(hs_mod, ctx, N):
    capi = hs_mod.capi
    poses, ij, z, w = lc.noisy_ring(N)
    rep = new_rep(hs_mod, ctx)
    forms = robust_forms(ij.shape[0], N - 1)
    for n, (kind, precond) in enumerate(COMBOS):
        spec = capi.pg_lm_spec(3, 20, check_every=6, precond=precond, kind=kind, phi=2.0, lambda0=1e-2, tol=1e-8)
        device_equals_hook(hs_mod, rep, poses, None, ij, z, w, spec, forms[sorted(forms)[n % 4]])
    rep.close()


@gpu
@pytest.mark.parametrize("E", [255, 256, 257])
def test_edge_counts(hs_mod, ctx, E):
    capi = hs_mod.capi
    poses, ij, z, w = lc.noisy_ring(200, n_edges=E)
    rep = new_rep(hs_mod, ctx)
    for name, robust in robust_forms(E, 199).items():
        for kind, precond in (("dcs", "tri"), ("gm", "jacobi")):
            spec = capi.pg_lm_spec(3, 20, precond=precond, kind=kind, phi=2.0, lambda0=1e-2, tol=1e-8)
            _, it, _, f = device_equals_hook(hs_mod, rep, poses, None, ij, z, w, spec, robust)
            assert name != "zero" or (f == 1.0).all()
    rep.close()


@gpu
@pytest.mark.parametrize("ulps", [-1, 0, 1])
def test_one_edge_at_phi(hs_mod, ctx, ulps):
    """r = (0.5, 0, 0) and wx = 4: c_e == phi == 1 exactly, and one ulp either side of it."""
    capi = hs_mod.capi
    poses, ij, z, w = lc.one_edge(ulps)
    rep = new_rep(hs_mod, ctx)
    for kind, precond in COMBOS:
        _, it, _, _ = device_equals_hook(hs_mod, rep, poses, None, ij, z, w, capi.pg_lm_spec(2, 5, precond=precond, kind=kind, phi=1.0))
        if ulps == 0 and kind != "gm":
            assert it[0]["F"] == 1.0
    rep.close()


# ---- 2. the run's life -----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("precond", ["jacobi", "tri"])
def test_ring_a_rejections_and_bounds(hs_mod, ctx, precond):
    capi = hs_mod.capi
    start, ij, z, w, _ = lc.ring_a(64, 0.03)
    rep = new_rep(hs_mod, ctx)
    kw = dict(precond=precond, tol=1e-8)
    _, it, _, _ = device_equals_hook(hs_mod, rep, start, None, ij, z, w, capi.pg_lm_spec(3, 256, lambda0=0.0, **kw))
    assert it["accepted"].tolist() == [0, 0, 0] and (it["lambda"] == 0.0).all()        # plain Gauss-Newton raises the cost: 0 * up stays 0
    got, it, F, _ = device_equals_hook(hs_mod, rep, start, None, ij, z, w, capi.pg_lm_spec(4, 256, lambda0=1e-3, lambda_max=1e-2, **kw))
    assert it["accepted"].tolist() == [0, 0, 0, 0] and it[0]["lambda"] == 1e-3 and (it["lambda"][2:] == 1e-2).all()   # spent on rejections, pinned above
    assert np.array_equal(got, start) and F == it[0]["F"] and (it["F"] == F).all()
    _, it, _, _ = device_equals_hook(hs_mod, rep, start, None, ij, z, w, capi.pg_lm_spec(8, 256, lambda0=1e-3, **kw))
    assert it[0]["accepted"] == 0 and it["accepted"].any() and (np.diff(it["F"]) <= 0).all()
    poses, ij, z, w = lc.noisy_ring(64)
    _, it, _, _ = device_equals_hook(hs_mod, rep, poses, None, ij, z, w, capi.pg_lm_spec(4, 256, lambda0=1.0, lambda_min=0.5, down=0.1, **kw))
    assert it["accepted"][:2].tolist() == [1, 1] and it["lambda"][:3].tolist() == [1.0, 0.5, 0.5]            # pinned below
    rep.close()


@gpu
def test_ftol_stop_leaves_later_records(hs_mod, ctx):
    capi = hs_mod.capi
    poses, ij, z, w = lc.noisy_ring(64)
    rep = new_rep(hs_mod, ctx)
    spec = capi.pg_lm_spec(5, 256, precond="tri", lambda0=0.0, ftol=1e-3, tol=1e-8)
    _, it, _, _ = device_equals_hook(hs_mod, rep, poses, None, ij, z, w, spec)
    n = len(it)
    assert 1 <= n < 5 and it[-1]["accepted"] == 1 and (it[-1]["F"] - it[-1]["F_trial"]) <= 1e-3 * it[-1]["F"]
    rep.PgSet(poses, None, ij, z, w)
    raw = np.full(5 * 8, -7.25, D); cnt = C.c_int32(-7); fin = C.c_double(0.0)
    capi.call("slamhip_hs_pg_relax_lm", rep._h, spec.ctypes.data_as(C.c_void_p), None, raw.ctypes.data_as(C.c_void_p), C.byref(cnt), C.byref(fin), None)
    assert cnt.value == n and (raw[8 * n:] == -7.25).all() and raw[:8 * n].tobytes() == it.tobytes()
    rep.close()


@gpu
def test_check_every_and_two_calls(hs_mod, ctx):
    capi = hs_mod.capi
    start, ij, z, w, _, rb = lc.graph_b()
    rep = new_rep(hs_mod, ctx)
    for precond in ("jacobi", "tri"):
        runs = []
        for every in (1, 7, 64):
            rep.PgSet(start, None, ij, z, w)
            it, F, f = rep.PgRelaxLM(capi.pg_lm_spec(4, 100, check_every=every, precond=precond, kind="dcs", tol=1e-8), rb)
            runs.append((rep.PgGet().tobytes(), it.tobytes(), F, f.tobytes()))
        assert runs[0] == runs[1] == runs[2]
    spec = capi.pg_lm_spec(3, 100, precond="tri", kind="dcs", tol=1e-8)
    mid, _, _, _ = device_equals_hook(hs_mod, rep, start, None, ij, z, w, spec, rb)
    device_equals_hook(hs_mod, rep, mid, None, ij, z, w, spec, rb, set_graph=False)                  # a second call continues, lambda from lambda0 again
    rep.close()


@gpu
def test_three_relax_kinds_in_turn(hs_mod, ctx):
    """LM, slamhip_hs_pg_relax, _relax_tri, LM on one graph: each equals its hook continued from the poses the one before left."""
    capi = hs_mod.capi
    start, ij, z, w, _, rb = lc.graph_b()
    rep = new_rep(hs_mod, ctx)
    lm = capi.pg_lm_spec(3, 80, precond="jacobi", kind="gm", tol=1e-8)
    p1, _, _, _ = device_equals_hook(hs_mod, rep, start, None, ij, z, w, lm, rb)
    old = capi.pg_spec(1, 80, lam=0.5, tol=1e-8)
    for precond, hook in (("jacobi", capi.debug_pg_relax), ("tri", capi.debug_pg_relax_tri)):
        it, fin = rep.PgRelax(old, precond=precond)
        want = hook(p1, None, ij, z, w, old)
        p1 = rep.PgGet()
        assert np.array_equal(p1, want[0]) and it.tobytes() == want[1].tobytes() and fin == want[2]
    device_equals_hook(hs_mod, rep, p1, None, ij, z, w, capi.pg_lm_spec(3, 80, precond="tri", kind="dcs", tol=1e-8), rb, set_graph=False)
    rep.close()


@gpu
@pytest.mark.parametrize("S", [4, 16])
def test_small_tail(hs_mod, ctx, S):
    """N = 257 through several global levels of the chain's solve (the developer's SLAMHIP_K22_TAIL, read at every call)."""
    poses, ij, z, w = lc.noisy_ring(257)
    rep = new_rep(hs_mod, ctx)
    with tail_blocks(S):
        device_equals_hook(hs_mod, rep, poses, None, ij, z, w, hs_mod.capi.pg_lm_spec(3, 30, check_every=3, precond="tri", kind="dcs", phi=2.0, tol=1e-8),
                           np.arange(ij.shape[0]) >= 256)
    rep.close()


@gpu
def test_refusals_and_state(hs_mod, ctx):
    capi = hs_mod.capi
    rep = new_rep(hs_mod, ctx)
    poses, ij, z, w = lc.noisy_ring(9)
    with pytest.raises(capi.SlamhipError) as e:                            # before slamhip_hs_pg_set
        rep.PgRelaxLM(capi.pg_lm_spec(1, 4))
    assert e.value.code == capi.ERR_STATE
    rep.PgSet(poses, None, ij, z, w)
    for kw in (dict(n_outer=0), dict(n_cg=0), dict(check_every=0), dict(precond=2), dict(kind=3), dict(reserved=1), dict(lambda0=-1.0), dict(up=1.0), dict(down=0.0),
               dict(lambda_min=2.0, lambda_max=1.0), dict(tol=-1.0), dict(ftol=-1.0), dict(kind="dcs", phi=0.0)):
        a = dict(n_outer=1, n_cg=4); a.update(kw)
        raw = np.full(8, -7.25, D); cnt = C.c_int32(-7); fin = C.c_double(-7.25); f = np.full(ij.shape[0], -7.25, D)
        rc = capi.lib().slamhip_hs_pg_relax_lm(rep._h, capi.pg_lm_spec(**a).ctypes.data_as(C.c_void_p), None, raw.ctypes.data_as(C.c_void_p), C.byref(cnt), C.byref(fin),
                                               f.ctypes.data_as(C.c_void_p))
        assert rc == capi.ERR_INVALID and (raw == -7.25).all() and cnt.value == -7 and fin.value == -7.25 and (f == -7.25).all(), kw
    assert np.array_equal(rep.PgGet(), poses)                              # nothing was launched
    spec = capi.pg_lm_spec(2, 20, precond="tri", kind="dcs")
    device_equals_hook(hs_mod, rep, poses, None, ij, z, w, spec)
    rep.PgClear()
    with pytest.raises(capi.SlamhipError) as e:
        rep.PgRelaxLM(spec)
    assert e.value.code == capi.ERR_STATE
    device_equals_hook(hs_mod, rep, poses, None, ij, z, w, spec)           # the blocks are made again
    big = lc.noisy_ring(513)
    device_equals_hook(hs_mod, rep, big[0], None, big[1], big[2], big[3], spec)          # ... and grow with the graph
    rep.Reset()                                                            # slamhip_hs_reset drops the graph
    with pytest.raises(capi.SlamhipError) as e:
        rep.PgRelaxLM(spec)
    assert e.value.code == capi.ERR_STATE
    rep.close()


# ---- 3. end to end -------------------------------------------------------------------------------------------------------------------
@gpu
def test_relax_keyframes_with_a_false_loop(hs_mod, ctx):
    """Graph B's nodes, start and loops through RelaxKeyframes(lm=...): 64 keyframes whose stored poses are the dead-reckoned start, the
    three loops with the last one's measurement corrupted.  (RelaxKeyframes forms the odometry edges from the STORED poses, so the
    chain's measurements are the start's, not the truth's, and at these weights DCS scales all three loops down: the case checks the
    path, not graph B's accuracy bound, which tests/test_hs_pg_lm_abi.py holds the hook to.)  Asserted: device ==
    hook over the same graph, the false edge's factor below 1e-2, the chain edges' factors 1, the store holds the relaxed poses, and
    lm=None is the call it was."""
    import test_hs_sig_abi as S
    capi = hs_mod.capi
    start, ij, z, w, true, rb = lc.graph_b()
    N = start.shape[0]
    scans = S.sim_lap()[3]
    proc = hs_mod.HectorSLAMProcessor(0.1, (256, 256), (0.0, 0.0, 0.0), 2, ctx=ctx)
    try:
        proc.MapRep.SigConfigure(S.SIM_SCALE, S.SIM_RINGS, S.SIM_RC)
        for i in range(N):
            proc.AddKeyframe(hs_mod.ScanCloud(scans[i % len(scans)], (0.0, 0.0, 0.0)), start[i].astype(np.float32))
        proc.MapRep.SigSetPoses(start.astype(np.float32))
        p0 = proc.MapRep.SigDownload()[1].astype(D)
        loops = [(int(ij[e, 0]), int(ij[e, 1]), z[e], lc.W_RING) for e in range(N - 1, ij.shape[0])]
        lm = capi.pg_lm_spec(30, 4 * N, precond="tri", kind="dcs", phi=1.0, tol=1e-8)
        out, iters, chi2, f = proc.RelaxKeyframes(loops, lc.W_RING, None, lm=lm)
        zz = np.array([capi.pg_edge_between(p0[k], p0[k + 1]) for k in range(N - 1)] + [l[2] for l in loops])
        hp, hit, _, hf = capi.debug_pg_relax_lm(p0, None, ij, zz, w, lm, rb)
        assert np.array_equal(out, hp) and np.array_equal(f, hf) and chi2.shape == f.shape == (ij.shape[0],)
        same_iters(iters, hit)
        print("false edge: f %.3g, chi2 %.4g; true loops: f %s; attempts %d, accepted %d" % (f[-1], chi2[-1], f[-3:-1].tolist(), len(iters), int(iters["accepted"].sum())))
        assert f[-1] < 1e-2 and (f[:N - 1] == 1.0).all()
        assert np.array_equal(proc.MapRep.SigDownload()[1], out.astype(np.float32))
        proc.MapRep.SigSetPoses(start.astype(np.float32))
        spec = capi.pg_spec(2, 4 * N, tol=1e-8)
        plain = proc.RelaxKeyframes(loops, lc.W_RING, spec, precond="tri")
        want = capi.debug_pg_relax_tri(p0, None, ij, zz, w, spec)
        assert len(plain) == 3 and np.array_equal(plain[0], want[0]) and plain[1].tobytes() == want[1].tobytes()
    finally:
        proc.Dispose()
