"""Marginal covariances of the pose graph (K27: slamhip_hs_pg_marginals, MapRepMultiMap.PgMarginals,
HectorSLAMProcessor.KeyframeCovariances / LoopMahalanobis) on the device, against the host hook slamhip_debug_pg_marginals, which
tests/test_hs_pg_marg_abi.py ties to the NumPy restatement of rules M1 - M5.  Blocks, records and info are compared by their bytes;
there is no tolerance anywhere but in the end-to-end case's ordering.

Shapes are the catalogue's (tests/pg_marg_cases.py): N = 1, 2, 3, rule 6's blocks 255 .. 257 per right-hand side, a chain in segments
with a dead node, duplicates and a reversed edge, lambda 0 and > 0, R = 0, 3, 6, 9, 12 and 21 right-hand sides and chunks of 1, 2, 3, 4,
5 and 9 for both instantiated groups, both preconditioners, SLAMHIP_K22_TAIL = 4 (37 and 257 nodes through global levels)."""
import contextlib
import os

import numpy as np
import pytest

import pg_lm_cases as lc
import pg_marg_cases as mc
from test_gpu_hector_pg_tri import new_rep, tail_blocks
from test_gpu_hector_shift import hs_mod, ctx                              # noqa: F401 (fixtures)

gpu = pytest.mark.gpu
D = np.float64
CASES = mc.cases()


@contextlib.contextmanager
def group(G):
    """The developer's G (read at every call; no result depends on it)."""
    old = os.environ.get("SLAMHIP_K27_GROUP")
    os.environ["SLAMHIP_K27_GROUP"] = str(G)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("SLAMHIP_K27_GROUP", None)
        else:
            os.environ["SLAMHIP_K27_GROUP"] = old


def spec_of(capi, c, pc, **kw):
    return capi.pg_marg_spec(kw.pop("n_cg", c["n_cg"][pc[1]]), precond=pc[0], lam=c["lam"], tol=c["tol"], **kw)


def same(got, want):
    for g, w, what in zip(got, want, ("blocks", "cols", "info")):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, g, w)


def device_equals_hook(hs_mod, rep, c, pc, **kw):
    capi = hs_mod.capi
    spec = spec_of(capi, c, pc, **kw)
    rep.PgSet(c["poses"], c["fixed"], c["ij"], c["z"], c["w"])
    got = rep.PgMarginals(c["pairs"], spec)
    same(got, capi.debug_pg_marginals(c["poses"], c["fixed"], c["ij"], c["z"], c["w"], spec, c["pairs"]))
    return got


# ---- 1. device == hook -----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("G", mc.GROUPS)
@pytest.mark.parametrize("pc", mc.PRECONDS, ids=lambda p: p[0])
@pytest.mark.parametrize("name", sorted(CASES))
def test_catalogue(hs_mod, ctx, name, pc, G):
    rep = new_rep(hs_mod, ctx)
    with group(G):
        blocks, cols, info = device_equals_hook(hs_mod, rep, CASES[name], pc)
    assert info["group"] == G and np.isfinite(blocks).all()
    rep.close()


@gpu
@pytest.mark.parametrize("G", mc.GROUPS)
@pytest.mark.parametrize("name", ["chain37", "ring257"])
def test_small_graphs_through_global_levels(hs_mod, ctx, name, G):
    rep = new_rep(hs_mod, ctx)
    with tail_blocks(4), group(G):
        device_equals_hook(hs_mod, rep, CASES[name], ("tri", 1), check_every=3)
    rep.close()


@gpu
@pytest.mark.parametrize("G", mc.GROUPS)
@pytest.mark.parametrize("pc", mc.PRECONDS, ids=lambda p: p[0])
@pytest.mark.parametrize("name", ["segments", "ring256"])
def test_chunks_and_check_every(hs_mod, ctx, name, pc, G):
    """max_bytes giving R_c = 1, 2, 3, 4, 5, 9 and R; check_every = 1 and large: all equal under ==, n_chunks as expected."""
    c = CASES[name]
    capi = hs_mod.capi
    rep = new_rep(hs_mod, ctx)
    B = mc.rhs_bytes(c["poses"].shape[0], pc[1])
    with group(G):
        base = device_equals_hook(hs_mod, rep, c, pc)
        R = int(base[2]["n_rhs"])
        assert base[2]["rhs_per_chunk"] == R and base[2]["n_chunks"] == 1
        for Rc in mc.CHUNKS + (R,):
            got = rep.PgMarginals(c["pairs"], spec_of(capi, c, pc, max_bytes=Rc * B, check_every=1 if Rc & 1 else 1000))
            assert got[0].tobytes() == base[0].tobytes() and got[1].tobytes() == base[1].tobytes()
            assert got[2]["rhs_per_chunk"] == min(Rc, R) and got[2]["n_chunks"] == -(-R // min(Rc, R)) and got[2]["group"] == G
        with pytest.raises(capi.SlamhipError) as e:
            rep.PgMarginals(c["pairs"], spec_of(capi, c, pc, max_bytes=B - 1))
        assert e.value.code == capi.ERR_NOMEM
        same(rep.PgMarginals(c["pairs"], spec_of(capi, c, pc)), base)
    rep.close()


# ---- 2. state ----------------------------------------------------------------------------------------------------------------------------
@gpu
def test_marginals_leave_the_graph_as_it_was(hs_mod, ctx):
    """PgGet is unchanged; PgRelax, PgRelaxLM and PgRelax(precond="tri") return the bits of a fresh handle that never asked; a second
    call equals the first; a second handle gives the same; PgClear, then ERR_STATE."""
    capi = hs_mod.capi
    c = CASES["ring255"]
    g = (c["poses"], c["fixed"], c["ij"], c["z"], c["w"])
    relax = [lambda r: r.PgRelax(capi.pg_spec(2, 40, tol=1e-8)), lambda r: r.PgRelaxLM(capi.pg_lm_spec(3, 40, precond="tri", tol=1e-8)),
             lambda r: r.PgRelax(capi.pg_spec(2, 40, tol=1e-8), precond="tri")]
    asked = new_rep(hs_mod, ctx); fresh = new_rep(hs_mod, ctx)
    first = None
    for pc in mc.PRECONDS:
        for run in relax:
            asked.PgSet(*g); fresh.PgSet(*g)
            m1 = asked.PgMarginals(c["pairs"], spec_of(capi, c, pc))
            assert np.array_equal(asked.PgGet(), c["poses"])
            same(asked.PgMarginals(c["pairs"], spec_of(capi, c, pc)), m1)
            a, f = run(asked), run(fresh)
            assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, f))
            assert np.array_equal(asked.PgGet(), fresh.PgGet())
            if pc[0] == "tri" and first is None:
                first = m1
    fresh.PgSet(*g)
    same(fresh.PgMarginals(c["pairs"], spec_of(capi, c, ("tri", 1))), first)
    with pytest.raises(capi.SlamhipError) as e:
        fresh.PgMarginals([(0, 300)], spec_of(capi, c, ("tri", 1)))
    assert e.value.code == capi.ERR_INVALID
    fresh.PgClear()
    with pytest.raises(capi.SlamhipError) as e:
        fresh.PgMarginals(c["pairs"], spec_of(capi, c, ("tri", 1)))
    assert e.value.code == capi.ERR_STATE
    asked.close(); fresh.close()


# ---- 3. end to end ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_keyframe_covariances_and_loop_mahalanobis(hs_mod, ctx):
    """64 keyframes (graph B of the K26 tests: its dead-reckoned start and its loops).  KeyframeCovariances' blocks equal the hook's over
    the graph RelaxKeyframes forms, rel equals capi.pg_relative_covariance of them, the store and RelaxKeyframes are as they were; a loop
    edge whose measurement is the stored poses' own relative pose has d2 = 0 up to rounding, the same edge shifted by 40 sigma in x a
    d2 beyond a 3 sigma gate (16.3 from the hook's blocks: 30 odometry steps lie between the two keyframes), which the device's equals."""
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
        loops = [(int(ij[e, 0]), int(ij[e, 1]), z[e], lc.W_RING) for e in range(N - 1, ij.shape[0] - 1)]     # graph B's two true loops
        pairs = [(5, 40), (40, 5), (63, 63), (0, 9)]
        spec = capi.pg_marg_spec(6 * len(loops) + 1, precond="tri", tol=1e-10)
        cov = proc.KeyframeCovariances(pairs, lc.W_RING, loops=loops, spec=spec)
        e2 = ij[:N - 1 + len(loops)]
        zz = np.array([capi.pg_edge_between(p0[k], p0[k + 1]) for k in range(N - 1)] + [l[2] for l in loops])
        ask = [(a, b) for i, j in pairs for a, b in ((i, i), (i, j), (j, i), (j, j))]
        hb, hc, hi = capi.debug_pg_marginals(p0, None, e2, zz, w[:e2.shape[0]], spec, ask)
        assert cov["blocks"].tobytes() == hb.tobytes() and cov["cols"].tobytes() == hc.tobytes() and cov["info"].tobytes() == hi.tobytes()
        q = hb.reshape(-1, 2, 2, 3, 3)
        for k, (i, j) in enumerate(pairs):
            assert np.array_equal(cov["rel"][k], capi.pg_relative_covariance(p0[i], p0[j], q[k, 0, 0], q[k, 0, 1], q[k, 1, 0], q[k, 1, 1]))
        assert not cov["rel"][3].any() or np.isfinite(cov["rel"]).all()
        assert np.array_equal(proc.MapRep.SigDownload()[1].astype(D), p0)
        i, j = 20, 50
        zt = np.array(capi.pg_edge_between(p0[i], p0[j]))
        sig = 1.0 / np.sqrt(np.asarray(lc.W_RING, D))
        hb2 = capi.debug_pg_marginals(p0, None, e2, zz, w[:e2.shape[0]], spec, [(i, i), (i, j), (j, i), (j, j)])[0]
        want_d2 = capi.pg_mahalanobis([40 * sig[0], 0.0, 0.0], capi.pg_relative_covariance(p0[i], p0[j], *hb2), lc.W_RING)
        d2, _ = proc.LoopMahalanobis([(i, j, zt, lc.W_RING), (i, j, zt + np.array([40 * sig[0], 0.0, 0.0]), lc.W_RING)], lc.W_RING, accepted=loops, spec=spec)
        print("LoopMahalanobis: d2 true %.3g, shifted by 40 sigma %.3g" % (d2[0], d2[1]))
        assert d2[0] < 1e-6 and d2[1] > 9.0 and np.isclose(d2[1], want_d2, rtol=1e-9)
        plain = proc.RelaxKeyframes(loops, lc.W_RING, capi.pg_spec(2, 4 * N, tol=1e-8), precond="tri")
        want = capi.debug_pg_relax_tri(p0, None, e2, zz, w[:e2.shape[0]], capi.pg_spec(2, 4 * N, tol=1e-8))
        assert np.array_equal(plain[0], want[0]) and plain[1].tobytes() == want[1].tobytes()
    finally:
        proc.Dispose()
