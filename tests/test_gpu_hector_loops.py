"""K23 on the device: slamhip_hs_loops_consistent through MapRepMultiMap / HectorSLAMProcessor, held to == against the host hook
(slamhip_debug_loops_consistent) on keep, deg, the info record and the whole matrix.  The cases: tests/loops_cases.py (each checked
on the CPU against a NumPy restatement by tests/test_hs_loops_abi.py)."""
import os

import numpy as np
import pytest

import loops_cases as lc
import render_cases as rc
import scanmatch_cases as sc
from test_gpu_hector import hs_mod, ctx                                  # noqa: F401 (fixtures)
from test_hs_loops_abi import hook, same, raw, refusals

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    import slam.net_amd.capi as capi
    return capi


@pytest.fixture(scope="module")
def rep(hs_mod, ctx):
    r = hs_mod.MapRepMultiMap(0.1, (64, 64), 2, ctx=ctx)
    yield r
    r.close()


def device(rep, capi, case, global_rows=False, **spec):
    """The device call; global_rows: k23_clique reads the matrix from global memory whatever L is (SLAMHIP_K23_GLOBAL is read at every call)."""
    old = os.environ.pop("SLAMHIP_K23_GLOBAL", None)
    try:
        if global_rows:
            os.environ["SLAMHIP_K23_GLOBAL"] = "1"
        return rep.LoopsConsistent(case["poses"], case["ij"], case["z"], case["w"], capi.loops_spec(**dict(case["spec"], **spec)), use=case["use"], adj=True)
    finally:
        os.environ.pop("SLAMHIP_K23_GLOBAL", None)
        if old is not None:
            os.environ["SLAMHIP_K23_GLOBAL"] = old


@pytest.mark.parametrize("name", sorted(lc.CASES) + ["first_non_resident"])
def test_case(rep, capi, name):
    case = lc.big_case(capi) if name == "first_non_resident" else lc.CASES[name]()
    want = hook(capi, case, adj=True)
    same(device(rep, capi, case), want, name)
    same(device(rep, capi, case, global_rows=True), want, (name, "rows from global memory"))
    plain = rep.LoopsConsistent(case["poses"], case["ij"], case["z"], case["w"], capi.loops_spec(**case["spec"]), use=case["use"])
    assert plain["adj"] is None and np.array_equal(plain["keep"], want["keep"]) and np.array_equal(plain["deg"], want["deg"])


@pytest.mark.parametrize("n_starts", [1, 2, 5, 21, 64])
def test_starts_and_launch_shape_change_nothing_else(rep, capi, n_starts):
    """One workgroup per start: 1, 2, 5, as many as there are edges, more than there are.  The matrix and the degrees do not depend
    on it; the winner is the hook's for the same n_starts; equal specs give equal bits across two calls and after LoopsClear."""
    case = lc.CASES["ring"]()
    want = hook(capi, dict(case, spec=dict(case["spec"], n_starts=n_starts)), adj=True)
    got = device(rep, capi, case, n_starts=n_starts)
    same(got, want, n_starts)
    assert int(got["info"]["n_starts"]) == min(n_starts, 21)
    rep.LoopsClear()
    rep.LoopsClear()                                                       # (never fails for an hs that has none)
    same(device(rep, capi, case, n_starts=n_starts), got, (n_starts, "after LoopsClear"))
    same(device(rep, capi, case, n_starts=n_starts, global_rows=True), got, (n_starts, "rows from global memory"))


def test_refusals_isolation_and_a_second_handle(hs_mod, ctx, capi):
    """The device call refuses what the hook refuses and writes nothing; a call leaves the map's checksum, the signature store, the
    scan store and the pose graph as they were; a second handle's unit and map are untouched."""
    case = lc.CASES["L65"]()
    a = hs_mod.MapRepMultiMap(0.1, (64, 64), 2, ctx=ctx)
    b = hs_mod.MapRepMultiMap(0.1, (64, 64), 2, ctx=ctx)
    try:
        for what, kw in refusals(capi):
            rcode, clean = raw(capi, "slamhip_hs_loops_consistent", a._h, **kw)
            assert rcode == capi.ERR_INVALID and clean, (what, rcode, clean)
        pts = sc.CASES["pairs_2"]()["scans"]
        for r in (a, b):
            r.UpdateByScan(hs_mod.ScanCloud(pts[0], (0.0, 0.0, 0.0)), (3.2, 3.2, 0.0))
            r.SigConfigure(*rc.LAP_SIG)
            r.set_scan(hs_mod.ScanCloud(pts[1], (0.0, 0.0, 0.0)))
            r.SigAdd((1.0, 2.0, 0.5))
            r.ScansAdd(hs_mod.ScanCloud(pts[0], (0.0, 0.0, 0.0)))
            r.PgSet([(0.0, 0.0, 0.0), (1.0, 0.0, 0.1)], None, [(0, 1)], [(1.0, 0.0, 0.0)], [(1.0, 1.0, 1.0)])

        def state(r):
            return ([r.Maps[l].checksum() for l in range(r.NumLevels)], r.SigDownload(), r.PgGet(), r.ScansGet(0), r.ScansCount())
        before = (state(a), state(b))
        want = hook(capi, case, adj=True)
        same(device(a, capi, case), want, "L65 on the first handle")
        ring = lc.CASES["ring"]()
        same(device(b, capi, ring), hook(capi, ring, adj=True), "ring on the second handle")
        same(device(a, capi, case), want, "L65 again on the first handle")
        after = (state(a), state(b))
        for s0, s1 in zip(before, after):
            assert s0[0] == s1[0] and s0[4] == s1[4]
            assert np.array_equal(s0[1][0], s1[1][0]) and np.array_equal(s0[1][1], s1[1][1]) and np.array_equal(s0[2], s1[2])
            assert np.array_equal(s0[3][0], s1[3][0]) and np.array_equal(s0[3][1], s1[3][1])
        a.Reset()                                                          # (slamhip_hs_reset leaves the unit's buffers alone: the next call just runs)
        same(device(a, capi, case), want, "after Reset")
    finally:
        a.close(); b.close()


def test_ring_through_the_processor(hs_mod, ctx, capi):
    """ConsistentLoops over the stored keyframe poses (binary32, as the store keeps them) == the hook on those poses and keeps exactly
    the 12 true loops; RelaxKeyframes with the kept edges then ends nearer the truth than the drifted chain."""
    case = lc.CASES["ring"]()
    proc = hs_mod.HectorSLAMProcessor(0.1, (64, 64), (0.0, 0.0, 0.0), 2, ctx=ctx)
    try:
        mr = proc.MapRep
        mr.SigConfigure(*rc.LAP_SIG)
        mr.SigUpload(np.zeros((200, rc.LAP_SIG[1]), np.uint64), case["poses"].astype(np.float32))
        stored = mr.SigDownload()[1].astype(np.float64)
        loops = [(int(case["ij"][n, 0]), int(case["ij"][n, 1]), case["z"][n], case["w"][n]) for n in range(21)]
        sp = capi.loops_spec(**case["spec"])
        got = proc.ConsistentLoops(loops, sp)
        want = hook(capi, dict(case, poses=stored))
        assert np.array_equal(got["keep"], want["keep"]) and np.array_equal(got["deg"], want["deg"]) and got["info"] == want["info"]
        assert np.array_equal(got["keep"], case["is_true"])
        kept = [l for l, k in zip(loops, got["keep"]) if k]
        poses, iters, chi2 = proc.RelaxKeyframes(kept, rc.LAP_ODOM_W, capi.pg_spec(6, 200, tol=1e-10), precond="tri")

        def err(p):
            return float(np.hypot(p[:, 0] - case["true"][:, 0], p[:, 1] - case["true"][:, 1]).max())
        print("largest translation error: drifted %.3f m, relaxed with the kept edges %.3f m" % (err(stored), err(poses)))
        assert err(poses) < err(stored)
    finally:
        proc.Dispose()


def test_close_loops_without_consistency_is_unchanged_and_with_it_filters(hs_mod, ctx, capi):
    """close_loops(consistency=None) on the lap of tests/test_gpu_hector_scanmatch.py returns the keys and the values of a call
    without the argument; with a spec the dict gains consistent and loops_info, and only kept edges are relaxed."""
    Lp = rc.lap()
    N = len(Lp["scans"])
    sp = capi.scanmatch_spec(**sc.LAP_SPEC)

    def run(**kw):
        proc = hs_mod.HectorSLAMProcessor(rc.LAP_CELL, rc.LAP_SIZE, (0.0, 0.0, 0.0), rc.LAP_LEVELS, ctx=ctx)
        try:
            proc.MapRep.SigConfigure(*rc.LAP_SIG)
            for i in range(N):
                proc.AddKeyframe(hs_mod.ScanCloud(Lp["scans"][i], (0.0, 0.0, 0.0)), Lp["drifted"][i], keep_scan=True)
            return proc.close_loops(sc.LAP_MIN_GAP, sp, sc.accept, odom_w=rc.LAP_ODOM_W, **kw)
        finally:
            proc.Dispose()
    base, none = run(), run(consistency=None)
    assert list(base.keys()) == list(none.keys()) == ["pairs", "results", "z", "w", "accepted", "poses", "iters", "chi2"]
    assert base["pairs"] == none["pairs"] and base["poses"] is not None
    for k in ("results", "z", "w", "accepted", "poses", "iters", "chi2"):
        assert np.array_equal(base[k], none[k]), k
    with_spec = run(consistency=capi.loops_spec(11.34, 1e-3, 1e-4, n_starts=8))
    assert list(with_spec.keys()) == list(base.keys()) + ["consistent", "loops_info"]
    assert np.array_equal(with_spec["accepted"], base["accepted"]) and not (with_spec["consistent"] & ~with_spec["accepted"]).any()
    assert int(with_spec["consistent"].sum()) == int(with_spec["loops_info"]["size"]) >= 1
    print("%d accepted, %d consistent" % (int(base["accepted"].sum()), int(with_spec["consistent"].sum())))
