"""K21 on the device: slamhip_hs_scans_match through MapRepMultiMap / HectorSLAMProcessor, held to == against the host hook
(slamhip_debug_scans_match) on every field of every result.  The cases: tests/scanmatch_cases.py (each checked on the CPU against a
NumPy restatement by tests/test_hs_scanmatch_abi.py)."""
import os

import numpy as np
import pytest

import render_cases as rc
import scanmatch_cases as sc
from test_gpu_hector import hs_mod, ctx                                  # noqa: F401 (fixtures)
from test_hs_scanmatch_abi import lap_relax, max_position_error

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    import slam.net_amd.capi as capi
    return capi


def same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for f in got.dtype.names:
        bad = np.flatnonzero(got[f] != want[f])
        assert bad.size == 0, (what, f, bad[:8], got[f][bad[:8]], want[f][bad[:8]])


def make(hs_mod, ctx, scans):
    rep = hs_mod.MapRepMultiMap(0.1, (64, 64), 2, ctx=ctx)
    for i, s in enumerate(scans):
        assert rep.ScansAdd(hs_mod.ScanCloud(s, (0.0, 0.0, 0.0))) == i
    return rep


def device(rep, capi, case, pairs=None):
    """The device call with the case's headings per workgroup (SLAMHIP_K21_HEADINGS is read at every call)."""
    old = os.environ.pop("SLAMHIP_K21_HEADINGS", None)
    try:
        if case.get("headings"):
            os.environ["SLAMHIP_K21_HEADINGS"] = str(case["headings"])
        return rep.scans_match(capi.scanmatch_spec(**case["spec"]), case["pairs"] if pairs is None else pairs)
    finally:
        os.environ.pop("SLAMHIP_K21_HEADINGS", None)
        if old is not None:
            os.environ["SLAMHIP_K21_HEADINGS"] = old


def hook(capi, case, pairs=None, scans=None):
    return capi.debug_scans_match(case["scans"] if scans is None else scans, capi.scanmatch_spec(**case["spec"]), case["pairs"] if pairs is None else pairs)


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_case(hs_mod, ctx, capi, name):
    case = sc.CASES[name]()
    rep = make(hs_mod, ctx, case["scans"])
    try:
        want = hook(capi, case)
        same(device(rep, capi, case), want, name)
        same(device(rep, capi, case), want, (name, "the same list again: keys and sums at rest between calls"))
    finally:
        rep.close()


@pytest.mark.parametrize("headings", [1, 2, 3, 7, 64])
def test_headings_per_workgroup_change_nothing(hs_mod, ctx, capi, headings):
    """Seven headings cut into blocks of 1, 2 (uneven: 2, 2, 2, 1), 3 (3, 3, 1), 7 and more than there are."""
    case = dict(sc.CASES["uneven_heading_blocks"](), headings=headings)
    rep = make(hs_mod, ctx, case["scans"])
    try:
        same(device(rep, capi, case), hook(capi, case), headings)
    finally:
        rep.close()


def test_pair_lists_store_growth_reset_and_processor(hs_mod, ctx, capi):
    """Lists of 1, 2 and 65 pairs on one handle; the processor's pass-through; the pool grown past its first 65536 points by
    doubling (the stored scans keep their points); after slamhip_hs_reset the empty store is SLAMHIP_ERR_STATE."""
    case = sc.CASES["pairs_65_one_reference"]()
    proc = hs_mod.HectorSLAMProcessor(0.1, (64, 64), (0.0, 0.0, 0.0), 2, ctx=ctx)
    try:
        rep = proc.MapRep
        for s in case["scans"]:
            rep.ScansAdd(hs_mod.ScanCloud(s, (0.0, 0.0, 0.0)))
        want = hook(capi, case)
        for n in (1, 2, 65):
            same(device(rep, capi, case, case["pairs"][:n]), want[:n], ("pairs", n))
        same(proc.scans_match(capi.scanmatch_spec(**case["spec"]), case["pairs"]), want, "processor")
        big = sc.CASES["scans_2049"]()["scans"]
        scans = list(case["scans"])
        for i in range(34):                                                # 9 x 48 + 34 x 2049 = 70098 points: past 65536
            scans.append(big[i % 2]); rep.ScansAdd(hs_mod.ScanCloud(big[i % 2], (0.0, 0.0, 0.0)))
        n = len(scans)
        pairs = case["pairs"][:3] + [(n - 2, n - 1, (0.0, 0.0, 0.0)), (0, n - 1, (0.25, 0.0, 0.0)), (n - 1, 3, (0.0, -0.25, 0.0))]
        same(device(rep, capi, case, pairs), hook(capi, case, pairs, scans), "after the pool grew")
        rep.Reset()
        assert rep.ScansCount() == 0
        with pytest.raises(capi.SlamhipError) as e:
            device(rep, capi, case, case["pairs"][:1])
        assert e.value.code == capi.ERR_STATE
    finally:
        proc.Dispose()


def test_refusals_and_isolation(hs_mod, ctx, capi):
    """The device call refuses what the hook refuses; a call leaves the map's checksum, the signature store and the pose graph as
    they were."""
    case = sc.CASES["pairs_2"]()
    rep = hs_mod.MapRepMultiMap(0.1, (64, 64), 2, ctx=ctx)
    try:
        sp = capi.scanmatch_spec(**case["spec"])
        with pytest.raises(capi.SlamhipError) as e:
            rep.scans_match(sp, case["pairs"])
        assert e.value.code == capi.ERR_STATE                               # no store at all
        for s in case["scans"]:
            rep.ScansAdd(hs_mod.ScanCloud(s, (0.0, 0.0, 0.0)))
        for bad in (dict(half=24), dict(nx=65), dict(scale=0.0), dict(reserved=1), dict(margin=-1)):
            with pytest.raises(capi.SlamhipError) as e:
                rep.scans_match(capi.scanmatch_spec(**dict(case["spec"], **bad)), case["pairs"])
            assert e.value.code == capi.ERR_INVALID, bad
        for pairs in ([(0, 3, (0.0, 0.0, 0.0))], [(-1, 0, (0.0, 0.0, 0.0))], [(0, 1, (float("nan"), 0.0, 0.0))]):
            with pytest.raises(capi.SlamhipError) as e:
                rep.scans_match(sp, pairs)
            assert e.value.code == capi.ERR_INVALID, pairs
        rep.UpdateByScan(hs_mod.ScanCloud(case["scans"][0], (0.0, 0.0, 0.0)), (3.2, 3.2, 0.0))
        rep.SigConfigure(*rc.LAP_SIG)
        rep.set_scan(hs_mod.ScanCloud(case["scans"][1], (0.0, 0.0, 0.0)))
        rep.SigAdd((1.0, 2.0, 0.5))
        rep.PgSet([(0.0, 0.0, 0.0), (1.0, 0.0, 0.1)], None, [(0, 1)], [(1.0, 0.0, 0.0)], [(1.0, 1.0, 1.0)])
        before = ([rep.Maps[l].checksum() for l in range(rep.NumLevels)], rep.SigDownload(), rep.PgGet())
        same(rep.scans_match(sp, case["pairs"]), hook(capi, case), "pairs_2")
        after = ([rep.Maps[l].checksum() for l in range(rep.NumLevels)], rep.SigDownload(), rep.PgGet())
        assert before[0] == after[0]
        assert np.array_equal(before[1][0], after[1][0]) and np.array_equal(before[1][1], after[1][1]) and np.array_equal(before[2], after[2])
    finally:
        rep.close()


def test_end_to_end_lap(hs_mod, ctx, capi):
    """The lap of tests/test_hs_scanmatch_abi.py on the device, with NO ground-truth edge: the keyframes stored at the drifted poses,
    HectorSLAMProcessor.close_loops -- candidates from slamhip_hs_sig_self, edges from slamhip_hs_scans_match alone, accepted by
    scanmatch_cases.accept -- then the render at the relaxed poses.  Each device result == the hook's.  Two orderings, no threshold:
    the largest keyframe position error is smaller relaxed than drifted, and the relaxed render differs from the true render in
    fewer cells than the drifted render does."""
    L = rc.lap()
    N = len(L["scans"])
    true = L["true"].astype(np.float64)
    proc = hs_mod.HectorSLAMProcessor(rc.LAP_CELL, rc.LAP_SIZE, (0.0, 0.0, 0.0), rc.LAP_LEVELS, ctx=ctx)
    try:
        rep = proc.MapRep
        rep.SigConfigure(*rc.LAP_SIG)
        for i in range(N):
            proc.AddKeyframe(hs_mod.ScanCloud(L["scans"][i], (0.0, 0.0, 0.0)), L["drifted"][i], keep_scan=True)
        cells = {}
        for name, poses in (("true", L["true"]), ("drifted", L["drifted"])):
            proc.RenderKeyframes(poses)
            cells[name] = rep.Maps[0].GetCells()
        sp = capi.scanmatch_spec(**sc.LAP_SPEC)
        out = proc.close_loops(sc.LAP_MIN_GAP, sp, sc.accept, odom_w=rc.LAP_ODOM_W, render=True)
        cells["relaxed"] = rep.Maps[0].GetCells()
        same(out["results"], capi.debug_scans_match(L["scans"], sp, out["pairs"]), "lap")
        loops = [(out["pairs"][n][0], out["pairs"][n][1], out["z"][n], out["w"][n]) for n in range(len(out["pairs"])) if out["accepted"][n]]
        print("%d candidates, %d accepted: %s" % (len(out["pairs"]), len(loops), [(l[0], l[1]) for l in loops]))
        assert loops and out["poses"] is not None
        assert np.array_equal(out["poses"], lap_relax(capi, L, loops))     # the device's relaxation == the hook's on the same edges
        e_drift, e_relax = max_position_error(L["drifted"], true), max_position_error(out["poses"], true)
        d_drift, d_relax = rc.sym_diff(cells["drifted"], cells["true"]), rc.sym_diff(cells["relaxed"], cells["true"])
        print("largest keyframe error: drifted %.3f m, relaxed %.3f m; cells that differ from the true render: drifted %d, relaxed %d" %
              (e_drift, e_relax, d_drift, d_relax))
        assert e_relax < e_drift
        assert d_relax < d_drift
    finally:
        proc.Dispose()
