"""GPU tests of the CoreSLAM search report (slamhip_search_report, include/slamhip.h): the report forms return what the plain
forms return, the kept distances are the oracle's, and every field of the report equals a restatement made here from the oracle's
pieces -- the distances of every candidate (oracle search), the winner's in-map count (np_oracle.poses_to_pxcs + the binary32
expressions of np_oracle.distance_batch_pxcs), the packed keys d << 32 | index.

The nine binary64 sums are compared with NumPy's binary64 sum of the same exact terms within Higham's bound for a sum of n terms
in any order, gamma_n * sum(|terms|), gamma_n = n u / (1 - n u), u = 2^-53 (Accuracy and Stability of Numerical Algorithms,
sec. 4.2) -- derived, not measured; every term is exact (the product of two binary32 values has 48 significant bits).

Launch counters of the per-scan flow with reports off (test_report_off_launches_what_it_launched): the flow's searches either
precede their scan's tables or start at once, and a plan accompanies only a search that waits in the stream (distance.hip,
k1_plan_launch), so plan_stats[0] stays 0 there by design; the test asserts the searches counted (with + without a plan) and the
launches ahead are non-zero and that all eight counters equal those of an identical earlier run."""
import glob
import math
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
INT_MAX = 2 ** 31 - 1
U = 2.0 ** -53


@pytest.fixture(scope="module")
def cs_mod():
    import slam.net_amd.coreslam as m
    return m


@pytest.fixture(scope="module")
def capi():
    import slam.net_amd.capi as c
    return c


@pytest.fixture(scope="module")
def ctx(cs_mod):
    c = cs_mod.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def det(oc):
    oc.set_trig_mode(oc.TRIG_DET)
    yield oc
    oc.set_trig_mode(oc.TRIG_LIBM)


# ---- the restatement -------------------------------------------------------------------------------------------------------
def expected_report(npo, size, scale, xy, base, offs, d, band):
    """slamhip_search_report from the oracle's distances d (flat order) -- integers exactly, the sums with their bounds."""
    d = np.asarray(d, np.int32)
    K = d.size
    offs = np.asarray(offs, np.float32)
    offs = offs.reshape(-1, 3) if offs.size else np.zeros((0, 3), np.float32)
    assert K == offs.shape[0] + 1
    keys = (d.astype(np.uint64) << np.uint64(32)) | np.arange(K, dtype=np.uint64)
    order = np.sort(keys)
    best = int(order[0])
    bd, bi = best >> 32, best & 0xFFFFFFFF
    runner = int(order[1]) if K > 1 else None
    pose = np.asarray(base, np.float32) if bi == 0 else (np.asarray(base, np.float32) + offs[bi - 1]).astype(np.float32)   # :635-637
    q = npo.poses_to_pxcs(pose[None], scale)                                   # :232-235
    X, Y = np.asarray(xy, np.float32).reshape(-1, 2).T
    fx = (q[0, 0] + q[0, 2] * X) - q[0, 3] * Y                                 # np_oracle.distance_batch_pxcs: :240
    fy = (q[0, 1] + q[0, 3] * X) + q[0, 2] * Y                                 # :241
    ix, iy = npo.f2i_array(fx), npo.f2i_array(fy)
    n_in = int(((ix >= 0) & (ix < size) & (iy >= 0) & (iy < size)).sum())      # :244
    scored = d != INT_MAX
    in_band = scored & (d.astype(np.int64) - bd <= band)
    o = np.vstack([np.zeros((1, 3), np.float32), offs]).astype(np.float64)[in_band]
    terms = [o[:, 0], o[:, 1], o[:, 2], o[:, 0] * o[:, 0], o[:, 0] * o[:, 1], o[:, 0] * o[:, 2], o[:, 1] * o[:, 1], o[:, 1] * o[:, 2], o[:, 2] * o[:, 2]]
    n = int(in_band.sum())
    gamma = n * U / (1.0 - n * U)
    ints = dict(best_dist=bd, best_index=bi, runner_dist=(runner >> 32) if runner is not None else INT_MAX,
                runner_index=(runner & 0xFFFFFFFF) if runner is not None else -1, dist0=int(d[0]), n_candidates=K,
                n_unscored=int((~scored).sum()), n_ties=int((d == bd).sum()), band=int(band), n_band=n,
                n_in_map=n_in if bd != INT_MAX else 0, n_points=int(X.size))
    sums = [float(np.sum(t)) if n else 0.0 for t in terms]
    bounds = [gamma * float(np.sum(np.abs(t))) if n else 0.0 for t in terms]
    return ints, sums, bounds


def check_report(rep, ints, sums, bounds, what=""):
    for k, v in ints.items():
        print("%s %s: got %d want %d" % (what, k, int(rep[k]), v))
        assert int(rep[k]) == v, (what, k, int(rep[k]), v)
    got = list(rep["sum_off"]) + list(rep["sum_off2"])
    for i, (g, s, b) in enumerate(zip(got, sums, bounds)):
        print("%s sum %d: got %.17g want %.17g |diff| %.3g bound %.3g" % (what, i, g, s, abs(g - s), b))
        assert abs(g - s) <= b, (what, i, g, s, b)
    if ints["n_band"] == 0:
        assert all(np.signbit(g) == False and g == 0.0 for g in got)       # noqa: E712  (+0.0)


def mid_band(d):
    """A band from the data with 1 < n_band < K: up to the median of the scored distances."""
    s = np.sort(d[d != INT_MAX].astype(np.int64))
    assert s.size >= 3 and s[0] != s[-1]
    band = int(s[s.size // 2] - s[0])
    if (s - s[0] <= band).sum() == d.size:                                  # (more than half of the field at one distance)
        band = int(s[1] - s[0]) if s[1] != s[-1] else 0
    return band


# ---- the cases -------------------------------------------------------------------------------------------------------------
class Case:
    pass


def _sim_case(cs_mod, ctx, sim, oc, size, R, K, kind):
    c = Case()
    segs = sim.default_field()
    dev = cs_mod.CoreSlamDevice(ctx, 40.0, size, max(size // 4, 16))
    rng = sim.PCG32(1234)
    for p in sim.trajectory(8):
        _, xy = sim.make_scan(segs, p, R, rng)
        dev.set_scan(xy)
        dev.update_holemap(p)
    c.pix = dev.holemap_download()
    true_pose = sim.trajectory(9)[-1]
    _, c.xy = sim.make_scan(segs, true_pose, R, sim.PCG32(99))
    c.base = (true_pose + np.array([0.03, -0.02, math.radians(1.0)], np.float32)).astype(np.float32)
    dev.set_scan(c.xy)
    if kind == "set":
        c.offs = sim.gaussian_offsets(K - 1)
        dev.set_offsets(c.offs)
    else:
        dev.generate_offsets(K - 1, 0.1, math.radians(10.0), seed=7, stream=3, lattice=(kind == "lattice"))
        c.offs = dev.offsets_download()
    c.dev, c.size, c.scale = dev, size, dev.hole_scale
    return c


def _golden_case(cs_mod, ctx, name):
    g = np.load(os.path.join(GOLD, name))
    c = Case()
    c.size = int(g["size"])
    dev = cs_mod.CoreSlamDevice(ctx, 40.0, c.size, 64)
    assert dev.hole_scale == float(g["scale"])
    dev.holemap_upload(g["pixels"])
    dev.set_scan(g["xy"])
    dev.set_offsets(g["offs"])
    c.dev, c.scale, c.pix, c.xy, c.base, c.offs = dev, dev.hole_scale, g["pixels"], g["xy"], g["base"].astype(np.float32), g["offs"]
    return c


GOLDEN = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLD, "cs_distance_*.npz")))
SIM = {
    "sim_256": (256, 360, 4001, "set"), "sim_400": (400, 360, 4001, "set"), "sim_2048": (2048, 1080, 16384, "set"),
    "kside_12288": (400, 360, 12288, "set"), "kside_12289": (400, 360, 12289, "set"),
    "kside_65535": (256, 200, 65535, "set"), "kside_65536": (256, 200, 65536, "set"),
    "generated": (512, 360, 20000, "gen"), "lattice": (512, 720, 16385, "lattice"),
    "fallback_300": (300, 360, 3001, "set"),                                   # a side that is not a multiple of 8: the fallback kernels
}
CASES = ["golden_" + n[:-4] for n in GOLDEN] + list(SIM)
_cache = {}


@pytest.fixture
def case(request, cs_mod, ctx, sim, det):
    name = request.param
    if name not in _cache:
        if name.startswith("golden_"):
            c = _golden_case(cs_mod, ctx, name[len("golden_"):] + ".npz")
        else:
            c = _sim_case(cs_mod, ctx, sim, det, *SIM[name])
        _, _, _, c.d = det.search(c.pix, c.size, c.scale, c.xy, c.base, c.offs)
        c.d = np.asarray(c.d, np.int32)
        _cache[name] = c
    return _cache[name]


@pytest.fixture(scope="module", autouse=True)
def _close_cases(ctx):                                                         # (after ctx in set-up, so before it in tear-down: the handles go first)
    yield
    for c in _cache.values():
        c.dev.close()
    _cache.clear()


# ---- 1. no pose changes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, indirect=True)
def test_no_pose_changes(case):
    dev = case.dev
    pose, dist, idx = dev.search(case.base)
    for band in (0, 7, INT_MAX):
        p2, rep = dev.search_report(case.base, band)
        assert p2.tobytes() == pose.tobytes() and int(rep["best_dist"]) == dist and int(rep["best_index"]) == idx, (band, pose, p2, dist, idx, rep)
    p3, d3, i3 = dev.search(case.base)
    assert p3.tobytes() == pose.tobytes() and (d3, i3) == (dist, idx)
    assert dev.selfcheck_failures == 0


# ---- 2. distances ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, indirect=True)
def test_distances(case):
    dev = case.dev
    dev.search_report(case.base, 0)
    got = dev.search_distances()
    assert got.dtype == np.int32 and got.shape == case.d.shape
    assert (got == case.d).all(), np.flatnonzero(got != case.d)[:8]


# ---- 3. fields -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, indirect=True)
def test_fields(case, npo):
    dev = case.dev
    mid = mid_band(case.d)
    for band in (0, mid, INT_MAX):
        ints, sums, bounds = expected_report(npo, case.size, case.scale, case.xy, case.base, case.offs, case.d, band)
        if band == mid:
            assert 1 < ints["n_band"] < case.d.size, (mid, ints["n_band"])
        _, rep = dev.search_report(case.base, band)
        check_report(rep, ints, sums, bounds, "band %d" % band)
        _, rep2 = dev.search_report(case.base, band)
        assert rep.tobytes() == rep2.tobytes()                                 # the same call, the same bits
        assert len(rep.tobytes()) == 120


def test_child_processes_on_other_paths():
    """The golden, simulated-map and group-size-threshold cases once more on the bounds-checked search kernels
    (SLAMHIP_K1_GLOBAL=1) and without the host mailbox (SLAMHIP_NO_HOSTWAIT=1: results come back by copy + synchronise)."""
    sel = "(test_no_pose_changes or test_distances or test_fields) and (golden_ or sim_ or kside_)"
    for extra in ({"SLAMHIP_K1_GLOBAL": "1"}, {"SLAMHIP_NO_HOSTWAIT": "1"}):
        env = dict(os.environ, **extra)
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-k", sel],
                           env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert r.returncode == 0, (extra, r.stdout.decode(errors="replace")[-3000:])


# ---- 4. edges --------------------------------------------------------------------------------------------------------------
def test_edges(cs_mod, capi, ctx, sim, det, npo):
    C = capi.C
    c = _sim_case(cs_mod, ctx, sim, det, 256, 360, 2001, "set")
    dev = c.dev
    try:
        # before any report search / after a search without a report: SLAMHIP_ERR_STATE; a wrong K: SLAMHIP_ERR_INVALID
        out = np.empty(2001, np.int32)
        L = capi.lib()
        assert L.slamhip_cs_search_distances(dev._h, capi.iptr(out), 2001) == capi.ERR_STATE
        dev.search(c.base)
        assert L.slamhip_cs_search_distances(dev._h, capi.iptr(out), 2001) == capi.ERR_STATE
        dev.search_report(c.base, 0)
        assert L.slamhip_cs_search_distances(dev._h, capi.iptr(out), 2000) == capi.ERR_INVALID
        assert L.slamhip_cs_search_distances(dev._h, capi.iptr(out), 2001) == capi.OK
        dev.search(c.base)
        assert L.slamhip_cs_search_distances(dev._h, capi.iptr(out), 2001) == capi.ERR_STATE
        dev.search_report(c.base, 0)
        dev.distance_poses(np.tile(c.base, (4, 1)))
        assert L.slamhip_cs_search_distances(dev._h, capi.iptr(out), 2001) == capi.ERR_STATE
        # negative band, null report
        sp = capi.f32(c.base); pose = np.empty(3, np.float32); rep = np.zeros(1, capi.SEARCH_REPORT_DTYPE)
        assert L.slamhip_cs_search_report(dev._h, capi.fptr(sp), -1, capi.fptr(pose), capi.srptr(rep)) == capi.ERR_INVALID
        assert L.slamhip_cs_search_report(dev._h, capi.fptr(sp), 0, capi.fptr(pose), None) == capi.ERR_INVALID
        assert L.slamhip_cs_search_and_update_report(dev._h, capi.fptr(sp), -1, C.c_float(0.6), 50, 10, capi.fptr(pose), capi.srptr(rep)) == capi.ERR_INVALID
        assert L.slamhip_cs_search_and_update_report(dev._h, capi.fptr(sp), 0, C.c_float(0.6), 50, 10, capi.fptr(pose), None) == capi.ERR_INVALID
        # a search pose far off the map: nothing is scored
        far = np.array([500.0, -700.0, 0.3], np.float32)
        _, _, _, d = det.search(c.pix, c.size, c.scale, c.xy, far, c.offs)
        d = np.asarray(d, np.int32)
        assert (d == INT_MAX).all()
        for band in (0, 1000, INT_MAX):
            p, rep = dev.search_report(far, band)
            ints, sums, bounds = expected_report(npo, c.size, c.scale, c.xy, far, c.offs, d, band)
            assert ints["n_band"] == 0 and ints["n_ties"] == ints["n_unscored"] == 2001 and ints["n_in_map"] == 0 and ints["best_index"] == 0
            check_report(rep, ints, sums, bounds, "far, band %d" % band)
            assert p.tobytes() == far.tobytes()
            assert (dev.search_distances() == INT_MAX).all()
        # the same offset three times: ties, the winner the lowest index, the runner-up the next index with the same distance
        _, rep = dev.search_report(c.base, 0)
        w = int(rep["best_index"])
        assert w > 0
        offs = c.offs.copy()
        for flat in (11, 14, 17):                                              # three more copies of the winner's jitter
            offs[flat - 1] = c.offs[w - 1]
        copies = sorted({w, 11, 14, 17})                                       # (no candidate below w has the winner's distance)
        dev.set_offsets(offs)
        _, _, _, d = det.search(c.pix, c.size, c.scale, c.xy, c.base, offs)
        d = np.asarray(d, np.int32)
        p, rep = dev.search_report(c.base, 0)
        ints, sums, bounds = expected_report(npo, c.size, c.scale, c.xy, c.base, offs, d, 0)
        check_report(rep, ints, sums, bounds, "triple")
        assert int(rep["n_ties"]) >= 3 and int(rep["best_index"]) == copies[0] and int(rep["runner_index"]) == copies[1]
        assert int(rep["runner_dist"]) == int(rep["best_dist"])
        ps, ds, is_ = dev.search(c.base)
        assert ps.tobytes() == p.tobytes() and is_ == copies[0]
        # K = 1: an empty jitter list
        capi.call("slamhip_cs_set_offsets", dev._h, None, 0)
        dev.n_offsets = 0
        d = npo.distance_batch_pxcs(c.pix, c.size, c.xy, npo.poses_to_pxcs(c.base[None], c.scale))
        p, rep = dev.search_report(c.base, 5)
        ints, sums, bounds = expected_report(npo, c.size, c.scale, c.xy, c.base, np.zeros((0, 3), np.float32), d, 5)
        assert ints["runner_dist"] == INT_MAX and ints["runner_index"] == -1 and ints["n_candidates"] == 1
        check_report(rep, ints, sums, bounds, "K = 1")
        assert (dev.search_distances() == d).all() and p.tobytes() == c.base.tobytes()
    finally:
        dev.close()


# ---- 5. fused --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,R,K,scan_form", [(1024, 900, 8192, False), (1024, 900, 8192, True), (300, 360, 3001, False)])
def test_fused(cs_mod, ctx, sim, size, R, K, scan_form):
    segs = sim.default_field()
    a, b, c = (cs_mod.CoreSlamDevice(ctx, 40.0, size, 256) for _ in range(3))
    rng = sim.PCG32(91)
    traj = sim.trajectory(12, step=(0.06, 0.02, math.radians(0.5)))
    offs = sim.gaussian_offsets(K - 1, 0.1, math.radians(8.0), seed=5)
    try:
        for d in (a, b, c):
            d.set_offsets(offs)
        for i, p in enumerate(traj):
            _, xy = sim.make_scan(segs, p, R, rng)
            if i < 4:
                for d in (a, b, c):
                    d.set_scan(xy); d.update_holemap(p, 0.6, 50); d.update_obstaclemap(p, 10)
                continue
            search = (p + np.array([0.03, -0.02, math.radians(0.8)], np.float32)).astype(np.float32)
            band = (0, 50, INT_MAX)[i % 3]
            if scan_form:
                pa, da, ia = a.scan_search_and_update(xy, search, 0.6, 50, 10)
                pb, rb = b.search_and_update_report(search, band, 0.6, 50, 10, xy=xy)
            else:
                a.set_scan(xy); b.set_scan(xy)
                pa, da, ia = a.search_and_update(search, 0.6, 50, 10)
                pb, rb = b.search_and_update_report(search, band, 0.6, 50, 10)
            assert pa.tobytes() == pb.tobytes() and da == int(rb["best_dist"]) and ia == int(rb["best_index"]), (i, pa, pb)
            # the third handle: the stand-alone report BEFORE its update -- the fused report describes the map that was searched
            c.set_scan(xy)
            pc, rc = c.search_report(search, band)
            assert rc.tobytes() == rb.tobytes(), (i, rc, rb)
            dist_b, dist_c = b.search_distances(), c.search_distances()
            assert (dist_b == dist_c).all()
            pcn = pc.copy()
            c.update_holemap(pb, 0.6, 50); c.update_obstaclemap(pb, 10)
            assert pcn[0] == pb[0] and pcn[1] == pb[1]                         # (theta: the fused forms return it normalised, :746)
            assert a.maps_checksum() == b.maps_checksum() == c.maps_checksum(), i
        assert (a.holemap_download() == b.holemap_download()).all() and (a.obstaclemap_download() == b.obstaclemap_download()).all()
    finally:
        for d in (a, b, c):
            d.close()


# ---- 6. processor ----------------------------------------------------------------------------------------------------------
def _run_processor(cs_mod, ctx, sim, report, band=40, scans=60, twin=None, npo=None):
    segs = sim.default_field()
    start = np.array([20.0, 20.0, 0.0], np.float32)
    proc = cs_mod.CoreSLAMProcessor(40.0, 1024, 128, start, 0.1, math.radians(10), 500, 4, ctx=ctx, searchReport=report, reportBand=band)
    proc.HoleWidth = 2.0
    offs = sim.gaussian_offsets(4000, seed=77)
    proc.SetOffsets(offs)
    if twin is not None:
        from slam.net_amd import capi
        twin.reset(-5)
        twin.set_offsets(offs)
        twin_pose, twin_odo = start.copy(), np.zeros(3, np.float32)           # CoreSLAMProcessor.cs:172-173
    rng = sim.PCG32(33)
    step = np.array([0.05, 0.02, math.radians(0.4)], np.float32)
    poses, reports = [], []
    assert proc.LastSearchReport is None
    for i, tp in enumerate(sim.trajectory(scans, step=(0.05, 0.02, math.radians(0.4)))):
        rays, _ = sim.make_scan(segs, tp, 720, rng)
        est = proc.Pose.copy()
        seg_pose = (est + step).astype(np.float32) if i else est
        searching = i >= 5
        proc.Update([cs_mod.ScanSegment(rays, seg_pose)])
        rep = proc.LastSearchReport
        if not report or not searching:
            assert rep is None, i
        else:
            assert rep is not None, i
        poses.append(proc.Pose.copy()); reports.append(None if rep is None else rep.copy())
        if twin is not None:
            # the same scan on the operator level: ScanSegmentsToCloud, then search_report + the updates (or the updates alone)
            xy = np.empty((rays.shape[0], 2), np.float32)
            sp = capi.f32(seg_pose[None]); st = np.array([0, rays.shape[0]], np.int32); rr = capi.f32(rays)
            capi.call("slamhip_scan_segments_to_cloud", capi.fptr(sp), capi.iptr(st), 1, capi.fptr(rr), capi.fptr(xy))
            twin.set_scan(xy)
            if searching:
                search = (twin_pose + (seg_pose - twin_odo)).astype(np.float32)               # :728
                tpose, trep = twin.search_report(search, band)
                assert rep is not None and trep.tobytes() == rep.tobytes(), (i, trep, rep)
                tpose = np.array([tpose[0], tpose[1], npo.normalize_angle(tpose[2])], np.float32)       # :746
            else:
                tpose = np.array([seg_pose[0], seg_pose[1], npo.normalize_angle(seg_pose[2])], np.float32)
            twin.update_holemap(tpose, 2.0, 50); twin.update_obstaclemap(tpose, 10)
            twin_pose, twin_odo = tpose, seg_pose
            assert tpose.tobytes() == proc.Pose.tobytes(), (i, tpose, proc.Pose)
    return proc, poses, reports


def test_processor(cs_mod, ctx, sim, npo):
    plain, poses0, reps0 = _run_processor(cs_mod, ctx, sim, False)
    twin = cs_mod.CoreSlamDevice(ctx, 40.0, 1024, 128)
    withrep, poses1, reps1 = _run_processor(cs_mod, ctx, sim, True, twin=twin, npo=npo)
    try:
        assert all(r is None for r in reps0) and plain.LastSearchReport is None
        assert len(poses0) == len(poses1) == 60
        for i, (p0, p1) in enumerate(zip(poses0, poses1)):
            assert p0.tobytes() == p1.tobytes(), (i, p0, p1)
        assert plain.device.maps_checksum() == withrep.device.maps_checksum() == twin.maps_checksum()
        assert sum(r is not None for r in reps1) == 55
        assert withrep.LastSearchReport is not None
        # switching reports off drops the last report; on again: none until the next searching scan; bad arguments change nothing
        from slam.net_amd import capi
        L = capi.lib()
        for on, band in ((2, 0), (-1, 0), (1, -1), (0, -5)):
            assert L.slamhip_csproc_set_search_report(withrep._h, on, band) == capi.ERR_INVALID
        assert withrep.LastSearchReport is not None and int(withrep.LastSearchReport["band"]) == 40
        withrep.SetSearchReport(False)
        assert withrep.LastSearchReport is None
        withrep.SetSearchReport(True, 3)
        assert withrep.LastSearchReport is None
        withrep.Reset()
        assert withrep.LastSearchReport is None
    finally:
        plain.Dispose(); withrep.Dispose(); twin.close()


# ---- 7. nothing moved with reports off ---------------------------------------------------------------------------------------
def test_report_off_launches_what_it_launched(cs_mod, ctx, sim):
    first, poses_a, _ = _run_processor(cs_mod, ctx, sim, False)
    stats_a = (first.device.prelaunch_stats, first.device.plan_stats, first.device.prepared_lists())
    first.Dispose()
    mid, _, _ = _run_processor(cs_mod, ctx, sim, True, scans=12)               # (a report run on the same context in between)
    mid.Dispose()
    second, poses_b, _ = _run_processor(cs_mod, ctx, sim, False)
    stats_b = (second.device.prelaunch_stats, second.device.plan_stats, second.device.prepared_lists())
    third, _, _ = _run_processor(cs_mod, ctx, sim, True, scans=30)
    rep_stats = (third.device.prelaunch_stats, third.device.plan_stats)
    second.Dispose(); third.Dispose()
    print("report off:", stats_a, stats_b, "report on:", rep_stats)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(poses_a, poses_b))
    if os.environ.get("SLAMHIP_PRELAUNCH", "1") != "0" and not os.environ.get("SLAMHIP_NO_HOSTWAIT"):
        assert stats_a[0][0] > 0, stats_a
    assert stats_a[1][0] + stats_a[1][1] > 0, stats_a
    assert stats_a == stats_b, (stats_a, stats_b)
    assert rep_stats[0][0] == 0 and rep_stats[1][0] == 0, rep_stats           # the report forms: nothing launched ahead, no plan
