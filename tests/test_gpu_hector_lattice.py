"""The pose-lattice search (K7: slamhip_hs_lattice_search, slamhip_hs_relocalise, slamhip_hsproc_relocalise) on the device against
the NumPy restatement of its definition in tests/test_hs_lattice_abi.py, which that module pins against the library's own host
arithmetic without a GPU.  Scores, keys and poses are compared with == on integers and on bit patterns; there is no tolerance.

Shapes are the smallest at which each path of the kernel can go wrong: a level whose rows are no whole number of packed words
(40 cells), a scan that is no multiple of a wavefront (97 points) or longer than one LDS chunk (5000 > 1024), a lattice narrower
than a tile (11 x 7) with nodes off the map on two sides, and a level too large for the staged rectangle (1024 x 1024)."""
import ctypes as C
import math

import numpy as np
import pytest

import test_gpu_hector_shift as S
import test_hs_lattice_abi as A
from test_gpu_hector_shift import hs_mod, ctx, det                         # noqa: F401 (fixtures)

gpu = pytest.mark.gpu
F = np.float32
EMPTY_KEY = 0x80000000FFFFFFFF


def class_values(rng, n):
    """Cell values drawn from {positive, negative, +0, -0, NaN}."""
    pick = rng.integers(0, 5, n)
    mag = rng.uniform(0.1, 3.0, n).astype(np.float32)
    v = np.select([pick == 0, pick == 1, pick == 2, pick == 3], [mag, -mag, F(0.0), F(-0.0)], F(np.nan)).astype(np.float32)
    assert all(int((pick == k).sum()) > 0 for k in range(5))
    return v


def put_values(hs_mod, rep, level, values):
    cells = np.zeros(values.size, hs_mod.capi.CELL_DTYPE)
    cells["update_index"] = -1
    cells["value"] = values
    rep.Maps[level].SetCells(cells)


def assert_search_equals(rep, scan, level, values, centre, nx, ny, n_theta, dtheta, tag):
    """The volume and the keys of one search against the restatement; the search without the volume returns the same keys."""
    w, h = rep.Maps[level].Dimensions
    cell = F(rep.Maps[level].CellLength)
    want = A.np_volume(values, w, h, cell, centre, nx, ny, n_theta, dtheta, scan.Points)
    keys, vol = rep.lattice_search(scan, level, centre, nx, ny, n_theta, dtheta, scores=True)
    assert vol.shape == want.shape and vol.dtype == np.int32
    assert np.array_equal(vol, want), (tag, np.argwhere(vol != want)[:8].tolist())
    assert np.array_equal(keys, A.np_keys(want)), tag
    keys2, none = rep.lattice_search(None, level, centre, nx, ny, n_theta, dtheta)
    assert none is None and np.array_equal(keys2, keys), tag
    return want, keys


@pytest.fixture(scope="module")
def small(hs_mod, ctx):
    """80 x 48 cells of 0.1 m, 2 levels (level 1: 40 x 24, a row of 2.5 packed words), every class of value on both levels."""
    rng = np.random.default_rng(7)
    rep = hs_mod.MapRepMultiMap(0.1, (80, 48), 2, ctx=ctx)
    values = [class_values(rng, 80 * 48), class_values(rng, 40 * 24)]
    for l in range(2):
        put_values(hs_mod, rep, l, values[l])
    yield rep, values
    rep.close()


def small_points(rng, n):
    xy = np.stack([rng.uniform(-1.0, 7.0, n), rng.uniform(-1.0, 4.0, n)], 1).astype(np.float32)
    xy[3] = (np.nan, 0.5)
    xy[11] = (1.0e6, -2.0e6)                                               # far away: off every map, still a valid point
    return xy


# ---- 1. volume and keys ------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("level", [0, 1])
def test_volume_and_keys(hs_mod, small, level):
    rep, values = small
    scan = hs_mod.ScanCloud(small_points(np.random.default_rng(11), 97))
    centre = np.array([0.27, 0.13, 0.3], np.float32)                       # near the map's corner: nodes fall off on two sides
    want, _ = assert_search_equals(rep, scan, level, values[level], centre, 5, 3, 7, F(0.4), level)
    assert np.count_nonzero(want) > want.size // 4 and len(np.unique(want)) > 8   # a volume worth comparing


# ---- 2. the global-memory path -----------------------------------------------------------------------------------------------------
@gpu
def test_global_memory_path(hs_mod, ctx):
    """The kernel stages at most K7_RECT_WORDS = 12288 words (48 KB, 196608 cells) of the class map per workgroup.  Here the points
    spread over about 900 x 900 cells of a 1024 x 1024 level: (900 / 16) words x 900 rows = 50000 words, about four times the budget,
    so every workgroup reads the packed map from global memory."""
    rng = np.random.default_rng(23)
    rep = hs_mod.MapRepMultiMap(0.05, (1024, 1024), 1, ctx=ctx)
    values = class_values(rng, 1024 * 1024)
    put_values(hs_mod, rep, 0, values)
    xy = rng.uniform(-22.5, 22.5, (200, 2)).astype(np.float32)
    xy[5] = (np.nan, np.nan)
    xy[6] = (27.0, 0.0)                                                    # off the map at some headings
    centre = np.array([25.6, 25.6, -0.2], np.float32)
    gx, gy, ok = A.np_point_cells(F(1.0) / F(0.05), centre, centre[2], xy)
    assert (np.ptp(gx[ok]) // 16) * np.ptp(gy[ok]) > 3 * 12288
    assert_search_equals(rep, hs_mod.ScanCloud(xy), 0, values, centre, 1, 1, 4, F(0.9), "global")
    rep.close()


# ---- 3. ties -----------------------------------------------------------------------------------------------------------------------
@gpu
def test_ties_on_an_empty_map(hs_mod, ctx):
    rep = hs_mod.MapRepMultiMap(0.1, (80, 48), 2, ctx=ctx)
    scan = hs_mod.ScanCloud(small_points(np.random.default_rng(11), 97))
    for level in (0, 1):
        keys, vol = rep.lattice_search(scan, level, (2.0, 2.0, 0.0), 5, 3, 7, 0.4, scores=True)
        assert (keys == np.uint64(EMPTY_KEY)).all() and not vol.any()
        assert hs_mod.decode_lattice_key(keys[0]) == (0, 0)
    rep.close()


# ---- 4. many points ----------------------------------------------------------------------------------------------------------------
@gpu
def test_many_points(hs_mod, small):
    rep, values = small
    scan = hs_mod.ScanCloud(small_points(np.random.default_rng(13), 5000))  # five LDS chunks, the last one partial
    want, _ = assert_search_equals(rep, scan, 0, values[0], np.array([0.9, 0.4, -1.0], np.float32), 1, 1, 2, F(2.0), "5000")
    assert np.abs(want).max() > 16


# ---- 5. stream order ---------------------------------------------------------------------------------------------------------------
@gpu
def test_stream_order(hs_mod, ctx, sim):
    w0, h0 = 72, 40
    rep = hs_mod.MapRepMultiMap(S.CELL, (w0, h0), S.LEVELS, ctx=ctx)
    scans = S.local_scans(sim, w0, h0)
    for xy, p in scans[:-1]:
        rep.UpdateByScan(hs_mod.ScanCloud(xy), p)
    xy, p = scans[-1]
    scan = hs_mod.ScanCloud(xy)
    centre = np.array([p[0] + F(0.2), p[1] - F(0.1), p[2] + F(0.1)], np.float32)
    lat = (3, 2, 5, F(0.15))
    rep.UpdateByScan(scan, p)                                              # the last update, and the search right behind it
    got = [rep.lattice_search(None, l, centre, *lat, scores=True) for l in range(S.LEVELS)]
    for l in range(S.LEVELS):
        w, h = rep.Maps[l].Dimensions
        values = rep.Maps[l].GetCells()["value"]
        assert np.count_nonzero(values) > 16
        want = A.np_volume(values, w, h, F(rep.Maps[l].CellLength), centre, *lat, xy)
        assert np.array_equal(got[l][1], want) and np.array_equal(got[l][0], A.np_keys(want)), l
        assert want.any()
    dx, dy = 3 * S.G, -2 * S.G
    rep.shift(dx, dy)
    cw = np.array([centre[0] - F(dx) * F(S.CELL), centre[1] - F(dy) * F(S.CELL), centre[2]], np.float32)   # the window's frame
    got = [rep.lattice_search(None, l, cw, *lat, scores=True) for l in range(S.LEVELS)]
    for l in range(S.LEVELS):
        w, h = rep.Maps[l].Dimensions
        want = A.np_volume(rep.Maps[l].GetCells()["value"], w, h, F(rep.Maps[l].CellLength), cw, *lat, xy)
        assert np.array_equal(got[l][1], want) and np.array_equal(got[l][0], A.np_keys(want)), ("shifted", l)
        assert want.any()
    rep.close()


# ---- the room of cases 6 to 9 ------------------------------------------------------------------------------------------------------
ROOM_CELL, ROOM_W, ROOM_LEVELS = 0.05, 256, 3
ROOM_TRUTH = np.array([6.1, 5.7, 0.9], np.float32)
ROOM_CENTRE = np.array([ROOM_TRUTH[0] + 1.07, ROOM_TRUTH[1] - 0.87, ROOM_TRUTH[2] - math.radians(37.0)], np.float32)
ROOM_LATTICE = (ROOM_LEVELS - 1, 8, 8, 72, F(math.radians(5.0)))           # the coarsest level, +-1.6 m, the full circle in 5 degree steps
_ROOM = {}


def room(sim):
    """The simulator's field shrunk to a 12.8 m window (256 x 256 cells of 0.05 m, 3 levels: the coarsest 64 x 64 of 0.2 m), the 24
    noise-free mapping scans and their poses, and the noise-free scan taken at ROOM_TRUTH."""
    if not _ROOM:
        segs = sim.default_field() * (ROOM_W * ROOM_CELL / 40.0)
        poses = [np.array([5.0 + 0.12 * i, 6.4 - 0.05 * i, 0.1 * i], np.float32) for i in range(24)]
        _ROOM["map"] = [(sim.make_scan(segs, p, 360, noise=False)[1], p) for p in poses]
        _ROOM["scan"] = sim.make_scan(segs, ROOM_TRUTH, 360, noise=False)[1]
    return _ROOM["map"], _ROOM["scan"]


def pose_error(pose, truth=ROOM_TRUTH):
    return (math.hypot(float(pose[0]) - float(truth[0]), float(pose[1]) - float(truth[1])),
            abs(math.remainder(float(pose[2]) - float(truth[2]), 2 * math.pi)))


def sorted_headings(keys):
    """The headings by key, descending; equal keys: the lower k first."""
    return sorted(range(len(keys)), key=lambda k: (-int(keys[k]), k))


@pytest.fixture(scope="module")
def room_rep(hs_mod, ctx, sim):
    rep = hs_mod.MapRepMultiMap(ROOM_CELL, (ROOM_W, ROOM_W), ROOM_LEVELS, ctx=ctx)
    for xy, p in room(sim)[0]:
        rep.UpdateByScan(hs_mod.ScanCloud(xy), p)
    yield rep
    rep.close()


# ---- 6. composition ----------------------------------------------------------------------------------------------------------------
@gpu
def test_relocalise_is_search_then_match_best(hs_mod, room_rep, sim):
    rep = room_rep
    scan = hs_mod.ScanCloud(room(sim)[1])
    level, nx, ny, n_theta, dth = ROOM_LATTICE
    m = hs_mod.ScanMatcher(1)
    for centre, n_th, B in ((ROOM_CENTRE, n_theta, 4), (ROOM_CENTRE, 3, 8)):
        keys, _ = rep.lattice_search(scan, level, centre, nx, ny, n_th, dth)
        order = sorted_headings(keys)[:min(B, n_th)]
        nodes = [(k,) + hs_mod.decode_lattice_key(keys[k]) for k in order]                 # (k, score, flat)
        hints = np.array([rep.lattice_node_pose(level, centre, nx, ny, n_th, dth, k, flat) for k, _, flat in nodes], np.float32)
        for hint, (k, _, flat) in zip(hints, nodes):
            assert S.same_bits(hint, A.np_node_pose(F(rep.Maps[level].CellLength), centre, nx, ny, dth, k, flat))
        want_pose, want_idx, want_rep = m.MatchDataBest(rep, scan, hints)
        pose, rpt, info = m.Relocalise(rep, scan, level, centre, nx, ny, n_th, dth, B=B)
        assert S.same_bits(pose, want_pose) and rpt.tobytes() == want_rep.tobytes()
        k, score, flat = nodes[want_idx]
        NX = 2 * nx + 1
        assert (int(info["n_hints"]), int(info["best_hint"])) == (min(B, n_th), want_idx)
        assert (int(info["k"]), int(info["ix"]), int(info["iy"]), int(info["score"])) == (k, flat % NX - nx, flat // NX - ny, score)
        assert int(info["top_score"]) == nodes[0][1]


# ---- 7. it relocalises -------------------------------------------------------------------------------------------------------------
@gpu
def test_it_relocalises(hs_mod, room_rep, det, sim):
    """The scan is taken 1.38 m and 37 degrees from the lattice's centre, far outside the matcher's basin.  The choice of room, pose
    and lattice is checked here on the CPU alone, on the checker's grid update of the same scans (the device's cells must equal
    it): the restatement's best key is heading k = 7, node (ix, iy) = (-5, 5) with score 232 of 360 points, 0.148 m (0.07 and
    0.13 m per axis, one 0.2 m cell) and 2.0 degrees (one 5 degree step) from the true pose; the checker's matcher started there
    ends 0.0066 m and 0.022 degrees from it, and started at the centre 1.18 m and 35 degrees from it."""
    oc = det
    rep = room_rep
    scans, xy = room(sim)
    level, nx, ny, n_theta, dth = ROOM_LATTICE
    ref = oc.make_pyramid(ROOM_CELL, ROOM_W, ROOM_W, ROOM_LEVELS)
    for sxy, p in scans:
        for g in ref:
            g.update_by_scan(sxy, p)
    for l in range(ROOM_LEVELS):
        assert np.array_equal(S.raw(rep.Maps[l].GetCells()), S.raw(ref[l].cells)), l
    g = ref[level]
    cell = F(rep.Maps[level].CellLength)
    want = A.np_volume(g.cells["value"], g.w, g.h, cell, ROOM_CENTRE, nx, ny, n_theta, dth, xy)
    want_keys = A.np_keys(want)
    k = sorted_headings(want_keys)[0]
    score, flat = hs_mod.decode_lattice_key(want_keys[k])
    node = A.np_node_pose(cell, ROOM_CENTRE, nx, ny, dth, k, flat)
    assert (k, flat % 17 - 8, flat // 17 - 8, score) == (7, -5, 5, 232)
    assert abs(float(node[0]) - float(ROOM_TRUTH[0])) <= float(cell) and abs(float(node[1]) - float(ROOM_TRUTH[1])) <= float(cell)
    assert pose_error(node)[1] <= float(dth)
    # the device
    scan = hs_mod.ScanCloud(xy)
    keys, vol = rep.lattice_search(scan, level, ROOM_CENTRE, nx, ny, n_theta, dth, scores=True)
    assert np.array_equal(vol, want) and np.array_equal(keys, want_keys)
    m = hs_mod.ScanMatcher(1)
    pose, rpt, info = m.Relocalise(rep, scan, level, ROOM_CENTRE, nx, ny, n_theta, dth, B=4)
    assert int(info["top_score"]) == score and sorted_headings(keys)[0] == k             # the library's winner is that node
    start = A.np_node_pose(cell, ROOM_CENTRE, nx, ny, dth, int(info["k"]), (int(info["iy"]) + ny) * 17 + int(info["ix"]) + nx)
    e_pose, e_start = pose_error(pose), pose_error(start)
    assert e_pose[0] <= e_start[0] and e_pose[1] <= e_start[1], (e_pose, e_start)
    plain = m.MatchData(rep, scan, ROOM_CENTRE)
    e_plain = pose_error(plain)
    assert e_plain[0] > e_pose[0] and e_plain[1] > e_pose[1], (e_plain, e_pose)
    assert e_pose[0] < 0.05 and e_plain[0] > 0.5                                          # found, against lost
    for g in ref:
        g.close()


# ---- 8. the processor --------------------------------------------------------------------------------------------------------------
@gpu
def test_processor_relocalise(hs_mod, ctx, sim):
    scans, xy = room(sim)
    level, nx, ny, n_theta, dth = ROOM_LATTICE
    g = 1 << (ROOM_LEVELS - 1)
    proc = hs_mod.HectorSLAMProcessor(ROOM_CELL, (ROOM_W, ROOM_W), scans[0][1], ROOM_LEVELS, ctx=ctx, scrollTrigger=100)
    for sxy, p in scans:
        proc.Update(hs_mod.ScanCloud(sxy), p, mapWithoutMatching=True)
    assert proc.get_origin() == (0, 0)                                     # (the path stays within the trigger)
    dx, dy = 3 * g, -2 * g
    proc.shift(dx, dy)
    assert proc.get_origin() == (dx, dy)
    off = np.array([F(dx) * F(ROOM_CELL), F(dy) * F(ROOM_CELL)], np.float32)
    scan = hs_mod.ScanCloud(xy)
    cw = np.array([ROOM_CENTRE[0] - off[0], ROOM_CENTRE[1] - off[1], ROOM_CENTRE[2]], np.float32)
    want, want_rep, want_info = hs_mod.ScanMatcher(1).Relocalise(proc.MapRep, scan, level, cw, nx, ny, n_theta, dth, B=4)
    want_world = np.array([want[0] + off[0], want[1] + off[1], want[2]], np.float32)
    before = (proc.MatchPose, proc.LastMapUpdatePose)
    pose, rpt, info = proc.Relocalise(scan, ROOM_CENTRE, level, nx, ny, n_theta, dth, B=4, adopt=False)
    assert S.same_bits(pose, want_world) and rpt.tobytes() == want_rep.tobytes() and info.tobytes() == want_info.tobytes()
    assert S.same_bits(proc.MatchPose, before[0]) and S.same_bits(proc.LastMapUpdatePose, before[1])
    assert pose_error(pose)[0] < 0.05
    pose2, _, _ = proc.Relocalise(scan, ROOM_CENTRE, level, nx, ny, n_theta, dth, B=4, adopt=True)
    assert S.same_bits(pose2, want_world)
    assert S.same_bits(proc.MatchPose, want_world) and S.same_bits(proc.LastMapUpdatePose, want_world)
    assert proc.get_origin() == (dx, dy)                                   # no scroll
    # the next Update matches from the adopted pose and, the robot not having moved, does not draw into the map
    sums = [proc.MapRep.Maps[l].checksum() for l in range(ROOM_LEVELS)]
    assert proc.Update(scan, proc.MatchPose) is False
    assert [proc.MapRep.Maps[l].checksum() for l in range(ROOM_LEVELS)] == sums
    assert pose_error(proc.MatchPose)[0] < 0.05 and S.same_bits(proc.LastMapUpdatePose, want_world)
    with pytest.raises(hs_mod.capi.SlamhipError) as e:
        spec = hs_mod.capi.lattice_spec(level, ROOM_CENTRE, nx, ny, n_theta, dth)
        out = np.empty(3, np.float32); r = np.zeros(1, hs_mod.capi.REPORT_DTYPE); inf = hs_mod.capi.RelocInfo()
        hs_mod.capi.call("slamhip_hsproc_relocalise", proc._h, hs_mod.capi.fptr(scan.Points), scan.Points.shape[0], None, C.byref(spec), 4, 2,
                         hs_mod.capi.fptr(out), hs_mod.capi.rptr(r), C.byref(inf))
    assert e.value.code == hs_mod.capi.ERR_INVALID
    proc.Dispose()


# ---- 9. errors, and what the feature leaves alone ----------------------------------------------------------------------------------
@gpu
def test_errors_leave_everything_unchanged(hs_mod, ctx, small):
    capi = hs_mod.capi
    rep, _ = small
    rep.set_scan(hs_mod.ScanCloud(small_points(np.random.default_rng(11), 97)))
    sums = [rep.Maps[l].checksum() for l in range(2)]
    good = dict(level=0, centre=(1.0, 1.0, 0.0), nx=2, ny=2, n_theta=3, dtheta=0.1)
    bad = [dict(level=-1), dict(level=2), dict(nx=-1), dict(nx=4097), dict(ny=-1), dict(ny=4097), dict(n_theta=0), dict(n_theta=4097),
           dict(nx=4096, ny=4096, n_theta=2),                                              # 2 * 8193^2 > 2^26 nodes
           dict(centre=(np.nan, 0.0, 0.0)), dict(centre=(0.0, np.inf, 0.0)), dict(centre=(0.0, 0.0, -np.inf)), dict(dtheta=np.nan)]
    for change in bad:
        a = dict(good, **change)
        spec = capi.lattice_spec(a["level"], a["centre"], a["nx"], a["ny"], a["n_theta"], a["dtheta"])
        keys = np.full(4097, 7, np.uint64)
        pose = np.full(3, 5, np.float32); r = np.zeros(1, capi.REPORT_DTYPE); info = capi.RelocInfo()
        L = capi.lib()
        assert L.slamhip_hs_lattice_search(rep._h, C.byref(spec), keys.ctypes.data_as(C.POINTER(C.c_uint64)), None) == capi.ERR_INVALID, change
        assert L.slamhip_hs_relocalise(rep._h, C.byref(spec), 4, capi.fptr(pose), capi.rptr(r), C.byref(info)) == capi.ERR_INVALID, change
        assert L.slamhip_hs_lattice_node_pose(rep._h, C.byref(spec), 0, 0, capi.fptr(pose)) == capi.ERR_INVALID, change
        assert (keys == 7).all() and (pose == 5).all()
    spec = capi.lattice_spec(**{k: good[k] for k in ("level", "centre", "nx", "ny", "n_theta", "dtheta")})
    pose = np.full(3, 5, np.float32); r = np.zeros(1, capi.REPORT_DTYPE); info = capi.RelocInfo()
    for B in (0, 65):
        assert capi.lib().slamhip_hs_relocalise(rep._h, C.byref(spec), B, capi.fptr(pose), capi.rptr(r), C.byref(info)) == capi.ERR_INVALID
    for k, flat in ((-1, 0), (3, 0), (0, -1), (0, 25)):
        assert capi.lib().slamhip_hs_lattice_node_pose(rep._h, C.byref(spec), k, flat, capi.fptr(pose)) == capi.ERR_INVALID
    assert (pose == 5).all()
    assert [rep.Maps[l].checksum() for l in range(2)] == sums
    # no scan: SLAMHIP_ERR_STATE
    fresh = hs_mod.MapRepMultiMap(0.1, (80, 48), 2, ctx=ctx)
    keys = np.full(3, 7, np.uint64)
    assert capi.lib().slamhip_hs_lattice_search(fresh._h, C.byref(spec), keys.ctypes.data_as(C.POINTER(C.c_uint64)), None) == capi.ERR_STATE
    assert capi.lib().slamhip_hs_relocalise(fresh._h, C.byref(spec), 4, capi.fptr(pose), capi.rptr(r), C.byref(info)) == capi.ERR_STATE
    assert (keys == 7).all() and (pose == 5).all()
    fresh.close()
    # the good spec does go through
    keys, _ = rep.lattice_search(None, **good)
    assert keys.shape == (3,) and (keys != 7).all()


@gpu
def test_other_flows_launch_what_they_launched(hs_mod, sim):
    """Match, update and shift issue no launch of K7's classes; a search issues one pack and one search launch and nothing of the
    matcher's or the grid update's."""
    capi = hs_mod.capi
    own = hs_mod.Context(0)
    own.timing_enable(-1)
    rep = hs_mod.MapRepMultiMap(S.CELL, (64, 64), S.LEVELS, ctx=own)
    scans = S.local_scans(sim, 64, 64)
    m = hs_mod.ScanMatcher(1)
    for xy, p in scans:
        m.MatchData(rep, hs_mod.ScanCloud(xy), p)
        rep.UpdateByScan(hs_mod.ScanCloud(xy), p)
    rep.shift(S.G, 0)
    counts = lambda: [own.timing_get(k)[1] for k in (capi.K_HS_MATCH, capi.K_HS_UPDATE, capi.K_HS_LATTICE_PACK, capi.K_HS_LATTICE)]
    c0 = counts()
    assert c0[0] == len(scans) and c0[1] >= len(scans) and c0[2:] == [0, 0]
    rep.lattice_search(hs_mod.ScanCloud(scans[-1][0]), 1, scans[-1][1], 2, 2, 3, 0.1)
    assert counts() == [c0[0], c0[1], 1, 1]
    rep.close()
    own.close()
