"""The world search (slamhip_hs_world_lattice_search: the lattice scored against the window over the tiles behind it) and the
relocalisation that brings the window to its winner (slamhip_hs_relocalise_world, slamhip_hsproc_relocalise_world) on the device,
against the NumPy restatement of the world definition in tests/test_hs_world_lattice_abi.py, fed from world_cells.  Scores, keys
and poses are compared with == on integers and on bit patterns; there is no tolerance but the pose error against the truth, whose
bounds are test_gpu_hector_lattice.py's for the same room.

Shapes are the smallest at which each path can go wrong: tiles of 8 cells (half a packed word) around an 80 x 48 window whose
level-1 origin is no multiple of 16, so that every piece edge falls inside a word; holes between the tiles; stale tile copies
under the window; a rectangle of 1120 x 1088 cells with a negative origin that no workgroup can stage."""
import ctypes as C
import math

import numpy as np
import pytest

import test_gpu_hector_lattice as L
import test_gpu_hector_shift as S
import test_hs_lattice_abi as A
import test_hs_world_lattice_abi as W
from test_gpu_hector_shift import hs_mod, ctx, det                         # noqa: F401 (fixtures)

gpu = pytest.mark.gpu
F = np.float32
POOL = 64 << 20


def fill(hs_mod, rep, rng):
    for l, m in enumerate(rep.Maps):
        w, h = m.Dimensions
        L.put_values(hs_mod, rep, l, L.class_values(rng, w * h))


def world_values(rep, level, rect):
    """(values, ax0, ay0): the Values of the WORLD rectangle rect = (x0, y0, w, h) of `level`, and the window-frame cell of its
    first element."""
    ox, oy = rep.origin()
    x0, y0, w, h = rect
    return rep.world_cells(level, x0, y0, w, h)["value"], x0 - (ox >> level), y0 - (oy >> level)


def assert_holds_the_world(rep, level, rect):
    """Everything of the level that is not Reset lies inside `rect`, and nothing was dropped."""
    e = rep.world_extends(level)
    x0, y0, w, h = rect
    assert e is not None and x0 <= e[2] and e[0] < x0 + w and y0 <= e[3] and e[1] < y0 + h, (e, rect)
    assert rep.backing_stats()["dropped_cells"] == 0


def assert_world_search_equals(rep, scan, level, rect, centre, nx, ny, n_theta, dtheta, tag):
    values, ax0, ay0 = world_values(rep, level, rect)
    cell = F(rep.Maps[level].CellLength)
    want = W.np_world_volume(values, ax0, ay0, cell, centre, nx, ny, n_theta, dtheta, scan.Points)
    keys, vol = rep.world_lattice_search(scan, level, centre, nx, ny, n_theta, dtheta, scores=True)
    assert vol.shape == want.shape and vol.dtype == np.int32
    assert np.array_equal(vol, want), (tag, int((vol != want).sum()), np.argwhere(vol != want)[:8].tolist())
    assert np.array_equal(keys, A.np_keys(want)), tag
    keys2, none = rep.world_lattice_search(None, level, centre, nx, ny, n_theta, dtheta)
    assert none is None and np.array_equal(keys2, keys), tag
    return want


# ---- 1. volume and keys over window + tiles ----------------------------------------------------------------------------------------
# every window position of `scattered`, grown to whole tiles and more: level 0, level 1 (world cells)
SCATTER_RECTS = [(-64, -48, 224, 144), (-32, -24, 112, 72)]


@pytest.fixture(scope="module")
def scattered(hs_mod, ctx):
    """80 x 48 cells of 0.1 m, 2 levels, tiles of 8 cells.  Both levels filled with every class of value, shifted by (34, -22),
    refilled, shifted by (-70, 30): the origin is (-36, 8); tiles lie to the right of the window and above it, with the never
    visited corner between them a hole, and the tiles of the first window lie under the new one with stale copies.  On level 1
    the window starts at world cell -18 and the tiles at multiples of 8: in the window's frame every tile edge is 2 (mod 8), so
    tile pieces, the window's right edge (cell 40) and R's own origin all fall inside packed words."""
    rng = np.random.default_rng(7)
    rep = hs_mod.MapRepMultiMap(0.1, (80, 48), 2, ctx=ctx)
    rep.set_backing(8, POOL)
    fill(hs_mod, rep, rng)
    rep.shift(34, -22)
    fill(hs_mod, rep, rng)
    rep.shift(-70, 30)
    assert rep.origin() == (-36, 8)
    yield rep
    rep.close()


@gpu
@pytest.mark.parametrize("level", [0, 1])
def test_volume_and_keys_over_window_and_tiles(hs_mod, scattered, level):
    rep = scattered
    rect = SCATTER_RECTS[level]
    assert_holds_the_world(rep, level, rect)
    assert rep.backing_stats()["tiles"] > 20
    scan = hs_mod.ScanCloud(L.small_points(np.random.default_rng(11), 97))  # a NaN point and (1e6, -2e6) among them
    centre = np.array([0.27, 0.13, 0.3], np.float32)                       # near the window's corner
    lat = (40, 30, 5, F(0.4))
    want = assert_world_search_equals(rep, scan, level, rect, centre, *lat, level)
    assert np.count_nonzero(want) > want.size // 4 and len(np.unique(want)) > 8
    # nodes reach beyond the rectangle the reference holds (and so beyond R), where everything is Reset
    ox, oy = rep.origin()
    gx, gy, ok = A.np_point_cells(F(1.0) / F(rep.Maps[level].CellLength), centre, centre[2], scan.Points)
    assert gx[ok].min() - lat[0] < rect[0] - (ox >> level)
    # not the window search under a new name
    keys_w, vol_w = rep.lattice_search(None, level, centre, *lat, scores=True)
    w, h = rep.Maps[level].Dimensions
    assert np.array_equal(vol_w, A.np_volume(rep.Maps[level].GetCells()["value"], w, h, F(rep.Maps[level].CellLength), centre, *lat, scan.Points))
    assert not np.array_equal(vol_w, want) and int((vol_w != want).sum()) > want.size // 8


# ---- 2. the window wins ------------------------------------------------------------------------------------------------------------
@gpu
def test_the_window_wins(hs_mod, ctx):
    rng = np.random.default_rng(19)
    rep = hs_mod.MapRepMultiMap(0.1, (80, 48), 2, ctx=ctx)
    rep.set_backing(8, POOL)
    fill(hs_mod, rep, rng)
    rep.shift(34, -22)
    rep.shift(-34, 22)                                                     # back: the tiles keep what they were given
    old = [rep.Maps[l].GetCells()["value"].copy() for l in range(2)]
    assert rep.backing_stats()["tiles"] > 20 and rep.backing_stats()["restored_cells"] > 0
    fill(hs_mod, rep, rng)                                                 # the window alone changes: the tiles under it are stale now
    scan = hs_mod.ScanCloud(L.small_points(np.random.default_rng(11), 97))
    centre = np.array([3.1, 2.2, -0.4], np.float32)
    lat = (12, 9, 3, F(0.7))
    for level in range(2):
        w, h = rep.Maps[level].Dimensions
        cell = F(rep.Maps[level].CellLength)
        new = rep.Maps[level].GetCells()["value"]
        want = assert_world_search_equals(rep, scan, level, SCATTER_RECTS[level], centre, *lat, ("wins", level))
        # outside the window the tiles hold the Reset cells of the exposed bands only: the world's volume is the new window's
        assert np.array_equal(want, A.np_volume(new, w, h, cell, centre, *lat, scan.Points))
        assert not np.array_equal(want, A.np_volume(old[level], w, h, cell, centre, *lat, scan.Points))
    rep.close()


# ---- 3. no tiles -------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("backing", [False, True])
def test_no_tiles_is_the_window_search(hs_mod, ctx, backing):
    rep = hs_mod.MapRepMultiMap(0.1, (80, 48), 2, ctx=ctx)
    if backing:
        rep.set_backing(8, POOL)
    fill(hs_mod, rep, np.random.default_rng(29))
    scan = hs_mod.ScanCloud(L.small_points(np.random.default_rng(11), 97))
    centre = np.array([0.27, 0.13, 0.3], np.float32)
    for level in range(2):
        keys_w, vol_w = rep.lattice_search(scan, level, centre, 40, 30, 5, 0.4, scores=True)
        keys, vol = rep.world_lattice_search(scan, level, centre, 40, 30, 5, 0.4, scores=True)
        assert np.array_equal(keys, keys_w) and np.array_equal(vol, vol_w) and vol.any(), level
    assert rep.backing_stats()["tiles"] == 0
    rep.close()


# ---- 4. the global-memory path of k7_search with an origin --------------------------------------------------------------------------
@gpu
def test_global_memory_path_with_an_origin(hs_mod, ctx):
    """As test_gpu_hector_lattice.test_global_memory_path, with the window shifted by (96, 64) off a filled 1024 x 1024 level: the
    tiles (256 cells) that took the departing cells are the column tx = 0 and the row ty = 0 of world [0, 1024)^2, the window is
    [96, 1120) x [64, 1088), so R is 1120 x 1088 cells from window-frame cell (-96, -64).  The points spread over about 900 x 900
    cells around cell (400, 420): (900 / 16) words x 900 rows, four times what a workgroup stages, and they overhang the window on
    the tiles' side."""
    rng = np.random.default_rng(23)
    rep = hs_mod.MapRepMultiMap(0.05, (1024, 1024), 1, ctx=ctx)
    rep.set_backing(256, POOL)
    L.put_values(hs_mod, rep, 0, L.class_values(rng, 1024 * 1024))
    rep.shift(96, 64)
    L.put_values(hs_mod, rep, 0, L.class_values(rng, 1024 * 1024))
    rect = (0, 0, 1120, 1088)
    assert_holds_the_world(rep, 0, rect)
    xy = rng.uniform(-22.5, 22.5, (200, 2)).astype(np.float32)
    xy[5] = (np.nan, np.nan)
    xy[6] = (27.0, 0.0)
    centre = np.array([20.0, 21.0, -0.2], np.float32)
    gx, gy, ok = A.np_point_cells(F(1.0) / F(0.05), centre, centre[2], xy)
    assert (np.ptp(gx[ok]) // 16) * np.ptp(gy[ok]) > 3 * 12288 and gx[ok].min() < 0 and gy[ok].min() < 0
    want = assert_world_search_equals(rep, hs_mod.ScanCloud(xy), 0, rect, centre, 1, 1, 4, F(0.9), "global")
    keys_w, vol_w = rep.lattice_search(None, 0, centre, 1, 1, 4, F(0.9), scores=True)
    assert not np.array_equal(vol_w, want)
    rep.close()


# ---- the room of cases 5 and 6, scrolled out of the window --------------------------------------------------------------------------
ROOM_SHIFT = (320, -288)                                                   # more than the window's 256 cells on both axes
ROOM_TILE = 64
# the lattice: level 2 (0.2 m), centred on the middle of the empty window, wide enough to reach the room 16.3 m and 13.7 m away
WIDE = (L.ROOM_LEVELS - 1, 90, 76, 72, F(math.radians(5.0)))
WIDE_CENTRE = np.array([6.4, 6.4, L.ROOM_CENTRE[2]], np.float32)


def scrolled_room(hs_mod, ctx, sim):
    rep = hs_mod.MapRepMultiMap(L.ROOM_CELL, (L.ROOM_W, L.ROOM_W), L.ROOM_LEVELS, ctx=ctx)
    rep.set_backing(ROOM_TILE, POOL)
    for xy, p in L.room(sim)[0]:
        rep.UpdateByScan(hs_mod.ScanCloud(xy), p)
    rep.shift(*ROOM_SHIFT)
    return rep


def scroll_rule(x, stm0, half, g):
    """q = ((c - half) / g) * g, C division, with c = (int)floorf(x * stm0)."""
    d = int(np.floor(F(F(x) * stm0))) - half
    return (abs(d) // g) * g * (1 if d >= 0 else -1)


# ---- 5. relocalise_world is search, shift, match-best ------------------------------------------------------------------------------
@gpu
def test_relocalise_world_is_search_shift_match_best(hs_mod, ctx, sim):
    a, b = scrolled_room(hs_mod, ctx, sim), scrolled_room(hs_mod, ctx, sim)
    scan = hs_mod.ScanCloud(L.room(sim)[1])
    level, nx, ny, n_th, dth = WIDE
    B = 4
    m = hs_mod.ScanMatcher(1)
    for l in range(L.ROOM_LEVELS):                                         # the room lies wholly in tiles
        assert not a.Maps[l].GetCells()["value"].any()
    st0 = a.backing_stats()
    # by hand, on the twin
    keys, _ = b.world_lattice_search(scan, level, WIDE_CENTRE, nx, ny, n_th, dth)
    assert np.array_equal(b.lattice_search(None, level, WIDE_CENTRE, nx, ny, n_th, dth)[0], np.full(n_th, L.EMPTY_KEY, np.uint64))
    order = L.sorted_headings(keys)[:B]
    nodes = [(k,) + hs_mod.decode_lattice_key(keys[k]) for k in order]     # (k, score, flat)
    hints = np.array([b.lattice_node_pose(level, WIDE_CENTRE, nx, ny, n_th, dth, k, flat) for k, _, flat in nodes], np.float32)
    cell0 = F(b.Maps[0].CellLength); stm0 = F(1.0) / cell0
    g = 1 << (L.ROOM_LEVELS - 1)
    q = [scroll_rule(hints[0][i], stm0, L.ROOM_W // 2, g) for i in range(2)]
    b.shift(*q)
    for i in range(2):
        hints[:, i] = hints[:, i] - F(F(q[i]) * cell0)
    inside = [i == 0 or all(F(0) <= F(hints[i][c] * stm0) < F(L.ROOM_W) for c in range(2)) for i in range(len(hints))]
    kept = [i for i in range(len(hints)) if inside[i]]
    want_pose, want_idx, want_rep = m.MatchDataBest(b, scan, hints[kept])
    # the call
    pose, rpt, info = m.RelocaliseWorld(a, scan, level, WIDE_CENTRE, nx, ny, n_th, dth, B=B)
    assert (int(info["dx"]), int(info["dy"])) == tuple(q) and q != [0, 0]
    assert a.origin() == (ROOM_SHIFT[0] + q[0], ROOM_SHIFT[1] + q[1]) == b.origin()
    st1 = a.backing_stats()
    assert st1["restored_cells"] > st0["restored_cells"] and st1["dropped_cells"] == 0
    assert S.same_bits(pose, want_pose) and rpt.tobytes() == want_rep.tobytes()
    k, score, flat = nodes[kept[want_idx]]
    NX = 2 * nx + 1
    assert (int(info["n_hints"]), int(info["n_far"]), int(info["best_hint"])) == (len(kept), B - len(kept), want_idx)
    assert (int(info["k"]), int(info["ix"]), int(info["iy"]), int(info["score"])) == (k, flat % NX - nx, flat // NX - ny, score)
    assert int(info["top_score"]) == nodes[0][1]
    for l in range(L.ROOM_LEVELS):
        assert np.array_equal(S.raw(a.Maps[l].GetCells()), S.raw(b.Maps[l].GetCells())), l
        assert a.Maps[l].GetCells()["value"].any()
    # found: test_it_relocalises' bounds, in the world frame
    ox, oy = a.origin()
    world = np.array([pose[0] + F(ox) * cell0, pose[1] + F(oy) * cell0, pose[2]], np.float32)
    start = np.array([hints[kept[want_idx]][0] + F(ox) * cell0, hints[kept[want_idx]][1] + F(oy) * cell0, hints[kept[want_idx]][2]], np.float32)
    e_pose, e_start = L.pose_error(world), L.pose_error(start)
    assert e_pose[0] <= e_start[0] and e_pose[1] <= e_start[1], (e_pose, e_start)
    assert e_pose[0] < 0.05, e_pose
    a.close(); b.close()


# ---- 6. the processor --------------------------------------------------------------------------------------------------------------
def scrolled_proc(hs_mod, ctx, sim):
    scans = L.room(sim)[0]
    proc = hs_mod.HectorSLAMProcessor(L.ROOM_CELL, (L.ROOM_W, L.ROOM_W), scans[0][1], L.ROOM_LEVELS, ctx=ctx, scrollBacking=(ROOM_TILE, POOL))
    for sxy, p in scans:
        proc.Update(hs_mod.ScanCloud(sxy), p, mapWithoutMatching=True)
    stored = (proc.MatchPose, proc.LastMapUpdatePose)                      # (origin (0, 0): the stored bits themselves)
    proc.shift(*ROOM_SHIFT)
    return proc, stored


@gpu
def test_processor_relocalise_world(hs_mod, ctx, sim):
    xy = L.room(sim)[1]
    scan = hs_mod.ScanCloud(xy)
    level, nx, ny, n_th, dth = WIDE
    cell0 = F(L.ROOM_CELL)
    proc, stored = scrolled_proc(hs_mod, ctx, sim)
    twin, _ = scrolled_proc(hs_mod, ctx, sim)
    off0 = np.array([F(ROOM_SHIFT[0]) * cell0, F(ROOM_SHIFT[1]) * cell0], np.float32)
    centre_world = np.array([WIDE_CENTRE[0] + off0[0], WIDE_CENTRE[1] + off0[1], WIDE_CENTRE[2]], np.float32)
    cw = np.array([centre_world[0] - off0[0], centre_world[1] - off0[1], centre_world[2]], np.float32)       # as the library takes it to the window
    want, want_rep, want_info = hs_mod.ScanMatcher(1).RelocaliseWorld(twin.MapRep, scan, level, cw, nx, ny, n_th, dth, B=4)
    q = (int(want_info["dx"]), int(want_info["dy"]))
    origin = (ROOM_SHIFT[0] + q[0], ROOM_SHIFT[1] + q[1])
    off1 = np.array([F(origin[0]) * cell0, F(origin[1]) * cell0], np.float32)
    want_world = np.array([want[0] + off1[0], want[1] + off1[1], want[2]], np.float32)
    # adopt = False: the stored poses are the old ones minus the shift
    pose, rpt, info = proc.RelocaliseWorld(scan, centre_world, level, nx, ny, n_th, dth, B=4, adopt=False)
    assert proc.get_origin() == origin and q != (0, 0)
    assert S.same_bits(pose, want_world) and rpt.tobytes() == want_rep.tobytes() and info.tobytes() == want_info.tobytes()
    for got, s0 in zip((proc.MatchPose, proc.LastMapUpdatePose), stored):
        s1 = [F(F(s0[i] - F(F(ROOM_SHIFT[i]) * cell0)) - F(F(q[i]) * cell0)) for i in range(2)]            # window frame: shift, then the relocalisation's shift
        assert S.same_bits(got, np.array([s1[0] + off1[0], s1[1] + off1[1], s0[2]], np.float32))
    assert L.pose_error(pose)[0] < 0.05
    # adopt = True: both become the result (the window is at the room now: the second call moves it by less than g, or not at all)
    pose2, _, info2 = proc.RelocaliseWorld(scan, centre_world, level, nx, ny, n_th, dth, B=4, adopt=True)
    assert S.same_bits(proc.MatchPose, pose2) and S.same_bits(proc.LastMapUpdatePose, pose2)
    assert L.pose_error(pose2)[0] < 0.05
    assert proc.get_origin() == (origin[0] + int(info2["dx"]), origin[1] + int(info2["dy"]))
    # the next Update matches from the adopted pose and, the robot not having moved, does not draw into the map
    sums = [proc.MapRep.Maps[l].checksum() for l in range(L.ROOM_LEVELS)]
    assert proc.Update(scan, proc.MatchPose) is False
    assert [proc.MapRep.Maps[l].checksum() for l in range(L.ROOM_LEVELS)] == sums
    assert L.pose_error(proc.MatchPose)[0] < 0.05 and S.same_bits(proc.LastMapUpdatePose, pose2)
    with pytest.raises(hs_mod.capi.SlamhipError) as e:
        capi = hs_mod.capi
        spec = capi.lattice_spec(level, centre_world, nx, ny, n_th, dth)
        out = np.empty(3, np.float32); r = np.zeros(1, capi.REPORT_DTYPE); inf = capi.WorldRelocInfo()
        capi.call("slamhip_hsproc_relocalise_world", proc._h, capi.fptr(scan.Points), scan.Points.shape[0], None, C.byref(spec), 4, 2,
                  capi.fptr(out), capi.rptr(r), C.byref(inf))
    assert e.value.code == hs_mod.capi.ERR_INVALID
    proc.Dispose(); twin.Dispose()


# ---- 7. errors change nothing ------------------------------------------------------------------------------------------------------
@gpu
def test_errors_change_nothing(hs_mod, ctx):
    capi = hs_mod.capi
    lib = capi.lib()
    rng = np.random.default_rng(31)
    pts = L.small_points(np.random.default_rng(11), 97)
    pts[20] = (2.0e5, 0.0)                                                 # 2e6 cells of level 0 away: counts (< 2^24), and bounds nothing
    good = dict(level=0, centre=(1.0, 1.0, 0.0), nx=2, ny=2, n_theta=3, dtheta=0.1)

    def attempt(rep, spec):
        """(rc of the world search, rc of relocalise_world), outputs untouched."""
        keys = np.full(4097, 7, np.uint64)
        pose = np.full(3, 5, np.float32); r = np.zeros(1, capi.REPORT_DTYPE); info = capi.WorldRelocInfo()
        rc = (lib.slamhip_hs_world_lattice_search(rep._h, C.byref(spec), keys.ctypes.data_as(C.POINTER(C.c_uint64)), None),
              lib.slamhip_hs_relocalise_world(rep._h, C.byref(spec), 4, capi.fptr(pose), capi.rptr(r), C.byref(info)))
        assert (rc[0] == 0 or (keys == 7).all()) and (pose == 5).all()
        return rc

    def state(rep):
        return rep.origin(), rep.backing_stats(), [S.raw(rep.Maps[l].GetCells()).copy() for l in range(2)]

    def same(s0, s1):
        return s0[0] == s1[0] and s0[1] == s1[1] and all(np.array_equal(x, y) for x, y in zip(s0[2], s1[2]))

    spec = capi.lattice_spec(**good)
    # backing off: the search works, the relocalisation refuses
    rep = hs_mod.MapRepMultiMap(0.1, (80, 48), 2, ctx=ctx)
    fill(hs_mod, rep, rng)
    rep.shift(6, -4)
    rep.set_scan(hs_mod.ScanCloud(pts))
    s0 = state(rep)
    assert attempt(rep, spec) == (0, capi.ERR_STATE) and same(s0, state(rep))
    rep.close()
    # backing on
    rep = hs_mod.MapRepMultiMap(0.1, (80, 48), 2, ctx=ctx)
    rep.set_backing(8, POOL)
    # no scan
    assert attempt(rep, spec) == (capi.ERR_STATE, capi.ERR_STATE)
    fill(hs_mod, rep, rng)
    rep.shift(34, -22)
    fill(hs_mod, rep, rng)
    rep.set_scan(hs_mod.ScanCloud(pts))
    s0 = state(rep)
    assert s0[1]["tiles"] > 0
    # the reference's cache on
    rep.set_reference_cache(1)
    assert attempt(rep, spec) == (0, capi.ERR_INVALID) and same(s0, state(rep))
    rep.set_reference_cache(0)
    # a bad spec
    for change in (dict(level=2), dict(nx=4097), dict(n_theta=0), dict(centre=(np.nan, 0.0, 0.0)), dict(dtheta=np.inf)):
        a = dict(good, **change)
        bad = capi.lattice_spec(a["level"], a["centre"], a["nx"], a["ny"], a["n_theta"], a["dtheta"])
        assert attempt(rep, bad) == (capi.ERR_INVALID, capi.ERR_INVALID), change
    pose = np.full(3, 5, np.float32); r = np.zeros(1, capi.REPORT_DTYPE); info = capi.WorldRelocInfo()
    for B in (0, 65):
        assert lib.slamhip_hs_relocalise_world(rep._h, C.byref(spec), B, capi.fptr(pose), capi.rptr(r), C.byref(info)) == capi.ERR_INVALID
    assert same(s0, state(rep))
    # R too large: one non-Reset cell 3e6 cells away on both axes
    far = np.zeros((1, 1), capi.CELL_DTYPE)
    far["update_index"] = 1; far["value"] = 1.0
    assert rep.world_put(0, 3000000, 3000000, far) == 0
    s1 = state(rep)
    assert s1[1]["tiles"] == s0[1]["tiles"] + 1
    assert attempt(rep, spec) == (capi.ERR_INVALID, capi.ERR_INVALID)
    # R in world cells of level 0: the first window's tiles start at (0, 0), the window at (34, -22), the far tile ends at 3000008
    msg = lib.slamhip_last_error().decode()
    assert "2^28" in msg and "is 3000008 x 3000030 cells" in msg, msg
    assert same(s1, state(rep))
    # level 1 holds no far tile: its search goes through
    keys, _ = rep.world_lattice_search(None, 1, (1.0, 1.0, 0.0), 2, 2, 3, 0.1)
    assert keys.shape == (3,)
    rep.close()


# ---- 8. other flows launch what they launched --------------------------------------------------------------------------------------
@gpu
def test_other_flows_launch_what_they_launched(hs_mod, sim):
    """Match, update, shift, the window search and Relocalise issue what test_gpu_hector_lattice counts for them and no world pack;
    a world search is one world pack and one search launch, and no window pack."""
    capi = hs_mod.capi
    own = hs_mod.Context(0)
    own.timing_enable(-1)
    rep = hs_mod.MapRepMultiMap(S.CELL, (64, 64), S.LEVELS, ctx=own)
    rep.set_backing(8, POOL)
    scans = S.local_scans(sim, 64, 64)
    m = hs_mod.ScanMatcher(1)
    for xy, p in scans:
        m.MatchData(rep, hs_mod.ScanCloud(xy), p)
        rep.UpdateByScan(hs_mod.ScanCloud(xy), p)
    rep.shift(S.G, 0)
    classes = (capi.K_HS_MATCH, capi.K_HS_UPDATE, capi.K_HS_LATTICE_PACK, capi.K_HS_LATTICE, capi.K_HS_LATTICE_PACK_WORLD)
    counts = lambda: [own.timing_get(k)[1] for k in classes]
    c0 = counts()
    assert c0[0] == len(scans) and c0[1] >= len(scans) and c0[2:] == [0, 0, 0]
    scan, p = hs_mod.ScanCloud(scans[-1][0]), scans[-1][1]
    rep.lattice_search(scan, 1, p, 2, 2, 3, 0.1)
    assert counts() == [c0[0], c0[1], 1, 1, 0]
    m.Relocalise(rep, scan, 1, p, 2, 2, 3, 0.1, B=2)
    assert counts() == [c0[0] + 1, c0[1], 2, 2, 0]
    rep.world_lattice_search(scan, 1, p, 2, 2, 3, 0.1)
    assert counts() == [c0[0] + 1, c0[1], 2, 3, 1]
    m.RelocaliseWorld(rep, scan, 1, p, 2, 2, 3, 0.1, B=2)
    assert counts() == [c0[0] + 2, c0[1], 2, 4, 2]
    rep.close()
    own.close()
