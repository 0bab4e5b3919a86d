"""The branch-and-bound pose-lattice search (K24: slamhip_hs_lattice_search_bnb, slamhip_hs_relocalise_bnb,
slamhip_hsproc_relocalise_bnb) on the device: against the host hook, which tests/test_hs_bnb_abi.py pins against K7's exhaustive
definition and the NumPy restatement of the rules without a GPU; against K7 itself (slamhip_hs_lattice_search,
slamhip_hs_world_lattice_search, the Relocalise family) from the same handle; and on one lattice K7 refuses.  Keys, infos, poses
and reports are compared with == on integers and on bit patterns; there is no tolerance.  The cases and what each is for:
tests/bnb_cases.py."""
import ctypes as C
import math

import numpy as np
import pytest

import bnb_cases as B
import test_gpu_hector_lattice as L
import test_gpu_hector_shift as S
import test_gpu_hector_world_lattice as WL
from test_gpu_hector_lattice import room_rep                               # noqa: F401 (fixture)
from test_gpu_hector_shift import hs_mod, ctx, det                         # noqa: F401 (fixtures)
from test_gpu_hector_world_lattice import scattered                        # noqa: F401 (fixture)

gpu = pytest.mark.gpu
F = np.float32


def make_rep(hs_mod, ctx, mp):
    rep = hs_mod.MapRepMultiMap(mp["cell0"], mp["dims"], mp["levels"], ctx=ctx)
    for l, v in enumerate(mp["values"]):
        L.put_values(hs_mod, rep, l, v)
    return rep


@pytest.fixture(scope="module")
def reps(hs_mod, ctx):
    """The catalogue's maps on the device, each made by the first case that needs it."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = make_rep(hs_mod, ctx, B.map_of(name))
        return made[name]
    yield get
    for rep in made.values():
        rep.close()


def hook(capi, c, values, w, h, cell, **kw):
    spec = capi.bnb_spec(c["level"], c["centre"], c["nx"], c["ny"], c["n_theta"], c["dtheta"], c["top"], **kw)
    keys, info = capi.bnb_call(values, w, h, cell, spec, c["xy"])
    return keys, B.info_dict(info)


# ---- 1. every case: the hook, and K7 from the same handle ------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", list(B.CASES))
def test_device_equals_hook_and_k7(hs_mod, reps, name):
    c = B.CASES[name]
    rep = reps(c["map"])
    values, w, h, cell = B.level_of(c)
    assert rep.Maps[c["level"]].Dimensions == (w, h) and F(rep.Maps[c["level"]].CellLength) == cell
    lat = (c["level"], c["centre"], c["nx"], c["ny"], c["n_theta"], c["dtheta"])
    keys, info = rep.lattice_search_bnb(hs_mod.ScanCloud(c["xy"]), *lat, c["top"])
    want_keys, want_info = hook(hs_mod.capi, c, values, w, h, cell)
    assert np.array_equal(keys, want_keys), name
    assert B.info_dict(info) == want_info, (name, B.info_dict(info), want_info)
    k7, _ = rep.lattice_search(None, *lat)
    assert np.array_equal(keys, k7), name
    keys2, info2 = rep.lattice_search_bnb(None, *lat, c["top"])           # again on the same handle: the unit's blocks are reused
    assert np.array_equal(keys2, keys) and info2.tobytes() == info.tobytes()


# ---- 2. the world ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("level", [0, 1])
def test_world_equals_the_world_search(hs_mod, scattered, level):          # noqa: F811
    rep = scattered
    assert rep.backing_stats()["tiles"] > 20
    scan = hs_mod.ScanCloud(L.small_points(np.random.default_rng(11), 97))
    lat = (level, np.array([0.27, 0.13, 0.3], np.float32), 40, 30, 5, F(0.4))
    want, _ = rep.world_lattice_search(scan, *lat)
    window, _ = rep.lattice_search(None, *lat)
    assert not np.array_equal(want, window)                                # the tiles matter here
    for top in (0, 3, 6):                                                  # R's origin, tile edges and the margin fall inside packed words
        keys, info = rep.lattice_search_bnb(None, *lat, top, world=True)
        assert np.array_equal(keys, want), (level, top)
        assert int(info["top"]) == top and int(info["evaluated"]) == int(info["blocks"].sum())
        keys_w, _ = rep.lattice_search_bnb(None, *lat, top, world=False)
        assert np.array_equal(keys_w, window), (level, top)


@gpu
def test_world_with_backing_off_is_the_window(hs_mod, reps):
    c = B.CASES["corner_top2_l1"]
    rep = reps("small")
    lat = (c["level"], c["centre"], c["nx"], c["ny"], c["n_theta"], c["dtheta"])
    a = rep.lattice_search_bnb(hs_mod.ScanCloud(c["xy"]), *lat, c["top"], world=False)
    b = rep.lattice_search_bnb(None, *lat, c["top"], world=True)
    assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes()


# ---- 3. the Relocalise family ------------------------------------------------------------------------------------------------------
@gpu
def test_relocalise_bnb_is_relocalise(hs_mod, ctx, room_rep, sim):         # noqa: F811
    scans, xy = L.room(sim)
    scan = hs_mod.ScanCloud(xy)
    level, nx, ny, n_theta, dth = L.ROOM_LATTICE
    m = hs_mod.ScanMatcher(1)
    want = m.Relocalise(room_rep, scan, level, L.ROOM_CENTRE, nx, ny, n_theta, dth, B=4)
    got = m.Relocalise(room_rep, scan, level, L.ROOM_CENTRE, nx, ny, n_theta, dth, B=4, search="bnb", top=2)
    assert len(want) == 3 and len(got) == 4
    assert S.same_bits(got[0], want[0]) and got[1].tobytes() == want[1].tobytes() and got[2].tobytes() == want[2].tobytes()
    assert int(got[3]["top"]) == 2 and 0 < int(got[3]["evaluated"])
    assert L.pose_error(got[0])[0] < 0.05
    # the processor: adopt as today
    proc = hs_mod.HectorSLAMProcessor(L.ROOM_CELL, (L.ROOM_W, L.ROOM_W), scans[0][1], L.ROOM_LEVELS, ctx=ctx, scrollTrigger=100)
    for sxy, p in scans:
        proc.Update(hs_mod.ScanCloud(sxy), p, mapWithoutMatching=True)
    before = (proc.MatchPose, proc.LastMapUpdatePose)
    want = proc.Relocalise(scan, L.ROOM_CENTRE, level, nx, ny, n_theta, dth, B=4, adopt=False)
    got = proc.Relocalise(scan, L.ROOM_CENTRE, level, nx, ny, n_theta, dth, B=4, adopt=False, search="bnb")      # top=None
    assert S.same_bits(got[0], want[0]) and got[1].tobytes() == want[1].tobytes() and got[2].tobytes() == want[2].tobytes()
    assert int(got[3]["top"]) == hs_mod.BNB_DEFAULT_TOP
    assert S.same_bits(proc.MatchPose, before[0]) and S.same_bits(proc.LastMapUpdatePose, before[1])
    ver = proc.VerifyLoop(scan, {"pose": L.ROOM_CENTRE}, level, nx, ny, n_theta, dth, B=4, search="bnb", top=3)
    assert S.same_bits(ver[0], want[0]) and S.same_bits(proc.MatchPose, before[0])
    got = proc.Relocalise(scan, L.ROOM_CENTRE, level, nx, ny, n_theta, dth, B=4, adopt=True, search="bnb", top=3)
    assert S.same_bits(got[0], want[0]) and S.same_bits(proc.MatchPose, want[0]) and S.same_bits(proc.LastMapUpdatePose, want[0])
    with pytest.raises(hs_mod.capi.SlamhipError) as e:
        capi = hs_mod.capi
        spec = capi.bnb_spec(level, L.ROOM_CENTRE, nx, ny, n_theta, dth, 3)
        out = np.empty(3, np.float32); r = np.zeros(1, capi.REPORT_DTYPE); inf = capi.RelocInfo(); bi = capi.BnbInfo()
        capi.call("slamhip_hsproc_relocalise_bnb", proc._h, capi.fptr(scan.Points), scan.Points.shape[0], None, C.byref(spec), 4, 2,
                  capi.fptr(out), capi.rptr(r), C.byref(inf), C.byref(bi))
    assert e.value.code == hs_mod.capi.ERR_INVALID
    proc.Dispose()


@gpu
def test_relocalise_world_bnb_is_relocalise_world(hs_mod, ctx, sim):
    scan = hs_mod.ScanCloud(L.room(sim)[1])
    level, nx, ny, n_th, dth = WL.WIDE
    a, b = WL.scrolled_room(hs_mod, ctx, sim), WL.scrolled_room(hs_mod, ctx, sim)
    m = hs_mod.ScanMatcher(1)
    want = m.RelocaliseWorld(b, scan, level, WL.WIDE_CENTRE, nx, ny, n_th, dth, B=4)
    got = m.RelocaliseWorld(a, scan, level, WL.WIDE_CENTRE, nx, ny, n_th, dth, B=4, search="bnb", top=4)
    assert S.same_bits(got[0], want[0]) and got[1].tobytes() == want[1].tobytes() and got[2].tobytes() == want[2].tobytes()
    assert (int(got[2]["dx"]), int(got[2]["dy"])) != (0, 0) and a.origin() == b.origin()
    for l in range(L.ROOM_LEVELS):
        assert np.array_equal(S.raw(a.Maps[l].GetCells()), S.raw(b.Maps[l].GetCells())), l
    a.close(); b.close()
    # the processor's form, and the pre-checks of slamhip_hs_relocalise_world
    proc, _ = WL.scrolled_proc(hs_mod, ctx, sim)
    twin, _ = WL.scrolled_proc(hs_mod, ctx, sim)
    cell0 = F(L.ROOM_CELL)
    cw = np.array([WL.WIDE_CENTRE[0] + F(WL.ROOM_SHIFT[0]) * cell0, WL.WIDE_CENTRE[1] + F(WL.ROOM_SHIFT[1]) * cell0, WL.WIDE_CENTRE[2]], np.float32)
    want = twin.RelocaliseWorld(scan, cw, level, nx, ny, n_th, dth, B=4, adopt=True)
    got = proc.RelocaliseWorldBnb(scan, cw, level, nx, ny, n_th, dth, B=4, adopt=True, top=4)
    assert S.same_bits(got[0], want[0]) and got[1].tobytes() == want[1].tobytes() and got[2].tobytes() == want[2].tobytes()
    assert proc.get_origin() == twin.get_origin() and S.same_bits(proc.MatchPose, twin.MatchPose)
    assert S.same_bits(proc.LastMapUpdatePose, twin.LastMapUpdatePose)
    proc.Dispose(); twin.Dispose()
    plain = hs_mod.MapRepMultiMap(0.1, (80, 48), 2, ctx=ctx)               # backing off: refused before anything moves
    with pytest.raises(hs_mod.capi.SlamhipError) as e:
        m.RelocaliseWorld(plain, scan, 0, (1.0, 1.0, 0.0), 2, 2, 3, 0.1, search="bnb")
    assert e.value.code == hs_mod.capi.ERR_STATE
    plain.close()


# ---- 4. rule 5 on the device, and rule 1 ---------------------------------------------------------------------------------------------
@gpu
def test_capacity_and_refusals(hs_mod, ctx, reps):
    capi = hs_mod.capi
    c = B.CASES["corner_top2"]
    rep = reps("small")
    rep.set_scan(hs_mod.ScanCloud(c["xy"]))
    values, w, h, cell = B.level_of(c)
    sums = [rep.Maps[l].checksum() for l in range(2)]

    def raw(**kw):
        a = dict(level=0, centre=c["centre"], nx=5, ny=3, n_theta=7, dtheta=0.4, top=2, world=0, max_blocks=0, reserved=0)
        a.update(kw)
        spec = capi.bnb_spec(a["level"], a["centre"], a["nx"], a["ny"], a["n_theta"], a["dtheta"], a["top"], a["world"], a["max_blocks"], a["reserved"])
        keys = np.full(4097, 7, np.uint64)
        info = capi.BnbInfo(); info.top = 77
        rc = capi.lib().slamhip_hs_lattice_search_bnb(rep._h, C.byref(spec), keys.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(info))
        return rc, keys, info
    # rule 5: 42 top blocks pass rule 1; the hook says where the search ends
    assert B.np_bnb(values, w, h, cell, c["centre"], 5, 3, 7, c["dtheta"], 2, c["xy"], max_blocks=42) is None
    rc, keys, info = raw(max_blocks=42)
    assert rc == capi.ERR_INVALID and (keys == 7).all() and info.top == 77
    msg = capi.lib().slamhip_last_error().decode()
    assert "height 1" in msg and "max_blocks" in msg and "top" in msg
    rc, keys, info = raw()                                                 # the next call on the same handle succeeds
    assert rc == capi.OK and np.array_equal(keys[:7], B.reference("corner_top2")[0]) and B.info_dict(capi.bnb_info(info)) == B.reference("corner_top2")[1]
    # rule 1
    for change in (dict(top=-1), dict(top=9), dict(world=2), dict(world=-1), dict(reserved=1), dict(max_blocks=-1), dict(max_blocks=41), dict(level=2),
                   dict(level=-1), dict(nx=4097), dict(ny=-1), dict(n_theta=0), dict(n_theta=4097), dict(centre=(np.nan, 0.0, 0.0)), dict(dtheta=np.inf),
                   dict(nx=4096, ny=4096, n_theta=4096, top=0)):
        rc, keys, info = raw(**change)
        assert rc == capi.ERR_INVALID and (keys == 7).all() and info.top == 77, change
    assert [rep.Maps[l].checksum() for l in range(2)] == sums
    fresh = hs_mod.MapRepMultiMap(0.1, (80, 48), 2, ctx=ctx)               # no scan
    spec = capi.bnb_spec(0, c["centre"], 5, 3, 7, 0.4, 2)
    keys = np.full(7, 7, np.uint64); info = capi.BnbInfo()
    assert capi.lib().slamhip_hs_lattice_search_bnb(fresh._h, C.byref(spec), keys.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(info)) == capi.ERR_STATE
    assert (keys == 7).all()
    fresh.close()


# ---- 5. beyond 2^26 nodes ----------------------------------------------------------------------------------------------------------
@gpu
def test_a_lattice_k7_refuses(hs_mod, ctx):
    """511 x 511 x 360 = 9.4e7 nodes on a 512 x 512 level: every cell free but the scan's end cells at one planted node.  The hook
    takes 0.05 s for it on the host (160041 blocks evaluated)."""
    capi = hs_mod.capi
    xy = B.small_points(np.random.default_rng(11), 97)
    centre = np.array([12.8, 12.8, 0.0], np.float32)
    nx = ny = 255; n_theta = 360; dth = F(2 * math.pi / 360); top = 6
    node = (40, 65, -127)                                                  # ix + nx = 320, iy + ny = 128: an origin of the top grid
    values, n_in = B.peak_values(512, 512, 0.05, centre, nx, ny, dth, xy, node)
    assert n_in == 95 and (2 * nx + 1) * (2 * ny + 1) * n_theta > 1 << 26
    rep = hs_mod.MapRepMultiMap(0.05, (512, 512), 1, ctx=ctx)
    L.put_values(hs_mod, rep, 0, values)
    scan = hs_mod.ScanCloud(xy)
    with pytest.raises(capi.SlamhipError) as e:
        rep.lattice_search(scan, 0, centre, nx, ny, n_theta, dth)
    assert e.value.code == capi.ERR_INVALID
    keys, info = rep.lattice_search_bnb(None, 0, centre, nx, ny, n_theta, dth, top)
    spec = capi.bnb_spec(0, centre, nx, ny, n_theta, dth, top)
    want_keys, want_info = capi.bnb_call(values, 512, 512, F(0.05), spec, xy)
    assert np.array_equal(keys, want_keys) and info.tobytes() == want_info.tobytes()
    k = int(np.argmax(keys))
    score, flat = hs_mod.decode_lattice_key(keys[k])
    assert (k, flat % 511 - nx, flat // 511 - ny, score) == (node[0], node[1], node[2], n_in)
    assert int(info["evaluated"]) < (2 * nx + 1) * (2 * ny + 1) * n_theta // 100
    rep.close()
