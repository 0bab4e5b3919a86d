"""K20 on the device: slamhip_hs_render and the scan store through MapRepMultiMap / HectorSLAMProcessor.  Every render is held to ==
against BOTH a second handle that runs the sequential set_scan + UpdateByScan loop on the device and the host hook
(slamhip_debug_render): every level's cells (update index and value bits), slamhip_hs_probability over all cells, slamhip_hs_checksum,
the bitmap -- and once more after one further ordinary UpdateByScan on both handles, which proves that the host's indices and epoch
moved.  The cases: tests/render_cases.py (each checked on the CPU by tests/test_hs_render_abi.py).  The whole group runs again in a
fresh interpreter with the other tile side (SLAMHIP_K20_TILE=64)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import k5_cases as kc
import render_cases as rc
from test_gpu_hector import hs_mod, ctx                                  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

INT_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def capi():
    import slam.net_amd.capi as capi
    return capi


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_cells(got, ref, what):
    for field in ("update_index", "value"):
        g, r = bits(got[field]), bits(ref[field])
        bad = np.flatnonzero(g != r)
        assert bad.size == 0, (what, field, bad.size, bad[:8], got[field][bad[:8]], ref[field][bad[:8]])


def same_maps(a, b, what, hook_cells=None):
    """Two pyramids on the device, bit for bit: cells, probabilities, checksum, bitmap; and the hook's cells, if given."""
    for l in range(a.NumLevels):
        ca, cb = a.Maps[l].GetCells(), b.Maps[l].GetCells()
        same_cells(ca, cb, (what, l, "loop"))
        if hook_cells is not None:
            same_cells(ca, hook_cells[l], (what, l, "hook"))
        idx = np.arange(ca.size, dtype=np.int32)
        assert (bits(a.Maps[l].GetCachedProbability(idx)) == bits(b.Maps[l].GetCachedProbability(idx))).all(), (what, l, "probability")
        assert a.Maps[l].checksum() == b.Maps[l].checksum(), (what, l, "checksum")
        assert (a.Maps[l].GetBitmapData() == b.Maps[l].GetBitmapData()).all(), (what, l, "bitmap")


def one_more(hs_mod, a, b, size, what):
    """One further ordinary update on both handles: equal only if the render left the host's indices where the loop left them."""
    sc = hs_mod.ScanCloud(np.array([[5.0, 2.0], [-3.0, 4.0], [2.0, -6.0]], np.float32))
    pose = (size[0] // 2, size[1] // 2, 0.0)
    a.UpdateByScan(sc, pose); b.UpdateByScan(sc, pose)
    same_maps(a, b, (what, "one more update"))


def make(hs_mod, ctx, b):
    rep = hs_mod.MapRepMultiMap(b.cell_len, b.size, b.levels, ctx=ctx)
    if b.factors:
        rep.SetUpdateFactorFree(b.factors[0]); rep.SetUpdateFactorOccupied(b.factors[1])
    return rep


def store(hs_mod, rep, b):
    for xy, origin, _ in b.steps:
        rep.ScansAdd(hs_mod.ScanCloud(xy, (origin[0], origin[1], 0.0)))
    return np.array([s[2] for s in b.steps], np.float32).reshape(-1, 3)


def loop(hs_mod, rep, b, first=0, last=None):
    for xy, origin, pose in b.steps[first:last]:
        rep.UpdateByScan(hs_mod.ScanCloud(xy, (origin[0], origin[1], 0.0)), pose)


def hook(capi, b, first=0, last=None, cells=None, ui=None, keep=False):
    dims = kc.level_dims(b.size, b.levels)
    if cells is None:
        cells = [np.zeros(w * h, kc.CELL) for w, h in dims]
    steps = b.steps[first:last]
    return capi.debug_render(dims, b.cell_len, cells, [0] * b.levels if ui is None else ui, [0] * b.levels, [s[0] for s in steps], [s[1] for s in steps],
                             [s[2] for s in steps], keep=keep, factors=b.factors or (0.4, 0.9))[0]


@pytest.mark.parametrize("name", list(rc.CASES))
def test_case(hs_mod, ctx, capi, name):
    b = rc.CASES[name]()
    a, ref = make(hs_mod, ctx, b), make(hs_mod, ctx, b)
    try:
        poses = store(hs_mod, a, b)
        assert a.ScansCount() == len(b.steps)
        a.Render(poses)
        loop(hs_mod, ref, b)
        same_maps(a, ref, name, hook(capi, b))
        if name == "clamp":
            assert a.Maps[0].GetCells()["value"].reshape(64, 64)[33, 40] >= 50.0
        one_more(hs_mod, a, ref, b.size, name)
    finally:
        a.close(); ref.close()


@pytest.mark.parametrize("split", ("0", "1", "N-1", "N"))
def test_sub_ranges_and_keep(hs_mod, ctx, capi, split):
    """render(0, a) then KEEP (a, N) equals render(0, N), for a in {0, 1, N - 1, N}; and render(2, 5) of a store of 8."""
    b = rc.CASES["six_scans_l2"]()
    N = len(b.steps)
    at = {"0": 0, "1": 1, "N-1": N - 1, "N": N}[split]
    a, ref = make(hs_mod, ctx, b), make(hs_mod, ctx, b)
    try:
        poses = store(hs_mod, a, b)
        a.Render(poses[:at], 0, at)
        a.Render(poses[at:], at, N, keep=True)
        loop(hs_mod, ref, b)
        same_maps(a, ref, ("split", split), hook(capi, b))
        one_more(hs_mod, a, ref, b.size, ("split", split))
    finally:
        a.close(); ref.close()


def test_middle_range_of_eight(hs_mod, ctx, capi):
    b6 = rc.CASES["six_scans_l2"]()
    b = kc.Built(b6.cell_len, b6.size, b6.levels, None, b6.steps + b6.steps[:2], None)
    a, ref = make(hs_mod, ctx, b), make(hs_mod, ctx, b)
    try:
        poses = store(hs_mod, a, b)
        a.Render(poses[2:5], 2, 5)
        loop(hs_mod, ref, b, 2, 5)
        same_maps(a, ref, "render(2, 5)", hook(capi, b, 2, 5))
        one_more(hs_mod, a, ref, b.size, "render(2, 5)")
    finally:
        a.close(); ref.close()


def test_keep_over_uploaded_cells(hs_mod, ctx, capi):
    """KEEP over cells uploaded with indices -1, curr .. curr + 3 and INT_MAX and values 49.9, 50, NaN and -0.0: the literal tests."""
    b = rc.CASES["tiles_65x63"]()
    w, h = b.size
    cells = np.zeros(w * h, kc.CELL)
    vals = np.array([49.9, 50.0, np.nan, -0.0], np.float32)
    k = np.arange(w * h)
    cells["value"] = vals[k % vals.size]
    # an upload moves the level's index past every uploaded index but INT_MAX, which nothing can pass: with 9 the largest other
    # index the level stands at curr = 12 after it, and the uploaded indices are -1, curr .. curr + 3 and INT_MAX
    curr = 12
    idxs = np.array([-1, 9, curr, curr + 1, curr + 2, curr + 3, INT_MAX], np.int32)
    cells["update_index"] = idxs[(k // vals.size) % idxs.size]
    first = cells.copy()
    first["update_index"][first["update_index"] > 9] = -1
    a, ref = make(hs_mod, ctx, b), make(hs_mod, ctx, b)
    try:
        for rep in (a, ref):
            rep.Maps[0].SetCells(first)                                   # (the level's index: 12)
            rep.Maps[0].SetCells(cells)                                   # (stays 12: curr + 3 asks for 18, INT_MAX for nothing)
        ui = kc.index_after_upload(cells, kc.index_after_upload(first, 0))
        assert kc.index_after_upload(first, 0) == curr
        poses = store(hs_mod, a, b)
        a.Render(poses, keep=True)
        loop(hs_mod, ref, b)
        same_maps(a, ref, "keep over upload", hook(capi, b, cells=[cells.copy()], ui=[ui], keep=True))
        one_more(hs_mod, a, ref, b.size, "keep over upload")
    finally:
        a.close(); ref.close()


def test_store(hs_mod, ctx, capi):
    """Add / info / download round trip with ==; xy == NULL takes the set scan; Reset empties the store and a later add starts at 0;
    ScansClear, then add again; a render leaves the handle's current scan as it was."""
    rep = hs_mod.MapRepMultiMap(1.0, (64, 64), 1, ctx=ctx)
    try:
        rng = np.random.default_rng(3)
        scans = [hs_mod.ScanCloud(rng.normal(0, 9, (n, 2)).astype(np.float32), (0.25 * n, -1.5, 0.0)) for n in (0, 1, 257, 1080, 3073, 5)]
        for k, sc in enumerate(scans):
            assert rep.ScansAdd(sc) == k
        assert rep.ScansCount() == len(scans)
        for k, sc in enumerate(scans):
            pts, org = rep.ScansGet(k)
            assert pts.shape == sc.Points.shape and (bits(pts) == bits(sc.Points)).all() and (bits(org) == bits(sc.Pose[:2])).all(), k
        rep.set_scan(scans[2])
        assert rep.ScansAdd() == len(scans)                               # xy == NULL: the scan that is set
        pts, org = rep.ScansGet(len(scans))
        assert (bits(pts) == bits(scans[2].Points)).all() and (bits(org) == bits(scans[2].Pose[:2])).all()
        with pytest.raises(capi.SlamhipError) as e:
            rep.ScansGet(len(scans) + 1)
        assert e.value.code == capi.ERR_INVALID
        with pytest.raises(capi.SlamhipError) as e:
            capi.call("slamhip_hs_scans_download", rep._h, 3, capi._vp(np.zeros((8, 2), np.float32)), 8)     # room for 8 of 1080 points
        assert e.value.code == capi.ERR_INVALID
        rep.Reset()
        assert rep.ScansCount() == 0 and rep.ScansAdd(scans[1]) == 0
        rep.ScansClear()
        assert rep.ScansCount() == 0 and rep.ScansAdd(scans[3]) == 0
        pts, _ = rep.ScansGet(0)
        assert (bits(pts) == bits(scans[3].Points)).all()
        # a render leaves the signature store, the pose graph and the current scan: SigDownload and PgGet give what they gave, and
        # a MATCH after the render, on a map made equal again, uses the scan set before it
        rep.SigConfigure(2.0, 8, 1)
        rep.set_scan(scans[3]); rep.SigAdd((1.0, 2.0, 0.5))
        rep.set_scan(scans[4]); rep.SigAdd((-3.0, 0.25, -0.5))
        sig0, sp0 = rep.SigDownload()
        gp = np.array([[0.0, 0.0, 0.0], [1.0, 0.5, 0.1]])
        rep.PgSet(gp, None, np.array([[0, 1]], np.int32), np.array([[1.0, 0.4, 0.1]]), np.array([[4.0, 4.0, 9.0]]))
        twin = hs_mod.MapRepMultiMap(1.0, (64, 64), 1, ctx=ctx)
        try:
            # the stored scan: the walls of a room of 24 x 24 cells seen from its middle; the scan that is set: every other point
            # of it, which a match pulls onto the walls; the scan it must not be taken for: a circle inside the room
            t = np.arange(-12.0, 12.0, 0.25)
            room = hs_mod.ScanCloud(np.concatenate([np.stack([t, np.full_like(t, -12.0)], 1), np.stack([np.full_like(t, 12.0), t], 1),
                                                    np.stack([-t, np.full_like(t, 12.0)], 1), np.stack([np.full_like(t, -12.0), -t], 1)]).astype(np.float32))
            probe = hs_mod.ScanCloud(room.Points[::2].copy())
            ang = np.linspace(0.0, 2.0 * np.pi, 97)[:-1]
            circle = hs_mod.ScanCloud((8.0 * np.stack([np.cos(ang), np.sin(ang)], 1)).astype(np.float32))
            rep.ScansClear(); rep.ScansAdd(room)
            for r in (rep, twin):
                r.set_scan(probe)
            rep.Render(np.array([[30.0, 30.0, 0.0]], np.float32))
            twin.UpdateByScan(room, (30.0, 30.0, 0.0))
            twin.set_scan(probe)
            sig1, sp1 = rep.SigDownload()
            assert sig1.tobytes() == sig0.tobytes() and sp1.tobytes() == sp0.tobytes() and rep.SigCount() == 2
            assert np.array_equal(rep.PgGet(), gp)
            out = []
            for r in (rep, twin):                                         # slamhip_hs_match on the scan that is set: no set_scan in between
                o = np.empty(3, np.float32)
                capi.call("slamhip_hs_match", r._h, capi.fptr(np.array([30.3, 29.8, 0.02], np.float32)), capi.fptr(o))
                out.append(o)
            assert bits(out[0]).tolist() == bits(out[1]).tolist()
            other_scan = np.empty(3, np.float32)
            twin.set_scan(circle)
            capi.call("slamhip_hs_match", twin._h, capi.fptr(np.array([30.3, 29.8, 0.02], np.float32)), capi.fptr(other_scan))
            assert bits(other_scan).tolist() != bits(out[0]).tolist()     # (the match does tell the two scans apart)
        finally:
            twin.close()
        rep.ScansClear(); rep.ScansAdd(scans[3])
        # ... and an update after a render draws the scan set before it
        other = hs_mod.MapRepMultiMap(1.0, (64, 64), 1, ctx=ctx)
        try:
            for r in (rep, other):
                r.set_scan(scans[5])
            rep.Render(np.array([[30.0, 30.0, 0.3]], np.float32))
            other.UpdateByScan(scans[3], (30.0, 30.0, 0.3))
            other.set_scan(scans[5])
            for r in (rep, other):
                capi.call("slamhip_hs_update_by_scan", r._h, capi.fptr(np.array([20.0, 25.0, 0.0], np.float32)))
            same_maps(rep, other, "current scan kept")
        finally:
            other.close()
    finally:
        rep.close()


def test_refusals(hs_mod, ctx, capi):
    """Every SLAMHIP_ERR_INVALID of the contract, each with the map's checksum and the indices unchanged."""
    b = rc.CASES["six_scans_l2"]()
    a, ref = make(hs_mod, ctx, b), make(hs_mod, ctx, b)
    try:
        poses = store(hs_mod, a, b)
        a.Render(poses)
        loop(hs_mod, ref, b)
        before = [m.checksum() for m in a.Maps]

        def refused(first, last, p, flags=0):
            with pytest.raises(capi.SlamhipError) as e:
                capi.call("slamhip_hs_render", a._h, first, last, capi._vp(np.ascontiguousarray(p, np.float32)), flags)
            assert e.value.code == capi.ERR_INVALID
            assert [m.checksum() for m in a.Maps] == before
        refused(-1, 2, poses[:3])
        refused(3, 2, poses[:1])
        refused(0, 7, np.zeros((7, 3), np.float32))
        refused(0, 6, poses, 2)
        for bad in (np.nan, np.inf):
            for k in range(3):
                p = poses.copy(); p[4, k] = bad
                refused(0, 6, p)
                refused(0, 6, p, capi.RENDER_KEEP)
        a.set_reference_cache(True)
        refused(0, 6, poses)
        a.set_reference_cache(False)
        # the update index: an upload moves it to just below INT_MAX - 3 * 6; KEEP then passes INT_MAX, a clearing render does not
        big = np.zeros(b.size[0] * b.size[1], kc.CELL)
        big["update_index"] = -1
        big["update_index"][0] = INT_MAX - 12
        a.Maps[0].SetCells(big); ref.Maps[0].SetCells(big)
        before = [m.checksum() for m in a.Maps]
        refused(0, 6, poses, capi.RENDER_KEEP)
        a.Render(poses[:2], 0, 2, keep=True)                              # (two scans still fit)
        loop(hs_mod, ref, b, 0, 2)
        same_maps(a, ref, "near INT_MAX")
        a.Render(poses)
        ref.Reset()
        loop(hs_mod, ref, b)
        same_maps(a, ref, "after the refusals")
        one_more(hs_mod, a, ref, b.size, "after the refusals")
    finally:
        a.close(); ref.close()


def test_empty_ranges(hs_mod, ctx, capi):
    """first == last without KEEP clears -- the indices too; with KEEP nothing happens."""
    b = rc.CASES["six_scans_l2"]()
    a, ref = make(hs_mod, ctx, b), make(hs_mod, ctx, b)
    try:
        poses = store(hs_mod, a, b)
        a.Render(poses)
        loop(hs_mod, ref, b)
        a.Render(poses[:0], 3, 3, keep=True)
        same_maps(a, ref, "empty KEEP")
        a.Render(poses[:0], 3, 3)
        ref.Reset()
        same_maps(a, ref, "empty render clears")
        assert a.ScansCount() == 6                                        # (the store is not the map)
        one_more(hs_mod, a, ref, b.size, "empty render clears")
    finally:
        a.close(); ref.close()


def test_processor_after_shift(hs_mod, ctx, capi):
    """A render after a window shift: the origin is kept, and slamhip_hsproc_render takes world poses to the window's frame."""
    b = rc.CASES["six_scans_l2"]()
    p = hs_mod.HectorSLAMProcessor(1.0, b.size, (0.0, 0.0, 0.0), b.levels, ctx=ctx)
    ref = make(hs_mod, ctx, b)
    try:
        p.shift(8, 4)
        org = p.get_origin()
        assert org == (8, 4)
        for xy, origin, _ in b.steps:
            p.MapRep.set_scan(hs_mod.ScanCloud(xy, (origin[0], origin[1], 0.0)))
            k = C.c_int32()
            capi.call("slamhip_hsproc_scans_add", p._h, C.byref(k))
        poses_window = np.array([s[2] for s in b.steps], np.float32)
        world = poses_window.copy()
        world[:, 0] += np.float32(8.0); world[:, 1] += np.float32(4.0)    # (integers: the subtraction gives the window poses back exactly)
        with pytest.raises(capi.SlamhipError) as e:                       # a range past the store: refused before a pose is read
            capi.call("slamhip_hsproc_render", p._h, 0, len(b.steps) + 1, capi._vp(world[:1].copy()), 0)
        assert e.value.code == capi.ERR_INVALID
        p.RenderKeyframes(world)
        assert p.get_origin() == org
        loop(hs_mod, ref, b)
        same_maps(p.MapRep, ref, "after a shift", hook(capi, b))
    finally:
        p.Dispose(); ref.close()


def test_backing_tiles_are_dropped(hs_mod, ctx, capi):
    """A render with backing tiles present: the directory is empty afterwards and backing_stats says so; the setting stays; a tile
    drawn at the old poses does not scroll back in -- shifting back brings Reset cells."""
    b = rc.CASES["six_scans_l2"]()
    a, ref = make(hs_mod, ctx, b), make(hs_mod, ctx, b)
    try:
        a.set_backing(16, 1 << 22)
        poses = store(hs_mod, a, b)
        loop(hs_mod, a, b)                                                # the map at the "old poses"
        a.shift(32, 16)                                                   # 32 columns and 16 rows scroll out into tiles
        st = a.backing_stats()
        assert st["on"] == 1 and st["tiles"] > 0 and st["evicted_cells"] > 0
        a.Render(poses)
        st2 = a.backing_stats()
        assert st2["tiles"] == 0 and st2["on"] == 1 and st2["tile"] == 16 and st2["capacity_bytes"] == st["capacity_bytes"]
        assert st2["bytes"] == st["bytes"]                                # (the pool stays, as slamhip_hs_reset leaves it: the tiles go)
        assert a.origin() == (32, 16)                                     # (the window's origin is not the map)
        loop(hs_mod, ref, b)
        same_maps(a, ref, "render over backing", hook(capi, b))
        a.shift(-32, -16)
        assert a.backing_stats()["restored_cells"] == st["restored_cells"]    # (nothing came back)
        for l, (w, h) in enumerate(kc.level_dims(b.size, b.levels)):
            c = a.Maps[l].GetCells().reshape(h, w)
            dx, dy = 32 >> l, 16 >> l
            assert (c["update_index"][:dy, :] == -1).all() and (bits(c["value"][:dy, :]) == 0).all(), l
            assert (c["update_index"][:, :dx] == -1).all() and (bits(c["value"][:, :dx]) == 0).all(), l
            want = kc.shifted(ref.Maps[l].GetCells(), w, h, -dx, -dy)
            same_cells(c.reshape(-1), want, ("shifted back", l))
    finally:
        a.close(); ref.close()


def test_end_to_end_lap(hs_mod, ctx, capi):
    """The lap of tests/test_gpu_hector_pg.py: the simulator's field, a keyframe every metre, a heading bias of 0.2 degrees per
    step, one loop edge; every keyframe added with keep_scan=True.  Three renders -- at the true poses, at the drifted poses, and
    after RelaxKeyframes at the relaxed poses the store then holds (RenderKeyframes' default) -- each == the hook's; the level-0
    set of cells with value > 0 differs from the true render's in fewer cells for the relaxed poses than for the drifted ones.
    An ordering, not a threshold (checked on the CPU first: tests/test_hs_render_abi.py; the counts: DESIGN.md section 4 "K20")."""
    L = rc.lap()
    N = len(L["scans"])
    proc = hs_mod.HectorSLAMProcessor(rc.LAP_CELL, rc.LAP_SIZE, (0.0, 0.0, 0.0), rc.LAP_LEVELS, ctx=ctx)
    try:
        rep = proc.MapRep
        rep.SigConfigure(*rc.LAP_SIG)
        for i in range(N):
            k, _, _ = proc.AddKeyframe(hs_mod.ScanCloud(L["scans"][i], (0.0, 0.0, 0.0)), L["true"][i], keep_scan=True)
            assert k == i
        assert rep.ScansCount() == rep.SigCount() == N
        cells = {}

        def render(name, poses_expected):
            proc.RenderKeyframes()                                        # the poses of the signature store
            got = [rep.Maps[l].GetCells() for l in range(rc.LAP_LEVELS)]
            want = rc.lap_hook_render(capi, L, poses_expected)
            for l in range(rc.LAP_LEVELS):
                same_cells(got[l], want[l], (name, l))
            cells[name] = got[0]
        render("true", L["true"])
        rep.SigSetPoses(L["drifted"])
        render("drifted", L["drifted"])
        spec = capi.pg_spec(5, 4 * N, tol=1e-8)
        out, _, _ = proc.RelaxKeyframes([L["loop"]], rc.LAP_ODOM_W, spec)
        p0, ij, z, w = rc.lap_graph(capi, L["drifted"], L["loop"])
        assert np.array_equal(out, capi.debug_pg_relax(p0, None, ij, z, w, spec)[0])
        render("relaxed", out.astype(np.float32))
        d_drift, d_relax = rc.sym_diff(cells["drifted"], cells["true"]), rc.sym_diff(cells["relaxed"], cells["true"])
        print("symmetric difference to the true render: drifted %d, relaxed %d" % (d_drift, d_relax))
        assert d_relax < d_drift
    finally:
        proc.Dispose()


def _chunk_group():
    return "six_scans_l2 or two_scans_l2 or counts or across_mid_0 or sub_ranges or middle_range or test_store"


def test_other_tile_and_chunks():
    """The cases again in fresh interpreters: with the other tile side, and with a launch boundary after every 1, 2 and 4 scans
    (SLAMHIP_K20_CHUNK), and with a pool of 64 points at first (SLAMHIP_K20_POOL_POINTS), so that test_store's add / info / download
    round trip runs across several reallocations of the pool."""
    here = os.path.abspath(__file__)
    runs = [({"SLAMHIP_K20_TILE": "64"}, "not other_tile")]
    runs += [({"SLAMHIP_K20_CHUNK": c, "SLAMHIP_K20_POOL_POINTS": "64"}, "(%s) and not other_tile" % _chunk_group()) for c in ("1", "2", "4")]
    for extra, select in runs:
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "pytest", here, "-m", "gpu", "-x", "-q", "-k", select],
                           env=dict(os.environ, **extra), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        out = r.stdout.decode(errors="replace")
        assert r.returncode == 0 and " passed" in out and "failed" not in out, (extra, out[-3000:])
