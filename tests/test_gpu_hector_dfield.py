"""The distance field and the end-point distance score (slamhip_hs_distance_field, slamhip_hs_distance_score,
slamhip_hsproc_distance_score) on the device, against the NumPy restatements of the definition in tests/test_hs_dfield_abi.py
(np_field, proved equal to the brute force there; the closed form of lone sites), fed from cells_download / world_cells_download.
Everything is compared with == on integers; there is no tolerance anywhere.

Shapes are the smallest at which each path can go wrong: the 80 x 48 x 2 pyramid whose rows are 5 and 2.5 packed words, a 528 x 144
level that spans two k9_rows segments and several k9_cols tiles each way, a window whose level-1 origin is odd over tiles of 16
cells, point counts on both sides of the 256-point chunk."""
import ctypes as C
import math

import numpy as np
import pytest

import test_gpu_hector_lattice as L
import test_gpu_hector_shift as S
import test_gpu_hector_trace as TR
import test_hs_dfield_abi as D
import test_hs_trace_abi as T
from test_gpu_hector_shift import hs_mod, ctx                              # noqa: F401 (fixtures)
from test_gpu_hector_trace import room                                     # noqa: F401 (fixture)

gpu = pytest.mark.gpu
F = np.float32
POOL = 64 << 20
# the kernels' tile constants (hs_dfield.hip)
SEG = 512                                                                  # K9_SEG: cells of one row a k9_rows workgroup owns
TX, TY = 64, 128                                                           # K9_TX, K9_TY: columns x rows of a k9_cols tile
CHUNK = 256                                                                # K9S_LANES: points per k9_score workgroup
LIMIT = F(16777216.0)


def window_classes(rep, level):
    w, h = rep.Maps[level].Dimensions
    return D.np_class_bits(rep.Maps[level].GetCells()["value"].reshape(h, w))


def grown(w, h, r, margin=2):
    """E of a w x h map, and `margin` cells more on every side."""
    return (-r - margin, -r - margin, w + 2 * (r + margin), h + 2 * (r + margin))


def np_end_cells(stm, pose, xy):
    """The end cells of the definition's step 5 -> (ex, ey, counted)."""
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    t = T.np_transform(stm, pose)
    if t is None:
        z = np.zeros(xy.shape[0], np.int64)
        return z, z, np.zeros(xy.shape[0], bool)
    with np.errstate(over="ignore", invalid="ignore"):
        exf, eyf = t.transform(xy[:, 0], xy[:, 1])
        assert exf.dtype == np.float32
        ok = (np.abs(exf) < LIMIT) & (np.abs(eyf) < LIMIT)
        ex = np.where(ok, np.rint(exf), 0).astype(np.int64); ey = np.where(ok, np.rint(eyf), 0).astype(np.int64)
    return ex, ey, ok


def np_point_values(field, rect, const, stm, pose, xy):
    """F at the end cells: `field` covers rect (which contains E), the constant holds outside; 0xFFFF for an ignored point."""
    ex, ey, ok = np_end_cells(stm, pose, xy)
    x0, y0, w, h = rect
    inside = ok & (ex >= x0) & (ex < x0 + w) & (ey >= y0) & (ey < y0 + h)
    out = np.full(ex.shape[0], const, np.int64)
    out[inside] = field[ey[inside] - y0, ex[inside] - x0]
    out[~ok] = 0xFFFF
    return out.astype(np.uint16)


@pytest.fixture(scope="module")
def small(hs_mod, ctx):
    """80 x 48 cells of 0.1 m, 2 levels, every class of value on both levels; the classes as cells_download gives them."""
    rng = np.random.default_rng(7)
    rep = hs_mod.MapRepMultiMap(0.1, (80, 48), 2, ctx=ctx)
    for l, n in enumerate((80 * 48, 40 * 24)):
        L.put_values(hs_mod, rep, l, L.class_values(rng, n))
    cls = [window_classes(rep, l) for l in range(2)]
    for c in cls:
        assert set(np.unique(c).tolist()) == {0, 1, 2}
        c.setflags(write=False)
    yield rep, cls
    rep.close()


# ---- 1. small pyramid, all classes -------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("r", [1, 16, 17, 255])
@pytest.mark.parametrize("mask", [1, 2, 3, 4, 6])
def test_small_pyramid(small, mask, r):
    rep, cls = small
    for level in (0, 1):
        h, w = cls[level].shape
        rect = grown(w, h, r)
        got = rep.distance_field(level, rect, site_mask=mask, radius=r)
        want = D.np_field(cls[level], mask, r, rect)
        assert got.dtype == np.uint16 and got.shape == want.shape
        assert np.array_equal(got, want), (level, mask, r, np.argwhere(got != want)[:5].tolist())
        const = 0 if mask & 1 else r * r
        assert (got[:2] == const).all() and (got[:, -2:] == const).all()
        if not mask & 1:
            assert (got == 0).sum() == (((mask >> cls[level].astype(np.int64)) & 1) == 1).sum() > 0


# ---- 2. tile seams ---------------------------------------------------------------------------------------------------------------
SEAM_W, SEAM_H = 528, 144


@gpu
@pytest.mark.parametrize("r", [15, 255])
def test_tile_seams(hs_mod, ctx, r):
    """Lone occupied cells beside a segment boundary of k9_rows (E column SEG = map column SEG - r) and a tile boundary of k9_cols
    (E row k * TY = map row k * TY - r), on either side of it, with the cells exactly r - 1, r and r + 1 away across the boundary
    probed by name; the whole of E and a margin against the closed form."""
    assert SEAM_W + 2 * r > SEG and SEAM_W > 2 * TX and SEAM_H > TY
    bx = SEG - r                                                           # the first map column of the second segment
    by = min(k * TY - r for k in range(1, 6) if 0 < k * TY - r < SEAM_H - 1)   # a tile's first map row
    sites = {(bx - 1, 10): (1, 0), (300, by - 1): (0, 1), (bx, SEAM_H - 1): (-1, 0), (500, by): (0, -1)}   # site: the way across the boundary
    rep = hs_mod.MapRepMultiMap(0.1, (SEAM_W, SEAM_H), 1, ctx=ctx)
    rect = grown(SEAM_W, SEAM_H, r)
    for (sx, sy), (dx, dy) in sites.items():                               # each alone: at r = 255 no two sites of this level are out of each other's reach
        v = np.zeros((SEAM_H, SEAM_W), np.float32)
        v[sy, sx] = 1.0
        L.put_values(hs_mod, rep, 0, v.ravel())
        want = D.np_closed_form([(sx, sy)], r, rect)
        got = rep.distance_field(0, rect, site_mask=2, radius=r)
        for k in (r - 1, r, r + 1):
            x, y = sx + k * dx, sy + k * dy
            assert want[y - rect[1], x - rect[0]] == min(k * k, r * r) == got[y - rect[1], x - rect[0]], ((sx, sy), k)
        assert np.array_equal(got, want), (r, (sx, sy), np.argwhere(got != want)[:5].tolist())
    # the unknown and occupied cells together: 0 everywhere; the free cells: none, capped everywhere
    assert not rep.distance_field(0, rect, site_mask=3, radius=r).any()
    assert (rep.distance_field(0, (0, 0, SEAM_W, SEAM_H), site_mask=4, radius=r) == r * r).all()
    rep.close()


# ---- 3. the world ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("level", [0, 1])
def test_world_variant(hs_mod, ctx, level):
    rng = np.random.default_rng(7)
    rep = hs_mod.MapRepMultiMap(0.1, (80, 48), 2, ctx=ctx)
    rep.set_backing(16, POOL)
    TR.fill(hs_mod, rep, rng)
    rep.shift(34, -22)
    TR.fill(hs_mod, rep, rng)
    rep.shift(-68, 30)                                                     # part of what was mapped now lies in tiles alone
    ox, oy = rep.origin()
    assert (ox, oy) == (-34, 8) and (ox >> 1) % 2 == 1 and rep.backing_stats()["tiles"] > 3
    e = rep.world_extends(level)
    x0, y0, w, h = TR.WORLD_RECTS[level]                                   # holds every tile, and ground no tile holds around them
    assert x0 < e[2] and e[0] < x0 + w - 1 and y0 < e[3] and e[1] < y0 + h - 1 and rep.backing_stats()["dropped_cells"] == 0
    values, ax0, ay0 = TR.world_values(rep, level, TR.WORLD_RECTS[level])
    cls = D.np_class_bits(values)
    W, H = rep.Maps[level].Dimensions
    for mask, r in ((2, 5), (3, 20), (4, 33), (1, 7)):
        rel = grown(w, h, r, 3)                                            # in the source array's cells: the world's E lies inside
        want = D.np_field(cls, mask, r, rel)
        got = rep.distance_field(level, (rel[0] + ax0, rel[1] + ay0, rel[2], rel[3]), site_mask=mask, radius=r, world=True)
        assert np.array_equal(got, want), (level, mask, r, np.argwhere(got != want)[:5].tolist())
        win = rep.distance_field(level, (rel[0] + ax0, rel[1] + ay0, rel[2], rel[3]), site_mask=mask, radius=r)
        assert np.array_equal(win, D.np_field(window_classes(rep, level), mask, r, (rel[0] + ax0, rel[1] + ay0, rel[2], rel[3])))
        assert not np.array_equal(win, got)                                # the tiles outside the window count in the world alone
    rep.close()


@gpu
def test_world_is_the_window_without_backing(small):
    rep, cls = small
    for level in (0, 1):
        h, w = cls[level].shape
        for mask, r in ((2, 9), (1, 40)):
            rect = grown(w, h, r, 5)
            a = rep.distance_field(level, rect, site_mask=mask, radius=r, world=False)
            b = rep.distance_field(level, rect, site_mask=mask, radius=r, world=True)
            assert np.array_equal(a, b) and a.any()


# ---- 4. the score ------------------------------------------------------------------------------------------------------------------
SCORE_R, SCORE_MASK = 12, 2


@pytest.fixture(scope="module")
def small_fields(small):
    """The field call's values over E and a margin, per level: what the score's look-ups are compared with."""
    rep, cls = small
    out = []
    for level in (0, 1):
        h, w = cls[level].shape
        rect = grown(w, h, SCORE_R)
        f = rep.distance_field(level, rect, site_mask=SCORE_MASK, radius=SCORE_R)
        f.setflags(write=False)
        out.append((rect, f))
    return out


@gpu
@pytest.mark.parametrize("n_points", [1, 63, CHUNK, CHUNK + 1, 2 * CHUNK + 1])
@pytest.mark.parametrize("B", [1, 3])
def test_score(hs_mod, small, small_fields, n_points, B):
    rep, _ = small
    rng = np.random.default_rng(200 + n_points)
    xy = np.stack([rng.uniform(-6.0, 6.0, n_points), rng.uniform(-4.0, 4.0, n_points)], 1).astype(np.float32)
    if n_points > 60:
        xy[3] = (np.nan, 1.0)                                              # ignored on every level
        xy[5] = (4000.0, 0.0)                                              # 40000 cells of level 0: counted, far outside E -- the constant
        xy[7] = (2.0e6, 1.0)                                               # 2e7 cells of level 0 (>= 2^24: ignored), 1e7 of level 1 (counted)
        xy[-1] = (-4000.0, 2.0e6)
    poses = np.array([(3.1, 2.2, 0.4), (7.7, 0.3, 2.0), (np.nan, 4.5, -1.0)][:B], np.float32)
    scan = hs_mod.ScanCloud(xy)
    for level in (0, 1):
        rect, field = small_fields[level]
        stm = TR.stm_of(rep, level)
        sums, pts = rep.distance_score(poses, level, site_mask=SCORE_MASK, radius=SCORE_R, points=True, scan=scan)
        assert pts.shape == (B, n_points) and pts.dtype == np.uint16 and sums.shape == (B,)
        for b in range(B):
            want = np_point_values(field, rect, SCORE_R * SCORE_R, stm, poses[b], xy)
            assert np.array_equal(pts[b], want), (n_points, b, level, np.flatnonzero(pts[b] != want)[:6].tolist())
            assert sums[b] == D.np_summary(want, SCORE_R), (n_points, b, level, sums[b])
        assert (sums["n_counted"] + sums["n_ignored"] == n_points).all()
        sums2, none = rep.distance_score(poses, level, site_mask=SCORE_MASK, radius=SCORE_R)   # without the records
        assert none is None and np.array_equal(sums2, sums)
        if n_points > 60:
            assert sums[0]["n_ignored"] == (3 if level == 0 else 1) and sums[0]["n_capped"] >= 1 and sums[0]["n_zero"] > 0
            assert pts[0, 5] == SCORE_R * SCORE_R and pts[0, 3] == 0xFFFF and (pts[0, 7] == 0xFFFF) == (level == 0)
        if B == 3:
            assert sums[2]["n_ignored"] == n_points and sums[2]["sum_d2"] == 0 and (pts[2] == 0xFFFF).all()


# ---- 5. the processor --------------------------------------------------------------------------------------------------------------
@gpu
def test_processor_score_after_a_scroll(hs_mod, sim):
    own = hs_mod.Context(0)
    proc = hs_mod.HectorSLAMProcessor(0.1, (64, 64), (3.0, 3.0, 0.0), 3, ctx=own, scrollTrigger=6)
    for i in range(8):
        true = np.array([3.0 + 0.18 * i, 3.0 + 0.05 * i, 0.04 * i], np.float32)
        proc.Update(hs_mod.ScanCloud(TR.room_scan(sim, true, 120)), true)
    ox, oy = proc.get_origin()
    assert (ox, oy) != (0, 0)                                              # the window has scrolled
    match, last = proc.MatchPose.copy(), proc.LastMapUpdatePose.copy()
    scan = hs_mod.ScanCloud(TR.room_scan(sim, true, 77))
    pw = np.array([match, (3.3, 3.9, 1.0)], np.float32)
    sums, pts = proc.DistanceScore(scan, pw, 1, site_mask=2, radius=10, points=True)
    cell0 = F(proc.MapRep.Maps[0].CellLength)
    pl = pw.copy()
    pl[:, 0] = pw[:, 0] - F(ox) * cell0; pl[:, 1] = pw[:, 1] - F(oy) * cell0
    s2, p2 = proc.MapRep.distance_score(pl, 1, site_mask=2, radius=10, points=True)   # the scan the processor's call set
    assert np.array_equal(pts, p2) and np.array_equal(sums, s2) and sums[0]["n_counted"] > 60 and sums[0]["n_zero"] > 0
    sw, pw_pts = proc.DistanceScore(scan, pw, 1, site_mask=2, radius=10, world=True, points=True)
    assert pw_pts.shape == pts.shape and (sw["n_counted"] == sums["n_counted"]).all()
    assert S.same_bits(proc.MatchPose, match) and S.same_bits(proc.LastMapUpdatePose, last) and proc.get_origin() == (ox, oy)
    proc.Dispose(); own.close()


# ---- 6. refusals, and no side effects ----------------------------------------------------------------------------------------------
@gpu
def test_refusals(hs_mod, ctx):
    capi = hs_mod.capi
    lib = capi.lib()
    rng = np.random.default_rng(3)
    pts = L.small_points(np.random.default_rng(11), 97)

    def field(rep, level=0, world=0, mask=2, r=8, w=4, h=4):
        out = np.full(16, 77, np.uint16)
        rc = lib.slamhip_hs_distance_field(rep._h, level, world, mask, r, 0, 0, w, h, out.ctypes.data_as(C.c_void_p))
        assert rc != 0 and (out == 77).all()
        return rc

    def score(rep, level=0, world=0, mask=2, r=8, B=1, with_points=False):
        poses = np.zeros((max(B, 1), 3), np.float32); poses[:, :2] = 2.0
        sums = np.zeros(max(B, 1), capi.DISTANCE_SUMMARY); sums["n_counted"] = 7
        mark = sums.copy()
        rec = np.full(max(B, 1) * 97 if with_points else 1, 77, np.uint16)
        rc = lib.slamhip_hs_distance_score(rep._h, level, world, mask, r, capi.fptr(poses), B, sums.ctypes.data_as(C.c_void_p),
                                           rec.ctypes.data_as(C.c_void_p) if with_points else None)
        assert rc != 0 and np.array_equal(sums, mark) and (rec == 77).all()
        return rc

    rep = hs_mod.MapRepMultiMap(0.1, (80, 48), 2, ctx=ctx)
    rep.set_backing(8, POOL)
    assert score(rep) == capi.ERR_STATE                                    # no scan
    TR.fill(hs_mod, rep, rng)
    rep.shift(34, -22)
    TR.fill(hs_mod, rep, rng)
    rep.set_scan(hs_mod.ScanCloud(pts))
    lat = (1, (1.0, 1.0, 0.0), 2, 2, 3, 0.1)
    k0, v0 = rep.world_lattice_search(None, *lat, scores=True)
    ck = [rep.Maps[l].checksum() for l in range(2)]
    for kw in (dict(level=-1), dict(level=2), dict(world=2), dict(world=-1), dict(mask=0), dict(mask=8), dict(r=0), dict(r=256)):
        assert field(rep, **kw) == capi.ERR_INVALID, kw
        assert score(rep, **kw) == capi.ERR_INVALID, kw
    for w, h in ((0, 4), (4, 0), (-1, 4), (4097, 4096)):
        assert field(rep, w=w, h=h) == capi.ERR_INVALID, (w, h)
    for B in (0, -1, 65537):
        assert score(rep, B=B) == capi.ERR_INVALID, B
    assert score(rep, B=43241, with_points=True) == capi.ERR_INVALID       # 43241 x 97 = 2^22 + 73 records
    assert [rep.Maps[l].checksum() for l in range(2)] == ck
    ok_s, ok_p = rep.distance_score(np.zeros((43240, 3), np.float32), 0, points=True)   # 43240 x 97 <= 2^22 goes through
    assert ok_p.shape == (43240, 97) and (ok_s == ok_s[0]).all()
    f0 = rep.distance_field(1, (-3, -3, 50, 40), site_mask=3, radius=9, world=True)
    k1, v1 = rep.world_lattice_search(None, *lat, scores=True)
    assert np.array_equal(k0, k1) and np.array_equal(v0, v1)               # the keys are what they were
    assert [rep.Maps[l].checksum() for l in range(2)] == ck
    # E too large: one non-Reset cell 9000 cells away on both axes -- R fits the class map's 2^28, E = R + 2 r does not fit 2^26
    far = np.zeros((1, 1), capi.CELL_DTYPE)
    far["update_index"] = 1; far["value"] = 1.0
    assert rep.world_put(0, 9000, 9000, far) == 0
    ck = [rep.Maps[l].checksum() for l in range(2)]
    assert field(rep, world=1) == capi.ERR_INVALID and "2^26" in lib.slamhip_last_error().decode() and " x " in lib.slamhip_last_error().decode()
    assert score(rep, world=1) == capi.ERR_INVALID and "2^26" in lib.slamhip_last_error().decode()
    assert [rep.Maps[l].checksum() for l in range(2)] == ck
    assert np.array_equal(rep.distance_field(1, (-3, -3, 50, 40), site_mask=3, radius=9, world=True), f0)   # level 1 holds no far tile
    rep.distance_field(0, (0, 0, 8, 8), world=False)                       # the window's field does not care
    k2, v2 = rep.world_lattice_search(None, *lat, scores=True)
    assert np.array_equal(k0, k2) and np.array_equal(v0, v2)
    rep.close()


@gpu
def test_poisoned_context_refuses(hs_mod):
    """A context poisoned by a blocking wait that timed out (the trace of tests/test_gpu_hector_trace.py: 1 ms against 4096 poses x
    1024 long beams) refuses the field and the score at once with SLAMHIP_ERR_TIMEOUT, nothing launched."""
    import time
    capi = hs_mod.capi
    own = hs_mod.Context(0)
    rep = hs_mod.MapRepMultiMap(0.05, (1024, 1024), 1, ctx=own)
    try:
        a = np.linspace(-math.pi, math.pi, 1024, endpoint=False)
        rep.set_scan(hs_mod.ScanCloud(np.stack([25.0 * np.cos(a), 25.0 * np.sin(a)], 1).astype(np.float32)))
        poses = np.tile(np.array([25.6, 25.6, 0.0], np.float32), (4096, 1))
        rep.trace(poses[:2], 0)
        assert rep.distance_score(poses[:2], 0, radius=4)[0]["n_counted"].tolist() == [1024, 1024]
        own.set_wait_timeout(1)
        with pytest.raises(capi.SlamhipError) as e:
            rep.trace(poses, 0)
        assert e.value.code == capi.ERR_TIMEOUT and own.poisoned
        t0 = time.perf_counter()
        with pytest.raises(capi.SlamhipError) as e1:
            rep.distance_field(0, (0, 0, 4, 4))
        with pytest.raises(capi.SlamhipError) as e2:
            rep.distance_score(poses[:1], 0)
        assert e1.value.code == capi.ERR_TIMEOUT and e2.value.code == capi.ERR_TIMEOUT and time.perf_counter() - t0 < 0.05
    finally:
        rep.close(); own.close()                                           # (destroy waits for the queue to drain: no bound there)


# ---- 7. meaning --------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("level", [0, 1])
def test_meaning_on_the_mapped_room(hs_mod, sim, room, level):
    rep = room
    truth = np.array([3.9, 3.6, 0.5], np.float32)
    scan = hs_mod.ScanCloud(TR.room_scan(sim, truth))
    poses = np.array([truth, (3.5, 3.9, 0.9), (2.2, 4.9, -2.1), (4.3, 3.3, 0.2)], np.float32)
    r = 20
    sums, pts = rep.distance_score(poses, level, site_mask=2, radius=r, points=True, scan=scan)
    assert (sums["n_counted"] == scan.Points.shape[0]).all() and scan.Points.shape[0] >= 85
    mean = sums["sum_d2"].astype(np.float64) / sums["n_counted"]
    assert (mean[0] < mean[1:]).all(), mean.tolist()                       # the true pose lies closest to the mapped walls
    cls = window_classes(rep, level)
    h, w = cls.shape
    for b, pose in enumerate(poses):
        ex, ey, ok = np_end_cells(TR.stm_of(rep, level), pose, scan.Points)
        inside = ok & (ex >= 0) & (ex < w) & (ey >= 0) & (ey < h)
        occupied = int((cls[ey[inside], ex[inside]] == 1).sum())
        assert sums[b]["n_zero"] == occupied == int((pts[b] == 0).sum()), (level, b)
    assert sums[0]["n_zero"] > 0
