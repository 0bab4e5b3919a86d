"""The frontier clusters (slamhip_hs_frontiers, slamhip_hsproc_frontiers) on the device, against the NumPy restatement of the
definition in tests/test_hs_frontier_abi.py (four shifted comparisons, a Python flood fill, np.lexsort), fed from cells_download /
world_cells_download.  Everything is compared with == on integers; there is no tolerance anywhere.

Shapes are the smallest at which each path can go wrong: the 80 x 48 x 2 pyramid whose rows are 2.5 and 1.25 frontier words, a
528 x 144 level that spans two workgroups across and nine down in every launch, a window whose level-1 origin is odd over tiles of 16
cells, and the 528 x 512 level that holds more isolated clusters than the record block has slots."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import test_gpu_hector_lattice as L
import test_gpu_hector_shift as S
import test_gpu_hector_trace as TR
import test_hs_dfield_abi as D
import test_hs_frontier_abi as FR
from test_gpu_hector_shift import hs_mod, ctx                              # noqa: F401 (fixtures)

gpu = pytest.mark.gpu
F = np.float32
POOL = 64 << 20
_SRC = open(os.path.join(FR.ROOT, "slam.net_amd", "csrc", "hs_frontier.hip")).read()
WG_WORDS = int(re.search(r"#define K10_WG_WORDS (\d+)", _SRC).group(1))    # frontier words of one row a workgroup owns
WG_ROWS = int(re.search(r"#define K10_WG_ROWS (\d+)", _SRC).group(1))
BX, BY = 32 * WG_WORDS, WG_ROWS                                            # the first column / row of the second workgroup
SEAM_W, SEAM_H = 528, 144


def window_classes(rep, level):
    w, h = rep.Maps[level].Dimensions
    return D.np_class_bits(rep.Maps[level].GetCells()["value"].reshape(h, w))


def put_classes(hs_mod, rep, level, cls):
    """Class bits -> values: 1 positive, 2 negative, 0 zero."""
    L.put_values(hs_mod, rep, level, np.select([cls.ravel() == 1, cls.ravel() == 2], [F(1.5), F(-0.75)], F(0.0)).astype(np.float32))


def np_labels_rect(lab, m, rect):
    """The label array of M = m = (mx0, my0, mw, mh) cut to rect = (x, y, w, h), -1 outside M."""
    x, y, w, h = rect
    out = np.full((h, w), -1, np.int32)
    x0, x1 = max(x, m[0]), min(x + w, m[0] + m[2]); y0, y1 = max(y, m[1]), min(y + h, m[1] + m[3])
    if x0 < x1 and y0 < y1:
        out[y0 - y:y1 - y, x0 - x:x1 - x] = lab[y0 - m[1]:y1 - m[1], x0 - m[0]:x1 - m[0]]
    return out


def assert_frontiers(rep, level, cls, m, min_cells, max_clusters, world, grow=3, want=None, tag=None):
    """One call with the label rectangle M grown by `grow` cells against the restatement over cls (the classes of M); the call
    without labels returns the same summary and records.  -> the call's result."""
    want = want or FR.np_frontiers(cls, min_cells, max_clusters, m[0], m[1])
    rect = (m[0] - grow, m[1] - grow, m[2] + 2 * grow, m[3] + 2 * grow)
    got = rep.frontiers(level, min_cells, max_clusters, world=world, labels_rect=rect)
    FR.check(got, (want[0], want[1], np_labels_rect(want[2], m, rect)), tag)
    if grow:
        assert (got[2][:grow] == -1).all() and (got[2][:, -grow:] == -1).all()
    FR.check(rep.frontiers(level, min_cells, max_clusters, world=world), want[:2], tag)
    return got


# ---- 1. small pyramid, all classes -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(hs_mod, ctx):
    """80 x 48 cells of 0.1 m, 2 levels, values drawn from {positive, negative, +0, -0, NaN}; the classes as cells_download gives them."""
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


@gpu
@pytest.mark.parametrize("max_clusters", [0, 3, FR.MAX_CLUSTERS])
@pytest.mark.parametrize("min_cells", [1, 2, 5])
def test_small_pyramid(small, min_cells, max_clusters):
    rep, cls = small
    for level in (0, 1):
        h, w = cls[level].shape
        got = assert_frontiers(rep, level, cls[level], (0, 0, w, h), min_cells, max_clusters, False, tag=(level, min_cells, max_clusters))
        assert got[0]["n_clusters"] > 10 and got[0]["n_returned"] == min(got[0]["n_kept"], max_clusters)


# ---- 2. workgroup seams ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seam_rep(hs_mod, ctx):
    assert BX < SEAM_W - 4 and SEAM_H > 7 * BY + 2
    rep = hs_mod.MapRepMultiMap(0.1, (SEAM_W, SEAM_H), 1, ctx=ctx)
    yield rep
    rep.close()


@gpu
@pytest.mark.parametrize("dy", [-2, -1, 0])
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_run_seams_on_workgroup_boundaries(hs_mod, seam_rep, kind, dy):
    """The three seam cases on the corner where four workgroups meet -- column BX, row BY -- and one cell either side of it in x (three
    placements on three row boundaries of one map) and in y (dy: the pair's rows lie before, across and after the row boundary)."""
    c = np.zeros((SEAM_H, SEAM_W), np.uint8)
    expect = []
    for i, dx in enumerate((-1, 0, 1)):
        y = (1 + 3 * i) * BY + dy                                          # rows y, y + 1; dy = -1: across the boundary
        name, one, clusters, runs = FR.seam_cases(SEAM_W, SEAM_H, BX + dx, y)[kind]
        c |= one
        expect.append((clusters, runs))
    put_classes(hs_mod, seam_rep, 0, c)
    assert np.array_equal(window_classes(seam_rep, 0), c)
    got = assert_frontiers(seam_rep, 0, c, (0, 0, SEAM_W, SEAM_H), 1, 256, False, tag=(kind, dy))
    assert got[0]["n_clusters"] == sum(e[0] for e in expect) and got[0]["n_runs"] == sum(e[1] for e in expect)


@gpu
@pytest.mark.parametrize("name", ["serpentine", "serpentine across", "comb"])
def test_long_chains_across_workgroups(hs_mod, seam_rep, name):
    """One cluster over the whole 528 x 144 level: the serpentine's parent chains run through every workgroup, the comb's 264 teeth
    are united only by the last row."""
    c = {"serpentine": lambda: FR.serpentine(SEAM_W, SEAM_H), "serpentine across": lambda: FR.serpentine(SEAM_H, SEAM_W).T.copy(),
         "comb": lambda: FR.comb(SEAM_W, SEAM_H)}[name]()
    put_classes(hs_mod, seam_rep, 0, c)
    got = assert_frontiers(seam_rep, 0, c, (0, 0, SEAM_W, SEAM_H), 1, 256, False, tag=name)
    s, r = got[0], got[1]
    assert s["n_clusters"] == 1 == s["n_kept"] and r[0]["n_cells"] == int((c == 2).sum()) == s["n_frontier_cells"]
    assert (r[0]["seed_x"], r[0]["seed_y"], r[0]["x_max"], r[0]["y_max"]) == (0, 0, SEAM_W - 1, SEAM_H - 1)
    if name == "comb":
        assert s["n_runs"] == (SEAM_W // 2) * (SEAM_H - 1) + 1
    inner = got[2][3:-3, 3:-3]
    assert (inner[c == 2] == 0).all() and (inner[c != 2] == -1).all()


# ---- 3. the world ------------------------------------------------------------------------------------------------------------------
def free_fill(hs_mod, rep, rng):
    """Mostly free, some occupied, some unknown, on every level."""
    for l, m in enumerate(rep.Maps):
        w, h = m.Dimensions
        put_classes(hs_mod, rep, l, rng.choice(np.array([0, 1, 2], np.uint8), size=(h, w), p=[0.08, 0.07, 0.85]))


def world_classes(rep, level, m):
    """The classes of M = m (window-frame cells) as world_cells_download gives them."""
    ox, oy = rep.origin()
    return D.np_class_bits(rep.world_cells(level, m[0] + (ox >> level), m[1] + (oy >> level), m[2], m[3])["value"])


def assert_world(rep, level, min_cells=1, max_clusters=FR.MAX_CLUSTERS):
    s = rep.frontiers(level, min_cells, max_clusters, world=True)[0]
    m = (int(s["mx0"]), int(s["my0"]), int(s["mw"]), int(s["mh"]))
    W, H = rep.Maps[level].Dimensions
    assert m[0] <= 0 and m[1] <= 0 and m[0] + m[2] >= W and m[1] + m[3] >= H           # R holds the window
    got = assert_frontiers(rep, level, world_classes(rep, level, m), m, min_cells, max_clusters, True, tag=("world", level))
    return m, got


@gpu
@pytest.mark.parametrize("level", [0, 1])
def test_world_variant(hs_mod, ctx, level):
    rng = np.random.default_rng(17)
    rep = hs_mod.MapRepMultiMap(0.1, (80, 48), 2, ctx=ctx)
    rep.set_backing(16, POOL)
    free_fill(hs_mod, rep, rng)
    rep.shift(34, -22)
    free_fill(hs_mod, rep, rng)
    rep.shift(-68, 30)                                                     # part of what was mapped now lies in tiles alone
    ox, oy = rep.origin()
    assert (ox, oy) == (-34, 8) and (ox >> 1) % 2 == 1 and rep.backing_stats()["tiles"] > 3
    W, H = rep.Maps[level].Dimensions
    m, got = assert_world(rep, level)
    assert m[2] * m[3] > W * H and (m[0] < 0 or m[1] < 0)
    r = got[1]
    spans = ((r["x_min"] < 0) & (r["x_max"] >= 0)) | ((r["x_min"] < W) & (r["x_max"] >= W)) | ((r["y_min"] < 0) & (r["y_max"] >= 0)) | \
        ((r["y_min"] < H) & (r["y_max"] >= H))
    assert spans.any()                                                     # clusters span the window's edge
    # R plays no part in the records: the same world over a larger rectangle (holes between the tiles, nothing around them)
    big = TR.WORLD_RECTS[level]
    assert big[0] < m[0] and big[1] < m[1] and big[0] + big[2] > m[0] + m[2] and big[1] + big[3] > m[1] + m[3]
    cls_big = world_classes(rep, level, big)
    assert (cls_big == 0).sum() > 0.3 * cls_big.size
    want_big = FR.np_frontiers(cls_big, 1, FR.MAX_CLUSTERS, big[0], big[1])
    assert np.array_equal(got[1], want_big[1])
    for f in ("n_frontier_cells", "n_runs", "n_clusters", "n_kept", "kept_cells"):
        assert got[0][f] == want_big[0][f], f
    assert_world(rep, level, 4, 5)
    # the window's own call sees its border as the end of the world
    win = assert_frontiers(rep, level, window_classes(rep, level), (0, 0, W, H), 1, FR.MAX_CLUSTERS, False, tag=("window", level))
    assert win[0]["n_frontier_cells"] != got[0]["n_frontier_cells"]
    rep.close()


@gpu
def test_world_is_the_window_without_tiles(hs_mod, small):
    rep, cls = small
    for level in (0, 1):
        h, w = cls[level].shape
        rect = (-5, -4, w + 9, h + 11)
        a = rep.frontiers(level, 2, 40, world=False, labels_rect=rect)
        b = rep.frontiers(level, 2, 40, world=True, labels_rect=rect)
        FR.check(a, b)
        assert tuple(a[0])[:4] == (0, 0, w, h) and a[0]["n_kept"] > 0


@gpu
def test_after_shift(hs_mod, ctx):
    rng = np.random.default_rng(5)
    rep = hs_mod.MapRepMultiMap(0.1, (80, 48), 2, ctx=ctx)
    rep.set_backing(16, POOL)
    free_fill(hs_mod, rep, rng)
    rep.shift(34, -22)
    free_fill(hs_mod, rep, rng)
    before = [assert_world(rep, l) for l in (0, 1)]
    rep.shift(-20, 14)
    for l in (0, 1):
        W, H = rep.Maps[l].Dimensions
        win = assert_frontiers(rep, l, window_classes(rep, l), (0, 0, W, H), 1, FR.MAX_CLUSTERS, False, tag=("window after shift", l))
        assert tuple(win[0])[:4] == (0, 0, W, H)                           # the window's M stays where it is
        m, got = assert_world(rep, l)
        m0, got0 = before[l]
        assert (m[0], m[1]) != (m0[0], m0[1])                              # ... and the world's moves with R
        assert got[0]["n_frontier_cells"] > 0
    rep.close()


# ---- 4. the processor --------------------------------------------------------------------------------------------------------------
@gpu
def test_processor_frontiers_after_a_scroll(hs_mod, sim):
    own = hs_mod.Context(0)
    proc = hs_mod.HectorSLAMProcessor(0.1, (64, 64), (3.0, 3.0, 0.0), 3, ctx=own, scrollTrigger=6)
    for i in range(8):
        true = np.array([3.0 + 0.18 * i, 3.0 + 0.05 * i, 0.04 * i], np.float32)
        proc.Update(hs_mod.ScanCloud(TR.room_scan(sim, true, 120)), true)
    ox, oy = proc.get_origin()
    assert (ox, oy) != (0, 0)                                              # the window has scrolled
    match, last = proc.MatchPose.copy(), proc.LastMapUpdatePose.copy()
    cell0 = F(proc.MapRep.Maps[0].CellLength)
    for level in (0, 1, 2):
        W, H = proc.MapRep.Maps[level].Dimensions
        kx, ky = ox >> level, oy >> level
        rect_w = (kx - 2, ky - 1, W + 5, H + 3)                            # world cells
        s, r, cen, lab = proc.Frontiers(level, min_cells=2, max_clusters=50, labels_rect=rect_w)
        ws, wr, wl = proc.MapRep.frontiers(level, 2, 50, labels_rect=(-2, -1, W + 5, H + 3))
        want = FR.np_frontiers(window_classes(proc.MapRep, level), 2, 50)
        FR.check((ws, wr), want[:2], level)
        assert s["n_kept"] >= 1 and np.array_equal(lab, wl)
        assert (s["mx0"], s["my0"]) == (kx, ky) and tuple(s)[2:] == tuple(ws)[2:]
        for f, k in (("seed_x", kx), ("x_min", kx), ("x_max", kx), ("seed_y", ky), ("y_min", ky), ("y_max", ky)):
            assert np.array_equal(r[f], wr[f] + k), f
        n = wr["n_cells"].astype(np.int64)
        assert np.array_equal(r["n_cells"], wr["n_cells"]) and np.array_equal(r["n_runs"], wr["n_runs"])
        assert np.array_equal(r["sum_x"], wr["sum_x"] + n * kx) and np.array_equal(r["sum_y"], wr["sum_y"] + n * ky)
        cell = float(F(proc.MapRep.Maps[level].CellLength))
        wx = want[1]["sum_x"] / n * cell + float(F(ox) * cell0); wy = want[1]["sum_y"] / n * cell + float(F(oy) * cell0)
        assert cen.shape == (r.shape[0], 2) and np.array_equal(cen[:, 0], wx) and np.array_equal(cen[:, 1], wy)
    assert S.same_bits(proc.MatchPose, match) and S.same_bits(proc.LastMapUpdatePose, last) and proc.get_origin() == (ox, oy)
    proc.Dispose(); own.close()


# ---- 5. the cap --------------------------------------------------------------------------------------------------------------------
@gpu
def test_more_clusters_than_slots(hs_mod, ctx):
    """A free cell at every (even x, even y) of 528 x 512: 264 * 256 = 67 584 isolated one-cell clusters, no two of them 8-adjacent."""
    capi = hs_mod.capi
    w, h = 528, 512
    c = np.zeros((h, w), np.uint8)
    c[0::2, 0::2] = 2
    rep = hs_mod.MapRepMultiMap(0.1, (w, h), 1, ctx=ctx)
    put_classes(hs_mod, rep, 0, c)
    s = np.zeros(1, FR.SUMMARY); rec = np.zeros(4, FR.CLUSTER)
    rc = capi.lib().slamhip_hs_frontiers(rep._h, 0, 0, 1, 4, s.ctypes.data_as(C.c_void_p), rec.ctypes.data_as(C.c_void_p), 0, 0, 0, 0, None)
    msg = capi.lib().slamhip_last_error().decode()
    assert rc == capi.ERR_INVALID and "67584" in msg and "min_cells" in msg
    assert tuple(s[0]) == (0, 0, w, h, 67584, 67584, 67584, 67584, 0, 67584) and not rec["n_cells"].any()
    got = rep.frontiers(0, 2, 16, labels_rect=(0, 0, w, h))
    assert tuple(got[0]) == (0, 0, w, h, 67584, 67584, 67584, 0, 0, 0) and got[1].shape == (0,)
    flat = np.arange(w * h, dtype=np.int32).reshape(h, w)
    assert np.array_equal(got[2], np.where(c == 2, flat, -1))              # every free cell is its own label
    c[300, 527] = 2                                                        # a 2 x 1 pair in place of the cell (526, 300): the last column touches no other
    put_classes(hs_mod, rep, 0, c)
    got = rep.frontiers(0, 2, 16)
    assert tuple(got[0]) == (0, 0, w, h, 67585, 67584, 67584, 1, 1, 2)
    assert tuple(got[1][0]) == (526, 300, 2, 1, 526, 300, 527, 300, 1053, 600)
    rep.close()


# ---- 6. refusals, and no side effects ----------------------------------------------------------------------------------------------
@gpu
def test_refusals(hs_mod, ctx):
    capi = hs_mod.capi
    lib = capi.lib()
    rng = np.random.default_rng(3)

    def call(rep, level=0, world=0, min_cells=1, max_clusters=4, clusters=True, lw=4, lh=4, labels=True):
        s = np.full(1, 77, FR.SUMMARY); rec = np.zeros(4, FR.CLUSTER); rec["n_cells"] = 77
        lab = np.full(16, 77, np.int32)
        rc = lib.slamhip_hs_frontiers(rep._h, level, world, min_cells, max_clusters, s.ctypes.data_as(C.c_void_p),
                                      rec.ctypes.data_as(C.c_void_p) if clusters else None, 0, 0, lw, lh,
                                      lab.ctypes.data_as(C.c_void_p) if labels else None)
        assert rc != 0 and (s["mw"] == 77).all() and (rec["n_cells"] == 77).all() and (lab == 77).all()
        return rc

    rep = hs_mod.MapRepMultiMap(0.1, (80, 48), 2, ctx=ctx)
    rep.set_backing(8, POOL)
    TR.fill(hs_mod, rep, rng)
    rep.shift(34, -22)
    TR.fill(hs_mod, rep, rng)
    ok0 = rep.frontiers(1, 2, 30, world=True, labels_rect=(-30, -30, 100, 90))
    for kw in (dict(level=-1), dict(level=2), dict(world=2), dict(world=-1), dict(min_cells=0), dict(min_cells=-1), dict(max_clusters=-1),
               dict(max_clusters=FR.MAX_CLUSTERS + 1), dict(clusters=False), dict(lw=0), dict(lh=0), dict(lw=-1), dict(lw=4097, lh=4096)):
        assert call(rep, **kw) == capi.ERR_INVALID, kw
        FR.check(rep.frontiers(1, 2, 30, world=True, labels_rect=(-30, -30, 100, 90)), ok0, kw)   # a second call on the same hs
    s, r = rep.frontiers(0, 1, 0)                                          # no records asked for: none needed
    assert s["n_returned"] == 0 and s["n_kept"] > 0 and r.shape == (0,)
    assert rep.frontiers(0, 1, 4, labels_rect=(0, 0, 4096, 4096))[2].shape == (4096, 4096)   # 2^24 labels go through
    # M too large: one non-Reset cell 9000 cells away on both axes -- R fits the class map's 2^28 and not the labelling's 2^25
    far = np.zeros((1, 1), capi.CELL_DTYPE)
    far["update_index"] = 1; far["value"] = 1.0
    assert rep.world_put(0, 9000, 9000, far) == 0
    ck = [rep.Maps[l].checksum() for l in range(2)]
    assert call(rep, world=1) == capi.ERR_INVALID and "2^25" in lib.slamhip_last_error().decode() and " x " in lib.slamhip_last_error().decode()
    assert [rep.Maps[l].checksum() for l in range(2)] == ck
    FR.check(rep.frontiers(1, 2, 30, world=True, labels_rect=(-30, -30, 100, 90)), ok0)   # level 1 holds no far tile
    assert rep.frontiers(0, 1, 4)[0]["mw"] == 80                           # the window's call does not care
    rep.close()


@gpu
def test_nothing_else_moved(hs_mod, ctx):
    rng = np.random.default_rng(4)
    rep = hs_mod.MapRepMultiMap(0.1, (80, 48), 2, ctx=ctx)
    rep.set_backing(16, POOL)
    TR.fill(hs_mod, rep, rng)
    rep.shift(34, -22)
    TR.fill(hs_mod, rep, rng)
    rep.set_scan(hs_mod.ScanCloud(L.small_points(np.random.default_rng(11), 97)))
    lat = (1, (1.0, 1.0, 0.0), 2, 2, 3, 0.1)

    def state():
        k, v = rep.world_lattice_search(None, *lat, scores=True)
        return ([rep.Maps[l].checksum() for l in range(2)], rep.distance_field(1, (-3, -3, 50, 40), site_mask=3, radius=9, world=True), k, v,
                [rep.Maps[l].GetCells().copy() for l in range(2)])
    a = state()
    first = [rep.frontiers(l, 1, 64, world=bool(wd), labels_rect=(-8, -8, 100, 70)) for l in (0, 1) for wd in (0, 1)]
    b = state()
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    assert all(S.raw(x).tobytes() == S.raw(y).tobytes() for x, y in zip(a[4], b[4]))
    again = [rep.frontiers(l, 1, 64, world=bool(wd), labels_rect=(-8, -8, 100, 70)) for l in (0, 1) for wd in (0, 1)]
    for x, y in zip(first, again):
        FR.check(x, y)                                                     # ... and the call repeats itself
    rep.set_reference_cache(1)                                             # cell values only: the reference's cache plays no part
    for x, y in zip(first, [rep.frontiers(l, 1, 64, world=bool(wd), labels_rect=(-8, -8, 100, 70)) for l in (0, 1) for wd in (0, 1)]):
        FR.check(x, y)
    rep.close()


@gpu
def test_poisoned_context_refuses(hs_mod):
    """A context poisoned by a blocking wait that timed out (the trace of tests/test_gpu_hector_trace.py: 1 ms against 4096 poses x
    1024 long beams) refuses the call at once with SLAMHIP_ERR_TIMEOUT, nothing launched."""
    import time
    capi = hs_mod.capi
    own = hs_mod.Context(0)
    rep = hs_mod.MapRepMultiMap(0.05, (1024, 1024), 1, ctx=own)
    try:
        a = np.linspace(-math.pi, math.pi, 1024, endpoint=False)
        rep.set_scan(hs_mod.ScanCloud(np.stack([25.0 * np.cos(a), 25.0 * np.sin(a)], 1).astype(np.float32)))
        poses = np.tile(np.array([25.6, 25.6, 0.0], np.float32), (4096, 1))
        rep.trace(poses[:2], 0)
        assert rep.frontiers(0)[0]["n_frontier_cells"] == 0                # nothing mapped yet
        own.set_wait_timeout(1)
        with pytest.raises(capi.SlamhipError) as e:
            rep.trace(poses, 0)
        assert e.value.code == capi.ERR_TIMEOUT and own.poisoned
        t0 = time.perf_counter()
        with pytest.raises(capi.SlamhipError) as e1:
            rep.frontiers(0)
        assert e1.value.code == capi.ERR_TIMEOUT and time.perf_counter() - t0 < 0.05
    finally:
        rep.close(); own.close()                                           # (destroy waits for the queue to drain: no bound there)
