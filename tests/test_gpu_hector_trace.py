"""The beam trace (slamhip_hs_trace, slamhip_hsproc_trace: what the map holds ALONG every beam of a scan, at many poses) on the
device, against the NumPy restatement of its definition in tests/test_hs_trace_abi.py, fed from cells_download /
world_cells_download.  Beam records and summaries are compared with == on integers; there is no tolerance anywhere.

Shapes are the smallest at which each path can go wrong: 64 x 64 x 3 and 80 x 48 x 2 pyramids whose rows are 2.5 and 5 packed
words, beam counts on both sides of the 256-beam chunk, a 1024 x 1024 level whose rectangle no workgroup can stage, a window
whose level-1 origin is odd over tiles of 16 cells."""
import ctypes as C
import math

import numpy as np
import pytest

import test_gpu_hector_lattice as L
import test_gpu_hector_shift as S
import test_hs_trace_abi as T
from test_gpu_hector_shift import hs_mod, ctx                              # noqa: F401 (fixtures)

gpu = pytest.mark.gpu
F = np.float32
POOL = 64 << 20
CHUNK = 256                                                                # beams per workgroup (K8_LANES)
RECT_WORDS = 12288                                                         # K7_RECT_WORDS


def stm_of(rep, level):
    return F(1.0) / F(rep.Maps[level].CellLength)


def window_values(rep, level):
    w, h = rep.Maps[level].Dimensions
    return rep.Maps[level].GetCells()["value"].reshape(h, w), 0, 0


def world_values(rep, level, rect):
    ox, oy = rep.origin()
    x0, y0, w, h = rect
    return rep.world_cells(level, x0, y0, w, h)["value"], x0 - (ox >> level), y0 - (oy >> level)


def assert_trace_equals(rep, scan, poses, level, src, world, tag, origin=(0.0, 0.0)):
    """Beam records and summaries of one trace against the restatement over src = (values, ax0, ay0); the trace without the records
    returns the same summaries.  -> (beams, summaries)."""
    poses = np.asarray(poses, np.float32).reshape(-1, 3)
    sums, beams = rep.trace(poses, level, world=world, beams=True, scan=scan)
    assert beams.shape == (poses.shape[0], scan.Points.shape[0]) and sums.shape == (poses.shape[0],)
    for b, pose in enumerate(poses):
        wb, ws = T.np_trace(src[0], src[1], src[2], stm_of(rep, level), pose, origin, scan.Points)
        bad = np.flatnonzero(beams[b] != wb)
        assert bad.size == 0, (tag, b, bad[:6].tolist(), beams[b][bad[:3]].tolist(), wb[bad[:3]].tolist())
        assert sums[b] == ws, (tag, b, sums[b], ws)
    sums2, none = rep.trace(poses, level, world=world)
    assert none is None and np.array_equal(sums2, sums), tag
    return beams, sums


# ---- 1. records and summaries on a mapped room -------------------------------------------------------------------------------------
ROOM = np.array([(1.0, 0.9, 5.3, 0.9), (5.3, 0.9, 5.3, 5.5), (5.3, 5.5, 1.0, 5.5), (1.0, 5.5, 1.0, 0.9),
                 (2.6, 2.4, 3.4, 2.4), (3.4, 2.4, 3.4, 3.1)], np.float64)   # four walls and an L-shaped obstacle, metres
ROOM_POSES = [(2.0, 1.8, 0.3), (4.4, 1.9, 1.4), (4.2, 4.4, 2.9), (1.9, 4.6, -1.2), (2.1, 3.1, 0.0), (3.0, 1.6, 0.7)]


def room_scan(sim, pose, n=90):
    return sim.make_scan(ROOM, np.asarray(pose, np.float32), n, sim.PCG32(int(pose[0] * 100)))[1]


@pytest.fixture(scope="module")
def room(hs_mod, ctx, sim):
    rep = hs_mod.MapRepMultiMap(0.1, (64, 64), 3, ctx=ctx)
    for p in ROOM_POSES:
        rep.UpdateByScan(hs_mod.ScanCloud(room_scan(sim, p)), np.asarray(p, np.float32))
    yield rep
    rep.close()


@gpu
@pytest.mark.parametrize("level", [0, 1, 2])
def test_room_records_and_summaries(hs_mod, sim, room, level):
    rep = room
    truth = np.array([3.9, 3.6, 0.5], np.float32)
    xy = room_scan(sim, truth)
    assert xy.shape[0] >= 85
    far = np.array([[4000.0 * math.cos(a), 4000.0 * math.sin(a)] for a in (0.1, 1.3, 2.9, -2.0, -0.4)], np.float32)
    scan = hs_mod.ScanCloud(np.concatenate([xy, far]))                     # 40000 cells of level 0, 20000 of level 1
    poses = np.array([truth, (3.5, 3.9, 0.9), (20.0, -7.0, 0.2), (np.nan, 3.0, 0.0), (2.2, 4.9, -2.1)], np.float32)
    beams, sums = assert_trace_equals(rep, scan, poses, level, window_values(rep, level), False, ("room", level))
    n = scan.Points.shape[0]
    # the far beams are ignored on level 0 alone; the NaN pose ignores everything; the room's beams from outside the map meet nothing
    assert (beams[0]["da"][-5:] == -1).all() == (level == 0) and sums[3]["n_ignored"] == n
    assert (beams[2]["first"][:-5] == -1).all() and (beams[2]["da"][:-5] >= 1).sum() > 80
    # the true pose: most beams meet an obstacle, and where the scan saw one; the other poses run into walls early
    met = sums["n_end_hit"] + sums["n_blocked"]
    assert met[0] > 70 and sums[0]["n_end_hit"] > sums[1]["n_end_hit"] and sums[0]["n_end_hit"] > sums[4]["n_end_hit"]
    assert (sums["n_walked"] + sums["n_same"] + sums["n_ignored"] == n).all()


# ---- 2. beam counts across the chunk boundary --------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n_points", [1, 63, CHUNK, CHUNK + 1, 2 * CHUNK + 1])
@pytest.mark.parametrize("B", [1, 3])
def test_beam_counts(hs_mod, L_small, n_points, B):
    rep, _ = L_small
    rng = np.random.default_rng(100 + n_points)
    xy = np.stack([rng.uniform(-6.0, 6.0, n_points), rng.uniform(-4.0, 4.0, n_points)], 1).astype(np.float32)
    if n_points > 60:
        xy[7] = (np.nan, 1.0); xy[-1] = (0.01, 0.0)                        # an ignored beam, and a same-cell beam in the last chunk
    poses = np.array([(3.1, 2.2, 0.4), (7.7, 0.3, 2.0), (0.2, 4.5, -1.0)][:B], np.float32)
    for level in (0, 1):
        beams, sums = assert_trace_equals(rep, hs_mod.ScanCloud(xy), poses, level, window_values(rep, level), False, (n_points, B, level))
        assert (sums["n_walked"] + sums["n_same"] + sums["n_ignored"] == n_points).all()
    if n_points > 60:
        assert sums[0]["n_blocked"] > 0 and sums[0]["n_ignored"] == 1 and sums[0]["n_same"] >= 1


@pytest.fixture(scope="module")
def L_small(hs_mod, ctx):
    """80 x 48 cells of 0.1 m, 2 levels, every class of value on both levels (test_gpu_hector_lattice's `small`)."""
    rng = np.random.default_rng(7)
    rep = hs_mod.MapRepMultiMap(0.1, (80, 48), 2, ctx=ctx)
    values = [L.class_values(rng, 80 * 48), L.class_values(rng, 40 * 24)]
    for l in range(2):
        L.put_values(hs_mod, rep, l, values[l])
    yield rep, values
    rep.close()


# ---- 3. both staging paths ---------------------------------------------------------------------------------------------------------
def np_chunk_words(lines, w, h):
    """The fit rule of k8_trace, per chunk of CHUNK beams: the words of the bounding box of the walked lines' ends, clipped to
    the w x h map, in whole 16-cell words; 0 for a chunk that stages nothing."""
    out = []
    for c in range(0, lines.shape[0], CHUNK):
        l = lines[c:c + CHUNK]
        l = l[l[:, 4] >= 1]
        if not l.shape[0]:
            out.append(0); continue
        x_lo, x_hi = max(min(l[:, 0].min(), l[:, 2].min()), 0), min(max(l[:, 0].max(), l[:, 2].max()), w - 1)
        y_lo, y_hi = max(min(l[:, 1].min(), l[:, 3].min()), 0), min(max(l[:, 1].max(), l[:, 3].max()), h - 1)
        out.append(((x_hi >> 4) - (x_lo >> 4) + 1) * (y_hi - y_lo + 1) if x_lo <= x_hi and y_lo <= y_hi else 0)
    return out


@gpu
def test_staged_rectangle(hs_mod, L_small):
    rep, _ = L_small
    rng = np.random.default_rng(31)
    xy = np.stack([rng.uniform(-9.0, 9.0, 300), rng.uniform(-6.0, 6.0, 300)], 1).astype(np.float32)   # beams leave the map on every side
    pose = np.array([4.1, 2.3, 0.8], np.float32)
    words = np_chunk_words(T.np_lines(stm_of(rep, 0), pose, (0.0, 0.0), xy), 80, 48)
    assert len(words) == 2 and all(0 < v <= RECT_WORDS for v in words) and max(words) == 5 * 48      # the whole map, staged
    assert_trace_equals(rep, hs_mod.ScanCloud(xy), [pose], 0, window_values(rep, 0), False, "lds")


@gpu
def test_global_memory_path(hs_mod, ctx):
    rng = np.random.default_rng(23)
    rep = hs_mod.MapRepMultiMap(0.05, (1024, 1024), 1, ctx=ctx)
    pick = rng.integers(0, 400, 1024 * 1024)                               # sparse obstacles: beams run long before they meet one, if at all
    v = np.select([pick == 0, pick < 40, pick == 40], [F(1.5), F(-0.7), F(np.nan)], F(0.0)).astype(np.float32)
    L.put_values(hs_mod, rep, 0, v)
    ang = rng.uniform(-math.pi, math.pi, 300); r = rng.uniform(18.0, 24.0, 300)
    r[::17] = 31.0                                                         # some end outside the map
    xy = np.stack([r * np.cos(ang), r * np.sin(ang)], 1).astype(np.float32)
    poses = np.array([(25.6, 25.6, 0.3), (24.0, 27.0, -1.1)], np.float32)
    for p in poses:
        words = np_chunk_words(T.np_lines(stm_of(rep, 0), p, (0.0, 0.0), xy), 1024, 1024)
        assert len(words) == 2 and min(words) > 3 * RECT_WORDS, words
    beams, sums = assert_trace_equals(rep, hs_mod.ScanCloud(xy), poses, 0, window_values(rep, 0), False, "global")
    assert beams["first"].max() > 100 and (beams["first"] == -1).sum() > 0 and sums[0]["unknown_cells"] > 1000
    rep.close()


# ---- 4. the world variant ----------------------------------------------------------------------------------------------------------
WORLD_RECTS = [(-128, -96, 352, 256), (-64, -48, 176, 128)]                # every window position below, grown by more than a tile


def fill(hs_mod, rep, rng):
    for l, m in enumerate(rep.Maps):
        w, h = m.Dimensions
        L.put_values(hs_mod, rep, l, L.class_values(rng, w * h))


@gpu
@pytest.mark.parametrize("level", [0, 1])
def test_world_variant(hs_mod, ctx, level):
    rng = np.random.default_rng(7)
    rep = hs_mod.MapRepMultiMap(0.1, (80, 48), 2, ctx=ctx)
    rep.set_backing(16, POOL)
    fill(hs_mod, rep, rng)
    rep.shift(34, -22)
    fill(hs_mod, rep, rng)
    rep.shift(-68, 30)                                                     # part of what was mapped now lies in tiles alone
    ox, oy = rep.origin()
    assert (ox, oy) == (-34, 8) and (ox >> 1) % 2 == 1 and rep.backing_stats()["tiles"] > 3
    e = rep.world_extends(level)
    x0, y0, w, h = WORLD_RECTS[level]
    assert x0 <= e[2] and e[0] < x0 + w and y0 <= e[3] and e[1] < y0 + h and rep.backing_stats()["dropped_cells"] == 0
    xy = np.stack([rng.uniform(-9.0, 9.0, 280), rng.uniform(-7.0, 7.0, 280)], 1).astype(np.float32)
    xy[3] = (np.nan, 0.5)
    scan = hs_mod.ScanCloud(xy)
    poses = np.array([(4.0, 2.4, 0.3), (7.9, 0.1, -2.0), (-2.5, 6.0, 1.0)], np.float32)   # the last one stands outside the window
    lines = T.np_lines(stm_of(rep, level), poses[0], (0.0, 0.0), xy)
    W, H = rep.Maps[level].Dimensions
    outside = (lines[:, 4] >= 1) & ((lines[:, 2] < 0) | (lines[:, 2] >= W) | (lines[:, 3] < 0) | (lines[:, 3] >= H))
    assert outside.sum() > 40
    wb, ws = assert_trace_equals(rep, scan, poses, level, world_values(rep, level, WORLD_RECTS[level]), True, ("world", level))
    nb, ns = assert_trace_equals(rep, scan, poses, level, window_values(rep, level), False, ("window", level))
    assert (nb[0]["end_class"][outside] == 0).all() and (wb[0]["end_class"][outside] != 0).sum() > 3
    assert (wb[:2] != nb[:2]).any(axis=1).all() and (ws[:2] != ns[:2]).all()  # (nothing was ever mapped around the third pose)
    rep.close()


@gpu
def test_world_variant_from_global_memory(hs_mod, ctx):
    """The world's class map read from global memory (k8_walk<false> with R's origin not (0, 0)): test_world_variant's world with one
    more tile 1500 x 900 cells away on level 0, and beams up to 100 m long.  R contains the window and every cell that is not Reset,
    so the fit rule evaluated over that smaller rectangle E is a lower bound of the kernel's (a bounding box clipped to R contains the
    one clipped to E; whole words of R's rows may add or drop one word per row): it is asserted at twice the budget."""
    rng = np.random.default_rng(13)
    rep = hs_mod.MapRepMultiMap(0.1, (80, 48), 2, ctx=ctx)
    rep.set_backing(16, POOL)
    fill(hs_mod, rep, rng)
    rep.shift(34, -22)
    fill(hs_mod, rep, rng)
    rep.shift(-68, 30)
    far = np.zeros((16, 16), hs_mod.capi.CELL_DTYPE)
    far["update_index"] = 1; far["value"] = L.class_values(rng, 256).reshape(16, 16)
    assert rep.world_put(0, 1504, 896, far) == 0
    ox, oy = rep.origin()
    e = rep.world_extends(0)                                               # (xmax, ymax, xmin, ymin), world cells
    ex0, ey0 = min(e[2], ox), min(e[3], oy)
    rect = (ex0, ey0, max(e[0], ox + 79) - ex0 + 1, max(e[1], oy + 47) - ey0 + 1)
    assert rect[2] > 1500 and rect[3] > 900 and (ex0, ey0) != (ox, oy)     # (the map's first cell is not the window's)
    n = 512
    xy = np.stack([rng.uniform(-9.0, 9.0, n), rng.uniform(-7.0, 7.0, n)], 1).astype(np.float32)
    xy[::2] = np.stack([rng.uniform(-100.0, 160.0, n // 2), rng.uniform(-60.0, 100.0, n // 2)], 1).astype(np.float32)
    xy[5] = (np.nan, 0.5)
    xy[6] = (150.6, 87.2)                                                  # from cell (40, 24) into the far tile's middle, window-frame cell (1546, 896)
    scan = hs_mod.ScanCloud(xy)
    poses = np.array([(4.0, 2.4, 0.0), (7.9, 0.1, -2.0)], np.float32)
    src = world_values(rep, 0, rect)
    for p in poses:
        ln = T.np_lines(stm_of(rep, 0), p, (0.0, 0.0), xy)
        ln[:, [0, 2]] -= src[1]; ln[:, [1, 3]] -= src[2]                   # into E's cells
        words = np_chunk_words(ln, rect[2], rect[3])
        assert len(words) == 2 and min(words) > 2 * RECT_WORDS, words
    wb, ws = assert_trace_equals(rep, scan, poses, 0, src, True, "world, global")
    nb, ns = assert_trace_equals(rep, scan, poses, 0, window_values(rep, 0), False, "window beside it")
    assert (wb != nb).any(axis=1).all() and wb[0]["da"][6] == 1506 and nb[0]["end_class"][6] == 0
    rep.close()


@gpu
def test_world_is_the_window_without_backing(hs_mod, L_small):
    rep, _ = L_small
    rng = np.random.default_rng(41)
    scan = hs_mod.ScanCloud(np.stack([rng.uniform(-9.0, 9.0, 300), rng.uniform(-7.0, 7.0, 300)], 1).astype(np.float32))
    poses = np.array([(4.0, 2.4, 0.3), (7.9, 0.1, -2.0)], np.float32)
    for level in (0, 1):
        s0, b0 = rep.trace(poses, level, world=False, beams=True, scan=scan)
        s1, b1 = rep.trace(poses, level, world=True, beams=True)
        assert np.array_equal(b0, b1) and np.array_equal(s0, s1) and s0["n_blocked"].min() > 0


# ---- 5. the inverse of the update --------------------------------------------------------------------------------------------------
@gpu
def test_inverse_of_the_update(hs_mod, ctx, sim):
    rep = hs_mod.MapRepMultiMap(0.1, (64, 64), 3, ctx=ctx)
    P = np.array([3.9, 3.6, 0.5], np.float32)
    scan = hs_mod.ScanCloud(room_scan(sim, P, 180))
    rep.UpdateByScan(scan, P)
    for level in range(3):
        sums, beams = rep.trace([P], level, beams=True)
        w, h = rep.Maps[level].Dimensions
        ln = T.np_lines(stm_of(rep, level), P, (0.0, 0.0), scan.Points)
        inside = (ln[:, 4] >= 1) & (ln[:, 0] >= 0) & (ln[:, 0] < w) & (ln[:, 1] >= 0) & (ln[:, 1] < h) & \
                 (ln[:, 2] >= 0) & (ln[:, 2] < w) & (ln[:, 3] >= 0) & (ln[:, 3] < h)
        assert inside.sum() > 150 and np.array_equal(beams[0]["da"], ln[:, 4])
        b = beams[0][inside]
        assert (b["first"] >= 0).all() and (b["end_class"] == 1).all()     # every end cell the update drew is occupied
        assert sums[0]["n_end_hit"] + sums[0]["n_blocked"] == inside.sum() == sums[0]["n_walked"]
        assert (b["n_unknown"] == 0).all()                                 # ... and every cell in front of it was drawn
    rep.close()


# ---- 6. stream order and no side effects -------------------------------------------------------------------------------------------
@gpu
def test_stream_order_and_no_side_effects(hs_mod, ctx, sim):
    rep = hs_mod.MapRepMultiMap(0.1, (64, 64), 3, ctx=ctx)
    for p in ROOM_POSES[:-1]:
        rep.UpdateByScan(hs_mod.ScanCloud(room_scan(sim, p)), np.asarray(p, np.float32))
    p = np.asarray(ROOM_POSES[-1], np.float32)
    scan = hs_mod.ScanCloud(room_scan(sim, p))
    q = np.array([p[0] + F(0.2), p[1] - F(0.1), p[2] + F(0.1)], np.float32)
    before = [window_values(rep, l)[0].copy() for l in range(3)]
    rep.UpdateByScan(scan, p)                                              # enqueue-only; the traces go right behind it
    got = [rep.trace([p, q], l, beams=True) for l in range(3)]
    sums_ck = [rep.Maps[l].checksum() for l in range(3)]
    for l in range(3):
        src = window_values(rep, l)
        assert not np.array_equal(src[0], before[l])
        for b, pose in enumerate((p, q)):
            wb, ws = T.np_trace(src[0], 0, 0, stm_of(rep, l), pose, (0.0, 0.0), scan.Points)
            assert np.array_equal(got[l][1][b], wb) and got[l][0][b] == ws, (l, b)
    lat = (1, p, 3, 2, 5, F(0.15))
    k0, v0 = rep.lattice_search(scan, *lat, scores=True)
    rep.trace([p, q], 1, beams=True)
    rep.trace([p, q], 2, world=True)
    k1, v1 = rep.lattice_search(None, *lat, scores=True)
    assert np.array_equal(k0, k1) and np.array_equal(v0, v1)
    assert [rep.Maps[l].checksum() for l in range(3)] == sums_ck
    rep.close()


# ---- 7. the processor ----------------------------------------------------------------------------------------------------------------
@gpu
def test_processor_trace_after_a_scroll(hs_mod, sim):
    def run(with_trace):
        own = hs_mod.Context(0)
        proc = hs_mod.HectorSLAMProcessor(0.1, (64, 64), (3.0, 3.0, 0.0), 3, ctx=own, scrollTrigger=6)
        out = []
        for i in range(10):
            true = np.array([3.0 + 0.18 * i, 3.0 + 0.05 * i, 0.04 * i], np.float32)
            proc.Update(hs_mod.ScanCloud(room_scan(sim, true, 120)), true)
            out.append(proc.MatchPose.copy())
            if with_trace and i == 7:
                assert proc.get_origin() != (0, 0)                         # the window has scrolled
                scan = hs_mod.ScanCloud(room_scan(sim, true, 77))
                pw = np.array([out[-1], (3.3, 3.9, 1.0)], np.float32)
                sums, beams = proc.Trace(scan, pw, 1, beams=True)
                ox, oy = proc.get_origin()
                cell0 = F(proc.MapRep.Maps[0].CellLength)
                pl = pw.copy()
                pl[:, 0] = pw[:, 0] - F(ox) * cell0; pl[:, 1] = pw[:, 1] - F(oy) * cell0
                s2, b2 = proc.MapRep.trace(pl, 1, beams=True)              # the scan the processor's call set
                assert np.array_equal(beams, b2) and np.array_equal(sums, s2)
                src = window_values(proc.MapRep, 1)
                wb, ws = T.np_trace(src[0], 0, 0, stm_of(proc.MapRep, 1), pl[0], (0.0, 0.0), scan.Points)
                assert np.array_equal(beams[0], wb) and sums[0] == ws and sums[0]["n_walked"] > 60
                sw, bw = proc.Trace(scan, pw, 1, world=True, beams=True)
                assert bw.shape == beams.shape
        last = proc.LastMapUpdatePose.copy()
        proc.Dispose(); own.close()
        return out, last

    a, la = run(False)
    b, lb = run(True)
    assert all(S.same_bits(x, y) for x, y in zip(a, b)) and S.same_bits(la, lb)


@gpu
def test_expected_scan_in_a_drawn_room(hs_mod, ctx):
    """One-cell-thick walls at x = 10 and 52, y = 8 and 50 of a 64 x 64 level of 0.1 m; the sensor in cell (30, 30).  East 22 cells,
    west 20, north 20, south 22.  The diagonals walk (30 +- a, 30 +- a): north-east meets the wall y = 50 at a = 20, north-west the
    corner (10, 50) at a = 20, south-west the wall x = 10 at a = 20, south-east the corner (52, 8) at a = 22."""
    rep = hs_mod.MapRepMultiMap(0.1, (64, 64), 2, ctx=ctx)
    v = np.zeros((64, 64), np.float32)
    v[8:51, 10] = 1.0; v[8:51, 52] = 1.0; v[8, 10:53] = 1.0; v[50, 10:53] = 1.0
    L.put_values(hs_mod, rep, 0, v.ravel())
    ang = [0.0, math.pi / 2, math.pi, -math.pi / 2, math.pi / 4, 3 * math.pi / 4, -3 * math.pi / 4, -math.pi / 4]
    cell = float(F(0.1))
    got = rep.ExpectedScan((3.0, 3.0, 0.0), ang, 10.0, 0)
    want = [22 * cell, 20 * cell, 20 * cell, 22 * cell] + [float(np.hypot(float(k), float(k))) * cell for k in (20, 20, 20, 22)]
    assert got.tolist() == want
    assert np.isinf(rep.ExpectedScan((3.0, 3.0, 0.0), ang, 1.5, 0)).all()   # the beams end before any wall
    assert np.isinf(rep.ExpectedScan((3.0, 3.0, 0.0), ang, 10.0, 1)).all()  # level 1 holds nothing
    rep.close()


# ---- 8. errors -----------------------------------------------------------------------------------------------------------------------
@gpu
def test_refusals(hs_mod, ctx):
    capi = hs_mod.capi
    lib = capi.lib()
    rng = np.random.default_rng(3)
    pts = L.small_points(np.random.default_rng(11), 97)

    def attempt(rep, level, B, world, with_beams=False, n=97):
        poses = np.zeros((max(B, 1), 3), np.float32); poses[:, :2] = 2.0
        sums = np.zeros(max(B, 1), capi.TRACE_SUMMARY); sums["n_walked"] = 7
        mark = sums.copy()
        beams = np.zeros(max(B, 1) * n if with_beams else 1, capi.TRACE_BEAM)
        rc = lib.slamhip_hs_trace(rep._h, level, capi.fptr(poses), B, world, sums.ctypes.data_as(C.c_void_p),
                                  beams.ctypes.data_as(C.c_void_p) if with_beams else None)
        assert rc != 0 and np.array_equal(sums, mark) and not beams["da"].any()
        return rc

    def state(rep):
        return rep.origin(), rep.backing_stats(), [S.raw(rep.Maps[l].GetCells()).copy() for l in range(2)]

    def same(s0, s1):
        return s0[0] == s1[0] and s0[1] == s1[1] and all(np.array_equal(x, y) for x, y in zip(s0[2], s1[2]))

    rep = hs_mod.MapRepMultiMap(0.1, (80, 48), 2, ctx=ctx)
    rep.set_backing(8, POOL)
    assert attempt(rep, 0, 1, 0) == capi.ERR_STATE                         # no scan
    fill(hs_mod, rep, rng)
    rep.shift(34, -22)
    fill(hs_mod, rep, rng)
    rep.set_scan(hs_mod.ScanCloud(pts))
    lat = (1, (1.0, 1.0, 0.0), 2, 2, 3, 0.1)
    k0, v0 = rep.world_lattice_search(None, *lat, scores=True)
    s0 = state(rep)
    for level, B, world in ((-1, 1, 0), (2, 1, 0), (0, 0, 0), (0, 65537, 1), (0, 1, 2), (0, 1, -1)):
        assert attempt(rep, level, B, world) == capi.ERR_INVALID, (level, B, world)
    assert attempt(rep, 0, 10811, 0, with_beams=True) == capi.ERR_INVALID   # 10811 x 97 = 2^20 + 91 records
    assert same(s0, state(rep))
    ok_s, ok_b = rep.trace(np.zeros((10810, 3), np.float32), 0, beams=True)  # 10810 x 97 <= 2^20 goes through
    assert ok_b.shape == (10810, 97) and (ok_s == ok_s[0]).all()
    # R too large: one non-Reset cell 3e6 cells away on both axes
    far = np.zeros((1, 1), capi.CELL_DTYPE)
    far["update_index"] = 1; far["value"] = 1.0
    assert rep.world_put(0, 3000000, 3000000, far) == 0
    s1 = state(rep)
    assert attempt(rep, 0, 1, 1) == capi.ERR_INVALID and "2^28" in lib.slamhip_last_error().decode()
    assert same(s1, state(rep)) and s1[1]["tiles"] == s0[1]["tiles"] + 1
    rep.trace(np.zeros((1, 3), np.float32), 0, world=False)                 # the window's trace does not care
    rep.trace(np.zeros((1, 3), np.float32), 1, world=True)                  # level 1 holds no far tile
    k1, v1 = rep.world_lattice_search(None, *lat, scores=True)
    assert np.array_equal(k0, k1) and np.array_equal(v0, v1)                 # the keys are what they were
    rep.close()


@gpu
def test_poisoned_context_refuses(hs_mod):
    """A trace that outlasts the context's bound (1 ms against 4096 poses x 1024 beams of 500 unknown cells each) returns
    SLAMHIP_ERR_TIMEOUT and poisons the context; the next trace is refused at once with the same code, nothing launched."""
    import time
    capi = hs_mod.capi
    own = hs_mod.Context(0)
    rep = hs_mod.MapRepMultiMap(0.05, (1024, 1024), 1, ctx=own)
    try:
        a = np.linspace(-math.pi, math.pi, 1024, endpoint=False)
        rep.set_scan(hs_mod.ScanCloud(np.stack([25.0 * np.cos(a), 25.0 * np.sin(a)], 1).astype(np.float32)))
        poses = np.tile(np.array([25.6, 25.6, 0.0], np.float32), (4096, 1))
        rep.trace(poses[:2], 0)                                            # (allocations and the first launch outside the bound)
        own.set_wait_timeout(1)
        with pytest.raises(capi.SlamhipError) as e:
            rep.trace(poses, 0)
        assert e.value.code == capi.ERR_TIMEOUT and own.poisoned
        t0 = time.perf_counter()
        with pytest.raises(capi.SlamhipError) as e2:
            rep.trace(poses[:1], 0)
        assert e2.value.code == capi.ERR_TIMEOUT and time.perf_counter() - t0 < 0.05
    finally:
        rep.close(); own.close()                                           # (destroy waits for the queue to drain: no bound there)
