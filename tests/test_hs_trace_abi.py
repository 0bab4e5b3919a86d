"""CPU-side checks of the beam trace's interface (slamhip_hs_trace, slamhip_hsproc_trace, slamhip_debug_trace_lines,
slamhip_debug_trace_cells) and the NumPy restatement of its definition (include/slamhip.h, slamhip_trace_beam) that
tests/test_gpu_hector_trace.py compares the device with: np.float32 operations one at a time (np_oracle.M32 for the Matrix3x2
product), np.rint for the banker's rounding, the closed form (da // 2 + a * db) // da for the walk -- the library walks with
Bresenham2D's recurrence, so the comparison is of two formulations.  Everything is compared with ==.  No compute calls on a device."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import np_oracle as npo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("slamhip_hs_trace", "slamhip_hsproc_trace", "slamhip_debug_trace_lines", "slamhip_debug_trace_cells")
F = np.float32
LIMIT = F(16777216.0)
MAX_DA = 32768


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def np_transform(stm, pose):
    """t of step 1, or None for a pose that is not finite (every float it forms is then NaN or infinite: all beams are ignored)."""
    pose = np.asarray(pose, np.float32).reshape(3)
    if not np.isfinite(pose).all():
        return None
    with np.errstate(over="ignore", invalid="ignore"):
        return npo.M32.rotation(pose[2]) * npo.M32.translation(pose[0], pose[1]) * npo.M32.scale(F(stm))


def np_lines(stm, pose, origin, xy):
    """Steps 1 and 2 -> (n, 5) int64 {bx, by, ex, ey, da}; an ignored beam is (0, 0, 0, 0, -1)."""
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    out = np.zeros((xy.shape[0], 5), np.int64)
    out[:, 4] = -1
    t = np_transform(stm, pose)
    if t is None:
        return out
    with np.errstate(over="ignore", invalid="ignore"):
        bxf, byf = t.transform(F(origin[0]), F(origin[1]))
        exf, eyf = t.transform(xy[:, 0], xy[:, 1])
        assert exf.dtype == np.float32 and np.asarray(bxf).dtype == np.float32
        ok = (np.abs(exf) < LIMIT) & (np.abs(eyf) < LIMIT) & bool(np.abs(bxf) < LIMIT) & bool(np.abs(byf) < LIMIT)
        bx, by = (int(np.rint(bxf)), int(np.rint(byf))) if ok.any() else (0, 0)
        ex = np.where(ok, np.rint(exf), 0).astype(np.int64); ey = np.where(ok, np.rint(eyf), 0).astype(np.int64)
    da = np.maximum(np.abs(ex - bx), np.abs(ey - by))
    ok &= da <= MAX_DA
    out[ok, 0] = bx; out[ok, 1] = by; out[ok, 2] = ex[ok]; out[ok, 3] = ey[ok]; out[ok, 4] = da[ok]
    return out


def np_cells(bx, by, ex, ey):
    """Step 3 -> (da + 1, 2) int64, da >= 1: the closed form, the end cell last."""
    dx, dy = ex - bx, ey - by
    adx, ady = abs(dx), abs(dy)
    da, db = max(adx, ady), min(adx, ady)
    assert da >= 1
    a = np.arange(da + 1, dtype=np.int64)
    m = (da // 2 + a * db) // da
    sx, sy = (dx > 0) - (dx < 0), (dy > 0) - (dy < 0)
    if adx >= ady:
        out = np.stack([bx + sx * a, by + sy * m], 1)
    else:
        out = np.stack([bx + sx * m, by + sy * a], 1)
    out[da] = (ex, ey)
    return out


def np_class_bits(values):
    v = np.asarray(values, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(v > 0, 1, np.where(v < 0, 2, 0)).astype(np.int64)


BEAM = np.dtype([("da", np.int32), ("first", np.int32), ("n_unknown", np.int32), ("end_class", np.int32), ("hx", np.int32), ("hy", np.int32)])
SUMMARY = np.dtype([("n_walked", np.int32), ("n_same", np.int32), ("n_ignored", np.int32), ("n_end_hit", np.int32), ("n_blocked", np.int32),
                    ("n_end_free", np.int32), ("unknown_cells", np.int64)])


def np_trace(values, ax0, ay0, stm, pose, origin, xy):
    """Steps 4 and 5 for one pose over the (h, w) array `values` whose first element is window-frame cell (ax0, ay0); every cell
    outside it is class 0.  -> (beams (n,) of BEAM, summary of SUMMARY)."""
    cls = np_class_bits(values)
    h, w = cls.shape
    lines = np_lines(stm, pose, origin, xy)
    beams = np.zeros(lines.shape[0], BEAM)
    beams["first"] = -1
    beams["da"] = lines[:, 4]
    for i, (bx, by, ex, ey, da) in enumerate(lines.tolist()):
        if da < 1:
            continue
        c = np_cells(bx, by, ex, ey)
        x, y = c[:, 0] - ax0, c[:, 1] - ay0
        ok = (x >= 0) & (x < w) & (y >= 0) & (y < h)
        k = np.where(ok, cls[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)], 0)
        occ = np.flatnonzero(k == 1)
        first = int(occ[0]) if occ.size else -1
        stop = first if first >= 0 else da + 1
        beams[i] = (da, first, int((k[:stop] == 0).sum()), int(k[da]), c[first, 0] if first >= 0 else 0, c[first, 1] if first >= 0 else 0)
    s = np.zeros(1, SUMMARY)[0]
    d, f = beams["da"], beams["first"]
    s["n_walked"] = (d >= 1).sum(); s["n_same"] = (d == 0).sum(); s["n_ignored"] = (d < 0).sum()
    s["n_end_hit"] = ((d >= 1) & (f == d)).sum(); s["n_blocked"] = ((d >= 1) & (f >= 0) & (f < d)).sum()
    s["n_end_free"] = ((d >= 1) & (f == -1) & (beams["end_class"] == 2)).sum()
    s["unknown_cells"] = beams["n_unknown"].astype(np.int64).sum()
    return beams, s


# ---- the interface -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def capi():
    import slam.net_amd.build as b
    b.build()
    import slam.net_amd.capi as capi
    return capi


def test_surface(capi):
    h = open(os.path.join(ROOT, "include", "slamhip.h")).read()
    assert capi.TRACE_BEAM.itemsize == 24 and capi.TRACE_SUMMARY.itemsize == 32
    assert capi.TRACE_BEAM == BEAM and capi.TRACE_SUMMARY == SUMMARY
    assert capi.TRACE_SUMMARY.fields["unknown_cells"][1] == 24                # six int32, then the int64: no padding
    assert "#define SLAMHIP_TRACE_MAX_DA 32768" in h and capi.TRACE_MAX_DA == MAX_DA
    assert "SLAMHIP_K_COUNT = 10" in h                                        # no new timing class
    L = capi.lib()
    for name in SYMBOLS:
        assert hasattr(L, name) and name in L._signatures and name in capi.declared_symbols(), name
    assert len(L._signatures["slamhip_hs_trace"][1]) == 7 and len(L._signatures["slamhip_hsproc_trace"][1]) == 10
    import slam.net_amd.hector as hm
    assert hasattr(hm.MapRepMultiMap, "trace") and hasattr(hm.MapRepMultiMap, "ExpectedScan") and hasattr(hm.HectorSLAMProcessor, "Trace")


def test_hooks_refuse(capi):
    n = C.c_int32(7)
    L = capi.lib()
    out = np.zeros((8, 2), np.int32)
    assert L.slamhip_debug_trace_cells(0, 0, 0, 0, capi.iptr(out), 8, C.byref(n)) == capi.ERR_INVALID and n.value == 0    # da = 0
    assert L.slamhip_debug_trace_cells(0, 0, MAX_DA + 1, 0, None, 0, C.byref(n)) == capi.ERR_INVALID and n.value == 0
    assert L.slamhip_debug_trace_cells(1 << 24, 0, (1 << 24) + 1, 0, capi.iptr(out), 8, C.byref(n)) == capi.ERR_INVALID and n.value == 0
    assert L.slamhip_debug_trace_cells(0, 0, 8, 0, capi.iptr(out), 8, C.byref(n)) == capi.ERR_INVALID and n.value == 9    # no room
    assert not out.any()
    assert L.slamhip_debug_trace_cells(0, 0, 7, 0, capi.iptr(out), 8, C.byref(n)) == 0 and n.value == 8


# ---- the restatement against the hooks -----------------------------------------------------------------------------------------------
def assert_lines(capi, stm, pose, origin, xy, tag):
    got = capi.trace_lines(stm, pose, origin, xy)
    want = np_lines(stm, pose, origin, xy)
    assert np.array_equal(got, want), (tag, np.argwhere(got != want)[:6].tolist())
    return want


def test_lines_random(capi):
    rng = np.random.default_rng(5)
    counts = np.zeros(3, np.int64)
    for it in range(60):
        stm = F(1.0) / F([0.05, 0.1, 0.2, 0.4][it % 4])
        pose = np.array([rng.uniform(-20, 20), rng.uniform(-20, 20), rng.uniform(-7, 7)], np.float32)
        if it % 10 == 0:
            pose[2] = F([0.0, math.pi / 2, math.pi, -math.pi / 2, 3 * math.pi, 1e-6][(it // 10) % 6])     # Matrix3x2.CreateRotation's exact cases
        origin = (rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3)) if it % 3 else (0.0, 0.0)
        xy = rng.uniform(-30, 30, (200, 2)).astype(np.float32)
        xy[:5] = np.float32(origin)                                            # the same cell as the sensor
        w = assert_lines(capi, stm, pose, origin, xy, it)
        counts += [(w[:, 4] >= 1).sum(), (w[:, 4] == 0).sum(), (w[:, 4] < 0).sum()]
    assert counts[0] > 10000 and counts[1] >= 300 and counts[2] == 0


def test_lines_half_cells_round_to_even(capi):
    """Points at .5 cell fractions with the identity rotation and stm = 1: rintf, not floor(x + 0.5)."""
    xs = np.arange(-6, 7, dtype=np.float32) + F(0.5)
    xy = np.stack([xs, -xs], 1)
    w = assert_lines(capi, 1.0, (0.0, 0.0, 0.0), (0.5, 1.5), xy, "half")
    assert w[0, :2].tolist() == [0, 2]                                        # 0.5 -> 0, 1.5 -> 2
    assert w[:, 2].tolist() == [-6, -4, -4, -2, -2, 0, 0, 2, 2, 4, 4, 6, 6]
    assert w[:, 3].tolist() == [6, 4, 4, 2, 2, 0, 0, -2, -2, -4, -4, -6, -6]


def test_lines_ignored(capi):
    nan, inf = float("nan"), float("inf")
    xy = np.array([[1, 1], [nan, 0], [0, nan], [inf, 0], [0, -inf], [16777216.0, 0], [16777215.0, 0], [0, -16777216.0], [3, 4]], np.float32)
    w = assert_lines(capi, 1.0, (0.0, 0.0, 0.0), (0.0, 0.0), xy, "points")
    assert w[:, 4].tolist() == [1, -1, -1, -1, -1, -1, -1, -1, 4]             # (16777215 counts as a float and fails the cap on da)
    assert not w[1:8, :4].any()
    # |f| >= 2^24 next to the sensor: da is small, the float rule alone refuses
    w = assert_lines(capi, 1.0, (16777210.0, 0.0, 0.0), (0.0, 0.0), [[5.0, 0.0], [6.0, 0.0], [7.0, 1.0]], "far sensor")
    assert w[:, 4].tolist() == [5, -1, -1]
    # a sensor cell that does not count ignores every beam, and so does a pose that is no number
    for pose in [(16777216.0, 0.0, 0.0), (nan, 0.0, 0.0), (0.0, inf, 0.0), (0.0, 0.0, nan), (0.0, 0.0, inf)]:
        w = assert_lines(capi, 1.0, pose, (0.0, 0.0), [[1.0, 2.0], [0.0, 0.0]], pose)
        assert w[:, 4].tolist() == [-1, -1] and not w[:, :4].any()
    # the cap: da = 32768 is walked, 32769 is not -- on either axis, in either direction
    xy = [[32768, 0], [32769, 0], [-32768, 5], [-32769, 5], [7, 32768], [7, -32769], [32768, 32768], [32769, 32769]]
    w = assert_lines(capi, 1.0, (0.0, 0.0, 0.0), (0.0, 0.0), xy, "cap")
    assert w[:, 4].tolist() == [32768, -1, 32768, -1, 32768, -1, 32768, -1]


def test_cells_all_octants(capi):
    rng = np.random.default_rng(9)
    ends = [(dx, dy) for dx in range(-9, 10) for dy in range(-9, 10) if (dx, dy) != (0, 0)]          # every octant, the axes, |dx| == |dy|
    ends += [(int(a), int(b)) for a, b in rng.integers(-700, 700, (300, 2)) if (a, b) != (0, 0)]
    ends += [(MAX_DA, 0), (-MAX_DA, MAX_DA), (MAX_DA, 1), (-1, -MAX_DA), (MAX_DA, MAX_DA - 1), (-MAX_DA + 1, MAX_DA), (32767, -16385)]
    for dx, dy in ends:
        bx, by = int(rng.integers(-50, 50)), int(rng.integers(-50, 50))
        got = capi.trace_cells(bx, by, bx + dx, by + dy)
        want = np_cells(bx, by, bx + dx, by + dy)
        assert got.shape == want.shape and np.array_equal(got, want), (dx, dy)
    # at the edge of the cells that count
    top = (1 << 24) - 1
    assert np.array_equal(capi.trace_cells(top - 3, -top, top, -top + 2), np_cells(top - 3, -top, top, -top + 2))


def test_hand_kats(capi):
    """The working, with e(a) = da // 2 + a * db and minor offset e(a) // da:
    axis-aligned (4, 0): db = 0, every minor offset is 2 // 4 = 0 -> (0,0) (1,0) (2,0) (3,0) (4,0).
    45 degrees (3, 3): da = db = 3, e = 1 + 3 a -> 4 // 3 = 1, 7 // 3 = 2, then the end cell -> (0,0) (1,1) (2,2) (3,3).
    (5, 2): da = 5, db = 2, e = 2 + 2 a = 4, 6, 8, 10 -> 0, 1, 1, 2, then the end -> (0,0) (1,0) (2,1) (3,1) (4,2) (5,2).
    y-major (2, 5): the same offsets along x.  Negative signs mirror the offsets, not the rounding: e is formed from |dx|, |dy|."""
    def cells(bx, by, ex, ey):
        return [tuple(c) for c in capi.trace_cells(bx, by, ex, ey).tolist()]
    assert cells(0, 0, 4, 0) == [(0, 0), (1, 0), (2, 0), (3, 0), (4, 0)]
    assert cells(2, 7, 2, 4) == [(2, 7), (2, 6), (2, 5), (2, 4)]
    assert cells(0, 0, 3, 3) == [(0, 0), (1, 1), (2, 2), (3, 3)]
    assert cells(1, 1, -2, 4) == [(1, 1), (0, 2), (-1, 3), (-2, 4)]
    base = [(0, 0), (1, 0), (2, 1), (3, 1), (4, 2), (5, 2)]
    assert cells(0, 0, 5, 2) == base
    assert cells(0, 0, -5, 2) == [(-x, y) for x, y in base]
    assert cells(0, 0, 5, -2) == [(x, -y) for x, y in base]
    assert cells(0, 0, -5, -2) == [(-x, -y) for x, y in base]
    assert cells(0, 0, 2, 5) == [(y, x) for x, y in base]
    assert cells(0, 0, -2, -5) == [(-y, -x) for x, y in base]
    assert cells(10, 20, 15, 22) == [(x + 10, y + 20) for x, y in base]
    assert cells(0, 0, 1, 0) == [(0, 0), (1, 0)] and cells(0, 0, -1, 1) == [(0, 0), (-1, 1)]    # da = 1: begin and end alone
    # the restatement of a whole record on a drawn map: a wall at x = 4, free before it, beam (0, 0) -> (6, 0) along the row y = 0
    v = np.zeros((3, 8), np.float32); v[:, 4] = 1.0; v[:, 1:3] = -1.0
    b, s = np_trace(v, 0, 0, 1.0, (0.0, 0.0, 0.0), (0.0, 0.0), [[6.0, 0.0], [3.0, 0.0], [4.0, 0.0], [0.2, 0.1], [2.0, 0.0], [-2.0, 0.0]])
    assert b.tolist() == [(6, 4, 2, 0, 4, 0),          # blocked at a = 4; cells 0 and 3 unknown in front of it; e = (6, 0) is unknown
                          (3, -1, 2, 0, 0, 0),         # ends in front of the wall on the unknown cell 3
                          (4, 4, 2, 1, 4, 0),          # ends on the wall
                          (0, -1, 0, 0, 0, 0),         # same cell
                          (2, -1, 1, 2, 0, 0),         # ends on a free cell: cell 0 unknown
                          (2, -1, 3, 0, 0, 0)]         # leaves the map: (0,0), (-1,0), (-2,0) all class 0
    assert s.tolist() == (5, 1, 0, 1, 1, 1, 10)


# ---- the walk IS the update's line ---------------------------------------------------------------------------------------------------
def test_walk_is_the_update_line(capi, oc):
    """200 single-point scans, each on a Reset 48 x 40 grid of the reference's restatement in C (oracle_c): the cells whose update
    index moved are the cells slamhip_debug_trace_cells lists, and the cell carrying the occupied mark -- the highest index of the
    three an update hands out -- is the last of them.  A beam whose begin or end cell lies outside the map is dropped whole by
    the update (OccGridMap.cs:158-161) and left out here: the points are drawn so that at most a quarter are."""
    oc.set_trig_mode(oc.TRIG_DET)
    try:
        w, h, cell = 48, 40, 0.1
        g = oc.Grid(cell, w, h)
        stm = F(1.0) / F(cell)
        rng = np.random.default_rng(21)
        dropped = same = compared = 0
        for it in range(200):
            g.reset()
            pose = np.array([rng.uniform(1.0, 3.8), rng.uniform(1.0, 3.0), rng.uniform(-4, 4)], np.float32)
            origin = np.array([rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1)], np.float32)
            r, a = rng.uniform(0.0, 2.4), rng.uniform(-math.pi, math.pi)
            xy = np.array([[r * math.cos(a), r * math.sin(a)]], np.float32)
            before = g.cells["update_index"].copy()
            g.update_by_scan(xy, pose, origin)
            idx = g.cells["update_index"].reshape(h, w)
            changed = np.argwhere(idx != before.reshape(h, w))[:, ::-1]        # (x, y)
            bx, by, ex, ey, da = capi.trace_lines(stm, pose, origin, xy)[0].tolist()
            assert da >= 0
            if da == 0:
                same += 1
                assert changed.size == 0
                continue
            if not (0 <= bx < w and 0 <= by < h and 0 <= ex < w and 0 <= ey < h):
                dropped += 1
                assert changed.size == 0
                continue
            cells = capi.trace_cells(bx, by, ex, ey)
            assert len(set(map(tuple, cells.tolist()))) == da + 1
            assert set(map(tuple, cells.tolist())) == set(map(tuple, changed.tolist())), it
            top = np.argwhere(idx == idx.max())[:, ::-1]
            assert top.tolist() == [cells[-1].tolist()] and cells[-1].tolist() == [ex, ey], it
            compared += 1
        assert dropped <= 50 and compared >= 140, (dropped, same, compared)
        g.close()
    finally:
        oc.set_trig_mode(oc.TRIG_LIBM)
