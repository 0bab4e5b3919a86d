"""CPU-side checks of the view gain's interface (slamhip_hs_view_gain, _view_select, _view_set_covered, _view_get_covered,
_view_clear, slamhip_hsproc_view_gain, _view_select, slamhip_debug_view) and the NumPy restatement of its definition
(include/slamhip.h, slamhip_view_summary) that tests/test_gpu_hector_view.py compares the device with.  Lines, cells and classes
are the beam trace's restatement (tests/test_hs_trace_abi.py); V is a Python set of cells and the greedy loop is written literally.
Everything is compared with ==.  No compute calls on a device: what needs an hs (the refusals and state errors of the device calls)
is checked in the GPU file."""
import math
import os
import re

import numpy as np
import pytest

from test_hs_trace_abi import np_cells, np_class_bits, np_lines, np_trace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("slamhip_hs_view_gain", "slamhip_hs_view_select", "slamhip_hs_view_set_covered", "slamhip_hs_view_get_covered", "slamhip_hs_view_clear",
           "slamhip_hsproc_view_gain", "slamhip_hsproc_view_select", "slamhip_debug_view")
F = np.float32
CELL0 = 0.1
STM = F(1.0) / F(CELL0)
FIELDS = ("n_walked", "n_same", "n_ignored", "n_cut", "n_seen", "n_unknown", "n_free", "n_occupied", "n_new", "n_new_unknown")
DIMS = [(40, 24), (64, 64), (96, 72)]          # w not a multiple of 32; a row of one word short of two; three words
KINDS = ["rooms", "wall", "unknown"]
REACHES = [1, 2, 31, 32, 33, 255]
SCAN_SIZES = [1, 63, 64, 65, 257, 1080]
ORIGIN = (0.03, -0.02)


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
def map_of(w, h, kind):
    """An (h, w) float32 array of cell Values: rooms (free inside walls, a door, an unknown patch, a NaN), a lone wall in the unknown,
    or all unknown."""
    v = np.zeros((h, w), F)
    if kind == "rooms":
        v[2:h - 2, 2:w - 2] = -0.7
        v[2, 2:w - 2] = v[h - 3, 2:w - 2] = 1.5
        v[2:h - 2, 2] = v[2:h - 2, w - 3] = 1.5
        v[2:h - 2, w // 2] = 0.4
        v[h // 2:h // 2 + 2, w // 2] = -0.7                                   # the door
        v[h // 3:h // 3 + 3, w // 4:w // 4 + 4] = 0.0
        v[h // 3 + 1, w // 4 + 1] = np.nan
        v[h // 3 + 1, w // 4 + 2] = -0.0
    elif kind == "wall":
        v[h // 4:3 * h // 4, (2 * w) // 3] = 2.0
    return v


def poses_of(w, h):
    """Window-frame poses: the middle, each corner, one cell outside each border, far outside (an empty box), and no number."""
    c = CELL0
    return [((w / 2 + 0.3) * c, (h / 2 - 0.2) * c, 0.4),
            (0.2 * c, 0.1 * c, 0.9), ((w - 1.2) * c, 0.2 * c, 2.2), (0.1 * c, (h - 1.1) * c, -0.6), ((w - 0.8) * c, (h - 0.9) * c, -2.4),
            (-1.0 * c, (h / 2) * c, 0.1), (w * c, (h / 3) * c, 3.0), ((w / 3) * c, -1.0 * c, 1.5), ((w / 2) * c, h * c, -1.6),
            (5000.0 * c, -5000.0 * c, 0.7),
            (float("nan"), 1.0, 0.0)]


def scan_of(n, seed=0):
    """n points in the robot's frame around ORIGIN: ranges from 2 to 70 cells and a few of 600 (cut at every reach here); with n >= 3
    a point equal to the origin (a same beam) and a NaN point (ignored)."""
    rng = np.random.default_rng(100 + n + seed)
    if n == 1:
        return (np.array([[0.9 * math.cos(0.3), 0.9 * math.sin(0.3)]]) + ORIGIN).astype(F)
    a = np.linspace(-math.pi, math.pi, n, endpoint=False) + 0.01
    r = rng.uniform(0.2, 7.0, n)
    r[::17] = 60.0
    xy = (np.stack([r * np.cos(a), r * np.sin(a)], 1) + ORIGIN).astype(F)
    if n >= 3:
        xy[1] = F(ORIGIN)
        xy[2] = (np.nan, 0.5)
    return xy


def covered_of(w, h, seed):
    """A random covered bitmap with every padding bit SET: they are to be ignored."""
    rng = np.random.default_rng(seed)
    m = rng.random((h, w)) < 0.4
    m[:, :w // 3] = True
    wpr = (w + 31) // 32
    pad = np.ones((h, wpr * 32), np.uint8)
    pad[:, :w] = m
    return np.packbits(pad, axis=1, bitorder="little").view(np.uint32).reshape(h, wpr), m


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def np_view(values, stm, pose, origin, xy, reach, covered_mask=None):
    """Steps 1 - 5 for one pose -> (V as a set of (x, y), the summary as a dict, sum over the walked and same beams of stop + 1)."""
    cls = np_class_bits(values)
    h, w = cls.shape
    V = set()
    s = dict.fromkeys(FIELDS, 0)
    bound = 0
    for bx, by, ex, ey, da in np_lines(stm, pose, origin, xy).tolist():
        if da < 0:
            s["n_ignored"] += 1
            continue
        if da == 0:
            s["n_same"] += 1
            bound += 1
            if 0 <= bx < w and 0 <= by < h:
                V.add((bx, by))
            continue
        s["n_walked"] += 1
        c = np_cells(bx, by, ex, ey)[:min(da, reach) + 1]
        x, y = c[:, 0], c[:, 1]
        ok = (x >= 0) & (x < w) & (y >= 0) & (y < h)
        k = np.where(ok, cls[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)], 0)
        occ = np.flatnonzero(k == 1)
        first = int(occ[0]) if occ.size else -1                               # (among the steps <= reach: a later one cannot lower stop)
        stop = min(first if first >= 0 else da, reach)
        bound += stop + 1
        if da > reach and first < 0:
            s["n_cut"] += 1
        V.update((int(p), int(q)) for p, q, o in zip(x[:stop + 1], y[:stop + 1], ok[:stop + 1]) if o)
    for (x, y) in V:
        k = int(cls[y, x])
        s["n_seen"] += 1
        s[("n_unknown", "n_occupied", "n_free")[k]] += 1
        if covered_mask is None or not covered_mask[y, x]:
            s["n_new"] += 1
            s["n_new_unknown"] += int(k == 0)
    return V, s, bound


def mask_of(V, w, h):
    m = np.zeros((h, w), bool)
    for x, y in V:
        m[y, x] = True
    return m


def np_select(views, cls, covered_mask, mode, min_gain, k):
    """Step 6, literally.  views: the poses' V as sets -> (order, gains, the layer after the choice as a set)."""
    C = {(int(x), int(y)) for y, x in np.argwhere(covered_mask)}
    chosen, order, gains = set(), [], []
    for _ in range(k):
        best, bg = -1, -1
        for p, V in enumerate(views):
            if p in chosen:
                continue
            new = V - C
            g = len(new) if mode == 0 else sum(1 for (x, y) in new if cls[y, x] == 0)
            if g > bg:
                best, bg = p, g
        if best < 0 or bg < min_gain:
            break
        order.append(best); gains.append(bg); chosen.add(best)
        C |= views[best]
    return order, gains, C


def sdict(rec):
    return {k: int(rec[k]) for k in FIELDS}


# ---- the interface -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def capi():
    import slam.net_amd.build as b
    b.build()
    import slam.net_amd.capi as capi
    return capi


def test_surface(capi):
    h = open(os.path.join(ROOT, "include", "slamhip.h")).read()
    assert capi.VIEW_SUMMARY.itemsize == 40 and capi.VIEW_SUMMARY.names == FIELDS
    assert all(capi.VIEW_SUMMARY.fields[n][1] == 4 * i for i, n in enumerate(FIELDS))         # ten int32, no padding
    assert "ten int32_t, 40 bytes, no padding" in h
    assert "SLAMHIP_K_COUNT = 10" in h                                        # no new timing class
    L = capi.lib()
    for name in SYMBOLS:
        assert hasattr(L, name) and name in L._signatures and name in capi.declared_symbols(), name
    assert len(L._signatures["slamhip_hs_view_gain"][1]) == 7 and len(L._signatures["slamhip_hs_view_select"][1]) == 11
    assert len(L._signatures["slamhip_hsproc_view_gain"][1]) == 10 and len(L._signatures["slamhip_hsproc_view_select"][1]) == 14
    assert len(L._signatures["slamhip_debug_view"][1]) == 12
    assert (capi.VIEW_MAX_REACH, capi.VIEW_MAX_POSES, capi.VIEW_MAX_K) == (4096, 4096, 64)
    import slam.net_amd.hector as hm
    for name in ("view_gain", "view_select", "covered", "view_clear"):
        assert hasattr(hm.MapRepMultiMap, name), name
    assert hasattr(hm.HectorSLAMProcessor, "ViewGain") and hasattr(hm.HectorSLAMProcessor, "ViewSelect")
    # the C# shim binds every entry point and its classes call them
    shim = os.path.join(ROOT, "bindings", "csharp", "SlamHip")
    native = open(os.path.join(shim, "SlamHip.Native.cs")).read()
    used = open(os.path.join(shim, "HectorSLAM", "MapRepMultiMap.Hip.cs")).read() + open(os.path.join(shim, "HectorSLAM", "HectorSLAMProcessor.Hip.cs")).read()
    for name in SYMBOLS:
        assert re.search(r"static extern int %s\(" % name, native), name
        assert "Native.%s(" % name in used, name
    assert "struct ViewSummary" in native
    # the K8 text points at K15
    assert "once per beam that crosses it" in h and "once per beam that crosses it" in open(os.path.join(ROOT, "DESIGN.md")).read()
    # the sources are part of the build
    import slam.net_amd.build as b
    assert "hs_view.hip" in b.SOURCES and "hs_view.h" in b.HEADERS
    lds = int(re.search(r"#define K15_LDS_WORDS (\d+)", open(os.path.join(b.CSRC, "hs_view.h")).read()).group(1))
    assert lds == capi.VIEW_LDS_WORDS and 511 * 17 <= lds and 2 * (4 * lds + 1024) <= 160 * 1024    # reach 255 fits; two workgroups per compute unit


def test_refusals_of_the_hook(capi):
    v = np.zeros((4, 4), F)
    for bad in (dict(reach=0), dict(reach=4097)):
        with pytest.raises(capi.SlamhipError) as e:
            capi.debug_view(v, 1.0, (0, 0, 0), (0, 0), [[1, 1]], bad["reach"])
        assert e.value.code == capi.ERR_INVALID
    L = capi.lib()
    out = np.zeros((4, 1), np.uint32); s = np.zeros(1, capi.VIEW_SUMMARY)
    p = capi.f32((0, 0, 0)); o = capi.f32((0, 0))
    import ctypes as C
    vp = C.c_void_p
    assert L.slamhip_debug_view(capi.fptr(v), 0, 4, C.c_float(1.0), capi.fptr(p), capi.fptr(o), None, 0, 1, None, out.ctypes.data_as(vp),
                                s.ctypes.data_as(vp)) == capi.ERR_INVALID
    assert L.slamhip_debug_view(capi.fptr(v), 4, 4, C.c_float(1.0), capi.fptr(p), capi.fptr(o), None, 0, 1, None, out.ctypes.data_as(vp),
                                s.ctypes.data_as(vp)) == 0                    # an empty scan is no error here
    assert sdict(s[0]) == dict.fromkeys(FIELDS, 0) and not out.any()


# ---- the restatement against the hook ------------------------------------------------------------------------------------------------
def sampled_cases():
    """(w, h, kind, reach, pose index, scan size, covered?) -- every map with every reach and pose; the scan size and the covered
    layer rotate so that every scan size meets every reach and every pose kind."""
    for mi, ((w, h), kind) in enumerate((d, k) for d in DIMS for k in KINDS):
        for ri, reach in enumerate(REACHES):
            for pi in range(len(poses_of(w, h))):
                yield w, h, kind, reach, pi, SCAN_SIZES[(mi + ri + pi) % len(SCAN_SIZES)], (mi + ri + pi) % 2 == 1


def check_case(capi, w, h, kind, reach, pi, n, with_cov):
    values = map_of(w, h, kind)
    pose = poses_of(w, h)[pi]
    xy = scan_of(n)
    cov_bits, cov_mask = covered_of(w, h, 7 * n + reach) if with_cov else (None, None)
    bits, rec = capi.debug_view(values, STM, pose, ORIGIN, xy, reach, cov_bits)
    V, s, bound = np_view(values, STM, pose, ORIGIN, xy, reach, cov_mask)
    tag = (w, h, kind, reach, pi, n, with_cov)
    assert sdict(rec) == s, (tag, sdict(rec), s)
    assert np.array_equal(capi.view_unpack(bits, w), mask_of(V, w, h)), tag
    assert np.array_equal(bits, capi.view_pack(mask_of(V, w, h))), tag        # (the padding bits of the output are zero)
    assert s["n_walked"] + s["n_same"] + s["n_ignored"] == n, tag
    assert s["n_unknown"] + s["n_free"] + s["n_occupied"] == s["n_seen"] and s["n_new_unknown"] <= s["n_new"] <= s["n_seen"], tag
    assert s["n_seen"] <= bound, tag
    return s, bound


@pytest.mark.parametrize("dims", DIMS)
def test_hook_equals_restatement(capi, dims):
    tot = dict.fromkeys(FIELDS, 0)
    for case in sampled_cases():
        if case[:2] != dims:
            continue
        s, _ = check_case(capi, *case)
        for k in FIELDS:
            tot[k] += s[k]
    assert all(tot[k] > 0 for k in FIELDS), tot                               # every field is exercised on every map size


def test_single_beam_inside_sees_stop_plus_one(capi):
    """One beam that stays inside the window: its cells are distinct, so n_seen == stop + 1."""
    for w, h in DIMS:
        for reach in REACHES:
            s, bound = check_case(capi, w, h, "unknown", reach, 0, 1, False)
            da = int(np_lines(STM, poses_of(w, h)[0], ORIGIN, scan_of(1))[0, 4])
            assert 5 <= da <= 9
            assert s["n_seen"] == bound == min(da, reach) + 1 and s["n_cut"] == (1 if reach < da else 0), (w, h, reach, s, bound)


def test_stop_at_reach_and_one_past(capi):
    """A wall at x = 20 + d in an unknown 64 x 64 map, the sensor in cell (20, 30), one beam along +x to cell (60, 30).  reach == d: the
    beam is stopped exactly at step reach -- the wall is seen, the beam is not cut.  reach == d - 1: the wall lies at step reach + 1
    -- the beam is cut and the wall is not seen.  reach > d: nothing past the wall is seen."""
    for d in (1, 2, 9, 31, 32, 33):
        v = np.zeros((64, 64), F)
        v[:, 20 + d] = 1.0
        pose = (20.0 * CELL0, 30.0 * CELL0, 0.0)
        xy = np.array([[40.0 * CELL0, 0.0]], F)
        for reach, seen, occ, cut in ((d, d + 1, 1, 0), (d + 2, d + 1, 1, 0)) + (((d - 1, d, 0, 1),) if d > 1 else ()):
            bits, rec = capi.debug_view(v, STM, pose, (0.0, 0.0), xy, reach)
            V, s, _ = np_view(v, STM, pose, (0.0, 0.0), xy, reach)
            assert sdict(rec) == s and V == {(20 + a, 30) for a in range(seen)}, (d, reach, s)
            assert (s["n_seen"], s["n_occupied"], s["n_cut"], s["n_walked"]) == (seen, occ, cut, 1), (d, reach, s)
            assert np.array_equal(capi.view_unpack(bits, 64), mask_of(V, 64, 64))


def test_fan_counts_cells_once(capi):
    """A 360-beam fan of 20-cell beams in an all-unknown map: the per-beam sum that the trace reports (unknown_cells) counts the cells
    next to the sensor once per beam; n_seen counts each once."""
    w, h = 64, 64
    v = np.zeros((h, w), F)
    a = np.linspace(-math.pi, math.pi, 360, endpoint=False)
    xy = np.stack([2.0 * np.cos(a), 2.0 * np.sin(a)], 1).astype(F)
    pose = (32.0 * CELL0, 32.0 * CELL0, 0.0)
    _, rec = capi.debug_view(v, STM, pose, (0.0, 0.0), xy, 255)
    _, ts = np_trace(v, 0, 0, STM, pose, (0.0, 0.0), xy)
    s = sdict(rec)
    assert s["n_seen"] == s["n_unknown"] == s["n_new"] == s["n_new_unknown"] and s["n_walked"] == 360 and s["n_cut"] == 0
    assert int(ts["unknown_cells"]) > 4 * s["n_seen"] and s["n_seen"] <= 41 * 41, (int(ts["unknown_cells"]), s)


def test_covered_everything_and_padding(capi):
    for w, h in DIMS:
        values = map_of(w, h, "rooms")
        xy = scan_of(257)
        pose = poses_of(w, h)[0]
        wpr = capi.view_words(w)
        full = np.full((h, wpr), 0xFFFFFFFF, np.uint32)
        bits, rec = capi.debug_view(values, STM, pose, ORIGIN, xy, 33, full)
        assert int(rec["n_new"]) == 0 and int(rec["n_new_unknown"]) == 0 and int(rec["n_seen"]) > 50
        # only padding bits set: the same as an empty layer
        pad_only = ~capi.view_pack(np.ones((h, w), bool))
        assert (w % 32 == 0) == (not pad_only.any())
        _, r0 = capi.debug_view(values, STM, pose, ORIGIN, xy, 33, None)
        _, r1 = capi.debug_view(values, STM, pose, ORIGIN, xy, 33, pad_only)
        assert sdict(r0) == sdict(r1) and int(r0["n_new"]) == int(r0["n_seen"])
        # V itself as the layer: nothing is new; its complement: everything is
        _, r2 = capi.debug_view(values, STM, pose, ORIGIN, xy, 33, bits)
        _, r3 = capi.debug_view(values, STM, pose, ORIGIN, xy, 33, ~bits)
        assert int(r2["n_new"]) == 0 and int(r3["n_new"]) == int(r3["n_seen"])
        assert np.array_equal(capi.view_pack(capi.view_unpack(bits, w)), bits)


def test_literal_greedy_loop():
    """np_select on hand-made sets: ties go to the lowest index, a repeated view gains nothing, min_gain stops the choice, and in mode 1
    all of V joins the layer."""
    cls = np.zeros((4, 8), np.int64); cls[0, :] = 2
    A = {(0, 0), (1, 0), (2, 1)}; B = {(5, 1), (6, 1), (7, 1)}; D = {(0, 0), (3, 2), (4, 2), (5, 2), (6, 2)}
    none = np.zeros((4, 8), bool)
    assert np_select([A, B, A, D], cls, none, 0, 1, 8)[:2] == ([3, 1, 0], [5, 3, 2])      # A == views[2] is never chosen twice
    assert np_select([A, B], cls, none, 0, 1, 8)[:2] == ([0, 1], [3, 3])                  # a tie: the lowest index first
    assert np_select([A, B, D], cls, none, 0, 4, 8)[:2] == ([2], [5])
    assert np_select([A, B, D], cls, none, 0, 6, 8)[:2] == ([], [])
    order, gains, C = np_select([A, B, D], cls, none, 1, 1, 2)
    assert (order, gains) == ([2, 1], [4, 3]) and C == D | B                              # (0, 0) is free: no gain in mode 1, but it joins C
