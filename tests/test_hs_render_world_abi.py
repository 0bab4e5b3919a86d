"""K25 (slamhip_hs_render_world) on the CPU, no GPU: the host hook slamhip_debug_render_world -- the definition over caller arrays,
from the header text the kernels run -- against the NumPy restatement of tests/render_world_cases.py (an unbounded grid, the window's
arrays and the tiles routed per cell, its own Bresenham) with == on every cell of every level and on the indices, for every case and
every tile side; against slamhip_debug_render where every line lies inside the window; five wrong copies of the definition, each of
which must fail a named case; the hook's refusals, each of which leaves its arrays untouched."""
import numpy as np
import pytest

import k5_cases as kc
import render_world_cases as wc


@pytest.fixture(scope="module")
def capi():
    import slam.net_amd.build as b
    b.build()
    import slam.net_amd.capi as capi
    return capi


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_cells(got, ref, what):
    for field in ("update_index", "value"):
        g, r = bits(got[field]), bits(ref[field])
        bad = np.flatnonzero(g != r)
        assert bad.size == 0, (what, field, bad.size, bad[:8], got[field][bad[:8]], ref[field][bad[:8]])


def differs(a, b):
    return any((bits(a[l]["value"]) != bits(b[l]["value"])).any() or (a[l]["update_index"] != b[l]["update_index"]).any() for l in range(len(a)))


def logodds(capi, factors):
    """lo_free and lo_occ as the library forms them, read off a three-cell strip after one line."""
    c = np.zeros(3, kc.CELL)
    c["update_index"] = -1
    out, _, _ = capi.debug_render_world([(0, 0, 3, 1)], 1.0, [c], [0], [0], [np.array([[2.0, 0.0]], np.float32)], [(0.0, 0.0)], [(0.0, 0.0, 0.0)], factors=factors)
    return out[0]["value"][0], out[0]["value"][2]


@pytest.fixture(scope="module")
def hooked(capi):
    """Every case through the hook, once."""
    return {name: wc.hook_calls(capi, fn()) for name, fn in wc.CASES.items()}


@pytest.mark.parametrize("T", wc.TILES)
def test_hook_against_restatement(capi, hooked, T):
    for name, fn in wc.CASES.items():
        c = fn()
        got, ui, ci = hooked[name]
        want, wui, wci, _ = wc.restate(c, T, *logodds(capi, c.factors or (0.4, 0.9)))
        for l in range(wc.LEVELS):
            same_cells(got[l], want[l], (name, T, l))
        assert (ui, ci) == (wui, wci), (name, T)


def test_cases_reach_what_they_claim(capi, hooked):
    """Cells outside the window, at negative coordinates on both axes, and the clamp at 50."""
    x0, y0, w, h = wc.rect_of(0)
    for name in ("ends_outside", "begin_outside", "wholly_outside", "negative", "origin_off_tile"):
        v = hooked[name][0][0]["value"].reshape(h, w)
        inside = np.zeros((h, w), bool)
        inside[-y0:-y0 + wc.WIN[1], -x0:-x0 + wc.WIN[0]] = True
        assert (v[~inside] != 0).sum() > 50, name
    assert (hooked["negative"][0][0]["value"].reshape(h, w)[:-y0, :-x0] != 0).sum() > 50
    cx, cy = wc.CLAMP_CELL
    assert hooked["clamp_outside"][0][0]["value"].reshape(h, w)[cy - y0, cx - x0] >= 50.0
    empty = hooked["empty_range_clear"]
    assert (empty[0][0]["update_index"] == -1).all() and empty[1] == [0, 0] and empty[2] == [0, 0]
    assert hooked["empty_range_keep"][1] == [18, 18]


def test_hook_equals_window_hook_when_contained(capi):
    """x0 = y0 = 0, the rectangle the window, every line inside: slamhip_debug_render bit for bit, KEEP included."""
    c = wc.CASES["inside"]()
    dims = kc.level_dims(wc.WIN, wc.LEVELS)
    rects = [(0, 0, w, h) for w, h in dims]
    a, aui, aci = wc.hook_calls(capi, c, rects)
    s = c.scans
    start = []
    for w, h in dims:
        z = np.zeros(w * h, kc.CELL)
        z["update_index"] = -1
        start.append(z)
    b, bui, bci = capi.debug_render(dims, wc.CELL_LEN, start, [0] * wc.LEVELS, [0] * wc.LEVELS, [x[0] for x in s], [x[1] for x in s], [x[2] for x in s])
    for l in range(wc.LEVELS):
        same_cells(a[l], b[l], ("contained", l))
        assert (b[l]["value"] != 0).sum() > 100
    assert (aui, aci) == (bui, bci)
    a2, aui2, _ = capi.debug_render_world(rects, wc.CELL_LEN, a, aui, aci, [x[0] for x in s[:3]], [x[1] for x in s[:3]], [x[2] for x in s[:3]], keep=True)
    b2, bui2, _ = capi.debug_render(dims, wc.CELL_LEN, b, bui, bci, [x[0] for x in s[:3]], [x[1] for x in s[:3]], [x[2] for x in s[:3]], keep=True)
    for l in range(wc.LEVELS):
        same_cells(a2[l], b2[l], ("contained, KEEP", l))
    assert aui2 == bui2


@pytest.mark.parametrize("variant,name", [("trunc", "negative"), ("window_clip", "ends_outside"), ("free_on_end", "free_after_end"),
                                          ("tile_under_window", "origin_off_tile"), ("empty_no_advance", "empty_scan")])
def test_wrong_copies_fail(capi, hooked, variant, name):
    """The cases tell the definition from its wrong copies: truncation instead of rintf (negative coordinates); validity clipped to
    the window; the free transition applied to a cell first touched by an end point; a cell under the window written to its tile
    where the tile straddles the window's edge; the indices not advanced for a scan of 0 points."""
    c = wc.CASES[name]()
    got, ui, ci = hooked[name]
    lo = logodds(capi, c.factors or (0.4, 0.9))
    wrong, wui, wci, _ = wc.restate(c, 16, *lo, variant=variant)
    assert differs(wrong, got) or (wui, wci) != (ui, ci), (variant, name)


def test_hook_refusals(capi):
    """SLAMHIP_ERR_INVALID, the arrays as they were: rule 7's list, the world bound, a line of more than 32767 cells, a box that
    leaves the rectangle -- the first scan valid each time, so that an early draw would show."""
    rects = [(-8, -8, 32, 32)]
    rng = np.random.default_rng(1)
    cells = np.zeros(32 * 32, kc.CELL)
    cells["update_index"] = rng.integers(-1, 5, cells.size)
    cells["value"] = rng.normal(0, 1, cells.size).astype(np.float32)
    good = np.array([[3.0, 1.0], [-4.0, 2.0]], np.float32)

    def refused(rects=rects, cells=cells, ui=(6,), scans=(good, good), poses=((4.0, 4.0, 0.0), (2.0, 1.0, 0.0)), **kw):
        keep0 = cells.copy()
        for keep in (False, True):
            with pytest.raises(capi.SlamhipError) as e:
                capi.debug_render_world(rects, 1.0, [cells], list(ui), [2], list(scans), [(0.0, 0.0)] * len(scans), list(poses), **dict(dict(keep=keep), **kw))
            assert e.value.code == capi.ERR_INVALID
            assert cells.tobytes() == keep0.tobytes()
    for bad in (np.nan, np.inf, -np.inf):
        for k in range(3):
            p = [2.0, 1.0, 0.0]
            p[k] = bad
            refused(poses=((4.0, 4.0, 0.0), tuple(p)))
    refused(flags=2)
    with pytest.raises(capi.SlamhipError):
        capi.debug_render_world(rects, 1.0, [cells], [2 ** 31 - 3], [0], [good], [(0.0, 0.0)], [(4.0, 4.0, 0.0)], keep=True)      # + 3 passes INT_MAX
    refused(poses=((4.0, 4.0, 0.0), (22.0, 1.0, 0.0)))                     # the second scan's end cell (25, 2) leaves the rectangle
    refused(poses=((4.0, 4.0, 0.0), (-9.0, 1.0, 0.0)))                     # ... its begin cell
    refused(poses=((4.0, 4.0, 0.0), (float(2 ** 20 + 1), 0.0, 0.0)))       # the begin cell beyond the world bound
    refused(scans=(good, np.array([[float(2 ** 20 + 1), 0.0]], np.float32)))                 # an end cell beyond it
    refused(scans=(good, np.array([[np.nan, 0.0]], np.float32)))           # a point that is not finite ends beyond it
    long_cells = np.zeros(40000, kc.CELL)
    refused(rects=[(0, 0, 40000, 1)], cells=long_cells, scans=(np.array([[5.0, 0.0]], np.float32), np.array([[32768.0, 0.0]], np.float32)),
            poses=((0.0, 0.0, 0.0), (1.0, 0.0, 0.0)))
    out, ui, _ = capi.debug_render_world([(0, 0, 40000, 1)], 1.0, [long_cells], [0], [0], [np.array([[32767.0, 0.0]], np.float32)], [(0.0, 0.0)], [(1.0, 0.0, 0.0)])
    assert out[0]["update_index"][32768] == 2 and ui == [3]                # ... and 32767 cells are drawn
    # a scan of 0 points asks nothing of its begin cell
    out, ui, ci = capi.debug_render_world(rects, 1.0, [cells], [6], [2], [np.zeros((0, 2), np.float32)], [(0.0, 0.0)], [(float(2 ** 21), 0.0, 0.0)], keep=True)
    assert out[0].tobytes() == cells.tobytes() and (ui, ci) == ([9], [3])
