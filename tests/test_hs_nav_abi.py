"""CPU-side checks of the cost-to-go field's interface (slamhip_hs_nav_field, slamhip_hsproc_nav_field, slamhip_debug_nav_field) and
the restatement of its definition (include/slamhip.h, slamhip_hs_nav_field, steps 2 - 9) that tests/test_gpu_hector_nav.py compares
the device with.

The restatement: traversability from a brute-force scan of squared distances over a padded site array, the allowed moves from
shifted NumPy arrays, the costs from a heapq Dijkstra, dir, goals and paths from literal loops.  It shares nothing with hs_nav.h,
whose text -- traversable words, 3-bit windows, a move mask -- the hook and the kernels run.  Every comparison is == on integers."""
import ctypes as C
import heapq
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("slamhip_hs_nav_field", "slamhip_hsproc_nav_field", "slamhip_debug_nav_field")
UNREACHED = 0xFFFFFFFF
MOVES = [(1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1)]   # step 3, d = 0 .. 7
SUMMARY_FIELDS = ("mx0", "my0", "mw", "mh", "n_traversable", "n_reached", "n_sources_used", "n_sources_blocked", "max_cost_reached")
SHAPES = [(1, 1), (1, 70), (70, 1), (33, 31), (97, 66)]                    # (w, h)
BIG = SHAPES[3:]                                                           # the shapes that hold the open block


def weight(d):
    return 7 if d % 2 else 5


def np_traversable(cls, c, site_mask):
    """Step 2 by brute force: free, and no site at a squared distance <= c * c.  Outside the array every cell is class 0."""
    free = cls == 2
    if c == 0:
        return free
    h, w = cls.shape
    site = (cls == 1) | (cls == 0) if site_mask == 3 else cls == 1
    P = np.pad(site, c, constant_values=(site_mask == 3))
    near = np.zeros((h, w), bool)
    for dy in range(-c, c + 1):
        for dx in range(-c, c + 1):
            if dx * dx + dy * dy <= c * c:
                near |= P[c + dy:c + dy + h, c + dx:c + dx + w]
    return free & ~near


def shifted(T, dx, dy):
    """N[y, x] = T[y + dy, x + dx], False outside."""
    h, w = T.shape
    return np.pad(T, 1)[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]


def np_allowed(T):
    """Step 3: allowed[d][y, x] iff the move d from (x, y) is allowed."""
    out = []
    for d, (dx, dy) in enumerate(MOVES):
        a = T & shifted(T, dx, dy)
        if d % 2:
            a = a & shifted(T, dx, 0) & shifted(T, 0, dy)
        out.append(a)
    return out


def np_nav(cls, sources, c=0, site_mask=2, max_cost=0, goals=(), n_paths=0, max_path_cells=1, x0=0, y0=0, rect=None):
    """The definition over cls, the classes of M whose first cell is (x0, y0) of the frame sources, goals and rect are given in.
    -> the dict capi.nav_call returns (the summary a plain dict without `rounds`)."""
    h, w = cls.shape
    T = np_traversable(cls, c, site_mask)
    allowed = np_allowed(T)
    cost = np.full((h, w), UNREACHED, np.uint32)
    used = blocked = 0
    heap = []
    for sx, sy in np.asarray(sources, np.int64).reshape(-1, 2):
        x, y = int(sx) - x0, int(sy) - y0
        if 0 <= x < w and 0 <= y < h and T[y, x]:
            used += 1
            cost[y, x] = 0
            heap.append((0, y, x))
        else:
            blocked += 1
    heapq.heapify(heap)
    while heap:
        k, y, x = heapq.heappop(heap)
        if k != cost[y, x]:
            continue
        for d, (dx, dy) in enumerate(MOVES):
            if allowed[d][y, x]:
                v = k + weight(d)
                if (max_cost == 0 or v <= max_cost) and v < cost[y + dy, x + dx]:
                    cost[y + dy, x + dx] = v
                    heapq.heappush(heap, (v, y + dy, x + dx))
    dirs = np.full((h, w), 255, np.uint8)
    for y in range(h):
        for x in range(w):
            k = int(cost[y, x])
            if k == UNREACHED:
                continue
            if k == 0:
                dirs[y, x] = 8
                continue
            for d, (dx, dy) in enumerate(MOVES):
                if allowed[d][y, x] and cost[y + dy, x + dx] != UNREACHED and int(cost[y + dy, x + dx]) + weight(d) == k:
                    dirs[y, x] = d
                    break
            assert dirs[y, x] < 8
    reached = cost != UNREACHED
    summary = dict(mx0=x0, my0=y0, mw=w, mh=h, n_traversable=int(T.sum()), n_reached=int(reached.sum()), n_sources_used=used,
                   n_sources_blocked=blocked, max_cost_reached=int(cost[reached].max()) if reached.any() else 0)
    res = []
    for gx0, gy0, gx1, gy1 in np.asarray(goals, np.int64).reshape(-1, 4):
        best = (UNREACHED, 0, 0)
        n = 0
        for y in range(max(int(gy0) - y0, 0), min(int(gy1) - y0, h - 1) + 1):
            for x in range(max(int(gx0) - x0, 0), min(int(gx1) - x0, w - 1) + 1):
                if reached[y, x]:
                    n += 1
                    if cost[y, x] < best[0]:
                        best = (int(cost[y, x]), x + x0, y + y0)
        res.append(best + (n,))
    paths, lengths = [], []
    for i in range(n_paths):
        cells = []
        if res[i][0] != UNREACHED:
            x, y = res[i][1] - x0, res[i][2] - y0
            while True:
                cells.append((x + x0, y + y0))
                d = int(dirs[y, x])
                if d == 8:
                    break
                x, y = x + MOVES[d][0], y + MOVES[d][1]
        lengths.append(len(cells))
        paths.append(np.array(cells[:max_path_cells], np.int32).reshape(-1, 2))
    out = dict(summary=summary, goals=res, paths=paths, path_cells=lengths)
    if rect is not None:
        out["cost"] = np_rect(cost, (x0, y0, w, h), rect, UNREACHED)
        out["dir"] = np_rect(dirs, (x0, y0, w, h), rect, 255)
    return out


def np_rect(a, m, rect, outside):
    """The array `a` over M = m = (mx0, my0, mw, mh) cut to rect = (x, y, w, h), `outside` outside M."""
    x, y, w, h = rect
    out = np.full((h, w), outside, a.dtype)
    xa, xb = max(x, m[0]), min(x + w, m[0] + m[2]); ya, yb = max(y, m[1]), min(y + h, m[1] + m[3])
    if xa < xb and ya < yb:
        out[ya - y:yb - y, xa - x:xb - x] = a[ya - m[1]:yb - m[1], xa - m[0]:xb - m[0]]
    return out


def check(got, want, tag=None):
    """A result of capi.nav_call against np_nav's."""
    for f in SUMMARY_FIELDS:
        assert int(got["summary"][f]) == want["summary"][f], (tag, f, got["summary"], want["summary"])
    assert [tuple(int(v) for v in r) for r in got["goals"]] == [tuple(r) for r in want["goals"]], tag
    assert [int(v) for v in got["path_cells"]] == list(want["path_cells"]), tag
    assert len(got["paths"]) == len(want["paths"])
    for a, b in zip(got["paths"], want["paths"]):
        assert np.array_equal(a, b), tag
    for f in ("cost", "dir"):
        if f in want and f in got:
            assert np.array_equal(got[f], want[f]), (tag, f, np.argwhere(got[f] != want[f])[:5])


def serpentine(w, h):
    """One-cell corridors on the even rows, joined by a one-cell gap at alternating ends of the odd rows; the rest occupied.  The only
    path from (0, 0) runs through every free cell: (h + 1) / 2 * w + (h - 1) / 2 cells (h odd), every move a straight one."""
    c = np.ones((h, w), np.uint8)
    c[0::2] = 2
    for i, y in enumerate(range(1, h, 2)):
        c[y, w - 1 if i % 2 == 0 else 0] = 2
    return c


def random_classes(shape, seed=0):
    """About 60 % free / 25 % occupied / 15 % unknown; the shapes of BIG also hold an open 9 x 9 block, so that a clearance of 3
    leaves something traversable."""
    w, h = shape
    rng = np.random.default_rng([seed, w, h])
    c = rng.choice(np.array([2, 1, 0], np.uint8), size=(h, w), p=[0.62, 0.24, 0.14])
    if shape in BIG:
        c[h // 2 - 4:h // 2 + 5, w // 2 - 4:w // 2 + 5] = 2
    return c


def random_sources(cls, n):
    """n = 1: the middle cell.  n = 5: the middle cell twice, an occupied cell (or the first cell), a cell outside, the last free cell."""
    h, w = cls.shape
    mid = (w // 2, h // 2)
    if n == 1:
        return [mid]
    occ = np.argwhere(cls == 1)
    free = np.argwhere(cls == 2)
    return [mid, tuple(int(v) for v in occ[0][::-1]) if len(occ) else (0, 0), (-3, 5), mid,
            tuple(int(v) for v in free[-1][::-1]) if len(free) else (w - 1, h - 1)]


def random_goals(shape):
    w, h = shape
    return [(0, 0, w - 1, h - 1), (w // 2, h // 2, w // 2, h // 2), (-5, -5, 2, 2), (w - 2, h // 3, w + 4, h // 3 + 3), (w + 2, 0, w + 9, 3),
            (w // 4, h // 4, w // 4 + 6, h // 4 + 5)]


@pytest.fixture(scope="module")
def capi():
    import slam.net_amd.build as b
    b.build()
    import slam.net_amd.capi as capi
    return capi


@pytest.fixture(scope="module")
def arrays():
    out = {s: random_classes(s) for s in SHAPES}
    for a in out.values():
        a.setflags(write=False)
    return out


# ---- the surface -------------------------------------------------------------------------------------------------------------------
def test_surface(capi):
    L = capi.lib()
    header = open(os.path.join(ROOT, "include", "slamhip.h")).read()
    for n in SYMBOLS:
        assert hasattr(L, n) and n in L._signatures and re.search(r"\b%s\s*\(" % n, header)
    assert len(L._signatures["slamhip_hs_nav_field"][1]) == 18 == len(L._signatures["slamhip_hsproc_nav_field"][1])
    assert len(L._signatures["slamhip_debug_nav_field"][1]) == 22
    sizes = {"spec": (capi.NAV_SPEC, 20, ["level", "world", "site_mask", "clearance", "max_cost"]),
             "goal_result": (capi.NAV_GOAL_RESULT, 16, ["cost", "bx", "by", "n_reached"]),
             "path": (capi.NAV_PATH, 8, ["n_cells", "n_written"]),
             "summary": (capi.NAV_SUMMARY, 40, list(SUMMARY_FIELDS) + ["rounds"])}
    for name, (dt, size, fields) in sizes.items():
        assert dt.itemsize == size and list(dt.names) == fields and [dt.fields[f][1] for f in fields] == list(range(0, size, 4)), name
        body = re.search(r"typedef struct slamhip_nav_%s \{(.*?)\} slamhip_nav_%s;" % (name, name), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        assert re.findall(r"(\w+)\s*[,;]", body) == fields, name           # the header's members, in order
    assert capi.NAV_SUMMARY.fields["max_cost_reached"][0] == np.uint32 and capi.NAV_GOAL_RESULT.fields["cost"][0] == np.uint32
    assert "#define SLAMHIP_NAV_UNREACHED 0xFFFFFFFFu" in header and capi.NAV_UNREACHED == UNREACHED
    assert list(zip(capi.NAV_DX, capi.NAV_DY)) == MOVES
    native = open(os.path.join(ROOT, "bindings", "csharp", "SlamHip", "SlamHip.Native.cs")).read()
    for n in SYMBOLS:
        assert n in native
    assert "struct NavSpec" in native and "struct NavGoalResult" in native and "struct NavPath" in native and "struct NavSummary" in native
    import slam.net_amd.build as b
    import slam.net_amd.hector as hm
    assert hasattr(hm.MapRepMultiMap, "nav_field") and hasattr(hm.HectorSLAMProcessor, "NavField") and hasattr(hm.HectorSLAMProcessor, "ExploreGoals")
    assert "hs_nav.hip" in b.SOURCES and "hs_nav.h" in b.HEADERS
    src = open(os.path.join(ROOT, "slam.net_amd", "csrc", "hs_nav.hip")).read()
    assert re.search(r"#define K11_TILE (\d+)", src) and re.search(r"#define K11_BATCH (\d+)", src)


# ---- random class arrays -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_cost", [0, 60])
@pytest.mark.parametrize("n_sources", [1, 5])
@pytest.mark.parametrize("site_mask", [2, 3])
@pytest.mark.parametrize("c", [0, 1, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_random_arrays(capi, arrays, shape, c, site_mask, n_sources, max_cost):
    cls = arrays[shape]
    w, h = shape
    src = random_sources(cls, n_sources)
    goals = random_goals(shape)
    rect = (-3, -2, w + 7, h + 5)
    want = np_nav(cls, src, c, site_mask, max_cost, goals, 3, 40, rect=rect)
    got = capi.debug_nav_field(cls, src, site_mask, c, max_cost, goals, 3, 40, rect=rect)
    check(got, want, (shape, c, site_mask, n_sources, max_cost))
    assert got["summary"]["rounds"] == 0
    if n_sources == 5:
        assert got["summary"]["n_sources_used"] + got["summary"]["n_sources_blocked"] == 5 and got["summary"]["n_sources_blocked"] >= 2
    only_cost = capi.debug_nav_field(cls, src, site_mask, c, max_cost, rect=rect, want_dir=False)
    assert "dir" not in only_cost and np.array_equal(only_cost["cost"], want["cost"])
    only_dir = capi.debug_nav_field(cls, src, site_mask, c, max_cost, rect=rect, want_cost=False)
    assert "cost" not in only_dir and np.array_equal(only_dir["dir"], want["dir"])


@pytest.mark.parametrize("site_mask", [2, 3])
@pytest.mark.parametrize("shape", BIG)
def test_random_arrays_hold_what_they_should(arrays, shape, site_mask):
    """The arrays exercise what they are meant to: with no clearance a source reaches at least a third of the free cells and
    leaves at least one traversable cell unreached; with a clearance of 3 something stays traversable."""
    cls = arrays[shape]
    frac = [(cls == k).mean() for k in (2, 1, 0)]
    assert 0.55 < frac[0] < 0.70 and 0.18 < frac[1] < 0.30 and 0.09 < frac[2] < 0.20, frac
    for n in (1, 5):
        s = np_nav(cls, random_sources(cls, n), 0, site_mask)["summary"]
        assert 3 * s["n_reached"] >= int((cls == 2).sum()) and s["n_reached"] < s["n_traversable"], s
    s = np_nav(cls, random_sources(cls, 1), 3, site_mask)["summary"]
    assert s["n_traversable"] >= 1 and s["n_reached"] >= 1, s
    capped = np_nav(cls, random_sources(cls, 1), 0, site_mask, 60)["summary"]
    assert 1 < capped["n_reached"] < np_nav(cls, random_sources(cls, 1), 0, site_mask)["summary"]["n_reached"] and capped["max_cost_reached"] <= 60


# ---- hand cases --------------------------------------------------------------------------------------------------------------------
def test_open_block_from_its_centre(capi):
    c = np.full((9, 9), 2, np.uint8)
    got = capi.debug_nav_field(c, [(4, 4)])
    a = np.abs(np.arange(9) - 4)
    want = 5 * np.abs(a[:, None] - a[None, :]) + 7 * np.minimum(a[:, None], a[None, :])
    assert np.array_equal(got["cost"], want.astype(np.uint32))
    assert got["dir"][4, 4] == 8 and got["dir"][4, 0] == 0 and got["dir"][0, 4] == 2 and got["dir"][0, 0] == 1 and got["dir"][8, 8] == 5
    s = got["summary"]
    assert (s["n_traversable"], s["n_reached"], s["n_sources_used"], s["n_sources_blocked"], s["max_cost_reached"]) == (81, 81, 1, 0, 28)
    check(got, np_nav(c, [(4, 4)], rect=(0, 0, 9, 9)))


def test_no_corner_cutting(capi):
    """Two free squares that meet only at a corner: the diagonal between them would cut two occupied corners."""
    c = np.ones((6, 6), np.uint8)
    c[0:3, 0:3] = 2
    c[3:6, 3:6] = 2
    got = capi.debug_nav_field(c, [(0, 0)], goals=[(3, 3, 5, 5), (2, 2, 2, 2)])
    assert (got["cost"][3:, 3:] == UNREACHED).all() and (got["dir"][3:, 3:] == 255).all()
    assert tuple(got["goals"][0]) == (UNREACHED, 0, 0, 0) and tuple(got["goals"][1]) == (14, 2, 2, 1)
    assert got["summary"]["n_traversable"] == 18 and got["summary"]["n_reached"] == 9
    c[2, 3] = 2                                                            # one of the two corners opened: still no diagonal, but a way round
    got = capi.debug_nav_field(c, [(0, 0)], goals=[(3, 3, 3, 3)])
    assert tuple(got["goals"][0]) == (14 + 5 + 5, 3, 3, 1)
    check(got, np_nav(c, [(0, 0)], goals=[(3, 3, 3, 3)], rect=(0, 0, 6, 6)))


def test_doorway_closes_with_clearance(capi):
    c = np.full((7, 11), 2, np.uint8)
    c[:, 5] = 1
    c[3, 5] = 2                                                            # a one-cell doorway in a wall
    open_ = capi.debug_nav_field(c, [(1, 3)], goals=[(9, 3, 9, 3)])
    assert tuple(open_["goals"][0]) == (40, 9, 3, 1) and open_["summary"]["n_reached"] == 7 * 10 + 1
    shut = capi.debug_nav_field(c, [(1, 3)], clearance=1, goals=[(9, 3, 9, 3)])
    assert tuple(shut["goals"][0]) == (UNREACHED, 0, 0, 0)
    # columns 4 and 6 touch the wall, but (4, 3) and (6, 3) touch only the doorway's free cell; the doorway itself touches the wall
    assert shut["summary"]["n_traversable"] == 2 * 7 * 4 + 2 and shut["summary"]["n_reached"] == 7 * 4 + 1 and shut["cost"][3, 5] == UNREACHED
    assert shut["cost"][3, 4] == 15 and shut["cost"][3, 6] == UNREACHED
    check(shut, np_nav(c, [(1, 3)], 1, goals=[(9, 3, 9, 3)], rect=(0, 0, 11, 7)))
    # the unknown beyond the array is a site only under mask 3: the border row then goes too
    assert capi.debug_nav_field(c, [(1, 3)], site_mask=3, clearance=1)["summary"]["n_traversable"] == 2 * 5 * 3 + 2


def test_dir_tie_takes_the_smaller_direction(capi):
    """From (2, 1) the source (4, 2) costs 12 through (3, 1) [d = 0: 5 + 7] and through (3, 2) [d = 1: 7 + 5]: 0 wins."""
    c = np.full((4, 6), 2, np.uint8)
    got = capi.debug_nav_field(c, [(4, 2)])
    assert got["cost"][1, 2] == 12 and got["cost"][1, 3] == 7 and got["cost"][2, 3] == 5 and got["dir"][1, 2] == 0
    assert got["dir"][1, 3] == 1 and got["dir"][2, 3] == 0
    check(got, np_nav(c, [(4, 2)], rect=(0, 0, 6, 4)))


def test_goal_tie_in_row_major_order(capi):
    c = np.full((5, 5), 2, np.uint8)
    got = capi.debug_nav_field(c, [(2, 2)], goals=[(0, 0, 4, 4), (1, 1, 3, 1), (3, 0, 4, 4), (0, 3, 4, 3)])
    assert [tuple(r) for r in got["goals"]] == [(0, 2, 2, 25), (5, 2, 1, 3), (5, 3, 2, 10), (5, 2, 3, 5)]
    corners = capi.debug_nav_field(c, [(2, 2)], goals=[(0, 0, 0, 0), (1, 1, 1, 1)])["goals"]
    assert tuple(corners[0]) == (14, 0, 0, 1) and tuple(corners[1]) == (7, 1, 1, 1)
    ring = c.copy()
    ring[2, 2] = 1                                                         # the four cells at cost 5 around a blocked middle, sources outside
    got = capi.debug_nav_field(ring, [(0, 0), (4, 0), (0, 4), (4, 4)], goals=[(1, 1, 3, 3)])
    assert tuple(got["goals"][0]) == (7, 1, 1, 8)                          # (1, 1), (3, 1), (1, 3), (3, 3) all cost 7: the first in row-major order


def test_goal_outside_the_map(capi):
    c = np.full((5, 5), 2, np.uint8)
    got = capi.debug_nav_field(c, [(2, 2)], goals=[(7, 7, 9, 9), (-9, 0, -1, 4), (-2, -2, 0, 0)], n_paths=2, max_path_cells=4)
    assert [tuple(r) for r in got["goals"]] == [(UNREACHED, 0, 0, 0), (UNREACHED, 0, 0, 0), (14, 0, 0, 1)]
    assert list(got["path_cells"]) == [0, 0] and all(p.shape == (0, 2) for p in got["paths"])
    far = capi.debug_nav_field(c, [(2, 2)], rect=(2**31 - 8, -2**31, 8, 8))
    assert (far["cost"] == UNREACHED).all() and (far["dir"] == 255).all()


def test_path_truncated(capi):
    c = np.full((3, 30), 2, np.uint8)
    got = capi.debug_nav_field(c, [(0, 1)], goals=[(29, 1, 29, 1), (3, 1, 3, 1)], n_paths=2, max_path_cells=10)
    assert list(got["path_cells"]) == [30, 4]
    assert np.array_equal(got["paths"][0], np.stack([np.arange(29, 19, -1), np.ones(10, int)], 1))
    assert np.array_equal(got["paths"][1], [[3, 1], [2, 1], [1, 1], [0, 1]])
    check(got, np_nav(c, [(0, 1)], goals=[(29, 1, 29, 1), (3, 1, 3, 1)], n_paths=2, max_path_cells=10, rect=(0, 0, 30, 3)))


def test_serpentine_corridor(capi):
    w, h = 41, 21
    c = serpentine(w, h)
    got = capi.debug_nav_field(c, [(0, 0)], goals=[(w - 1, h - 1, w - 1, h - 1)], n_paths=1, max_path_cells=1000)
    n = (h + 1) // 2 * w + (h - 1) // 2
    assert n == 461 and list(got["path_cells"]) == [n] and tuple(got["goals"][0]) == (5 * (n - 1), w - 1, h - 1, 1)
    assert got["summary"]["n_reached"] == n == int((c == 2).sum()) and got["summary"]["max_cost_reached"] == 5 * (n - 1)
    p = got["paths"][0]
    assert tuple(p[0]) == (w - 1, h - 1) and tuple(p[-1]) == (0, 0) and (np.abs(np.diff(p, axis=0)).sum(1) == 1).all()
    check(got, np_nav(c, [(0, 0)], goals=[(w - 1, h - 1, w - 1, h - 1)], n_paths=1, max_path_cells=1000, rect=(0, 0, w, h)))
    cut = capi.debug_nav_field(c, [(0, 0)], max_cost=5 * 100)
    assert cut["summary"]["n_reached"] == 101 and cut["summary"]["max_cost_reached"] == 500


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def refusal_cases():
    return [dict(site_mask=1), dict(site_mask=4), dict(site_mask=7), dict(clearance=-1), dict(clearance=255), dict(S=0), dict(S=4097), dict(sources=False),
            dict(G=-1), dict(G=4097), dict(goals=False), dict(results=False), dict(n_paths=-1), dict(n_paths=3), dict(G=70, n_paths=65),
            dict(max_path_cells=0), dict(max_path_cells=65537), dict(G=40, n_paths=33, max_path_cells=32768), dict(n_paths=1, paths=False),
            dict(n_paths=1, cells=False), dict(inverted=(3, 1, 2, 1)), dict(inverted=(1, 3, 1, 2)), dict(rw=0), dict(rh=0), dict(rw=-1),
            dict(rw=4097, rh=4096), dict(rw=0, want_cost=False)]


def refusal_buffers(S=1, G=2, n_paths=0, max_path_cells=4, inverted=None):
    """The arrays of one refused call, the outputs filled with 77."""
    src = np.zeros((4097, 2), np.int32)
    goals = np.zeros((4097, 4), np.int32)
    if inverted:
        goals[min(max(G, 1), 4096) - 1] = inverted
    res = np.full(4097, 77, np.dtype([("cost", np.uint32), ("bx", np.int32), ("by", np.int32), ("n_reached", np.int32)]))
    heads = np.full((65, 2), 77, np.int32)
    cells = np.full(64, 77, np.int32)                                      # (a refused call writes nothing: no need for n_paths * max_path_cells pairs)
    cost = np.full(16, 77, np.uint32); dirs = np.full(16, 77, np.uint8)
    summary = np.full(10, 77, np.int32)
    return src, goals, res, heads, cells, cost, dirs, summary


def refusal_args(bufs, S=1, G=2, n_paths=0, max_path_cells=4, rw=4, rh=4, sources=True, goals=True, results=True, paths=True, cells=True,
                 want_cost=True, want_dir=True, inverted=None):
    p = lambda a, on=True: a.ctypes.data_as(C.c_void_p) if on else None
    src, gl, res, heads, pc, cost, dirs, summary = bufs
    return [p(src, sources), S, p(gl, goals), G, p(res, results), n_paths, max_path_cells, p(heads, paths), p(pc, cells), 0, 0, rw, rh,
            p(cost, want_cost), p(dirs, want_dir), p(summary)]


def untouched(bufs):
    return all((np.frombuffer(b.tobytes(), np.uint8).reshape(-1, b.itemsize)[:, 0] == 77).all() for b in bufs[2:])


@pytest.mark.parametrize("kw", refusal_cases(), ids=lambda kw: ",".join("%s=%s" % i for i in kw.items()).replace(" ", ""))
def test_refusals_leave_the_outputs_untouched(capi, kw):
    lib = capi.lib()
    c = np.full((8, 8), 2, np.uint8)
    spec = dict(site_mask=kw.pop("site_mask", 2), clearance=kw.pop("clearance", 0))
    bufs = refusal_buffers(**{k: v for k, v in kw.items() if k in ("S", "G", "n_paths", "max_path_cells", "inverted")})
    rc = lib.slamhip_debug_nav_field(c.ctypes.data_as(C.c_void_p), 8, 8, spec["site_mask"], spec["clearance"], 0, *refusal_args(bufs, **kw))
    assert rc == capi.ERR_INVALID and lib.slamhip_last_error(), kw
    assert untouched(bufs), kw


def test_refusals_of_the_class_array(capi):
    lib = capi.lib()
    c = np.full((8, 8), 2, np.uint8)
    for cw, ch in ((0, 8), (8, 0), (-1, 8), (1 << 13, (1 << 12) + 1)):
        bufs = refusal_buffers()
        assert lib.slamhip_debug_nav_field(c.ctypes.data_as(C.c_void_p), cw, ch, 2, 0, 0, *refusal_args(bufs)) == capi.ERR_INVALID
        assert untouched(bufs)
    bufs = refusal_buffers()
    assert lib.slamhip_debug_nav_field(c.ctypes.data_as(C.c_void_p), 8, 8, 2, 0, 0, *refusal_args(bufs)) == 0 and not untouched(bufs)   # the call itself is fine
    ok = capi.debug_nav_field(c, [(0, 0)], goals=np.zeros((0, 4)), rect=None)                     # no goals, no rectangle
    assert ok["summary"]["n_reached"] == 64 and ok["goals"].shape == (0,) and "cost" not in ok
