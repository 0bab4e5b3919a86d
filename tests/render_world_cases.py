"""Case builders for K25 (slamhip_hs_render_world) and an independent NumPy restatement of its definition:
tests/test_hs_render_world_abi.py holds the host hook (slamhip_debug_render_world) to the restatement on the CPU,
tests/test_gpu_hector_render_world.py holds the device to the hook.

A case is a WCase: a window of WIN cells x LEVELS levels at CELL_LEN, first shifted by `shift` level-0 cells; scans (xy, origin, pose)
with poses (bx, by, 0) and points on whole level-0 cells, all in the window's frame AFTER the shift; `calls`, the renders in order as
(first, last, keep); RECT, the level-0 rectangle in window-frame cells every scan's box stays inside (level l: every number >> l).

The restatement keeps the world the way the library stores it -- the window's arrays and a dict of tiles of T x T cells, routed per
cell, the window winning when the world is read -- on an unbounded integer grid, with its own Bresenham walk and its own
transitions.  `variant` names a deliberately wrong copy; each must fail some case."""
import collections
import math

import numpy as np

import k5_cases as kc

F = np.float32
INF = 0x7fffffff
CELL_LEN, WIN, LEVELS = 0.125, (64, 64), 2
TILES = (8, 16, 32)
RECT = (-96, -96, 288, 288)
WCase = collections.namedtuple("WCase", "shift scans calls factors")
CASES = {}
VARIANTS = ("trunc", "window_clip", "free_on_end", "tile_under_window", "empty_no_advance")


def case(name):
    def deco(fn):
        CASES[name] = fn
        return fn
    return deco


def rect_of(level):
    return tuple(v >> level for v in RECT)


def from_to(begin, ends):
    """One scan whose lines run from the level-0 cell `begin` to the cells `ends` (window frame)."""
    b = np.array(begin, np.float64)
    e = np.array(ends, np.float64).reshape(-1, 2)
    return ((e - b) * CELL_LEN).astype(np.float32), (0.0, 0.0), (float(b[0] * CELL_LEN), float(b[1] * CELL_LEN), 0.0)


def rand_scan(seed, begin, lo, hi, n=64):
    rng = np.random.default_rng(seed)
    return from_to(begin, rng.integers(lo, hi + 1, (n, 2)))


def whole(scans, shift=(0, 0), factors=None):
    return WCase(shift, scans, [(0, len(scans), False)], factors)


@case("inside")
def _inside():
    return whole([rand_scan(10 + k, (12 + 7 * k, 50 - 6 * k), 1, 62) for k in range(6)])


@case("ends_outside")
def _ends_outside():
    return whole([rand_scan(20 + k, (8 + 9 * k, 20 + 5 * k), -60, 150, 90) for k in range(6)])


@case("begin_outside")
def _begin_outside():
    return whole([rand_scan(30 + k, b, -40, 110) for k, b in enumerate(((-20, 30), (70, 10), (30, 90), (-9, -9), (64, 64), (-1, 0)))])


@case("wholly_outside")
def _wholly_outside():
    return whole([rand_scan(40, (30, 30), 2, 60), rand_scan(41, (100, 100), 80, 125), rand_scan(42, (-50, 100), -80, -20), rand_scan(43, (100, -40), 70, 130),
                  rand_scan(44, (101, 99), 80, 125), rand_scan(45, (31, 33), 2, 60)])


@case("negative")
def _negative():
    # odd negative cells: on level 1 they lie at -k.5, where rintf (ties to even) and a truncation part
    return whole([rand_scan(50 + k, (-31 - 4 * k, -25 - 2 * k), -79, 9) for k in range(5)] + [from_to((-7, -5), [(-15, -9), (-3, -1), (-33, -7), (-7, -45)])])


@case("tile_edges")
def _tile_edges():
    along = [from_to((-40, y), [(100, y)]) for y in (31, 32, 63, 64, -1, 0)] + [from_to((x, 100), [(x, -40)]) for x in (31, 32, 63, 64, -1, 0)]
    corner = [from_to((70, 70), [(95, 95), (96, 96), (64, 64), (63, 63)]), from_to((-20, -20), [(-1, -1), (-32, -32), (-33, -33), (0, 0), (-8, -16)])]
    return whole(along[:4] + corner + along[4:])


@case("origin_off_tile")
def _origin_off_tile():
    # (4, 6): no multiple of any tile side on level 0, (2, 3) on level 1 -- render blocks straddle the window's edge
    return whole([rand_scan(60 + k, (10 + 8 * k, 56 - 9 * k), -50, 120, 80) for k in range(6)] + [from_to((-3, -3), [(3, 3), (70, 70), (-3, 70)])], shift=(4, 6))


@case("empty_scan")
def _empty_scan():
    s = [rand_scan(70 + k, (20 + 5 * k, 70 - 9 * k), -30, 100) for k in range(6)]
    s.insert(2, from_to((10, 10), np.zeros((0, 2))))
    s.append(from_to((70, 70), np.zeros((0, 2))))
    return whole(s)


CLAMP_FACTORS = (0.9, 0.9)


@case("clamp_outside")
def _clamp():
    """Scans that end in one cell OUTSIDE the window until its value has passed 50: the occupied transition then stops adding."""
    lo_occ = float(np.log(np.float32(0.9) / (np.float32(1.0) - np.float32(0.9))))
    n = int(math.ceil(50.0 / lo_occ)) + 2
    return whole([from_to((50 + (k % 5), 40), [(90, 77)]) for k in range(n)], factors=CLAMP_FACTORS)


CLAMP_CELL = (90, 77)


@case("same_end_twice")
def _same_end():
    return whole([from_to((20, 20), [(80, 33), (70, 90)]), from_to((40, 10), [(80, 33), (-10, 20)]), from_to((81, 30), [(79, 36)]), from_to((10, 50), [(80, 33)]),
                  rand_scan(81, (60, 60), 40, 100), rand_scan(82, (75, 30), 60, 100)])


@case("free_after_end")
def _free_after_end():
    """A cell X outside the window that line 3 of a scan ends in and line 7 of the same scan crosses, after two scans have crossed
    it (its value is then one at which adding and taking back the free log-odds shows in the bits): the occupied transition alone."""
    x, y = 85, 45
    b = (x - 6, y - 3)
    ends = [(b[0] - 3, b[1] + k) for k in range(8)]
    ends[3], ends[7], ends[5] = (x, y), (x + 6, y + 3), (x - 6, y + 9)
    pre = from_to((x - 8, y + 1), [(x + 8, y - 1)])
    return whole([pre, pre, from_to(b, ends), rand_scan(85, (70, 40), 50, 110), rand_scan(86, (30, 30), 5, 100), rand_scan(87, (90, 50), 60, 110)])


@case("keep_existing")
def _keep_existing():
    s = [rand_scan(90 + k, (15 + 6 * k, 25 + 4 * k), -40, 120) for k in range(10)]
    return WCase((0, 0), s, [(0, 5, False), (5, 10, True)], None)


@case("keep_missing_tile")
def _keep_missing():
    s = [rand_scan(100 + k, (30, 30), 5, 80) for k in range(4)] + [rand_scan(110 + k, (120, 130), 100, 170) for k in range(2)] + \
        [rand_scan(120 + k, (-30, 100), -80, 20) for k in range(2)]
    return WCase((0, 0), s, [(0, 4, False), (4, 8, True)], None)


@case("empty_range_keep")
def _empty_keep():
    s = [rand_scan(130 + k, (20 + 5 * k, 40), -30, 100) for k in range(6)]
    return WCase((0, 0), s, [(0, 6, False), (3, 3, True)], None)


@case("empty_range_clear")
def _empty_clear():
    s = [rand_scan(130 + k, (20 + 5 * k, 40), -30, 100) for k in range(6)]
    return WCase((0, 0), s, [(0, 6, False), (3, 3, False)], None)


@case("sub_range_off_tile")
def _sub_range():
    s = [rand_scan(140 + k, (6 + 9 * k, 60 - 8 * k), -45, 115, 72) for k in range(8)]
    return WCase((-6, 10), s, [(2, 7, False), (0, 2, True)], None)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def floor_div(a, b):
    return a // b                                                   # (Python: floor for negative a too)


def cells_of(scan, level, variant=None):
    """Begin cell and end cells of one scan on one level: rotation(0) * translation * scale in float32, then rintf."""
    xy, origin, pose = scan
    rnd = np.trunc if variant == "trunc" else np.rint
    bxf, byf = kc.transformed(CELL_LEN, level, pose, F(origin[0]), F(origin[1]))
    exf, eyf = kc.transformed(CELL_LEN, level, pose, xy[:, 0], xy[:, 1])
    return int(rnd(bxf)), int(rnd(byf)), rnd(exf).astype(np.int64), rnd(eyf).astype(np.int64)


def walk(bx, by, ex, ey):
    """Bresenham2D (OccGridMap.cs:220-239) from the begin cell: the da cells in front of the end cell."""
    dx, dy = ex - bx, ey - by
    adx, ady = abs(dx), abs(dy)
    sx, sy = (dx > 0) - (dx < 0), (dy > 0) - (dy < 0)
    out = []
    x, y = bx, by
    if adx >= ady:
        err = adx // 2
        for _ in range(adx):
            out.append((x, y))
            x += sx; err += ady
            if err >= adx:
                y += sy; err -= adx
    else:
        err = ady // 2
        for _ in range(ady):
            out.append((x, y))
            y += sy; err += adx
            if err >= ady:
                x += sx; err -= ady
    assert (x, y) == (ex, ey)
    return out


class World:
    """The window's arrays and the tiles, as the library stores them; T the tile side, (ox, oy) the window's origin."""

    def __init__(self, T, origin, variant=None):
        self.T, self.origin, self.variant = T, origin, variant
        self.dims = kc.level_dims(WIN, LEVELS)
        self.ui, self.ci = [0] * LEVELS, [0] * LEVELS
        self.clear()

    def clear(self):
        self.win = [{} for _ in range(LEVELS)]                      # (x, y) -> (index, value); absent: Reset
        self.tiles = {}                                             # (level, ty, tx) -> {(lx, ly): (index, value)}

    def route(self, l, x, y):
        """-> the dict and the key the cell lives under."""
        w, h = self.dims[l]
        T = self.T
        X, Y = (self.origin[0] >> l) + x, (self.origin[1] >> l) + y
        tx, ty = floor_div(X, T), floor_div(Y, T)
        in_window = 0 <= x < w and 0 <= y < h
        if self.variant == "tile_under_window" and in_window:
            # the wrong copy: a cell goes to the window only where its whole tile lies under the window
            x0, y0 = tx * T - (self.origin[0] >> l), ty * T - (self.origin[1] >> l)
            in_window = x0 >= 0 and y0 >= 0 and x0 + T <= w and y0 + T <= h
        if in_window:
            return self.win[l], (x, y)
        return self.tiles.setdefault((l, ty, tx), {}), (X - tx * T, Y - ty * T)

    def get(self, l, x, y):
        """The world as it is read: the window wins."""
        w, h = self.dims[l]
        if 0 <= x < w and 0 <= y < h:
            return self.win[l].get((x, y), (-1, F(0.0)))
        T = self.T
        X, Y = (self.origin[0] >> l) + x, (self.origin[1] >> l) + y
        tx, ty = floor_div(X, T), floor_div(Y, T)
        return self.tiles.get((l, ty, tx), {}).get((X - tx * T, Y - ty * T), (-1, F(0.0)))

    def rect(self, l):
        x0, y0, w, h = rect_of(l)
        out = np.zeros((h, w), kc.CELL)
        out["update_index"] = -1
        for y in range(h):
            for x in range(w):
                u, v = self.get(l, x0 + x, y0 + y)
                if u != -1 or v != 0:
                    out[y, x] = (u, v)
        return out.reshape(-1)


def restate(c, T, lo_free, lo_occ, variant=None):
    """The case by the definition -> (cells of RECT per level, update indices, cache epochs, the World)."""
    W = World(T, c.shift, variant)
    lo_free, lo_occ = F(lo_free), F(lo_occ)
    w0, h0 = WIN
    for first, last, keep in c.calls:
        if not keep:
            W.clear()
            W.ui, W.ci = [0] * LEVELS, [0] * LEVELS
        for k in range(first, last):
            for l in range(LEVELS):
                w, h = W.dims[l]
                bx, by, ex, ey = cells_of(c.scans[k], l, variant)
                ff, fo = {}, {}
                for i in range(ex.size):
                    e = (int(ex[i]), int(ey[i]))
                    if e == (bx, by):
                        continue
                    if variant == "window_clip" and not (0 <= bx < w and 0 <= by < h and 0 <= e[0] < w and 0 <= e[1] < h):
                        continue
                    for cell in walk(bx, by, e[0], e[1]):
                        ff.setdefault(cell, i)
                    fo.setdefault(e, i)
                mark_free, mark_occ = W.ui[l] + 1, W.ui[l] + 2
                for cell in set(ff) | set(fo):
                    f0, o0 = ff.get(cell, INF), fo.get(cell, INF)
                    store, key = W.route(l, cell[0], cell[1])
                    u, v = store.get(key, (-1, F(0.0)))
                    free_first = f0 != INF if variant == "free_on_end" else f0 < o0
                    if free_first and u < mark_free:
                        v = F(v + lo_free); u = mark_free
                    if o0 != INF and u < mark_occ:
                        if u == mark_free:
                            v = F(v - lo_free)
                        if v < F(50.0):
                            v = F(v + lo_occ)
                        u = mark_occ
                    store[key] = (u, v)
                if not (variant == "empty_no_advance" and ex.size == 0):
                    W.ui[l] += 3
                    W.ci[l] += 1
    return [W.rect(l) for l in range(LEVELS)], list(W.ui), list(W.ci), W


def hook_calls(capi, c, rects=None):
    """The case through the host hook, call by call -> (cells per level, update indices, cache epochs)."""
    rects = [rect_of(l) for l in range(LEVELS)] if rects is None else rects
    cells = []
    for _, _, w, h in rects:
        a = np.zeros(w * h, kc.CELL)
        a["update_index"] = -1
        cells.append(a)
    ui, ci = [0] * LEVELS, [0] * LEVELS
    for first, last, keep in c.calls:
        s = c.scans[first:last]
        cells, ui, ci = capi.debug_render_world(rects, CELL_LEN, cells, ui, ci, [x[0] for x in s], [x[1] for x in s], [x[2] for x in s], keep=keep,
                                                factors=c.factors or (0.4, 0.9))
    return cells, ui, ci
