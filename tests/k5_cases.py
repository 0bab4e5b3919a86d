"""Case builders for the K5 (Hector grid update) edge tests: tests/test_k5_cases_cpu.py checks every case on the CPU (both oracles,
the kernel's rule restated in NumPy, and the property the case claims to exercise), tests/test_gpu_grid_update_edges.py runs them on
the device.

A case is one pyramid and a short sequence of steps: `build()` returns Built(cell_len, (w, h), levels, start, steps, factors).
`start` is None or one CELL array per level (uploaded with SetCells, which moves the level's current update index past every
uploaded index: index_after_upload); a step is a scan (xy, origin, pose) or one of ("reset",),
("set_cells", [cells per level]), ("shift", dx, dy); `factors` is None or (free, occupied).  All cases use cell_len = 1 on level 0,
the pose (bx, by, 0) and integer or half-integer points: a point (X, Y) ends in cell rint(X + bx), rint(Y + by) of level 0 by
construction, and `geometry()` restates begin and end cells per level with the reference's own operations -- the float32
transform of OccGridMap.cs:120-134 at angle 0 and ToRoundPoint's banker's rounding -- without touching an oracle or the device.

`touches(g)` lists the cells the lines of one level draw, by the closed form of Bresenham2D (OccGridMap.cs:220-239; pinned against
the literal loop by tests/test_closed_forms.py): the claims and the CPU restatement of the kernel's rule go by it.
"""
import collections

import numpy as np

F = np.float32
INT_MAX = 2 ** 31 - 1
INT_MIN = -(2 ** 31)
CELL = np.dtype([("update_index", np.int32), ("value", np.float32)])
ZONE = 16                              # K5_ZONE (csrc/hs_update.hip)
NBUCK = 1024                           # RS_NBUCK (csrc/raster.h)
LDS_LINES = 3072                       # K5_LDS_LINES (csrc/hs_internal.h)

Case = collections.namedtuple("Case", "name build claims")
Built = collections.namedtuple("Built", "cell_len size levels start steps factors")
Level = collections.namedtuple("Level", "w h bx by inside ex ey valid da sdb major_x smaj cls")
CASES = []


def case(name, *claims):
    def deco(fn):
        CASES.append(Case(name, fn, claims))
        return fn
    return deco


def by_name(name):
    return next(c for c in CASES if c.name == name)


def scan(deltas, pose, origin=(0.0, 0.0)):
    xy = np.array(deltas, np.float64).reshape(-1, 2).astype(np.float32)
    return (xy, (float(origin[0]), float(origin[1])), (float(pose[0]), float(pose[1]), 0.0))


def is_scan(step):
    return not isinstance(step[0], str)


def level_dims(size, levels):
    return [(size[0] >> l, size[1] >> l) for l in range(levels)]       # MapRepMultiMap.cs:40-58


def random_cells(size, levels, seed):
    """Per level: values around zero with a few at and beyond the 50 of :211, indices mostly -1 and a few that an early update's
    marks equal."""
    rng = np.random.default_rng(seed)
    out = []
    for w, h in level_dims(size, levels):
        c = np.empty(w * h, CELL)
        c["value"] = rng.normal(0, 2, w * h).astype(np.float32)
        c["value"][rng.random(w * h) < 0.02] = rng.choice(np.array([50.0, 49.99, 51.0, -0.0], np.float32), 1)[0]
        c["update_index"] = rng.choice(np.array([-1, -1, -1, -1, 0, 1, 2, 4, 5], np.int32), w * h)
        out.append(c)
    return out


def index_after_upload(cells, cur):
    """The level's current update index after an upload (slamhip_hs_cells_upload; the reference has no upload): the next scan's
    marks cur + 1, cur + 2 must exceed every stored index -- where marks can: an index near INT_MAX moves nothing."""
    mx = int(cells["update_index"].max())
    need = (mx // 3 + 1) * 3
    return need if mx >= 0 and need <= INT_MAX - 2 and need > cur else cur


def shifted(cells, w, h, dx, dy):
    """slamhip_hs_shift on one level: new cell (x, y) holds what old cell (x + dx, y + dy) held, exposed cells are reset."""
    out = np.empty(w * h, CELL)
    out["update_index"] = -1
    out["value"] = 0
    src, dst = cells.reshape(h, w), out.reshape(h, w)
    x0, x1, y0, y1 = max(0, -dx), min(w, w - dx), max(0, -dy), min(h, h - dy)
    if x0 < x1 and y0 < y1:
        dst[y0:y1, x0:x1] = src[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


# ---- what the numbers of a case imply ----------------------------------------------------------------------------------------
def _f2i(a):
    a = np.asarray(a, np.float32)
    bad = ~np.isfinite(a) | (a >= F(2147483648.0)) | (a <= F(-2147483904.0))
    out = np.where(bad, 0, a).astype(np.int64)
    out[bad] = INT_MIN
    return out


def _round(a, rounding):
    return np.rint(a) if rounding == "rint" else np.floor(a + F(0.5))  # ("floor": the wrong copy the rounding cases must catch)


def transformed(cell_len, l, pose, x, y):
    """rotation(0) * translation(pose) * scale(1 / cell length of level l) applied to (x, y), in float32 (Matrix3x2 row vectors)."""
    assert pose[2] == 0.0
    cell = F(cell_len)
    for _ in range(l):
        cell = F(cell * F(2.0))
    stm = F(F(1.0) / cell)
    m11, m21, m12, m22 = stm, F(0.0), F(0.0), stm
    m31 = F(F(F(pose[0]) * stm) + F(F(pose[1]) * F(0.0)))
    m32 = F(F(F(pose[0]) * F(0.0)) + F(F(pose[1]) * stm))
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    with np.errstate(all="ignore"):
        return (x * m11 + y * m21) + m31, (x * m12 + y * m22) + m32


def geometry(built, rounding="rint"):
    """Per step None (not a scan) or one Level per pyramid level: begin cell, and per point the end cell, validity (:137, :158-161),
    major length da, signed minor length sdb, major axis and its sign, direction class (0 E, 1 W: x major; 2 S, 3 N: y major;
    -1 invalid)."""
    out = []
    for step in built.steps:
        if not is_scan(step):
            out.append(None)
            continue
        xy, origin, pose = step
        lv = []
        for l, (w, h) in enumerate(level_dims(built.size, built.levels)):
            bxf, byf = transformed(built.cell_len, l, pose, F(origin[0]), F(origin[1]))
            bx, by = int(_f2i(_round(bxf, rounding))), int(_f2i(_round(byf, rounding)))
            exf, eyf = transformed(built.cell_len, l, pose, xy[:, 0], xy[:, 1])
            ex, ey = _f2i(_round(exf, rounding)), _f2i(_round(eyf, rounding))
            inside = 0 <= bx < w and 0 <= by < h
            dx, dy = ex - bx, ey - by
            valid = ((dx != 0) | (dy != 0)) & (ex >= 0) & (ex < w) & (ey >= 0) & (ey < h) & inside
            adx, ady = np.abs(dx), np.abs(dy)
            major_x = adx >= ady                                       # :175
            da = np.where(valid, np.where(major_x, adx, ady), 0)
            sdb = np.where(valid, np.where(major_x, dy, dx), 0)
            smaj = np.where(valid, np.sign(np.where(major_x, dx, dy)), 0)
            cls = np.where(valid, np.where(major_x, np.where(smaj >= 0, 0, 1), np.where(smaj >= 0, 2, 3)), -1)
            lv.append(Level(w, h, bx, by, inside, ex, ey, valid, da, sdb, major_x, smaj, cls))
        out.append(lv)
    return out


def minor_steps(da, db, a):
    """Minor offset after `a` steps of a line (da, db >= 0): floor((da / 2 + a * db) / da), :228-235 in closed form."""
    return (da // 2 + a * db) // da


def touches(g, variant=None):
    """The cells one level's lines draw: (free cells, their line indices, end cells, their line indices), lines in scan order.
    variant: None, or a deliberately wrong copy -- "no_half" (e = a * db), "end_free" (a <= da counts as free: the end cell is one
    more free cell), "zone_diag" (inside the zone a diagonal cell asks its x-major class only)."""
    v = np.flatnonzero(g.valid)
    da, sdb = g.da[v], g.sdb[v]
    n = int(da.sum())
    line = np.repeat(np.arange(v.size), da)
    a = np.arange(n, dtype=np.int64) - np.repeat(np.cumsum(da) - da, da)
    DA, DB = da[line], np.abs(sdb)[line]
    m = (a * DB + (0 if variant == "no_half" else DA // 2)) // DA
    minor, major, mx = np.sign(sdb)[line] * m, g.smaj[v][line] * a, g.major_x[v][line]
    dx, dy = np.where(mx, major, minor), np.where(mx, minor, major)
    keep = np.ones(n, bool)
    if variant == "zone_diag":
        keep = ~((np.abs(dx) == np.abs(dy)) & (np.abs(dx) > 0) & (np.abs(dx) < ZONE) & ~mx)
    free_cells, free_lines = ((g.by + dy) * g.w + g.bx + dx)[keep], v[line][keep]
    end_cells, end_lines = g.ey[v] * g.w + g.ex[v], v
    if variant == "end_free":
        return np.concatenate([free_cells, end_cells]), np.concatenate([free_lines, end_lines]), end_cells[:0], end_lines[:0]
    return free_cells, free_lines, end_cells, end_lines


def first_touches(g, variant=None):
    """Per cell of the level the smallest index of a line that crosses it as free and of one that ends in it (INT_MAX: none)."""
    fc, fl, ec, el = touches(g, variant)
    ff = np.full(g.w * g.h, INT_MAX, np.int64)
    fo = np.full(g.w * g.h, INT_MAX, np.int64)
    ff[fc[::-1]] = fl[::-1]                                             # (a repeated index keeps the last value: the smallest line)
    fo[ec[::-1]] = el[::-1]
    return ff, fo


KINDS = ("free", "hit", "free_hit", "hit_free")


def kinds(g):
    """Per cell: -1 untouched, else the index into KINDS -- crossed only, ended in only, crossed before / after the first end."""
    ff, fo = first_touches(g)
    k = np.full(g.w * g.h, -1, np.int64)
    k[(ff != INT_MAX) & (fo == INT_MAX)] = 0
    k[(ff == INT_MAX) & (fo != INT_MAX)] = 1
    k[(ff != INT_MAX) & (fo != INT_MAX) & (ff < fo)] = 2
    k[(ff != INT_MAX) & (fo != INT_MAX) & (ff >= fo)] = 3
    return k


def cheb(g):
    """Chebyshev distance of every cell of the level from the begin cell."""
    y, x = np.divmod(np.arange(g.w * g.h), g.w)
    return np.maximum(np.abs(x - g.bx), np.abs(y - g.by))


def shared_offsets(g, i, j):
    """Major offsets (>= 1) at which lines i and j of one class draw the same cell (the end cell counts)."""
    assert g.cls[i] == g.cls[j] >= 0
    n = int(min(g.da[i], g.da[j]))
    a = np.arange(1, n + 1, dtype=np.int64)
    mi = np.sign(g.sdb[i]) * minor_steps(int(g.da[i]), abs(int(g.sdb[i])), a)
    mj = np.sign(g.sdb[j]) * minor_steps(int(g.da[j]), abs(int(g.sdb[j])), a)
    return a[mi == mj]


def bucket(sdb, da):
    """rs_bucket of the line's slope (csrc/raster.h), float32."""
    t = F(F(sdb) / F(da))
    return int(min(max(np.floor(F(F(t + F(1.0)) * F(NBUCK // 2))), 0), NBUCK - 1))


# ---- zone and block edges -------------------------------------------------------------------------------------------------------
def star(da, minors=None):
    """Lines of major length da in the 8 octants, on the 4 axes and the 4 diagonals: db in {0, 1, da / 2, da - 1, da}."""
    out = []
    for b in sorted({0, 1, da // 2, da - 1, da} if minors is None else minors):
        if 0 <= b <= da:
            for sx in (1, -1):
                for sy in (1, -1):
                    out += [(sx * da, sy * b), (sx * b, sy * da)]
    return list(dict.fromkeys(out))


EDGE_DAS = {"zone_octants_128": (128, (1, 2, 14, 15, 16, 17)), "block_octants_192": (192, (78, 79, 80, 81)),
            "block_octants_320": (320, (143, 144, 145))}
for _name, (_S, _das) in EDGE_DAS.items():
    def _mk(name=_name, S=_S, das=_das):
        @case(name, "octants:" + ",".join(map(str, das)))
        def _edges():
            """Both sides of the zone's rim and of each block of 64 steps, the end cell on lane 0 and lane 63; two updates."""
            d = [p for da in das for p in star(da)]
            return Built(1.0, (S, S), 1, random_cells((S, S), 1, S), [scan(d, (S // 2, S // 2)), scan(d[::-1], (S // 2, S // 2))], None)
    _mk()


@case("block_thin_320x64", "octants_x:143,144,145")
def _block_thin():
    """x-major lines of 143 .. 145 steps on a map 64 rows high (and y-major ones on its transpose: block_thin_64x320)."""
    d = [(sx * da, sy * b) for da in (143, 144, 145) for b in (0, 1, 30, 31) for sx in (1, -1) for sy in (1, -1)]
    return Built(1.0, (320, 64), 1, random_cells((320, 64), 1, 5), [scan(d, (160, 32))], None)


@case("block_thin_64x320", "octants_x:143,144,145")
def _block_thin_t():
    d = [(sy * b, sx * da) for da in (143, 144, 145) for b in (0, 1, 30, 31) for sx in (1, -1) for sy in (1, -1)]
    return Built(1.0, (64, 320), 1, random_cells((64, 320), 1, 6), [scan(d, (32, 160))], None)


@case("short_then_long", "short_then_long")
def _short_then_long():
    """The longest line is 15: no step lanes run and the sector record is dropped; the next scan has as many points, long lines."""
    short = [p for da in (15, 9, 3) for p in star(da)][:40]
    long_ = [p for da in (100, 40) for p in star(da)][:40]
    s = [scan(short, (120, 120)), scan(long_, (120, 120)), scan(short, (121, 119)), scan(long_, (121, 119))]
    return Built(1.0, (256, 256), 1, random_cells((256, 256), 1, 7), s, None)


_BEGINS = {"sw": (0, 0), "se": (63, 0), "nw": (0, 63), "ne": (63, 63), "s": (30, 0), "n": (30, 63), "w": (0, 30), "e": (63, 30)}
for _where, _b in _BEGINS.items():
    def _mk(where=_where, b=_b):
        @case("begin_%s_64" % where, "begin_on_border")
        def _begin():
            """The begin cell in a corner / on a border: part of the zone lies outside the map, many lines end outside."""
            d = [p for da in (3, 15, 16, 20, 40) for p in star(da)]
            return Built(1.0, (64, 64), 1, random_cells((64, 64), 1, 11 + b[0] + 2 * b[1]), [scan(d, b), scan(d[::-1], b)], None)
    _mk()


@case("begin_outside_64", "begin_outside")
def _begin_outside():
    """The begin cell one cell outside on each side: nothing changes; then the same points from inside."""
    d = [p for da in (3, 16, 40) for p in star(da)]
    s = [scan(d, b) for b in ((-1, 20), (64, 20), (20, -1), (20, 64), (-1, -1), (64, 64))] + [scan(d, (20, 20))]
    return Built(1.0, (64, 64), 1, random_cells((64, 64), 1, 12), s, None)


@case("ends_at_border_64", "ends_at_border")
def _ends_at_border():
    """End points on the last row / column, one past it and far past it, in the eight directions and two oblique ones."""
    d = []
    for ux, uy in ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (1, -1), (-1, 1), (-1, -1)):
        room = min([31 if ux > 0 else 32 if ux < 0 else 99] + [31 if uy > 0 else 32 if uy < 0 else 99])
        for n in (room, room + 1, room + 1000):
            d += [(ux * n, uy * n), (ux * n, uy * 5) if ux else (7, uy * n)]
    return Built(1.0, (64, 64), 1, random_cells((64, 64), 1, 13), [scan(d, (32, 32))], None)


@case("point_is_begin", "point_is_begin", "all_invalid_then_normal")
def _point_is_begin():
    """Points in the begin cell (:137) among others, a scan of nothing else (no valid line), then an ordinary scan of as many."""
    s = [scan([(0, 0), (20, 3), (0, 0), (-4, 1), (0.25, -0.25)], (30, 30)), scan([(0, 0)] * 3, (30, 30)),
         scan([(25, 3), (3, 25), (-17, -2)], (30, 30))]
    return Built(1.0, (64, 64), 1, random_cells((64, 64), 1, 14), s, None)


@case("all_invalid_then_normal", "all_invalid_then_normal")
def _all_invalid():
    """Every end point outside the map (nv == 0: the record is dropped), then a scan of the same count, then both again."""
    out = [(100 + i, i) for i in range(20)] + [(-40 - i, 3) for i in range(20)]
    ok = [p for da in (20, 30) for p in star(da)][:40]
    return Built(1.0, (64, 64), 1, random_cells((64, 64), 1, 15), [scan(ok, (32, 32)), scan(out, (32, 32)), scan(ok, (32, 32)),
                                                                  scan(out, (32, 32)), scan(ok[::-1], (31, 33))], None)


@case("one_point", "one_point")
def _one_point():
    """Scans of a single point: in the zone, beyond it, on the block edge, the same cell again."""
    s = [scan([p], (32, 32)) for p in ((5, 2), (31, -7), (-16, 16), (-17, 3), (5, 2), (0, 0), (31, -7))]
    s += [scan([(80, 1)], (10, 10)), scan([(79, -1)], (10, 10))]
    return Built(1.0, (96, 64), 1, random_cells((96, 64), 1, 16), s, None)


# ---- rounding of ToRoundPoint -----------------------------------------------------------------------------------------------------
def _round_case(axis, side):
    """Along x (axis 0) or y (axis 1), on a map `side` cells long there: end points and begin cells at ties."""
    targets = [-1.5, -0.50001, -0.5, 0.5, 1.5, 2.5, 3.5, side - 2.5, side - 1.5, side - 0.5, side - 0.50001, side + 0.5]
    b = (6, 5)
    d = [(t - b[0], k - 5) for k, t in enumerate(targets)]
    steps = [scan(d, b)]
    for o in (0.5, 1.5, -6.5, -6.50001, side - 6.5, side - 7.5):       # the begin cell at 6.5, 7.5, -0.5, just below, side - 0.5, side - 1.5
        steps.append(scan([(9 - b[0] + o, 4), (o + 0.5, -3)], b, origin=(o, 0)))
    steps.append(scan(d, (6.5, 5)))                                    # a pose at the tie: points at integers land on ties
    steps.append(scan(d, (7.5, 5)))
    size = (side, 12)
    if axis == 1:
        size = (12, side)
        steps = [(xy[:, ::-1].copy(), origin[::-1], (pose[1], pose[0], 0.0)) for xy, origin, pose in steps]
    return Built(1.0, size, 1, random_cells(size, 1, 20 + side + axis), steps, None)


for _axis in (0, 1):
    for _side in (16, 15):
        def _mk(axis=_axis, side=_side):
            @case("round_%s_%d" % ("xy"[axis], side), "rint_ties:%d" % axis)
            def _r():
                return _round_case(axis, side)
        _mk()


# ---- cell state -----------------------------------------------------------------------------------------------------------------
STATE_VALUES = np.array([49.9, np.nextafter(F(50.0), F(0.0)), 50.0, np.nextafter(F(50.0), F(100.0)), 60.0, np.inf, -np.inf, np.nan, -0.0], np.float32)
# three updates: curr = 0, 3, 6, and an uploaded index of -1, curr .. curr + 3 for each of them, INT_MAX -- which no mark can exceed,
# so that the upload leaves curr at 0 (index_after_upload) and the other indices lie at and above the marks of their update
STATE_INDICES = np.array([-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, INT_MAX], np.int32)
STATE_COMBOS = [(v, u) for v in STATE_VALUES for u in STATE_INDICES]
# (and two values that tell the order of the transitions: ((v + lo_free) - lo_free) + lo_occ != v + lo_occ in float32, the first
# with the default factors, the second with 0.3 / 0.8; the values above give the same either way)
STATE_COMBOS += [(F(v), u) for v in (-1.9, -1.8) for u in (-1, 6)]


def ring(r):
    return [(x, y) for y in range(-r, r + 1) for x in range(-r, r + 1) if max(abs(x), abs(y)) == r]


def _state_case(beyond, factors):
    """End points on whole rings around the begin cell, ordered so that each ring's cells are crossed only, ended in only, crossed
    and then ended in, or ended in and then crossed (a fan to the outer ring crosses everything inside it); every (value, index)
    combination is then dealt to the cells of each kind, in the zone (beyond = False) or beyond it."""
    fan, hit_first, hit_last = (30, (20, 24), (26, 22)) if beyond else (15, (10, 12), (13, 11))
    d = [p for r in hit_first for p in ring(r)] + ring(fan) + [p for r in hit_last for p in ring(r)]
    side, b = (64, (32, 32)) if beyond else (41, (20, 20))
    if not beyond:
        d += [(20, 0), (-20, 0), (0, 20), (0, -20)]                    # (the longest line beyond the zone: the step lanes run)
    steps = [scan(d, b)] * 3
    built = Built(1.0, (side, side), 1, None, steps, factors)
    g = geometry(built)[0][0]
    k, c = kinds(g), cheb(g)
    start = np.empty(side * side, CELL)
    start["value"] = 0.25
    start["update_index"] = -1
    for kind in range(4):
        cells = np.flatnonzero((k == kind) & ((c >= ZONE) if beyond else ((c < ZONE) & (c > 0))))
        for j, cell in enumerate(cells):
            start["value"][cell], start["update_index"][cell] = STATE_COMBOS[j % len(STATE_COMBOS)]
    return built._replace(start=[start])


for _beyond in (False, True):
    for _factors in (None, (0.3, 0.8)):
        def _mk(beyond=_beyond, factors=_factors):
            @case("state_%s%s" % ("beyond" if beyond else "zone", "_factors" if factors else ""), "state:%d" % beyond)
            def _s():
                return _state_case(beyond, factors)
        _mk()


# ---- ownership among lines that share cells beyond the zone -------------------------------------------------------------------------
def _fan_built(lines, cls, orders=True, seed=0):
    """Lines (da, signed db) of class E turned into class `cls` (0 E, 1 W, 2 S, 3 N) on the smallest map that holds them; three
    updates: index order, reversed, shuffled."""
    W = max(da for da, _ in lines) + 1
    half = max(abs(db) for _, db in lines) + 1
    H = 2 * half + 1
    turn = {0: lambda a, b: (a, b), 1: lambda a, b: (-a, b), 2: lambda a, b: (b, a), 3: lambda a, b: (b, -a)}[cls]
    begin = {0: (0, half), 1: (W - 1, half), 2: (half, 0), 3: (half, W - 1)}[cls]
    size = (W, H) if cls < 2 else (H, W)
    d = [turn(a, b) for a, b in lines]
    steps = [scan(d, begin)]
    if orders:
        perm = np.random.default_rng(seed + len(lines)).permutation(len(d))
        steps += [scan(d[::-1], begin), scan([d[i] for i in perm], begin)]
    start = random_cells(size, 1, seed + cls) if size[0] * size[1] <= (1 << 20) else None
    return Built(1.0, size, 1, start, steps, None)


FANS = {
    "dup": ([(100, 7)] * 5 + [(32, 5), (64, 10), (96, 15)], ("shares_beyond_zone", "equal_slopes")),
    "unit_2047_n2": ([(2047, 3), (2047, 4)], ("shares_beyond_zone", "gap_at_most:5e-4")),
    "unit_2047_n3": ([(2047, 3), (2047, 4), (2047, 5)], ("shares_beyond_zone", "gap_at_most:5e-4")),
    "unit_2047_n40": ([(2047, k) for k in range(-19, 21)], ("shares_beyond_zone", "gap_at_most:5e-4", "fan_of:40")),
    "gap_da2_small": ([(201, 100), (203, 101)], ("shares_beyond_zone", "gap_at_most:3e-5")),
    "gap_da2_2001": ([(2001, 1000), (2003, 1001)], ("shares_beyond_zone", "gap_at_most:4e-6")),
    "bucket_1": ([(512, 6), (512, 7)], ("shares_beyond_zone", "gap_buckets:1")),
    "rim_11": ([(512, 3), (512, 14), (512, -8)], ("gap_buckets:11",)),
    "rim_12": ([(512, 3), (512, 15), (512, -9)], ("gap_buckets:12",)),
    "rim_13": ([(512, 3), (512, 16), (512, -10)], ("gap_buckets:13",)),
    "far_40": ([(512, 3), (512, 43), (512, -37)], ("gap_buckets:40",)),
    "shortest_first": ([(40, 1), (300, 7), (300, 8), (200, 5), (300, 6), (150, 4)], ("shares_beyond_zone", "owner_ends_first")),
    "sign_pair_300": ([(300, 1), (300, -1)], ("shares_across_sign",)),
    "sign_pair_2047": ([(2047, 1), (2047, -1), (64, 0)], ("shares_across_sign",)),
    "clamp": ([(100, 100), (100, 99), (100, -100), (100, -99), (50, 50), (51, -51)], ("bucket_clamp", "shares_beyond_zone")),
    "end_crossed": ([(16, 3), (32, 6), (79, 10), (158, 20), (80, 10), (160, 20), (500, 60), (1000, 120)], ("end_crossed:16,79,80,500",)),
}
for _name, (_lines, _claims) in FANS.items():
    for _cls in range(2 if _name == "clamp" else 4):                   # (adx == ady is x-major, :175: no y-major line has db = da)
        def _mk(name=_name, lines=_lines, claims=_claims, cls=_cls):
            @case("fan_%s_%s" % (name, "EWSN"[cls]), "fan_class:%d" % cls, *claims)
            def _f():
                return _fan_built(lines, cls, seed=len(name))
        _mk()


for _q, (_sx, _sy) in enumerate(((1, 1), (-1, 1), (1, -1), (-1, -1))):
    def _mk(q=_q, sx=_sx, sy=_sy):
        @case("rim_diag_q%d" % q, "diagonal_meeting")
        def _rim_diag():
            """x-major and y-major lines of one quadrant and the exact diagonal (adx == ady counts as x-major, :175), which meet on
            the diagonal cells, in the zone and beyond it; index order, reversed, shuffled."""
            d = [(100, 100), (100, 99), (99, 100), (100, 100), (60, 60), (59, 60), (60, 59), (99, 98), (98, 99), (17, 16), (16, 17)]
            d = [(sx * x, sy * y) for x, y in d]
            perm = np.random.default_rng(q).permutation(len(d))
            s = [scan(d, (104, 104)), scan(d[::-1], (104, 104)), scan([d[i] for i in perm], (104, 104))]
            return Built(1.0, (208, 208), 1, random_cells((208, 208), 1, 30 + q), s, None)
    _mk()


@case("rim_diag_zone", "zone_diagonal_y_major_only")
def _rim_diag_zone():
    """Diagonal cells of the zone that only a y-major line draws."""
    s = [scan([(14, 15)], (24, 24)), scan([(7, 8), (-8, -9), (-5, 6), (10, -11)], (24, 24)), scan([(-14, -15), (30, 31)], (16, 16))]
    return Built(1.0, (48, 48), 1, random_cells((48, 48), 1, 35), s, None)


# ---- division width ---------------------------------------------------------------------------------------------------------------
DIV_SIZES = ((2048, 2048), (2049, 2049), (2048, 2049), (2049, 2048))


def div_minors(da):
    return sorted({0, 1, da // 3, da // 2, da - 1, da})


def _div_built(size, corner):
    w, h = size
    bx, by = (0 if corner[1] == "w" else w - 1), (0 if corner[0] == "s" else h - 1)
    sx, sy = (1 if bx == 0 else -1), (1 if by == 0 else -1)
    d = [(sx * da, sy * db) for da in range(ZONE, w) for db in div_minors(da) if db <= h - 1]
    d += [(sx * db, sy * da) for da in range(ZONE, h) for db in div_minors(da) if db <= w - 1]
    d = list(dict.fromkeys(d))
    perm = np.random.default_rng(w + 2 * h + bx + by).permutation(len(d))
    d = [d[i] for i in perm]
    steps, p, k = [], 0, 0
    while p < len(d):                                                  # 3072, 3073, 3072, ... points: both table paths
        n = LDS_LINES + (k & 1)
        steps.append(scan(d[p:p + n], (bx, by)))
        p += n; k += 1
    return Built(1.0, size, 1, None, steps, None)


for _size in DIV_SIZES:
    for _corner in ("sw", "se", "nw", "ne"):
        def _mk(size=_size, corner=_corner):
            @case("div_%dx%d_%s" % (size[0], size[1], corner), "division_width")
            def _d():
                """From a corner: every major length from 16 to the side - 1, both major axes, db in {0, 1, da / 3, da / 2, da - 1,
                da}, in scans of 3072 and 3073 points."""
                return _div_built(size, corner)
        _mk()


# ---- long thin maps ---------------------------------------------------------------------------------------------------------------
THIN_DAS = (8190, 8191, 8192, 8193, 32767)
THIN_COARSE = (16380, 16382, 16384, 16386)


def _thin_built(size, levels):
    w, h = size
    xm = w > h
    steps = []
    # (with coarser levels: lines that are 8190 .. 8193 long on level 1 as well)
    for k, da in enumerate(THIN_DAS + (THIN_COARSE if levels > 1 else ())):
        far = k & 1 if k < len(THIN_DAS) else 0                        # (from the map's far end every other time: classes W / N)
        b = ((w - 1 if far else 0), h // 2) if xm else (w // 2, (h - 1 if far else 0))
        s = -1 if far else 1
        for minors in ((1,), (1, 2)):                                  # alone, and with a neighbour one unit of db apart
            d = [(s * da, m) if xm else (m, s * da) for m in minors]
            steps.append(scan(d, b))
    return Built(1.0, size, levels, None, steps, None)


for _size, _levels in (((32768, 8), 1), ((8, 32768), 1), ((32768, 16), 3)):
    def _mk(size=_size, levels=_levels):
        @case("thin_%dx%d_L%d" % (size[0], size[1], levels), "thin")
        def _t():
            """Lines of 8190 .. 8193 and 32767 steps: the 13-bit lone-line field saturates at 8191, a line has up to 512 blocks."""
            return _thin_built(size, levels)
    _mk()


# ---- point counts -----------------------------------------------------------------------------------------------------------------
COUNTS = (1, 2, 3, 5, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 3071, 3072, 3073, 4097)


def _count_built(n):
    rng = np.random.default_rng(n)
    d = rng.integers(-140, 141, (n, 2))
    d[rng.random(n) < 0.05] = 0                                        # (some points in the begin cell)
    steps = [scan(d, (128, 128))]
    for k in sorted({0, n - 1, 1023, 1024}):
        if k < n:
            lone = np.stack([1000 + np.arange(n), np.arange(n) % 7], 1)     # every end point outside the map ...
            lone[k] = (100, 37 + k % 5)                                 # ... but one
            steps.append(scan(lone, (128, 128)))
    return Built(1.0, (256, 256), 1, random_cells((256, 256), 1, n), steps, None)


for _n in COUNTS:
    def _mk(n=_n):
        @case("count_%d" % n, "count:%d" % n)
        def _c():
            """A scan of n points, and scans whose only valid line is at index 0, n - 1, 1023, 1024."""
            return _count_built(n)
    _mk()


@case("count_alternating", "count_alternating")
def _count_alternating():
    """3072- and 3073-point scans in turn on one pyramid: the one-launch form and the two-launch form in turn."""
    rng = np.random.default_rng(99)
    steps = [scan(rng.integers(-120, 121, (LDS_LINES + (k & 1), 2)), (128 + k, 128 - k)) for k in range(6)]
    return Built(1.0, (256, 256), 2, random_cells((256, 256), 2, 98), steps, None)


# ---- sector records -----------------------------------------------------------------------------------------------------------------
SECTOR_COUNTS = (8, 9, 15, 16, 17, 1080)


def _sector_built(n, between=None):
    rng = np.random.default_rng(1000 + n)

    def pts(long_idx):
        d = rng.integers(-9, 10, (n, 2))                                # short lines: inside the zone, no block of steps
        ang = rng.uniform(-np.pi, np.pi, n)
        rad = rng.integers(60, 121, n)
        far = np.stack([np.rint(rad * np.cos(ang)), np.rint(rad * np.sin(ang))], 1).astype(np.int64)
        d[long_idx] = far[long_idx]
        return d
    eighth = max(n // 8, 1)
    layouts = [np.arange(eighth), np.arange(n - eighth, n), np.array([n // 2]), np.arange(n)]
    steps = [scan(pts(ix), (128, 128)) for ix in layouts]
    if between is not None:
        steps = steps[:2] + [between] + steps[2:] + [scan(pts(layouts[0]), (128, 128))]
    return Built(1.0, (256, 256), 2, random_cells((256, 256), 2, n), steps, None)


for _n in SECTOR_COUNTS:
    def _mk(n=_n):
        @case("sector_%d" % n, "sector:%d" % n)
        def _s():
            """A constant point count; the long lines in the first eighth of the indices, the last eighth, one index, everywhere."""
            return _sector_built(n)
    _mk()

for _n in (16, 1080):
    def _mk(n=_n):
        @case("sector_reset_%d" % n, "sector:%d" % n, "op:reset")
        def _a():
            return _sector_built(n, ("reset",))

        @case("sector_set_cells_%d" % n, "sector:%d" % n, "op:set_cells")
        def _b():
            return _sector_built(n, ("set_cells", random_cells((256, 256), 2, 7 * n)))

        @case("sector_shift_%d" % n, "sector:%d" % n, "op:shift")
        def _c():
            return _sector_built(n, ("shift", 8, -4))
    _mk()


# ---- levels -----------------------------------------------------------------------------------------------------------------------
LEVEL_SHAPES = (((256, 256), 1), ((256, 256), 2), ((256, 256), 3), ((256, 256), 5), ((256, 256), 8), ((384, 256), 8),
                ((258, 256), 2), ((258, 256), 3), ((512, 2), 1))


def _levels_built(size, levels):
    w, h = size
    d = [p for da in (1, 2, 3, 15, 16, 17, 31, 32, 33, 64, 100) for p in star(da)]
    b0, b1 = (w // 2 + 1, h // 2 - 1 if h > 2 else 1), (w // 2 - 2, h // 2 + 1 if h > 2 else 0)
    return Built(1.0, size, levels, random_cells(size, levels, w + levels), [scan(d, b0), scan(d[::-1], b1)], None)


for _size, _levels in LEVEL_SHAPES:
    def _mk(size=_size, levels=_levels):
        @case("levels_%dx%d_L%d" % (size[0], size[1], levels), "levels:%d" % levels)
        def _l():
            """Lines valid on level 0 collapse to one cell or into the zone on the coarser levels; the coarsest is 2 x 2 or 3 x 2."""
            return _levels_built(size, levels)
    _mk()
