"""Case builders for the K3 (ObstacleMap update) edge tests: tests/test_k3_cases_cpu.py checks every case on the CPU (both oracles,
and the property the case claims to exercise), tests/test_gpu_obstacle_edges.py runs them on the device, stand-alone and riding.

A case is one scan on one map: `build()` returns (size, start_map, xy, pxcs, max_hits).  All cases use c = 1, s = 0,
integer-valued points and px = x1 + 0.5, py = y1 + 0.5: fx = px + X is then exact while |X| < 2^22 or so, and the end cell is
(x1 + X, y1 + Y) by construction -- no trigonometry, no rounding to argue about (but for the truncation of :566-567 towards zero:
an end point at -1 has fx = -0.5, which is cell 0).  For the few larger points (the width-switch cases:
2^30, 2^31) the end cell is what float32 makes of px + X; `geometry()` computes it with the same two float32 operations
(:566-567) and everything below goes by those integers.

`geometry(case)` and `trace(case)` restate what the case's integers imply -- deltas, iteration counts, the cells a literal walk
crosses -- without touching an oracle or the device: the CPU test checks the claims with them.
"""
import collections

import numpy as np

INT_MIN = -(2 ** 31)
F = np.float32

Case = collections.namedtuple("Case", "name build claims")
CASES = []
CUS_ASSUMED = 256                      # the stride of the riding cell pass is 64 * 16 * CUs cells (k2_pixels: one workgroup per CU)


def case(name, *claims):
    def deco(fn):
        CASES.append(Case(name, fn, claims))
        return fn
    return deco


def by_name(name):
    return next(c for c in CASES if c.name == name)


def pxcs_at(x1, y1):
    return np.array([x1 + 0.5, y1 + 0.5, 1.0, 0.0], np.float32)


def random_map(size, seed):
    """Every int8 value, the extremes included."""
    return np.random.default_rng(seed).integers(-128, 128, (size, size)).astype(np.int8)


def pts(deltas):
    return np.array(deltas, np.float64).reshape(-1, 2).astype(np.float32)


# ---- what the integers of a case imply ---------------------------------------------------------------------------------------
def _f2i(f):
    f = float(f)
    if not (f > -2147483904.0 and f < 2147483648.0):
        return INT_MIN
    return int(f)


def _wrap32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v & 0x80000000 else v


def geometry(built):
    """Per ray (x1, y1, x2, y2, ddx, ddy) -- ddx, ddy wrapped to 32 bits as C# does -- or None for the whole scan if the robot is
    outside the map."""
    size, _, xy, pxcs, _ = built
    px, py, c, s = [F(v) for v in pxcs]
    x1, y1 = _f2i(px), _f2i(py)
    if not (0 <= x1 < size and 0 <= y1 < size):
        return None
    out = []
    with np.errstate(all="ignore"):
        for X, Y in np.asarray(xy, np.float32).reshape(-1, 2):
            fx = F(F(px + F(c * X)) - F(s * Y))
            fy = F(F(py + F(s * X)) + F(c * Y))
            x2, y2 = _f2i(fx), _f2i(fy)
            out.append((x1, y1, x2, y2, _wrap32(x2 - x1), _wrap32(y2 - y1)))
    return out


def literal_cells(size, x1, y1, x2, y2):
    """The literal loop (:456-490) in Python integers: (cells crossed as noHit, end cell or None)."""
    ddx, ddy = _wrap32(x2 - x1), _wrap32(y2 - y1)
    if ddx == INT_MIN or ddy == INT_MIN:
        return [], None
    dx, dy = abs(ddx), abs(ddy)
    sx, sy = (ddx > 0) - (ddx < 0), (ddy > 0) - (ddy < 0)
    e = dx if dx > dy else -dy
    err = abs(e) // 2 * (1 if e >= 0 else -1)
    crossed = []
    while True:
        if not (0 <= x1 < size and 0 <= y1 < size):
            return crossed, None
        if x1 == x2 and y1 == y2:
            return crossed, (x1, y1)
        crossed.append((x1, y1))
        e2 = err
        if e2 > -dx:
            err = _wrap32(err - dy); x1 = _wrap32(x1 + sx)
        if e2 < dy:
            err = _wrap32(err + dx); y1 = _wrap32(y1 + sy)


def trace(built):
    """(hits per cell, set of crossed cells, per ray number of in-map iterations) of the whole scan, by the literal loop."""
    size = built[0]
    hits, crossed, inmap = collections.Counter(), set(), []
    for x1, y1, x2, y2, _, _ in geometry(built) or []:
        cr, end = literal_cells(size, x1, y1, x2, y2)
        crossed.update(cr)
        if end is not None:
            hits[end] += 1
        inmap.append(len(cr) + (end is not None))
    return hits, crossed, inmap


def chunks_per_ray(size):
    return (size + 1 + 63) // 64


# ---- walk geometry -------------------------------------------------------------------------------------------------------------
GEOM_SIZES = (8, 63, 64, 65, 127, 128)


def _octant_deltas(a):
    """Major delta a: axis-aligned, the exact diagonal, dx = dy +- 1, a shallow and a steep slope -- in every octant and sign."""
    out = []
    for b in (0, 1, a // 2, a - 1, a):
        for sx in (1, -1):
            for sy in (1, -1):
                out.append((sx * a, sy * b))
                out.append((sx * b, sy * a))
    return out


for _S in GEOM_SIZES:
    def _mk(S=_S):
        @case("octants_%d" % S, "octants", "tie", "odd_even_major")
        def _octants():
            """From the centre: every octant, axes, ties, dx = dy +- 1, an odd and an even major delta."""
            a = S // 2 - 1
            return S, random_map(S, S), pts(_octant_deltas(a) + _octant_deltas(a - 1)), pxcs_at(S // 2, S // 2), 10

        @case("n_values_%d" % S, "n_values", "last_cell")
        def _n_values():
            """From the corner (0, 0): end points at iteration 0, 1, 63, 64, 65, size - 1 (those that fit), along the axis, the
            diagonal and two slopes; the last one of the diagonal is the last cell of the map."""
            d = []
            for n in (0, 1, 63, 64, 65, S - 1):
                if n <= S - 1:
                    d += [(n, 0), (0, n), (n, n), (n, n // 2), (n // 3, n), (n, max(n - 1, 0))]
            return S, random_map(S, S + 1), pts(d), pxcs_at(0, 0), 10

        robots = {"sw": (0, 0), "se": (S - 1, 0), "nw": (0, S - 1), "ne": (S - 1, S - 1),
                  "s": (S // 2, 0), "n": (S // 2, S - 1), "w": (0, S // 2), "e": (S - 1, S // 2)}
        for where, (rx, ry) in robots.items():
            @case("robot_%s_%d" % (where, S), "border_outside")
            def _robot(rx=rx, ry=ry):
                """Robot in a corner / on a border; in each of the eight directions an end point on the last cell inside, one outside
                and far outside: the in-map prefix of the latter two is noHit and nothing else."""
                d = []
                for ux, uy in ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (1, -1), (-1, 1), (-1, -1)):
                    # steps until the walk along (ux, uy) leaves the map
                    room = min([S - 1 - rx if ux > 0 else rx if ux < 0 else S] + [S - 1 - ry if uy > 0 else ry if uy < 0 else S])
                    for n in (room, room + 1, room + 2, room + 1000):       # (towards negative coordinates -0.5 truncates to cell 0: room + 2 is the first one outside there)
                        d.append((ux * n, uy * n))
                    d.append((ux * (room + 1000), uy * (room + 333)))       # far outside, off the diagonal
                    d.append((ux * (room + 2), uy * (room + 1001)))
                return S, random_map(S, 100 + rx * 7 + ry), pts(d), pxcs_at(rx, ry), 10

        for R in (1, 3, 5):
            @case("rays_%d_%d" % (R, S), "idle_wavefronts")
            def _few(R=R):
                """So few rays that the last k3_rays workgroup (4 wavefronts) has idle wavefronts."""
                d = [(S - 2, 1), (-1, S // 2), (S // 3, S // 3), (2, -1), (S, S - 1)][:R]
                return S, random_map(S, 7 * S + R), pts(d), pxcs_at(1, 1), 10
    _mk()


@case("every_cell_16", "every_cell_twice")
def _every_cell():
    """Every cell of a 16^2 map is an end point twice, on a map random over the whole int8 range."""
    x1, y1 = 5, 9
    d = [(x - x1, y - y1) for y in range(16) for x in range(16)] * 2
    return 16, random_map(16, 16), pts(d), pxcs_at(x1, y1), 10


@case("robot_outside_low", "robot_outside")
def _outside_low():
    """px = -1.5 truncates to -1: outside (px = -0.5 would truncate to 0, inside): nothing is drawn, nothing decays."""
    return 16, random_map(16, 3), pts([(3, 3), (20, 1)]), pxcs_at(-2, 4), 10


@case("robot_outside_high", "robot_outside")
def _outside_high():
    return 16, random_map(16, 4), pts([(-3, 3), (-20, 1)]), pxcs_at(5, 16), 10


# ---- width switch: (dx | dy) < 16384 walks in 32-bit arithmetic, everything else in 64-bit ------------------------------------
# (2^31 - 128 is the largest float32 below 2^31; 2^31 - 1, less x1 resp. y1, would make x2 = INT32_MAX but rounds to 2^31 as a
# float32: the end coordinate is int.MinValue and the delta wraps -- the reference's arithmetic, and a walk all the same)
WIDTH_MAJORS = (16383, 16384, 16385, 2 ** 20, 2 ** 30, 2 ** 31 - 128, 2 ** 31 - 1)


def _width_minors(major):
    return sorted(m for m in {0, 200, major // 2, major - 1, major, 8191, 8192, 8193} if m <= major)


def _delta(u, mag, c0):
    """The point coordinate that makes the end cell's delta u * mag from cell c0 (a negative end coordinate truncates towards
    zero, :566-567: one more)."""
    return u * mag - (1 if c0 + u * mag < 0 and mag < 2 ** 22 else 0)


def _width_deltas(majors, ux, uy, x1, y1):
    d = []
    for M in majors:
        for m in _width_minors(M):
            d.append((_delta(ux, M - (x1 if M == 2 ** 31 - 1 else 0), x1), _delta(uy, m, y1)))
            d.append((_delta(ux, m, x1), _delta(uy, M - (y1 if M == 2 ** 31 - 1 else 0), y1)))
    return d


for _name, (_x1, _y1, _ux, _uy) in {"pp": (3, 4, 1, 1), "mm": (60, 59, -1, -1), "pm": (3, 59, 1, -1), "mp": (60, 4, -1, 1)}.items():
    def _mk(name=_name, x1=_x1, y1=_y1, ux=_ux, uy=_uy):
        @case("width_%s" % name, "width_both_paths", "minor_step_64bit")
        def _width():
            """Major deltas either side of 16384 and far above, minor deltas from 0 to the major one, signs by the robot's corner."""
            return 64, random_map(64, 64 + x1), pts(_width_deltas(WIDTH_MAJORS, ux, uy, x1, y1)), pxcs_at(x1, y1), 10

        @case("width_twin_%s" % name, "width_32bit_only")
        def _twin():
            """The same minor deltas with every major delta at 16383: all of it on the 32-bit path."""
            d = []
            for M in WIDTH_MAJORS:
                for m in _width_minors(M):
                    m = min(m, 16383)
                    d += [(_delta(ux, 16383, x1), _delta(uy, m, y1)), (_delta(ux, m, x1), _delta(uy, 16383, y1))]
            return 64, random_map(64, 64 + x1), pts(d), pxcs_at(x1, y1), 10
    _mk()


_GARBAGE = [(1e30, 5.0), (-3e9, 2.0), (np.nan, 1.0), (np.inf, 0.0), (-np.inf, 0.0), (5.0, np.nan), (7.0, 1e30), (3.0, -np.inf),
            (2147483648.0, 3.0), (-2147483648.0, 3.0), (6.0, 5.0)]


@case("int_min_refused", "int_min_delta")
def _int_min():
    """Robot in column / row 0: an end coordinate of int.MinValue (NaN, inf, out of range) gives a delta of int.MinValue, whose
    Math.Abs throws in the reference (deviation D2: the ray is skipped)."""
    return 64, random_map(64, 5), np.array(_GARBAGE, np.float32), pxcs_at(0, 0), 10


@case("int_min_wraps", "int_min_wrapped_delta")
def _int_min_wraps():
    """The same points from (3, 4): int.MinValue - 3 wraps to a large POSITIVE delta, and the ray is walked up and right."""
    return 64, random_map(64, 6), np.array(_GARBAGE, np.float32), pxcs_at(3, 4), 10


# ---- saturation ---------------------------------------------------------------------------------------------------------------
SAT_MAX = (0, 1, 10, 127, -3)


def _sat_case(max_hits):
    size, x1, y1 = 16, 2, 2
    start = random_map(size, 40 + max_hits)
    vals = sorted({v for v in (max_hits - 1, max_hits, max_hits + 1, 127, -128, 0, 1, -1) if -128 <= v <= 127})
    targets = [(v, h) for v in vals for h in (1, 2, 40)] + [(max_hits - 1, 300), (-128, 300), (max_hits, 300)]
    cells = [(x, y) for y in range(5, 16) for x in range(5, 16) if (x + y) % 2 == 0]     # (a chequerboard far corner: rays to one target cross others)
    d = []
    for (v, h), (x, y) in zip(targets, cells):
        start[y, x] = v
        d += [(x - x1, y - y1)] * h
    assert len(targets) <= len(cells)
    # decay at the extremes: the two cells next to the robot, crossed by every ray that starts that way
    start[y1, x1 + 1] = 127
    start[y1 + 1, x1] = -128
    start[y1 + 1, x1 + 1] = 0
    d += [(9, 0), (0, 9), (13, 1), (1, 13)]
    return size, start, pts(d), pxcs_at(x1, y1), max_hits


for _m in SAT_MAX:
    def _mk(m=_m):
        @case("saturation_max_%d" % m, "saturation")
        def _sat():
            """Start cells at Max - 1, Max, Max + 1, 127, -128, 0, +-1, each hit 1, 2, 40 times (three of them 300 times); rays to
            one target cross others (hit and crossed in one scan); cells at 127 and -128 decay."""
            return _sat_case(m)
    _mk()


# ---- ObstacleMaps of more cells than one stride of the riding cell pass -------------------------------------------------------
def big_sizes(cus=CUS_ASSUMED):
    """Three sides whose squares exceed 64 * 16 * cus cells: 513, 520 and 1024 on 256 CUs."""
    import math
    side = math.isqrt(64 * 16 * cus) + 1
    return (max(513, side), max(520, side + 7), max(1024, 2 * (side - 1)))


def big_case(size, seed=0):
    """Robot in the last rows; end points and crossed cells there (the cells a second and later stride own) and a few long rays back
    over the whole map."""
    rng = np.random.default_rng(1000 + size + seed)
    x1, y1 = size - 9 - seed, size - 2
    d = [(int(rng.integers(-60, 9)), int(rng.integers(-2, 2))) for _ in range(150)]
    d += [(int(rng.integers(-size, 0)), int(rng.integers(-size, 0))) for _ in range(40)]
    d += [(-x1, 1), (8 + seed, 1), (0, 0), (-x1, -y1), (3, 2), (-200, 1)] + [(-7, 1)] * 50
    return size, random_map(size, size + seed), pts(d), pxcs_at(x1, y1), 10


for _i in range(3):
    def _mk(i=_i):
        @case("big_%d" % big_sizes()[i], "beyond_first_stride")
        def _big():
            return big_case(big_sizes()[i])
    _mk()
