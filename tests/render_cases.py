"""Case builders for K20 (slamhip_hs_render): tests/test_hs_render_abi.py checks every case on the CPU (the host hook against the C
oracle's sequential update, and against the tile rule restated in NumPy), tests/test_gpu_hector_render.py runs them on the device.

A case is a k5_cases.Built: one pyramid (cell_len = 1 on level 0) and a sequence of scans (xy, origin, pose) with the pose
(bx, by, 0) and integer or half-integer points, so that a point (X, Y) ends in cell rint(X + bx), rint(Y + by) of level 0 by
construction (k5_cases.geometry restates begin and end cells per level).  TILES: the tile sides the kernel is built for.
"""
import math

import numpy as np

import k5_cases as kc

TILES = (32, 64)
CASES = {}
OCTANTS = ((1, 0), (2, 1), (1, 1), (1, 2), (0, 1), (-1, 2), (-1, 1), (-2, 1), (-1, 0), (-2, -1), (-1, -1), (-1, -2), (0, -1), (1, -2), (1, -1), (2, -1))


def case(name):
    def deco(fn):
        CASES[name] = fn
        return fn
    return deco


def built(size, levels, scans, factors=None):
    return kc.Built(1.0, size, levels, None, scans, factors)


def from_to(begin, ends):
    """One scan whose lines run from the cell `begin` to the cells `ends` (level 0)."""
    b = np.array(begin, np.float64)
    return kc.scan(np.array(ends, np.float64).reshape(-1, 2) - b, (b[0], b[1]))


def star(begin, size, lengths=(1, 15, 31, 32, 33, 40, 70)):
    """Lines in all sixteen half-octants from `begin`, of every length of `lengths` that ends inside the map."""
    ends = []
    for dx, dy in OCTANTS:
        for d in lengths:
            k = d / max(abs(dx), abs(dy))
            ex, ey = begin[0] + round(dx * k), begin[1] + round(dy * k)
            if 0 <= ex < size[0] and 0 <= ey < size[1]:
                ends.append((ex, ey))
    return from_to(begin, ends)


def tile_scans(size):
    """Begins on tile corner cells, ends on the last and the first cell of a tile, runs along a tile border on either side,
    diagonals across a tile corner, lines across four tiles -- for both tile sides, whatever lies inside the map."""
    w, h = size
    scans = []
    for b in ((32, 32), (31, 31), (31, 32), (63, 31), (64, 32), (0, 0), (w - 1, h - 1), (w // 2, h // 2)):
        if 0 <= b[0] < w and 0 <= b[1] < h:
            scans.append(star(b, size))
    for y in (31, 32):                                             # along the border between two tile rows, on either side, both ways
        if y < h:
            scans.append(from_to((0, y), [(w - 1, y)]))
            scans.append(from_to((w - 1, y), [(0, y)]))
    for x in (31, 32, 63, 64):
        if x < w:
            scans.append(from_to((x, 0), [(x, h - 1)]))
            scans.append(from_to((x, h - 1), [(x, 0)]))
    if w > 36 and h > 36:                                          # across the corner (31 | 32, 31 | 32) diagonally, all four ways, and a line over four tiles
        scans.append(from_to((29, 29), [(35, 35), (35, 34)]))
        scans.append(from_to((35, 35), [(29, 29), (28, 29)]))
        scans.append(from_to((35, 28), [(28, 35), (29, 35)]))
        scans.append(from_to((28, 35), [(35, 28), (35, 29)]))
        scans.append(from_to((20, 27), [(36, 36), (34, 33)]))
    return scans


for _name, _size, _levels in (("tiles_64", (64, 64), 1), ("tiles_65x63", (65, 63), 1), ("tiles_130x70", (130, 70), 1), ("tiles_256_l3", (256, 256), 3),
                              ("tiles_48x40_l3", (48, 40), 3)):
    CASES[_name] = (lambda s=_size, l=_levels: built(s, l, tile_scans(s)))


@case("thin_2048x16")
def _thin():
    return built((2048, 16), 1, [from_to((0, 8), [(2047, 9), (2047, 8), (2047, 15), (2047, 0)]), from_to((2047, 3), [(0, 4), (0, 3), (0, 15)])])


def _order_scans(X, size=(96, 96)):
    """cross: a line through X; end: a line that ends in X; both: one scan that crosses X with line 0 and ends in it with line 1."""
    x, y = X
    cross = from_to((x - 9, y - 4), [(x + 9, y + 4)])
    end = from_to((x + 7, y - 3), [(x, y)])
    both = from_to((x - 5, y + 5), [(x + 5, y - 5), (x, y)])
    return {"cross": cross, "end": end, "both": both}


for _where, _X in (("mid", (45, 45)), ("border", (31, 32)), ("corner", (32, 32))):
    for _i, _order in enumerate((("cross", "end", "both"), ("cross", "both", "end"), ("end", "cross", "both"), ("end", "both", "cross"),
                                 ("both", "cross", "end"), ("both", "end", "cross"))):
        CASES["across_%s_%d" % (_where, _i)] = (lambda X=_X, o=_order: built((96, 96), 1, [_order_scans(X)[k] for k in o]))
    CASES["across_%s_end_cross" % _where] = (lambda X=_X: built((96, 96), 1, [_order_scans(X)["end"], _order_scans(X)["cross"]]))
    CASES["across_%s_cross_end" % _where] = (lambda X=_X: built((96, 96), 1, [_order_scans(X)["cross"], _order_scans(X)["end"]]))


def _within(X, first):
    """Two scans that cross X (its value is then one at which adding and taking back the free log-odds shows in the bits), then a
    scan of eight lines from one begin cell: line 3 crosses X and line 7 ends in it (first = "cross"), or the reverse."""
    x, y = X
    b = (x - 6, y - 3)
    far, other = (x + 6, y + 3), (x - 6, y + 9)
    ends = [(b[0] - 3, b[1] + k) for k in range(8)]
    if first == "cross":
        ends[3], ends[7] = far, (x, y)
    else:
        ends[3], ends[7] = (x, y), far
    ends[5] = other
    pre = from_to((x - 8, y + 1), [(x + 8, y - 1)])
    return built((96, 96), 1, [pre, pre, from_to(b, ends)])


for _where, _X in (("mid", (45, 45)), ("border", (31, 32)), ("corner", (32, 32)), ("edge64", (63, 64))):
    CASES["within_%s_cross_end" % _where] = (lambda X=_X: _within(X, "cross"))
    CASES["within_%s_end_cross" % _where] = (lambda X=_X: _within(X, "end"))


@case("within_duplicates")
def _dups():
    pre = from_to((37, 46), [(53, 44)])
    return built((96, 96), 1, [pre, pre, from_to((39, 42), [(45, 45), (51, 48), (45, 45), (51, 48), (51, 48), (45, 45)])])


CLAMP_FACTORS = (0.9, 0.9)


def clamp_count(lo_occ):
    """Scans that end in one cell until its value has passed 50: every hit adds lo_occ while the value is below 50."""
    return int(math.ceil(50.0 / lo_occ))


@case("clamp")
def _clamp():
    lo_occ = float(np.log(np.float32(0.9) / (np.float32(1.0) - np.float32(0.9))))
    n = clamp_count(lo_occ) + 2
    return built((64, 64), 1, [from_to((10 + (k % 5), 12), [(40, 33)]) for k in range(n)], CLAMP_FACTORS)


def _random_scan(n, size, seed, begin=(40, 30)):
    rng = np.random.default_rng(seed)
    ends = np.stack([rng.integers(0, size[0], n), rng.integers(0, size[1], n)], 1) if n else np.zeros((0, 2))
    return from_to(begin, ends)


COUNTS = (0, 1, 255, 256, 257, 1080, 3073)


@case("counts")
def _counts():
    size = (130, 70)
    scans = [_random_scan(n, size, 100 + n) for n in COUNTS]
    scans.append(from_to((-5, 30), [(20, 20), (40, 40)]))          # the robot outside the map: every line invalid
    scans.append(from_to((40, 30), [(140, 30), (40, 75), (-3, -3)]))   # every end point outside
    scans.append(from_to((40, 30), [(40, 30), (41, 30), (40, 30)]))    # points equal to the begin cell
    scans.append(_random_scan(64, size, 7, begin=(129, 69)))
    return built(size, 1, scans)


@case("six_scans_l2")
def _six():
    size = (96, 80)
    return built(size, 2, [_random_scan(40 + 7 * k, size, 40 + k, begin=(20 + 9 * k, 17 + 8 * k)) for k in range(6)])


@case("two_scans_l2")
def _two():
    size = (96, 80)
    return built(size, 2, [_random_scan(50, size, 71, begin=(30, 40)), _random_scan(33, size, 72, begin=(70, 20))])


# ---- the end-to-end lap (the lap of tests/test_gpu_hector_pg.py, its helpers restated) ------------------------------------------------
LAP_CELL, LAP_SIZE, LAP_LEVELS = 0.1, (512, 512), 2        # 51.2 m a side: the simulator's field (5 .. 35 m) lies inside
LAP_SIG = (2.0, 32, 1)                                     # the signature spec of tests/test_hs_sig_abi.py's lap
LAP_ODOM_W, LAP_LOOP_W = (400.0, 400.0, 2500.0), (1e4, 1e4, 1e4)
TWO_PI = 6.283185307179586


def _wrap(a):
    return a - TWO_PI * np.rint(a / TWO_PI)


def _rel(pi, pj):
    c, s = np.cos(pi[2]), np.sin(pi[2])
    dx, dy = pj[0] - pi[0], pj[1] - pi[1]
    return np.array([c * dx + s * dy, c * dy - s * dx, _wrap(pj[2] - pi[2])])


def _compose(pi, zz):
    c, s = np.cos(pi[2]), np.sin(pi[2])
    return np.array([pi[0] + c * zz[0] - s * zz[1], pi[1] + s * zz[0] + c * zz[1], pi[2] + zz[2]])


def lap():
    """The simulator's field, a keyframe every metre of one lap (720 rays, no noise); the drifted poses: odometry with a heading
    bias of 0.2 degrees (and 2 mm) per step chained from the first true pose; ONE loop edge, the true relative pose of the first
    keyframe seen from the last.  -> dict(true (N, 3) float32, scans, drifted (N, 3) float32, loop (i, j, z, w))."""
    from slam.net_amd import sim
    segs = sim.default_field()
    true, _ = sim.lap_trajectory(step=1.0)
    scans = [sim.make_scan(segs, p, 720, noise=False)[1] for p in true]
    t64 = true.astype(np.float64)
    N = len(scans)
    drifted = [t64[0]]
    for k in range(N - 1):
        drifted.append(_compose(drifted[-1], _rel(t64[k], t64[k + 1]) + np.array([0.002, 0.0, np.radians(0.2)])))
    drifted = np.stack(drifted)
    drifted[:, 2] = _wrap(drifted[:, 2])
    return dict(true=true.astype(np.float32), scans=scans, drifted=drifted.astype(np.float32), loop=(N - 1, 0, _rel(t64[N - 1], t64[0]), LAP_LOOP_W))


def lap_graph(capi, stored, loop):
    """The graph HectorSLAMProcessor.RelaxKeyframes forms from the store's poses and one loop -> (poses, ij, z, w) for the hook."""
    p0 = np.asarray(stored, np.float32).astype(np.float64)
    N = p0.shape[0]
    ij = [(k, k + 1) for k in range(N - 1)] + [(int(loop[0]), int(loop[1]))]
    z = [capi.pg_edge_between(p0[k], p0[k + 1]) for k in range(N - 1)] + [tuple(float(v) for v in loop[2])]
    w = [LAP_ODOM_W] * (N - 1) + [tuple(loop[3])]
    return p0, np.array(ij, np.int32), np.array(z, np.float64), np.array(w, np.float64)


def lap_hook_render(capi, L, poses):
    dims = kc.level_dims(LAP_SIZE, LAP_LEVELS)
    N = len(L["scans"])
    return capi.debug_render(dims, LAP_CELL, [np.zeros(w * h, kc.CELL) for w, h in dims], [0] * LAP_LEVELS, [0] * LAP_LEVELS, L["scans"],
                             np.zeros((N, 2), np.float32), poses)[0]


def sym_diff(a, b):
    """Cells of level 0 that are occupied (value > 0) in exactly one of two renders."""
    return int(((a["value"] > 0) != (b["value"] > 0)).sum())
