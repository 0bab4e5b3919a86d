"""Case builders for K21 (slamhip_hs_scans_match): tests/test_hs_scanmatch_abi.py checks every case on the CPU (the host hook
against a NumPy restatement of rules 1 - 5), tests/test_gpu_hector_scanmatch.py runs them on the device against the hook.

A case is a dict: scans (a list of (n, 2) float32 arrays standing for the scan store), spec (the keyword arguments of
capi.scanmatch_spec), pairs ((ref, query, guess) tuples) and, optionally, headings (SLAMHIP_K21_HEADINGS for the device call: the
headings a workgroup owns).  Unless a case says otherwise the points are small binary fractions, scale is a power of two and every
heading is 0, where the deterministic trigonometry gives c = 1 and s = 0 exactly: a point's cell is floor(p * scale) + H by
construction.  CHUNK and TILE restate the kernel's staging chunk and its translations per tile, whose two sides the sizes straddle.
"""
import math

import numpy as np

F = np.float32
CHUNK = 1024                                                   # K21_CHUNK: query points per LDS chunk
TILE = 256                                                     # translations a workgroup takes at a time
CASES = {}


def case(name):
    def deco(fn):
        CASES[name] = fn
        return fn
    return deco


def spec(scale=1.0, half=16, nx=0, ny=0, nt=0, dtheta=0.0, margin=0):
    return dict(scale=scale, half=half, nx=nx, ny=ny, nt=nt, dtheta=dtheta, margin=margin)


def pts(rows):
    return np.array(rows, np.float32).reshape(-1, 2)


def fractions(n, seed, reach, denom=4):
    """n points on the lattice of 1 / denom inside [-reach, reach)^2, seeded."""
    g = np.random.Generator(np.random.Philox(seed))
    return (g.integers(-reach * denom, reach * denom, size=(n, 2)).astype(np.float32) / F(denom)).astype(np.float32)


def walls(n, seed, reach):
    """n points on the sides of a few boxes inside [-reach, reach]^2, on the lattice of 1 / 4: something a shift can lock onto."""
    g = np.random.Generator(np.random.Philox(seed))
    out = []
    for _ in range(n):
        side = int(g.integers(0, 4)); t = float(g.integers(-reach * 4, reach * 4 + 1)) / 4.0; r = float(reach) * (1.0 if side < 2 else 0.5)
        t = max(min(t, r), -r)
        out.append((t, r) if side == 0 else (r, t) if side == 1 else (t, -r) if side == 2 else (-r, t))
    return pts(out)


@case("one_one")
def _one_one():
    return dict(scans=[pts([(0.5, 0.5)]), pts([(1.5, -0.5)])], spec=spec(nx=2, ny=2, nt=1, dtheta=0.25), pairs=[(0, 1, (0.0, 0.0, 0.0))])


@case("self_pair")
def _self_pair():
    return dict(scans=[walls(60, 3, 6)], spec=spec(scale=2.0, nx=3, ny=3, nt=1, dtheta=0.125, margin=4), pairs=[(0, 0, (0.0, 0.0, 0.0))])


@case("empty_query_and_reference")
def _empty():
    a = walls(20, 4, 5)
    return dict(scans=[a, np.zeros((0, 2), np.float32)], spec=spec(nx=1, ny=2, nt=1, dtheta=0.5, margin=3),
                pairs=[(0, 1, (0.0, 0.0, 0.0)), (1, 0, (0.0, 0.0, 0.0)), (1, 1, (0.0, 0.0, 0.0))])


@case("cell_borders")
def _borders():
    """Points exactly on cell borders and at -0.0; scale 4 puts a border at every quarter.  Negative coordinates tell floor from
    truncation: (-0.25, -0.25) * 4 = -1 exactly, (-0.125, ...) * 4 = -0.5 -> floor -1, truncation 0."""
    ref = pts([(0.0, 0.0), (-0.0, -0.0), (0.25, -0.25), (-0.25, 0.25), (-0.125, -0.125), (-1.0, -1.0), (-1.125, 0.875), (0.75, -0.875)])
    qry = pts([(-0.0, 0.0), (-0.125, -0.125), (-0.25, -0.25), (0.25, 0.25), (-0.625, 0.375), (-1.0, -1.0)])
    return dict(scans=[ref, qry], spec=spec(scale=4.0, nx=2, ny=2, margin=1), pairs=[(0, 1, (0.0, 0.0, 0.0)), (1, 0, (-0.125, 0.125, 0.0))])


def _edge_reference(H):
    """Reference cells 0, 1, 2H - 2 and 2H - 1 on both axes and in the corners, points one cell outside the grid on every side, and
    |f| on both sides of 2^14 (counted in n_ref or ignored), and a NaN."""
    e = [-H + 0.5, -H + 1.5, H - 1.5, H - 0.5]
    ref = [(x, y) for x in e for y in e] + [(x, 0.5) for x in e] + [(0.5, y) for y in e]
    ref += [(-H - 0.5, 0.5), (H + 0.0, 0.5), (0.5, -H - 0.5), (0.5, H + 0.0), (-H - 0.5, -H - 0.5), (H + 0.0, H + 0.0)]
    ref += [(16383.5, 0.5), (16384.0, 0.5), (0.5, -16383.5), (0.5, -16384.0), (float("nan"), 0.5), (0.5, float("nan"))]
    return pts(ref)


@case("reference_edges_H16")
def _ref_edges():
    """The dilation against each border and corner of the grid: the query covers every cell of the grid and a frame of two cells
    round it, so shifts of up to 2 put query cells on -1, -2, 2H and 2H + 1."""
    H = 16
    q = np.arange(-H - 2, H + 2, dtype=np.float32) + F(0.5)
    qry = np.stack(np.meshgrid(q, q), -1).reshape(-1, 2)
    return dict(scans=[_edge_reference(H), qry, pts([(-H + 0.5, 0.5), (H - 0.5, 0.5), (0.5, -H + 0.5), (0.5, H - 0.5)])],
                spec=spec(half=H, nx=2, ny=2, margin=1 << 30), pairs=[(0, 1, (0.0, 0.0, 0.0)), (0, 2, (0.0, 0.0, 0.0)), (0, 2, (1.0, -1.0, 0.0))])


@case("reference_edges_H192")
def _ref_edges_192():
    H = 192
    ref = np.concatenate([_edge_reference(H) / F(8.0), walls(300, 5, 20)])   # (scale 8: the edge points keep their cells; 2^14 / 8 stays exact)
    e = [(-H + 0.5) / 8, (H - 0.5) / 8, 0.0625]
    qry = np.concatenate([pts([(x, y) for x in e for y in e]), walls(200, 6, 20)])
    return dict(scans=[ref, qry], spec=spec(scale=8.0, half=H, nx=4, ny=4, nt=1, dtheta=0.01, margin=8), pairs=[(0, 1, (0.0, 0.0, 0.0)), (0, 1, (0.25, -0.125, 0.0))])


@case("single_node")
def _single():
    a = walls(40, 7, 6)
    return dict(scans=[a, a + F(0.25)], spec=spec(scale=2.0), pairs=[(0, 1, (0.0, 0.0, 0.0)), (0, 1, (-0.25, -0.25, 0.0))])


@case("wide_x")
def _wide_x():
    a = walls(50, 8, 10)
    return dict(scans=[a, a + np.array([3.0, 0.0], np.float32)], spec=spec(half=32, nx=64, ny=0, margin=2), pairs=[(0, 1, (0.0, 0.0, 0.0))])


@case("wide_y")
def _wide_y():
    a = walls(50, 9, 10)
    return dict(scans=[a, a + np.array([0.0, -5.0], np.float32)], spec=spec(half=32, nx=0, ny=64, margin=2), pairs=[(0, 1, (0.0, 0.0, 0.0))])


def _tile_case(nx, ny, seed):
    a = walls(40, seed, 8)
    return dict(scans=[a, a + np.array([1.0, -2.0], np.float32)], spec=spec(half=32, nx=nx, ny=ny, nt=1, dtheta=0.0625, margin=3), pairs=[(0, 1, (0.0, 0.0, 0.0))])


# translations per heading on both sides of one tile and of two: 15 x 17 = 255, 7 x 37 = 259, 7 x 73 = 511, 27 x 19 = 513
@case("tile_255")
def _t255():
    return _tile_case(7, 8, 10)


@case("tile_259")
def _t259():
    return _tile_case(3, 18, 11)


@case("tile_511")
def _t511():
    return _tile_case(3, 36, 12)


@case("tile_513")
def _t513():
    return _tile_case(13, 9, 13)


@case("uneven_heading_blocks")
def _uneven():
    """Seven headings in blocks of three: 3, 3 and 1; generic headings and generic points."""
    g = np.random.Generator(np.random.Philox(14))
    a = (g.standard_normal((80, 2)) * 4.0).astype(np.float32)
    th = 0.11
    c, s = math.cos(th), math.sin(th)
    b = np.stack([c * a[:, 0] + s * a[:, 1] - 0.4, -s * a[:, 0] + c * a[:, 1] + 0.7], 1).astype(np.float32)
    return dict(scans=[a, b], spec=spec(scale=3.0, half=32, nx=4, ny=4, nt=3, dtheta=0.04, margin=5), pairs=[(0, 1, (0.3, -0.6, 0.07)), (1, 0, (0.0, 0.0, -0.1))],
                headings=3)


@case("all_nodes_tie")
def _all_tie():
    """A block of hit cells and one query point in its middle: every node scores 2 and the lowest flat wins; dtheta = 0 makes the five
    headings identical, so the tie runs across heading blocks -- across workgroups."""
    q = np.arange(-6, 6, dtype=np.float32) + F(0.5)
    ref = np.stack(np.meshgrid(q, q), -1).reshape(-1, 2)
    return dict(scans=[ref, pts([(0.5, 0.5)])], spec=spec(nx=2, ny=2, nt=2, dtheta=0.0, margin=0), pairs=[(0, 1, (0.0, 0.0, 0.0))], headings=2)


@case("tie_across_heading_blocks")
def _tie_blocks():
    """The best score is reached at one translation of EVERY heading (dtheta = 0) and nowhere else: the winner is heading -nt, which
    another workgroup than heading 0's finds."""
    a = walls(30, 15, 5)
    return dict(scans=[a, a], spec=spec(nx=3, ny=3, nt=2, dtheta=0.0, margin=0), pairs=[(0, 1, (0.0, 0.0, 0.0))], headings=1)


def _margin_case(margin):
    """129 x 129 nodes over a reference that fills a block: tens of thousands of positive nodes in the 64-bit sums."""
    q = np.arange(-40, 40, dtype=np.float32) + F(0.5)
    ref = np.stack(np.meshgrid(q, q), -1).reshape(-1, 2)[::3]
    return dict(scans=[ref, walls(24, 16, 10)], spec=spec(half=96, nx=64, ny=64, nt=1, dtheta=0.0, margin=margin), pairs=[(0, 1, (0.0, 0.0, 0.0))])


@case("margin_zero")
def _margin_zero():
    return _margin_case(0)


@case("margin_everything")
def _margin_all():
    return _margin_case(0x7fffffff)


def _size_case(nq, seed, nr=64):
    a = walls(nr, seed, 10)
    return dict(scans=[a, fractions(nq, seed + 100, 12)], spec=spec(half=32, nx=2, ny=2, nt=1, dtheta=0.03125, margin=6), pairs=[(0, 1, (0.0, 0.0, 0.0))])


@case("query_1023")
def _q1023():
    return _size_case(CHUNK - 1, 17)


@case("query_1024")
def _q1024():
    return _size_case(CHUNK, 18)


@case("query_1025")
def _q1025():
    """... with more than one tile of translations (17 x 17 = 289), so the chunks are staged again for the second tile."""
    d = _size_case(CHUNK + 1, 19)
    d["spec"].update(nx=8, ny=8)
    return d


@case("scans_2049")
def _s2049():
    return _size_case(2 * CHUNK + 1, 20, nr=2 * CHUNK + 1)


def _store(n_scans, n_points, seed):
    return [walls(n_points, seed + i, 8) + np.array([0.25 * (i % 5), -0.25 * (i % 3)], np.float32) for i in range(n_scans)]


@case("pairs_2")
def _pairs_2():
    return dict(scans=_store(3, 48, 30), spec=spec(half=32, nx=3, ny=3, nt=1, dtheta=0.0625, margin=2), pairs=[(0, 1, (0.0, 0.0, 0.0)), (2, 1, (0.25, 0.0, 0.0))])


@case("pairs_65_one_reference")
def _pairs_65():
    return dict(scans=_store(9, 48, 40), spec=spec(half=32, nx=3, ny=3, nt=1, dtheta=0.0625, margin=2),
                pairs=[(0, 1 + i % 8, (0.25 * (i % 4), -0.25 * (i % 3), 0.0)) for i in range(65)])


# ---- the end-to-end lap: render_cases.lap() with loop edges from the scan-to-scan match alone --------------------------------------------
LAP_SCALE, LAP_HALF = 8.0, 192                                 # cells of 0.125 m; the raster reaches 24 m round the reference
LAP_SPEC = dict(scale=LAP_SCALE, half=LAP_HALF, nx=20, ny=20, nt=24, dtheta=2.0 * math.pi / 1024.0, margin=8)   # +-2.5 m; +-24 steps of 1/16 sector: a sector and a half
LAP_MIN_GAP = 40                                               # keyframes a loop must span: of the lap's 49 only its two ends qualify, not the look-alikes across the field
SECTOR = 2.0 * math.pi / 64.0


def lap_true_pairs(true, max_dist=2.5, min_gap=LAP_MIN_GAP):
    """The true loop pairs of a lap: keyframes (i, j), j <= i - min_gap, whose true positions lie within max_dist -> (i, j) tuples."""
    t = np.asarray(true, np.float64)
    out = []
    for i in range(t.shape[0]):
        for j in range(0, i - min_gap + 1):
            if math.hypot(t[i, 0] - t[j, 0], t[i, 1] - t[j, 1]) < max_dist:
                out.append((i, j))
    return out


def lap_sector_guess(true, i, j):
    """What K18 can know of a pair: no translation, and the relative heading to the nearest sector."""
    d = math.remainder(float(true[j][2]) - float(true[i][2]), 2.0 * math.pi)
    return (0.0, 0.0, round(d / SECTOR) * SECTOR)


def accept(r):
    """The predicate of the lap's tests over a result: the score reaches the number of query points used -- on average every point
    lands on a reference cell's neighbour (1) or on the cell itself (2).  Scans of one place seen from two poses share most of their
    walls; scans of two places share few."""
    return int(r["cnt"]) > 0 and int(r["score"]) >= int(r["n_query"])
