"""Case builders for the K1 (scan-to-map distance + arg-min) edge tests: tests/test_k1_cases_cpu.py checks every case on the CPU (both
oracles, and what the case claims about the kernel's tile steps), tests/test_gpu_search_edges.py runs them on the device.

A case is one map, one scan and one candidate list: `build()` returns (size, pixels, xy, pxcs).  Unless said otherwise c = 1, s = 0 (or
an exact quarter turn), the points are small binary fractions and px = x + 0.5: every operation of :240-241 is exact and the end pixel
of every (candidate, ray) is known without trigonometry.  Maps are one pixel per metre: the mode-1 / mode-2 pose (px - 0.5, py - 0.5, 0)
gives exactly the case's (px, py, 1, 0) (`pose_form`, asserted on the CPU).

`expected(built)` restates the reference rule (CoreSLAMProcessor.cs:226-259, :644) once, with Python integers for everything behind the
two float32 coordinates; `WRONG` names subtly wrong copies of it, each of which must fail a named case (the CPU test).

`plan_piece` / `ray_box` / `one_piece` restate the kernel's decision for ONE piece (k1_ray_box, the planner lambda of k1_pieces.inc) so
that a case can claim the step kind its piece takes; the device test confirms the claim with the per-kind counters
(slamhip_cs_selfcheck_counts) under SLAMHIP_K1_VERIFY=1.  Kind claims are made for the first launch behind set_scan only (a second
search of the same scan may cut the ray ranges by cost), at the default tile budget, with 1024-candidate groups (explicit lists).
"""
import collections

import numpy as np

INT_MAX = 2 ** 31 - 1
F = np.float32
BUDGET = 60 * 1024                     # SLAMHIP_K1_TILE_KB default
MAXBANDS = 4
BAND_STAGE = 5.0
SHARED, GLOBAL, BAND = "shared", "global", "band"
COUNTER_WORD = {SHARED: 1, GLOBAL: 3, BAND: 4}

Case = collections.namedtuple("Case", "name group build claims")
CASES = []


def case(name, group, **claims):
    def deco(fn):
        CASES.append(Case(name, group, fn, claims))
        return fn
    return deco


def by_name(name):
    return next(c for c in CASES if c.name == name)


# ---- maps and candidates ----------------------------------------------------------------------------------------------------------
def pattern(size):
    """pix[y, x] = (131 x + 71 y + 1) mod 65536: neighbours differ in every direction, so a wrong pixel shows in the sum."""
    y, x = np.mgrid[0:size, 0:size].astype(np.int64)
    return ((x * 131 + y * 71 + 1) % 65536).astype(np.uint16)


def uniform(size, v):
    return np.full((size, size), v, np.uint16)


def cand(cells, c=1.0, s=0.0):
    """(cx + 0.5, cy + 0.5, c, s) per cell."""
    cells = np.asarray(cells, np.float64).reshape(-1, 2)
    out = np.empty((cells.shape[0], 4), np.float32)
    out[:, 0] = cells[:, 0] + 0.5
    out[:, 1] = cells[:, 1] + 0.5
    out[:, 2] = c
    out[:, 3] = s
    return out


def pts(p):
    return np.asarray(p, np.float64).reshape(-1, 2).astype(np.float32)


def box_cells(x0, y0, w, h, K, seed):
    """K integer cells in [x0, x0 + w) x [y0, y0 + h): the four corners first, the rest drawn from the seed."""
    rng = np.random.default_rng(seed)
    cells = np.stack([rng.integers(x0, x0 + w, K), rng.integers(y0, y0 + h, K)], 1)
    corners = [(x0, y0), (x0 + w - 1, y0 + h - 1), (x0, y0 + h - 1), (x0 + w - 1, y0)]
    for k, cxy in enumerate(corners[:K]):
        cells[k] = cxy
    return cells


def pose_form(built):
    """(search pose, offsets, poses) of a c = 1, s = 0 case at one pixel per metre, or None."""
    pxcs = built[3]
    if not ((pxcs[:, 2] == 1).all() and (pxcs[:, 3] == 0).all()) or pxcs.shape[0] < 2:
        return None
    poses = np.zeros((pxcs.shape[0], 3), np.float32)
    poses[:, 0] = pxcs[:, 0] - F(0.5)
    poses[:, 1] = pxcs[:, 1] - F(0.5)
    offs = (poses[1:] - poses[:1]).astype(np.float32)
    back = (poses[:1] + offs).astype(np.float32)
    if not ((back == poses[1:]).all() and ((poses[:, :2] + F(0.5)) == pxcs[:, :2]).all()):
        return None
    if (np.signbit(pxcs[:, :2]) & (pxcs[:, :2] == 0)).any():             # (-0.0 does not survive x + 0.5)
        return None
    return poses[0].copy(), offs, poses


# ---- the reference rule, once -----------------------------------------------------------------------------------------------------
WRONG = ("floor", "le_size", "div_count", "max_when_sum0", "mul32", "last_min", "contracted")


def end_points(built, wrong=None):
    """float32 (fx, fy) of every (candidate, ray), one rounding per operation, :240-241."""
    _, _, xy, pxcs = built
    X, Y = xy[None, :, 0], xy[None, :, 1]
    px, py, c, s = (pxcs[:, k:k + 1] for k in range(4))
    with np.errstate(all="ignore"):
        if wrong == "contracted":
            fx = (px + ((c * X).astype(F) - (s * Y).astype(F)).astype(F)).astype(F)
            fy = (py + ((s * X).astype(F) + (c * Y).astype(F)).astype(F)).astype(F)
        else:
            fx = ((px + (c * X).astype(F)).astype(F) - (s * Y).astype(F)).astype(F)
            fy = ((py + (s * X).astype(F)).astype(F) + (c * Y).astype(F)).astype(F)
    return fx, fy


def expected(built, wrong=None):
    """(distance of every candidate, index of the first strict minimum, that minimum) by the reference rule: truncation toward zero,
    in the map iff 0 <= x < size, sum * 1024 / R over ALL rays, int.MaxValue when no end point is in the map, first strict minimum."""
    size, pixels, xy, pxcs = built
    R = xy.shape[0]
    flat = np.asarray(pixels, np.uint16).reshape(-1)
    rnd = np.floor if wrong == "floor" else np.trunc
    hi = size + 1 if wrong == "le_size" else size
    sums, cnts = [], []
    step = max(1, (1 << 22) // max(R, 1))                              # (candidates a block at a time: memory, not arithmetic)
    for k0 in range(0, pxcs.shape[0], step):
        fx, fy = end_points((size, pixels, xy, pxcs[k0:k0 + step]), wrong)
        ix, iy = rnd(fx.astype(np.float64)).astype(np.int64), rnd(fy.astype(np.float64)).astype(np.int64)
        ok = (ix >= 0) & (ix < hi) & (iy >= 0) & (iy < hi)
        idx = np.where(ok, np.clip(iy, 0, size - 1) * size + np.clip(ix, 0, size - 1), 0)
        sums += np.where(ok, flat[idx].astype(np.int64), 0).sum(axis=1).tolist()
        cnts += ok.sum(axis=1).tolist()
    dist = []
    for sm, cn in zip(sums, cnts):                                     # Python integers from here on
        num = sm * 1024
        if wrong == "mul32":
            num &= 0xFFFFFFFF
        den = cn if wrong == "div_count" else R
        none = sm == 0 if wrong == "max_when_sum0" else cn == 0
        dist.append(INT_MAX if none or den == 0 else num // den)
    best = 0
    for k in range(1, len(dist)):
        if dist[k] <= dist[best] if wrong == "last_min" else dist[k] < dist[best]:
            best = k
    return np.array(dist, np.int64).astype(np.int32), best, dist[best]


def key_of(dist, index):
    return (int(dist) << 32) | int(index)


# ---- the kernel's decision for one piece, restated --------------------------------------------------------------------------------
def bounds_of(pxcs):
    """{pxmin, pxmax, pymin, pymax, cmin, cmax, smin, smax} of an explicit list (the workgroup's min / max reduction)."""
    return np.array([pxcs[:, 0].min(), pxcs[:, 0].max(), pxcs[:, 1].min(), pxcs[:, 1].max(),
                     pxcs[:, 2].min(), pxcs[:, 2].max(), pxcs[:, 3].min(), pxcs[:, 3].max()], np.float32)


def ray_box(b, xy):
    """k1_ray_box over the rays xy: (x0, y0, x1, y1), truncated, min / max over the rays."""
    X, Y = xy[:, 0].astype(F), xy[:, 1].astype(F)
    cx0, cx1, sy0, sy1 = b[4] * X, b[5] * X, b[6] * Y, b[7] * Y
    sx0, sx1, cy0, cy1 = b[6] * X, b[7] * X, b[4] * Y, b[5] * Y
    xlo = (b[0] + np.minimum(cx0, cx1)).astype(F) - np.maximum(sy0, sy1)
    xhi = (b[1] + np.maximum(cx0, cx1)).astype(F) - np.minimum(sy0, sy1)
    ylo = (b[2] + np.minimum(sx0, sx1)).astype(F) + np.minimum(cy0, cy1)
    yhi = (b[3] + np.maximum(sx0, sx1)).astype(F) + np.maximum(cy0, cy1)
    t = lambda v: np.trunc(v.astype(np.float64)).astype(np.int64)
    return int(t(xlo).min()), int(t(ylo).min()), int(t(xhi).max()), int(t(yhi).max())


Plan = collections.namedtuple("Plan", "nsteps kind xa ww nb bands cost")


def _shift(vpr):
    return 0 if vpr <= 1 else (vpr - 1).bit_length()


def plan_piece(box, nr, S, budget=BUDGET, group=1024, nopad=False, rows=64):
    """The planner lambda of k1_pieces.inc for one piece: box (x0, y0, x1, y1), nr rays.  rows = PF * NW (64 for every group size)."""
    cpl = {512: 1, 1024: 2, 2048: 4}[group]
    cx0, cy0, cx1, cy1 = max(box[0], 0), max(box[1], 0), min(box[2], S - 1), min(box[3], S - 1)
    if cx1 < cx0 or cy1 < cy0:
        return Plan(0, None, 0, 8, 0, [], 0.0)
    xa = cx0 & ~7
    ww = ((cx1 - xa + 1) + 7) & ~7
    H = cy1 - cy0 + 1
    if group >= 1024 and not (ww & 8) and not nopad and ww < 512 and (xa + ww + 8 <= S or xa >= 8):
        wp, vu = ww + 8, ww >> 3
        hp = min(budget // (wp * 2), rows * (64 >> _shift(wp >> 3)))
        hu = min(budget // (ww * 2), rows * (64 >> _shift(vu)))
        if hp >= 1 and hu >= 1 and -(-H // hp) == -(-H // hu):
            if xa + ww + 8 <= S:
                ww += 8
            else:
                xa -= 8
                ww += 8
    vpr = ww >> 3
    hmax = min(budget // (ww * 2), rows * (64 >> _shift(vpr)))
    nb = -(-H // hmax) if hmax >= 1 else MAXBANDS + 1
    pays = nb == 1 or F(nb) * (F(BAND_STAGE) + F(1.9) * F(nr)) < F(4.5) * F(nr)
    if vpr <= 64 and hmax >= 1 and nb <= MAXBANDS and pays:
        hb = -(-H // nb)
        whole = nb == 1 and (cx0, cy0, cx1, cy1) == tuple(box)
        bands = [(cy0 + k * hb, min(hb, cy1 + 1 - (cy0 + k * hb))) for k in range(nb)]
        stage = F(nb) * F(6.0) + F(20.0) * F(ww * 2) * F(H) / F(budget)
        cost = stage * (F(2.0) / F(cpl)) + (F(nr) if whole else F(1.9) * F(nb) * F(nr))
        return Plan(nb, SHARED if whole else BAND, xa, ww, nb, bands, float(cost))
    return Plan(1, GLOBAL, 0, 8, nb, [], float(F(4.5) * F(nr)))


def sorted_rays(xy):
    """The rays in set_scan's order at one pixel per metre: Z order of the 64-pixel cells, ties in ray order."""
    def spread(v):
        out = 0
        for k in range(16):
            out |= ((v >> k) & 1) << (2 * k)
        return out
    cells = np.clip(xy.astype(F) * F(1.0 / 64.0) + F(32768.0), 0, 65535).astype(np.int64)
    codes = [spread(int(cx)) | (spread(int(cy)) << 1) for cx, cy in cells]
    return np.array(sorted(range(len(codes)), key=lambda i: (codes[i], i)), np.int64)


def one_piece(built):
    """True when the first launch behind set_scan has one workgroup per group and one piece: fewer than 24 rays (n_groups * R / 12 <
    2 workgroups per group) within 64 pixels of each other in both axes (one ray block whatever the extent limit is)."""
    xy = built[2]
    return xy.shape[0] < 24 and float(np.ptp(xy[:, 0])) <= 64 and float(np.ptp(xy[:, 1])) <= 64


def steps_of(built, group=1024, budget=BUDGET, nopad=False, nosplit=False):
    """The step kinds of a one-piece case's workgroups (one per group of `group` candidates): a list of (kind, rays, Plan) per group,
    the piece planned whole or as two halves as k1_pieces.inc does."""
    size, _, xy, pxcs = built
    assert one_piece(built)
    order = sorted_rays(xy)
    rays = xy[order]
    out = []
    for g0 in range(0, pxcs.shape[0], group):
        b = bounds_of(pxcs[g0:g0 + group])
        nr = rays.shape[0]
        full = plan_piece(ray_box(b, rays), nr, size, budget, group, nopad)
        steps = [(full.kind, nr, full)] if full.nsteps else []
        if group >= 1024 and not nosplit and nr >= 8 and full.nsteps > 1:
            h1 = (nr // 2 + 1) & ~1
            pa = plan_piece(ray_box(b, rays[:h1]), h1, size, budget, group, nopad)
            pb = plan_piece(ray_box(b, rays[h1:]), nr - h1, size, budget, group, nopad)
            if F(pa.cost) + F(pb.cost) < F(full.cost):
                steps = [(p.kind, n, p) for p, n in ((pa, h1), (pb, nr - h1)) if p.nsteps]
        out.append(steps)
    return out


# ---- A: truncation and border -----------------------------------------------------------------------------------------------------
A_SIZES = (8, 16, 64, 63, 65)          # 63, 65: not a multiple of 8 -- the fallback kernels


def a_values(S):
    return (-1.0, -0.75, 0.0, 0.5, S - 0.5, S - 1 + 0.99, float(S))


def a_points(S):
    """From the candidate (0.5, 0.5): end points at every value of a_values on each axis (the other axis mid-map) and at the four
    corners just inside and just outside."""
    mid = float(S // 2)
    p = [(v - 0.5, mid) for v in a_values(S)] + [(mid, v - 0.5) for v in a_values(S)]
    p += [(-1.25, -1.25), (S - 1.0, -1.25), (-1.25, S - 1.0), (S - 1.0, S - 1.0), (-0.5, S - 0.51), (S - 0.5, S - 0.5)]
    return pts(p)


for _S in A_SIZES:
    def _mk(S=_S):
        tiled = S % 8 == 0

        @case("a_inside_%d" % S, "A", **({"kinds": {SHARED}} if tiled else {}))
        def _inside():
            """Set 1: the box of the group has truncated corners exactly 0 and size - 1: SHARED at the border on all four sides."""
            cells = [(x, y) for y in (0, S // 2, S - 1) for x in (0, S // 3, S - 1)]
            return S, pattern(S), pts([(0.0, 0.0), (0.49, 0.25), (0.25, 0.49)]), cand(cells)

        @case("a_border_%d" % S, "A", **({"kinds": {BAND}} if tiled and S < 64 else {}))     # (64: the points span 65 px, perhaps two blocks)
        def _border():
            """Set 2: every value of a_values on both axes from (0.5, 0.5); two more candidates one pixel up-right and one down-left:
            the box reaches -2 and size + 1 -- one clipped BAND."""
            return S, pattern(S), a_points(S), cand([(0, 0), (1, 1), (-1, -1)])

        @case("a_negzero_%d" % S, "A", **({"kinds": {SHARED}} if tiled else {}))
        def _negzero():
            """px = -0.0, s = -0.0 and the point (-0.0, -0.0): fx = -0.0, pixel 0, in the map; its neighbour at fx = 0.25 - 0.25."""
            q = cand([(0, 0), (0, 0)])
            q[0, :2] = -0.0
            q[0, 3] = -0.0                                               # (fx = (-0 + -0) - (+0) = -0; with s = +0 it would be -0 - (-0) = +0)
            q[1, :2] = 0.25
            return S, pattern(S), pts([(-0.0, -0.0), (-0.25, -0.25)]), q

        @case("a_outside_%d" % S, "A", **({"kinds": set()} if tiled and S < 64 else {}))
        def _outside():
            """Set 3: every candidate left of the map by more than the points reach: the box misses the map, no steps, every distance
            int.MaxValue, index 0."""
            return S, pattern(S), a_points(S), cand([(-S - 3, 0), (-S - 4, S - 1), (-2 * S, -S - 3), (-S - 3, 2 * S + 2), (-S - 3, -S - 3)])

        for nm, (c, s) in {"q1": (0.0, 1.0), "q2": (-1.0, 0.0), "q3": (0.0, -1.0)}.items():
            @case("a_turn_%s_%d" % (nm, S), "A")
            def _turn(c=c, s=s):
                """The same points under an exact quarter turn about the map's centre pixel."""
                m = S // 2
                p = a_points(S) - F(m)
                return S, pattern(S), p, cand([(m, m), (m - 1, m), (m, m + 1)], c, s)
    _mk()


# ---- B, C, D: one piece on a 1024^2 map, an explicit list of 1024 candidates spanning a chosen box ---------------------------------
SB = 1024


def box_case(x0, y0, w, h, nr, spot=(0.0, 0.0), K=1024, seed=0, S=SB, second=None):
    """K candidates on the integer cells of [x0, x0 + w) x [y0, y0 + h) (corners included), nr rays on one spot -- or, with
    second = (spot, n), the last n of them on another."""
    p = [spot] * nr
    if second:
        p = [spot] * (nr - second[1]) + [second[0]] * second[1]
    return S, pattern(S), pts(p), cand(box_cells(x0, y0, w, h, K, seed + 7 * w + h))


def hmax_of(ww, budget=BUDGET, rows=64):
    """Rows of a tile ww px wide: what the budget holds and what one staging pass (rows wave-wide loads per wavefront set) covers."""
    return min(budget // (ww * 2), rows * (64 >> _shift(ww >> 3)))


def _b(name, x0, y0, w, h, nr, kinds, group="B", plan=None, split=None, **kw):
    extra = {"plan": plan} if plan else {}
    if split:
        extra["split"] = split

    @case(name, group, kinds=kinds, **extra)
    def _f():
        return box_case(x0, y0, w, h, nr, **kw)


# a box 504 px wide from x = 104: ww = 504 (no padding: 504 & 8), 63 lanes per row; the BUDGET holds 61440 / 1008 = 60 rows, one staging
# pass 64
assert hmax_of(504) == 60 and BUDGET // 1008 == 60
_b("b_fits_one_tile", 104, 300, 504, 60, 20, {SHARED}, plan=dict(nb=1, ww=504))
# One row taller: two bands, which pay at 20 rays -- and the banded piece is then tried as two halves of 10 rays, whose two bands do NOT
# pay: two GLOBAL halves (4.5 * 20 = 90 ray units against 32 + 3.8 * 20 = 108).  With every ray on one spot a two-band piece stays
# banded only from 46 rays on, more than a ray range of the first launch ever holds; SLAMHIP_K1_NOSPLIT=1 keeps the bands.
_b("b_one_row_taller", 104, 300, 504, 61, 20, {GLOBAL}, plan=dict(nb=2, kind=BAND, ww=504), split=(10, 10))
# 3 and 4 bands never pay (3 * 1.9 > 4.5, whatever the ray count): GLOBAL, like the fifth band and a box wider than 512 px
_b("b_three_bands", 104, 300, 504, 121, 23, {GLOBAL}, plan=dict(nb=3))
_b("b_four_bands", 104, 300, 504, 181, 23, {GLOBAL}, plan=dict(nb=4))
_b("b_five_bands", 104, 300, 504, 241, 23, {GLOBAL}, plan=dict(nb=5))
_b("b_width_504", 104, 300, 504, 50, 20, {SHARED}, plan=dict(nb=1, ww=504))
_b("b_width_512", 104, 300, 512, 50, 20, {SHARED}, plan=dict(nb=1, ww=512))
_b("b_width_520", 104, 300, 520, 50, 20, {GLOBAL})
# bands pay when nb * (5 + 1.9 nr) < 4.5 nr: two bands from 15 rays on (BANDS_PAY_FROM, computed on the CPU)
_b("b_two_bands_3_rays", 104, 300, 504, 61, 3, {GLOBAL}, plan=dict(nb=2))
_b("b_two_bands_14_rays", 104, 300, 504, 61, 14, {GLOBAL}, plan=dict(nb=2))
_b("b_two_bands_15_rays", 104, 300, 504, 61, 15, {GLOBAL}, plan=dict(nb=2, kind=BAND, ww=504), split=(8, 7))
# the staging pass: a tile 40 px wide takes 8 lanes per row, 8 rows per wave-wide load, 64 loads: 512 rows (the budget allows 768)
assert hmax_of(40) == 512 and BUDGET // 80 == 768
_b("b_staging_rows_512", 80, 100, 40, 512, 20, {SHARED}, plan=dict(nb=1, ww=40))
_b("b_staging_rows_513", 80, 100, 40, 513, 20, {GLOBAL}, plan=dict(nb=2, kind=BAND, ww=40), split=(10, 10))

# the halves: a banded piece of 8 rays or more is tried as two halves of h1 = (nr / 2 + 1) & ~1 and nr - h1 rays.  Two bands pay from 15
# rays on, three from 83, four never (BANDS_PAY_FROM), so no piece of 7 .. 11 rays is ever banded and the `nr >= 8` edge of the split
# cannot be reached (the CPU test proves it for every band count); the halves are tested at 15 .. 19 rays (h1 = 8, 8, 8, 10, 10): the
# first h1 rays on one spot, the rest 60 px above it (the next 64-pixel cell of the Z order), on a box whose tile holds either spot
# (100 rows of 128) and not the union (160).
assert hmax_of(200) == 128
for _nr in (15, 16, 17, 18, 19):
    def _mk(nr=_nr):
        h1 = (nr // 2 + 1) & ~1

        @case("b_halves_%d" % nr, "B", kinds={SHARED}, split=(h1, nr - h1))
        def _halves():
            return box_case(104, 300, 200, 100, nr, spot=(0.0, 10.0), second=((0.0, 70.0), nr - h1))
    _mk()

# C: pitch padding -- a width that is a multiple of 16 px gets 8 more columns where the map has room
for _w in (8, 16, 24, 32, 192, 496, 504, 512):
    _b("c_width_%d" % _w, 104, 300, _w, 40, 20, {SHARED}, group="C", plan=dict(nb=1, ww=_w + (8 if _w % 16 == 0 and _w < 512 else 0)))
_b("c_right_border_192", SB - 192, 300, 192, 40, 20, {SHARED}, group="C", plan=dict(nb=1, ww=200, xa=SB - 200))
_b("c_right_border_496", SB - 496, 300, 496, 40, 20, {SHARED}, group="C", plan=dict(nb=1, ww=504, xa=SB - 504))
for _S in (16, 32):
    def _mk(S=_S):
        @case("c_whole_map_%d" % S, "C", kinds={SHARED}, plan=dict(nb=1, ww=S, xa=0))
        def _whole():
            """The tile spans the whole map: no room on either side, no padding."""
            return box_case(0, 0, S, S, 20, S=S)
    _mk()

# D: the gather loops -- four rays per round, then a pair, then the odd one, primed with the zero word -- in each step kind
D_RAYS = (1, 2, 3, 4, 5, 6, 7, 8, 9)
D_RAYS_CUT = (63, 64, 65)
for _nr in D_RAYS + D_RAYS_CUT:
    _sfx = "%d" % _nr if _nr in D_RAYS else "%d_in_ranges" % _nr
    _b("d_shared_" + _sfx, 104, 300, 100, 40, _nr, {SHARED}, group="D")
    _b("d_band_" + _sfx, 0, 300, 100, 40, _nr, {BAND}, group="D", spot=(-3.0, 0.0))        # (clipped at x = 0: one band, range-tested)
    _b("d_global_" + _sfx, 104, 300, 520, 40, _nr, {GLOBAL}, group="D")
# (one spot: a ray range of any length is one piece of the same box.  With ONE group of 1024 candidates the first launch cuts 63, 64
# and 65 rays into ranges of about 12 -- the *_in_ranges cases; the 65th ray is a block of its own.)


def first_launch_ranges(n_groups, R):
    """Ray ranges per group of the first launch behind set_scan for an explicit list (k1_layout_choose, k1_make_layout without the
    groups' spreads): the target is 512 workgroups (768 beyond 64 groups), or a workgroup per 12 rays of a group if that is fewer, and
    a range holds at most 512 rays.  (A scan of R <= 64 rays on one spot is one block: every count of ranges is legal.)"""
    target = 512 if n_groups <= 64 else 768
    by_work = n_groups * R // 12
    if by_work < target:
        target = max(by_work, n_groups)
    want = max(int(target / n_groups + 0.5), 1)
    return min(max(want, -(-R // 512)), R)


# A piece of 63 or 64 rays -- the gather loops at full length -- needs ONE range per group: 768 / n_groups < 1.5, 513 groups or more.
ONE_PIECE_GROUPS = 513
assert first_launch_ranges(ONE_PIECE_GROUPS, 63) == 1 and first_launch_ranges(ONE_PIECE_GROUPS, 64) == 1 and first_launch_ranges(512, 64) == 2
for _nr in (63, 64):
    for _kind, (_x0, _w, _spot) in {SHARED: (104, 100, (0.0, 0.0)), BAND: (0, 100, (-3.0, 0.0)), GLOBAL: (104, 520, (0.0, 0.0))}.items():
        def _mk(nr=_nr, kind=_kind, x0=_x0, w=_w, spot=_spot):
            @case("d_%s_%d_one_piece" % (kind, nr), "D", kinds={kind}, one_piece_of=nr, big=True, many_groups=True)
            def _one():
                """513 groups of 1024 candidates on the cells of one box (the same 1024 cells in every group, shifted by the group's
                number mod 3 in y inside the box's rows): every workgroup has one range, one piece of nr rays."""
                S, pix, xy, q = box_case(x0, 300, w, 38, nr, spot=spot)
                q = np.tile(q, (ONE_PIECE_GROUPS, 1))
                q[:, 1] += np.repeat(np.arange(ONE_PIECE_GROUPS) % 3, 1024).astype(np.float32)
                return S, pix, xy, q
        _mk()


# ---- E: chunks and pieces ---------------------------------------------------------------------------------------------------------
for _R in (16, 17, 64, 600):
    def _mk(R=_R):
        @case("e_own_blocks_%d" % R, "E")
        def _own():
            """Every ray in a block of its own: the points of a 25 x 25 grid of 131 px pitch (any two differ by more than the block
            extent limit of 128 px in an axis), in a shuffled order, on a 4096^2 map."""
            k = np.random.default_rng(R).permutation(625)[:R]
            p = np.stack([(k % 25) * 131.0, (k // 25) * 131.0], 1)
            cells = box_cells(20, 20, 60, 60, 40, R)
            return 4096, pattern(4096), pts(p), cand(cells)
    _mk()

for _R in (511, 512, 513, 1024):
    def _mk(R=_R):
        @case("e_one_spot_%d" % R, "E")
        def _spot():
            return box_case(104, 300, 100, 40, R, K=70, S=256, spot=(3.0, -5.0), seed=R)
    _mk()

RAY_LIMIT = 2 ** 20                    # the accumulator's pixel sum holds R < 2^20 rays x 65535


def many_rays_case(R, patterned):
    pix = pattern(64) if patterned else uniform(64, 65535)
    return 64, pix, np.zeros((R, 2), np.float32), cand([(5, 9), (63, 63), (64, 3)])


for _R, _nm in ((RAY_LIMIT - 1, "below"), (RAY_LIMIT, "at")):
    for _pat in (False, True):
        def _mk(R=_R, nm=_nm, pat=_pat):
            @case("e_ray_limit_%s_%s" % (nm, "pattern" if pat else "65535"), "E", big=True, many_rays=True)
            def _lim():
                """2^20 - 1 rays: the tiled path with every accumulator at its limit; 2^20: the fallback kernels."""
                return many_rays_case(R, pat)
        _mk()


# ---- F: in-map flag, sum and finish -----------------------------------------------------------------------------------------------
def zero_only_case(kind, where):
    """40 rays in three or more ray ranges.  ONE ray (spot P, a ray block of its own) ends in the map, on a pixel forced to 0 for
    candidate 0: its distance is 0, not int.MaxValue.  The other 39 (spots Q, 2000 px above or below: the first / last of the Z order)
    end outside for every candidate: no steps.  BAND and GLOBAL: candidate 1, in the same lane group, is outside with P too:
    int.MaxValue.  (SHARED: every candidate of the group is in the map with P by the kind's definition.)"""
    S, R = SB, 40
    w = {SHARED: 100, BAND: 100, GLOBAL: 520}[kind]
    x0 = 0 if kind == BAND else 104
    P = (-3.0, 0.0) if kind == BAND else (0.0, 0.0)
    up, down = (P[0], 2000.0), (P[0], -2000.0)
    q_spots = {"first": [up] * (R - 1), "last": [down] * (R - 1), "middle": [down] * (R // 2) + [up] * (R - 1 - R // 2)}[where]
    cells = box_cells(x0, 300, w, 40, 1024, 11)
    cells[4] = (x0 + 50, 305)
    cells[[0, 4]] = cells[[4, 0]]                                        # candidate 0 mid-box (the corners stay in the list)
    if kind == BAND:
        cells[1] = (1, 310)                                              # fx = 1.5 - 3 = -1.5: pixel -1
    if kind == GLOBAL:
        cells[1] = (-700, 310)
    pix = pattern(S)
    pix[305, int(x0 + 50 + P[0])] = 0
    return S, pix, pts(q_spots[:7] + [P] + q_spots[7:]), cand(cells)


for _kind in (SHARED, BAND, GLOBAL):
    for _where in ("first", "middle", "last"):
        def _mk(kind=_kind, where=_where):
            @case("f_zero_only_%s_%s" % (kind, where), "F", kinds={kind}, spots=True)
            def _zero():
                return zero_only_case(kind, where)
        _mk()

F_R = (3, 7, 1079, 1081, 4097)


def sum_case(R, rem):
    """One candidate column whose pixel sum s has s * 1024 mod R = rem (rem = -1: R - 1): all rays on pixel (2, 3) of a 16^2 map of
    zeros but the last, on pixel (4, 5) holding the adjustment; plus 65535 everywhere for the largest sum."""
    S = 16
    pix = uniform(S, 0)
    want = rem % R
    v = next(v for v in range(1, 65536) if (v * 1024) % R == want)
    pix[5, 4] = v
    p = [(0.0, 0.0)] * (R - 1) + [(2.0, 2.0)]
    q = cand([(2, 3), (9, 9), (2, 3)])
    return S, pix, pts(p), q


for _R in F_R:
    for _rem in (0, 1, -1):
        def _mk(R=_R, rem=_rem):
            @case("f_sum_mod_%d_%s" % (R, {0: "0", 1: "1", -1: "Rm1"}[rem]), "F")
            def _sum():
                return sum_case(R, rem)
        _mk()

    def _mk(R=_R):
        @case("f_sum_largest_%d" % R, "F")
        def _largest():
            """65535 at every end point of every ray: sum * 1024 = R * 67 107 840 needs 64 bits from 64 rays on."""
            return 16, uniform(16, 65535), pts([(float(k % 5), float(k % 3)) for k in range(R)]), cand([(2, 3), (9, 9), (40, 3), (0, 0)])
    _mk()


def tie_case(K, winners, seed):
    """K candidates on a map of 100s with a few cells of 50: the candidates of `winners` sit on a 50-cell, all others on 100."""
    S = 64
    pix = uniform(S, 100)
    rng = np.random.default_rng(seed)
    cells = np.stack([rng.integers(0, 32, K), rng.integers(0, 64, K)], 1)
    pix[:, 40] = 50
    for k in winners:
        cells[k] = (40, int(rng.integers(0, 64)))
    return S, pix, pts([(0.0, 0.0)] * 5), cand(cells)


@case("f_tie_uniform", "F")
def _tie_uniform():
    """A uniform map: all candidates equal, index 0 wins."""
    S, _, xy, q = tie_case(2049, (), 1)
    return S, uniform(S, 777), xy, q


for _nm, _K, _w in (("0", 2049, (0, 1023, 1024, 2048)), ("1023", 2049, (1023, 1024, 2048)), ("1024", 2049, (1024, 2048)), ("last", 2049, (2048,)),
                    ("1023_1024", 1500, (1024, 1023))):
    def _mk(nm=_nm, K=_K, w=_w):
        @case("f_tie_first_%s" % nm, "F")
        def _tie():
            """Equal minima across lane groups: the smallest flat index wins."""
            return tie_case(K, w, K + len(w))
    _mk()


# ---- G: candidate counts ----------------------------------------------------------------------------------------------------------
G_COUNTS = (1, 2, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049)


def count_case(K):
    """K candidates, the strict winner the LAST one: the last lane of the last, partly filled group."""
    S = 64
    pix = pattern(S)
    pix[60, 60] = 0
    rng = np.random.default_rng(K)
    cells = np.stack([rng.integers(0, 50, K), rng.integers(0, 50, K)], 1)
    cells[K - 1] = (60, 60)
    return S, pix, pts([(0.0, 0.0), (0.0, 0.25), (0.25, 0.0)]), cand(cells)


for _K in G_COUNTS:
    def _mk(K=_K):
        @case("g_count_%d" % K, "G")
        def _count():
            return count_case(K)
    _mk()


# ---- I: address width -------------------------------------------------------------------------------------------------------------
# k1_tile_addr_d (tile addresses as binary32 denormals) is exact while S * pitch2 + 2 S + 2^18 < 2^23: on an 8192^2 map up to a pitch
# of 494 px; a tile 504 px wide takes the integer address.  On 4096^2 both take the denormal one.
def denormal_ok(S, ww):
    return S * 2 * ww + 2 * S + 2 ** 18 < 2 ** 23


def address_case(S, w):
    return box_case(S - 600, S - 200, w, 40, 20, S=S, seed=S)


for _S in (4096, 8192):
    for _w, _ww in ((480, 488), (504, 504)):
        def _mk(S=_S, w=_w, ww=_ww):
            @case("i_address_%d_w%d" % (S, w), "I", kinds={SHARED}, plan=dict(nb=1, ww=ww), big=S == 8192, denormal=denormal_ok(S, ww))
            def _addr():
                """A SHARED tile in the last rows of the map, where the tile's byte offset is largest."""
                return address_case(S, w)
        _mk()


# ---- seeded cases: real rotations, non-integer values (expectation: the C oracle under deterministic trigonometry) -----------------
def seeded_case(seed, S=64, R=64, K=256):
    """Non-integer points and candidates with a real rotation, from the seed."""
    rng = np.random.default_rng(seed)
    xy = (rng.random((R, 2)) * 40 - 20).astype(np.float32)
    th = rng.random(K) * 6.0 - 3.0
    q = np.stack([rng.random(K) * S, rng.random(K) * S, np.cos(th), np.sin(th)], 1).astype(np.float32)
    return S, pattern(S), xy, q


def find_contracted_seed(limit=200):
    """The first seed whose case tells (px + c X) - s Y from px + (c X - s Y)."""
    for seed in range(limit):
        b = seeded_case(seed)
        if (expected(b)[0] != expected(b, "contracted")[0]).any():
            return seed
    raise AssertionError("no seed below %d separates the contracted form" % limit)


CONTRACTED_SEED_FOUND = 64             # find_contracted_seed() (asserted equal on the CPU)


@case("s_rotations_contracted", "S", seeded=True)
def _seeded():
    return seeded_case(CONTRACTED_SEED_FOUND)


for _seed in (101, 102, 103):
    def _mk(seed=_seed):
        @case("s_rotations_%d" % seed, "S", seeded=True)
        def _rot():
            return seeded_case(seed, S=128, R=300, K=700)
    _mk()


# ---- H: bounds from the jitter (mode 1 only; expectation: the C oracle's search under deterministic trigonometry) -------------------
HCase = collections.namedtuple("HCase", "name size pose offs xy")
H_CASES = []
HALF_PI = 1.5707963267948966


def _h(name, pose, dth, reach=20.0, size=256, K=600, seed=0, dxy=3.0):
    """K - 1 jitters whose headings span exactly [dth[0], dth[1]] (both ends present), translations within +-dxy."""
    rng = np.random.default_rng(1000 + len(H_CASES) + seed)
    offs = np.stack([rng.uniform(-dxy, dxy, K - 1), rng.uniform(-dxy, dxy, K - 1), rng.uniform(dth[0], dth[1], K - 1)], 1)
    offs[0, 2], offs[1, 2] = dth[0], dth[1]
    ang = rng.uniform(0, 2 * np.pi, 90)
    rad = rng.uniform(0.2 * reach, reach, 90)
    xy = np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1)
    H_CASES.append(HCase(name, size, np.array(pose, np.float32), offs.astype(np.float32), xy.astype(np.float32)))


for _k in (0, 1, 2, 3, -1):
    _h("h_ends_on_%d_half_pi" % _k, (128, 128, _k * HALF_PI - 0.3), (0.0, 0.3))
    _h("h_ends_5e-4_inside_%d" % _k, (128, 128, _k * HALF_PI - 0.3), (0.0, 0.3 - 5e-4))
    _h("h_ends_2e-3_outside_%d" % _k, (128, 128, _k * HALF_PI - 0.3), (0.0, 0.3 + 2e-3))
_h("h_span_6.1", (128, 128, 0.4), (-3.05, 3.05))
_h("h_span_6.3", (128, 128, 0.4), (-3.15, 3.15))
_h("h_straddles_pi", (128, 128, 3.1), (-0.2, 0.2))
_h("h_straddles_minus_pi", (128, 128, -3.1), (-0.2, 0.2))
_h("h_heading_plus_100", (128, 128, 100.0), (-0.1, 0.1))
_h("h_heading_minus_100", (128, 128, -100.0), (-0.1, 0.1))
for _d in (10.0, 1e3, 1e5, 1e8):
    _h("h_pad_only_%g" % _d, (128, 128, 0.0), (0.0, 0.0), reach=_d)


def spot_kinds(built, group=1024, budget=BUDGET, nopad=False):
    """For a case whose rays lie on a few spots more than 128 px apart (every spot's rays: ray blocks of their own): the set of step
    kinds over every spot, candidate group and piece length 1 .. 64 -- whatever the ray ranges are, a piece is some rays of ONE spot."""
    size, _, xy, pxcs = built
    spots = np.unique(xy, axis=0)
    for i in range(len(spots)):
        for j in range(i):
            assert np.abs(spots[i] - spots[j]).max() > 128
    kinds = set()
    for g0 in range(0, pxcs.shape[0], group):
        b = bounds_of(pxcs[g0:g0 + group])
        for sp in spots:
            n = int((xy == sp).all(axis=1).sum())
            box = ray_box(b, sp[None, :])
            for nr in range(1, min(n, 64) + 1):
                p = plan_piece(box, nr, size, budget, group, nopad)
                if p.nsteps:
                    kinds.add(p.kind)
    return kinds


def bands_pay_from(nb, limit=10000):
    """The smallest ray count from which nb bands pay (nb * (5 + 1.9 nr) < 4.5 nr in binary32), or None."""
    for nr in range(1, limit):
        if F(nb) * (F(BAND_STAGE) + F(1.9) * F(nr)) < F(4.5) * F(nr):
            return nr
    return None


# ---- mode-1 ties: equal minima whose headings sort the later flat index first ---------------------------------------------------------
# Every ray on the point (0, 0): the end point is (px, py) whatever the heading, so the distances are those of the c = 1, s = 0 case and
# the jitters' headings only decide the order in which the device evaluates the candidates (theta-sorted).  The winner is the smallest
# flat index among the equal minima.
TCase = collections.namedtuple("TCase", "name base order")
T_CASES = [TCase("t_%s_%s" % (b, o), "f_tie_" + b, o) for b in ("uniform", "first_0", "first_1023", "first_1024", "first_last", "first_1023_1024")
           for o in ("descending", "shuffled")]


def t_by_name(name):
    return next(c for c in T_CASES if c.name == name)


def tie_heading_form(tc):
    """(built, search pose, offsets) of a mode-1 tie case: the pose form of its base case with dtheta descending in the flat index (the
    theta sort reverses the flat order) or shuffled."""
    built = by_name(tc.base).build()
    assert (built[2] == 0).all()
    pose, offs, _ = pose_form(built)
    n = offs.shape[0]
    dth = np.linspace(0.5, -0.5, n).astype(np.float32)
    if tc.order == "shuffled":
        dth = dth[np.random.default_rng(n).permutation(n)]
    offs = offs.copy()
    offs[:, 2] = dth
    return built, pose, offs


def h_by_name(name):
    return next(c for c in H_CASES if c.name == name)
