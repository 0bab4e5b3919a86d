"""GPU tests of the Hector matcher (K4) on RAW maps, bit for bit, and of the probability grid against binary64.

The other bit-exact matcher tests (test_gpu_hector_refsum.py, _report.py, _refcache.py) quantise their maps so that every
probability is exactly 0.5 or 1.0, because the device's expf and the oracle's libm expf may differ in the last place.  On
such a map the interpolation of ScanMatcher.cs:245-248 multiplies by 0.5 and 1.0 only -- exact products, which a fused
multiply-add, a reassociated sum or a swapped tap round the same as the literal form.  Here the maps stay as UpdateByScan
left them, and the one legitimate difference is taken out of the comparison instead: the device's own probability grid
(GetCachedProbability of every cell) is installed in the oracle (Grid.set_prob_table, "pinned").  The device in reference
order T and the oracle at T threads then perform the same binary32 operations on the same inputs, and every result is
compared with same_bits.  Whose expf it is, is tested on its own (a): every cell against a binary64 reference, with a bound
derived from the documented accuracy of the device's expf.

Nothing here accepts a neighbourhood or an envelope.  The one comparison that is not an equality (c, the default summation
order) uses the any-order bound for a binary32 sum, derived and not measured."""
import math

import numpy as np
import pytest

from test_gpu_hector_refsum import HINT_OFFS, TRUE_POSE, build_pyramid, capi_mod, ctx, det, hs_mod, same_bits  # noqa: F401
from test_gpu_hector_report import chunk_sum, in_map, residual_terms, transform_points

pytestmark = pytest.mark.gpu

F = np.float32
TS = (1, 2, 3, 4, 7, 16, 64)
# id: cells (w, h), cell length, levels, iterations per level, rays, T values, update factors, scan origin
MAPS = {
    "square400": ((400, 400), 0.1, 4, [7, 4, 4, 4], 400, TS, None, (0.0, 0.0)),
    "c4": ((2048, 2048), 40.0 / 2048, 3, [3, 3, 3], 1080, (1, 4, 64), None, (0.0, 0.0)),
    "wide": ((640, 256), 0.1, 3, [3, 3, 3], 400, TS, None, (0.0, 0.0)),       # 64 m x 25.6 m: part of every scan ends outside
    "tall": ((256, 640), 0.1, 3, [3, 3, 3], 400, TS, None, (0.0, 0.0)),
    "odd": ((401, 233), 0.1, 3, [3, 3, 3], 400, TS, None, (0.0, 0.0)),        # levels 401x233, 200x116, 100x58
    "factors": ((301, 301), 0.13, 2, [3, 3], 400, TS, (0.3, 0.8), (0.5, -0.25)),
}
SPECIAL = ("square400", "wide", "odd")                                         # the maps every special scan / hint runs on
BORDER = ("wide", "tall", "odd")
RUNAWAY = (0.8, 0.0, 0.25)                                                     # a hint 0.8 m and 0.25 rad off
POSE_B = np.array([24.0, 22.0, 1.0], np.float32)
POSE_IN = np.array([12.0, 14.0, 0.5], np.float32)                              # every point inside on all maps: the control

# ---- (a) the bound on the probability grid ---------------------------------------------------------------------------------
# The device evaluates OccGridMap.cs:101-102 in binary32: o = expf(v); p = o / (o + 1).  Against P = e^v / (e^v + 1):
#   * expf: the HIP math API documents a maximum error of 1 ulp for expf (E = 1).  One ulp of a normal binary32 number o is
#     at most 2^-23 |o|, so o = e^v (1 + d1), |d1| <= E 2^-23.
#   * conditioning of f(o) = o / (o + 1): f'(o) o / f(o) = 1 / (o + 1), so d1 enters p as d1 / (o + 1) (to first order; the
#     second-order term is below 2^-45).
#   * the add and the divide are correctly rounded: half an ulp each, relative errors |d2|, |d3| <= 2^-24.
# Relative error of p: E 2^-23 / (1 + o) + 2^-24 + 2^-24.  A relative error d of a binary32 value x is at most d 2^24 ulp(x)
# (x < 2^24 ulp(x)), hence in ulp:  2 E / (1 + o) + 2.  The reference value is P rounded once to binary32: another 1/2.
#   bound(v) = 2 E / (1 + e^v) + 2.5 ulp          (4.5 ulp for very negative v, 2.5 for large v, 3.5 at v = 0)
# In the denormal range (e^v < 2^-126) relative bounds do not hold, but there o + 1 == 1 and o / 1 == o exactly, so
# p = o = e^v +- E denormal ulps, and P = e^v (1 - ~e^v) rounds within half: E + 0.5 <= bound(v), with ulp = 2^-149.
# Second-order terms and the rounding of e^v in the bound itself are covered by the 1e-3 added below.
EXPF_MAX_ULP = 1.0


def p64(v):
    """1 / (1 + exp(-v)) in binary64 from binary32 cell values."""
    v = np.asarray(v, np.float32).astype(np.float64)
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-v))


def prob_bound_ulp(v):
    v = np.asarray(v, np.float32).astype(np.float64)
    with np.errstate(over="ignore"):
        return 2.0 * EXPF_MAX_ULP / (1.0 + np.exp(v)) + 2.5 + 1e-3


def prob_error_ulp(got, v):
    """|got - round32(p64(v))| in ulps of the rounded reference (np.spacing: 2^-149 in the denormal range and at zero)."""
    want = p64(v).astype(np.float32)
    ulp = np.spacing(np.abs(want)).astype(np.float64)
    return np.abs(np.asarray(got, np.float32).astype(np.float64) - want.astype(np.float64)) / ulp


def pin_probabilities(rep, ref):
    """The device's probability of every cell of every level, installed in the oracle level (call again after every update
    of the maps).  Returns the tables."""
    tables = []
    for l, m in enumerate(rep.Maps):
        w, h = m.Dimensions
        p = m.GetCachedProbability(np.arange(w * h, dtype=np.int32))
        ref[l].set_prob_table(p)
        tables.append(p)
    return tables


class RawMap:
    def __init__(self, name, hs_mod, ctx, oc, sim, npo):
        dims, cell, levels, iters, R, ts, factors, origin = MAPS[name]
        self.name, self.dims, self.cell, self.levels, self.iters, self.R, self.ts, self.origin = name, dims, cell, levels, iters, R, ts, origin
        self.hs, self.oc, self.sim, self.npo = hs_mod, oc, sim, npo
        self.rep, self.ref, self.segs, self.rng = build_pyramid(hs_mod, ctx, oc, sim, dims, cell, levels, R, 12, False,
                                                                factors=factors, origin=origin)
        for l, it in enumerate(iters):
            self.rep.Maps[l].EstimateIterations = it
        for l in range(levels):                                            # built on both sides, NOT quantised: cells bit-equal
            c = self.rep.Maps[l].GetCells()
            assert (c["update_index"] == self.ref[l].cells["update_index"]).all(), (name, l)
            assert same_bits(c["value"], self.ref[l].cells["value"]), (name, l)
            assert len(np.unique(c["value"])) > 4, (name, l)
        self.pin()

    def pin(self):
        self.tables = pin_probabilities(self.rep, self.ref)
        self.grids = []
        for l, m in enumerate(self.rep.Maps):                              # NumPy twins on the same probabilities (for c)
            w, h = m.Dimensions
            g = self.npo.NpGrid(np.float32(m.CellLength), w, h, trig="det")
            g.set_prob_table(self.tables[l])
            self.grids.append(g)

    def scan(self, pose, R=None):
        return self.sim.make_scan(self.segs, np.asarray(pose, np.float32), R or self.R, self.rng)[1]

    def close(self):
        self.rep.close()
        for g in self.ref:
            g.close()


@pytest.fixture(scope="module")
def maps(hs_mod, ctx, det, sim, npo):
    """name -> RawMap, built on first use and shared by the tests of this module"""
    built = {}

    def get(name):
        if name not in built:
            built[name] = RawMap(name, hs_mod, ctx, det, sim, npo)
        return built[name]
    yield get
    for M in built.values():
        M.close()


ALL = pytest.mark.parametrize("name", list(MAPS))
ON_SPECIAL = pytest.mark.parametrize("name", SPECIAL)


# ---- the oracle's side of a report ------------------------------------------------------------------------------------------
def oracle_points(M, l, xy, pose_map):
    """(M per point, in-map mask) on oracle level l at pose_map.  A pose that is not finite leaves every point outside the map
    (NaN or infinite coordinates, MapProperties.cs:83-87)."""
    g = M.ref[l]
    n = xy.shape[0]
    if not np.isfinite(np.asarray(pose_map, np.float32)).all():
        return np.zeros(n, np.float32), np.zeros(n, bool)
    mx, my = transform_points(M.npo, g.cell_len, xy, pose_map)
    vals = np.array([g.interp(float(a), float(b))[0] for a, b in zip(mx, my)], np.float32).reshape(n)
    return vals, in_map(g.w, g.h, mx, my)


def oracle_residual(M, l, xy, pose_world, T):
    vals, inside = oracle_points(M, l, xy, M.ref[l].map_pose(pose_world))
    return chunk_sum(residual_terms(vals), T), int(inside.sum())


def check_report(M, l, xy, out_pose, r, T, tag):
    """pose_map, H, dTr, residual, n_in_map of a reference-order report: same_bits with the oracle at T on the pinned
    probabilities."""
    g = M.ref[l]
    pm = g.map_pose(out_pose)
    assert same_bits(r["pose_map"], pm), (tag, r["pose_map"], pm)
    Hr, dr = g.hessian(xy, pm, T)
    assert same_bits(r["H"], Hr) and same_bits(r["dTr"], dr), (tag, r["H"], Hr, r["dTr"], dr)
    want, cnt = oracle_residual(M, l, xy, out_pose, T)
    assert same_bits(r["residual"], want), (tag, r["residual"], want)
    assert int(r["n_in_map"]) == cnt, (tag, int(r["n_in_map"]), cnt)
    assert int(r["n_points"]) == xy.shape[0] and int(r["level"]) == l, tag


def host_key_argmin(residuals):
    """slamhip_hs_match_best's key, restated: (bits(residual) << 32 | index), 64-bit minimum."""
    bits = np.ascontiguousarray(residuals, np.float32).view(np.uint32).astype(np.uint64)
    return int(np.argmin((bits << np.uint64(32)) | np.arange(bits.shape[0], dtype=np.uint64)))


def check_case(M, xy, hints, ts, tag, levels=True, batches=True):
    """Everything the matcher offers for one scan, in reference order T, against the oracle at T, bit for bit:
    slamhip_hs_hessian on every level; MatchData on the pyramid and on each level at 1 iteration and at the level's own count,
    each with its report; MatchDataBatch at B = 3 and 12 (both kernels) with reports; MatchDataBest."""
    hs, oc, rep, ref, iters = M.hs, M.oc, M.rep, M.ref, M.iters
    xy = np.ascontiguousarray(xy, np.float32)
    scan = hs.ScanCloud(xy)
    n_cmp = 0
    try:
        for T in ts:
            m = hs.ScanMatcher(T, referenceSummation=True)
            rep.set_match_threads(T)
            rep.set_scan(scan)
            for l in range(M.levels if levels else 1):
                for hint in hints:
                    est = ref[l].map_pose(hint)
                    H, d = rep.Maps[l].Hessian(est)
                    Hr, dr = ref[l].hessian(xy, est, T)
                    assert same_bits(H, Hr) and same_bits(d, dr), (tag, "hessian", l, hint, T, H, Hr, d, dr)
                    n_cmp += 1
            for hint in hints:
                want = oc.match_pyramid(ref, xy, hint, iters, n_threads=T)
                pose, r = m.MatchDataReport(rep, scan, hint)
                assert same_bits(pose, want), (tag, "pyramid", hint, T, pose, want)
                assert same_bits(m.MatchData(rep, scan, hint), want), (tag, "pyramid, plain", hint, T)
                check_report(M, 0, xy, pose, r, T, (tag, "pyramid report", hint, T))
                n_cmp += 1
            for l in range(M.levels if levels else 1):
                for its in sorted({1, iters[l]}):                          # (one iteration keeps the step large)
                    rep.Maps[l].EstimateIterations = its
                    for hint in hints:
                        want = ref[l].match(xy, hint, its, T)
                        pose, r = m.MatchDataReport(rep.Maps[l], scan, hint)
                        assert same_bits(pose, want), (tag, "level", l, its, hint, T, pose, want)
                        check_report(M, l, xy, pose, r, T, (tag, "level report", l, its, hint, T))
                        n_cmp += 1
                rep.Maps[l].EstimateIterations = iters[l]
            if batches:
                many = np.stack([hints[i % len(hints)] + F(1e-3) * F(i // len(hints)) * np.array([1, -1, 0.5], np.float32) for i in range(12)])
                wants = [oc.match_pyramid(ref, xy, h, iters, n_threads=T) for h in many]
                res = [oracle_residual(M, 0, xy, w, T)[0] for w in wants]
                for B in (3, 12):
                    poses, reps = m.MatchDataBatchReport(rep, scan, many[:B])
                    plain = m.MatchDataBatch(rep, scan, many[:B])
                    for i in range(B):
                        assert same_bits(poses[i], wants[i]) and same_bits(plain[i], wants[i]), (tag, "batch", B, i, T, poses[i], wants[i])
                        assert same_bits(reps[i]["residual"], res[i]), (tag, "batch residual", B, i, T)
                    for i in (0, B - 1):
                        check_report(M, 0, xy, poses[i], reps[i], T, (tag, "batch report", B, i, T))
                    pose, idx, r = m.MatchDataBest(rep, scan, many[:B])
                    if not np.isnan(np.array(res[:B], np.float32)).any():  # (a NaN's sign and payload are the unit's own: no key to restate)
                        assert idx == host_key_argmin(res[:B]), (tag, "best", B, T, idx, res[:B])
                    assert same_bits(pose, wants[idx]), (tag, "best pose", B, T, idx)
                    check_report(M, 0, xy, pose, r, T, (tag, "best report", B, T))
                    n_cmp += B + 1
    finally:
        for l, it in enumerate(iters):
            rep.Maps[l].EstimateIterations = it
        rep.set_match_threads(0)
    return n_cmp


# ---- (a) -------------------------------------------------------------------------------------------------------------------
@ALL
def test_probability_grid_binary64(maps, name):
    """Every cell of every level after mapping: the device's probability within bound(v) ulp of p64 rounded once."""
    M = maps(name)
    for l in range(M.levels):
        v = M.ref[l].cells["value"]
        got = M.tables[l]
        assert np.isfinite(v).all() and (np.abs(v) < 80).all()             # (the maps stay far from the ends of the ladder below)
        err, bound = prob_error_ulp(got, v), prob_bound_ulp(v)
        worst = int(np.argmax(err - bound))
        print("probabilities %s level %d: %d cells, %d distinct values, max error %.3f ulp (bound there %.3f)"
              % (M.name, l, v.size, len(np.unique(v)), float(err.max()), float(bound[int(np.argmax(err))])))
        assert (err <= bound).all(), (M.name, l, worst, v[worst], got[worst], err[worst], bound[worst])
        # ... and against the C oracle's float expression (libm expf): both are within their bounds of the same curve
        # (prob_literal: the oracle's own expression; prob reads the pinned table)
        some = np.flatnonzero(v != 0)[:2000]
        own = np.array([M.ref[l].prob_literal(int(i)) for i in some], np.float32)
        assert (prob_error_ulp(own, v[some]) <= prob_bound_ulp(v[some])).all()


def test_probability_ladder(hs_mod, ctx, det):
    """A hand-made ladder of cell values uploaded with SetCells, to both ends of binary32's exp: overflow (expf = inf from
    v ~ 88.7228 on: inf / (inf + 1) is NaN in the reference too, OccGridMap.cs:101-102) and the denormal range (expf below
    2^-126 for v < ~ -87.34, zero below ~ -103.97).  Inside the binary64 curve: bound(v).  Where the reference's float
    expression leaves it, what the C oracle's float expression gives: NaN where it gives NaN; in the denormal range the
    oracle's value exactly or within bound(v) -- a device that flushes denormals answers 0 there and fails this."""
    oc = det
    rep = hs_mod.MapRepMultiMap(1.0, (32, 32), 1, ctx=ctx)
    g = oc.Grid(1.0, 32, 32)
    lo_free, lo_occ = g.logodds
    ladder = [0.0]
    for x in (lo_free, lo_occ, 1e-3, 10.0, 50.0, np.inf):
        ladder += [x, -x]
    ladder += [87.0, 88.5, 88.72, 88.73, 89.0, 100.0, -87.0, -87.4, -100.0, -103.9, -104.0, np.nan]
    ladder += [-87.3, -87.34, -90.0, -95.0, -103.97, -103.98, 88.7228, 88.7229, 1e-30, -1e-30, 1e30, -1e30]    # (around the thresholds, and tiny / huge)
    ladder = np.array(ladder, np.float32)
    cells = rep.Maps[0].GetCells()
    cells["value"][:ladder.size] = ladder
    rep.Maps[0].SetCells(cells)
    g.cells["value"][:] = cells["value"]
    got = rep.Maps[0].GetCachedProbability(np.arange(ladder.size, dtype=np.int32))
    want_c = np.array([g.prob(i) for i in range(ladder.size)], np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        e64 = np.exp(ladder.astype(np.float64))
    err, bound = prob_error_ulp(got, ladder), prob_bound_ulp(ladder)
    n_nan = n_den = 0
    for i, v in enumerate(ladder):
        print("ladder v = %-12g device %-14.9g C oracle %-14.9g p64 %-14.9g error %.3f ulp (bound %.3f)"
              % (v, got[i], want_c[i], p64(v), err[i], bound[i]))
        if np.isnan(want_c[i]):                                            # overflow, +inf, NaN
            assert np.isnan(got[i]), (v, got[i])
            n_nan += 1
        elif e64[i] < 2.0 ** -126:                                         # the denormal range (and below it)
            assert got[i] == want_c[i] or err[i] <= bound[i], (v, got[i], want_c[i], err[i], bound[i])
            n_den += 1
        else:
            assert err[i] <= bound[i], (v, got[i], want_c[i], err[i], bound[i])
    assert n_nan >= 6 and n_den >= 8
    # the ends as such
    at = {float(v): i for i, v in enumerate(ladder) if not np.isnan(v)}
    assert got[at[0.0]] == 0.5 and got[at[-np.inf]] == 0.0 and got[at[88.5]] == 1.0
    assert got[at[float(F(-100.0))]] > 0.0, "the device flushed a denormal probability to zero"
    rep.close()
    g.close()


# ---- (b) -------------------------------------------------------------------------------------------------------------------
@ALL
def test_ordinary_and_runaway_hints(maps, name):
    """The hints of the quantised tests and a runaway hint 0.8 m / 0.25 rad off, on every map, T over the map's list: the
    whole battery of check_case."""
    M = maps(name)
    xy = M.scan(TRUE_POSE)
    hints = [TRUE_POSE + np.array(d, np.float32) for d in HINT_OFFS + (RUNAWAY,)]
    oc, ref = M.oc, M.ref
    # the check discriminates: on raw maps the oracle's own answers differ between thread counts
    assert any(not same_bits(ref[0].hessian(xy, ref[0].map_pose(h), 1)[0], ref[0].hessian(xy, ref[0].map_pose(h), 4)[0]) for h in hints)
    n = check_case(M, xy, hints, M.ts, (M.name, "ordinary"))
    print("%s: %d reference-order comparisons" % (M.name, n))


@ON_SPECIAL
def test_few_ray_scans(maps, name):
    """3, 4, 6 and 11 points: near-singular H; Matrix4x4.Invert refusing is a legal outcome and must be the same one."""
    M = maps(name)
    hints = [TRUE_POSE + np.array(d, np.float32) for d in HINT_OFFS[1:3]]
    for R in (3, 4, 6, 11):
        xy = M.scan(TRUE_POSE, R)
        assert xy.shape[0] == R
        check_case(M, xy, hints, M.ts, (M.name, "few", R))


@ON_SPECIAL
def test_long_scan(maps, name):
    """More than 2048 points: the points are read from global memory, not from LDS."""
    M = maps(name)
    xy = M.scan(TRUE_POSE, 2500)
    assert xy.shape[0] > 2048
    hints = [TRUE_POSE + np.array(d, np.float32) for d in HINT_OFFS[1:3]]
    check_case(M, xy, hints, (1, 3, 4, 64), (M.name, "long"))


@ON_SPECIAL
def test_hostile_points(maps, name):
    """The soak's hostile points (far away, a duplicate, the origin, NaN -- a NaN point makes rotDeriv NaN * 0) and a scan whose
    every point lies outside the map."""
    M = maps(name)
    hints = [TRUE_POSE + np.array(d, np.float32) for d in HINT_OFFS[1:3]]
    base = M.scan(TRUE_POSE)
    no_nan = base.copy()
    no_nan[0] = [3.0e4, -2.0e4]; no_nan[1] = no_nan[2]; no_nan[3] = [0.0, 0.0]
    with_nan = no_nan.copy()
    with_nan[4] = [np.nan, 1.0]
    outside = (base + np.array([900.0, -700.0], np.float32)).astype(np.float32)
    for tag, xy in (("hostile", no_nan), ("hostile+nan", with_nan), ("outside", outside)):
        check_case(M, xy, hints, M.ts, (M.name, tag))
    assert oracle_residual(M, 0, outside, hints[0], 1) == (F(outside.shape[0]), 0)     # (every point adds exactly 1)


@ALL
@pytest.mark.parametrize("where", ["true_pose", "pose_b", "all_in"])
def test_border_scans(maps, name, where):
    """Robot poses at which the scan straddles the map border: between 10 % and 90 % of the points out of the map on level 0
    at the matched pose.  That share is a condition on the inputs: it is computed from the oracle's pose and asserted before
    the device is looked at.  (12, 14, 0.5) is the control: every point inside, on every map.  (It is a degenerate one: that pose
    lies on an edge of the field's inner obstacle, so every range is the noise around zero, the points sit on unmapped cells
    beside the robot and H is zero -- the `H[0] != 0` gate of ScanMatcher.cs:97 stays shut on both sides.  No pose inside the
    field keeps a whole 360-degree scan inside both the 25.6 m wide and the 25.6 m high map with walls in view.)"""
    M = maps(name)
    pose = {"true_pose": TRUE_POSE, "pose_b": POSE_B, "all_in": POSE_IN}[where]
    xy = M.scan(pose)
    hints = [pose + np.array(d, np.float32) for d in HINT_OFFS[:3]]
    n = xy.shape[0]
    for hint in hints:
        for T in (1, 4):
            want = M.oc.match_pyramid(M.ref, xy, hint, M.iters, n_threads=T)
            _, cnt = oracle_residual(M, 0, xy, want, T)
            share_out = 1.0 - cnt / n
            if where == "all_in" or M.name not in BORDER:
                assert share_out == 0.0, (M.name, where, hint, T, share_out)
            else:
                assert 0.10 <= share_out <= 0.90, (M.name, where, hint, T, share_out)
    if M.name not in BORDER:
        return                                                             # (all inside: nothing the ordinary hints do not already cover)
    check_case(M, xy, hints, M.ts, (M.name, "border", where))


PI32, HALF_PI32 = F(3.14159274), F(F(3.14159274) / F(2))
HEADINGS = {                                                                # name: (heading, inside a snapping window)
    "0": (0.0, True), "+1e-6": (1e-6, True), "-1e-6": (-1e-6, True),
    "pi/2": (float(HALF_PI32), True), "pi/2+1e-6": (float(HALF_PI32) + 1e-6, True), "pi/2-1e-6": (float(HALF_PI32) - 1e-6, True),
    "-pi/2": (-float(HALF_PI32), True), "-pi/2+1e-6": (-float(HALF_PI32) + 1e-6, True), "-pi/2-1e-6": (-float(HALF_PI32) - 1e-6, True),
    "pi-1e-6": (float(PI32) - 1e-6, True), "-pi+1e-6": (-float(PI32) + 1e-6, True),
    # just outside the 0.001 degree (1.745e-5 rad) window of Matrix3x2.CreateRotation
    "+3e-5": (3e-5, False), "-3e-5": (-3e-5, False), "pi/2+3e-5": (float(HALF_PI32) + 3e-5, False),
    "-pi/2-3e-5": (-float(HALF_PI32) - 3e-5, False), "pi-3e-5": (float(PI32) - 3e-5, False), "-pi+3e-5": (-float(PI32) + 3e-5, False),
    # |theta| >= pi: hs_rotation_sc falls back to the general CreateRotation (IEEERemainder first; +-pi itself is snapped)
    "pi": (float(PI32), True), "-pi": (-float(PI32), True), "3.2": (3.2, False), "-3.5": (-3.5, False), "7.0": (7.0, False),
}


@ON_SPECIAL
@pytest.mark.parametrize("heading", list(HEADINGS), ids=list(HEADINGS))
def test_heading_windows(maps, name, heading):
    """True headings and hints inside the snapping windows of Matrix3x2.CreateRotation (the rotation matrix is snapped to
    exact 0 / 90 / 180 / 270 degrees; sinRot / cosRot of ScanMatcher.cs:145-146 are not), just outside them, and at
    |theta| >= pi.  The Hessian at exactly that heading, one-iteration matches (the first step is taken inside the window)
    and full matches."""
    M = maps(name)
    th, inside = F(HEADINGS[heading][0]), HEADINGS[heading][1]
    true = np.array([20.6, 20.25, math.remainder(float(th), 2 * math.pi)], np.float32)
    xy = M.scan(true)
    hints = [np.array([20.6, 20.25, th], np.float32), np.array([20.68, 20.19, th], np.float32)]
    # a condition on the inputs: the rotation of this heading is snapped to exact 0 / +-1 entries inside a window and is not
    # outside, while the sine and cosine of the derivative (:145-146) are never snapped
    rot = [float(v) for v in M.npo.M32.rotation(th, "det").m[:2]]
    assert (rot[0] in (0.0, 1.0, -1.0) and rot[1] in (0.0, 1.0, -1.0)) == inside, (heading, rot)
    check_case(M, xy, hints, (1, 4, 64), (M.name, "heading", heading))


def test_reference_cache_transparent_on_odd(maps):
    """The reference's probability cache on, no Reset: the same bits as with it off -- on a rectangular, odd-sided map, where
    the cache's idx + w + 1 addressing differs from the square maps'.  (The probabilities were pinned while the cache was off.)"""
    M = maps("odd")
    xy = M.scan(TRUE_POSE)
    hints = [TRUE_POSE + np.array(d, np.float32) for d in HINT_OFFS[:3]]
    border = M.scan(POSE_B)
    M.rep.set_reference_cache(1)
    try:
        check_case(M, xy, hints, (1, 4, 7), (M.name, "refcache"))
        check_case(M, border, [POSE_B + np.array(d, np.float32) for d in HINT_OFFS[:2]], (1, 4), (M.name, "refcache border"))
    finally:
        M.rep.set_reference_cache(0)


@pytest.mark.parametrize("name", ["odd", "factors"])
def test_pin_again_after_update(maps, name):
    """One more UpdateByScan (with the map's scan origin), the probabilities pinned again: still bit for bit.  (Without the
    second pin the oracle would read probabilities of a map that no longer exists.)"""
    M = maps(name)
    p = np.array([20.7, 20.3, 0.13], np.float32)
    upd = M.scan(p)
    before = [t.copy() for t in M.tables]
    M.rep.UpdateByScan(M.hs.ScanCloud(upd, (M.origin[0], M.origin[1], 0.0)), p)
    for l, g in enumerate(M.ref):
        g.update_by_scan(upd, p, origin=M.origin)
        c = M.rep.Maps[l].GetCells()
        assert (c["update_index"] == g.cells["update_index"]).all() and same_bits(c["value"], g.cells["value"]), l
    M.pin()
    assert any(not same_bits(a, b) for a, b in zip(before, M.tables))
    xy = M.scan(TRUE_POSE)
    check_case(M, xy, [TRUE_POSE + np.array(d, np.float32) for d in HINT_OFFS[:3]], (1, 4, 16), (M.name, "after update"))


# ---- (c) -------------------------------------------------------------------------------------------------------------------
def exact_sums(M, l, xy, pose_map):
    """The ten sums of a report at pose_map from the per-point binary32 terms (NumPy restatement on the pinned probabilities),
    summed exactly: (S[10], A[10] = sum of |term|), order dTr.x, dTr.y, dTr.z, H11, H22, H33, H12, H13, H23, residual."""
    terms, vals = M.grids[l].hessian_terms(xy, pose_map)
    terms = np.concatenate([terms, residual_terms(vals)[None, :]]).astype(np.float64)
    return [math.fsum(t) for t in terms], [math.fsum(np.abs(t)) for t in terms]


@ALL
def test_default_order_against_exact_sum(maps, name):
    """T = 0, the device's own summation order: H, dTr and the residual of slamhip_match_report and H, dTr of slamhip_hs_hessian
    against the exact sum S of the same binary32 terms: |got - S| <= gamma_n * sum |term|, gamma_n = n u / (1 - n u), u = 2^-24
    -- the bound of ANY order of binary32 additions (Higham, Accuracy and Stability of Numerical Algorithms, sec. 4.2), derived
    and not measured; both sides on the same probabilities."""
    M = maps(name)
    u = 2.0 ** -24
    poses = [TRUE_POSE] + ([POSE_B, POSE_IN] if M.name in BORDER else [])
    m = M.hs.ScanMatcher(1)
    for pose in poses:
        xy = M.scan(pose)
        scan = M.hs.ScanCloud(xy)
        n = xy.shape[0]
        gamma = n * u / (1 - n * u)
        hints = [pose + np.array(d, np.float32) for d in HINT_OFFS]
        cases = [(m.MatchDataReport(M.rep, scan, h)[1], 0) for h in hints]
        cases += [(m.MatchDataReport(M.rep.Maps[l], scan, hints[1])[1], l) for l in range(M.levels)]
        bp, br = m.MatchDataBatchReport(M.rep, scan, np.stack(hints * 3))
        cases += [(br[i], 0) for i in (0, 11)]
        for r, l in cases:
            pm = r["pose_map"]
            assert np.isfinite(pm).all()
            S, A = exact_sums(M, l, xy, pm)
            H = r["H"].reshape(3, 3)
            got = [r["dTr"][0], r["dTr"][1], r["dTr"][2], H[0, 0], H[1, 1], H[2, 2], H[0, 1], H[0, 2], H[1, 2], r["residual"]]
            assert H[1, 0] == H[0, 1] and H[2, 0] == H[0, 2] and H[2, 1] == H[1, 2]
            for k in range(10):
                assert abs(float(got[k]) - S[k]) <= gamma * A[k], (M.name, pose, l, k, float(got[k]), S[k], gamma * A[k])
            mx, my = transform_points(M.npo, M.ref[l].cell_len, xy, pm)
            assert int(r["n_in_map"]) == int(in_map(M.ref[l].w, M.ref[l].h, mx, my).sum()) and int(r["n_points"]) == n
            # slamhip_hs_hessian at the same pose
            M.rep.set_match_threads(0)
            M.rep.set_scan(scan)
            Hh, dh = M.rep.Maps[l].Hessian(pm)
            goth = [dh[0], dh[1], dh[2], Hh[0, 0], Hh[1, 1], Hh[2, 2], Hh[0, 1], Hh[0, 2], Hh[1, 2]]
            for k in range(9):
                assert abs(float(goth[k]) - S[k]) <= gamma * A[k], (M.name, pose, l, "hessian", k, float(goth[k]), S[k], gamma * A[k])
