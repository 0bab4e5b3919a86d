"""The scrolling map window (slamhip_hs_shift, slamhip_hsproc_set_scroll) against the checker, bit for bit.

K4 and K5 work in the window's frame and are not touched, so the checker's side of a shift is NumPy: on level l new cell (x, y)
holds what old cell (x + (dx >> l), y + (dy >> l)) held, and a cell whose source lies outside the level is LogOddsCell.Reset(),
(UpdateIndex -1, Value 0.0f) -- `shifted` below, applied to the checker's own arrays (oracle_c.Grid.cells is a writable view) at
the moments the device shifts.

Probabilities: the device's expf and the checker's libm expf may differ in the last place, so -- as in
test_gpu_hector_rawparity.py -- a bit-exact match needs the device's own probability grid installed in the checker
(Grid.set_prob_table).  A stale grid must not slip through that way, so a table is only ever taken from the device after it
was compared with 1 / (1 + exp(-Value)) in binary64 (PROB_ATOL), and ACROSS a shift it is never taken from the device at all:
the table from before the shift is moved by the rule above, 0.5f in the exposed band, and the device must equal it bit for bit.

The maps are the smallest at which each path of the kernel can go wrong (16-byte units of the destination: two cells, four
probabilities): 64x64 (everything aligned on level 0, odd source offsets on the coarsest level), 72x40 (non-square), 70x46
(level 1 is 35x23, level 2 17x11: rows that are no multiple of a unit, units that straddle rows, an array tail)."""
import math

import numpy as np
import pytest

gpu = pytest.mark.gpu

F = np.float32
CELL = 0.1
LEVELS = 3
G = 1 << (LEVELS - 1)
SHAPES = [(64, 64), (72, 40), (70, 46)]
SHAPE_IDS = ["64x64", "72x40", "70x46"]
ITERS = [3, 3, 3]
POS_TOL = 1e-4
ANG_TOL = 1e-4
# |p32 - P| for the device's p32 = o / (o + 1), o = expf(v), against P in binary64: at most 4.5 ulp of p32
# (test_gpu_hector_rawparity.py derives 2 E / (1 + e^v) + 2.5 ulp with E = 1 for expf), p32 <= 1, ulp <= 2^-24 below 1:
# 4.5 * 2^-24 = 2.7e-7.  A probability that did not follow its cell is off by far more.
PROB_ATOL = 4.5 * 2.0 ** -24 + 1e-9


def shifts_of(w0, h0):
    return [(G, 0), (0, -G), (-2 * G, 3 * G), (w0, 0), (-w0 - G, h0 + G)]


@pytest.fixture(scope="module")
def hs_mod():
    import slam.net_amd.hector as m
    return m


@pytest.fixture(scope="module")
def ctx(hs_mod):
    c = hs_mod.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def det(oc):
    oc.set_trig_mode(oc.TRIG_DET)
    yield oc
    oc.set_trig_mode(oc.TRIG_LIBM)


def same_bits(a, b):
    a = np.ascontiguousarray(a, np.float32).ravel(); b = np.ascontiguousarray(b, np.float32).ravel()
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def raw(cells):
    """The 8-byte records {UpdateIndex, Value} as they lie in memory."""
    return np.ascontiguousarray(cells).view(np.uint64)


def shifted(a, w, h, sx, sy, fill):
    """The rule of slamhip_hs_shift on one level: out[y, x] = a[y + sy, x + sx], `fill` where the source is outside."""
    a = np.asarray(a).reshape(h, w)
    out = np.empty_like(a)
    out[...] = np.array(fill, a.dtype)
    x0, x1 = max(0, -sx), min(w, w - sx)
    y0, y1 = max(0, -sy), min(h, h - sy)
    if x0 < x1 and y0 < y1:
        out[y0:y1, x0:x1] = a[y0 + sy:y1 + sy, x0 + sx:x1 + sx]
    return out.ravel()


def shift_checker(ref, dx, dy):
    for l, g in enumerate(ref):
        g.cells[:] = shifted(g.cells.copy(), g.w, g.h, dx >> l, dy >> l, (-1, 0.0))


def shift_tables(ref, tables, dx, dy):
    return [shifted(t, g.w, g.h, dx >> l, dy >> l, 0.5).astype(np.float32) for l, (g, t) in enumerate(zip(ref, tables))]


def device_prob(rep, l):
    w, h = rep.Maps[l].Dimensions
    return rep.Maps[l].GetCachedProbability(np.arange(w * h, dtype=np.int32))


def checked_tables(rep, ref):
    """The device's probability grids, each compared with its cells' values in binary64 before it is trusted."""
    out = []
    for l, g in enumerate(ref):
        p = device_prob(rep, l)
        v = g.cells["value"].astype(np.float64)
        with np.errstate(over="ignore"):
            want = 1.0 / (1.0 + np.exp(-v))
        err = np.abs(p.astype(np.float64) - want)
        assert err.max() <= PROB_ATOL, (l, float(err.max()))
        out.append(p)
    return out


def pin(ref, tables):
    for g, t in zip(ref, tables):
        g.set_prob_table(t)


# ---- maps filled by real updates ------------------------------------------------------------------------------------------------
_SCANS = {}


def fill_scans(sim):
    """The update inputs of tests/test_gpu_hector.py at its small size (400 rays in the default field, poses
    (20 + 0.25 i, 20 - 0.1 i, 0.15 i)), made once."""
    if "fill" not in _SCANS:
        segs = sim.default_field()
        rng = sim.PCG32(400)
        out = []
        for it in range(7):
            p = np.array([20 + 0.25 * it, 20 - 0.1 * it, 0.15 * it], np.float32)
            out.append((sim.make_scan(segs, p, 400, rng)[1], p))
        _SCANS["fill"] = out
    return _SCANS["fill"]


def local_scans(sim, w0, h0):
    """... shrunk so that the 40 m world is as wide as the window (the field's walls then lie inside a 6.4 m map, where a beam
    that ends outside would be dropped whole, OccGridMap.cs:158-161), the robot's path through the window's middle."""
    s = F(w0 * CELL / 40.0)
    out = []
    for xy, p in fill_scans(sim):
        pl = np.array([p[0] * s, F(h0 * CELL / 2) + (p[1] - F(20)) * s, p[2]], np.float32)
        out.append(((xy * s).astype(np.float32), pl))
    return out


def build(hs_mod, ctx, oc, sim, dims):
    w0, h0 = dims
    rep = hs_mod.MapRepMultiMap(CELL, dims, LEVELS, ctx=ctx)
    ref = oc.make_pyramid(CELL, w0, h0, LEVELS)
    for xy, p in local_scans(sim, w0, h0):
        rep.UpdateByScan(hs_mod.ScanCloud(xy), p)
        for g in ref:
            g.update_by_scan(xy, p)
    for l in range(LEVELS):
        assert np.array_equal(raw(rep.Maps[l].GetCells()), raw(ref[l].cells)), l
    assert np.count_nonzero(ref[0].cells["value"]) > (w0 * h0) // 8           # a map worth moving
    assert len(np.unique(ref[LEVELS - 1].cells["value"])) > 4
    return rep, ref


def assert_maps_equal(rep, ref, checksum_np, tag):
    for l, g in enumerate(ref):
        got = rep.Maps[l].GetCells()
        assert np.array_equal(raw(got), raw(g.cells)), (tag, l)
        assert (rep.Maps[l].GetBitmapData() == g.bitmap()).all(), (tag, l)
        assert rep.Maps[l].GetMapExtends() == g.map_extends(), (tag, l)
        assert rep.Maps[l].checksum() == (checksum_np(got["value"]), checksum_np(got["update_index"])), (tag, l)


def assert_prob_equal(rep, ref, tables, tag):
    """The device's probabilities of all indices against the expected tables and against the checker's prob() on them."""
    pin(ref, tables)
    for l, g in enumerate(ref):
        p = device_prob(rep, l)
        assert same_bits(p, tables[l]), (tag, l)
        assert same_bits(p, np.array([g.prob(i) for i in range(g.w * g.h)], np.float32)), (tag, l)


def close_all(rep, ref):
    rep.close()
    for g in ref:
        g.close()


# ---- 1. contents after a shift ---------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dims", SHAPES, ids=SHAPE_IDS)
def test_contents_after_shift(hs_mod, ctx, det, sim, checksum_np, dims):
    w0, h0 = dims
    rep, ref = build(hs_mod, ctx, det, sim, dims)
    orig = [g.cells.copy() for g in ref]
    tables0 = checked_tables(rep, ref)
    for k, (dx, dy) in enumerate(shifts_of(w0, h0)):
        if k:                                                              # every shift starts from the filled map
            for l in range(LEVELS):
                rep.Maps[l].SetCells(orig[l])
                ref[l].cells[:] = orig[l]
            tables0 = checked_tables(rep, ref)
        before = rep.origin()
        if dx % G or dy % G:
            # 70x46: w0 and h0 are no multiples of g = 4, so the list's (w0, 0) and (-w0 - g, h0 + g) are shifts the interface
            # refuses (each level must move by whole cells) -- with maps and origin unchanged.  What those two entries are there for,
            # a move by the level's size or more that clears every level, is then made with each component taken away from zero to
            # the next multiple of g (72, and (-76, 52)): still past the size of every level.
            sums = [rep.Maps[l].checksum() for l in range(LEVELS)]
            with pytest.raises(hs_mod.capi.SlamhipError) as e:
                rep.shift(dx, dy)
            assert e.value.code == hs_mod.capi.ERR_INVALID
            assert rep.origin() == before and [rep.Maps[l].checksum() for l in range(LEVELS)] == sums
            assert_maps_equal(rep, ref, checksum_np, ("refused", dx, dy))
            assert abs(dx) >= w0 or abs(dy) >= h0, (dx, dy)                # (only the clearing entries of the list can be odd ones)
            up = lambda v: int(math.copysign(-(-abs(v) // G) * G, v)) if v else 0
            dx, dy = up(dx), up(dy)
        rep.shift(dx, dy)
        assert rep.origin() == (before[0] + dx, before[1] + dy)
        shift_checker(ref, dx, dy)
        if abs(dx) >= w0 or abs(dy) >= h0:
            assert all((g.cells["update_index"] == -1).all() and (raw(g.cells) == raw(g.cells)[0]).all() for g in ref)
        else:
            assert any(np.count_nonzero(g.cells["value"]) for g in ref)     # something did stay in the window
        assert_maps_equal(rep, ref, checksum_np, (dx, dy))
        assert_prob_equal(rep, ref, shift_tables(ref, tables0, dx, dy), (dx, dy))
    close_all(rep, ref)


# ---- 2. the map still works after it moved ---------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dims", SHAPES, ids=SHAPE_IDS)
def test_match_and_update_after_shift(hs_mod, ctx, det, sim, dims):
    oc = det
    w0, h0 = dims
    rep, ref = build(hs_mod, ctx, oc, sim, dims)
    tables = checked_tables(rep, ref)
    dx, dy = G, -G
    rep.shift(dx, dy)
    shift_checker(ref, dx, dy)
    tables = shift_tables(ref, tables, dx, dy)
    pin(ref, tables)
    xy, p_world = local_scans(sim, w0, h0)[-1]
    p_win = np.array([p_world[0] - F(dx) * F(CELL), p_world[1] - F(dy) * F(CELL), p_world[2]], np.float32)
    hints = [p_win + np.array(d, np.float32) for d in ((0, 0, 0), (0.03, -0.02, 0.02), (-0.04, 0.03, -0.03))]
    scan = hs_mod.ScanCloud(xy)
    m1 = hs_mod.ScanMatcher(1, referenceSummation=True)
    m0 = hs_mod.ScanMatcher(1)
    for hint in hints:
        got = m1.MatchData(rep, scan, hint)
        want = oc.match_pyramid(ref, xy, hint, ITERS, n_threads=1)
        assert same_bits(got, want), (hint, got, want)
        assert not same_bits(got, hint)                                    # the map was there to match against
    rep.UpdateByScan(scan, p_win)                                          # a stale pointer, probability grid or sector record shows here
    for g in ref:
        g.set_prob_table(None)
        g.update_by_scan(xy, p_win)
    for l in range(LEVELS):
        assert np.array_equal(raw(rep.Maps[l].GetCells()), raw(ref[l].cells)), l
    pin(ref, checked_tables(rep, ref))
    for hint in hints:
        want = oc.match_pyramid(ref, xy, hint, ITERS, n_threads=1)
        assert same_bits(m1.MatchData(rep, scan, hint), want), hint
        got = m0.MatchData(rep, scan, hint)                                # the device's own summation order
        assert abs(got[0] - want[0]) < POS_TOL and abs(got[1] - want[1]) < POS_TOL, (hint, got, want)
        assert abs(math.remainder(float(got[2]) - float(want[2]), 2 * math.pi)) < ANG_TOL, (hint, got, want)
    close_all(rep, ref)


# ---- 3. round trip ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dims", SHAPES, ids=SHAPE_IDS)
def test_round_trip(hs_mod, ctx, det, sim, checksum_np, dims):
    rep, ref = build(hs_mod, ctx, det, sim, dims)
    tables = checked_tables(rep, ref)
    for dx, dy in ((G, 0), (-2 * G, 3 * G)):
        orig = [g.cells.copy() for g in ref]
        rep.shift(dx, dy)
        rep.shift(-dx, -dy)
        assert rep.origin() == (0, 0)
        for l, g in enumerate(ref):                                        # the original with the exposed bands cleared
            once = shifted(orig[l], g.w, g.h, dx >> l, dy >> l, (-1, 0.0))
            g.cells[:] = shifted(once, g.w, g.h, (-dx) >> l, (-dy) >> l, (-1, 0.0))
            keep = raw(g.cells) == raw(orig[l])
            assert keep.any() and (g.cells["update_index"][~keep] == -1).all() and (g.cells["value"][~keep] == 0).all()
        tables = shift_tables(ref, shift_tables(ref, tables, dx, dy), -dx, -dy)
        assert_maps_equal(rep, ref, checksum_np, (dx, dy))
        assert_prob_equal(rep, ref, tables, (dx, dy))
    close_all(rep, ref)


# ---- 4. stream order -------------------------------------------------------------------------------------------------------------
@gpu
def test_stream_order(hs_mod, ctx, det, sim):
    """Update, shift, shift and match issued back to back equal the same calls with the stream drained after each.  (At the
    operator level UpdateByScan itself ends with a wait; the un-waited update -> shift -> match order is what
    HectorSLAMProcessor.Update issues, test_processor_scrolls_and_keeps_mapping.)"""
    dims = (70, 46)
    xy, p = local_scans(sim, *dims)[-1]
    scan = hs_mod.ScanCloud(xy)
    results = []
    for waited in (False, True):
        rep, ref = build(hs_mod, ctx, det, sim, dims)
        rep.set_match_threads(1)
        sync = ctx.synchronize if waited else (lambda: None)
        rep.UpdateByScan(scan, p); sync()
        rep.shift(G, 0); sync()
        rep.shift(-2 * G, G); sync()
        p_win = np.array([p[0] + F(G) * F(CELL), p[1] - F(G) * F(CELL), p[2]], np.float32)
        rep.set_scan(scan)
        out = np.empty(3, np.float32)
        hs_mod.capi.call("slamhip_hs_match", rep._h, hs_mod.capi.fptr(p_win), hs_mod.capi.fptr(out)); sync()
        rep.shift(0, 2 * G)                                                # ... and one behind the match
        results.append((out.copy(), [rep.Maps[l].GetCells() for l in range(LEVELS)], [device_prob(rep, l) for l in range(LEVELS)]))
        if waited:                                                         # the waited sequence is the checker's
            for g in ref:
                g.update_by_scan(xy, p)
            for d in ((G, 0), (-2 * G, G), (0, 2 * G)):
                shift_checker(ref, *d)
            for l in range(LEVELS):
                assert np.array_equal(raw(results[-1][1][l]), raw(ref[l].cells)), l
        close_all(rep, ref)
    (pose_a, cells_a, prob_a), (pose_b, cells_b, prob_b) = results
    assert same_bits(pose_a, pose_b)
    for l in range(LEVELS):
        assert np.array_equal(raw(cells_a[l]), raw(cells_b[l])) and same_bits(prob_a[l], prob_b[l]), l


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------
@gpu
def test_refusals(hs_mod, ctx, det, sim):
    capi = hs_mod.capi
    rep, ref = build(hs_mod, ctx, det, sim, (64, 64))
    rep.shift(G, -G)                                                       # a non-zero origin to keep
    state = lambda: ([rep.Maps[l].checksum() for l in range(LEVELS)], rep.origin())
    s0 = state()
    assert s0[1] == (G, -G)
    for dx, dy in ((G - 1, 0), (0, G - 1), (-1, G), (G, 2)):
        with pytest.raises(capi.SlamhipError) as e:
            rep.shift(dx, dy)
        assert e.value.code == capi.ERR_INVALID and "multiple" in str(e.value)
        assert state() == s0
    rep.set_reference_cache(1)
    with pytest.raises(capi.SlamhipError) as e:
        rep.shift(G, 0)
    assert e.value.code == capi.ERR_INVALID and "cache" in str(e.value)
    assert state() == s0
    rep.set_reference_cache(0)
    rep.shift(0, 0)
    assert state() == s0
    rep.shift(G, 0)                                                        # (and with the cache off again it moves)
    assert rep.origin() == (2 * G, -G) and state()[0] != s0[0]
    rep.Reset()
    assert rep.origin() == (0, 0)
    close_all(rep, ref)


@gpu
def test_scroll_setting_validation(hs_mod, ctx):
    capi = hs_mod.capi
    proc = hs_mod.HectorSLAMProcessor(CELL, (72, 40), [3.6, 2.0, 0.0], LEVELS, ctx=ctx)
    lim = 40 // 2 - G                                                      # valid: [0, min(w0, h0) / 2 - g)
    proc.set_scroll(lim - 1)
    for bad in (-1, lim, lim + 100):
        with pytest.raises(capi.SlamhipError) as e:
            proc.set_scroll(bad)
        assert e.value.code == capi.ERR_INVALID
    proc.set_scroll(0)
    assert proc.get_origin() == (0, 0)
    proc.Dispose()


# ---- 6. the processor drives out of the window and keeps mapping -----------------------------------------------------------------
W = 128                                                                    # window: 128 x 128 x 3 levels of 0.1 m = 12.8 m
TRIGGER = 16
N_SCANS = 80
RAYS = 180
MIN_DIST, MIN_ANGLE = 0.3, 0.13                                            # HectorSLAMProcessor.cs:51,56 (the defaults)
START = np.array([6.4, 6.4, 0.0], np.float32)                              # the window's middle


def corridor():
    """A straight corridor along x, 70 m long (more than five windows) and 4 m wide, with 1 m deep alcoves every 2.5 m,
    alternating sides, of widths that do not repeat within a window (so that a scan knows where along the axis it is)."""
    x0, x1, ya, yb = -5.0, 65.0, 4.4, 8.4
    segs = [(x0, ya, x0, yb), (x1, ya, x1, yb)]
    for side, y, out in ((0, ya, -1.0), (1, yb, 1.0)):
        x = x0
        k = 0
        while x < x1:
            a = x0 + 2.5 * k + (1.25 if side else 0.0) + 0.6
            wdt = 0.5 + 0.13 * ((7 * k + 3 * side) % 9)
            if a + wdt >= x1:
                segs.append((x, y, x1, y))
                break
            segs += [(x, y, a, y), (a, y, a, y + out), (a, y + out, a + wdt, y + out), (a + wdt, y + out, a + wdt, y)]
            x = a + wdt
            k += 1
    return np.array(segs, np.float64)


def drive(sim):
    """(true pose, scan) per step, the lidar looking forward only (so that a robot beyond a fixed window sees nothing of it,
    whatever lies behind): 40 steps of 0.35 m (every scan redraws the map: the launch-ahead update) and 40 of 0.2 m
    (every second one does); both below 2 x MinDistanceDiffForMapUpdate.  22 m in all, 1.7 windows."""
    if "drive" not in _SCANS:
        segs = corridor()
        rng = sim.PCG32(77)
        out = []
        x = float(START[0])
        for i in range(N_SCANS):
            if i:
                x += 0.35 if i <= 40 else 0.2
            tp = np.array([x, 6.4 + 0.05 * math.sin(0.3 * i), 0.02 * math.sin(0.2 * i)], np.float32)
            xy = sim.make_scan(segs, tp, 2 * RAYS, rng)[1]
            out.append((tp, np.ascontiguousarray(xy[xy[:, 0] > 0.2])))    # a forward-looking lidar: at most RAYS points
        _SCANS["drive"] = out
    return _SCANS["drive"]


def odometry(i, sim):
    d = drive(sim)
    return (d[i][0] - d[i - 1][0]).astype(np.float32) if i else np.zeros(3, np.float32)


def moved_enough(oc, pose, last):
    """HectorSLAMProcessor.cs:107-108 in binary32."""
    ddx, ddy = F(pose[0]) - F(last[0]), F(pose[1]) - F(last[1])
    with np.errstate(over="ignore", invalid="ignore"):
        d2 = F(F(ddx * ddx) + F(ddy * ddy))
    return bool(d2 > F(F(MIN_DIST) * F(MIN_DIST)) or F(oc.deg_diff(float(pose[2]), float(last[2]))) > F(MIN_ANGLE))


def n_in_map(g, xy, pose):
    """Points of the scan inside level g at the window-frame pose (MapProperties.cs:83-87), in binary64: a count for the control."""
    c, s = math.cos(float(pose[2])), math.sin(float(pose[2]))
    mx = (float(pose[0]) + c * xy[:, 0].astype(np.float64) - s * xy[:, 1]) / g.cell_len
    my = (float(pose[1]) + s * xy[:, 0].astype(np.float64) + c * xy[:, 1]) / g.cell_len
    return int(((mx >= 0) & (mx <= g.w - 2) & (my >= 0) & (my <= g.h - 2)).sum())


class CheckerProcessor:
    """The reference's Update (HectorSLAMProcessor.cs:86-126) on the checker's grids, in the window's frame, with the scroll rule
    of slamhip_hsproc_set_scroll restated: poses in, out and stored as the issue states them, one binary32 rounding per
    operation."""

    def __init__(self, oc, trigger):
        self.oc, self.trigger = oc, trigger
        self.ref = oc.make_pyramid(CELL, W, W, LEVELS)
        self.match = START.copy()                                          # window frame
        self.last = np.full(3, np.finfo(np.float32).min, np.float32)       # float.MinValue
        self.ox = self.oy = 0
        self.stm0 = F(1.0) / F(CELL)
        self.n_shifts = 0

    def offset(self):
        return np.array([F(self.ox) * F(CELL), F(self.oy) * F(CELL), 0.0], np.float32)

    def world(self, pose_win):
        return (np.asarray(pose_win, np.float32) + self.offset()).astype(np.float32)

    def update(self, xy, hint_world, match_fn):
        """match_fn(hint_win) -> window-frame pose.  Returns (updated, (qx, qy))."""
        hint_win = (np.asarray(hint_world, np.float32) - self.offset()).astype(np.float32)
        self.match = np.asarray(match_fn(hint_win), np.float32).copy()
        updated = moved_enough(self.oc, self.match, self.last)
        if updated:
            for g in self.ref:
                g.set_prob_table(None)
                g.update_by_scan(xy, self.match)
            self.last = self.match.copy()
        q = [0, 0]
        if self.trigger > 0:
            for a in range(2):
                c = int(np.floor(F(self.match[a]) * self.stm0))
                d = c - W // 2
                if abs(d) > self.trigger:
                    q[a] = int(d / G) * G                                  # C division: toward zero
            if q[0] or q[1]:
                shift_checker(self.ref, q[0], q[1])
                self.ox += q[0]; self.oy += q[1]
                self.n_shifts += 1
                for a in range(2):
                    m = F(F(q[a]) * F(CELL))
                    self.match[a] = F(self.match[a]) - m
                    with np.errstate(over="ignore"):
                        self.last[a] = F(self.last[a]) - m
        return updated, tuple(q)

    def centre_offset(self):
        return [abs(int(np.floor(F(self.match[a]) * self.stm0)) - W // 2) for a in range(2)]

    def close(self):
        for g in self.ref:
            g.close()


def checker_alone(oc, sim, trigger):
    """The drive on the checker alone (its own match decides the pose): -> (checker, in-map counts per scan on level 0)."""
    ck = CheckerProcessor(oc, trigger)
    counts = []
    hint = START.copy()
    for i, (tp, xy) in enumerate(drive(sim)):
        hint = (hint + odometry(i, sim)).astype(np.float32)
        ck.update(xy, hint, lambda hw: oc.match_pyramid(ck.ref, xy, hw, ITERS, n_threads=1))
        counts.append(n_in_map(ck.ref[0], xy, ck.match))
        hint = ck.world(ck.match)
    return ck, counts


def test_drive_leaves_a_fixed_window(det, sim):
    """The control, on the CPU with the checker alone: without scrolling this drive leaves the window -- no point of the last
    scans lies in the map -- and with scrolling it stays inside and keeps its scans in the map."""
    fixed, counts = checker_alone(det, sim, 0)
    assert counts[0] > RAYS // 4 and max(counts[-10:]) == 0, counts
    assert fixed.n_shifts == 0 and (fixed.ox, fixed.oy) == (0, 0)
    fixed.close()
    scrolled, counts = checker_alone(det, sim, TRIGGER)
    assert min(counts) > RAYS // 4, counts
    assert scrolled.n_shifts >= 3 and scrolled.ox >= W
    err = scrolled.world(scrolled.match) - drive(sim)[-1][0]
    assert math.hypot(err[0], err[1]) < 0.2, err                           # it still knows where it is
    scrolled.close()


@gpu
def test_processor_scrolls_and_keeps_mapping(hs_mod, ctx, det, sim):
    oc = det
    proc = hs_mod.HectorSLAMProcessor(CELL, (W, W), START, LEVELS, 1, ctx=ctx, referenceSummation=True, scrollTrigger=TRIGGER)
    ck = CheckerProcessor(oc, TRIGGER)
    tables = checked_tables(proc.MapRep, ck.ref)
    hint = START.copy()
    n_updates = 0
    for i, (tp, xy) in enumerate(drive(sim)):
        hint = (hint + odometry(i, sim)).astype(np.float32)
        pin(ck.ref, tables)
        origin_before = proc.get_origin()
        assert origin_before == (ck.ox, ck.oy)
        updated = proc.Update(hs_mod.ScanCloud(xy), hint)
        want_updated, q = ck.update(xy, hint, lambda hw: oc.match_pyramid(ck.ref, xy, hw, ITERS, n_threads=1))
        origin = proc.get_origin()
        assert origin == (ck.ox, ck.oy) == (origin_before[0] + q[0], origin_before[1] + q[1]), (i, origin, q)
        got = proc.MatchPose
        assert same_bits(got, ck.world(ck.match)), (i, got, ck.world(ck.match))
        assert updated == want_updated, i
        assert same_bits(proc.LastMapUpdatePose, ck.world(ck.last)), i
        n_updates += updated
        off = ck.centre_offset()
        assert off[0] <= TRIGGER + G and off[1] <= TRIGGER + G, (i, off)
        if q != (0, 0) or i == N_SCANS - 1:
            for l in range(LEVELS):
                assert np.array_equal(raw(proc.MapRep.Maps[l].GetCells()), raw(ck.ref[l].cells)), (i, l)
        # the probabilities the next match reads: after an update from the device, compared with the cells as they lie NOW (behind
        # the shift, if there was one); across a shift alone by rule, bit for bit
        if q != (0, 0):
            for l, g in enumerate(ck.ref):
                band = shifted(np.zeros(g.w * g.h, np.int8), g.w, g.h, q[0] >> l, q[1] >> l, 1).astype(bool)
                assert band.any() and (device_prob(proc.MapRep, l)[band] == F(0.5)).all(), (i, l)
        if updated:
            tables = checked_tables(proc.MapRep, ck.ref)
        elif q != (0, 0):
            tables = shift_tables(ck.ref, tables, q[0], q[1])
            for l in range(LEVELS):
                assert same_bits(device_prob(proc.MapRep, l), tables[l]), (i, l)
        hint = got.copy()
    assert ck.n_shifts >= 3
    assert 40 < n_updates < N_SCANS                                        # gated and ungated scans both
    final = proc.MatchPose
    assert math.hypot(final[0] - START[0], final[1] - START[1]) > W * CELL
    err = final - drive(sim)[-1][0]
    assert math.hypot(err[0], err[1]) < 0.2, err
    proc.Reset()                                                           # the setting survives, the origin does not
    assert proc.get_origin() == (0, 0) and same_bits(proc.MatchPose, START)
    proc.Dispose()
    ck.close()


# ---- 7. scrolling off changes nothing --------------------------------------------------------------------------------------------
@gpu
def test_scroll_off_changes_nothing(hs_mod, ctx, sim):
    """scrollTrigger = 0 against the mirror without the argument: the same poses, cells and numbers of K4 and K5 launches."""
    capi = hs_mod.capi
    runs = []
    for kw in ({}, {"scrollTrigger": 0}):
        proc = hs_mod.HectorSLAMProcessor(CELL, (W, W), START, LEVELS, 1, ctx=ctx, **kw)
        ctx.timing_enable(-1)
        ctx.timing_reset()
        poses = []
        hint = START.copy()
        for i, (tp, xy) in enumerate(drive(sim)[:20]):
            hint = (hint + odometry(i, sim)).astype(np.float32)
            upd = proc.Update(hs_mod.ScanCloud(xy), hint)
            hint = proc.MatchPose.copy()
            poses.append((hint, upd, proc.LastMapUpdatePose.copy()))
        cells = [proc.MapRep.Maps[l].GetCells() for l in range(LEVELS)]
        launches = (ctx.timing_get(capi.K_HS_MATCH)[1], ctx.timing_get(capi.K_HS_UPDATE)[1])
        ctx.timing_enable(0)
        assert proc.get_origin() == (0, 0)
        runs.append((poses, cells, launches))
        proc.Dispose()
    (pa, ca, la), (pb, cb, lb) = runs
    for (ma, ua, lasta), (mb, ub, lastb) in zip(pa, pb):
        assert same_bits(ma, mb) and ua == ub and same_bits(lasta, lastb)
    for l in range(LEVELS):
        assert np.array_equal(raw(ca[l]), raw(cb[l])), l
    assert la == lb and la[0] > 0 and la[1] > 0, (la, lb)
