"""The backing store of the scrolling window (slamhip_hs_set_backing, slamhip_hs_world_cells_download) against a NumPy model,
bit for bit.

The model is a "world canvas" per level: a dense array with an offset, filled with LogOddsCell.Reset() (UpdateIndex -1, Value 0.0f)
and probability 0.5f.  On a shift the old window is written into the canvas and the new window is read out of it; updates and
matches go through the checker in the window's frame, exactly as in test_gpu_hector_shift.py -- including its rule for the
probabilities: a table is taken from the device only after it was compared with the cells' values in binary64 (PROB_ATOL), and
across a shift alone it is never taken from the device at all -- it goes through the canvas like the cells, and the device must
equal it bit for bit.  (The processor test, where an update and a shift can fall into one scan, keeps a table entry "unknown"
from the moment the checker's update changes its cell until the device's value for it has passed that comparison.)

Maps: 64 x 64 and 70 x 46 with 3 levels and tiles of 16 cells: level 0 spans several tiles, the coarsest level (16 x 16, 17 x 11)
straddles one as soon as the origin is no multiple of 64; 70 x 46 has levels 35 x 23 and 17 x 11 -- rows that are no multiple of
a 16-byte unit on either side."""
import math

import numpy as np
import pytest

import test_gpu_hector_shift as S
from test_gpu_hector_shift import hs_mod, ctx, det                         # noqa: F401 (fixtures)

gpu = pytest.mark.gpu

F = np.float32
CELL, LEVELS, G, ITERS = S.CELL, S.LEVELS, S.G, S.ITERS
TILE = 16
SLOT = 12 * TILE * TILE
ENOUGH = 4 << 20
DIMS = [(64, 64), (70, 46)]
DIM_IDS = ["64x64", "70x46"]


def up(v):
    """Away from zero to the next multiple of g (the clearing entries of shifts_of on maps whose size is no multiple of g)."""
    return int(math.copysign(-(-abs(v) // G) * G, v)) if v else 0


def reset_cells(shape, dtype):
    a = np.zeros(shape, dtype)
    a["update_index"] = -1
    return a


class Canvas:
    """Per level a dense world array around the origin: cells (Reset) and probabilities (0.5f); world cell X lies at index
    X + half on each axis."""

    def __init__(self, ref, reach):
        self.half = [(reach >> l) + 2 for l in range(len(ref))]
        self.cells = [reset_cells((2 * h, 2 * h), g.cells.dtype) for g, h in zip(ref, self.half)]
        self.prob = [np.full((2 * h, 2 * h), 0.5, np.float32) for h in self.half]

    def _sl(self, l, OX, OY, w, h):
        x, y = OX + self.half[l], OY + self.half[l]
        assert 0 <= x and x + w <= 2 * self.half[l] and 0 <= y and y + h <= 2 * self.half[l], (l, OX, OY)
        return (slice(y, y + h), slice(x, x + w))

    def write(self, l, OX, OY, cells, table, w, h):
        sl = self._sl(l, OX, OY, w, h)
        self.cells[l][sl] = np.asarray(cells).reshape(h, w)
        self.prob[l][sl] = np.asarray(table, np.float32).reshape(h, w)

    def read(self, l, OX, OY, w, h):
        sl = self._sl(l, OX, OY, w, h)
        return self.cells[l][sl].copy().ravel(), self.prob[l][sl].copy().ravel()

    def shift(self, ref, tables, origin, dx, dy):
        """The model's shift: the old window into the canvas, the new one out of it.  -> the new tables."""
        out = []
        for l, g in enumerate(ref):
            self.write(l, origin[0] >> l, origin[1] >> l, g.cells, tables[l], g.w, g.h)
            c, p = self.read(l, (origin[0] + dx) >> l, (origin[1] + dy) >> l, g.w, g.h)
            g.cells[:] = c
            out.append(p)
        return out


def build_at(hs_mod, ctx, oc, sim, dims, origin, backing=(TILE, ENOUGH)):
    """S.build's filled map, made in a window that was first moved (empty) to `origin`, with backing on from the start."""
    w0, h0 = dims
    rep = hs_mod.MapRepMultiMap(CELL, dims, LEVELS, ctx=ctx)
    if backing:
        rep.set_backing(*backing)
    if origin != (0, 0):
        rep.shift(*origin)
    ref = oc.make_pyramid(CELL, w0, h0, LEVELS)
    for xy, p in S.local_scans(sim, w0, h0):
        rep.UpdateByScan(hs_mod.ScanCloud(xy), p)
        for g in ref:
            g.update_by_scan(xy, p)
    for l in range(LEVELS):
        assert np.array_equal(S.raw(rep.Maps[l].GetCells()), S.raw(ref[l].cells)), l
    assert np.count_nonzero(ref[0].cells["value"]) > (w0 * h0) // 8
    assert rep.origin() == origin
    return rep, ref


def assert_tables_on_device(rep, tables, tag):
    for l, t in enumerate(tables):
        assert S.same_bits(S.device_prob(rep, l), t), (tag, l)


# ---- 1. round trip keeps the map -------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("origin", [(0, 0), (-52, -36)], ids=["o0", "oneg"])
@pytest.mark.parametrize("dims", DIMS, ids=DIM_IDS)
def test_round_trip_keeps_the_map(hs_mod, ctx, det, sim, checksum_np, dims, origin):
    w0, h0 = dims
    rep, ref = build_at(hs_mod, ctx, det, sim, dims, origin)
    tables0 = S.checked_tables(rep, ref)
    for dx, dy in S.shifts_of(w0, h0):
        dx, dy = (up(dx), up(dy)) if (dx % G or dy % G) else (dx, dy)
        rep.shift(dx, dy)
        assert rep.origin() == (origin[0] + dx, origin[1] + dy)
        if abs(dx) >= w0 or abs(dy) >= h0:                                 # (the window did go empty in between)
            assert all((rep.Maps[l].GetCells()["update_index"] == -1).all() for l in range(LEVELS))
        rep.shift(-dx, -dy)
        assert rep.origin() == origin
        S.assert_maps_equal(rep, ref, checksum_np, (dx, dy))               # the ORIGINAL: ref was never touched
        S.assert_prob_equal(rep, ref, tables0, (dx, dy))
    st = rep.backing_stats()
    assert st["on"] == 1 and st["tile"] == TILE and st["tiles"] > 0 and st["dropped_cells"] == 0
    assert st["evicted_cells"] > 0 and st["restored_cells"] > 0 and SLOT <= st["bytes"] <= st["capacity_bytes"] == ENOUGH
    S.close_all(rep, ref)


# ---- 2. a walk -------------------------------------------------------------------------------------------------------------------
def walk_steps(w0, h0):
    """Both axes, both signs, one clearing move (and the way back over it), returns over earlier ground; "u": an UpdateByScan in
    the window's frame."""
    far = up(w0) + G
    return [(G, 0), "u", (0, -G), (2 * G, 2 * G), "u", (-3 * G, G), (0, 3 * G), (-2 * G, -4 * G), "u", (far, 0), "u", (-far, 0),
            (4 * G, -2 * G), (-2 * G, 2 * G), "u", (-2 * G, 0)]


def walk(hs_mod, ctx, oc, sim, checksum_np, dims):
    w0, h0 = dims
    rep, ref = build_at(hs_mod, ctx, oc, sim, dims, (0, 0))
    canvas = Canvas(ref, 4 * max(w0, h0))
    tables = S.checked_tables(rep, ref)
    origin = (0, 0)
    scans = S.local_scans(sim, w0, h0)
    n_u = 0
    for step in walk_steps(w0, h0):
        if step == "u":
            xy, p = scans[(3 * n_u + 1) % len(scans)]
            n_u += 1
            rep.UpdateByScan(hs_mod.ScanCloud(xy), p)
            for g in ref:
                g.set_prob_table(None)
                g.update_by_scan(xy, p)
            for l in range(LEVELS):
                assert np.array_equal(S.raw(rep.Maps[l].GetCells()), S.raw(ref[l].cells)), (step, l)
            tables = S.checked_tables(rep, ref)
            continue
        dx, dy = step
        rep.shift(dx, dy)
        tables = canvas.shift(ref, tables, origin, dx, dy)
        origin = (origin[0] + dx, origin[1] + dy)
        assert rep.origin() == origin
        S.assert_maps_equal(rep, ref, checksum_np, step)
        S.assert_prob_equal(rep, ref, tables, step)
    assert rep.backing_stats()["dropped_cells"] == 0
    return rep, ref, canvas, tables, origin


@gpu
@pytest.mark.parametrize("dims", DIMS, ids=DIM_IDS)
def test_walk(hs_mod, ctx, det, sim, checksum_np, dims):
    oc = det
    rep, ref, canvas, tables, origin = walk(hs_mod, ctx, oc, sim, checksum_np, dims)
    assert np.count_nonzero(ref[0].cells["value"]) > (dims[0] * dims[1]) // 8   # the walk came home to a map
    S.pin(ref, tables)
    xy, p = S.local_scans(sim, *dims)[-1]
    p_win = np.array([p[0] - F(origin[0]) * F(CELL), p[1] - F(origin[1]) * F(CELL), p[2]], np.float32)
    scan = hs_mod.ScanCloud(xy)
    m1 = hs_mod.ScanMatcher(1, referenceSummation=True)
    for d in ((0, 0, 0), (0.03, -0.02, 0.02), (-0.04, 0.03, -0.03)):
        hint = p_win + np.array(d, np.float32)
        got = m1.MatchData(rep, scan, hint)
        want = oc.match_pyramid(ref, xy, hint, ITERS, n_threads=1)
        assert S.same_bits(got, want), (hint, got, want)
        assert not S.same_bits(got, hint)
    S.close_all(rep, ref)


# ---- 3. the world download -------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dims", DIMS, ids=DIM_IDS)
def test_world_download(hs_mod, ctx, det, sim, checksum_np, dims):
    w0, h0 = dims
    rep, ref, canvas, tables, origin = walk(hs_mod, ctx, det, sim, checksum_np, dims)
    for l, g in enumerate(ref):                                            # everything visited plus a margin: the canvas itself
        canvas.write(l, origin[0] >> l, origin[1] >> l, g.cells, tables[l], g.w, g.h)
        n = 2 * canvas.half[l]
        got = rep.world_cells(l, -canvas.half[l], -canvas.half[l], n, n)
        assert np.array_equal(S.raw(got), S.raw(canvas.cells[l])), l
        assert (got["update_index"][0] == -1).all() and (got["value"][:, -1] == 0).all()   # (Reset out there)
    # evict a band (half of the window), return, update it, download: the window's values win over the tile's older copy
    rep.shift(8 * G, 0)
    tables = canvas.shift(ref, tables, origin, 8 * G, 0)
    rep.shift(-8 * G, 0)
    tables = canvas.shift(ref, tables, (origin[0] + 8 * G, origin[1]), -8 * G, 0)
    xy, p = S.local_scans(sim, w0, h0)[2]
    band_before = [g.cells.reshape(g.h, g.w)[:, :(8 * G) >> l].copy() for l, g in enumerate(ref)]
    rep.UpdateByScan(hs_mod.ScanCloud(xy), p)
    for g in ref:
        g.set_prob_table(None)
        g.update_by_scan(xy, p)
    assert any((S.raw(g.cells.reshape(g.h, g.w)[:, :(8 * G) >> l]) != S.raw(band_before[l])).any() for l, g in enumerate(ref))
    for l, g in enumerate(ref):
        got = rep.world_cells(l, (origin[0] >> l) - 3, (origin[1] >> l) - 2, g.w + 5, g.h + 4)
        want = reset_cells((g.h + 4, g.w + 5), g.cells.dtype)
        c, _ = canvas.read(l, (origin[0] >> l) - 3, (origin[1] >> l) - 2, g.w + 5, g.h + 4)
        want[...] = c.reshape(g.h + 4, g.w + 5)
        want[2:2 + g.h, 3:3 + g.w] = g.cells.reshape(g.h, g.w)
        assert np.array_equal(S.raw(got), S.raw(want)), l
    # backing off: the window in a frame of Reset cells
    rep.set_backing(0, 0)
    for l, g in enumerate(ref):
        got = rep.world_cells(l, (origin[0] >> l) - 20, (origin[1] >> l) - 20, g.w + 40, g.h + 40)
        want = reset_cells((g.h + 40, g.w + 40), g.cells.dtype)
        want[20:20 + g.h, 20:20 + g.w] = g.cells.reshape(g.h, g.w)
        assert np.array_equal(S.raw(got), S.raw(want)), l
    with pytest.raises(hs_mod.capi.SlamhipError) as e:
        rep.world_cells(0, 0, 0, 1 << 14, (1 << 12) + 1)                   # past the bound of 2^26 cells
    assert e.value.code == hs_mod.capi.ERR_INVALID
    S.close_all(rep, ref)


# ---- 4. capacity -----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dims", DIMS, ids=DIM_IDS)
def test_capacity(hs_mod, ctx, det, sim, dims):
    capi = hs_mod.capi
    w0, h0 = dims
    rep, ref = build_at(hs_mod, ctx, det, sim, dims, (0, 0), backing=(TILE, 2 * SLOT))
    orig = [g.cells.copy() for g in ref]
    dx = up(w0)
    plan_out = capi.backing_plan(LEVELS, w0, h0, 0, 0, dx, 0, TILE)
    plan_back = capi.backing_plan(LEVELS, w0, h0, dx, 0, -dx, 0, TILE)
    area = lambda jobs: int((jobs["nx"].astype(np.int64) * jobs["ny"])[jobs["kind"] == capi.BACKING_EVICT].sum())
    rep.shift(dx, 0)                                                       # SLAMHIP_OK (anything else raises)
    st = rep.backing_stats()
    assert st["bytes"] <= st["capacity_bytes"] == 2 * SLOT and st["tiles"] == 2
    assert st["dropped_cells"] > 0 and st["evicted_cells"] + st["dropped_cells"] == area(plan_out)
    rep.shift(-dx, 0)
    st = rep.backing_stats()
    assert st["bytes"] <= st["capacity_bytes"] and st["tiles"] == 2
    assert st["evicted_cells"] + st["dropped_cells"] == area(plan_out) + area(plan_back)
    first = plan_out[plan_out["kind"] == capi.BACKING_EVICT][:2]
    assert (first["level"] == 0).all()
    assert st["evicted_cells"] == int((first["nx"] * first["ny"]).sum()) == st["restored_cells"]
    for l, g in enumerate(ref):
        got = rep.Maps[l].GetCells().reshape(g.h, g.w)
        want = reset_cells((g.h, g.w), g.cells.dtype)
        if l == 0:
            for j in first:                                                # the cells of the first two jobs in plan order: the original
                sl = (slice(j["wy"], j["wy"] + j["ny"]), slice(j["wx"], j["wx"] + j["nx"]))
                want[sl] = orig[0].reshape(g.h, g.w)[sl]
            assert (S.raw(want) != S.raw(reset_cells((g.h, g.w), g.cells.dtype))).any()
        is_orig = S.raw(got) == S.raw(orig[l].reshape(g.h, g.w))
        is_reset = (got["update_index"] == -1) & (got["value"].view(np.uint32) == 0)
        assert (is_orig | is_reset).all(), l                               # every cell either the original or Reset
        assert np.array_equal(S.raw(got), S.raw(want)), l
    S.close_all(rep, ref)


# ---- 4b. jobs of more than one piece ----------------------------------------------------------------------------------------------
BIG_DIMS, BIG_TILE, BIG_SHIFT = (128, 128), 64, (-68, 72)


@gpu
@pytest.mark.parametrize("origin", [(0, 0), (-52, -36)], ids=["o0", "oneg"])
def test_jobs_of_two_pieces(hs_mod, ctx, det, sim, checksum_np, origin):
    """Tiles of 64 cells under a window of 128: evict and restore jobs of 64 x 64 and 64 x 56 cells (origin (0, 0)) or 64 x 36
    (origin (-52, -36), from row 28 of their tiles) -- more than the 2048 cells of a piece, so k6_page gets each as two
    workgroups' pieces, the second from row `rows` of the job and of the tile.  Out and back, cells and probabilities bit for bit."""
    capi = hs_mod.capi
    jobs = capi.backing_plan(LEVELS, *BIG_DIMS, *origin, *BIG_SHIFT, BIG_TILE)
    big = jobs[jobs["nx"].astype(np.int64) * jobs["ny"] > 2048]
    assert set(big["kind"].tolist()) == {capi.BACKING_EVICT, capi.BACKING_RESTORE}
    if origin == (0, 0):
        assert len(jobs) == 24 and {(64, 64), (64, 56)} <= set(zip(big["nx"].tolist(), big["ny"].tolist()))
    else:
        assert (big["ly"] > 0).any()                                       # a second piece at ly + r0 with ly > 0
    rep, ref = build_at(hs_mod, ctx, det, sim, BIG_DIMS, origin, backing=(BIG_TILE, ENOUGH))
    canvas = Canvas(ref, 4 * BIG_DIMS[0])
    tables = S.checked_tables(rep, ref)
    at = origin
    for dx, dy in (BIG_SHIFT, (-BIG_SHIFT[0], -BIG_SHIFT[1])):
        rep.shift(dx, dy)
        tables = canvas.shift(ref, tables, at, dx, dy)
        at = (at[0] + dx, at[1] + dy)
        assert rep.origin() == at
        S.assert_maps_equal(rep, ref, checksum_np, (dx, dy))
        S.assert_prob_equal(rep, ref, tables, (dx, dy))
    assert at == origin and np.count_nonzero(ref[0].cells["value"]) > (BIG_DIMS[0] * BIG_DIMS[1]) // 8   # home, with the map
    st = rep.backing_stats()
    assert st["dropped_cells"] == 0 and st["restored_cells"] > 0 and st["tile"] == BIG_TILE
    S.close_all(rep, ref)


# ---- 5. off is today -------------------------------------------------------------------------------------------------------------
ZERO_STATS = dict(tiles=0, bytes=0, capacity_bytes=0, evicted_cells=0, restored_cells=0, dropped_cells=0, tile=0, on=0)


@gpu
@pytest.mark.parametrize("was_on", [False, True], ids=["never", "switched_off"])
def test_off_is_today(hs_mod, ctx, det, sim, checksum_np, was_on):
    rep, ref = build_at(hs_mod, ctx, det, sim, (70, 46), (0, 0), backing=None)
    if was_on:
        rep.set_backing(TILE, ENOUGH)
        rep.shift(G, 0); rep.shift(-G, 0)                                  # (tiles exist, and the round trip kept the map)
        S.assert_maps_equal(rep, ref, checksum_np, "on")
        assert rep.backing_stats()["tiles"] > 0
        rep.set_backing(TILE, 0)
    assert rep.backing_stats() == ZERO_STATS
    tables = S.checked_tables(rep, ref)
    lost = [0] * LEVELS                                                    # mapped cells the two round trips cleared, per level
    for dx, dy in ((G, 0), (-2 * G, 3 * G)):                               # test_round_trip's expectation: the bands cleared
        orig = [g.cells.copy() for g in ref]
        rep.shift(dx, dy)
        rep.shift(-dx, -dy)
        for l, g in enumerate(ref):
            once = S.shifted(orig[l], g.w, g.h, dx >> l, dy >> l, (-1, 0.0))
            g.cells[:] = S.shifted(once, g.w, g.h, (-dx) >> l, (-dy) >> l, (-1, 0.0))
            lost[l] += int((S.raw(g.cells) != S.raw(orig[l])).sum())
        tables = S.shift_tables(ref, S.shift_tables(ref, tables, dx, dy), -dx, -dy)
        S.assert_maps_equal(rep, ref, checksum_np, (dx, dy))
        S.assert_prob_equal(rep, ref, tables, (dx, dy))
    assert all(n > 0 for n in lost), lost                                  # (the second trip's bands do hold mapped cells: today's loss)
    assert rep.backing_stats() == ZERO_STATS
    S.close_all(rep, ref)


@gpu
def test_setting_and_reset(hs_mod, ctx, det, sim):
    capi = hs_mod.capi
    rep, ref = build_at(hs_mod, ctx, det, sim, (64, 64), (0, 0), backing=None)
    orig = [g.cells.copy() for g in ref]
    for tile, mb in ((4, ENOUGH), (12, ENOUGH), (512, ENOUGH), (16, SLOT - 1)):
        with pytest.raises(capi.SlamhipError) as e:
            rep.set_backing(tile, mb)
        assert e.value.code == capi.ERR_INVALID and rep.backing_stats() == ZERO_STATS
    rep.set_backing(TILE, ENOUGH)
    D = 8 * G                                                              # half of the window: a band that does hold mapped cells
    rep.shift(-D, 0)                                                       # window cells x < D >> l lie at world X < 0 now
    for l in range(LEVELS):
        rep.Maps[l].SetCells(orig[l])                                      # (the window only)
    rep.shift(D, 0)                                                        # ... and are evicted
    st = rep.backing_stats()
    assert st["tiles"] > 0 and st["evicted_cells"] > 0
    with pytest.raises(capi.SlamhipError) as e:
        rep.set_backing(2 * TILE, ENOUGH)                                  # tiles exist: the tile size cannot change
    assert e.value.code == capi.ERR_INVALID and rep.backing_stats() == st
    rep.shift(-D, 0)                                                       # the tiles do hold the band
    for l, g in enumerate(ref):
        b = D >> l
        got = rep.Maps[l].GetCells().reshape(g.h, g.w)
        assert np.array_equal(S.raw(got[:, :b]), S.raw(orig[l].reshape(g.h, g.w)[:, :b])), l
        assert np.count_nonzero(got["value"][:, :b]) > 0, l
    rep.shift(D, 0)
    restored = rep.backing_stats()["restored_cells"]
    assert restored > 0
    rep.Reset()                                                            # the setting survives, the tiles do not
    st = rep.backing_stats()
    assert st["on"] == 1 and st["tile"] == TILE and st["tiles"] == 0 and st["capacity_bytes"] == ENOUGH and rep.origin() == (0, 0)
    rep.shift(-D, 0)                                                       # the same world cells come in: nothing to restore
    assert rep.backing_stats()["restored_cells"] == restored
    for l in range(LEVELS):
        got = rep.Maps[l].GetCells()
        assert (got["update_index"] == -1).all() and (got["value"].view(np.uint32) == 0).all(), l
    rep.set_backing(0, 0)                                                  # off, then on with another tile size
    assert rep.backing_stats() == ZERO_STATS
    rep.set_backing(2 * TILE, ENOUGH)
    assert rep.backing_stats()["tile"] == 2 * TILE and rep.backing_stats()["bytes"] == 0
    S.close_all(rep, ref)


# ---- 6. the processor drives out and back ----------------------------------------------------------------------------------------
W, TRIGGER, START = S.W, S.TRIGGER, S.START


_BACK = {}


def out_and_back(sim):
    """S.drive's 80 poses out (22 m, 1.7 windows), then the robot turns round and drives over the same positions back, its
    forward-looking lidar now facing the ground it came over (scans made once, as S.drive's are)."""
    if "d" not in _BACK:
        d = S.drive(sim)
        segs = S.corridor()
        rng = sim.PCG32(78)
        back = []
        for k, (tp, _) in enumerate(d[::-1]):
            tb = np.array([tp[0], tp[1], 3.0 + 0.02 * math.sin(0.2 * k)], np.float32)
            xy = sim.make_scan(segs, tb, 2 * S.RAYS, rng)[1]
            back.append((tb, np.ascontiguousarray(xy[xy[:, 0] > 0.2])))
        _BACK["d"] = d + back
    return _BACK["d"]


class CanvasProcessor(S.CheckerProcessor):
    """S.CheckerProcessor with the canvas in its shift (canvas=None: its own Reset-filling shift), and the probability tables
    carried along: NaN marks an entry whose cell the checker's update changed and whose device value has not been seen yet."""

    def __init__(self, oc, trigger, with_canvas, with_tables):
        super().__init__(oc, trigger)
        self.canvas = Canvas(self.ref, 4 * W) if with_canvas else None
        self.tables = [np.full(g.w * g.h, 0.5, np.float32) for g in self.ref] if with_tables else None
        self.after_shift = []                                              # level-0 count of non-Reset cells just after each shift

    def update(self, xy, hint_world, match_fn):
        hint_win = (np.asarray(hint_world, np.float32) - self.offset()).astype(np.float32)
        self.match = np.asarray(match_fn(hint_win), np.float32).copy()
        updated = S.moved_enough(self.oc, self.match, self.last)
        if updated:
            before = [g.cells.copy() for g in self.ref]
            for g in self.ref:
                g.set_prob_table(None)
                g.update_by_scan(xy, self.match)
            if self.tables is not None:
                for l, g in enumerate(self.ref):
                    self.tables[l][S.raw(g.cells) != S.raw(before[l])] = np.nan
            self.last = self.match.copy()
        q = [0, 0]
        for a in range(2):
            c = int(np.floor(F(self.match[a]) * self.stm0))
            d = c - W // 2
            if abs(d) > self.trigger:
                q[a] = int(d / G) * G                                      # C division: toward zero
        if q[0] or q[1]:
            tabs = self.tables if self.tables is not None else [np.full(g.w * g.h, 0.5, np.float32) for g in self.ref]
            if self.canvas is not None:
                tabs = self.canvas.shift(self.ref, tabs, (self.ox, self.oy), q[0], q[1])
            else:
                S.shift_checker(self.ref, q[0], q[1])
                tabs = S.shift_tables(self.ref, tabs, q[0], q[1])
            if self.tables is not None:
                self.tables = tabs
            self.ox += q[0]; self.oy += q[1]
            self.n_shifts += 1
            c0 = self.ref[0].cells
            self.after_shift.append(int(((c0["update_index"] != -1) | (c0["value"].view(np.uint32) != 0)).sum()))
            for a in range(2):
                m = F(F(q[a]) * F(CELL))
                self.match[a] = F(self.match[a]) - m
                with np.errstate(over="ignore"):
                    self.last[a] = F(self.last[a]) - m
        return updated, tuple(q)


def checker_out_and_back(oc, sim, with_canvas):
    ck = CanvasProcessor(oc, TRIGGER, with_canvas, False)
    d = out_and_back(sim)
    hint = START.copy()
    shifts_at = []
    for i, (tp, xy) in enumerate(d):
        if i:
            hint = (hint + (tp - d[i - 1][0]).astype(np.float32)).astype(np.float32)
        _, q = ck.update(xy, hint, lambda hw: oc.match_pyramid(ck.ref, xy, hw, ITERS, n_threads=1))
        if q != (0, 0):
            shifts_at.append(i)
        hint = ck.world(ck.match)
    return ck, shifts_at


def test_coming_back_finds_the_map(det, sim):
    """The control, on the CPU with the checker alone: on the way back every shift brings more mapped cells into the window with
    the canvas than without it, and the robot knows where it is at the end in both runs."""
    n_out = len(S.drive(sim))
    runs = {}
    for with_canvas in (False, True):
        ck, at = checker_out_and_back(det, sim, with_canvas)
        err = ck.world(ck.match) - out_and_back(sim)[-1][0]
        assert math.hypot(err[0], err[1]) < 0.2, (with_canvas, err)
        assert (ck.ox, ck.oy) != (0, 0) or ck.n_shifts >= 6
        runs[with_canvas] = [(i, n) for i, n in zip(at, ck.after_shift) if i >= n_out]
        ck.close()
    assert len(runs[True]) >= 3 and [i for i, _ in runs[True]] == [i for i, _ in runs[False]], runs
    for (i, n_canvas), (_, n_plain) in zip(runs[True], runs[False]):
        assert n_canvas > n_plain, (i, n_canvas, n_plain)


@gpu
def test_processor_out_and_back(hs_mod, ctx, det, sim):
    oc = det
    proc = hs_mod.HectorSLAMProcessor(CELL, (W, W), START, LEVELS, 1, ctx=ctx, referenceSummation=True, scrollTrigger=TRIGGER,
                                      scrollBacking=(TILE, 64 << 20))
    ck = CanvasProcessor(oc, TRIGGER, True, True)
    ck.tables = S.checked_tables(proc.MapRep, ck.ref)
    d = out_and_back(sim)
    hint = START.copy()
    n_back_shifts = 0
    for i, (tp, xy) in enumerate(d):
        if i:
            hint = (hint + (tp - d[i - 1][0]).astype(np.float32)).astype(np.float32)
        S.pin(ck.ref, ck.tables)
        updated = proc.Update(hs_mod.ScanCloud(xy), hint)
        want_updated, q = ck.update(xy, hint, lambda hw: oc.match_pyramid(ck.ref, xy, hw, ITERS, n_threads=1))
        assert proc.get_origin() == (ck.ox, ck.oy), (i, q)
        got = proc.MatchPose
        assert S.same_bits(got, ck.world(ck.match)), (i, got, ck.world(ck.match))
        assert updated == want_updated, i
        assert S.same_bits(proc.LastMapUpdatePose, ck.world(ck.last)), i
        if q != (0, 0) or i == len(d) - 1:
            n_back_shifts += i >= len(S.drive(sim))
            for l in range(LEVELS):
                assert np.array_equal(S.raw(proc.MapRep.Maps[l].GetCells()), S.raw(ck.ref[l].cells)), (i, l)
        # the probabilities the next match reads: entries the model knows, bit for bit; the others from the device once they have
        # been compared with the cells in binary64
        if updated or q != (0, 0):
            for l, g in enumerate(ck.ref):
                p = S.device_prob(proc.MapRep, l)
                known = ~np.isnan(ck.tables[l])
                assert (p[known].view(np.uint32) == ck.tables[l][known].view(np.uint32)).all(), (i, l)
                with np.errstate(over="ignore"):
                    want = 1.0 / (1.0 + np.exp(-g.cells["value"].astype(np.float64)))
                assert np.abs(p.astype(np.float64) - want).max() <= S.PROB_ATOL, (i, l)
                ck.tables[l] = p
        hint = got.copy()
    assert n_back_shifts >= 3
    st = proc.backing_stats()
    assert st["dropped_cells"] == 0 and st["restored_cells"] > 0 and st["tiles"] > 0
    err = proc.MatchPose - d[-1][0]
    assert math.hypot(err[0], err[1]) < 0.2, err
    proc.Dispose()
    ck.close()
