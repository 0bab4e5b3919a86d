"""GPU tests of the opt-in reference probability cache (slamhip_hs_set_reference_cache; MapRepMultiMap.set_reference_cache,
HectorSLAMProcessor(..., referenceCache=True)): OccGridMap.GetCachedProbability with the reference's own cacheArray
(OccGridMap.cs:16-19,38-42,97-107,147,248), which serves pre-reset probabilities after Reset (deviation D5).

The host-side model is LiteralNpGrid below: NpGrid with the C# cache -- Index -1 from the constructor, the epoch up by one
after every UpdateByScan, Reset sets the epoch to 0 and keeps the entries, an upload touches neither.  It keeps the
LOG-ODDS a fill saw, so the grid a read "sees" is the current cells with every entry that hits replaced by that value
(LiteralNpGrid.effective) -- the grid oc.match_pyramid is run on.  Bit-exact claims are made on quantised maps (values 50
or 0: probabilities exactly 1.0 and 0.5 whatever the expf, tests/test_gpu_hector_refsum.py), tolerances on raw maps."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = np.float32
F_MIN = F(-3.40282347e+38)
POS_TOL = 1e-4
ANG_TOL = 1e-4
PROB_TOL = 2e-7                       # device expf against libm expf (tests/test_gpu_hector.py)
SIDE, CELL, LEVELS, R = 400, 0.1, 2, 360
TRUE_POSE = np.array([20.3, 20.1, 0.1], np.float32)
HINT_OFFS = ((0, 0, 0), (0.1, -0.08, 0.03), (-0.12, 0.1, -0.04))
PATH_A = [np.array([20 + 0.05 * i, 20 + 0.02 * i, 0.01 * i], np.float32) for i in range(8)]
PATH_B = [np.array([20.4 - 0.05 * i, 19.9 + 0.03 * i, 0.25 - 0.02 * i], np.float32) for i in range(8)]


@pytest.fixture(scope="module")
def hs_mod():
    import slam.net_amd.hector as m
    return m


@pytest.fixture(scope="module")
def capi_mod():
    import slam.net_amd.capi as c
    return c


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
    """Equal bit for bit, except that any NaN equals any NaN."""
    a = np.ascontiguousarray(a, np.float32).ravel(); b = np.ascontiguousarray(b, np.float32).ravel()
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all() and (a.view(np.uint32)[~na] == b.view(np.uint32)[~nb]).all())


def quantise_cells(cells):
    cells["value"] = np.where(cells["value"] > 0, np.float32(50.0), np.float32(0.0))


@pytest.fixture(scope="module")
def literal_cls(npo):
    class LiteralNpGrid(npo.NpGrid):
        """NpGrid with OccGridMap's cache (OccGridMap.cs:16-19,38-42,97-107,147,248).  cv holds the log-odds the fill read,
        so the entry's Value is prob(cv).  Only in-range points read taps and fill (ScanMatcher.cs:216-219): NpGrid.interp
        reads cell 0 for the others and masks afterwards, which would fill cell 0 here."""

        def __init__(self, cell_len, w, h):
            super().__init__(cell_len, w, h, trig="det")
            self.cidx = np.full(w * h, -1, np.int64)                     # :38-42
            self.cv = np.zeros(w * h, np.float32)
            self.epoch = 0                                                # :19

        def update_by_scan(self, xy, pose, origin=(0.0, 0.0)):
            super().update_by_scan(xy, pose, origin)
            self.epoch += 1                                               # :147

        def take_update(self, values):
            """An UpdateByScan done elsewhere (the C oracle's grid): its cells, and the epoch moves on."""
            self.value[:] = values
            self.epoch += 1

        def reset(self):                                                  # :244-252 (the cache entries stay)
            self.value[:] = 0.0
            self.upd[:] = -1
            self.cur = 0
            self.epoch = 0

        def _read(self, idx):
            """GetCachedProbability of in-range cells idx (any order: every fill writes the current value)."""
            hit = self.cidx[idx] == self.epoch                            # :99
            miss = idx[~hit]
            self.cv[miss] = self.value[miss]                              # :101-103
            self.cidx[miss] = self.epoch
            odds = np.exp(self.cv[idx].astype(np.float64)).astype(np.float32)
            return (odds / (odds + F(1.0))).astype(np.float32)            # :106

        def effective(self):
            """The log-odds every read in this epoch answers with (the current value where the entry misses)."""
            v = self.value.copy()
            hit = self.cidx == self.epoch
            v[hit] = self.cv[hit]
            return v

        def stale_count(self):
            hit = self.cidx == self.epoch
            return int((self.cv[hit] != self.value[hit]).sum())

        def interp(self, cx, cy):                                         # ScanMatcher.cs:211-249
            cx = np.asarray(cx, np.float32); cy = np.asarray(cy, np.float32)
            with np.errstate(invalid="ignore"):
                oob = np.isnan(cx) | np.isnan(cy) | (cx < 0) | (cx > F(self.w - 2.0)) | (cy < 0) | (cy > F(self.h - 2.0))
            cxs = np.where(oob, F(0), cx); cys = np.where(oob, F(0), cy)
            ix = np.floor(cxs).astype(np.int64); iy = np.floor(cys).astype(np.int64)
            fx = cxs - ix.astype(np.float32); fy = cys - iy.astype(np.float32)
            idx = (iy * self.w + ix)[~oob]
            taps = []
            for off in (0, 1, self.w, self.w + 1):                        # :230-233
                t = np.zeros(cx.shape, np.float32)
                t[~oob] = self._read(idx + off)
                taps.append(t)
            i0, i1, i2, i3 = taps
            xi, yi = F(1.0) - fx, F(1.0) - fy
            P = ((i0 * xi + i1 * fx) * yi) + ((i2 * xi + i3 * fx) * fy)
            gx = -(((i0 - i1) * xi) + ((i2 - i3) * fx))
            gy = -(((i0 - i2) * yi) + ((i1 - i3) * fy))
            z = F(0)
            return np.where(oob, z, P), np.where(oob, z, gx), np.where(oob, z, gy)

    return LiteralNpGrid


def models_for(literal_cls, oc_levels):
    return [literal_cls(np.float32(g.cell_len), g.w, g.h) for g in oc_levels]


@pytest.fixture(scope="module")
def quantised_ab(det, sim):
    """Quantised cells of two pyramids mapped along paths A and B through the same area (overlapping cells that differ)."""
    segs = sim.default_field()
    out = []
    for seed, path in ((21, PATH_A), (22, PATH_B)):
        rng = sim.PCG32(seed)
        g = det.make_pyramid(CELL, SIDE, SIDE, LEVELS)
        for p in path:
            xy = sim.make_scan(segs, p, R, rng)[1]
            for x in g:
                x.update_by_scan(xy, p)
        cells = []
        for x in g:
            c = x.cells.copy()
            quantise_cells(c)
            cells.append(c)
            x.close()
        out.append(cells)
    a, b = out
    assert any((a[l]["value"] != b[l]["value"]).sum() > 100 for l in range(LEVELS))
    rng = sim.PCG32(23)
    xy = sim.make_scan(segs, TRUE_POSE, R, rng)[1]
    xy_u = np.ascontiguousarray(sim.make_scan(segs, PATH_A[0], R, rng)[1][:12])
    return a, b, xy, xy_u


def upload(rep, models, cells):
    for l, c in enumerate(cells):
        rep.Maps[l].SetCells(c)
        if models is not None:
            models[l].value[:] = c["value"]                               # (an upload leaves the cache alone)


def start_literal(hs_mod, ctx, literal_cls, det, ab, T, literal=True):
    """A pyramid (and its models) after: reference cache on, UpdateByScan, upload of quantised A -- epoch 1, no entry filled."""
    a, _, _, xy_u = ab
    rep = hs_mod.MapRepMultiMap(CELL, (SIDE, SIDE), LEVELS, ctx=ctx)
    if literal:
        rep.set_reference_cache(1)
    rep.set_match_threads(T)
    grids = det.make_pyramid(CELL, SIDE, SIDE, LEVELS)
    models = models_for(literal_cls, grids)
    rep.UpdateByScan(hs_mod.ScanCloud(xy_u), PATH_A[0])
    for m in models:
        m.update_by_scan(xy_u, PATH_A[0])
    upload(rep, models, a)
    return rep, grids, models


def reset_update_upload_b(hs_mod, rep, models, ab):
    _, b, _, xy_u = ab
    rep.Reset()
    rep.UpdateByScan(hs_mod.ScanCloud(xy_u), PATH_A[0])
    for m in models:
        m.reset()
        m.update_by_scan(xy_u, PATH_A[0])
    upload(rep, models, b)


def map_pose(m, world):
    return np.array([F(world[0]) * m.stm, F(world[1]) * m.stm, world[2]], np.float32)


def replay_match(det, grids, models, xy, hint, iters, T):
    """ScanMatcher.MatchData(MapRepMultiMap) (:41-84) one iteration at a time: the taps of every iteration are marked in the
    models' caches (LiteralNpGrid.hessian at the iteration's pose), the step is the C oracle's on the effective grids."""
    for g, m in zip(grids, models):
        g.cells["value"][:] = m.effective()
    est_w = np.asarray(hint, np.float32)
    for l in range(len(grids) - 1, -1, -1):
        est = grids[l].map_pose(est_w)
        for _ in range(iters[l]):
            models[l].hessian(xy, est, T)
            _, est = grids[l].estimate_step(xy, est, T)
        est[2] = det.normalize_angle(est[2])
        est_w = grids[l].world_pose(est)
    want = det.match_pyramid(grids, xy, hint, iters, n_threads=T)
    assert same_bits(est_w, want), (est_w, want)
    for g, m in zip(grids, models):
        g.cells["value"][:] = m.value
    return want


# ---- 1. the hand case ----------------------------------------------------------------------------------------------------
def test_hand_case_reset_aliasing(hs_mod, ctx, det, capi_mod):
    """tests/test_oracle_kat.py::test_hector_reset_cache_aliasing_d5 through the library: scan A, query, Reset, scan B --
    the mode serves the pre-reset 0.9 where the default serves 0.4."""
    cell = 10 * 32 + 15
    pose = np.array([10.0, 10.0, 0.0], np.float32)
    scan_a = hs_mod.ScanCloud(np.array([[5.0, 0.0]], np.float32))
    scan_b = hs_mod.ScanCloud(np.array([[8.0, 0.0]], np.float32))
    lit = hs_mod.MapRepMultiMap(1.0, (32, 32), 1, ctx=ctx)
    dfl = hs_mod.MapRepMultiMap(1.0, (32, 32), 1, ctx=ctx)
    lit.set_reference_cache(1)
    g = det.Grid(1.0, 32, 32)
    q = lambda rep: float(rep.Maps[0].GetCachedProbability(cell)[0])
    for rep in (lit, dfl):
        rep.UpdateByScan(scan_a, pose)
    g.update_by_scan(scan_a.Points, pose)
    assert abs(q(lit) - 0.9) < 1e-6 and q(lit) == q(dfl)
    assert abs(q(lit) - g.prob_literal(cell)) <= PROB_TOL
    for rep in (lit, dfl):
        rep.Reset()
        rep.UpdateByScan(scan_b, pose)
    g.reset()
    g.update_by_scan(scan_b.Points, pose)
    assert abs(q(dfl) - 0.4) < 1e-6                                      # the default: the current value's probability
    assert abs(q(lit) - 0.9) < 1e-6                                       # the reference's cache: the map that was reset away
    assert abs(q(lit) - g.prob_literal(cell)) <= PROB_TOL
    for rep in (lit, dfl):                                                # one more scan moves the epoch on: transparent again
        rep.UpdateByScan(scan_b, pose)
    assert q(lit) == q(dfl)

    # a query between Reset and the next scan re-tags the entry with epoch 0: no aliasing
    lit.set_reference_cache(0); lit.set_reference_cache(1)               # (off -> on: a new OccGridMap's cache)
    lit.Reset()
    lit.UpdateByScan(scan_a, pose)
    q(lit)
    lit.Reset()
    assert q(lit) == 0.5
    lit.UpdateByScan(scan_b, pose)
    assert abs(q(lit) - 0.4) < 1e-6

    # without a Reset the cache is transparent: every cell on the ray, after every scan
    lit.set_reference_cache(0); lit.set_reference_cache(1)
    for rep in (lit, dfl):
        rep.Reset()
    cells = np.arange(10 * 32 + 8, 10 * 32 + 20, dtype=np.int32)
    for s in (scan_a, scan_b, scan_a):
        for rep in (lit, dfl):
            rep.UpdateByScan(s, pose)
        assert same_bits(lit.Maps[0].GetCachedProbability(cells), dfl.Maps[0].GetCachedProbability(cells))

    # switching: on -> on keeps the entries; off -> on clears them; a refused value changes nothing
    lit.Reset()
    lit.UpdateByScan(scan_a, pose)
    q(lit)
    lit.set_reference_cache(1)
    with pytest.raises(capi_mod.SlamhipError) as e:
        lit.set_reference_cache(2)
    assert e.value.code == capi_mod.ERR_INVALID
    lit.Reset()
    lit.UpdateByScan(scan_b, pose)
    assert abs(q(lit) - 0.9) < 1e-6                                       # still on, the entry still there
    lit.Reset()
    lit.UpdateByScan(scan_a, pose)
    q(lit)
    lit.set_reference_cache(0)
    lit.set_reference_cache(1)
    lit.Reset()
    lit.UpdateByScan(scan_b, pose)
    assert abs(q(lit) - 0.4) < 1e-6                                       # cleared by the switch
    lit.close(); dfl.close(); g.close()


# ---- 2. probability sequences --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [1, 2, 3])
def test_probability_sequences(hs_mod, ctx, det, sim, levels):
    """Random sequences of UpdateByScan, Reset, upload and probability queries (index lists with repeats): every answer
    equals oc.Grid.prob_literal run through the same operations -- stale or fresh exactly as there, values within the
    device expf's tolerance."""
    side, cell = 96, 0.4
    rng = np.random.default_rng(700 + levels)
    segs = sim.default_field()
    prng = sim.PCG32(700 + levels)
    rep = hs_mod.MapRepMultiMap(cell, (side, side), levels, ctx=ctx)
    rep.set_reference_cache(1)
    ref = det.make_pyramid(cell, side, side, levels)
    pools = [rng.integers(0, g.w * g.h, 300).astype(np.int32) for g in ref]
    stale = queries = 0
    for step in range(90):
        op = rng.choice(["update", "reset", "upload", "query", "query"], p=[0.3, 0.12, 0.1, 0.24, 0.24])
        if op == "update":
            p = (np.array([19.0, 19.0, 0.0]) + rng.uniform(-1, 1, 3) * np.array([2.0, 2.0, 0.5])).astype(np.float32)
            xy = sim.make_scan(segs, p, 180, prng)[1]
            rep.UpdateByScan(hs_mod.ScanCloud(xy), p)
            for g in ref:
                g.update_by_scan(xy, p)
        elif op == "reset":
            rep.Reset()
            for g in ref:
                g.reset()
        elif op == "upload":
            l = int(rng.integers(0, levels))
            c = rep.Maps[l].GetCells().copy()
            k = rng.choice(pools[l], 60)
            c["value"][k] = rng.uniform(-3, 3, k.size).astype(np.float32)
            rep.Maps[l].SetCells(c)
            ref[l].cells["value"][:] = c["value"]
        else:
            l = int(rng.integers(0, levels))
            idx = rng.choice(pools[l], int(rng.integers(1, 200))).astype(np.int32)
            got = rep.Maps[l].GetCachedProbability(idx)
            want = np.array([ref[l].prob_literal(int(i)) for i in idx], np.float32)
            cur = np.array([ref[l].prob(int(i)) for i in idx], np.float32)
            assert np.abs(got - want).max() <= PROB_TOL, (step, l)
            far = np.abs(want - cur) > 10 * PROB_TOL                     # a stale answer: exactly where the literal cache has one
            assert (np.abs(got[far] - cur[far]) > 5 * PROB_TOL).all(), (step, l)
            stale += int(far.sum()); queries += idx.size
    assert stale > 0 and queries > 1000, (stale, queries)
    rep.close()
    for g in ref:
        g.close()


# ---- 3. H / dTr bit for bit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 4])
def test_hessian_bitwise_across_reset(hs_mod, ctx, det, literal_cls, quantised_ab, T):
    """Update, upload quantised A, H at poses P; Reset, update, upload quantised B, H at P again: H and dTr equal
    LiteralNpGrid.hessian bit for bit, and differ from the default mode's -- the aliasing took place."""
    _, b, xy, _ = quantised_ab
    rep, grids, models = start_literal(hs_mod, ctx, literal_cls, det, quantised_ab, T)
    dfl = hs_mod.MapRepMultiMap(CELL, (SIDE, SIDE), LEVELS, ctx=ctx)
    dfl.set_match_threads(T)
    upload(dfl, None, b)
    poses = [TRUE_POSE + np.array(d, np.float32) for d in HINT_OFFS]
    scan = hs_mod.ScanCloud(xy)

    def evaluate():
        rep.set_scan(scan)
        res = []
        for l in range(LEVELS):
            for p in poses:
                est = map_pose(models[l], p)
                H, d = rep.Maps[l].Hessian(est)
                Hr, dr = models[l].hessian(xy, est, T)
                assert same_bits(H, Hr) and same_bits(d, dr), (l, p, H, Hr, d, dr)
                res.append((l, est, H, d))
        return res

    evaluate()
    reset_update_upload_b(hs_mod, rep, models, quantised_ab)
    assert sum(m.stale_count() for m in models) > 0
    differs = 0
    dfl.set_scan(scan)
    for l, est, H, d in evaluate():
        Hd, dd = dfl.Maps[l].Hessian(est)
        differs += not (same_bits(H, Hd) and same_bits(d, dd))
    assert differs > 0
    rep.close(); dfl.close()
    for g in grids:
        g.close()


# ---- 4. match bit for bit -------------------------------------------------------------------------------------------------
def test_match_bitwise_on_effective_grids(hs_mod, ctx, det, literal_cls, quantised_ab):
    """After a match on A, Reset and B: the match (T = 1) equals oc.match_pyramid on the effective grids -- B's cells with
    every stale entry's value as the pre-reset match's taps stored it (replayed with Grid.estimate_step)."""
    _, b, xy, _ = quantised_ab
    T, iters = 1, [3] * LEVELS
    rep, grids, models = start_literal(hs_mod, ctx, literal_cls, det, quantised_ab, T)
    dfl = hs_mod.MapRepMultiMap(CELL, (SIDE, SIDE), LEVELS, ctx=ctx)
    upload(dfl, None, b)
    scan = hs_mod.ScanCloud(xy)
    m = hs_mod.ScanMatcher(T, referenceSummation=True)
    hint = TRUE_POSE + np.array(HINT_OFFS[1], np.float32)
    got = m.MatchData(rep, scan, hint)
    assert same_bits(got, replay_match(det, grids, models, xy, hint, iters, T))
    reset_update_upload_b(hs_mod, rep, models, quantised_ab)
    assert sum(mm.stale_count() for mm in models) > 0
    posts = []
    for hint2 in (hint, TRUE_POSE + np.array(HINT_OFFS[2], np.float32)):
        got = m.MatchData(rep, scan, hint2)
        want = replay_match(det, grids, models, xy, hint2, iters, T)
        assert same_bits(got, want), (hint2, got, want)
        posts.append(got)
    # the first post-reset match read stale entries: it differs from the default mode's match on B
    assert not same_bits(posts[0], m.MatchData(dfl, scan, hint))
    rep.close(); dfl.close()
    for g in grids:
        g.close()


# ---- 5. batch -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 4])
@pytest.mark.parametrize("B", [1, 7, 64])
def test_batch_equals_single(hs_mod, ctx, det, literal_cls, quantised_ab, T, B):
    """In the mode, after a match on A, Reset and B: a batch equals the single matches bit for bit, and leaves the same cache
    (probed by probability queries of every cell after another Reset and an update)."""
    _, _, xy, xy_u = quantised_ab
    scan = hs_mod.ScanCloud(xy)
    rng = np.random.default_rng(50 + B)
    hints = [TRUE_POSE + (rng.uniform(-1, 1, 3) * np.array([0.15, 0.15, 0.05])).astype(np.float32) for _ in range(B)]
    m = hs_mod.ScanMatcher(T, referenceSummation=True)
    reps = []
    for _ in range(2):
        rep, grids, models = start_literal(hs_mod, ctx, literal_cls, det, quantised_ab, T)
        m.MatchData(rep, scan, TRUE_POSE)
        reset_update_upload_b(hs_mod, rep, models, quantised_ab)
        reps.append(rep)
        for g in grids:
            g.close()
    singles = np.stack([m.MatchData(reps[0], scan, h) for h in hints])
    batch = m.MatchDataBatch(reps[1], scan, np.stack(hints))
    for i in range(B):
        assert same_bits(batch[i], singles[i]), (T, B, i, batch[i], singles[i])
    probes = []
    for rep in reps:
        rep.Reset()
        rep.UpdateByScan(hs_mod.ScanCloud(xy_u), PATH_A[0])
        probes.append([mp.GetCachedProbability(np.arange(mp.Dimensions[0] * mp.Dimensions[1], dtype=np.int32)) for mp in rep.Maps])
    for l in range(LEVELS):
        assert same_bits(probes[0][l], probes[1][l]), l
    for rep in reps:
        rep.close()


# ---- 6. transparency ------------------------------------------------------------------------------------------------------
def test_transparent_without_reset(hs_mod, ctx, det, sim):
    """With no Reset in the history the mode equals the default bit for bit at the same T: matches, batches, Hessian."""
    segs = sim.default_field()
    reps = [hs_mod.MapRepMultiMap(CELL, (SIDE, SIDE), 3, ctx=ctx) for _ in range(2)]
    reps[1].set_reference_cache(1)
    rng = sim.PCG32(31)
    scans = [(p, sim.make_scan(segs, p, R, rng)[1]) for p in PATH_A]
    xy = sim.make_scan(segs, TRUE_POSE, R, rng)[1]
    scan = hs_mod.ScanCloud(xy)
    hints = [TRUE_POSE + np.array(d, np.float32) for d in HINT_OFFS]
    for k, (p, s) in enumerate(scans):
        for rep in reps:
            rep.UpdateByScan(hs_mod.ScanCloud(s), p)
        if k < 5:
            continue
        for T in (0, 1, 4):
            m = hs_mod.ScanMatcher(max(T, 1), referenceSummation=T > 0)
            res = []
            for rep in reps:
                r = [m.MatchData(rep, scan, h) for h in hints]
                r.append(m.MatchData(rep.Maps[1], scan, hints[1]))
                r.append(m.MatchDataBatch(rep, scan, np.stack(hints * 4)))
                rep.set_scan(scan)
                for l in range(3):
                    est = np.array([TRUE_POSE[0] / np.float32(CELL * 2 ** l), TRUE_POSE[1] / np.float32(CELL * 2 ** l), TRUE_POSE[2]], np.float32)
                    r.extend(rep.Maps[l].Hessian(est))
                res.append(r)
            for i, (x, y) in enumerate(zip(*res)):
                assert same_bits(x, y), (k, T, i, x, y)
    for rep in reps:
        rep.close()


@pytest.mark.parametrize("T,refsum", [(1, False), (4, True)])
def test_processor_transparent_without_reset(hs_mod, ctx, sim, T, refsum):
    """A 40-scan HectorSLAMProcessor run (device-gated flow included) gives the same poses, decisions and maps in the mode."""
    segs = sim.default_field()
    start = np.array([20.0, 20.0, 0.0], np.float32)
    procs = [hs_mod.HectorSLAMProcessor(CELL, (SIDE, SIDE), start, 3, T, ctx=ctx, referenceSummation=refsum, referenceCache=rc)
             for rc in (False, True)]
    rng = sim.PCG32(41)
    for k in range(40):
        tp = np.array([20.0 + 0.09 * k, 20.0 + 0.03 * k, 0.01 * k], np.float32)
        scan = hs_mod.ScanCloud(sim.make_scan(segs, tp, R, rng)[1])
        hint = tp + np.array([0.03, -0.02, 0.01], np.float32)
        upd = [p.Update(scan, hint, False) for p in procs]
        assert upd[0] == upd[1], k
        assert same_bits(procs[0].MatchPose, procs[1].MatchPose), (k, procs[0].MatchPose, procs[1].MatchPose)
    for l in range(3):
        assert (procs[0].MapRep.Maps[l].GetCells() == procs[1].MapRep.Maps[l].GetCells()).all(), l
    for p in procs:
        p.Dispose()


# ---- 7. the processor across Reset ---------------------------------------------------------------------------------------
def moved_enough(pose, last, min_dist=0.3, min_angle=0.13):
    """HectorSLAMProcessor.cs:107-108 in binary32 (MathEx.DegDiff of the radians, as the reference does)."""
    with np.errstate(over="ignore", invalid="ignore"):
        ddx, ddy = F(pose[0]) - F(last[0]), F(pose[1]) - F(last[1])
        dist2 = F(ddx * ddx) + F(ddy * ddy)
        d = F(F(F(pose[2]) - F(last[2])) + F(180.0)) / F(360.0)
        dd = F(F(d - np.floor(d)) * F(360.0)) - F(180.0)
        return bool(dist2 > F(min_dist) * F(min_dist) or dd > F(min_angle))


def test_processor_across_reset(hs_mod, ctx, det, sim, literal_cls):
    """Path A mapped and matched, Reset, path B through A's area: with referenceCache the poses differ from the default's at
    least once and equal the oracle-side replay -- the cache tracker, the effective grids, oc.match_pyramid (T = 1) and the
    processor's gate -- within 1e-4 m / 1e-4 rad; the update decisions are equal.  The maps are raw (device expf against
    libm expf), so the poses are compared with the tolerance; the replay updates its grids with the device's matched poses,
    so the cells stay identical.  With this seed and these paths no tap lies close enough to a cell border for the
    ulp-level difference of the two expf to move it; another choice could put one there (a moved tap fills another entry,
    and the replay's caches would then part from the device's), so change them only together with a check of that."""
    iters = [3, 3, 3]
    segs = sim.default_field()
    start = np.array([20.0, 20.0, 0.0], np.float32)
    lit = hs_mod.HectorSLAMProcessor(CELL, (SIDE, SIDE), start, 3, 1, ctx=ctx, referenceSummation=True, referenceCache=True)
    dfl = hs_mod.HectorSLAMProcessor(CELL, (SIDE, SIDE), start, 3, 1, ctx=ctx, referenceSummation=True)
    grids = det.make_pyramid(CELL, SIDE, SIDE, 3)
    models = models_for(literal_cls, grids)
    rng = sim.PCG32(61)
    path_a = [np.array([19.6 + 0.35 * k, 20.0 + 0.05 * k, 0.02 * k], np.float32) for k in range(8)]
    path_b = [p + np.array([0.15, 0.12, 0.03], np.float32) for p in path_a]
    off = np.array([0.03, -0.02, 0.01], np.float32)
    last = np.full(3, F_MIN, np.float32)
    differ = 0
    for phase, path in enumerate((path_a, path_b)):
        if phase == 1:
            lit.Reset(); dfl.Reset()
            for g, m in zip(grids, models):
                g.reset(); m.reset()
            last = np.full(3, F_MIN, np.float32)
        for k, tp in enumerate(path):
            xy = sim.make_scan(segs, tp, R, rng)[1]
            scan = hs_mod.ScanCloud(xy)
            hint = tp + off
            want = replay_match(det, grids, models, xy, hint, iters, 1)
            gate = moved_enough(want, last)
            upd = lit.Update(scan, hint, False)
            dfl.Update(scan, hint, False)
            got = lit.MatchPose
            assert upd == gate, (phase, k, got, want)
            assert abs(got[0] - want[0]) < POS_TOL and abs(got[1] - want[1]) < POS_TOL, (phase, k, got, want)
            assert abs(math.remainder(float(got[2]) - float(want[2]), 2 * math.pi)) < ANG_TOL, (phase, k, got, want)
            if phase == 0:
                assert same_bits(got, dfl.MatchPose), k                   # no Reset yet: transparent
            else:
                differ += not same_bits(got, dfl.MatchPose)
            if gate:
                last = want
                for g, m in zip(grids, models):
                    g.update_by_scan(xy, got)
                    m.take_update(g.cells["value"])
    assert differ > 0
    for l in range(3):
        assert (lit.MapRep.Maps[l].GetCells() == grids[l].cells).all(), l
    lit.Dispose(); dfl.Dispose()
    for g in grids:
        g.close()
