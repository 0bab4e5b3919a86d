"""GPU tests of the matcher's opt-in reference summation order (slamhip_hs_set_match_threads; ScanMatcher(numThreads,
referenceSummation=True)): GetCompleteHessianDerivs summed as ScanMatcher.cs:149-195 sums it for T threads.

Bit-exact claims are made where both sides read identical cell probabilities.  The device's probability grid comes from the
device's expf (within 1 ulp of libm, tests/test_gpu_hector.py), so
  * quantised maps -- every cell rewritten to 50 where its value is > 0, else 0, on both sides -- have probabilities exactly
    0.5 and 1.0 whatever the expf: there H, dTr and every pose must equal the C oracle's bit for bit;
  * on raw maps H and dTr must equal NpGrid.hessian(T) evaluated on the device's own probabilities bit for bit, and poses
    the oracle's at the same T within 1e-4 m / 1e-4 rad.
Nothing here accepts a neighbourhood or an envelope."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

POS_TOL = 1e-4
ANG_TOL = 1e-4
TS = (1, 2, 3, 4, 7, 64)
SIZES = [(400, 0.1, 4, 400, [7, 4, 4, 4]), (2048, 40.0 / 2048, 3, 1080, [3, 3, 3])]
SIZE_IDS = ["400x4x400", "2048x3x1080"]
TRUE_POSE = np.array([20.6, 20.25, 0.12], np.float32)
HINT_OFFS = ((0, 0, 0), (0.1, -0.08, 0.03), (-0.15, 0.1, -0.05), (0.02, 0.3, 0.0))


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
    """Equal bit for bit, except that any NaN equals any NaN (the sign and payload of a NaN made by an invalid operation
    differ between the host's and the device's arithmetic units)."""
    a = np.ascontiguousarray(a, np.float32).ravel(); b = np.ascontiguousarray(b, np.float32).ravel()
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all() and (a.view(np.uint32)[~na] == b.view(np.uint32)[~nb]).all())


def quantise_cells(cells):
    cells["value"] = np.where(cells["value"] > 0, np.float32(50.0), np.float32(0.0))


def build_pyramid(hs_mod, ctx, oc, sim, side, cell, levels, R, n_scans, quantised, with_oracle=True, seed=3, factors=None,
                  origin=(0.0, 0.0)):
    """MapRepMultiMap and the oracle's pyramid after n_scans UpdateByScan with the same poses (bit-exact cells), then
    optionally quantised on both sides.  side: cells along one side of a square map, or (w, h); factors: (free, occupied)
    update factors in place of the defaults; origin: the scan origin of every update."""
    segs = sim.default_field()
    w, h = (side, side) if np.isscalar(side) else side
    rep = hs_mod.MapRepMultiMap(cell, (w, h), levels, ctx=ctx)
    ref = oc.make_pyramid(cell, w, h, levels) if with_oracle else None
    if factors is not None:
        rep.SetUpdateFactorFree(factors[0]); rep.SetUpdateFactorOccupied(factors[1])
        for g in ref or ():
            g.set_factors(factors[0], factors[1])
    rng = sim.PCG32(seed)
    for it in range(n_scans):
        p = np.array([20 + 0.05 * it, 20 + 0.02 * it, 0.01 * it], np.float32)
        _, xy = sim.make_scan(segs, p, R, rng)
        rep.UpdateByScan(hs_mod.ScanCloud(xy, (origin[0], origin[1], 0.0)), p)
        for g in ref or ():
            g.update_by_scan(xy, p, origin=origin)
    if quantised:
        for l, m in enumerate(rep.Maps):
            c = m.GetCells()
            quantise_cells(c)
            m.SetCells(c)
            if ref is not None:
                quantise_cells(ref[l].cells)
                assert (m.GetCells() == ref[l].cells).all()
            w, h = m.Dimensions
            p = m.GetCachedProbability(np.arange(w * h, dtype=np.int32))
            assert set(np.unique(p).tolist()) <= {0.5, 1.0}, l       # the precondition of the bit-exact claims
    return rep, ref, segs, rng


@pytest.fixture(scope="module", params=SIZES, ids=SIZE_IDS)
def qpair(request, hs_mod, ctx, det, sim):
    side, cell, levels, R, iters = request.param
    rep, ref, segs, rng = build_pyramid(hs_mod, ctx, det, sim, side, cell, levels, R, 12, True)
    for l, it in enumerate(iters):
        rep.Maps[l].EstimateIterations = it
    _, xy = sim.make_scan(segs, TRUE_POSE, R, rng)
    hints = [TRUE_POSE + np.array(d, np.float32) for d in HINT_OFFS]
    yield rep, ref, xy, hints, iters
    rep.close()


def test_hessian_quantised_bitwise(hs_mod, det, qpair):
    """H and dTr (slamhip_hs_hessian) equal oracle_hs_hessian(T) bit for bit on every level."""
    oc = det
    rep, ref, xy, hints, _ = qpair
    rep.set_scan(hs_mod.ScanCloud(xy))
    for l in range(rep.NumLevels):
        for hint in hints:
            est = ref[l].map_pose(hint)
            for T in TS:
                rep.set_match_threads(T)
                H, d = rep.Maps[l].Hessian(est)
                Hr, dr = ref[l].hessian(xy, est, T)
                assert same_bits(H, Hr) and same_bits(d, dr), (l, hint, T, H, Hr, d, dr)
    rep.set_match_threads(0)


@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_hessian_raw_device_probabilities(hs_mod, ctx, det, sim, npo, size):
    """Raw maps: H and dTr equal NpGrid.hessian(T) evaluated on the device's own probabilities, bit for bit; the poses equal
    the oracle's at the same T within the usual tolerance."""
    oc = det
    side, cell, levels, R, iters = size
    rep, ref, segs, rng = build_pyramid(hs_mod, ctx, oc, sim, side, cell, levels, R, 12, False)
    for l, it in enumerate(iters):
        rep.Maps[l].EstimateIterations = it
    _, xy = sim.make_scan(segs, TRUE_POSE, R, rng)
    hints = [TRUE_POSE + np.array(d, np.float32) for d in HINT_OFFS]

    class DeviceProbGrid(npo.NpGrid):
        def __init__(self, m):
            w, h = m.Dimensions
            super().__init__(np.float32(m.CellLength), w, h, trig="det")
            self._p = m.GetCachedProbability(np.arange(w * h, dtype=np.int32))

        def prob(self, idx):
            return self._p[idx]

    rep.set_scan(hs_mod.ScanCloud(xy))
    for l in range(levels):
        g = DeviceProbGrid(rep.Maps[l])
        for hint in hints[:2]:
            est = ref[l].map_pose(hint)
            for T in TS:
                rep.set_match_threads(T)
                H, d = rep.Maps[l].Hessian(est)
                Hr, dr = g.hessian(xy, est, T)
                assert same_bits(H, Hr) and same_bits(d, dr), (l, hint, T, H, Hr, d, dr)
    for T in (1, 4):
        m = hs_mod.ScanMatcher(T, referenceSummation=True)
        for hint in hints:
            got = m.MatchData(rep, hs_mod.ScanCloud(xy), hint)
            want = oc.match_pyramid(ref, xy, hint, iters, n_threads=T)
            assert abs(got[0] - want[0]) < POS_TOL and abs(got[1] - want[1]) < POS_TOL, (hint, T, got, want)
            assert abs(math.remainder(float(got[2]) - float(want[2]), 2 * math.pi)) < ANG_TOL, (hint, T, got, want)
    rep.close()


def test_match_quantised_bitwise(hs_mod, det, qpair):
    """MatchData(MapRepMultiMap) and MatchData(OccGridMap) equal the oracle's T-thread match bit for bit."""
    oc = det
    rep, ref, xy, hints, iters = qpair
    scan = hs_mod.ScanCloud(xy)
    # the check discriminates: for some hint the oracle's 1- and 4-thread poses differ, so no single device order can equal
    # both.  (A converged match hides the order -- its last step is far below an ulp of the pose -- so the single-level form
    # is also run for one iteration, where the step that differs in its last bits is still large.)
    forms = [(None, None)] + [(l, its) for l in range(len(ref)) for its in sorted({1, iters[l]})]

    def oracle(form, hint, T):
        l, its = form
        return oc.match_pyramid(ref, xy, hint, iters, n_threads=T) if l is None else ref[l].match(xy, hint, its, T)

    assert any(not same_bits(oracle(f, h, 1), oracle(f, h, 4)) for f in forms for h in hints)
    try:
        for T in TS:
            m = hs_mod.ScanMatcher(T, referenceSummation=True)
            for form in forms:
                l, its = form
                if l is not None:
                    rep.Maps[l].EstimateIterations = its
                for hint in hints:
                    got = m.MatchData(rep if l is None else rep.Maps[l], scan, hint)
                    assert same_bits(got, oracle(form, hint, T)), (form, hint, T, got)
                if l is not None:
                    rep.Maps[l].EstimateIterations = iters[l]
    finally:
        for l, it in enumerate(iters):
            rep.Maps[l].EstimateIterations = it


def test_batch_equals_single_bitwise(hs_mod, qpair):
    """A batch of any size (up to 8 hints: the single match's kernel; beyond: 256 lanes per hint) gives the single match's bits."""
    rep, ref, xy, hints, _ = qpair
    scan = hs_mod.ScanCloud(xy)
    rng = np.random.default_rng(5)
    many = [TRUE_POSE + (rng.uniform(-1, 1, 3) * np.array([0.2, 0.2, 0.06])).astype(np.float32) for _ in range(64)]
    many[:len(hints)] = hints
    for T in TS:
        m = hs_mod.ScanMatcher(T, referenceSummation=True)
        singles = [m.MatchData(rep, scan, h) for h in many]
        for B in (1, 3, 12, 64):
            batch = m.MatchDataBatch(rep, scan, np.stack(many[:B]))
            for i in range(B):
                assert same_bits(batch[i], singles[i]), (T, B, i, batch[i], singles[i])


def test_long_scan_bitwise(hs_mod, ctx, det, sim):
    """2500 points: beyond the points the matcher keeps in LDS and beyond one window of terms, single match and batch."""
    oc = det
    rep, ref, segs, rng = build_pyramid(hs_mod, ctx, oc, sim, 400, 0.1, 3, 400, 10, True)
    _, xy = sim.make_scan(segs, TRUE_POSE, 2500, rng)
    assert xy.shape[0] > 2048
    scan = hs_mod.ScanCloud(xy)
    hints = [TRUE_POSE + np.array(d, np.float32) for d in HINT_OFFS[1:3]]
    for T in (1, 3, 64):
        m = hs_mod.ScanMatcher(T, referenceSummation=True)
        wants = [oc.match_pyramid(ref, xy, h, [3, 3, 3], n_threads=T) for h in hints]
        for h, want in zip(hints, wants):
            got = m.MatchData(rep, scan, h)
            assert same_bits(got, want), (T, h, got, want)
        batch = m.MatchDataBatch(rep, scan, np.stack(hints * 6))
        for i in range(12):
            assert same_bits(batch[i], wants[i % 2]), (T, i, batch[i], wants[i % 2])
        rep.set_scan(scan)
        est = ref[0].map_pose(hints[0])
        H, d = rep.Maps[0].Hessian(est)
        Hr, dr = ref[0].hessian(xy, est, T)
        assert same_bits(H, Hr) and same_bits(d, dr), T
    rep.close()


def test_edge_cases(hs_mod, ctx, det, sim, capi_mod):
    oc = det
    rep, ref, segs, rng = build_pyramid(hs_mod, ctx, oc, sim, 400, 0.1, 3, 400, 10, True)
    _, xy = sim.make_scan(segs, TRUE_POSE, 400, rng)
    hint = TRUE_POSE + np.array([0.05, -0.04, 0.02], np.float32)
    m64 = hs_mod.ScanMatcher(64, referenceSummation=True)
    # T > n: empty chunks add +0
    few = np.ascontiguousarray(xy[::80][:5])
    assert few.shape[0] == 5
    assert same_bits(m64.MatchData(rep, hs_mod.ScanCloud(few), hint), oc.match_pyramid(ref, few, hint, [3, 3, 3], n_threads=64))
    rep.set_scan(hs_mod.ScanCloud(few))
    est = ref[1].map_pose(hint)
    H, d = rep.Maps[1].Hessian(est)
    Hr, dr = ref[1].hessian(few, est, 64)
    assert same_bits(H, Hr) and same_bits(d, dr)
    # an empty scan returns the hint (:82-83)
    empty = hs_mod.ScanCloud(np.zeros((0, 2), np.float32))
    assert (m64.MatchData(rep, empty, hint) == hint).all()
    assert (m64.MatchData(rep.Maps[0], empty, hint) == hint).all()
    # far points (outside the map: zero gradient) and a NaN point (rotDeriv = NaN * 0) as the reference treats them
    odd = xy.copy()
    odd[7] = (1e6, -1e6)
    odd[11] = (np.nan, 1.0)
    for T in (1, 4):
        rep.set_match_threads(T)
        rep.set_scan(hs_mod.ScanCloud(odd))
        H, d = rep.Maps[0].Hessian(est)
        Hr, dr = ref[0].hessian(odd, est, T)
        assert same_bits(H, Hr) and same_bits(d, dr), T
        m = hs_mod.ScanMatcher(T, referenceSummation=True)
        assert same_bits(m.MatchData(rep, hs_mod.ScanCloud(odd), hint), oc.match_pyramid(ref, odd, hint, [3, 3, 3], n_threads=T))
    far_only = odd.copy()
    far_only[11] = (1e6, 1e6)
    got = m64.MatchData(rep, hs_mod.ScanCloud(far_only), hint)
    assert same_bits(got, oc.match_pyramid(ref, far_only, hint, [3, 3, 3], n_threads=64))
    # argument checks: the setting is unchanged by a refused value
    rep.set_match_threads(4)
    for bad in (-1, 65):
        with pytest.raises(capi_mod.SlamhipError) as e:
            rep.set_match_threads(bad)
        assert e.value.code == capi_mod.ERR_INVALID
    out = np.empty(3, np.float32)
    rep.set_scan(hs_mod.ScanCloud(xy))
    capi_mod.call("slamhip_hs_match", rep._h, capi_mod.fptr(hint), capi_mod.fptr(out))
    assert same_bits(out, oc.match_pyramid(ref, xy, hint, [3, 3, 3], n_threads=4))
    # T, then 0: the default order again, the same bits as a fresh pyramid that never left it
    rep.set_match_threads(0)
    capi_mod.call("slamhip_hs_match", rep._h, capi_mod.fptr(hint), capi_mod.fptr(out))
    fresh, _, _, _ = build_pyramid(hs_mod, ctx, oc, sim, 400, 0.1, 3, 400, 10, True, with_oracle=False)
    want = hs_mod.ScanMatcher(4).MatchData(fresh, hs_mod.ScanCloud(xy), hint)
    assert same_bits(out, want)
    assert same_bits(hs_mod.ScanMatcher(4).MatchData(rep, hs_mod.ScanCloud(xy), hint), want)
    fresh.close()
    rep.close()


@pytest.fixture(scope="module")
def capi_mod():
    import slam.net_amd.capi as c
    return c


@pytest.mark.parametrize("T", [1, 4, 7])
def test_processor_reference_summation(hs_mod, ctx, det, sim, T):
    """HectorSLAMProcessor(..., referenceSummation=True): the deferred, device-gated per-scan flow (slamhip_hsproc_update)
    matches in the T-thread order -- the first Update against the oracle, the next 40 against ScanMatcher on a second pyramid
    kept in step with UpdateByScan."""
    oc = det
    start = np.array([20.0, 20.0, 0.0], np.float32)
    proc = hs_mod.HectorSLAMProcessor(0.1, (400, 400), start, 3, T, ctx=ctx, referenceSummation=True)
    built, ref, _, _ = build_pyramid(hs_mod, ctx, oc, sim, 400, 0.1, 3, 400, 10, True)
    built.close()
    # the quantised maps uploaded to the processor and to a fresh twin pyramid; both update counters start at 0, so the
    # uploaded cells' update indices are cleared (no cell is held back from the next UpdateByScan on either side)
    twin = hs_mod.MapRepMultiMap(0.1, (400, 400), 3, ctx=ctx)
    for l in range(3):
        cells = ref[l].cells.copy()
        cells["update_index"] = 0
        proc.MapRep.Maps[l].SetCells(cells)
        twin.Maps[l].SetCells(cells)
    segs = sim.default_field()
    rng = sim.PCG32(17)
    matcher = hs_mod.ScanMatcher(T, referenceSummation=True)
    hint = np.array([20.42, 20.15, 0.06], np.float32)
    for k in range(41):
        tp = np.array([20.45 + 0.03 * k, 20.18 + 0.01 * k, 0.07 + 0.004 * k], np.float32)
        _, xy = sim.make_scan(segs, tp, 400, rng)
        scan = hs_mod.ScanCloud(xy)
        want = oc.match_pyramid(ref, xy, hint, [3, 3, 3], n_threads=T) if k == 0 else matcher.MatchData(twin, scan, hint)
        updated = proc.Update(scan, hint, False)
        got = proc.MatchPose
        assert same_bits(got, want), (k, got, want)
        if updated:
            twin.UpdateByScan(scan, got)
        hint = got.copy()
    for l in range(3):
        assert (proc.MapRep.Maps[l].GetCells() == twin.Maps[l].GetCells()).all(), l
    twin.close()
    proc.Dispose()


def test_randomised_slice(hs_mod, ctx, det, sim):
    """Seeded random cases on quantised maps -- sides, levels, 3 .. 1080 rays (few-ray, near-singular scans included), T and
    hints -- each compared directly and bit for bit with the oracle, with no neighbourhood or envelope acceptance."""
    oc = det
    rng = np.random.default_rng(20261016)
    segs = sim.default_field()
    cases = 0
    for build in range(12):
        side = int(rng.choice([128, 200, 256, 400, 512]))
        levels = int(rng.integers(1, 5))
        cell = float(np.float32(40.0 / side))
        rep, ref, _, prng = build_pyramid(hs_mod, ctx, oc, sim, side, cell, levels, int(rng.choice([90, 360, 720])), 6, True,
                                          seed=100 + build)
        iters = [int(rng.integers(1, 6)) for _ in range(levels)]
        for l, it in enumerate(iters):
            rep.Maps[l].EstimateIterations = it
        for _ in range(5):
            R = int(rng.choice([3, 4, 6, 11, 40, 180, 400, 1080]))
            tp = (np.array([20.3, 20.2, 0.1]) + rng.uniform(-1, 1, 3) * np.array([0.3, 0.3, 0.1])).astype(np.float32)
            _, xy = sim.make_scan(segs, tp, R, prng)
            T = int(rng.choice([1, 2, 3, 4, 5, 7, 8, 13, 16, 31, 64]))
            hint = (tp + rng.uniform(-1, 1, 3) * np.array([0.15, 0.15, 0.05])).astype(np.float32)
            got = hs_mod.ScanMatcher(T, referenceSummation=True).MatchData(rep, hs_mod.ScanCloud(xy), hint)
            want = oc.match_pyramid(ref, xy, hint, iters, n_threads=T)
            assert same_bits(got, want), (build, side, levels, iters, R, xy.shape[0], T, hint, got, want)
            cases += 1
        rep.close()
    assert cases == 60
