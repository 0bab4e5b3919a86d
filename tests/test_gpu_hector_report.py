"""GPU tests of the match report (slamhip_match_report: H, dTr, residual, in-map count at the pose a match ends on) and of
best-of-batch on the device (slamhip_hs_match_best).

Fixtures and the quantised-map / raw-map split are those of tests/test_gpu_hector_refsum.py: on quantised maps every
probability is exactly 0.5 or 1.0, so the C oracle's bits are the device's bits; on raw maps the host model is evaluated on the
device's own probabilities.  The report is restated here from the oracle's pieces: Grid.map_pose, Grid.hessian, Grid.interp
(M per point) and np_oracle's transform.  Nothing accepts a neighbourhood or an envelope; the one bound that is not an
equality (default order, residual) is the textbook bound for summing n non-negative binary32 terms in any order,
|sum - S| <= gamma_n * S with gamma_n = n u / (1 - n u), u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms,
sec. 4.2), derived and not measured."""
import numpy as np
import pytest

from test_gpu_hector_refsum import (HINT_OFFS, SIZE_IDS, SIZES, TRUE_POSE, build_pyramid, capi_mod, ctx, det, hs_mod,  # noqa: F401
                                    same_bits)

pytestmark = pytest.mark.gpu

F = np.float32
T_SUBSET = (1, 4, 7, 64)


def transform_points(npo, cell, xy, pm):
    """The scan in map cells at pose_map (ScanMatcher.cs:139-142,161), np_oracle's binary32 restatement."""
    cell = F(cell); stm = F(F(1.0) / cell)
    t = npo.M32.rotation(pm[2], "det") * npo.M32.translation(F(pm[0]) * cell, F(pm[1]) * cell) * npo.M32.scale(stm)
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    return t.transform(xy[:, 0], xy[:, 1])


def in_map(w, h, mx, my):
    """not IsPointOutOfMapBounds (MapProperties.cs:83-87), NaN coordinates counted outside as the matcher's taps treat them"""
    with np.errstate(invalid="ignore"):
        return ~(np.isnan(mx) | np.isnan(my) | (mx < 0) | (mx > F(w - 2.0)) | (my < 0) | (my > F(h - 2.0)))


def residual_terms(M):
    f = F(1.0) - np.asarray(M, np.float32)                                # :164, its own rounding
    return (f * f).astype(np.float32)                                      # ... and the product's


def chunk_sum(terms, T):
    """ScanMatcher.cs:149-195 for one sum: ceil(n/T)-point chunks sequentially in binary32 from +0, partials in thread order."""
    n = terms.shape[0]
    chunk = (n + T - 1) // T if n else 0
    tot = F(0.0)
    for th in range(T):
        part = terms[th * chunk:min(n, (th + 1) * chunk)]
        loc = np.add.accumulate(part, dtype=np.float32)[-1] if part.size else F(0.0)   # (accumulate: strictly left to right)
        tot = F(tot + loc)
    return tot


def oracle_M(grid, mx, my):
    return np.array([grid.interp(float(a), float(b))[0] for a, b in zip(mx, my)], np.float32)


def check_report_quantised(npo, grid, xy, out_pose, rep, T, level, tag):
    """Item 2: every field of a reference-order report on a quantised map against the oracle model, bit for bit."""
    pm = grid.map_pose(out_pose)
    assert same_bits(rep["pose_map"], pm), (tag, rep["pose_map"], pm)
    Hr, dr = grid.hessian(xy, pm, T)
    assert same_bits(rep["H"], Hr) and same_bits(rep["dTr"], dr), (tag, rep["H"], Hr, rep["dTr"], dr)
    mx, my = transform_points(npo, grid.cell_len, xy, pm)
    want = chunk_sum(residual_terms(oracle_M(grid, mx, my)), T)
    assert same_bits(rep["residual"], want), (tag, rep["residual"], want)
    assert int(rep["n_in_map"]) == int(in_map(grid.w, grid.h, mx, my).sum()), tag
    assert int(rep["n_points"]) == xy.shape[0] and int(rep["level"]) == level, tag
    return want


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


def many_hints(n, seed=5):
    rng = np.random.default_rng(seed)
    return np.stack([TRUE_POSE + (rng.uniform(-1, 1, 3) * np.array([0.2, 0.2, 0.06])).astype(np.float32) for _ in range(n)])


@pytest.mark.parametrize("rc", [0, 1], ids=["nocache", "refcache"])
def test_reports_change_no_pose(hs_mod, qpair, rc):
    """Item 1: out_pose of every _report entry point equals the plain call's bit for bit, in both summation modes and both cache
    modes, at both widths; match_best's pose is the batch's pose at its index."""
    rep, ref, xy, hints, iters = qpair
    scan = hs_mod.ScanCloud(xy)
    many = many_hints(12)
    rep.set_reference_cache(rc)
    try:
        for T in (0, 1, 4):
            m = hs_mod.ScanMatcher(max(T, 1), referenceSummation=T > 0)
            for hint in hints:
                assert same_bits(m.MatchDataReport(rep, scan, hint)[0], m.MatchData(rep, scan, hint)), (T, hint)
                for l in range(rep.NumLevels):
                    assert same_bits(m.MatchDataReport(rep.Maps[l], scan, hint)[0], m.MatchData(rep.Maps[l], scan, hint)), (T, l, hint)
            for B in (1, 3, 8, 9, 12):
                plain = m.MatchDataBatch(rep, scan, many[:B])
                poses, reps = m.MatchDataBatchReport(rep, scan, many[:B])
                assert same_bits(poses, plain), (T, B)
                pose, idx, r = m.MatchDataBest(rep, scan, many[:B])
                assert same_bits(pose, plain[idx]), (T, B, idx)
    finally:
        rep.set_reference_cache(0)


def test_reference_order_quantised(hs_mod, det, npo, qpair):
    """Item 2: single, level and batch reports (B on both sides of 8) in the reference's order, bit for bit."""
    rep, ref, xy, hints, iters = qpair
    scan = hs_mod.ScanCloud(xy)
    many = many_hints(9)
    many[:len(hints)] = hints
    for T in T_SUBSET:
        m = hs_mod.ScanMatcher(T, referenceSummation=True)
        for hint in hints[:3]:
            pose, r = m.MatchDataReport(rep, scan, hint)
            assert same_bits(pose, det.match_pyramid(ref, xy, hint, iters, n_threads=T))
            check_report_quantised(npo, ref[0], xy, pose, r, T, 0, ("single", T, hint))
        for l in range(rep.NumLevels):
            pose, r = m.MatchDataReport(rep.Maps[l], scan, hints[1])
            check_report_quantised(npo, ref[l], xy, pose, r, T, l, ("level", T, l))
        singles = [m.MatchDataReport(rep, scan, h) for h in many]
        for B in (3, 9):
            poses, reps = m.MatchDataBatchReport(rep, scan, many[:B])
            for i in range(B):
                assert same_bits(poses[i], singles[i][0]), (T, B, i)
                assert reps[i].tobytes() == singles[i][1].tobytes(), (T, B, i, reps[i], singles[i][1])
            check_report_quantised(npo, ref[0], xy, poses[B - 1], reps[B - 1], T, 0, ("batch", T, B))


def test_reference_order_long_scan(hs_mod, ctx, det, sim, npo):
    """Item 2, the global-memory path: 2500 points, beyond the points kept in LDS and beyond one window of terms."""
    rep, ref, segs, rng = build_pyramid(hs_mod, ctx, det, sim, 400, 0.1, 3, 400, 10, True)
    _, xy = sim.make_scan(segs, TRUE_POSE, 2500, rng)
    assert xy.shape[0] > 2048
    scan = hs_mod.ScanCloud(xy)
    hints = np.stack([TRUE_POSE + np.array(d, np.float32) for d in HINT_OFFS[1:3]] * 6)
    for T in (1, 4, 64):
        m = hs_mod.ScanMatcher(T, referenceSummation=True)
        pose, r = m.MatchDataReport(rep, scan, hints[0])
        assert same_bits(pose, det.match_pyramid(ref, xy, hints[0], [3, 3, 3], n_threads=T))
        check_report_quantised(npo, ref[0], xy, pose, r, T, 0, ("long", T))
        poses, reps = m.MatchDataBatchReport(rep, scan, hints)
        for i in (0, 1, 11):
            check_report_quantised(npo, ref[0], xy, poses[i], reps[i], T, 0, ("long batch", T, i))
        m0 = hs_mod.ScanMatcher(1)
        assert same_bits(m0.MatchDataReport(rep, scan, hints[0])[0], m0.MatchData(rep, scan, hints[0]))
    rep.close()


@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_reference_order_raw(hs_mod, ctx, det, sim, npo, size):
    """Item 3: raw maps -- H, dTr equal slamhip_hs_hessian(level, report.pose_map) at the same T bit for bit, the residual equals
    the NpGrid model evaluated on the device's own probabilities."""
    side, cell, levels, R, iters = size
    rep, ref, segs, rng = build_pyramid(hs_mod, ctx, det, sim, side, cell, levels, R, 12, False, with_oracle=False)
    for l, it in enumerate(iters):
        rep.Maps[l].EstimateIterations = it
    _, xy = sim.make_scan(segs, TRUE_POSE, R, rng)
    scan = hs_mod.ScanCloud(xy)
    hint = TRUE_POSE + np.array(HINT_OFFS[1], np.float32)

    class DeviceProbGrid(npo.NpGrid):
        def __init__(self, m):
            w, h = m.Dimensions
            super().__init__(np.float32(m.CellLength), w, h, trig="det")
            self._p = m.GetCachedProbability(np.arange(w * h, dtype=np.int32))

        def prob(self, idx):
            return self._p[idx]

    grids = [DeviceProbGrid(m) for m in rep.Maps]
    for T in T_SUBSET:
        m = hs_mod.ScanMatcher(T, referenceSummation=True)
        for target, l in [(rep, 0)] + [(rep.Maps[k], k) for k in range(levels)]:
            pose, r = m.MatchDataReport(target, scan, hint)
            rep.set_scan(scan)
            H, d = rep.Maps[l].Hessian(r["pose_map"])
            assert same_bits(r["H"], H) and same_bits(r["dTr"], d), (T, l)
            g = grids[l]
            mx, my = transform_points(npo, g.cell, xy, r["pose_map"])
            want = chunk_sum(residual_terms(g.interp(mx, my)[0]), T)
            assert same_bits(r["residual"], want), (T, l, r["residual"], want)
            assert int(r["n_in_map"]) == int(in_map(g.w, g.h, mx, my).sum()) and int(r["level"]) == l
    rep.close()


def test_default_order_quantised(hs_mod, det, npo, qpair):
    """Item 4: T = 0 -- H, dTr within test_grid_golden's tolerances of the oracle at report.pose_map; the residual within
    gamma_n * S of S, the binary64 sum of the same binary32 terms; the count exact.  Both widths."""
    rep, ref, xy, hints, iters = qpair
    scan = hs_mod.ScanCloud(xy)
    m = hs_mod.ScanMatcher(1)
    n = xy.shape[0]
    u = 2.0 ** -24
    gamma = n * u / (1 - n * u)
    cases = [(m.MatchDataReport(rep, scan, h), 0) for h in hints]
    cases += [(m.MatchDataReport(rep.Maps[l], scan, hints[1]), l) for l in range(rep.NumLevels)]
    poses, reps = m.MatchDataBatchReport(rep, scan, many_hints(9))
    cases += [((poses[i], reps[i]), 0) for i in (0, 8)]
    for (pose, r), l in cases:
        g = ref[l]
        assert same_bits(r["pose_map"], g.map_pose(pose))
        Hr, dr = g.hessian(xy, r["pose_map"], 1)
        print("default order H", r["H"].ravel(), Hr.ravel(), "dTr", r["dTr"], dr)
        assert np.allclose(r["H"], Hr, rtol=1e-4, atol=1e-4) and np.allclose(r["dTr"], dr, rtol=1e-4, atol=1e-3), (l, r, Hr, dr)
        mx, my = transform_points(npo, g.cell_len, xy, r["pose_map"])
        S = float(residual_terms(oracle_M(g, mx, my)).astype(np.float64).sum())
        print("default order residual", float(r["residual"]), S, gamma * S)
        assert abs(float(r["residual"]) - S) <= gamma * S, (l, r["residual"], S)
        assert int(r["n_in_map"]) == int(in_map(g.w, g.h, mx, my).sum()) and int(r["n_points"]) == n and int(r["level"]) == l


def test_edges(hs_mod, ctx, det, npo, capi_mod):
    """Item 5: an empty scan; a hint that throws the scan off the map; a point exactly on Limits and one ulp beyond."""
    # the hand KAT's grid (tests/test_hand_kats.py): 32 x 32, CellLength 1, Limits 30
    rep = hs_mod.MapRepMultiMap(1.0, (32, 32), 1, ctx=ctx)
    g = det.make_pyramid(1.0, 32, 32, 1)[0]
    cells = rep.Maps[0].GetCells()
    cells["value"][:] = 0.0
    cells["value"][(np.arange(32 * 32) % 7) == 3] = 50.0                   # probabilities exactly 0.5 / 1.0
    rep.Maps[0].SetCells(cells)
    g.cells["value"][:] = cells["value"]
    pose = np.array([10.0, 20.0, 0.0], np.float32)
    on, beyond = F(30.0), np.nextafter(F(30.0), F(np.inf))
    xy = np.array([[on - 10.0, -14.5], [beyond - 10.0, -14.5], [3.25, on - 20.0], [3.25, beyond - 20.0], [1.5, 2.5]], np.float32)
    assert xy[0, 0] + F(10.0) == on and xy[1, 0] + F(10.0) == beyond
    for T in (0, 1, 4):
        m = hs_mod.ScanMatcher(max(T, 1), referenceSummation=T > 0)
        rep.Maps[0].EstimateIterations = 0                                 # the report at the hint itself
        p, r = m.MatchDataReport(rep.Maps[0], hs_mod.ScanCloud(xy), pose)
        assert same_bits(p, pose)
        mx, my = transform_points(npo, 1.0, xy, r["pose_map"])
        assert in_map(32, 32, mx, my).tolist() == [True, False, True, False, True]
        assert int(r["n_in_map"]) == 3 and int(r["n_points"]) == 5
        if T:
            check_report_quantised(npo, g, xy, p, r, T, 0, ("limits", T))
        # the empty scan: the hint comes back, every sum is zero
        empty = hs_mod.ScanCloud(np.zeros((0, 2), np.float32))
        for target in (rep, rep.Maps[0]):
            p, r = m.MatchDataReport(target, empty, pose)
            assert (p == pose).all() and same_bits(r["pose_map"], g.map_pose(pose))
            assert not r["H"].any() and not r["dTr"].any() and r["residual"] == 0 and r["n_in_map"] == 0 and r["n_points"] == 0
        poses, reps = m.MatchDataBatchReport(rep, empty, np.stack([pose] * 9))
        assert (poses == pose).all() and not reps["residual"].any() and not reps["H"].any()
        # off the map: every point contributes exactly 1
        rep.Maps[0].EstimateIterations = 3
        far = np.array([500.0, -300.0, 0.3], np.float32)
        pts = np.ascontiguousarray(np.random.default_rng(1).uniform(-5, 5, (777, 2)).astype(np.float32))
        for target in (rep, rep.Maps[0]):
            p, r = m.MatchDataReport(target, hs_mod.ScanCloud(pts), far)
            assert same_bits(p, m.MatchData(target, hs_mod.ScanCloud(pts), far))
            assert r["residual"] == F(777.0) and r["n_in_map"] == 0 and r["n_points"] == 777 and not r["H"].any() and not r["dTr"].any()
    # argument checks
    out = np.empty(3, np.float32); r1 = np.zeros(1, capi_mod.REPORT_DTYPE); idx = capi_mod.C.c_int32()
    L = capi_mod.lib()
    assert L.slamhip_hs_match_level_report(rep._h, 1, capi_mod.fptr(pose), 3, capi_mod.fptr(out), capi_mod.rptr(r1)) == capi_mod.ERR_INVALID
    assert L.slamhip_hs_match_best(rep._h, capi_mod.fptr(pose), 0, capi_mod.fptr(out), capi_mod.C.byref(idx), capi_mod.rptr(r1)) == capi_mod.ERR_INVALID
    assert L.slamhip_hs_match_report(rep._h, capi_mod.fptr(pose), capi_mod.fptr(out), None) == capi_mod.ERR_INVALID
    rep.close()
    g.close()


def host_key_argmin(reps):
    """The device's key, restated: (bits(residual) << 32 | index), 64-bit minimum."""
    bits = np.ascontiguousarray(reps["residual"]).view(np.uint32).astype(np.uint64)
    keys = (bits << np.uint64(32)) | np.arange(reps.shape[0], dtype=np.uint64)
    return int(np.argmin(keys))


def test_best_of_batch(hs_mod, det, npo, qpair):
    """Item 6: match_best returns the index, pose and report of the host's argmin over match_batch_report's keys, for B on both
    sides of the width switch and far beyond; repeated hints go to the first; at T = 1 the index is the oracle model's."""
    rep, ref, xy, hints, iters = qpair
    scan = hs_mod.ScanCloud(xy)
    many = many_hints(1000, seed=11)
    for T in (0, 1):
        m = hs_mod.ScanMatcher(1, referenceSummation=T > 0)
        for B in (1, 8, 9, 1000):
            poses, reps = m.MatchDataBatchReport(rep, scan, many[:B])
            want = host_key_argmin(reps)
            for _ in range(2):                                             # (twice: the key word was put back in-stream)
                pose, idx, r = m.MatchDataBest(rep, scan, many[:B])
                assert idx == want, (T, B, idx, want)
                assert same_bits(pose, poses[want]) and r.tobytes() == reps[want].tobytes(), (T, B)
        # the same hint three times among hints that throw the scan off the map (residual n_points): the first of the three wins
        # (the list is judged by its own batch: the default order's bits depend on the launch's width)
        off_map = np.array([5000.0, -3000.0, 0.3], np.float32)
        for n_off in (1, 4):                                               # 5 and 11 hints: both widths
            trip = np.stack([off_map] * n_off + [many[0], off_map, many[0], many[0]] + [off_map] * n_off)
            poses, reps = m.MatchDataBatchReport(rep, scan, trip)
            assert reps["residual"][0] == F(xy.shape[0]) and reps["residual"][n_off] < reps["residual"][0]
            assert reps[n_off].tobytes() == reps[n_off + 2].tobytes() == reps[n_off + 3].tobytes()
            pose, idx, r = m.MatchDataBest(rep, scan, trip)
            assert idx == n_off == host_key_argmin(reps) and same_bits(pose, poses[n_off]), (T, n_off, idx)
    # T = 1, quantised: the winner is the one the oracle model selects
    B = 12
    res = []
    for h in many[:B]:
        p = det.match_pyramid(ref, xy, h, iters, n_threads=1)
        mx, my = transform_points(npo, ref[0].cell_len, xy, ref[0].map_pose(p))
        res.append(chunk_sum(residual_terms(oracle_M(ref[0], mx, my)), 1))
    model = np.zeros(B, [("residual", np.float32)]); model["residual"] = res
    m = hs_mod.ScanMatcher(1, referenceSummation=True)
    assert m.MatchDataBest(rep, scan, many[:B])[1] == host_key_argmin(model)


def test_relocalisation(hs_mod, ctx, sim):
    """Item 6, on real data: a map built by 30 simulated updates; a hint lattice around a displaced centre that contains the true
    pose as one of its hints.  The winner's residual is <= the residual of the match started at the true pose (a minimum: it guards
    the key's ordering); the winner's distance from the truth is recorded, not asserted."""
    segs = sim.default_field()
    rep = hs_mod.MapRepMultiMap(0.1, (400, 400), 3, ctx=ctx)
    rng = sim.PCG32(23)
    for it in range(30):
        p = np.array([20 + 0.05 * it, 20 + 0.02 * it, 0.01 * it], np.float32)
        rep.UpdateByScan(hs_mod.ScanCloud(sim.make_scan(segs, p, 400, rng)[1]), p)
    centre = np.array([20.0, 19.8, 0.0], np.float64)
    lat = hs_mod.hint_lattice(centre, 1.0, 0.2, 0.3, 0.1)
    assert lat.shape == (11 * 11 * 7, 3) and lat.dtype == np.float32 and (lat[0] == centre.astype(np.float32)).all()
    truth = lat[np.argmin(np.abs(lat - np.array([20.8, 20.4, 0.2])).sum(axis=1))].copy()
    xy = sim.make_scan(segs, truth, 400, rng)[1]
    scan = hs_mod.ScanCloud(xy)
    m = hs_mod.ScanMatcher(1)
    pose, idx, r = m.MatchDataBest(rep, scan, lat)
    p_true, r_true = m.MatchDataReport(rep, scan, truth)
    assert 0 <= idx < lat.shape[0]
    assert float(r["residual"]) <= float(r_true["residual"]), (r["residual"], r_true["residual"])
    print("relocalisation: winner %d of %d, residual per point %.4f (from the true pose %.4f), distance from the truth %.3f m / %.4f rad"
          % (idx, lat.shape[0], float(r["residual"]) / xy.shape[0], float(r_true["residual"]) / xy.shape[0],
             float(np.hypot(pose[0] - truth[0], pose[1] - truth[1])), abs(float(pose[2] - truth[2]))))
    rep.close()


def test_reference_cache_report_fills_nothing(hs_mod, ctx, sim):
    """Item 7: three pyramids with the same history including a Reset in mid-epoch.  X runs _report matches where Y runs plain
    ones (and, for a level match of zero iterations, nothing at all where X evaluates a report); Z runs the Hessian entry --
    an evaluation that does fill -- at the poses X reports on.  Afterwards the probability of every cell and the next plain
    match are equal on X and Y bit for bit, and Z differs from Y: the scenario can see a fill."""
    segs = sim.default_field()
    side, cell, R, n_upd = 400, 0.1, 400, 6
    reps = [hs_mod.MapRepMultiMap(cell, (side, side), 3, ctx=ctx) for _ in range(3)]
    X, Y, Z = reps
    for r in reps:
        r.set_reference_cache(1)
    rng = sim.PCG32(31)
    path_a = [np.array([19.6 + 0.35 * k, 20.0 + 0.05 * k, 0.02 * k], np.float32) for k in range(n_upd)]
    path_b = [p + np.array([0.15, 0.12, 0.03], np.float32) for p in path_a]
    scans_a = [sim.make_scan(segs, p, R, rng)[1] for p in path_a]
    scans_b = [sim.make_scan(segs, p, R, rng)[1] for p in path_b]
    m = hs_mod.ScanMatcher(1, referenceSummation=True)
    for r in reps:
        for p, xy in zip(path_a, scans_a):
            r.UpdateByScan(hs_mod.ScanCloud(xy), p)
    # epoch n_upd, before the Reset: matches with and without the report
    probe = hs_mod.ScanCloud(scans_a[-1])
    hint = path_a[-1] + np.array([0.12, -0.1, 0.04], np.float32)
    away = path_a[2] + np.array([0.4, 0.3, 0.1], np.float32)               # cells no iteration of these matches taps
    px, rx = m.MatchDataReport(X, probe, hint)
    assert same_bits(px, m.MatchData(Y, probe, hint)) and same_bits(px, m.MatchData(Z, probe, hint))
    X.Maps[0].EstimateIterations = 0
    p0, r0 = m.MatchDataReport(X.Maps[0], probe, away)                    # X evaluates a report at `away`; Y does nothing
    X.Maps[0].EstimateIterations = 3
    Z.set_scan(probe)
    Z.set_match_threads(1)
    Z.Maps[0].Hessian(rx["pose_map"]); Z.Maps[0].Hessian(r0["pose_map"])  # ... and Z fills at both poses
    # without a Reset the report equals the cache-off report
    W = hs_mod.MapRepMultiMap(cell, (side, side), 3, ctx=ctx)
    for p, xy in zip(path_a, scans_a):
        W.UpdateByScan(hs_mod.ScanCloud(xy), p)
    pw, rw = m.MatchDataReport(W, probe, hint)
    assert same_bits(pw, px) and rw.tobytes() == rx.tobytes()
    W.close()
    # Reset in mid-epoch, then path B up to the same epoch
    for r in reps:
        r.Reset()
        for p, xy in zip(path_b, scans_b):
            r.UpdateByScan(hs_mod.ScanCloud(xy), p)
    hint_b = path_b[-1] + np.array([-0.1, 0.08, -0.03], np.float32)
    probe_b = hs_mod.ScanCloud(scans_b[-1])
    px, rx = m.MatchDataReport(X, probe_b, hint_b)
    assert same_bits(px, m.MatchData(Y, probe_b, hint_b))
    probs = []
    for r in reps:
        probs.append([mp.GetCachedProbability(np.arange(mp.Dimensions[0] * mp.Dimensions[1], dtype=np.int32)) for mp in r.Maps])
    for l in range(3):
        assert same_bits(probs[0][l], probs[1][l]), l
    assert not same_bits(probs[2][0], probs[1][0]), "the scenario cannot see a fill: Z's Hessian calls left no stale entry"
    for hint2 in (hint_b, away):
        assert same_bits(m.MatchData(X, probe_b, hint2), m.MatchData(Y, probe_b, hint2))
    for r in reps:
        r.close()


@pytest.mark.parametrize("T", [0, 1])
def test_processor_reports(hs_mod, ctx, sim, T):
    """Item 8: 40 scans with matchReport=True leave poses, Update's return values and every level's checksum equal to the same
    run without; each scan's report equals the one a twin pyramid driven by MatchDataReport + UpdateByScan under the same gate
    produces; LastMatchReport is None before the first scan, after Reset and after a mapWithoutMatching update."""
    start = np.array([20.0, 20.0, 0.0], np.float32)
    kw = dict(ctx=ctx, referenceSummation=T > 0)
    on = hs_mod.HectorSLAMProcessor(0.1, (400, 400), start, 3, 1, matchReport=True, **kw)
    off = hs_mod.HectorSLAMProcessor(0.1, (400, 400), start, 3, 1, **kw)
    twin = hs_mod.MapRepMultiMap(0.1, (400, 400), 3, ctx=ctx)
    matcher = hs_mod.ScanMatcher(1, referenceSummation=T > 0)
    segs = sim.default_field()
    rng = sim.PCG32(17)
    assert on.LastMatchReport is None and off.LastMatchReport is None
    on.MinDistanceDiffForMapUpdate = off.MinDistanceDiffForMapUpdate = 0.05   # (every scan moves 0.1 m: every scan updates)
    hint = start.copy()
    n_upd = 0
    for k in range(40):
        tp = np.array([20.0 + 0.1 * k, 20.0 + 0.02 * k, 0.012 * k], np.float32)
        scan = hs_mod.ScanCloud(sim.make_scan(segs, tp, 400, rng)[1])
        # the first scan only maps (an empty map matches nothing); scan 20 maps without matching behind a matched scan, whose
        # report must not outlive it
        without = k in (0, 20)
        assert k != 20 or on.LastMatchReport is not None
        u_on, u_off = on.Update(scan, hint, without), off.Update(scan, hint, without)
        assert u_on == u_off and same_bits(on.MatchPose, off.MatchPose), k
        assert off.LastMatchReport is None
        if without:
            assert on.LastMatchReport is None
            twin.UpdateByScan(scan, hint)
        else:
            want_pose, want = matcher.MatchDataReport(twin, scan, hint)
            got = on.LastMatchReport
            assert got is not None and same_bits(on.MatchPose, want_pose), k
            assert got.tobytes() == want.tobytes(), (k, got, want)
            if u_on:
                twin.UpdateByScan(scan, want_pose)
        n_upd += u_on
        hint = on.MatchPose.copy()
    assert n_upd > 20                                                     # (the launch-ahead, device-gated flow was taken)
    for l in range(3):
        assert on.MapRep.Maps[l].checksum() == off.MapRep.Maps[l].checksum() == twin.Maps[l].checksum(), l
    on.Reset()
    assert on.LastMatchReport is None
    twin.close(); on.Dispose(); off.Dispose()


def test_without_mailbox():
    """SLAMHIP_NO_HOSTWAIT=1 (no host mailbox: results come back by copy and synchronise, and k4_best_pick writes the winner into
    device memory that overlaps what it reads) must give the same results: the tests above that cover every entry point, B = 1
    included, once more in a process of their own."""
    import os
    import subprocess
    import sys
    sel = "(test_reports_change_no_pose or test_best_of_batch or test_edges or test_processor_reports) and not 2048"
    env = dict(os.environ); env["SLAMHIP_NO_HOSTWAIT"] = "1"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider", "-k", sel],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and " passed" in out and "no tests ran" not in out, out[-3000:]
