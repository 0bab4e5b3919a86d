"""K4, the Hector scan matcher, at its edges -- the cases of tests/k4_cases.py (each checked on the CPU for the property it claims:
tests/test_k4_cases_cpu.py) on the device through MapRepMultiMap and ScanMatcher.  Every comparison is `==` on bits (any NaN equals
any NaN, as same_bits of tests/test_gpu_hector_refsum.py); there is no tolerance anywhere.

Per case, with the reference cache off and on, at T = 0 (the default order; "exact" cases only, whose sums are the same in every
order) and at every T of the case (the reference order), for every scan of the case:
  * Hessian on each level at the case's pose;
  * the level match with 0 iterations -- its report is the evaluation at the hint -- and with 1 iteration, pose and report;
  * the pyramid match with the case's iteration counts, pose and report;
  * MatchDataBatch / MatchDataBatchReport / MatchDataBest at the case's batch sizes: every entry equal to its single match.
"Exact" cases are held to kc.expected() (rational arithmetic) wherever the pose is the dyadic hint, and to the C oracle elsewhere;
"order" cases to the C oracle at T.  A report away from the hint is modelled from the oracle's pieces as in
tests/test_gpu_hector_report.py, whose own assertions (best-of-batch ties, NaN last, the cache that a report must not fill) are not
repeated here."""
import numpy as np
import pytest

import k4_cases as kc
from test_gpu_hector_refsum import ctx, det, hs_mod, same_bits           # noqa: F401 (fixtures)
from test_gpu_hector_report import host_key_argmin, in_map, residual_terms, transform_points

pytestmark = pytest.mark.gpu

F = np.float32
NAMES = [c.name for c in kc.CASES]
FLOATS, INTS = ("pose_map", "H", "dTr", "residual"), ("n_in_map", "n_points", "level")


def same_report(a, b):
    return all(same_bits(a[f], b[f]) for f in FLOATS) and all(int(a[f]) == int(b[f]) for f in INTS)


class Pair:
    """One case on the device and in the oracles."""

    def __init__(self, hs_mod, ctx, oc, npo, b):
        import slam.net_amd.capi as capi
        self.b, self.oc, self.npo = b, oc, npo
        self.rep = hs_mod.MapRepMultiMap(1.0, b.size, b.levels, ctx=ctx)
        self.ref = oc.make_pyramid(1.0, b.size[0], b.size[1], b.levels)
        self.np = []
        for l, (w, h) in enumerate(kc.level_dims(b.size, b.levels)):
            assert self.rep.Maps[l].Dimensions == (w, h)
            cells = np.empty(w * h, capi.CELL_DTYPE)
            cells["update_index"] = -1
            cells["value"] = b.cells[l]
            self.rep.Maps[l].SetCells(cells)
            self.ref[l].cells[:] = cells
            # the precondition of every bit-exact claim: the device's probabilities are the exact ones
            assert same_bits(self.rep.Maps[l].GetCachedProbability(np.arange(w * h, dtype=np.int32)), kc.prob_of(b.cells[l])), l
            g = npo.NpGrid(F(2 ** l), w, h, trig="det")
            g.set_prob_table(kc.prob_of(b.cells[l]))
            self.np.append(g)
            self.rep.Maps[l].EstimateIterations = b.iters[l]

    def close(self):
        self.rep.close()
        for g in self.ref:
            g.close()

    def model(self, l, xy, pose_world, T):
        """The report of level l at the pose a match ended on, in the reference's order, from the oracles' pieces."""
        pm = self.ref[l].map_pose(pose_world)
        H, d = self.ref[l].hessian(xy, pm, T)
        _, P = self.np[l].hessian_terms(xy, pm)
        mx, my = transform_points(self.npo, self.ref[l].cell_len, xy, pm)
        return pm, H, d, kc.ref_sum(residual_terms(P), T), int(in_map(self.ref[l].w, self.ref[l].h, mx, my).sum())

    def check_report(self, r, l, xy, pose_world, T, tag, at_hint=False):
        b = self.b
        n = xy.shape[0]
        assert int(r["n_points"]) == n and int(r["level"]) == l, tag
        assert same_bits(r["pose_map"], self.ref[l].map_pose(pose_world)), tag
        if n == 0:
            assert not r["H"].any() and not r["dTr"].any() and r["residual"] == 0 and r["n_in_map"] == 0, tag
            return
        if at_hint and b.family == "exact":
            H, d, res, n_in = kc.expected(kc.geometry(b.cells, b.size, l, kc.map_pose(b.pose, l), xy))
        elif T > 0:
            _, H, d, res, n_in = self.model(l, xy, pose_world, T)
        else:
            return                                                     # (the default order away from the dyadic hint: no bits to hold it to)
        assert same_bits(r["H"], H) and same_bits(r["dTr"], d), (tag, r["H"], H, r["dTr"], d)
        assert same_bits(r["residual"], res) and int(r["n_in_map"]) == n_in, (tag, r["residual"], res, r["n_in_map"], n_in)


@pytest.mark.parametrize("name", NAMES)
def test_case(hs_mod, ctx, det, npo, name):
    oc = det
    b = kc.by_name(name).build()
    P = Pair(hs_mod, ctx, oc, npo, b)
    rep, ref = P.rep, P.ref
    hint = np.array(b.pose, np.float32)
    exact = b.family == "exact"
    try:
        for rc in (0, 1):
            rep.set_reference_cache(rc)
            for T in ((0,) if exact else ()) + b.Ts:
                To = max(T, 1)                                         # (an exact case's oracle: any T gives the same bits)
                m = hs_mod.ScanMatcher(To, referenceSummation=T > 0)
                for si, xy in enumerate(b.scans):
                    scan = hs_mod.ScanCloud(xy)
                    n = xy.shape[0]
                    tag = (name, rc, T, si)
                    for l in range(b.levels):
                        pm = kc.map_pose(b.pose, l)
                        rep.set_scan(scan)
                        rep.set_match_threads(T)
                        H, d = rep.Maps[l].Hessian(pm)
                        Hr, dr = kc.expected(kc.geometry(b.cells, b.size, l, pm, xy))[:2] if exact else ref[l].hessian(xy, pm, T)
                        assert same_bits(H, Hr) and same_bits(d, dr), (tag, l, H, Hr, d, dr)
                        rep.Maps[l].EstimateIterations = 0
                        p, r = m.MatchDataReport(rep.Maps[l], scan, hint)
                        assert same_bits(p, hint), (tag, l)
                        P.check_report(r, l, xy, hint, T, (tag, l, "its0"), at_hint=True)
                        rep.Maps[l].EstimateIterations = 1
                        p, r = m.MatchDataReport(rep.Maps[l], scan, hint)
                        want = ref[l].match(xy, hint, 1, To)
                        assert same_bits(p, want) and same_bits(m.MatchData(rep.Maps[l], scan, hint), want), (tag, l, p, want)
                        P.check_report(r, l, xy, p, T, (tag, l, "its1"))
                        rep.Maps[l].EstimateIterations = b.iters[l]
                    if si >= 2:                                        # (the one-point scans of the border cases: the level forms only)
                        continue
                    full = T > 0 or sum(b.iters) <= 1                  # (T = 0 is exact up to the first step only)
                    if full:
                        p, r = m.MatchDataReport(rep, scan, hint)
                        want = oc.match_pyramid(ref, xy, hint, b.iters, n_threads=To)
                        assert same_bits(p, want) and same_bits(m.MatchData(rep, scan, hint), want), (tag, p, want)
                        P.check_report(r, 0, xy, p, T, (tag, "pyramid"), at_hint=n == 0 or sum(b.iters) == 0)
                    for B in b.batch if full and si == 0 else ():
                        hints = kc.batch_hints(b, B)
                        singles = [m.MatchDataReport(rep, scan, h) for h in hints]
                        poses, reps = m.MatchDataBatchReport(rep, scan, hints)
                        plain = m.MatchDataBatch(rep, scan, hints)
                        for i in range(B):
                            assert same_bits(poses[i], singles[i][0]) and same_bits(plain[i], singles[i][0]), (tag, B, i, poses[i], singles[i][0])
                            assert same_bits(poses[i], oc.match_pyramid(ref, xy, hints[i], b.iters, n_threads=To)), (tag, B, i)
                            if T > 0:
                                assert same_report(reps[i], singles[i][1]), (tag, B, i, reps[i], singles[i][1])
                            else:
                                # (a default-order report after a step sums inexact terms: its bits depend on the width.  What
                                # does not: the pose it is taken at and the counts)
                                assert same_bits(reps[i]["pose_map"], singles[i][1]["pose_map"]), (tag, B, i)
                                assert all(int(reps[i][f]) == int(singles[i][1][f]) for f in INTS), (tag, B, i, reps[i], singles[i][1])
                        pose, idx, r = m.MatchDataBest(rep, scan, hints)
                        assert idx == host_key_argmin(reps) and same_bits(pose, poses[idx]) and same_report(r, reps[idx]), (tag, B, idx)
                        if T == 0:
                            # the default order's reports of a batch, bit for bit: no iteration, so every report is the evaluation
                            # at its own dyadic hint, where the sums are exact (test_batch_hints_are_exact_too)
                            for l in range(b.levels):
                                rep.Maps[l].EstimateIterations = 0
                            poses, reps = m.MatchDataBatchReport(rep, scan, hints)
                            for l in range(b.levels):
                                rep.Maps[l].EstimateIterations = b.iters[l]
                            assert same_bits(poses, hints), (tag, B)
                            for i in range(B):
                                H, d, res, n_in = kc.expected(kc.geometry(b.cells, b.size, 0, kc.map_pose(hints[i], 0), xy))
                                assert same_bits(reps[i]["H"], H) and same_bits(reps[i]["dTr"], d) and same_bits(reps[i]["residual"], res), (tag, B, i)
                                assert int(reps[i]["n_in_map"]) == n_in and int(reps[i]["n_points"]) == n, (tag, B, i)
    finally:
        rep.set_reference_cache(0)
        P.close()


@pytest.mark.parametrize("n", [kc.LDS_PTS - 1, kc.LDS_PTS, kc.LDS_PTS + 1])
def test_fresh_scan_then_update(hs_mod, ctx, det, npo, n):
    """Group C: a fresh ScanCloud of 2047, 2048, 2049 points matched once -- up to 2048 the single match pulls the points from the
    staging block itself -- then UpdateByScan at the matched pose: cells == oracle; then matched again, from a fresh cloud and from
    the points the device now holds: the same bits (and, in the reference order, a batch entry's)."""
    oc = det
    b = kc.by_name("count_%d" % n).build()
    xy = b.scans[0]
    hint = np.array(b.pose, np.float32)
    for T in (0, 1):
        P = Pair(hs_mod, ctx, oc, npo, b)
        try:
            m = hs_mod.ScanMatcher(1, referenceSummation=T > 0)
            scan = hs_mod.ScanCloud(xy.copy())
            p, r = m.MatchDataReport(P.rep, scan, hint)
            want = oc.match_pyramid(P.ref, xy, hint, b.iters, n_threads=1)
            assert same_bits(p, want), (n, T, p, want)
            P.rep.UpdateByScan(scan, p)
            P.ref[0].update_by_scan(xy, want)
            got, cells = P.rep.Maps[0].GetCells(), P.ref[0].cells
            for f in ("update_index", "value"):
                assert (np.ascontiguousarray(got[f]).view(np.uint32) == np.ascontiguousarray(cells[f]).view(np.uint32)).all(), (n, T, f)
            q, r2 = m.MatchDataReport(P.rep, hs_mod.ScanCloud(xy.copy()), hint)
            assert same_bits(m.MatchData(P.rep, scan, hint), q), (n, T)
            if T:
                assert same_bits(m.MatchDataBatch(P.rep, scan, np.stack([hint] * 9))[8], q), (n, T)
        finally:
            P.close()
