"""The K5 edge cases (tests/k5_cases.py) on the CPU: every case through the C oracle and through np_oracle.NpGrid, cell for cell on
every level after every update; the property each case claims, asserted from the case's own geometry; the kernel's rule -- per cell
the smallest index of a line that crosses it and of one that ends in it, by the closed form, then the two transitions -- restated
in NumPy, equal to the oracles on every case, and six wrong copies of it that named cases catch; the bound behind the lone-line
shortcut and the float estimate of the step lanes' division, over the sets the kernel's comments claim them for."""
import math

import numpy as np
import pytest

import k5_cases as kc

F = np.float32
INT_MAX = kc.INT_MAX
NAMES = [c.name for c in kc.CASES]


@pytest.fixture(scope="module")
def det(oc):
    oc.set_trig_mode(oc.TRIG_DET)
    yield oc
    oc.set_trig_mode(oc.TRIG_LIBM)


def bits(cells):
    return np.ascontiguousarray(cells).view(np.uint32)


def logodds(p):
    return F(math.log(float(F(F(p) / F(F(1.0) - F(p))))))              # OccGridMap.cs:86-90


# ---- the kernel's rule -------------------------------------------------------------------------------------------------------------
class Rule:
    """k5_cells restated: first_touches (k5_hit's closed form) and k5_transition on whole levels.  variant: None or a wrong copy."""

    def __init__(self, built, variant=None):
        self.built, self.variant = built, variant
        self.dims = kc.level_dims(built.size, built.levels)
        self.cells = [np.zeros(w * h, kc.CELL) for w, h in self.dims]
        self.lo_free, self.lo_occ = logodds(0.4), logodds(0.9)
        if built.factors:
            self.lo_free, self.lo_occ = logodds(built.factors[0]), logodds(built.factors[1])
        self.geo = kc.geometry(built, "floor" if variant == "floor" else "rint")
        self.reset()

    def reset(self):
        for c in self.cells:
            c["value"] = 0
            c["update_index"] = -1
        self.cur = [0] * len(self.cells)

    def scan(self, k):
        for l, (g, c) in enumerate(zip(self.geo[k], self.cells)):
            mark_free, mark_occ = self.cur[l] + 1, self.cur[l] + 2
            self.cur[l] += 3
            if g.valid.any():
                ff, fo = kc.first_touches(g, self.variant if self.variant in ("no_half", "end_free", "zone_diag") else None)
                t = np.flatnonzero((ff != INT_MAX) | (fo != INT_MAX))
                ff, fo, v, u = ff[t], fo[t], c["value"][t], c["update_index"][t].astype(np.int64)
                with np.errstate(invalid="ignore"):
                    free = (u < mark_free) & ((ff != INT_MAX) if self.variant == "fixed_order" else (ff < fo))
                    v = np.where(free, v + self.lo_free, v).astype(np.float32)
                    u = np.where(free, mark_free, u)
                    occ = (fo != INT_MAX) & (u < mark_occ)
                    v = np.where(occ & (u == mark_free), v - self.lo_free, v).astype(np.float32)
                    below = (v <= F(50.0)) if self.variant == "le50" else (v < F(50.0))
                    v = np.where(occ & below, v + self.lo_occ, v).astype(np.float32)
                    u = np.where(occ, mark_occ, u)
                c["value"][t] = v
                c["update_index"][t] = u


def run(built, oc, npo=None, variant=None, stop_at_mismatch=False, keep=False):
    """The case through the C oracle, NpGrid (if given) and the rule, compared after every step.  Returns (all equal, trace):
    trace[k] = (cells before, cells after) per level of step k, kept for small cases only."""
    levels, dims = built.levels, kc.level_dims(built.size, built.levels)
    ref = oc.make_pyramid(built.cell_len, built.size[0], built.size[1], levels)
    nps = None
    if npo is not None:
        nps, res = [], F(built.cell_len)
        for w, h in dims:
            nps.append(npo.NpGrid(res, w, h))
            res = F(res * F(2.0))
    rule = Rule(built, variant)
    if built.factors:
        for g in ref:
            g.set_factors(*built.factors)
        for g in nps or []:
            g.set_factors(*built.factors)

    def upload(cells):
        for l in range(levels):
            ref[l].cells[:] = cells[l]
            rule.cells[l][:] = cells[l]
            if nps:
                nps[l].value[:] = cells[l]["value"]
                nps[l].upd[:] = cells[l]["update_index"]
            cur = kc.index_after_upload(cells[l], rule.cur[l])           # (the library's upload moves the current index; the oracles
            while rule.cur[l] < cur:                                     #  follow with empty scans)
                ref[l].update_by_scan(np.zeros((0, 2), np.float32), (0.0, 0.0, 0.0))
                if nps:
                    nps[l].update_by_scan(np.zeros((0, 2), np.float32), (0.0, 0.0, 0.0))
                rule.cur[l] += 3
    if built.start is not None:
        upload(built.start)
    trace, equal = [], True
    for k, step in enumerate(built.steps):
        before = [g.cells.copy() for g in ref] if keep else None
        if kc.is_scan(step):
            xy, origin, pose = step
            for l in range(levels):
                ref[l].update_by_scan(xy, pose, origin=origin)
                if nps:
                    nps[l].update_by_scan(xy, pose, origin=origin)
            rule.scan(k)
        elif step[0] == "reset":
            for l in range(levels):
                ref[l].reset()
                if nps:
                    nps[l].reset()
            rule.reset()
        elif step[0] == "set_cells":
            upload(step[1])
        elif step[0] == "shift":
            upload([kc.shifted(ref[l].cells.copy(), dims[l][0], dims[l][1], step[1] >> l, step[2] >> l) for l in range(levels)])
        for l in range(levels):
            if nps:
                assert np.array_equal(bits(nps[l].value), bits(ref[l].cells["value"])), (k, l, "NpGrid value")
                assert np.array_equal(nps[l].upd, ref[l].cells["update_index"]), (k, l, "NpGrid index")
            same = np.array_equal(bits(rule.cells[l]["value"]), bits(ref[l].cells["value"])) and \
                np.array_equal(rule.cells[l]["update_index"], ref[l].cells["update_index"])
            equal = equal and same
        if stop_at_mismatch and not equal:
            break
        trace.append((before, [g.cells.copy() for g in ref]) if keep else None)
    for g in ref:
        g.close()
    return equal, trace


# ---- the claims --------------------------------------------------------------------------------------------------------------------
def _scans(built, geo):
    return [(k, geo[k]) for k, s in enumerate(built.steps) if kc.is_scan(s)]


def _pairs(g):
    v = np.flatnonzero(g.valid)
    return [(int(i), int(j)) for a, i in enumerate(v) for j in v[a + 1:] if g.cls[i] == g.cls[j]]


def _slope_gap(g, i, j):
    return abs(int(g.sdb[i]) * int(g.da[j]) - int(g.sdb[j]) * int(g.da[i])) / (int(g.da[i]) * int(g.da[j]))


def claim_octants(built, geo, arg, trace, x_only=False):
    g = geo[0][0]
    for da in map(int, arg.split(",")):
        sel = np.flatnonzero(g.valid & (g.da == da))
        have = {(int(g.cls[i]), int(g.sdb[i])) for i in sel}
        classes = {c for c, _ in have}
        if x_only:
            assert len(classes) == 2 and all({0, 1, -1} <= {b for c, b in have if c == cl} for cl in classes), (da, have)
            continue
        assert classes == {0, 1, 2, 3}, (da, have)
        for cl in range(4):
            minors = {b for c, b in have if c == cl}
            assert 0 in minors, (da, cl)                                 # the axis
            want = {1, da // 2, da - 1} - {0, da}
            assert all(b in minors and -b in minors for b in want), (da, cl, minors)     # both octants of the class
        assert {(0, da), (0, -da), (1, da), (1, -da)} <= have            # the four exact diagonals (adx == ady is x-major)
    das = set(map(int, arg.split(",")))
    lanes = {(d - kc.ZONE) % 64 for d in das if d >= kc.ZONE}
    if das & {16, 80, 144}:
        assert 0 in lanes                                                # the end cell on lane 0 of a block ...
    if das & {79, 143}:
        assert 63 in lanes                                               # ... and on lane 63


def claim_octants_x(built, geo, arg, trace):
    claim_octants(built, geo, arg, trace, x_only=True)


def claim_short_then_long(built, geo, arg, trace):
    a, b = geo[0][0], geo[1][0]
    assert a.da.max() == kc.ZONE - 1 and a.valid.sum() > 8
    assert b.da.size == a.da.size and b.da.max() >= 80


def claim_begin_on_border(built, geo, arg, trace):
    g = geo[0][0]
    assert g.inside and (g.bx in (0, g.w - 1) or g.by in (0, g.h - 1))
    assert (g.valid & (g.da >= kc.ZONE)).any() and (g.valid & (g.da < kc.ZONE)).any() and (~g.valid).any()


def claim_begin_outside(built, geo, arg, trace):
    for k in range(6):
        g = geo[k][0]
        assert not g.inside and not g.valid.any()
        assert max(-g.bx, g.bx - (g.w - 1), -g.by, g.by - (g.h - 1)) == 1
        assert np.array_equal(bits(trace[k][0][0]), bits(trace[k][1][0]))     # nothing changed
    assert geo[6][0].valid.sum() > 20
    assert not np.array_equal(bits(trace[6][0][0]), bits(trace[6][1][0]))


def claim_ends_at_border(built, geo, arg, trace):
    g = geo[0][0]
    for e, last in ((g.ex, g.w - 1), (g.ey, g.h - 1)):
        assert (g.valid & (e == last)).any() and (g.valid & (e == 0)).any()
        assert (~g.valid & (e == last + 1)).any() and (~g.valid & (e == -1)).any()
        assert (~g.valid & (e > last + 900)).any() and (~g.valid & (e < -900)).any()


def claim_point_is_begin(built, geo, arg, trace):
    g = geo[0][0]
    same = (g.ex == g.bx) & (g.ey == g.by)
    assert same.sum() >= 3 and not (g.valid & same).any() and g.valid.any()


def claim_all_invalid_then_normal(built, geo, arg, trace):
    sc = _scans(built, geo)
    assert any(not a[0].valid.any() and a[0].inside and b[0].valid.any() and a[0].da.size == b[0].da.size
               for (_, a), (_, b) in zip(sc, sc[1:]))


def claim_one_point(built, geo, arg, trace):
    das = [int(g[0].da[0]) for _, g in _scans(built, geo)]
    assert all(g[0].da.size == 1 for _, g in _scans(built, geo))
    assert {0, 5, 16, 17, 31, 79, 80} <= set(das)


def claim_rint_ties(built, geo, arg, trace):
    axis = int(arg)
    wrong = kc.geometry(built, "floor")
    g = geo[0][0]
    side = (g.w, g.h)[axis]
    xy, _, pose = built.steps[0]
    t = kc.transformed(1.0, 0, pose, xy[:, 0], xy[:, 1])[axis]
    e = (g.ex, g.ey)[axis]
    assert e[t == F(-0.5)] == 0 and g.valid[t == F(-0.5)].all()          # -0.5 is cell 0, inside
    assert e[t == F(-1.5)] == -2 and (e[(t < F(-0.5)) & (t > F(-0.6))] == -1).all()
    assert (e[t == F(0.5)] == 0).all() and (e[t == F(1.5)] == 2).all() and (e[t == F(2.5)] == 2).all() and (e[t == F(3.5)] == 4).all()
    top = t == F(side - 0.5)
    assert top.sum() == 1 and e[top] == (side if side % 2 == 0 else side - 1) and bool(g.valid[top]) == (side % 2 == 1)
    differs = begin_ties = 0
    for k, lv in _scans(built, geo):
        a, b = lv[0], wrong[k][0]
        differs += int(((a.ex != b.ex) | (a.ey != b.ey)).sum())
        begin_ties += (a.bx, a.by) != (b.bx, b.by)
    assert differs >= 6 and begin_ties >= 2                              # ties where floor(x + 0.5) goes the other way: end points, begin cells
    begins = [((lv[0].bx, lv[0].by)[axis], lv[0].inside) for _, lv in _scans(built, geo)]
    assert (0, True) in begins and (-1, False) in begins and ((side, False) in begins or (side - 1, True) in begins)


def claim_state(built, geo, arg, trace):
    beyond = int(arg)
    combos = {(np.float32(v).tobytes(), int(u)) for v, u in kc.STATE_COMBOS}
    assert len(combos) == 9 * 12 + 4
    start = built.start[0]
    for k, lv in _scans(built, geo):
        g = lv[0]
        kind, c = kc.kinds(g), kc.cheb(g)
        region = (c >= kc.ZONE) if beyond else ((c < kc.ZONE) & (c > 0))
        before = trace[k][0][0]
        mark_free, mark_occ = 3 * k + 1, 3 * k + 2
        for q in range(4):
            cells = np.flatnonzero((kind == q) & region)
            got = {(start["value"][i].tobytes(), int(start["update_index"][i])) for i in cells}
            assert got == combos, (kc.KINDS[q], len(cells), len(got))
            # cells whose index equals this update's marks before it, and the neighbours of the marks
            idx = set(before["update_index"][cells].tolist())
            assert {mark_free - 2 if k == 0 else mark_free - 1, mark_free, mark_occ, mark_occ + 1, INT_MAX} <= idx, (k, q, sorted(idx))
            at_mark = cells[before["update_index"][cells] == mark_free]
            assert len({before["value"][i].tobytes() for i in at_mark}) >= 5
    assert (kc.geometry(built)[0][0].da.max() >= kc.ZONE)


def claim_fan_class(built, geo, arg, trace):
    for _, lv in _scans(built, geo):
        assert lv[0].valid.all() and (lv[0].cls == int(arg)).all()


def claim_shares_beyond_zone(built, geo, arg, trace):
    g = geo[0][0]
    assert any((kc.shared_offsets(g, i, j) >= kc.ZONE).any() for i, j in _pairs(g))


def claim_equal_slopes(built, geo, arg, trace):
    g = geo[0][0]
    eq = [(i, j) for i, j in _pairs(g) if _slope_gap(g, i, j) == 0]
    assert any(g.da[i] == g.da[j] for i, j in eq) and any(g.da[i] != g.da[j] for i, j in eq)
    assert {32, 64} <= {int(g.da[i]) for p in eq for i in p}


def claim_gap_at_most(built, geo, arg, trace):
    g = geo[0][0]
    gaps = [_slope_gap(g, i, j) for i, j in _pairs(g)]
    assert 0 < min(gaps) <= float(arg), min(gaps)


def claim_fan_of(built, geo, arg, trace):
    assert geo[0][0].valid.sum() == int(arg)


def claim_gap_buckets(built, geo, arg, trace):
    g = geo[0][0]
    diffs = {abs(kc.bucket(int(g.sdb[i]), int(g.da[i])) - kc.bucket(int(g.sdb[j]), int(g.da[j]))) for i, j in _pairs(g)}
    assert int(arg) in diffs, diffs


def claim_owner_ends_first(built, geo, arg, trace):
    g = geo[0][0]
    assert g.da[0] == g.da.min() and g.da[0] >= kc.ZONE + 8
    assert sum((kc.shared_offsets(g, 0, j) >= kc.ZONE).any() for j in range(1, g.da.size)) >= 3


def claim_shares_across_sign(built, geo, arg, trace):
    g = geo[0][0]
    assert any(g.sdb[i] * g.sdb[j] < 0 and (kc.shared_offsets(g, i, j) >= kc.ZONE).any() for i, j in _pairs(g))


def claim_bucket_clamp(built, geo, arg, trace):
    g = geo[0][0]
    assert (g.sdb == g.da).any() and (g.sdb == -g.da).any()
    assert kc.bucket(100, 100) == kc.NBUCK - 1 and kc.bucket(-100, 100) == 0
    assert (F(100) / F(100) + F(1.0)) * F(kc.NBUCK // 2) == kc.NBUCK       # (unclamped it would be one past the table)


def claim_end_crossed(built, geo, arg, trace):
    orders = set()
    for s in map(int, arg.split(",")):
        for _, lv in _scans(built, geo):
            g = lv[0]
            for i in np.flatnonzero(g.da == s):
                for j in np.flatnonzero(g.da > s):
                    if s in kc.shared_offsets(g, int(i), int(j)):
                        orders.add((s, bool(i < j)))
    assert orders == {(s, o) for s in map(int, arg.split(",")) for o in (False, True)}, orders


def _diagonal_classes(g):
    """Per diagonal cell (offset |dx| == |dy| > 0 from the begin cell): Chebyshev distance and which of x-major / y-major lines draw it."""
    fc, fl, ec, el = kc.touches(g)
    cells, lines = np.concatenate([fc, ec]), np.concatenate([fl, el])
    dy, dx = np.divmod(cells, g.w)
    dx, dy = dx - g.bx, dy - g.by
    on = (np.abs(dx) == np.abs(dy)) & (dx != 0)
    out = {}
    for c, l, r in zip(cells[on], lines[on], np.abs(dx[on])):
        out.setdefault((int(c), int(r)), set()).add(bool(g.major_x[l]))
    return out


def claim_diagonal_meeting(built, geo, arg, trace):
    d = _diagonal_classes(geo[0][0])
    both = [r for (_, r), s in d.items() if s == {True, False}]
    assert any(r < kc.ZONE for r in both) and any(r >= kc.ZONE for r in both) and max(both) >= 3 * kc.ZONE
    g = geo[0][0]
    assert (g.valid & (np.abs(g.sdb) == g.da) & g.major_x).sum() >= 3    # adx == ady: x-major


def claim_zone_diagonal_y_major_only(built, geo, arg, trace):
    for _, lv in _scans(built, geo):
        d = _diagonal_classes(lv[0])
        assert any(s == {False} and r < kc.ZONE for (_, r), s in d.items())


def claim_division_width(built, geo, arg, trace):
    w, h = built.size
    sc = _scans(built, geo)
    sizes = [lv[0].da.size for _, lv in sc]
    assert max(sizes) == kc.LDS_LINES + 1 and kc.LDS_LINES in sizes and all(lv[0].valid.all() for _, lv in sc)
    g0 = sc[0][1][0]
    assert g0.bx in (0, w - 1) and g0.by in (0, h - 1)
    for xm, side, other in ((True, w, h), (False, h, w)):
        have = set()
        for _, lv in sc:
            g = lv[0]
            m = g.major_x == xm
            have |= set(zip(g.da[m].tolist(), np.abs(g.sdb[m]).tolist()))
        for da in range(kc.ZONE, side):
            for db in kc.div_minors(da):
                if db <= other - 1 and not (db == da and not xm):       # (adx == ady is x-major)
                    assert (da, db) in have, (xm, da, db)
    assert (max(w, h) > 2048) == (built.size != (2048, 2048))


def claim_thin(built, geo, arg, trace):
    sc = _scans(built, geo)
    want = kc.THIN_DAS + (kc.THIN_COARSE if built.levels > 1 else ())
    das = [sorted(set(lv[0].da.tolist())) for _, lv in sc]
    assert [d[0] for d in das] == [da for da in want for _ in range(2)] and all(len(d) == 1 for d in das)
    assert [lv[0].da.size for _, lv in sc] == [1, 2] * len(want)
    assert (32767 - kc.ZONE) // 64 + 1 == 512
    for _, lv in sc[1::2]:
        assert abs(int(lv[0].sdb[0]) - int(lv[0].sdb[1])) == 1 and (kc.shared_offsets(lv[0], 0, 1) >= kc.ZONE).any()
    assert len({int(lv[0].cls[0]) for _, lv in sc}) == 2
    if built.levels > 1:
        coarse = {int(d) for _, lv in sc for d in lv[1].da[lv[1].valid]}
        assert {8190, 8191, 8192, 8193} <= coarse, coarse


def claim_count(built, geo, arg, trace):
    n = int(arg)
    sc = _scans(built, geo)
    assert all(lv[0].da.size == n for _, lv in sc)
    lone = [int(np.flatnonzero(lv[0].valid)[0]) for _, lv in sc[1:] if lv[0].valid.sum() == 1]
    assert lone == sorted(k for k in {0, n - 1, 1023, 1024} if k < n) and len(lone) == len(sc) - 1
    if n > 8:
        assert sc[0][1][0].valid.sum() > n // 2 and (~sc[0][1][0].valid).any()


def claim_count_alternating(built, geo, arg, trace):
    assert [lv[0].da.size for _, lv in _scans(built, geo)] == [kc.LDS_LINES, kc.LDS_LINES + 1] * 3


def claim_sector(built, geo, arg, trace):
    n = int(arg)
    sc = _scans(built, geo)
    assert all(lv[0].da.size == n for _, lv in sc)
    eighth = max(n // 8, 1)
    longs = [np.flatnonzero(lv[0].valid & (lv[0].da >= kc.ZONE)) for _, lv in sc]
    assert longs[0].size and longs[0].max() < eighth
    assert longs[1].size and longs[1].min() >= n - eighth
    assert longs[2].tolist() == [n // 2]
    assert longs[3].size >= n - 1
    assert (n < 16) == (n in (8, 9, 15))                                 # fewer lines than 2 per sector: the bounds collide


def claim_op(built, geo, arg, trace):
    ops = [s[0] for s in built.steps if not kc.is_scan(s)]
    assert ops == [arg]
    k = [kc.is_scan(s) for s in built.steps].index(False)
    assert 0 < k < len(built.steps) - 1 and built.steps[k - 1][0].shape == built.steps[k + 1][0].shape     # the same count either side


def claim_levels(built, geo, arg, trace):
    L = int(arg)
    dims = kc.level_dims(built.size, L)
    assert built.levels == L
    if L == 8:
        assert dims[-1] in ((2, 2), (3, 2))
    if built.size == (258, 256) and L > 1:
        assert dims[1][0] % 2 == 1
    for _, lv in _scans(built, geo):
        assert all(g.inside for g in lv)
        if L > 1:
            v0 = lv[0].valid & (lv[0].da >= kc.ZONE)
            assert (v0 & lv[1].valid & (lv[1].da < kc.ZONE)).any()        # into the zone on the coarser level
            same = (lv[1].ex == lv[1].bx) & (lv[1].ey == lv[1].by)
            assert (lv[0].valid & same).any()                            # ... or into the begin cell


CLAIMS = {"octants": claim_octants, "octants_x": claim_octants_x, "short_then_long": claim_short_then_long,
          "begin_on_border": claim_begin_on_border, "begin_outside": claim_begin_outside, "ends_at_border": claim_ends_at_border,
          "point_is_begin": claim_point_is_begin, "all_invalid_then_normal": claim_all_invalid_then_normal, "one_point": claim_one_point,
          "rint_ties": claim_rint_ties, "state": claim_state, "fan_class": claim_fan_class, "shares_beyond_zone": claim_shares_beyond_zone,
          "equal_slopes": claim_equal_slopes, "gap_at_most": claim_gap_at_most, "fan_of": claim_fan_of, "gap_buckets": claim_gap_buckets,
          "owner_ends_first": claim_owner_ends_first, "shares_across_sign": claim_shares_across_sign, "bucket_clamp": claim_bucket_clamp,
          "end_crossed": claim_end_crossed, "diagonal_meeting": claim_diagonal_meeting,
          "zone_diagonal_y_major_only": claim_zone_diagonal_y_major_only, "division_width": claim_division_width, "thin": claim_thin,
          "count": claim_count, "count_alternating": claim_count_alternating, "sector": claim_sector, "op": claim_op, "levels": claim_levels}


def test_case_names_are_unique_and_claims_known():
    assert len(NAMES) == len(set(NAMES))
    used = {k.split(":")[0] for c in kc.CASES for k in c.claims}
    assert all(c.claims for c in kc.CASES) and used == set(CLAIMS)      # no case without a claim, no claim without a case


@pytest.mark.parametrize("name", NAMES)
def test_case(det, npo, name):
    c = kc.by_name(name)
    built = c.build()
    assert built.cell_len == 1.0 and 1 <= built.levels <= 8
    cells = sum(w * h for w, h in kc.level_dims(built.size, built.levels))
    for step in built.steps:
        if kc.is_scan(step):
            xy, origin, pose = step
            assert xy.dtype == np.float32 and xy.shape[1] == 2 and pose[2] == 0.0
    small = cells <= (1 << 18)
    equal, trace = run(built, det, npo, keep=small)
    assert equal, "the rule differs from the oracles"
    geo = kc.geometry(built)
    for k in c.claims:
        head, _, arg = k.partition(":")
        CLAIMS[head](built, geo, arg, trace)


# ---- wrong copies of the rule ------------------------------------------------------------------------------------------------------
MUTANTS = {"no_half": ("zone_octants_128", "block_octants_192", "fan_unit_2047_n2_E"),
           "end_free": ("one_point", "state_zone"),
           "fixed_order": ("state_zone", "state_beyond", "state_zone_factors", "zone_octants_128"),
           "floor": ("round_x_16", "round_x_15", "round_y_16", "round_y_15"),
           "le50": ("state_zone", "state_beyond"),
           "zone_diag": ("rim_diag_zone",)}


@pytest.mark.parametrize("variant", sorted(MUTANTS))
def test_a_wrong_rule_is_caught(det, variant):
    """Negative check: e = a * db without da / 2; a <= da counted as free; the transitions in fixed free-then-occupied order;
    floor(x + 0.5) for rint; v <= 50 for v < 50; the zone's x-major class only on diagonal cells -- each must differ from the oracle
    on the named cases."""
    for name in MUTANTS[variant]:
        equal, _ = run(kc.by_name(name).build(), det, None, variant=variant, stop_at_mismatch=True)
        assert not equal, (variant, name)


# ---- the lone-line shortcut --------------------------------------------------------------------------------------------------------
def alone_from(gap, tilt, r_ulps):
    """The step from which the kernel takes a line to be alone (8191: never), float32 as in k5_cells' table phase, for slope gaps
    `gap` (float64 arrays, true values): each slope moved by 2.5e-7 against (tilt = -1) or away from (+1) the other, the hardware
    reciprocal r_ulps float32 steps off the correctly rounded one."""
    g = (gap + tilt * 5.0e-7).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        r = (F(1.0) / (g - F(1.0e-6))).astype(np.float32)
        for _ in range(abs(r_ulps)):
            r = np.nextafter(r, F(np.inf) if r_ulps > 0 else F(-np.inf))
        x = ((F(1.0625) * r).astype(np.float32) * F(1.0001)).astype(np.float32)
        xa = np.minimum(np.where(np.isfinite(x), x, 1e9).astype(np.int64) + 2, 8191)
    return np.where((g > F(4.0e-6)) & (gap > 0), xa, 8191)


def last_shared(da_i, sdb_i, da_j, sdb_j, chunk=1 << 22):
    """Per pair of same-class lines the largest major offset (>= 1) at which they draw the same cell, 0 if none."""
    out = np.zeros(da_i.size, np.int64)
    n = np.minimum(da_i, da_j)
    order = np.argsort(n, kind="stable")
    p = 0
    while p < order.size:
        q = p + 1
        while q < order.size and (q - p + 1) * int(n[order[q]]) <= chunk:
            q += 1
        ix = order[p:q]
        a = np.arange(1, int(n[ix].max()) + 1, dtype=np.int64)[None, :]
        di, dj, bi, bj = da_i[ix, None], da_j[ix, None], sdb_i[ix, None], sdb_j[ix, None]
        mi = np.sign(bi) * ((di // 2 + a * np.abs(bi)) // di)
        mj = np.sign(bj) * ((dj // 2 + a * np.abs(bj)) // dj)
        hit = (mi == mj) & (a <= n[ix, None])
        out[ix] = np.where(hit, a, 0).max(axis=1)
        p = q
    return out


def check_lone_bound(da_i, sdb_i, da_j, sdb_j):
    da_i, sdb_i, da_j, sdb_j = [np.asarray(v, np.int64) for v in (da_i, sdb_i, da_j, sdb_j)]
    gap = np.abs(sdb_i * da_j - sdb_j * da_i) / (da_i * da_j).astype(np.float64)
    last = last_shared(da_i, sdb_i, da_j, sdb_j)
    for tilt in (-1, 0, 1):
        for r_ulps in (-1, 0, 1):
            xa = alone_from(gap, tilt, r_ulps)
            bad = np.flatnonzero((xa < 8191) & (last >= xa))
            assert bad.size == 0, (tilt, r_ulps, da_i[bad[:4]], sdb_i[bad[:4]], da_j[bad[:4]], sdb_j[bad[:4]], last[bad[:4]], xa[bad[:4]])
    never = (gap <= 3.5e-6) | (gap == 0)                                # (4e-6 less the slopes' error: whatever the tilt)
    assert (alone_from(gap, 1, 1)[never & (gap + 5e-7 <= 4.0e-6)] == 8191).all() and (alone_from(gap, 0, 0)[gap == 0] == 8191).all()
    return gap


def test_lone_line_bound_exhaustive_16_to_48():
    """Every pair of signed slopes with 16 <= da <= 48 (one class; a pair of another class is its mirror image)."""
    da = np.concatenate([np.full(2 * d + 1, d) for d in range(16, 49)])
    sdb = np.concatenate([np.arange(-d, d + 1) for d in range(16, 49)])
    i, j = np.triu_indices(da.size, 1)
    gap = check_lone_bound(da[i], sdb[i], da[j], sdb[j])
    assert i.size > 2_000_000 and (gap == 0).sum() > 1000


def test_lone_line_bound_fans_and_sample():
    """All pairs of every fan case, and 20 000 seeded pairs with da up to 32767 -- half of them neighbours in slope."""
    q = [[], [], [], []]
    for c in kc.CASES:
        if c.name.startswith(("fan_", "rim_diag", "thin_")):
            built = c.build()
            for _, lv in _scans(built, kc.geometry(built))[:1 if c.name.startswith("fan_") else None]:    # (a fan's other scans are its permutations)
                g = lv[0]
                for i, j in _pairs(g):
                    for k, v in enumerate((g.da[i], g.sdb[i], g.da[j], g.sdb[j])):
                        q[k].append(int(v))
    assert len(q[0]) > 3000
    gap = check_lone_bound(*q)
    assert (gap == 0).any() and ((gap > 0) & (gap <= 4e-6)).any()
    rng = np.random.default_rng(5)
    n = 20000
    da_i = np.exp(rng.uniform(np.log(16), np.log(32767), n)).astype(np.int64)
    da_j = np.exp(rng.uniform(np.log(16), np.log(32767), n)).astype(np.int64)
    da_i[:50], da_j[:50] = 32767, rng.integers(32000, 32768, 50)
    sdb_i = (rng.uniform(-1, 1, n) * da_i).astype(np.int64)
    sdb_j = (rng.uniform(-1, 1, n) * da_j).astype(np.int64)
    near = np.arange(n) % 2 == 0
    sdb_j[near] = np.clip(np.rint(sdb_i[near] / da_i[near] * da_j[near]).astype(np.int64) + rng.integers(-1, 2, near.sum()), -da_j[near], da_j[near])
    gap = check_lone_bound(da_i, sdb_i, da_j, sdb_j)
    assert ((gap > 0) & (gap < 1e-3)).sum() > 1000


# ---- the step lanes' division ------------------------------------------------------------------------------------------------------
def test_float_division_estimate_within_one():
    """K5_FETCH on maps of up to 2048 a side: m = (int)((float)e * rcp(da)), settled by one remainder fix-up, needs the estimate
    within one of e / da: every da in 16 .. 2047 with the db of the division-width cases, e at the ends of each block of 64 steps
    and at the end cell, the reciprocal at the three float32 values around 1 / da."""
    rows = []
    for da in range(kc.ZONE, 2048):
        i = np.unique(np.concatenate([np.arange(kc.ZONE, da + 1, 64), np.arange(kc.ZONE + 63, da + 1, 64), [da]]))
        for db in kc.div_minors(da):
            rows.append(np.stack([np.full(i.size, da), da // 2 + i * db], 1))
    rows = np.concatenate(rows).astype(np.int64)
    da, e = rows[:, 0], rows[:, 1]
    assert e.max() < 2 ** 24 and e.max() > 2 ** 21 and rows.shape[0] > 300000
    r0 = (F(1.0) / da.astype(np.float32)).astype(np.float32)
    for r in (np.nextafter(r0, F(0)), r0, np.nextafter(r0, F(1))):
        m = (e.astype(np.float32) * r).astype(np.float32).astype(np.int64)
        assert np.abs(m - e // da).max() <= 1
