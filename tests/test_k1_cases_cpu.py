"""The K1 edge cases (tests/k1_cases.py) on the CPU: `expected()` -- the reference rule restated once -- equals the C oracle and the NumPy
oracle on every case; every case's claim about the kernel's tile steps holds by the restated planner; the restated planner's bands cover
every in-map row exactly once within the budget; and each wrong copy of the rule fails a named case (the suite has teeth)."""
import numpy as np
import pytest

import k1_cases as kc


@pytest.fixture(scope="module")
def det(oc):
    oc.set_trig_mode(oc.TRIG_DET)
    yield oc
    oc.set_trig_mode(oc.TRIG_LIBM)


_BUILT = {}


def built(name):
    if name not in _BUILT:
        c = kc.by_name(name)
        b = c.build()
        if c.claims.get("big"):
            return b                                                     # (128 MiB maps, 2^20 rays: not kept)
        _BUILT[name] = b
    return _BUILT[name]


NAMES = [c.name for c in kc.CASES]


def test_case_list():
    assert len(set(NAMES)) == len(NAMES) and {c.group for c in kc.CASES} == set("ABCDEFGIS")
    for g in "ABCDEFGIS":
        assert sum(c.group == g for c in kc.CASES) >= 4, g


@pytest.mark.parametrize("name", NAMES)
def test_expected_is_both_oracles(oc, npo, name):
    b = built(name)
    size, pix, xy, pxcs = b
    dist, idx, best = kc.expected(b)
    od, oi, ob = oc.distance_batch_pxcs(pix.reshape(-1), size, xy, pxcs)
    assert (od == dist).all() and (oi, ob) == (idx, best), (name, np.flatnonzero(od != dist)[:8])
    if xy.shape[0] * pxcs.shape[0] <= 1 << 22:
        nd = npo.distance_batch_pxcs(pix.reshape(-1), size, xy, pxcs)
        assert (nd == dist).all() and npo.argmin_first(nd) == idx, name


@pytest.mark.parametrize("name", [c.name for c in kc.CASES if not c.claims.get("big")])
def test_pose_form_gives_the_cases_pxcs(det, name):
    """One pixel per metre: the poses (px - 0.5, py - 0.5, 0) and the mode-1 jitters from the first of them give the case's pxcs exactly."""
    b = built(name)
    pf = kc.pose_form(b)
    c = kc.by_name(name)
    if pf is None:
        assert c.group in "AS" or b[3].shape[0] < 2, name                # (quarter turns, -0.0, seeded rotations, K = 1)
        return
    pose, offs, poses = pf
    assert (det.poses_to_pxcs(poses, 1.0) == b[3]).all(), name
    if poses.shape[0] <= 2049 and b[2].shape[0] <= 4097:
        bi, bpose, bd, all_d = det.search(b[1].reshape(-1), b[0], 1.0, b[2], pose, offs)
        dist, idx, best = kc.expected(b)
        assert (all_d == dist).all() and (bi, bd) == (idx, best), name


# ---- what the cases claim -----------------------------------------------------------------------------------------------------------
CLAIMED = [c.name for c in kc.CASES if "kinds" in c.claims]


@pytest.mark.parametrize("name", CLAIMED)
def test_claimed_step_kinds(name):
    c = kc.by_name(name)
    b = built(name)
    want = c.claims["kinds"]
    if "one_piece_of" in c.claims:
        # many groups: one ray range per group, so the whole one-spot scan is ONE piece of that many rays in every workgroup
        nr, ng = c.claims["one_piece_of"], b[3].shape[0] // 1024
        assert b[2].shape[0] == nr and len(np.unique(b[2], axis=0)) == 1 and b[3].shape[0] == ng * 1024
        assert kc.first_launch_ranges(ng, nr) == 1 and kc.first_launch_ranges(1, nr) > 1
        for g in (0, 1, 2, ng - 1):                                      # (the groups repeat with period 3)
            p = kc.plan_piece(kc.ray_box(kc.bounds_of(b[3][g * 1024:(g + 1) * 1024]), b[2]), nr, b[0])
            assert {p.kind} == want and p.nsteps == 1, (name, g, p)
    elif kc.one_piece(b):
        steps = kc.steps_of(b)
        assert len(steps) == 1                                           # (one group of 1024)
        assert {k for k, _, _ in steps[0]} == want, (name, steps)
        if "plan" in c.claims:
            p = kc.plan_piece(kc.ray_box(kc.bounds_of(b[3]), b[2]), b[2].shape[0], b[0])
            for k, v in c.claims["plan"].items():
                assert getattr(p, k) == v, (name, k, p)
        if "split" in c.claims:
            assert [n for _, n, _ in steps[0]] == list(c.claims["split"]), (name, steps)
            assert kc.steps_of(b, nosplit=True)[0][0][0] == kc.BAND
        else:
            assert len(steps[0]) <= 1
    else:
        assert kc.spot_kinds(b) == want, name
    # the denormal tile address: which side of S * pitch2 + 2 S + 2^18 < 2^23 the tile is on
    if "denormal" in c.claims:
        p = kc.plan_piece(kc.ray_box(kc.bounds_of(b[3]), b[2]), b[2].shape[0], b[0])
        assert kc.denormal_ok(b[0], p.ww) == c.claims["denormal"]


@pytest.mark.parametrize("name", [c.name for c in kc.CASES if c.group == "C"])
def test_groups_of_512_never_pad(name):
    """The same boxes with 512-candidate groups (what a mode-1 search of up to 12 288 candidates takes): the tile is as wide as the box
    rounded to 8 px; with 1024-candidate groups it is the claimed, padded width."""
    b = built(name)
    box = kc.ray_box(kc.bounds_of(b[3]), b[2])
    plain = ((box[2] - (box[0] & ~7) + 1) + 7) & ~7
    p512 = kc.plan_piece(box, b[2].shape[0], b[0], group=512)
    assert p512.ww == plain and p512.xa == box[0] & ~7 and p512.kind == kc.SHARED, (name, p512)
    assert kc.plan_piece(box, b[2].shape[0], b[0], nopad=True).ww == plain
    assert kc.plan_piece(box, b[2].shape[0], b[0]).ww == kc.by_name(name).claims["plan"]["ww"] >= plain


@pytest.mark.parametrize("name", [c.name for c in kc.T_CASES])
def test_mode1_tie_case(det, name):
    """Equal minima whose headings sort the later flat index first: the C oracle's search agrees with the restated rule on the c = 1
    twin, the winner is the smallest flat index of the minima, and in theta order a later minimum comes before it."""
    tc = kc.t_by_name(name)
    b, pose, offs = kc.tie_heading_form(tc)
    dist, idx, best = kc.expected(b)
    bi, bpose, bd, all_d = det.search(b[1].reshape(-1), b[0], 1.0, b[2], pose, offs)
    assert (all_d == dist).all() and (bi, bd) == (idx, best), name
    minima = np.flatnonzero(dist == best)
    assert minima[0] == idx and minima.size >= 1
    theta = np.concatenate([[0.0], offs[:, 2]])
    order = np.argsort(theta, kind="stable")
    first_sorted = next(int(j) for j in order if dist[j] == best)
    if tc.order == "descending":                                         # (shuffled: whatever order the seed gives)
        assert (np.diff(offs[:, 2]) < 0).all()
        if minima.size > 1:
            assert first_sorted == minima[-1] != idx, (name, first_sorted, idx)   # (the first minimum in sorted order would be the wrong answer)


def test_address_cases_straddle_the_denormal_limit():
    got = {(c.name, c.claims["denormal"]) for c in kc.CASES if c.group == "I"}
    assert got == {("i_address_4096_w480", True), ("i_address_4096_w504", True), ("i_address_8192_w480", True), ("i_address_8192_w504", False)}
    assert kc.denormal_ok(8192, 488) and not kc.denormal_ok(8192, 496)


def test_group_a_reaches_its_edges():
    for S in kc.A_SIZES:
        b = built("a_border_%d" % S)
        fx, fy = kc.end_points(b)
        for v in kc.a_values(S):
            assert (fx[0] == np.float32(v)).any() and (fy[0] == np.float32(v)).any(), (S, v)
        assert (fx == -0.75).any() and int(np.trunc(-0.75)) == 0
        box = kc.ray_box(kc.bounds_of(b[3]), b[2])
        assert box[0] < 0 and box[1] < 0 and box[2] >= S and box[3] >= S
        bi = built("a_inside_%d" % S)
        assert kc.ray_box(kc.bounds_of(bi[3]), bi[2]) == (0, 0, S - 1, S - 1)
        bo = built("a_outside_%d" % S)
        assert (kc.expected(bo)[0] == kc.INT_MAX).all()
        bz = built("a_negzero_%d" % S)
        fxz, _ = kc.end_points(bz)
        assert np.signbit(fxz[0, 0]) and fxz[0, 0] == 0 and kc.expected(bz)[0][0] != kc.INT_MAX


def test_bands_pay_rule():
    """Two bands pay from 15 rays on; no piece of 7 .. 11 rays is banded with 2, 3 or 4 bands (so the split's `nr >= 8` edge is out of
    reach and the halves are tested from 15 rays on)."""
    assert kc.bands_pay_from(2) == 15
    assert kc.bands_pay_from(3) is None and kc.bands_pay_from(4) is None   # 3 * 1.9 > 4.5: never
    for nr in range(1, 65):
        for nb in (2, 3, 4):
            p = kc.plan_piece((104, 300, 104 + 503, 300 + 60 * nb - 1), nr, 1024)
            assert p.nb == nb and (p.kind == kc.BAND) == (nb == 2 and nr >= 15), (nr, nb, p)
    for nr in (15, 16, 17, 18, 19):
        h1 = (nr // 2 + 1) & ~1
        assert kc.by_name("b_halves_%d" % nr).claims["split"] == (h1, nr - h1) and h1 in (8, 10)


def test_f_cases_reach_their_edges():
    for kind in (kc.SHARED, kc.BAND, kc.GLOBAL):
        for where in ("first", "middle", "last"):
            b = built("f_zero_only_%s_%s" % (kind, where))
            S = b[0]
            fx, fy = kc.end_points(b)
            ok = (fx >= 0) & (fx < S) & (fy >= 0) & (fy < S)
            assert ok[0].sum() == 1
            r = int(np.flatnonzero(ok[0])[0])
            assert b[1][int(fy[0, r]), int(fx[0, r])] == 0
            dist = kc.expected(b)[0]
            assert dist[0] == 0
            if kind != kc.SHARED:
                assert ok[1].sum() == 0 and dist[1] == kc.INT_MAX
            pos = int(np.flatnonzero(kc.sorted_rays(b[2]) == r)[0])
            assert {"first": pos == 0, "last": pos == b[2].shape[0] - 1, "middle": 12 < pos < 27}[where], (where, pos)
    for R in kc.F_R:
        for rem, nm in ((0, "0"), (1, "1"), (R - 1, "Rm1")):
            b = built("f_sum_mod_%d_%s" % (R, nm))
            fx, fy = kc.end_points(b)
            s = int(b[1][fy[0].astype(int), fx[0].astype(int)].astype(np.int64).sum())
            assert s > 0 and (s * 1024) % R == rem and b[2].shape[0] == R
        b = built("f_sum_largest_%d" % R)
        assert kc.expected(b)[0][0] == 65535 * 1024 and (R < 64 or 65535 * R * 1024 >= 2 ** 32)
    for nm, first in (("0", 0), ("1023", 1023), ("1024", 1024), ("last", 2048), ("1023_1024", 1023)):
        d, idx, best = kc.expected(built("f_tie_first_%s" % nm))
        assert idx == first and (d == best).sum() >= (2 if nm != "last" else 1)
    d, idx, _ = kc.expected(built("f_tie_uniform"))
    assert idx == 0 and (d == d[0]).all()


def test_g_winner_is_the_last_candidate():
    for K in kc.G_COUNTS:
        d, idx, best = kc.expected(built("g_count_%d" % K))
        assert d.shape[0] == K and idx == K - 1 and (K == 1 or (d[:-1] > best).all())


def test_e_every_ray_its_own_block():
    for R in (16, 17, 64, 600):
        xy = built("e_own_blocks_%d" % R)[2]
        s = xy[kc.sorted_rays(xy)]
        assert (np.abs(np.diff(s, axis=0)).max(axis=1) > 128).all() and len(np.unique(xy, axis=0)) == R
    assert kc.RAY_LIMIT == 1 << 20 and 65535 * (kc.RAY_LIMIT - 1) < 1 << 36


# ---- the restated planner: every in-map row in exactly one band, within the budget ---------------------------------------------------
@pytest.mark.parametrize("kb", [1, 8, 16, 24, 60])
def test_planner_bands_cover_every_row_once(kb):
    budget = kb * 1024
    for w in range(8, 521, 8):
        for x0 in (104, 1024 - w):
            for H in list(range(1, 140)) + list(range(140, 601, 7)) + [511, 512, 513, 599, 600]:
                for nopad in (False, True):
                    p = kc.plan_piece((x0, 10, x0 + w - 1, 10 + H - 1), 64, 1024, budget, 1024, nopad)
                    if p.kind == kc.GLOBAL:
                        continue
                    assert p.ww <= 512 and p.ww * 2 * max(h for _, h in p.bands) <= budget, (w, H, p)
                    assert p.xa % 8 == 0 and p.xa >= 0 and p.xa <= x0 and p.xa + p.ww >= x0 + w and p.xa + p.ww <= 1024, (w, H, p)
                    assert all(h >= 1 for _, h in p.bands), (w, H, p)          # no band is empty
                    rows = [y for y0, h in p.bands for y in range(y0, y0 + h)]
                    assert rows == list(range(10, 10 + H)), (w, H, p)          # every row in exactly one band


# ---- teeth: each wrong copy of the rule fails a named case ---------------------------------------------------------------------------
TEETH = {"floor": "a_border_8", "le_size": "a_border_16", "div_count": "a_border_64", "max_when_sum0": "f_zero_only_band_first",
         "mul32": "f_sum_largest_1079", "last_min": "f_tie_uniform", "contracted": "s_rotations_contracted"}


@pytest.mark.parametrize("wrong", kc.WRONG)
def test_wrong_copy_fails_its_case(wrong):
    b = built(TEETH[wrong])
    good, bad = kc.expected(b), kc.expected(b, wrong)
    assert (good[0] != bad[0]).any() or good[1] != bad[1], wrong


def test_contracted_seed_is_the_first_that_separates():
    assert kc.find_contracted_seed() == kc.CONTRACTED_SEED_FOUND


# ---- H: the mode-1 cases ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in kc.H_CASES])
def test_h_case(det, npo, name):
    """Both oracles agree under deterministic trigonometry, some candidate scores, and the heading range is where the name says."""
    c = kc.h_by_name(name)
    pix = kc.pattern(c.size).reshape(-1)
    bi, pose, bd, all_d = det.search(pix, c.size, 1.0, c.xy, c.pose, c.offs)
    ni, _, nd, nall = npo.search(pix, c.size, 1.0, c.xy, c.pose, c.offs)
    assert (bi, bd) == (ni, nd) and (all_d == nall).all()
    if "pad_only" not in name or c.xy.max() < 200:
        assert (all_d != kc.INT_MAX).any()
    th = (np.float32(c.pose[2]) + c.offs[:, 2]).astype(np.float64)
    hi, lo = th.max(), min(th.min(), float(c.pose[2]))
    k = np.round(hi / kc.HALF_PI)
    if "ends_on" in name:
        assert abs(hi - k * kc.HALF_PI) < 1e-6
    if "5e-4_inside" in name:
        assert 3e-4 < k * kc.HALF_PI - hi < 7e-4
    if "2e-3_outside" in name:
        assert 1.5e-3 < hi - k * kc.HALF_PI < 2.5e-3
    if "span_6.1" in name:
        assert 6.05 < hi - lo < 6.2
    if "span_6.3" in name:
        assert hi - lo > 6.2832
    if "straddles" in name:
        assert lo < np.sign(c.pose[2]) * np.pi < hi
    if "pad_only" in name:
        assert (c.offs[:, 2] == 0).all()
