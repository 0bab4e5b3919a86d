"""The K4 edge cases (tests/k4_cases.py) on the CPU: every scan of every case through the C oracle (Grid.hessian, estimate_step,
match, match_pyramid at T) and through np_oracle's hessian_terms, against the restated rule (kc.geometry, kc.sums_ref, kc.step) and,
for the "exact" family, against kc.expected(); the exactness condition of that family and the order sensitivity of the other; what
each case claims (which points are in the map, which index is informative, chunk residues and lengths, which branch of the step is
taken), asserted from the case's own numbers; and ten wrong copies of the rule that each fail a named case and pass a benign one."""
import fractions

import numpy as np
import pytest

import k4_cases as kc

F = np.float32
NAMES = [c.name for c in kc.CASES]
ALL_T = (1, 2, 3, 4, 7, 16, 63, 64)


@pytest.fixture(scope="module")
def det(oc):
    oc.set_trig_mode(oc.TRIG_DET)
    yield oc
    oc.set_trig_mode(oc.TRIG_LIBM)


def same_bits(a, b):
    """Equal bit for bit, except that any NaN equals any NaN (tests/test_gpu_hector_refsum.py)."""
    a = np.ascontiguousarray(a, np.float32).ravel(); b = np.ascontiguousarray(b, np.float32).ravel()
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all() and (a.view(np.uint32)[~na] == b.view(np.uint32)[~nb]).all())


def pyramid(oc, b):
    ref = oc.make_pyramid(1.0, b.size[0], b.size[1], b.levels)
    for l, g in enumerate(ref):
        g.cells["value"][:] = b.cells[l]
        g.cells["update_index"][:] = -1
    return ref


def close(ref):
    for g in ref:
        g.close()


def exactness(g):
    """The condition of the "exact" family on one level's terms: every term a multiple of 2^-e, the |terms| summing below
    2^(24 - e) -- then every partial sum in every order is a multiple of 2^-e below 2^24 * 2^-e: a binary32 number."""
    for k in range(10):
        t = g.terms[k]
        if np.isnan(t).any():                                           # (the sum is NaN in every order)
            continue
        assert np.isfinite(t).all()
        nz = [fractions.Fraction(float(v)) for v in t[t != 0]]
        if not nz:
            continue
        e = max(f.denominator for f in nz).bit_length() - 1
        assert all(f.denominator & (f.denominator - 1) == 0 for f in nz)
        assert sum(abs(f) for f in nz) * 2 ** e < 2 ** 24, (k, e)


@pytest.mark.parametrize("name", NAMES)
def test_case_vs_oracles(det, npo, name):
    oc = det
    b = kc.by_name(name).build()
    ref = pyramid(oc, b)
    dims = kc.level_dims(b.size, b.levels)
    nps = []
    for l, (w, h) in enumerate(dims):
        g = npo.NpGrid(F(2 ** l), w, h, trig="det")
        g.set_prob_table(kc.prob_of(b.cells[l]))
        nps.append(g)
    nan_case = "nan_tap" in kc.by_name(name).claims or "nan_sums" in kc.by_name(name).claims
    differs = False
    try:
        for si, xy in enumerate(b.scans):
            for l in range(b.levels):
                pm = kc.map_pose(b.pose, l)
                assert same_bits(pm, ref[l].map_pose(np.array(b.pose, np.float32)))
                g = kc.geometry(b.cells, b.size, l, pm, xy)
                terms, P = nps[l].hessian_terms(xy, pm)
                assert same_bits(terms, g.terms[:9]) and same_bits(P, g.P), (name, si, l)
                for T in sorted(set(b.Ts) | {1}):
                    H, d = kc.pack(kc.sums_ref(g, T))
                    Hr, dr = ref[l].hessian(xy, pm, T)
                    assert same_bits(H, Hr) and same_bits(d, dr), (name, si, l, T, H, Hr, d, dr)
                    est, _ = kc.step(H, d, pm)
                    ok, er = ref[l].estimate_step(xy, pm, T)
                    assert same_bits(est, er), (name, si, l, T, est, er)
                if b.family == "exact" and not nan_case:
                    g64 = kc.geometry(b.cells, b.size, l, pm, xy, np.float64)
                    fin = np.isfinite(xy).all(axis=1) & (np.abs(xy) < 1e20).all(axis=1)
                    assert (g64.terms[:, fin] == g.terms[:, fin].astype(np.float64)).all(), (name, si, l)
                    assert (g64.inmap == g.inmap).all() and (g64.idx == g.idx).all()
                    exactness(g)
                    H, d, res, n_in = kc.expected(g)
                    for T in ALL_T:
                        Hr, dr = ref[l].hessian(xy, pm, T)
                        assert same_bits(H, Hr) and same_bits(d, dr), (name, si, l, T)
                        assert same_bits(kc.sums_ref(g, T)[9], res)
                elif b.family == "order":
                    s = [kc.sums_ref(g, T)[:9] for T in ALL_T if T != b.Ts[0]]
                    mine = kc.sums_ref(g, b.Ts[0])[:9]
                    differs |= any(not same_bits(mine, o) for o in s)
            # the matches the device test asks for
            hint = np.array(b.pose, np.float32)
            for T in b.Ts:
                for l in range(b.levels):
                    want = ref[l].match(xy, hint, 1, T)
                    if xy.shape[0]:
                        est, _ = kc.step(*kc.pack(kc.sums_ref(kc.geometry(b.cells, b.size, l, kc.map_pose(b.pose, l), xy), T)), kc.map_pose(b.pose, l))
                        back = np.array([est[0] * F(2 ** l), est[1] * F(2 ** l), est[2]], np.float32)
                        if not np.isnan(back).any() and abs(float(back[2])) < 3.0:
                            assert same_bits(want[:2], back[:2]), (name, si, l, T, want, back)
                    else:
                        assert same_bits(want, hint)
                oc.match_pyramid(ref, xy, hint, b.iters, n_threads=T)
        if b.family == "order":
            n = b.scans[0].shape[0]
            # (three terms or fewer are added left to right by every chunking; from four on the order shows)
            assert differs or n < 4, name
    finally:
        close(ref)


@pytest.mark.parametrize("name", [c.name for c in kc.CASES if c.build().batch and c.build().family == "exact"])
def test_batch_hints_are_exact_too(name):
    """The hints of a batch are distinct, dyadic, and keep the sums exact: at T = 0 a batch entry (256 lanes from nine hints on)
    must then equal its single match (512 lanes) bit for bit."""
    b = kc.by_name(name).build()
    hints = kc.batch_hints(b, max(b.batch))
    assert len({tuple(h) for h in hints.tolist()}) == max(b.batch) and (hints[0] == np.array(b.pose, np.float32)).all()
    assert min(b.batch) < kc.WIDE_FROM <= max(b.batch)                 # both widths
    for h in hints:
        for l in range(b.levels):
            pm = kc.map_pose(h, l)
            g = kc.geometry(b.cells, b.size, l, pm, b.scans[0])
            assert (kc.geometry(b.cells, b.size, l, pm, b.scans[0], np.float64).terms == g.terms).all()
            exactness(g)


def test_exact_family_covers_every_pass_and_window():
    """The counts of group B lie on both sides of every structural count of the kernel."""
    ns = {int(c.claims[0].split(":")[1]) for c in kc.CASES if c.claims[0].startswith("count:")}
    for m in (64, 256, 512, kc.W_BATCH, kc.W_SINGLE, kc.LDS_PTS, 2 * kc.W_BATCH, 2 * kc.W_SINGLE):
        assert {m - 1, m, m + 1} <= ns, m
    assert {0, 1, 2, 4097} <= ns


@pytest.mark.parametrize("name", [c.name for c in kc.CASES if c.claims[0].startswith("count:") and c.name != "count_0"])
def test_count_claims(name):
    b = kc.by_name(name).build()
    xy = b.scans[0]
    n = xy.shape[0]
    g = kc.geometry(b.cells, b.size, 0, kc.map_pose(b.pose, 0), xy)
    inf = kc.informative_indices(n)
    assert np.flatnonzero(g.inmap).tolist() == inf
    assert {0, n - 1} <= set(inf)
    for m in kc.STRIDES:
        for k in range(m, n + 1, m):
            assert k - 1 in inf and (k in inf or k == n)
    # every informative point changes every sum it can: losing or doubling one changes H, dTr and the residual
    assert (g.terms[:, inf] != 0).all(), name
    H, d, res, n_in = kc.expected(g)
    assert n_in == len(inf)
    rest = fractions.Fraction(float(res)) - (n - n_in)
    assert 0 < rest < n_in                                             # (residual = the points outside + a fraction per informative point)
    # neighbours differ, so that one lost and its neighbour doubled does not cancel
    for i, j in zip(inf[:-1], inf[1:]):
        if j == i + 1:
            assert not (g.terms[:, i] == g.terms[:, j]).all(), (i, j)


def frac(v):
    return fractions.Fraction(float(v))


@pytest.mark.parametrize("name", [c.name for c in kc.CASES if c.claims[0].startswith("border:")])
def test_border_claims(name):
    c = kc.by_name(name)
    b = c.build()
    l = int(c.claims[0].split(":")[1])
    w, h = kc.level_dims(b.size, b.levels)[l]
    xy = b.scans[1]
    assert (b.scans[0] == xy[:-len(kc.SPECIAL)]).all() and np.isfinite(b.scans[0]).all()
    g = kc.geometry(b.cells, b.size, l, kc.map_pose(b.pose, l), xy)
    # the in-map test restated in rational arithmetic on the exact position (x + tx) / 2^l
    fin = np.isfinite(xy).all(axis=1)
    for i in np.flatnonzero(fin & (np.abs(xy) < 1e20).all(axis=1)):
        ex = (frac(xy[i, 0]) + frac(b.pose[0])) / 2 ** l
        ey = (frac(xy[i, 1]) + frac(b.pose[1])) / 2 ** l
        assert frac(g.cx[i]) == ex and frac(g.cy[i]) == ey, (name, i)
        assert bool(g.inmap[i]) == (0 <= ex <= w - 2 and 0 <= ey <= h - 2), (name, i)
        if g.inmap[i]:
            assert g.idx[i] == int(ey // 1) * w + int(ex // 1) and g.idx[i] + w + 1 < w * h
    assert not g.inmap[~fin].any() and not g.inmap[(np.abs(xy) > 1e20).any(axis=1)].any()
    limx, limy = F(w - 2.0), F(h - 2.0)
    # a point on each limit (inside), one ulp beyond (outside), on zero, below zero, and the far corner: the last valid idx
    for lim, c_ in ((limx, g.cx), (limy, g.cy)):
        assert g.inmap[c_ == lim].any() and (c_ == np.nextafter(lim, F(np.inf))).any() and not g.inmap[c_ == np.nextafter(lim, F(np.inf))].any()
        assert g.inmap[c_ == 0].any() and (c_ == F(-0.5)).any()
    assert (g.idx[g.inmap] == (h - 2) * w + w - 2).any()
    if "last_idx" in c.claims:
        assert max(w, h) == 32768 and (g.idx[g.inmap] + w + 1 == w * h - 1).any()
    if b.pose[0] == 0 and l == 0 and min(w, h) >= 4:
        assert g.inmap[g.cx == F(kc.DEN)].any() and g.inmap[g.cy == F(kc.DEN)].any()    # (the smallest denormal is inside)
        neg0 = np.signbit(xy[:, 0]) & (xy[:, 0] == 0)
        assert neg0.any() and not np.signbit(g.cx[neg0]).any()         # (x = -0.0 arrives as cx = +0: the transform ends in + m31 = +0)
    if len(b.scans) > 2:
        assert len(b.scans) == 2 + xy.shape[0] and all((s == xy[i:i + 1]).all() or np.isnan(s).any() for i, s in enumerate(b.scans[2:]))


def test_chunk_claims():
    """Group D: chunk starts of every residue mod 4 relative to the window, the chunk lengths the issue lists, every loop of
    hs_chain, T > n, a short and an empty last chunk, chunks across the window boundary at both widths, n = W and W + 1."""
    lens, residues, paths, straddle = set(), set(), set(), set()
    cases = [tuple(map(int, c.claims[0].split(":")[1:])) for c in kc.CASES if c.claims[0].startswith("chunks:")]
    for T, n in cases:
        ch = kc.chunks(n, T)
        assert ch[0][0] == 0 and max(hi for _, hi in ch) == n and all(a[1] == b_[0] or b_[0] == n for a, b_ in zip(ch[:-1], ch[1:]))
        lens.add(ch[0][1] - ch[0][0])
        for W in (kc.W_BATCH, kc.W_SINGLE):
            seg = kc.segments(n, T, W)
            assert sum(hi - lo for _, _, lo, hi in seg) == n
            for c, wi, lo, hi in seg:
                residues.add(lo & 3)
                paths |= kc.chain_paths(lo, hi)
            per_chunk = {}
            for c, wi, lo, hi in seg:
                per_chunk.setdefault(c, set()).add(wi)
            if any(len(v) > 1 for v in per_chunk.values()):
                straddle.add(W)
    assert lens >= {1, 3, 4, 5, 31, 32, 33, 35, 63, 64, 65, 96, 97}
    assert residues == {0, 1, 2, 3} and paths == {"head", "body", "tail4", "tail1"}
    assert straddle == {kc.W_BATCH, kc.W_SINGLE}
    assert {(64, 1), (64, 5), (64, 63)} <= set(cases)                  # T > n
    assert kc.chunks(190, 64)[63] == (189, 190) and kc.chunks(130, 64)[44:] == [(130, 130)] * 20   # short, empty
    for W in (kc.W_BATCH, kc.W_SINGLE):
        assert (7, W) in cases and (7, W + 1) in cases
    # chain_paths against the sum itself: adding by the four loops is adding left to right
    assert kc.chain_paths(1, 2) == {"head"} and kc.chain_paths(0, 32) == {"body"} and kc.chain_paths(4, 8) == {"tail4"}
    assert kc.chain_paths(3, 40) == {"head", "body", "tail4"} and kc.chain_paths(0, 3) == {"tail1"}


STEP_CASES = [c.name for c in kc.CASES if c.claims[0].startswith("step:")]


@pytest.mark.parametrize("name", STEP_CASES)
def test_step_claims(det, name):
    c = kc.by_name(name)
    b = c.build()
    xy = b.scans[0]
    pm = kc.map_pose(b.pose, 0)
    g = kc.geometry(b.cells, b.size, 0, pm, xy)
    H, d = kc.pack(kc.sums_ref(g, 1))
    est, branch = kc.step(H, d, pm)
    assert branch == c.claims[0].split(":")[1], (name, branch, H, d)
    ref = pyramid(det, b)
    try:
        ok, er = ref[0].estimate_step(xy, pm, 1)
        assert same_bits(est, er)
        if branch in ("h_zero", "singular"):
            assert same_bits(est, pm) and same_bits(ref[0].match(xy, np.array(b.pose, np.float32), 3, 1), np.array(b.pose, np.float32))
        if branch == "h_zero":
            assert not ok
        if branch == "singular":
            assert H[0, 0] != 0 and H[1, 1] != 0 and kc.invert_h(H) is None
        if branch == "clamp+":
            assert est[2] == F(0.2)
        if branch == "clamp-":
            assert est[2] == F(-0.2)
        if branch == "inside":
            assert 0 < abs(float(est[2])) < 0.2
    finally:
        close(ref)
    if "h11_zero" in c.claims:
        assert H[0, 0] == 0 and H[1, 1] != 0
    if "h22_zero" in c.claims:
        assert H[1, 1] == 0 and H[0, 0] != 0
    if "nan_sums" in c.claims:
        assert np.isnan(H[0, 2]) and H[0, 0] == 0
    if name == "step_all_out":
        assert not g.inmap.any() and not H.any() and not d.any()


def test_nan_tap_claim():
    b = kc.by_name("step_nan_tap").build()
    g = kc.geometry(b.cells, b.size, 0, kc.map_pose(b.pose, 0), b.scans[0])
    bad = np.isnan(g.P)
    assert bad.sum() == 1 and g.inmap[bad].all()                       # one point's taps, and it is inside the map
    H, d = kc.pack(kc.sums_ref(g, 1))
    assert np.isnan(H).all() and np.isnan(d).all()
    assert np.isnan(kc.step(H, d, kc.map_pose(b.pose, 0))[0]).all()


def first_level(name, rule=None, pad=0):
    b = kc.by_name(name).build()
    g = kc.geometry(b.cells, b.size, 0, kc.map_pose(b.pose, 0), b.scans[0], rule=rule)
    return kc.expected(g, pad)


def same_expected(a, b):
    return same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and same_bits(a[2], b[2]) and a[3] == b[3]


@pytest.mark.parametrize("rule, fails, passes", [
    ("ge", "border_16x16", "levels_1"), ("w1", "border_16x16", "levels_1"), ("limy_w", "border_24x16", "border_16x16"),
    ("idx_h", "border_24x16", "border_16x16"), ("trunc", "border_16x16", "levels_1"), ("out_zero", "count_63", "step_const_x")])
def test_wrong_geometry_rules(rule, fails, passes):
    """Each wrong copy of the point rule changes the expected sums of the case named for it, and of no case without that edge."""
    assert not same_expected(first_level(fails), first_level(fails, rule)), rule
    assert same_expected(first_level(passes), first_level(passes, rule)), rule
    if rule == "out_zero":
        b = kc.by_name(passes).build()                                 # (benign: no point of it lies outside)
        assert kc.geometry(b.cells, b.size, 0, kc.map_pose(b.pose, 0), b.scans[0]).inmap.all()


def test_wrong_padding_lanes():
    """A padding lane that adds 1 to the residual: wrong wherever n is no multiple of the pass, right where it is."""
    for name, per_pass in (("count_1", kc.W_SINGLE), ("count_1281", kc.W_BATCH), ("count_1537", kc.W_SINGLE)):
        n = kc.by_name(name).build().scans[0].shape[0]
        assert kc.padding_lanes(n, per_pass) > 0
        assert not same_expected(first_level(name), first_level(name, pad=kc.padding_lanes(n, per_pass)))
    assert kc.padding_lanes(1280, kc.W_BATCH) == 0 and kc.padding_lanes(1536, kc.W_SINGLE) == 0


def test_wrong_chunk_floor():
    """chunk = n / T rounded down loses the scan's tail (13 points at T = 3) -- and is the same where T divides n (679 at T = 7)."""
    for name, differs in (("chunk_T3_n13", True), ("chunk_T7_n679", False)):
        b = kc.by_name(name).build()
        g = kc.geometry(b.cells, b.size, 0, kc.map_pose(b.pose, 0), b.scans[0])
        assert same_bits(kc.sums_ref(g, b.Ts[0]), kc.sums_ref(g, b.Ts[0], floor=True)) != differs, name


def test_wrong_steps():
    def both(name, variant):
        b = kc.by_name(name).build()
        g = kc.geometry(b.cells, b.size, 0, kc.map_pose(b.pose, 0), b.scans[0])
        H, d = kc.pack(kc.sums_ref(g, 1))
        pm = kc.map_pose(b.pose, 0)
        return kc.step(H, d, pm)[0], kc.step(H, d, pm, variant)[0]
    for name in ("step_clamp_pos", "step_clamp_neg"):
        a, b_ = both(name, "no_clamp")
        assert not same_bits(a, b_) and abs(float(b_[2])) > 0.2
    assert same_bits(*both("step_inside", "no_clamp"))
    a, b_ = both("step_const_x_nan_point", "no_h_test")
    assert not same_bits(a, b_) and np.isnan(b_).any() and not np.isnan(a).any()
    assert same_bits(*both("step_const_x", "no_h_test"))               # (without the NaN the inverse refuses: the test is not needed)
    assert same_bits(*both("step_inside", "no_h_test"))
