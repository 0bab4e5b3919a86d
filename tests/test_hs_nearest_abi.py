"""CPU-side checks of the nearest-site field's interface (slamhip_hs_nearest_field, slamhip_hs_nearest_pairs,
slamhip_hsproc_nearest_pairs, slamhip_debug_nearest_field) and the NumPy restatements of its definition (include/slamhip.h,
slamhip_hs_nearest_field) that tests/test_gpu_hector_nearest.py compares the device with.

np_nearest_brute is the yardstick: for every cell the arg-min over ALL shifts in [-r, r]^2 of a padded site array by the key (D2,
sy, sx) -- the definition word for word.  np_nearest is a separable restatement (signed nearest site of a row by running maxima,
ties to the left; then the minimum of (o^2 + dy^2, dy) over the row shifts) for the larger cases of the GPU file; it is proved equal
to the brute force here, on the small arrays, before anything relies on it.  The library's hook runs a third formulation (site bits
by word, clz / ctz, magnitude bytes and signs apart, an early-exit column walk).  Everything is compared with == on integers.  No
compute calls on a device."""
import ctypes as C
import os

import numpy as np
import pytest

import test_hs_dfield_abi as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("slamhip_hs_nearest_field", "slamhip_hs_nearest_pairs", "slamhip_hsproc_nearest_pairs", "slamhip_debug_nearest_field")
SUMMARY = np.dtype([(n, np.int32) for n in ("n_counted", "n_ignored", "n_matched", "n_zero")] +
                   [(n, np.int64) for n in ("sum_d2", "sum_ex", "sum_ey", "sum_qx", "sum_qy", "sum_exqx", "sum_eyqy", "sum_exqy", "sum_eyqx")])
NONE, IGNORED = 32767, -32768
BIG = np.int64(1) << 40


# ---- the restatements --------------------------------------------------------------------------------------------------------------
def np_nearest_brute(cls, site_mask, r, rect, ties_right=False, closed=False):
    """N of every cell of rect -> (h, w, 2) int16: over all (dx, dy) in [-r, r]^2 with a site at (x + dx, y + dy) and dx^2 + dy^2 <
    r^2, the one with the least key (D2, y + dy, x + dx); NONE twice if there is none.  ties_right / closed: two WRONG copies of
    the rule (the larger column wins a tie; D2 <= r^2 counts) that the named cases below must tell from the right one."""
    x, y, w, h = rect
    s = D.np_sites(cls, site_mask, rect, r)
    K = np.int64(2 * r + 1)
    best = np.full((h, w), BIG, np.int64)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            d = dx * dx + dy * dy
            if d < r * r or (closed and d == r * r):
                key = (np.int64(d) * K + (dy + r)) * K + ((-dx if ties_right else dx) + r)
                np.minimum(best, np.where(s[r + dy:r + dy + h, r + dx:r + dx + w], key, BIG), out=best)
    out = np.full((h, w, 2), NONE, np.int16)
    ok = best < BIG
    kx = best % K - r
    out[..., 0][ok] = (-kx if ties_right else kx)[ok]
    out[..., 1][ok] = ((best // K) % K - r)[ok]
    return out


def np_nearest(cls, site_mask, r, rect):
    """The same field, separably: the signed offset o to the nearest site of the row with |o| < r (from the left by a running
    maximum of site positions, from the right by a running minimum; a tie goes left), then over the row shifts |dy| < r the least
    (o^2 + dy^2, dy) with the first part below r^2."""
    x, y, w, h = rect
    s = D.np_sites(cls, site_mask, rect, r)                                # (h + 2 r, w + 2 r)
    n = s.shape[1]
    idx = np.arange(n, dtype=np.int64)[None, :]
    dl = idx - np.maximum.accumulate(np.where(s, idx, -BIG), axis=1)       # to the last site at or left of the cell
    dr = np.minimum.accumulate(np.where(s, idx, BIG)[:, ::-1], axis=1)[:, ::-1] - idx
    o = np.where(dl <= dr, -dl, dr)[:, r:r + w]
    o2 = np.where(np.abs(o) < r, o * o, BIG)
    K = np.int64(2 * r + 1)
    best = np.full((h, w), BIG, np.int64); bo = np.zeros((h, w), np.int64)
    for dy in range(-r + 1, r):
        d2 = o2[r + dy:r + dy + h] + dy * dy
        key = np.where(d2 < r * r, d2 * K + (dy + r), BIG)
        better = key < best
        best = np.where(better, key, best); bo = np.where(better, o[r + dy:r + dy + h], bo)
    out = np.full((h, w, 2), NONE, np.int16)
    ok = best < BIG
    out[..., 0][ok] = bo[ok]
    out[..., 1][ok] = (best % K - r)[ok]
    return out


def np_pairs(field, rect, mask, ex, ey, ok):
    """The per-point records of one pose: `field` is N over rect (which contains E), the constant holds outside; IGNORED twice for an
    ignored point."""
    x0, y0, w, h = rect
    inside = ok & (ex >= x0) & (ex < x0 + w) & (ey >= y0) & (ey < y0 + h)
    out = np.full((ex.shape[0], 2), 0 if mask & 1 else NONE, np.int16)
    out[inside] = field[ey[inside] - y0, ex[inside] - x0]
    out[~ok] = IGNORED
    return out


def np_pair_summary(pairs, ex, ey):
    """slamhip_pair_summary of one pose's per-point records and end cells, in int64."""
    p = np.asarray(pairs).astype(np.int64)
    ok = p[:, 0] != IGNORED
    m = ok & (p[:, 0] != NONE)
    s = np.zeros(1, SUMMARY)[0]
    s["n_counted"] = ok.sum(); s["n_ignored"] = (~ok).sum(); s["n_matched"] = m.sum()
    s["n_zero"] = (m & (p[:, 0] == 0) & (p[:, 1] == 0)).sum()
    e_x, e_y = np.asarray(ex, np.int64)[m], np.asarray(ey, np.int64)[m]
    qx, qy = e_x + p[m, 0], e_y + p[m, 1]
    s["sum_d2"] = (p[m, 0] ** 2 + p[m, 1] ** 2).sum()
    s["sum_ex"] = e_x.sum(); s["sum_ey"] = e_y.sum(); s["sum_qx"] = qx.sum(); s["sum_qy"] = qy.sum()
    s["sum_exqx"] = (e_x * qx).sum(); s["sum_eyqy"] = (e_y * qy).sum(); s["sum_exqy"] = (e_x * qy).sum(); s["sum_eyqx"] = (e_y * qx).sum()
    return s


def d2_of(n):
    """dx^2 + dy^2 of a field of pairs, and where it is NONE."""
    p = n.astype(np.int64)
    none = (p[..., 0] == NONE) & (p[..., 1] == NONE)
    return np.where(none, -1, p[..., 0] ** 2 + p[..., 1] ** 2), none


# ---- the interface -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def capi():
    import slam.net_amd.build as b
    b.build()
    import slam.net_amd.capi as capi
    return capi


def check(capi, cls, mask, r, rect, brute=True):
    """The hook over rect against the restatements, and against the distance field's hook by the identity -> the hook's result."""
    got = capi.debug_nearest_field(cls, mask, r, rect)
    assert got.dtype == np.int16 and got.shape == (rect[3], rect[2], 2)
    sep = np_nearest(cls, mask, r, rect)
    assert np.array_equal(got, sep), (mask, r, rect, np.argwhere(got != sep)[:5].tolist())
    if brute:
        want = np_nearest_brute(cls, mask, r, rect)
        assert np.array_equal(got, want), (mask, r, rect, np.argwhere(got != want)[:5].tolist())
    f = capi.debug_distance_field(cls, mask, r, rect).astype(np.int64)
    d2, none = d2_of(got)
    assert np.array_equal(none, f == r * r) and np.array_equal(d2[~none], f[~none]), (mask, r, rect)
    assert ((got[..., 0] == NONE) == (got[..., 1] == NONE)).all()
    return got


def at(n, rect, x, y):
    return tuple(int(v) for v in n[y - rect[1], x - rect[0]])


def test_surface(capi):
    h = open(os.path.join(ROOT, "include", "slamhip.h")).read()
    native = open(os.path.join(ROOT, "bindings", "csharp", "SlamHip", "SlamHip.Native.cs")).read()
    assert capi.PAIR_SUMMARY == SUMMARY and capi.PAIR_SUMMARY.itemsize == 88                     # the struct size
    assert [capi.PAIR_SUMMARY.fields[n][1] for n in SUMMARY.names] == [0, 4, 8, 12] + list(range(16, 88, 8))   # no padding
    assert (capi.NEAREST_NONE, capi.NEAREST_IGNORED) == (NONE, IGNORED) == (np.iinfo(np.int16).max, np.iinfo(np.int16).min)
    assert "SLAMHIP_K_COUNT = 10" in h                                       # no new timing class
    L = capi.lib()
    for name in SYMBOLS:
        assert hasattr(L, name) and name in L._signatures and name in capi.declared_symbols() and name in native, name
    assert "struct PairSummary" in native
    assert len(L._signatures["slamhip_hs_nearest_field"][1]) == 10 and len(L._signatures["slamhip_hs_nearest_pairs"][1]) == 9
    assert len(L._signatures["slamhip_hsproc_nearest_pairs"][1]) == 12 and len(L._signatures["slamhip_debug_nearest_field"][1]) == 10
    import slam.net_amd.hector as hm
    assert hasattr(hm.MapRepMultiMap, "nearest_field") and hasattr(hm.MapRepMultiMap, "nearest_pairs")
    assert hasattr(hm.HectorSLAMProcessor, "NearestPairs") and hasattr(hm.HectorSLAMProcessor, "AlignStep")


def test_hook_refuses(capi):
    L = capi.lib()
    cls = np.zeros((4, 6), np.uint8)
    out = np.full((3, 3, 2), 77, np.int16)

    def rc(mask, r, w, h, cw=6, ch=4):
        return L.slamhip_debug_nearest_field(cls.ctypes.data_as(C.c_void_p), cw, ch, mask, r, 0, 0, w, h, out.ctypes.data_as(C.c_void_p))
    for mask, r, w, h in ((0, 3, 3, 3), (8, 3, 3, 3), (2, 0, 3, 3), (2, 256, 3, 3), (2, 3, 0, 3), (2, 3, 3, 0), (2, 3, 4097, 4096)):
        assert rc(mask, r, w, h) == capi.ERR_INVALID, (mask, r, w, h)
    assert rc(2, 3, 3, 3, cw=0) == capi.ERR_INVALID and rc(2, 3, 3, 3, ch=0) == capi.ERR_INVALID
    assert (out == 77).all()
    assert rc(2, 3, 3, 3) == 0 and (out == NONE).all()
    assert rc(1, 3, 3, 3) == 0 and (out == 0).all()


# ---- named cases -------------------------------------------------------------------------------------------------------------------
def test_lone_site(capi):
    c = np.zeros((21, 23), np.uint8)
    c[9, 12] = 1
    r = 7
    rect = (-r - 2, -r - 2, 23 + 2 * r + 4, 21 + 2 * r + 4)
    n = check(capi, c, 2, r, rect)
    ys, xs = np.mgrid[rect[1]:rect[1] + rect[3], rect[0]:rect[0] + rect[2]]
    near = (12 - xs) ** 2 + (9 - ys) ** 2 < r * r
    assert np.array_equal(n[..., 0][near], (12 - xs)[near]) and np.array_equal(n[..., 1][near], (9 - ys)[near]) and (n[~near] == NONE).all()
    assert at(n, rect, 12, 9) == (0, 0) and at(n, rect, 10, 13) == (2, -4)


def tie_lr():
    c = np.zeros((5, 11), np.uint8)
    c[2, 2] = c[2, 8] = 1                                                  # cell (5, 2) lies 3 from both
    return c, 2, 6, (-8, -8, 27, 21)


def test_left_right_tie_goes_left(capi):
    c, mask, r, rect = tie_lr()
    n = check(capi, c, mask, r, rect)
    assert at(n, rect, 5, 2) == (-3, 0) and at(n, rect, 5, 0) == (-3, 2) and at(n, rect, 6, 2) == (2, 0) and at(n, rect, 4, 2) == (-2, 0)


def test_up_down_tie_goes_up(capi):
    c = np.zeros((11, 5), np.uint8)
    c[2, 2] = c[8, 2] = 1
    rect = (-8, -8, 21, 27)
    n = check(capi, c, 2, 6, rect)
    assert at(n, rect, 2, 5) == (0, -3) and at(n, rect, 4, 5) == (-2, -3) and at(n, rect, 2, 6) == (0, 2)
    # a diagonal tie: the site above and to the RIGHT beats the one level with the cell and to the left
    c = np.zeros((9, 9), np.uint8)
    c[4, 1] = c[1, 4] = 1                                                  # both 3 from (4, 4)
    n = check(capi, c, 2, 5, (0, 0, 9, 9))
    assert at(n, (0, 0, 9, 9), 4, 4) == (0, -3)


def test_twelve_sites_at_25(capi):
    c = np.zeros((15, 15), np.uint8)
    offs = [(sx * a, sy * b) for a, b in ((3, 4), (4, 3)) for sx in (-1, 1) for sy in (-1, 1)] + [(5, 0), (-5, 0), (0, 5), (0, -5)]
    assert len(set(offs)) == 12 and all(dx * dx + dy * dy == 25 for dx, dy in offs)
    for dx, dy in offs:
        c[7 + dy, 7 + dx] = 1
    for r in (6, 9):
        n = check(capi, c, 2, r, (-r, -r, 15 + 2 * r, 15 + 2 * r))
        assert at(n, (-r, -r, 0, 0), 7, 7) == (0, -5)
    c[2, 7] = 0                                                            # without (0, -5): the smaller row still, then the smaller column
    n = check(capi, c, 2, 6, (0, 0, 15, 15))
    assert at(n, (0, 0, 0, 0), 7, 7) == (-3, -4)
    assert (check(capi, c, 2, 5, (7, 7, 1, 1)) == NONE).all()              # D2 = 25 is not below 5^2


def axis_r():
    c = np.zeros((3, 40), np.uint8)
    c[1, 20] = 1
    return c, 2, 9, (0, -10, 40, 23)


def test_axis_distance_r_is_none(capi):
    c, mask, r, rect = axis_r()
    n = check(capi, c, mask, r, rect)
    assert at(n, rect, 20 - r, 1) == (NONE, NONE) and at(n, rect, 20 + r, 1) == (NONE, NONE)
    assert at(n, rect, 20 - r + 1, 1) == (r - 1, 0) and at(n, rect, 20 + r - 1, 1) == (-(r - 1), 0)
    assert at(n, rect, 20, 1 - r) == (NONE, NONE) and at(n, rect, 20, 1 + r) == (NONE, NONE)
    assert at(n, rect, 20, 2 - r) == (0, r - 1) and at(n, rect, 20, r) == (0, -(r - 1))


def test_wrong_copies_fail_named_cases(capi):
    """Ties to the right fails the left/right tie; D2 <= r^2 fails the site at axis distance exactly r.  The right rule passes both."""
    c, mask, r, rect = tie_lr()
    got = capi.debug_nearest_field(c, mask, r, rect)
    assert np.array_equal(got, np_nearest_brute(c, mask, r, rect))
    wrong = np_nearest_brute(c, mask, r, rect, ties_right=True)
    assert not np.array_equal(got, wrong) and at(wrong, rect, 5, 2) == (3, 0)
    c, mask, r, rect = axis_r()
    got = capi.debug_nearest_field(c, mask, r, rect)
    assert np.array_equal(got, np_nearest_brute(c, mask, r, rect))
    wrong = np_nearest_brute(c, mask, r, rect, closed=True)
    assert not np.array_equal(got, wrong) and at(wrong, rect, 20 - r, 1) == (r, 0)


def test_radius_one(capi):
    rng = np.random.default_rng(1)
    c = rng.integers(0, 3, (9, 19)).astype(np.uint8)
    for mask in range(1, 8):
        rect = (-3, -3, 25, 15)
        n = check(capi, c, mask, 1, rect)
        site = D.np_sites(c, mask, rect, 0)
        assert (n[site] == 0).all() and (n[~site] == NONE).all()


def test_radius_255(capi):
    c = np.zeros((3, 600), np.uint8)
    c[1, 300] = 1
    rect = (40, -2, 520, 7)
    n = check(capi, c, 2, 255, rect, brute=False)
    assert at(n, rect, 300 - 254, 1) == (254, 0) and at(n, rect, 300 + 254, 1) == (-254, 0)
    assert at(n, rect, 300 - 255, 1) == (NONE, NONE) and at(n, rect, 300 + 255, 1) == (NONE, NONE)
    assert at(n, rect, 300 - 254, 2) == (254, -1) and at(n, rect, 300 - 254, 4) == (254, -3)      # 254^2 + 9 = 64525 < 65025
    ys, xs = np.mgrid[rect[1]:rect[1] + rect[3], rect[0]:rect[0] + rect[2]]
    near = (300 - xs) ** 2 + (1 - ys) ** 2 < 255 * 255
    assert np.array_equal(n[..., 0][near], (300 - xs)[near]) and np.array_equal(n[..., 1][near], (1 - ys)[near]) and (n[~near] == NONE).all()
    c = np.zeros((600, 3), np.uint8)                                       # ... and down a column
    c[300, 1] = 1
    rect = (-2, 40, 7, 520)
    n = check(capi, c, 2, 255, rect, brute=False)
    assert at(n, rect, 1, 300 - 254) == (0, 254) and at(n, rect, 1, 300 + 254) == (0, -254) and at(n, rect, 1, 300 + 255) == (NONE, NONE)


WORD_XS = (15, 16, 17, 31, 32, 33, 63, 64)


def test_word_boundaries(capi):
    """Sites and queried cells at the columns where a packed word (16 cells) or a site word (32 cells) ends."""
    for sx in WORD_XS:
        c = np.zeros((3, 70), np.uint8)
        c[1, sx] = 1
        rect = (-6, -5, 82, 13)
        n = check(capi, c, 2, 5, rect)
        for qx in WORD_XS:
            want = (sx - qx, 0) if abs(sx - qx) < 5 else (NONE, NONE)
            assert at(n, rect, qx, 1) == want, (sx, qx)
    c = np.zeros((3, 70), np.uint8)                                        # all of them at once, and their complement
    c[1, list(WORD_XS)] = 1
    check(capi, c, 2, 20, (-22, -21, 114, 45))
    check(capi, c, 1, 20, (-22, -21, 114, 45))


@pytest.mark.parametrize("w", [1, 15, 16, 17, 31, 32, 33, 65])
def test_map_widths(capi, w):
    rng = np.random.default_rng(100 + w)
    c = (rng.random((7, w)) < 0.2).astype(np.uint8)
    c[3, w - 1] = 1; c[5, 0] = 1
    for mask, r in ((2, 4), (3, 4), (1, 19), (2, 19)):
        check(capi, c, mask, r, (-r - 2, -r - 2, w + 2 * r + 4, 7 + 2 * r + 4))


@pytest.fixture(scope="module")
def random_maps():
    """40 x 37 class maps, one per (mask, per cent): that share of the cells are sites OF THE MASK -- a class the mask selects, drawn
    evenly -- and the others a class it does not select (mask 7 selects every class: all cells are sites whatever the share)."""
    rng = np.random.default_rng(16)
    out = {}
    for mask in range(1, 8):
        inside = np.array([k for k in range(3) if mask >> k & 1]); outside = np.array([k for k in range(3) if not mask >> k & 1])
        for pct in (0.5, 5, 50):
            site = rng.random((37, 40)) < pct / 100.0
            site[5, 7] = True; site[30, 33] = False
            c = np.where(site, rng.choice(inside, (37, 40)), rng.choice(outside if outside.size else inside, (37, 40))).astype(np.uint8)
            c.setflags(write=False)
            out[mask, pct] = c
    return out


@pytest.mark.parametrize("r", [1, 2, 3, 8, 32])
@pytest.mark.parametrize("pct", [0.5, 5, 50])
def test_random_maps_all_masks(capi, random_maps, pct, r):
    for mask in range(1, 8):
        c = random_maps[mask, pct]
        share = ((mask >> c.astype(np.int64)) & 1).mean()
        assert mask == 7 or 0.4 * pct / 100 < share < 2.5 * pct / 100, (mask, pct, share)
        n = check(capi, c, mask, r, (-r - 2, -r - 2, 40 + 2 * r + 4, 37 + 2 * r + 4))   # sticks out beyond E on all four sides
        const = 0 if mask & 1 else NONE
        assert (n[:2] == const).all() and (n[-2:] == const).all() and (n[:, :2] == const).all() and (n[:, -2:] == const).all()
        if mask == 7:
            assert not n.any()


def test_corners_and_edges_with_bit_0(capi):
    """With bit 0 the cells outside M are sites.  A non-site cell at M's corner has four of them at distance 1; the smaller row wins."""
    c = np.ones((6, 8), np.uint8)                                          # every cell of M occupied: no site of mask 1 inside
    for r in (2, 5):
        rect = (-r - 1, -r - 1, 8 + 2 * r + 2, 6 + 2 * r + 2)
        n = check(capi, c, 1, r, rect)
        assert at(n, rect, 0, 0) == (0, -1) and at(n, rect, 7, 0) == (0, -1)                # the top corners: up, not sideways
        assert at(n, rect, 0, 5) == (-1, 0) and at(n, rect, 7, 5) == (1, 0)                 # the bottom corners: the row of the cell beats the row below
        assert at(n, rect, 3, 0) == (0, -1) and at(n, rect, 3, 5) == (0, 1) and at(n, rect, 0, 2) == (-1, 0) and at(n, rect, 7, 3) == (1, 0)
        # two cells in: D2 = 4, out of reach for r = 2; else up beats left, and the cell's own row beats the row below
        assert at(n, rect, 1, 1) == ((0, -2) if r > 2 else (NONE, NONE)) and at(n, rect, 6, 4) == ((2, 0) if r > 2 else (NONE, NONE))
        assert at(n, rect, -1, 0) == (0, 0) and at(n, rect, 3, -1) == (0, 0) and at(n, rect, 8, 6) == (0, 0)
    for mask in (3, 5):                                                    # ... and with sites inside as well
        cc = c.copy()
        cc[2, 3] = 2; cc[0, 0] = 0
        check(capi, cc, mask, 4, (-6, -6, 20, 18))


def test_rectangles_outside_E(capi):
    c = np.ones((5, 7), np.uint8)
    for r in (1, 16, 255):
        for mask, const in ((2, NONE), (3, 0), (1, 0), (4, NONE), (6, NONE)):
            for rect in ((7 + r, 0, 4, 5), (-r - 4, 0, 4, 5), (0, 5 + r, 7, 3), (0, -r - 3, 7, 3), (1 << 30, -(1 << 30), 2, 2)):
                assert (capi.debug_nearest_field(c, mask, r, rect) == const).all(), (r, mask, rect)
        # partly outside: the last column of E is not constant for the obstacles
        edge = capi.debug_nearest_field(c, 2, r, (7 + r - 2, 0, 3, 1))[0].tolist()
        assert edge == [[-(r - 1), 0], [NONE, NONE], [NONE, NONE]], (r, edge)
    big = check(capi, c, 2, 6, (-10, -9, 27, 23))
    for sub in ((-10, 2, 8, 3), (5, -9, 6, 9), (6, 4, 11, 10), (-3, -3, 3, 3)):   # across one edge of E each, and a corner
        x, y, w, h = sub
        assert np.array_equal(capi.debug_nearest_field(c, 2, 6, sub), big[y + 9:y + 9 + h, x + 10:x + 10 + w]), sub


# ---- the separable restatement is the brute force ----------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [1, 2, 15, 16, 17, 40])
def test_separable_restatement_equals_brute_force(r):
    rng = np.random.default_rng(9)
    c = D.random_classes(rng, 21, 37)
    rect = (-r - 3, -r - 3, 37 + 2 * r + 6, 21 + 2 * r + 6)
    for mask in range(1, 8):
        assert np.array_equal(np_nearest(c, mask, r, rect), np_nearest_brute(c, mask, r, rect)), (mask, r)


# ---- the two hooks run one skeleton: their fields agree cell for cell ---------------------------------------------------------------
@pytest.mark.parametrize("r", [1, 16, 17, 40])
def test_hook_identity_with_the_distance_field(capi, r):
    """min(r^2, dx^2 + dy^2) of the nearest-site hook, NONE standing for r^2, is the distance field's hook: the identity the device
    test asserts, over a rectangle that reaches past E on all four sides, for every mask."""
    c = D.random_classes(np.random.default_rng(9), 21, 37)
    rect = (-r - 3, -r - 3, 37 + 2 * r + 6, 21 + 2 * r + 6)
    for mask in range(1, 8):
        d2, none = d2_of(capi.debug_nearest_field(c, mask, r, rect))
        want = capi.debug_distance_field(c, mask, r, rect).astype(np.int64)
        got = np.minimum(np.where(none, r * r, d2), r * r)
        assert np.array_equal(got, want), (mask, r, np.argwhere(got != want)[:5].tolist())


def test_pair_summary_restatement():
    pairs = np.array([(IGNORED, IGNORED), (NONE, NONE), (0, 0), (-3, 4), (2, -1)], np.int16)
    ex = np.array([0, 5, 7, -2, 1 << 24]); ey = np.array([0, 5, -7, 3, -(1 << 24)])
    s = np_pair_summary(pairs, ex, ey)
    assert (s["n_counted"], s["n_ignored"], s["n_matched"], s["n_zero"], s["sum_d2"]) == (4, 1, 3, 1, 30)
    assert s["sum_ex"] == 7 - 2 + (1 << 24) and s["sum_qx"] == 7 - 5 + (1 << 24) + 2 and s["sum_qy"] == -7 + 7 - (1 << 24) - 1
    assert s["sum_exqy"] == 7 * -7 + -2 * 7 + (1 << 24) * (-(1 << 24) - 1)


def test_align_step_arithmetic(capi):
    """align_step on hand-made summaries: a pure shift gives a rotation of exactly 0.0 and the shift; a quarter turn gives pi / 2."""
    import math
    import slam.net_amd.hector as hm
    e = np.array([(3, 4), (10, -2), (-7, 9), (20, 20), (1, 1)], np.int64)
    pr = np.tile(np.array([(-3, 0)], np.int16), (5, 1))
    s = np_pair_summary(pr, e[:, 0], e[:, 1])
    pose, dth, t = hm.align_step((1.5, -2.0, 0.3), s, 8.0)
    assert dth == 0.0 and t == (-3.0, 0.0) and pose.dtype == np.float32
    assert pose.tolist() == [np.float32(1.5 - 3 / 8.0), np.float32(-2.0), np.float32(0.3)]
    q = np.stack([-e[:, 1], e[:, 0]], 1)                                   # e turned by +90 degrees about the origin
    s = np_pair_summary((q - e).astype(np.int16), e[:, 0], e[:, 1])
    pose, dth, t = hm.align_step((0.0, 0.0, 0.0), s, 1.0)
    assert abs(dth - math.pi / 2) < 1e-15 and abs(t[0]) < 1e-12 and abs(t[1]) < 1e-12
    one = np_pair_summary(np.array([(2, 5)], np.int16), [4], [4])          # one matched point: a shift, no rotation
    assert hm.align_step((0.0, 0.0, 1.0), one, 2.0)[0].tolist() == [1.0, 2.5, 1.0]
    none = np_pair_summary(np.array([(NONE, NONE)], np.int16), [4], [4])   # none: the pose as it is
    assert hm.align_step((0.25, 0.5, 1.0), none, 2.0)[0].tolist() == [0.25, 0.5, 1.0]
