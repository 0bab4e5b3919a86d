"""CPU-side checks of the distance field's interface (slamhip_hs_distance_field, slamhip_hs_distance_score,
slamhip_hsproc_distance_score, slamhip_debug_distance_field) and the NumPy restatements of its definition (include/slamhip.h,
slamhip_hs_distance_field) that tests/test_gpu_hector_dfield.py compares the device with.

np_field_brute is the yardstick: for every cell the minimum over ALL shifts in [-r, r]^2 of a padded site array -- the definition
word for word.  np_field is a separable restatement (nearest site of a row by running maxima, then a minimum over 2 r + 1 row
shifts) for the larger cases of the GPU file; it is proved equal to the brute force here, on the small arrays, before anything
relies on it.  The library's hook runs a third formulation (site bits by word, ctz / clz, an early-exit column walk).  Everything
is compared with == on integers.  No compute calls on a device."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("slamhip_hs_distance_field", "slamhip_hs_distance_score", "slamhip_hsproc_distance_score", "slamhip_debug_distance_field")
SUMMARY = np.dtype([("n_counted", np.int32), ("n_ignored", np.int32), ("n_zero", np.int32), ("n_capped", np.int32), ("sum_d2", np.int64)])
BIG = np.int64(1) << 40


# ---- the restatements --------------------------------------------------------------------------------------------------------------
def np_sites(cls, site_mask, rect, r):
    """The site array of the cells of rect = (x, y, w, h) grown by r on every side: cls is the (H, W) array of class bits whose first
    element is cell (0, 0); every cell outside it is class 0.  A cell is a site iff bit cls of site_mask is set."""
    cls = np.asarray(cls).astype(np.int64)
    H, W = cls.shape
    x, y, w, h = rect
    full = np.zeros((h + 2 * r, w + 2 * r), np.int64)                      # class 0
    gx0, gy0 = x - r, y - r                                                # the grown rectangle's first cell
    sx0, sx1 = max(gx0, 0), min(gx0 + w + 2 * r, W)
    sy0, sy1 = max(gy0, 0), min(gy0 + h + 2 * r, H)
    if sx0 < sx1 and sy0 < sy1:
        full[sy0 - gy0:sy1 - gy0, sx0 - gx0:sx1 - gx0] = cls[sy0:sy1, sx0:sx1]
    return ((int(site_mask) >> full) & 1).astype(bool)


def np_field_brute(cls, site_mask, r, rect):
    """F of every cell of rect: min over all (dx, dy) in [-r, r]^2 with a site at (x + dx, y + dy) of dx^2 + dy^2, capped at r^2."""
    x, y, w, h = rect
    s = np_sites(cls, site_mask, rect, r)
    best = np.full((h, w), r * r, np.int64)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            d = dx * dx + dy * dy
            if d < r * r:
                np.minimum(best, np.where(s[r + dy:r + dy + h, r + dx:r + dx + w], d, BIG), out=best)
    return best.astype(np.uint16)


def np_field(cls, site_mask, r, rect):
    """The same field, separably: the distance to the nearest site of the row (from the left by a running maximum of site positions,
    from the right by a running minimum), capped at r + 1; then the minimum over row shifts of g^2 + dy^2."""
    x, y, w, h = rect
    s = np_sites(cls, site_mask, rect, r)                                  # (h + 2 r, w + 2 r)
    n = s.shape[1]
    idx = np.arange(n, dtype=np.int64)[None, :]
    left = np.maximum.accumulate(np.where(s, idx, -BIG), axis=1)           # the last site at or left of the cell
    right = np.minimum.accumulate(np.where(s, idx, BIG)[:, ::-1], axis=1)[:, ::-1]
    g = np.minimum(np.minimum(idx - left, right - idx), r + 1)[:, r:r + w]   # (sites more than r away play no part)
    g2 = g * g
    best = np.full((h, w), r * r, np.int64)
    for dy in range(-r, r + 1):
        np.minimum(best, g2[r + dy:r + dy + h] + dy * dy, out=best)
    return best.astype(np.uint16)


def np_closed_form(sites, r, rect):
    """The field of a few lone sites [(a, b), ...]: min over them of (x - a)^2 + (y - b)^2, capped at r^2."""
    x, y, w, h = rect
    xs = np.arange(x, x + w, dtype=np.int64)[None, :]; ys = np.arange(y, y + h, dtype=np.int64)[:, None]
    best = np.full((h, w), r * r, np.int64)
    for a, b in sites:
        np.minimum(best, (xs - a) ** 2 + (ys - b) ** 2, out=best)
    return best.astype(np.uint16)


def np_class_bits(values):
    v = np.asarray(values, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(v > 0, 1, np.where(v < 0, 2, 0)).astype(np.uint8)


def np_summary(f_points, r):
    """slamhip_distance_summary of one pose's per-point values (0xFFFF: ignored)."""
    f = np.asarray(f_points).astype(np.int64)
    ok = f != 0xFFFF
    s = np.zeros(1, SUMMARY)[0]
    s["n_counted"] = ok.sum(); s["n_ignored"] = (~ok).sum()
    s["n_zero"] = (ok & (f == 0)).sum(); s["n_capped"] = (ok & (f == r * r)).sum()
    s["sum_d2"] = f[ok].sum()
    return s


def random_classes(rng, h, w):
    """Every class, in patches: runs of unknown wide enough that a radius of 15 .. 17 finds nothing in places."""
    c = rng.integers(0, 3, (h, w)).astype(np.uint8)
    c[rng.random((h, w)) < 0.55] = 0
    c[h // 4:h // 4 + 9, w // 5:w // 5 + 24] = 2                           # a free patch without obstacles
    c[h // 2:h // 2 + 7, w // 2:w // 2 + 12] = 0                           # an unknown patch
    return c


# ---- the interface -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def capi():
    import slam.net_amd.build as b
    b.build()
    import slam.net_amd.capi as capi
    return capi


def test_surface(capi):
    h = open(os.path.join(ROOT, "include", "slamhip.h")).read()
    native = open(os.path.join(ROOT, "bindings", "csharp", "SlamHip", "SlamHip.Native.cs")).read()
    assert capi.DISTANCE_SUMMARY == SUMMARY and capi.DISTANCE_SUMMARY.itemsize == 24
    assert [capi.DISTANCE_SUMMARY.fields[n][1] for n in SUMMARY.names] == [0, 4, 8, 12, 16]     # 4 int32 + 1 int64: no padding
    assert "SLAMHIP_K_COUNT = 10" in h                                       # no new timing class
    L = capi.lib()
    for name in SYMBOLS:
        assert hasattr(L, name) and name in L._signatures and name in capi.declared_symbols() and name in native, name
    assert "struct DistanceSummary" in native
    assert len(L._signatures["slamhip_hs_distance_field"][1]) == 10 and len(L._signatures["slamhip_hs_distance_score"][1]) == 9
    assert len(L._signatures["slamhip_hsproc_distance_score"][1]) == 12 and len(L._signatures["slamhip_debug_distance_field"][1]) == 10
    import slam.net_amd.hector as hm
    assert hasattr(hm.MapRepMultiMap, "distance_field") and hasattr(hm.MapRepMultiMap, "distance_score")
    assert hasattr(hm.HectorSLAMProcessor, "DistanceScore")


def test_hook_refuses(capi):
    L = capi.lib()
    cls = np.zeros((4, 6), np.uint8)
    out = np.full((3, 3), 77, np.uint16)

    def rc(mask, r, w, h):
        return L.slamhip_debug_distance_field(cls.ctypes.data_as(C.c_void_p), 6, 4, mask, r, 0, 0, w, h, out.ctypes.data_as(C.c_void_p))
    for mask, r, w, h in ((0, 3, 3, 3), (8, 3, 3, 3), (2, 0, 3, 3), (2, 256, 3, 3), (2, 3, 0, 3), (2, 3, 3, 0), (2, 3, 4097, 4096)):
        assert rc(mask, r, w, h) == capi.ERR_INVALID, (mask, r, w, h)
    assert (out == 77).all()
    assert rc(2, 3, 3, 3) == 0 and (out == 9).all()


# ---- the separable restatement is the brute force ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def arrays():
    rng = np.random.default_rng(9)
    return {"37x21": random_classes(rng, 21, 37), "80x48": random_classes(rng, 48, 80)}


RADII = (1, 2, 15, 16, 17, 40)
_brute = {}


def brute(arrays, name, mask, r):
    """np_field_brute over E plus a margin of 3 cells: computed once per case and shared."""
    key = (name, mask, r)
    if key not in _brute:
        c = arrays[name]
        rect = (-r - 3, -r - 3, c.shape[1] + 2 * r + 6, c.shape[0] + 2 * r + 6)
        _brute[key] = (rect, np_field_brute(c, mask, r, rect))
        _brute[key][1].setflags(write=False)
    return _brute[key]


@pytest.mark.parametrize("name", ["37x21", "80x48"])
@pytest.mark.parametrize("r", RADII)
def test_separable_restatement_equals_brute_force(arrays, name, r):
    for mask in range(1, 8):
        rect, want = brute(arrays, name, mask, r)
        assert np.array_equal(np_field(arrays[name], mask, r, rect), want), (name, mask, r)


# ---- the hook against the brute force ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["37x21", "80x48"])
@pytest.mark.parametrize("r", RADII)
def test_hook_equals_brute_force(capi, arrays, name, r):
    c = arrays[name]
    H, W = c.shape
    for mask in range(1, 8):
        rect, want = brute(arrays, name, mask, r)                          # sticks out beyond E on all four sides
        got = capi.debug_distance_field(c, mask, r, rect)
        assert got.dtype == np.uint16 and np.array_equal(got, want), (name, mask, r, np.argwhere(got != want)[:5].tolist())
        const = 0 if mask & 1 else r * r
        assert (got[:3] == const).all() and (got[-3:] == const).all() and (got[:, :3] == const).all() and (got[:, -3:] == const).all()
        if mask == 7:
            assert not got.any()
        # sub-rectangles: inside the map, across one edge of E, and wholly outside E
        for sub in ((5, 3, 20, 11), (-r - 2, 4, r + 9, 6), (W - 4, H - 2, r + 6, r + 4), (W + r, -r - 3, 3, 3), (-1000, 2000, 3, 2)):
            g = capi.debug_distance_field(c, mask, r, sub)
            x, y, w, h = sub
            if x == -1000 or x == W + r:
                assert (g == const).all(), (mask, r, sub)
            if x != -1000:
                ox, oy = x - rect[0], y - rect[1]
                assert np.array_equal(g, want[oy:oy + h, ox:ox + w]), (name, mask, r, sub)


def test_classes_present(arrays):
    for c in arrays.values():
        assert set(np.unique(c).tolist()) == {0, 1, 2}
    # a radius of 15 leaves capped cells inside the free patch for mask 2 | 1 = 3 and the radii differ there
    rect, f15 = brute(arrays, "80x48", 2, 15)
    _, f17 = brute(arrays, "80x48", 2, 17)
    assert (f15 == 225).any() and (f17 == 289).any()


def test_single_site_closed_form(capi):
    """One occupied cell at (a, b) of a 600 x 300 array, r = 255: min((x - a)^2 + (y - b)^2, r^2) over E and beyond."""
    c = np.zeros((300, 600), np.uint8)
    a, b = 417, 93
    c[b, a] = 1
    r = 255
    rect = (-r - 2, -r - 2, 600 + 2 * r + 4, 300 + 2 * r + 4)
    want = np_closed_form([(a, b)], r, rect)
    got = capi.debug_distance_field(c, 2, r, rect)
    assert np.array_equal(got, want)
    assert got[b - rect[1], a - rect[0]] == 0 and got[b - rect[1], a - 255 - rect[0]] == 65025 and got[b - rect[1], a - 254 - rect[0]] == 64516
    assert np.array_equal(np_field(c, 2, r, rect), want)                   # ... and the separable restatement at the largest radius
    # the free cells' field: nothing is free, so it is capped everywhere; the unknown's field is 0 but at the site
    assert (capi.debug_distance_field(c, 4, r, (0, 0, 600, 300)) == 65025).all()
    unk = capi.debug_distance_field(c, 1, r, (a - 2, b - 2, 5, 5))
    assert unk[2, 2] == 1 and unk.sum() == 1


def test_constant_outside_E(capi):
    c = np.ones((5, 7), np.uint8)                                           # every cell occupied
    for r in (1, 16, 255):
        for mask, const in ((2, r * r), (3, 0), (1, 0), (4, r * r), (6, r * r)):
            for rect in ((7 + r, 0, 4, 5), (-r - 4, 0, 4, 5), (0, 5 + r, 7, 3), (0, -r - 3, 7, 3), (1 << 30, -(1 << 30), 2, 2)):
                assert (capi.debug_distance_field(c, mask, r, rect) == const).all(), (r, mask, rect)
        # ... and the last column of E is not constant for the obstacles: r cells from the map's edge is still closer than the cap
        edge = capi.debug_distance_field(c, 2, r, (7 + r - 2, 0, 3, 1))[0].tolist()
        assert edge == [(r - 1) ** 2, r * r, r * r] and (r - 1) ** 2 < r * r
