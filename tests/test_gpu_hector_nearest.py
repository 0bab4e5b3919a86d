"""The nearest-site field and the scan-to-map pairs (slamhip_hs_nearest_field, slamhip_hs_nearest_pairs,
slamhip_hsproc_nearest_pairs) on the device, against the host hook and the NumPy restatements of the definition in
tests/test_hs_nearest_abi.py (np_nearest, proved equal to the brute force there), fed from cells_download / world_cells_download.
Everything is compared with == on integers; there is no tolerance anywhere.

Shapes are the smallest at which each path can go wrong: maps whose E is one below, at and one above a k16_cols tile (64 x 128) and a
k16_rows segment (512 cells), point counts on both sides of the 256-point chunk of k16_pairs, one radius of 255 on a 200 x 20 map.
(A map is at least 2 cells wide: the width-1 case of the CPU file runs on the host hook alone.)"""
import ctypes as C
import math

import numpy as np
import pytest

import test_gpu_hector_dfield as G
import test_gpu_hector_lattice as L
import test_gpu_hector_shift as S
import test_gpu_hector_trace as TR
import test_hs_dfield_abi as D
import test_hs_nearest_abi as N
from test_gpu_hector_shift import hs_mod, ctx                              # noqa: F401 (fixtures)

gpu = pytest.mark.gpu
F = np.float32
POOL = 64 << 20
NONE, IGNORED = N.NONE, N.IGNORED
# the kernels' tile constants (hs_nearest.hip)
SEG = 512                                                                  # K16_SEG: cells of one row a k16_rows workgroup owns
TX, TY = 64, 128                                                           # K16_TX, K16_TY: columns x rows of a k16_cols tile
CHUNK = 256                                                                # K16P_LANES: points per k16_pairs workgroup


def rep_of(hs_mod, ctx, cls, levels=1):
    """A pyramid whose level 0 has the classes of `cls`."""
    h, w = cls.shape
    rep = hs_mod.MapRepMultiMap(0.1, (w, h), levels, ctx=ctx)
    L.put_values(hs_mod, rep, 0, np.select([cls == 1, cls == 2], [F(1.5), F(-0.7)], F(0.0)).astype(np.float32).ravel())
    return rep


def device_equals(hs_mod, rep, cls, mask, r, rect, level=0):
    """The device's N over rect == the hook == np_nearest, and == the device's own distance field by the identity."""
    got = rep.nearest_field(level, rect, site_mask=mask, radius=r)
    assert got.dtype == np.int16 and got.shape == (rect[3], rect[2], 2)
    hook = hs_mod.capi.debug_nearest_field(cls, mask, r, rect)
    assert np.array_equal(got, hook), (mask, r, rect, np.argwhere(got != hook)[:5].tolist())
    want = N.np_nearest(cls, mask, r, rect)
    assert np.array_equal(got, want), (mask, r, rect, np.argwhere(got != want)[:5].tolist())
    f = rep.distance_field(level, rect, site_mask=mask, radius=r).astype(np.int64)
    d2, none = N.d2_of(got)
    assert np.array_equal(none, f == r * r) and np.array_equal(d2[~none], f[~none]), (mask, r, rect)
    return got


# ---- 1. the CPU file's cases ---------------------------------------------------------------------------------------------------------
def named_cases():
    out = []
    c, mask, r, rect = N.tie_lr()
    out.append(("left/right tie", c, mask, r, rect, {(5, 2): (-3, 0)}))
    c = np.zeros((11, 5), np.uint8); c[2, 2] = c[8, 2] = 1
    out.append(("up/down tie", c, 2, 6, (-8, -8, 21, 27), {(2, 5): (0, -3)}))
    c = np.zeros((15, 15), np.uint8)
    for dx, dy in [(sx * a, sy * b) for a, b in ((3, 4), (4, 3)) for sx in (-1, 1) for sy in (-1, 1)] + [(5, 0), (-5, 0), (0, 5), (0, -5)]:
        c[7 + dy, 7 + dx] = 1
    out.append(("twelve at 25", c, 2, 6, (-6, -6, 27, 27), {(7, 7): (0, -5)}))
    c, mask, r, rect = N.axis_r()
    out.append(("axis distance r", c, mask, r, rect, {(20 - r, 1): (NONE, NONE), (20 - r + 1, 1): (r - 1, 0), (20, 1 + r): (NONE, NONE)}))
    c = np.zeros((21, 23), np.uint8); c[9, 12] = 1
    out.append(("lone site", c, 2, 7, (-9, -9, 41, 39), {(12, 9): (0, 0), (10, 13): (2, -4)}))
    out.append(("radius 1", c, 2, 1, (-3, -3, 29, 27), {(12, 9): (0, 0), (11, 9): (NONE, NONE)}))
    c = np.ones((6, 8), np.uint8)
    out.append(("corners with bit 0", c, 1, 5, (-6, -6, 20, 18), {(0, 0): (0, -1), (7, 0): (0, -1), (0, 5): (-1, 0), (7, 5): (1, 0), (-1, 0): (0, 0)}))
    c = np.zeros((3, 70), np.uint8); c[1, list(N.WORD_XS)] = 1
    out.append(("word boundaries", c, 2, 20, (-22, -21, 114, 45), {(x, 1): (0, 0) for x in N.WORD_XS}))
    out.append(("word boundaries, unknown", c, 1, 20, (-22, -21, 114, 45), {(x, 1): (0, -1) for x in N.WORD_XS}))
    return out


@gpu
def test_named_cases(hs_mod, ctx):
    for name, c, mask, r, rect, probes in named_cases():
        rep = rep_of(hs_mod, ctx, c)
        got = device_equals(hs_mod, rep, c, mask, r, rect)
        for (x, y), want in probes.items():
            assert N.at(got, rect, x, y) == want, (name, (x, y))
        rep.close()


@gpu
@pytest.mark.parametrize("w", [15, 16, 17, 31, 32, 33, 65])
def test_map_widths(hs_mod, ctx, w):
    rng = np.random.default_rng(100 + w)
    c = (rng.random((7, w)) < 0.2).astype(np.uint8)
    c[3, w - 1] = 1; c[5, 0] = 1
    rep = rep_of(hs_mod, ctx, c)
    for mask, r in ((2, 4), (3, 4), (1, 19), (2, 19)):
        device_equals(hs_mod, rep, c, mask, r, (-r - 2, -r - 2, w + 2 * r + 4, 7 + 2 * r + 4))
    rep.close()


@gpu
@pytest.mark.parametrize("pct", [0.5, 5, 50])
def test_random_maps_all_masks(hs_mod, ctx, pct):
    rng = np.random.default_rng(16)
    c = rng.integers(0, 3, (37, 40)).astype(np.uint8)
    keep = rng.random((37, 40)) < pct / 100.0
    rep = None
    for mask in range(1, 8):
        inside = [k for k in range(3) if mask >> k & 1]; outside = [k for k in range(3) if not mask >> k & 1] or inside
        cm = np.where(keep, rng.choice(inside, c.shape), rng.choice(outside, c.shape)).astype(np.uint8)
        if rep is not None:
            rep.close()
        rep = rep_of(hs_mod, ctx, cm)
        for r in (1, 2, 3, 8, 32):
            got = device_equals(hs_mod, rep, cm, mask, r, (-r - 2, -r - 2, 40 + 2 * r + 4, 37 + 2 * r + 4))
            const = 0 if mask & 1 else NONE
            assert (got[:2] == const).all() and (got[:, -2:] == const).all()
        for sub in ((44 + 32, 0, 4, 5), (-40, 0, 4, 5), (1 << 30, -(1 << 30), 2, 2), (30, 30, 20, 20)):   # wholly and partly outside E
            g = rep.nearest_field(0, sub, site_mask=mask, radius=32)
            assert np.array_equal(g, hs_mod.capi.debug_nearest_field(cm, mask, 32, sub)), (mask, sub)
            if sub[0] != 30:
                assert (g == (0 if mask & 1 else NONE)).all()
    rep.close()


# ---- 2. tile seams -------------------------------------------------------------------------------------------------------------------
SEAM_R = 3


@gpu
@pytest.mark.parametrize("ew,eh", [(TX - 1, TY - 1), (TX, TY), (TX + 1, TY + 1), (SEG - 1, 8), (SEG, 8), (SEG + 1, 8), (2 * TX + 1, 2 * TY + 1)])
def test_tile_dimensions(hs_mod, ctx, ew, eh):
    """E one below, at and one above a k16_cols tile in both axes and a k16_rows segment, with sites in M's last and first columns and
    rows, beside every tile boundary, and scattered."""
    r = SEAM_R
    w, h = ew - 2 * r, eh - 2 * r
    rng = np.random.default_rng(ew * 1000 + eh)
    c = (rng.random((h, w)) < 0.01).astype(np.uint8)
    c[0, 0] = c[h - 1, w - 1] = c[0, w - 1] = c[h - 1, 0] = 1
    for bx in range(TX - r, w, TX):                                        # E column k * TX = map column k * TX - r
        c[h // 2, bx - 1] = 1
        c[1, min(bx, w - 1)] = 1
    for by in range(TY - r, h, TY):
        c[by - 1, w // 2] = 1
        c[min(by, h - 1), 1] = 1
    rep = rep_of(hs_mod, ctx, c)
    for mask in (2, 1):
        device_equals(hs_mod, rep, c, mask, r, (-r - 2, -r - 2, ew + 4, eh + 4))
    device_equals(hs_mod, rep, c, 2, 40, (-42, -42, w + 84, h + 84))       # ... and a radius that reaches across tiles
    rep.close()


@gpu
def test_radius_255(hs_mod, ctx):
    c = np.zeros((20, 200), np.uint8)
    c[3, 7] = c[17, 190] = c[10, 100] = 1
    rep = rep_of(hs_mod, ctx, c)
    rect = (-257, -257, 200 + 514, 20 + 514)                               # E is 710 x 530: 12 x 5 tiles, two segments
    got = device_equals(hs_mod, rep, c, 2, 255, rect)
    assert N.at(got, rect, 7 - 254, 3) == (254, 0) and N.at(got, rect, 7 - 255, 3) == (NONE, NONE) and N.at(got, rect, 190, 17 + 254) == (0, -254)
    assert N.at(got, rect, 190 + 254, 17) == (-254, 0) and N.at(got, rect, 7, 3 - 254) == (0, 254) and N.at(got, rect, 7, 3 - 255) == (NONE, NONE)
    rep.close()


# ---- 3. the world, and a shifted window ----------------------------------------------------------------------------------------------
@gpu
def test_world_variant(hs_mod, ctx):
    level = 1
    rng = np.random.default_rng(7)
    rep = hs_mod.MapRepMultiMap(0.1, (80, 48), 2, ctx=ctx)
    rep.set_backing(16, POOL)
    TR.fill(hs_mod, rep, rng)
    rep.shift(34, -22)
    TR.fill(hs_mod, rep, rng)
    rep.shift(-68, 30)                                                     # part of what was mapped now lies in tiles alone
    assert rep.origin() == (-34, 8) and rep.backing_stats()["tiles"] > 3
    x0, y0, w, h = TR.WORLD_RECTS[level]
    values, ax0, ay0 = TR.world_values(rep, level, TR.WORLD_RECTS[level])
    cls = D.np_class_bits(values)
    for mask, r in ((2, 5), (3, 20), (4, 33)):
        rel = G.grown(w, h, r, 3)                                          # in the source array's cells: the world's E lies inside
        rect = (rel[0] + ax0, rel[1] + ay0, rel[2], rel[3])
        want = N.np_nearest(cls, mask, r, rel)
        got = rep.nearest_field(level, rect, site_mask=mask, radius=r, world=True)
        assert np.array_equal(got, want), (mask, r, np.argwhere(got != want)[:5].tolist())
        assert np.array_equal(got, hs_mod.capi.debug_nearest_field(cls, mask, r, rel))
        win = rep.nearest_field(level, rect, site_mask=mask, radius=r)
        assert np.array_equal(win, N.np_nearest(G.window_classes(rep, level), mask, r, rect))
        assert not np.array_equal(win, got)                                # the tiles outside the window count in the world alone
    rep.close()


@gpu
def test_after_a_shift(hs_mod, ctx):
    rng = np.random.default_rng(5)
    rep = hs_mod.MapRepMultiMap(0.1, (80, 48), 2, ctx=ctx)
    TR.fill(hs_mod, rep, rng)
    before = rep.nearest_field(0, (0, 0, 80, 48), site_mask=2, radius=9)
    rep.shift(6, -4)
    for level in (0, 1):
        cls = G.window_classes(rep, level)
        h, w = cls.shape
        got = device_equals(hs_mod, rep, cls, 2, 9, G.grown(w, h, 9), level=level)
        if level == 0:                                                     # what stayed in the window kept its nearest site where that stayed too
            assert not np.array_equal(got[11:11 + 48, 11:11 + 80], before)
    rep.close()


# ---- 4. the device's two fields agree ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(hs_mod, ctx):
    """80 x 48 cells of 0.1 m, 2 levels, every class of value on both levels; the classes as cells_download gives them."""
    rng = np.random.default_rng(7)
    rep = hs_mod.MapRepMultiMap(0.1, (80, 48), 2, ctx=ctx)
    for l, n in enumerate((80 * 48, 40 * 24)):
        L.put_values(hs_mod, rep, l, L.class_values(rng, n))
    cls = [G.window_classes(rep, l) for l in range(2)]
    for c in cls:
        c.setflags(write=False)
    yield rep, cls
    rep.close()


@gpu
@pytest.mark.parametrize("mask,r", [(2, 1), (2, 16), (3, 17), (4, 40), (1, 255), (6, 9)])
def test_identity_with_the_distance_field(hs_mod, small, mask, r):
    rep, cls = small
    for level in (0, 1):
        h, w = cls[level].shape
        rect = G.grown(w, h, r)
        n = rep.nearest_field(level, rect, site_mask=mask, radius=r)
        f = rep.distance_field(level, rect, site_mask=mask, radius=r).astype(np.int64)
        d2, none = N.d2_of(n)
        assert np.array_equal(none, f == r * r) and np.array_equal(d2[~none], f[~none]) and (~none).any()
        assert np.array_equal(n, rep.nearest_field(level, rect, site_mask=mask, radius=r, world=True))   # no backing: the world is the window
        if r <= 40:
            assert np.array_equal(n, hs_mod.capi.debug_nearest_field(cls[level], mask, r, rect))


# ---- 5. pairs --------------------------------------------------------------------------------------------------------------------------
PAIR_R = 12


@pytest.fixture(scope="module")
def small_fields(small):
    """N over E and a margin, per mask and level: what the pairs' look-ups are compared with (itself checked against np_nearest)."""
    rep, cls = small
    out = {}
    for mask in (2, 3):
        for level in (0, 1):
            h, w = cls[level].shape
            rect = G.grown(w, h, PAIR_R)
            n = rep.nearest_field(level, rect, site_mask=mask, radius=PAIR_R)
            assert np.array_equal(n, N.np_nearest(cls[level], mask, PAIR_R, rect))
            n.setflags(write=False)
            out[mask, level] = (rect, n)
    return out


def pair_poses(B):
    rng = np.random.default_rng(B)
    p = np.stack([rng.uniform(0.5, 7.5, B), rng.uniform(0.5, 4.5, B), rng.uniform(-3.0, 3.0, B)], 1).astype(np.float32)
    p[0] = (3.1, 2.2, 0.4)
    if B >= 3:
        p[2] = (np.nan, 4.5, -1.0)                                         # a NaN pose: every point ignored
    if B > 3:
        p[5] = (7.7, np.inf, 2.0); p[B - 1] = (1.0e5, -1.0e5, 1.0)         # ... an infinite one, and one that puts every point far outside E
    return p


@gpu
@pytest.mark.parametrize("n_points", [1, 64, 65, CHUNK + 1])
@pytest.mark.parametrize("B", [1, 3, 257])
def test_pairs(hs_mod, small, small_fields, n_points, B):
    rep, _ = small
    rng = np.random.default_rng(200 + n_points)
    xy = np.stack([rng.uniform(-6.0, 6.0, n_points), rng.uniform(-4.0, 4.0, n_points)], 1).astype(np.float32)
    if n_points > 60:
        xy[3] = (np.nan, 1.0)                                              # ignored on every level
        xy[5] = (4000.0, 0.0)                                              # 40000 cells of level 0: counted, far outside E -- the constant
        xy[7] = (1.6e6, 1.0)                                               # 1.6e7 cells of level 0, below 2^24: counted; 8e6 of level 1
        xy[9] = (2.0e6, 1.0)                                               # 2e7 cells of level 0 (>= 2^24: ignored), 1e7 of level 1 (counted)
        xy[-1] = (-4000.0, 2.0e6)
    poses = pair_poses(B)
    scan = hs_mod.ScanCloud(xy)
    for mask in (2, 3):
        for level in (0, 1):
            rect, field = small_fields[mask, level]
            stm = TR.stm_of(rep, level)
            sums, prs = rep.nearest_pairs(poses, level, site_mask=mask, radius=PAIR_R, pairs=True, scan=scan)
            assert prs.shape == (B, n_points, 2) and prs.dtype == np.int16 and sums.shape == (B,) and sums.dtype == N.SUMMARY
            for b in range(B):
                ex, ey, ok = G.np_end_cells(stm, poses[b], xy)
                want = N.np_pairs(field, rect, mask, ex, ey, ok)
                assert np.array_equal(prs[b], want), (n_points, b, mask, level, np.flatnonzero((prs[b] != want).any(1))[:6].tolist())
                assert sums[b] == N.np_pair_summary(want, ex, ey), (n_points, b, mask, level, sums[b])
            assert (sums["n_counted"] + sums["n_ignored"] == n_points).all() and (sums["n_zero"] <= sums["n_matched"]).all()
            assert (sums["n_matched"] <= sums["n_counted"]).all()
            sums2, none = rep.nearest_pairs(poses, level, site_mask=mask, radius=PAIR_R)   # without the records
            assert none is None and np.array_equal(sums2, sums)
            if n_points > 60:
                assert sums[0]["n_ignored"] == (3 if level == 0 else 1) and sums[0]["n_matched"] > 0
                assert tuple(prs[0, 3]) == (IGNORED, IGNORED) and tuple(prs[0, 5]) == ((0, 0) if mask & 1 else (NONE, NONE))
                assert (tuple(prs[0, 9]) == (IGNORED, IGNORED)) == (level == 0)
                if mask == 3:                                              # a far point is its own site: its cell enters the sums, ~1.6e7 squared
                    assert tuple(prs[0, 7]) == (0, 0) and sums[0]["sum_exqx"] > (1 << 45)
            if B >= 3:
                assert sums[2]["n_ignored"] == n_points and sums[2]["n_matched"] == 0 and (prs[2] == IGNORED).all()
                assert not any(sums[2][k] for k in N.SUMMARY.names[4:])


# ---- 6. the alignment step -------------------------------------------------------------------------------------------------------------
K = 3
SITES = [(x, y) for y in range(12, 52, 2 * K + 3) for x in range(10, 50, 2 * K + 3)]   # 9 apart: more than 2 K + 1


def site_processor(hs_mod, own):
    proc = hs_mod.HectorSLAMProcessor(0.1, (64, 64), (0.0, 0.0, 0.0), 3, ctx=own)
    v = np.zeros((64, 64), np.float32)
    for x, y in SITES:
        v[y, x] = 1.0
    L.put_values(hs_mod, proc.MapRep, 0, v.ravel())
    return proc


@gpu
@pytest.mark.parametrize("moved", [False, True])
def test_align_step_on_isolated_sites(hs_mod, moved):
    own = hs_mod.Context(0)
    proc = site_processor(hs_mod, own)
    if moved:
        proc.shift(8, -8)                                                  # the window's frame is no longer the world's
        assert proc.get_origin() == (8, -8)
    sites = np.array(SITES, np.float64)
    scan = hs_mod.ScanCloud(((sites + (K, 0)) * 0.1).astype(np.float32))   # end cells at pose 0: the sites shifted by (K, 0)
    pose0 = np.zeros(3, np.float32)
    sums, prs = proc.NearestPairs(scan, pose0[None], 0, site_mask=2, radius=8, pairs=True)
    assert sums[0]["n_counted"] == sums[0]["n_matched"] == len(SITES) >= 16 and sums[0]["n_zero"] == 0
    assert (prs[0] == (-K, 0)).all() and sums[0]["sum_d2"] == K * K * len(SITES)
    pose1, s1 = proc.AlignStep(scan, pose0, 0, site_mask=2, radius=8)
    assert s1 == sums[0]
    assert pose1.dtype == np.float32 and pose1[2] == 0.0 and not np.signbit(pose1[2])           # the rotation is exactly 0.0
    assert abs(float(pose1[0]) + K * 0.1) < 1e-6 and abs(float(pose1[1])) < 1e-6
    after, _ = proc.NearestPairs(scan, pose1[None], 0, site_mask=2, radius=8)
    assert after[0]["n_zero"] == after[0]["n_matched"] == after[0]["n_counted"] == len(SITES) and after[0]["sum_d2"] == 0
    pose2, s2 = proc.AlignStep(scan, pose1, 0, site_mask=2, radius=8)      # the identity case: end cells on sites give a zero step
    assert s2 == after[0] and S.same_bits(pose2, pose1)
    proc.Dispose(); own.close()


@gpu
def test_align_step_through_the_pyramid_object(hs_mod, ctx):
    """MapRepMultiMap.nearest_pairs + align_step in the window's frame, at a pose that is not the origin."""
    c = np.zeros((64, 64), np.uint8)
    for x, y in SITES:
        c[y, x] = 1
    rep = rep_of(hs_mod, ctx, c)
    sites = np.array(SITES, np.float64)
    pose = np.array([0.5, -0.25, 0.0], np.float32)
    scan = hs_mod.ScanCloud(((sites + (K, 0)) * 0.1 - (0.5, -0.25)).astype(np.float32))
    sums, prs = rep.nearest_pairs(pose[None], 0, site_mask=2, radius=8, pairs=True, scan=scan)
    assert (prs[0] == (-K, 0)).all()
    stepped, dth, t = rep.align_step(pose, 0, sums[0])
    assert dth == 0.0 and t == (-float(K), 0.0) and stepped[2] == 0.0
    again, _ = rep.nearest_pairs(stepped[None], 0, site_mask=2, radius=8)
    assert again[0]["n_zero"] == again[0]["n_matched"] == again[0]["n_counted"] == len(SITES)
    assert S.same_bits(rep.align_step(stepped, 0, again[0])[0], stepped)
    rep.close()


# ---- 7. no side effects, refusals ------------------------------------------------------------------------------------------------------
@gpu
def test_update_is_bit_equal_around_a_call(hs_mod, sim):
    """Two processors fed the same scans; one of them asks for pairs, a field and a step between its Updates.  Poses and maps agree
    bit for bit: the calls read cell values only."""
    own = hs_mod.Context(0)
    procs = [hs_mod.HectorSLAMProcessor(0.1, (64, 64), (3.0, 3.0, 0.0), 3, ctx=own) for _ in range(2)]
    for i in range(6):
        true = np.array([3.0 + 0.18 * i, 3.0 + 0.05 * i, 0.04 * i], np.float32)
        scan = hs_mod.ScanCloud(TR.room_scan(sim, true, 120))
        for k, p in enumerate(procs):
            p.Update(scan, true)
            if k == 1:
                p.NearestPairs(scan, true[None], i % 3, site_mask=2, radius=10, pairs=True)
                p.MapRep.nearest_field(i % 3, (-5, -5, 40, 40), site_mask=3, radius=7)
                p.AlignStep(scan, true, 0, radius=6)
        assert S.same_bits(procs[0].MatchPose, procs[1].MatchPose) and S.same_bits(procs[0].LastMapUpdatePose, procs[1].LastMapUpdatePose)
    for l in range(3):
        assert procs[0].MapRep.Maps[l].checksum() == procs[1].MapRep.Maps[l].checksum()
    s, _ = procs[1].NearestPairs(scan, true[None], 0, radius=10)
    assert s[0]["n_matched"] > 60                                          # ... and the calls had something to say
    for p in procs:
        p.Dispose()
    own.close()


@gpu
def test_processor_pairs_after_a_scroll(hs_mod, sim):
    own = hs_mod.Context(0)
    proc = hs_mod.HectorSLAMProcessor(0.1, (64, 64), (3.0, 3.0, 0.0), 3, ctx=own, scrollTrigger=6)
    for i in range(8):
        true = np.array([3.0 + 0.18 * i, 3.0 + 0.05 * i, 0.04 * i], np.float32)
        proc.Update(hs_mod.ScanCloud(TR.room_scan(sim, true, 120)), true)
    ox, oy = proc.get_origin()
    assert (ox, oy) != (0, 0)                                              # the window has scrolled
    match, last = proc.MatchPose.copy(), proc.LastMapUpdatePose.copy()
    scan = hs_mod.ScanCloud(TR.room_scan(sim, true, 77))
    pw = np.array([match, (3.3, 3.9, 1.0)], np.float32)
    sums, prs = proc.NearestPairs(scan, pw, 1, site_mask=2, radius=10, pairs=True)
    cell0 = F(proc.MapRep.Maps[0].CellLength)
    pl = pw.copy()
    pl[:, 0] = pw[:, 0] - F(ox) * cell0; pl[:, 1] = pw[:, 1] - F(oy) * cell0
    s2, p2 = proc.MapRep.nearest_pairs(pl, 1, site_mask=2, radius=10, pairs=True)   # the scan the processor's call set
    assert np.array_equal(prs, p2) and np.array_equal(sums, s2) and sums[0]["n_matched"] > 60 and sums[0]["n_zero"] > 0
    assert S.same_bits(proc.MatchPose, match) and S.same_bits(proc.LastMapUpdatePose, last) and proc.get_origin() == (ox, oy)
    proc.Dispose(); own.close()


@gpu
def test_refusals(hs_mod, ctx):
    capi = hs_mod.capi
    lib = capi.lib()
    rng = np.random.default_rng(3)
    pts = L.small_points(np.random.default_rng(11), 97)

    def field(rep, level=0, world=0, mask=2, r=8, w=4, h=4):
        out = np.full(32, 77, np.int16)
        rc = lib.slamhip_hs_nearest_field(rep._h, level, world, mask, r, 0, 0, w, h, out.ctypes.data_as(C.c_void_p))
        assert rc != 0 and (out == 77).all()
        return rc

    def pairs(rep, level=0, world=0, mask=2, r=8, B=1, with_pairs=False):
        poses = np.zeros((max(B, 1), 3), np.float32); poses[:, :2] = 2.0
        sums = np.zeros(max(B, 1), capi.PAIR_SUMMARY); sums["n_counted"] = 7
        mark = sums.copy()
        rec = np.full(2 * max(B, 1) * 97 if with_pairs else 2, 77, np.int16)
        rc = lib.slamhip_hs_nearest_pairs(rep._h, level, world, mask, r, capi.fptr(poses), B, sums.ctypes.data_as(C.c_void_p),
                                          rec.ctypes.data_as(C.c_void_p) if with_pairs else None)
        assert rc != 0 and np.array_equal(sums, mark) and (rec == 77).all()
        return rc

    rep = hs_mod.MapRepMultiMap(0.1, (80, 48), 2, ctx=ctx)
    rep.set_backing(8, POOL)
    assert pairs(rep) == capi.ERR_STATE                                    # no scan
    TR.fill(hs_mod, rep, rng)
    rep.shift(34, -22)
    TR.fill(hs_mod, rep, rng)
    rep.set_scan(hs_mod.ScanCloud(pts))
    ck = [rep.Maps[l].checksum() for l in range(2)]
    for kw in (dict(level=-1), dict(level=2), dict(world=2), dict(world=-1), dict(mask=0), dict(mask=8), dict(r=0), dict(r=256)):
        assert field(rep, **kw) == capi.ERR_INVALID, kw
        assert pairs(rep, **kw) == capi.ERR_INVALID, kw
    for w, h in ((0, 4), (4, 0), (-1, 4), (4097, 4096)):
        assert field(rep, w=w, h=h) == capi.ERR_INVALID, (w, h)
    for B in (0, -1, 65537):
        assert pairs(rep, B=B) == capi.ERR_INVALID, B
    assert pairs(rep, B=43241, with_pairs=True) == capi.ERR_INVALID        # 43241 x 97 = 2^22 + 73 records
    ok_s, ok_p = rep.nearest_pairs(np.zeros((43240, 3), np.float32), 0, pairs=True)   # 43240 x 97 <= 2^22 goes through
    assert ok_p.shape == (43240, 97, 2) and (ok_s == ok_s[0]).all()
    n0 = rep.nearest_field(1, (-3, -3, 50, 40), site_mask=3, radius=9, world=True)
    # E too large: one non-Reset cell 9000 cells away on both axes -- R fits the class map's 2^28, E = R + 2 r does not fit 2^26
    far = np.zeros((1, 1), capi.CELL_DTYPE)
    far["update_index"] = 1; far["value"] = 1.0
    assert rep.world_put(0, 9000, 9000, far) == 0
    assert field(rep, world=1) == capi.ERR_INVALID and "2^26" in lib.slamhip_last_error().decode() and " x " in lib.slamhip_last_error().decode()
    assert pairs(rep, world=1) == capi.ERR_INVALID and "2^26" in lib.slamhip_last_error().decode()
    assert np.array_equal(rep.nearest_field(1, (-3, -3, 50, 40), site_mask=3, radius=9, world=True), n0)   # level 1 holds no far tile
    rep.nearest_field(0, (0, 0, 8, 8), world=False)                        # the window's field does not care
    assert [rep.Maps[l].checksum() for l in range(2)] == ck
    rep.close()


@gpu
def test_poisoned_context_refuses(hs_mod):
    """A context poisoned by a blocking wait that timed out (the trace of tests/test_gpu_hector_trace.py: 1 ms against 4096 poses x
    1024 long beams) refuses the field and the pairs at once with SLAMHIP_ERR_TIMEOUT, nothing launched."""
    import time
    capi = hs_mod.capi
    own = hs_mod.Context(0)
    rep = hs_mod.MapRepMultiMap(0.05, (1024, 1024), 1, ctx=own)
    try:
        a = np.linspace(-math.pi, math.pi, 1024, endpoint=False)
        rep.set_scan(hs_mod.ScanCloud(np.stack([25.0 * np.cos(a), 25.0 * np.sin(a)], 1).astype(np.float32)))
        poses = np.tile(np.array([25.6, 25.6, 0.0], np.float32), (4096, 1))
        rep.trace(poses[:2], 0)
        assert rep.nearest_pairs(poses[:2], 0, radius=4)[0]["n_counted"].tolist() == [1024, 1024]
        own.set_wait_timeout(1)
        with pytest.raises(capi.SlamhipError) as e:
            rep.trace(poses, 0)
        assert e.value.code == capi.ERR_TIMEOUT and own.poisoned
        t0 = time.perf_counter()
        with pytest.raises(capi.SlamhipError) as e1:
            rep.nearest_field(0, (0, 0, 4, 4))
        with pytest.raises(capi.SlamhipError) as e2:
            rep.nearest_pairs(poses[:1], 0)
        assert e1.value.code == capi.ERR_TIMEOUT and e2.value.code == capi.ERR_TIMEOUT and time.perf_counter() - t0 < 0.05
    finally:
        rep.close(); own.close()                                           # (destroy waits for the queue to drain: no bound there)
