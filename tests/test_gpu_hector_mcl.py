"""The particle-filter localisation step (slamhip_hs_mcl_set / _step / _get, slamhip_hsproc_mcl_step) on the device, against the host
hook slamhip_debug_mcl_step (hs_mcl.h in plain loops) and the NumPy / Python-integer restatement of tests/test_hs_mcl_abi.py, fed
from cells_download / world_cells_download.  Integers are compared with ==, floats by their bit patterns; nothing has a tolerance.

Shapes: a 128 x 96 pyramid of two levels; N = 1, 64, 65 (a wavefront and one more), 1000 (several workgroups of every kernel),
4097 (one past k13_scan's chunk of 4096), 8193 (one past the 4 x 2048 particles k13_score's grid takes at one per wavefront: the
first wavefront takes a second particle and carries its minima; three chunks of the scan: the carry is carried again) and 65536
(the library's largest set: eight particles per wavefront, sixteen chunks, an index that fills key_best's 16 bits); scans of 1
point and of 360 (lanes with 5 and with 6 points)."""
import ctypes as C
import math

import numpy as np
import pytest

import test_gpu_hector_lattice as L
import test_gpu_hector_shift as S
import test_gpu_hector_trace as TR
import test_hs_dfield_abi as D
import test_hs_mcl_abi as M
from test_gpu_hector_shift import hs_mod, ctx                              # noqa: F401 (fixtures)

gpu = pytest.mark.gpu
F = np.float32
POOL = 64 << 20
W0, H0 = 128, 96
ROOM_M = (1.6, 1.2, 11.2, 8.0)                                             # metres: cells 16 .. 112 x 12 .. 80 of level 0, 8 .. 56 x 6 .. 40 of level 1
TRUTH = np.array([5.3, 4.4, 0.3], F)
R, MASK = 8, 2


def room_values(level):
    """The room on one level: walls > 0, the inside < 0, a pillar, unknown space around."""
    w, h = W0 >> level, H0 >> level
    x0, y0, x1, y1 = (int(round(v * 10)) >> level for v in ROOM_M)
    v = np.zeros((h, w), F)
    v[y0:y1 + 1, x0:x1 + 1] = 1.5
    v[y0 + 1:y1, x0 + 1:x1] = -0.7
    v[h // 2:h // 2 + 3, w // 2 + 6:w // 2 + 9] = 2.0
    return v


def draw(hs_mod, rep):
    for level in range(2):
        L.put_values(hs_mod, rep, level, room_values(level).ravel())


def window_classes(rep, level):
    w, h = rep.Maps[level].Dimensions
    return D.np_class_bits(rep.Maps[level].GetCells()["value"].reshape(h, w))


def field_of(cls, mask, r, ax0=0, ay0=0):
    """(field, rect, const) for M.np_mcl_step: cls's first element is window-frame cell (ax0, ay0); the rectangle is E and a margin."""
    h, w = cls.shape
    rel = (-r - 2, -r - 2, w + 2 * r + 4, h + 2 * r + 4)
    return D.np_field(cls, mask, r, rel), (rel[0] + ax0, rel[1] + ay0, rel[2], rel[3]), 0 if mask & 1 else r * r


def hook_spec(spec):
    """The spec as the hook takes it: its one level is level 0, its class array the whole map."""
    h = spec.copy()
    h["level"] = 0; h["world"] = 0
    return h


def got_of(rep, summary):
    p, a, k = rep.mcl_get()
    return p, a, k, summary


def assert_same(got, hook, tag):
    """The device's (particles, acc, ancestors, summary) against the hook's, field by field."""
    for f in M.SUMMARY_FIELDS:
        assert int(got[3][f]) == int(hook[3][f]), (tag, f, int(got[3][f]), int(hook[3][f]))
    assert np.array_equal(got[2], hook[2]), (tag, "ancestors")
    assert np.array_equal(got[1], hook[1]), (tag, "acc")
    assert np.array_equal(M.bits(got[0]), M.bits(hook[0])), (tag, "particles", np.argwhere(M.bits(got[0]) != M.bits(hook[0]))[:4].tolist())


@pytest.fixture(scope="module")
def pyramid(hs_mod, ctx):
    rep = hs_mod.MapRepMultiMap(0.1, (W0, H0), 2, ctx=ctx)
    draw(hs_mod, rep)
    cls = [window_classes(rep, l) for l in range(2)]
    fields = [field_of(c, MASK, R) for c in cls]
    for c, f in zip(cls, fields):
        c.setflags(write=False); f[0].setflags(write=False)
    yield rep, cls, fields
    rep.close()


# ---- 1. device against hook and restatement ----------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("n_points", [1, 360])
@pytest.mark.parametrize("N", [1, 64, 65, 1000, 4097, 8193, 65536])
def test_five_steps(hs_mod, pyramid, N, n_points, level):
    """Five consecutive steps on the window, mcl_get compared after each: n_eff_min = 0, N + 1, a middle value, 0, N + 1 -- both
    branches, and each branch entered from the other.  The hook runs every step at every N.  The restatement, pure Python per
    particle, is limited ON PURPOSE above N = 1000 so that a case stays within seconds (it takes the hook's particles, which are the
    device's, as its input, so any step can be checked alone): every step up to N = 1000; steps 0, 1 and 4 of N = 4097 -- the first
    step, the first resampling entered from accumulated costs, the last; steps 0 and 1 of N = 8193; none at N = 65536, where one
    step of it takes nine seconds: there the device is held to the hook, which tests/test_hs_mcl_abi.py holds to the restatement."""
    capi = hs_mod.capi
    rep, cls, fields = pyramid
    stm = TR.stm_of(rep, level)
    xy = M.room_scan(n_points, TRUTH, ROOM_M)
    p = M.cloud(N, 900 + N + n_points + level, centre=TRUTH)
    rep.set_scan(hs_mod.ScanCloud(xy))
    rep.mcl_set(p)
    g0 = rep.mcl_get()
    assert np.array_equal(M.bits(g0[0]), M.bits(p)) and not g0[1].any() and g0[2].tolist() == list(range(N))
    acc = None
    beta = capi.mcl_beta(2.0, max(1.0, n_points / 8.0))
    seen = set()
    for step, n_eff_min in enumerate((0, N + 1, N // 2 + 1, 0, N + 1)):
        spec = capi.mcl_spec(level, R, (0.06, -0.01, 0.03), (0.02, 0.01, 0.01), beta, n_eff_min, seed=0xFEEDFACE12345 + N, stream=step, site_mask=MASK)
        got = got_of(rep, rep.mcl_step(spec))
        hook = capi.debug_mcl_step(cls[level], stm, xy, p, hook_spec(spec), acc)
        assert_same(got, hook, (N, n_points, level, step))
        if N <= 1000 or (N == 4097 and step in (0, 1, 4)) or (N == 8193 and step in (0, 1)):
            f = fields[level]
            M.check(got, M.np_mcl_step(f[0], f[1], f[2], stm, xy, p, acc, M.spec_dict(spec)), (N, n_points, level, step, "restatement"))
        seen.add(int(got[3]["resampled"]))
        p, acc = got[0], got[1]
        if not got[3]["resampled"]:                                        # acc' = a - min a: the first particle with acc' = 0 is key_best's index
            assert int(got[3]["key_best"]) & 0xFFFF == int(np.argmin(got[1])) and got[1].min() == 0
    assert seen == {0, 1}


# ---- 2. the world, a shift, frame_offset -------------------------------------------------------------------------------------------
WORLD_RECTS = [(-64, -64, 288, 256), (-32, -32, 144, 128)]                 # world cells per level: every window position below and its tiles, grown


@gpu
@pytest.mark.parametrize("level", [0, 1])
def test_world_variant_after_a_shift(hs_mod, ctx, level):
    """A pyramid with a backing store: two steps, then slamhip_hs_shift moves the window so that part of the room lies in tiles
    alone, and the next steps carry frame_offset = -(shift) * cell.  world = 1 scores against the window AND the tiles (the
    restatement over world_cells_download), world = 0 against the window alone (hook and restatement); the two differ."""
    capi = hs_mod.capi
    N, n_points = 257, 360
    rep = hs_mod.MapRepMultiMap(0.1, (W0, H0), 2, ctx=ctx)
    rep.set_backing(16, POOL)
    draw(hs_mod, rep)
    stm = TR.stm_of(rep, level)
    xy = M.room_scan(n_points, TRUTH, ROOM_M)
    rep.set_scan(hs_mod.ScanCloud(xy))
    p = M.cloud(N, 5 + level, centre=TRUTH)
    rep.mcl_set(p)
    acc = None
    beta = capi.mcl_beta(2.0, 45.0)
    dx, dy = 44, -26
    costs = {}
    for step, (world, n_eff_min) in enumerate(((1, 0), (0, N + 1), (1, 0), (0, 0), (1, N + 1))):
        fo = (0.0, 0.0)
        if step == 2:
            rep.shift(dx, dy)
            assert rep.origin() == (dx, dy) and rep.backing_stats()["tiles"] > 3
            fo = (-(F(dx) * F(0.1)), -(F(dy) * F(0.1)))
        spec = capi.mcl_spec(level, R, (0.05, 0.02, -0.02), (0.02, 0.02, 0.01), beta, n_eff_min, seed=77, stream=step, site_mask=MASK, world=world,
                             frame_offset=fo)
        got = got_of(rep, rep.mcl_step(spec))
        cls = window_classes(rep, level)
        if world:
            values, ax0, ay0 = TR.world_values(rep, level, WORLD_RECTS[level])
            f = field_of(D.np_class_bits(values), MASK, R, ax0, ay0)
        else:
            f = field_of(cls, MASK, R)
            assert_same(got, capi.debug_mcl_step(cls, stm, xy, p, hook_spec(spec), acc), (level, step, "hook"))
        M.check(got, M.np_mcl_step(f[0], f[1], f[2], stm, xy, p, acc, M.spec_dict(spec)), (level, step, world))
        costs[step] = (int(got[3]["cost_min"]), int(got[3]["cost_max"]))
        p, acc = got[0], got[1]
    # after the shift the window has lost the room's left part: the window alone scores the best particle worse than the world does
    assert costs[3][0] > costs[2][0] and costs[2][0] < n_points * 4
    rep.close()


# ---- 3. nothing else changes -------------------------------------------------------------------------------------------------------
@gpu
def test_other_calls_unaffected(hs_mod, pyramid):
    capi = hs_mod.capi
    rep, cls, _ = pyramid
    xy = M.room_scan(360, TRUTH, ROOM_M)
    rep.set_scan(hs_mod.ScanCloud(xy))
    poses = M.cloud(65, 3, centre=TRUTH)
    rect = (-R - 2, -R - 2, W0 + 2 * R + 4, H0 + 2 * R + 4)
    before = (rep.distance_score(poses, 0, site_mask=MASK, radius=R, points=True), rep.distance_field(0, rect, site_mask=3, radius=21),
              rep.distance_score(poses, 1, site_mask=3, radius=30), [rep.Maps[l].checksum() for l in range(2)])
    rep.mcl_set(poses)
    for step, (level, n_eff_min) in enumerate(((0, 0), (1, 66), (0, 66))):
        s = rep.mcl_step(capi.mcl_spec(level, R, (0.05, 0.0, 0.01), (0.02, 0.02, 0.01), 4000, n_eff_min, seed=1, stream=step, site_mask=MASK))
        assert s["n_particles"] == 65 and s["resampled"] == (n_eff_min == 66)
    after = (rep.distance_score(poses, 0, site_mask=MASK, radius=R, points=True), rep.distance_field(0, rect, site_mask=3, radius=21),
             rep.distance_score(poses, 1, site_mask=3, radius=30), [rep.Maps[l].checksum() for l in range(2)])
    assert np.array_equal(before[0][0], after[0][0]) and np.array_equal(before[0][1], after[0][1]) and before[0][0]["n_zero"].sum() > 0
    assert np.array_equal(before[1], after[1]) and np.array_equal(before[2][0], after[2][0]) and before[3] == after[3]
    for l in range(2):
        assert np.array_equal(window_classes(rep, l), cls[l])
    # the step's cost is the score's: sum_d2 + r^2 * n_ignored at the predicted poses (sigma = 0, no motion: the poses themselves)
    rep.mcl_set(poses)
    s = rep.mcl_step(capi.mcl_spec(0, R, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 4000, 0, site_mask=MASK))
    sums = before[0][0]
    cost = sums["sum_d2"].astype(np.int64) + R * R * sums["n_ignored"].astype(np.int64)
    assert s["cost_min"] == cost.min() and s["cost_max"] == cost.max() and np.array_equal(rep.mcl_get()[1].astype(np.int64), cost - cost.min())


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------
@gpu
def test_refusals(hs_mod, ctx):
    capi = hs_mod.capi
    lib = capi.lib()
    vp = C.c_void_p
    rep = hs_mod.MapRepMultiMap(0.1, (W0, H0), 2, ctx=ctx)
    draw(hs_mod, rep)
    N = 9

    def step(**kw):
        spec = capi.mcl_spec(0, R, (0.1, 0.0, 0.0), (0.01, 0.01, 0.01), 100, 2)
        for k, v in kw.items():
            if k in ("delta", "sigma", "frame_offset"):
                spec[k][0][v[0]] = v[1]
            else:
                spec[k] = v
        out = np.full(96, 7, np.uint8)
        rc = lib.slamhip_hs_mcl_step(rep._h, spec.ctypes.data_as(vp), out.ctypes.data_as(vp))
        assert rc != 0 and (out == 7).all()
        return rc

    assert step() == capi.ERR_STATE                                        # no particle set
    buf = np.full((N, 3), 7.0, F)
    assert lib.slamhip_hs_mcl_get(rep._h, buf.ctypes.data_as(vp), None, None, N) == capi.ERR_STATE and (buf == 7.0).all()
    good = M.cloud(N, 1, centre=TRUTH)
    for bad_n in (0, -1, 65537):
        assert lib.slamhip_hs_mcl_set(rep._h, good.ctypes.data_as(vp), bad_n) == capi.ERR_INVALID
    bad = good.copy(); bad[4, 2] = np.nan
    assert lib.slamhip_hs_mcl_set(rep._h, bad.ctypes.data_as(vp), N) == capi.ERR_INVALID
    assert step() == capi.ERR_STATE                                        # still no set
    rep.mcl_set(good)
    assert step() == capi.ERR_STATE and b"scan" in lib.slamhip_last_error()   # no scan
    rep.set_scan(hs_mod.ScanCloud(M.room_scan(37, TRUTH, ROOM_M)))
    ck = [rep.Maps[l].checksum() for l in range(2)]
    cases = [dict(level=2), dict(level=-1), dict(world=2), dict(world=-1), dict(site_mask=0), dict(site_mask=8), dict(radius=0), dict(radius=256),
             dict(beta=0), dict(n_eff_min=-1), dict(n_eff_min=N + 2)]
    cases += [dict([(name, (i, v))]) for name, n in (("delta", 3), ("sigma", 3), ("frame_offset", 2)) for i in range(n) for v in (np.nan, np.inf)]
    for kw in cases:
        assert step(**kw) == capi.ERR_INVALID, kw
    assert lib.slamhip_hs_mcl_get(rep._h, buf.ctypes.data_as(vp), None, None, N + 1) == capi.ERR_INVALID and (buf == 7.0).all()
    rep.set_scan(hs_mod.ScanCloud(np.zeros((capi.MCL_MAX_POINTS + 1, 2), F)))
    assert step() == capi.ERR_INVALID and b"LDS" in lib.slamhip_last_error()
    rep.set_scan(hs_mod.ScanCloud(np.zeros((capi.MCL_MAX_POINTS, 2), F)))  # the largest scan the LDS takes goes through
    s = rep.mcl_step(capi.mcl_spec(0, R, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 100, N + 1))
    assert s["resampled"] == 1 and s["n_particles"] == N and s["cost_max"] <= capi.MCL_MAX_POINTS * R * R
    p, a, k = rep.mcl_get()
    assert not a.any() and np.all(np.diff(k) >= 0) and [rep.Maps[l].checksum() for l in range(2)] == ck
    assert rep.mcl_get(poses=False, acc=False)[2].tolist() == k.tolist() and rep.mcl_get(ancestors=False)[2] is None
    rep.close()


@gpu
def test_poisoned_context_refuses(hs_mod):
    """A context poisoned by a blocking wait that timed out (the trace of tests/test_gpu_hector_trace.py: 1 ms against 4096 poses x
    1024 long beams) refuses set, step and get at once with SLAMHIP_ERR_TIMEOUT, nothing launched."""
    import time
    capi = hs_mod.capi
    own = hs_mod.Context(0)
    rep = hs_mod.MapRepMultiMap(0.05, (1024, 1024), 1, ctx=own)
    try:
        a = np.linspace(-math.pi, math.pi, 1024, endpoint=False)
        rep.set_scan(hs_mod.ScanCloud(np.stack([25.0 * np.cos(a), 25.0 * np.sin(a)], 1).astype(np.float32)))
        poses = np.tile(np.array([25.6, 25.6, 0.0], np.float32), (4096, 1))
        rep.trace(poses[:2], 0)
        rep.mcl_set(poses[:8])
        spec = capi.mcl_spec(0, 4, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 100, 0)
        assert rep.mcl_step(spec)["n_particles"] == 8
        own.set_wait_timeout(1)
        with pytest.raises(capi.SlamhipError) as e:
            rep.trace(poses, 0)
        assert e.value.code == capi.ERR_TIMEOUT and own.poisoned
        t0 = time.perf_counter()
        for call in (lambda: rep.mcl_step(spec), lambda: rep.mcl_set(poses[:8]), lambda: rep.mcl_get()):
            with pytest.raises(capi.SlamhipError) as e1:
                call()
            assert e1.value.code == capi.ERR_TIMEOUT
        assert time.perf_counter() - t0 < 0.05
    finally:
        rep.close(); own.close()                                           # (destroy waits for the queue to drain: no bound there)


# ---- 5. the processor --------------------------------------------------------------------------------------------------------------
@gpu
def test_processor_localise_across_a_shift(hs_mod):
    """LocaliseInit / LocaliseStep take and give WORLD poses; when the window moves between two steps the second carries the movement
    as frame_offset.  Expected: the hook on the window's classes with that offset; MatchPose and the map stay what they were."""
    capi = hs_mod.capi
    own = hs_mod.Context(0)
    proc = hs_mod.HectorSLAMProcessor(0.1, (W0, H0), (5.0, 4.0, 0.0), 2, ctx=own)
    rep = proc.MapRep
    draw(hs_mod, rep)
    N = 300
    scan = hs_mod.ScanCloud(M.room_scan(180, TRUTH, ROOM_M))
    pw = M.cloud(N, 8, spread=(0.3, 0.3, 0.2), centre=TRUTH, outliers=False)
    proc.LocaliseInit(pw)
    match = proc.MatchPose.copy()
    beta = capi.mcl_beta(2.0, 20.0)
    kw = dict(level=0, beta=beta, site_mask=MASK, radius=R, seed=4)
    pose, n_eff, n_distinct, s0 = proc.LocaliseStep(scan, (0.0, 0.0, 0.0), (0.01, 0.01, 0.005), n_eff_min=N + 1, stream=0, **kw)
    hook = capi.debug_mcl_step(window_classes(rep, 0), TR.stm_of(rep, 0), scan.Points, pw,
                               capi.mcl_spec(0, R, (0.0, 0.0, 0.0), (0.01, 0.01, 0.005), beta, N + 1, seed=4, stream=0, site_mask=MASK))
    assert_same(got_of(rep, s0), hook, "before")
    assert np.hypot(pose[0] - TRUTH[0], pose[1] - TRUTH[1]) < 0.15 and abs(pose[2] - TRUTH[2]) < 0.05 and 1.0 <= n_eff <= N and n_distinct == s0["n_distinct"]
    ck = [rep.Maps[l].checksum() for l in range(2)]
    proc.shift(12, -8)
    ck2 = [rep.Maps[l].checksum() for l in range(2)]
    fo = (-(F(12) * F(0.1)), -(F(-8) * F(0.1)))
    pose2, n_eff2, _, s1 = proc.LocaliseStep(scan, (0.0, 0.0, 0.0), (0.01, 0.01, 0.005), n_eff_min=0, stream=1, **kw)
    hook2 = capi.debug_mcl_step(window_classes(rep, 0), TR.stm_of(rep, 0), scan.Points, hook[0],
                                capi.mcl_spec(0, R, (0.0, 0.0, 0.0), (0.01, 0.01, 0.005), beta, 0, seed=4, stream=1, site_mask=MASK, frame_offset=fo), hook[1])
    assert_same(got_of(rep, s1), hook2, "after")
    assert np.hypot(pose2[0] - TRUTH[0], pose2[1] - TRUTH[1]) < 0.15 and abs(pose2[2] - TRUTH[2]) < 0.05   # still a WORLD pose
    assert S.same_bits(proc.MatchPose, match) and [rep.Maps[l].checksum() for l in range(2)] == ck2 and ck != ck2
    proc.Dispose(); own.close()


# ---- 6. convergence ----------------------------------------------------------------------------------------------------------------
@gpu
def test_convergence_on_a_simulated_drive(hs_mod, pyramid):
    """2000 particles spread 0.5 m / 20 degrees around the truth, 20 steps of a drive through the room (0.08 m and 0.02 rad per step,
    180 wall points per scan, odometry exact, noise 0.02 m / 0.01 rad).  The device's weighted-mean pose must end no further from the
    truth than the restatement's own filter run here on the CPU with the same seeds; every summary is compared on the way, so the two
    are bit-equal and the bound has no slack.  The library sets no threshold.  Reached on an MI355X, and by the restatement: 0.0006 m
    and 0.0005 rad from the truth after the 20 steps (0.0196 m after the first), n_eff 1828 of 2000; the run prints its figures."""
    capi = hs_mod.capi
    rep, cls, fields = pyramid
    level, N, n_points = 0, 2000, 180
    stm = TR.stm_of(rep, level)
    f = fields[level]
    truth = TRUTH.astype(np.float64)
    p = M.cloud(N, 2024, centre=TRUTH, outliers=False)
    rep.mcl_set(p)
    acc = None
    beta = capi.mcl_beta(2.0, n_points / 8.0)
    delta = (0.08, 0.0, 0.02)
    for step in range(20):
        truth = np.array([truth[0] + math.cos(truth[2]) * delta[0], truth[1] + math.sin(truth[2]) * delta[0], truth[2] + delta[2]])
        xy = M.room_scan(n_points, truth, ROOM_M)
        spec = capi.mcl_spec(level, R, delta, (0.02, 0.02, 0.01), beta, N // 2, seed=99, stream=step, site_mask=MASK)
        s = rep.mcl_step(spec, scan=hs_mod.ScanCloud(xy))
        want = M.np_mcl_step(f[0], f[1], f[2], stm, xy, p, acc, M.spec_dict(spec))
        for name in M.SUMMARY_FIELDS:
            assert int(s[name]) == want[3][name], (step, name)
        p, acc = want[0], want[1]
    got = rep.mcl_get()
    assert np.array_equal(M.bits(got[0]), M.bits(p)) and [int(v) for v in got[1]] == acc
    dev, _ = capi.mcl_mean(s)
    cpu, n_eff = capi.mcl_mean({k: want[3][k] for k in ("A", "Q", "sum_hx", "sum_hy", "sum_hs", "sum_hc")})
    d_dev, d_cpu = math.hypot(dev[0] - truth[0], dev[1] - truth[1]), math.hypot(cpu[0] - truth[0], cpu[1] - truth[1])
    print("convergence: %.4f m, %.4f rad from the truth after 20 steps, n_eff %.1f" % (d_dev, abs(dev[2] - truth[2]), n_eff))
    assert d_dev <= d_cpu and abs(dev[2] - truth[2]) <= abs(cpu[2] - truth[2])
