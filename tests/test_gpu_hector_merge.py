"""The map merge (slamhip_hs_merge_set_source / _score / _apply / _clear_source, slamhip_hsproc_merge_*) on the device, against the
host hook slamhip_debug_merge (hs_merge.h in plain loops) and the NumPy restatement of tests/test_hs_merge_abi.py.  Integers are
compared with ==, Values by their bit patterns; nothing has a tolerance.

Shapes: two-level pyramids of 128 x 96 (2 x 3 tiles of k14_apply, 2 x 6 of k14_score), of 4 x 4 (the smallest slamhip_hs_create
accepts: one partial tile) and of 100 x 70 (neither a multiple of a tile's width nor of its height); sources of 1 x 1, 33 x 31,
200 x 150 (larger than the window) and one whose first cell has negative coordinates; theta 0, 0.3, pi / 4, pi / 2 and -3; a pose
that sources nothing and one that sources exactly one corner cell."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import test_hs_merge_abi as A
from test_gpu_hector_shift import hs_mod, ctx                              # noqa: F401 (fixtures)

gpu = pytest.mark.gpu
F = np.float32
CELL0 = 0.1
DIMS = [(128, 96), (4, 4), (100, 70)]
SOURCES = [(1, 1, 0, 0), (33, 31, 0, 0), (200, 150, -20, -30), (33, 31, -40, -17)]   # w, h, ax, ay
THETAS = [0.0, 0.3, math.pi / 4, math.pi / 2, -3.0]
ADD, FILL, REPLACE = A.ADD, A.FILL, A.REPLACE


def stm_of(rep, level):
    return F(1.0) / F(rep.Maps[level].CellLength)


def poses_for(dims, src, level=0):
    """Window-frame poses for a source: the listed angles about a translation that brings the source over the window, a pose that
    sources nothing, and the identity."""
    c = CELL0 * (1 << level)
    w, h = dims[0] >> level, dims[1] >> level
    sw, sh, ax, ay = src
    # the source's centre cell lands near the window's centre
    P = []
    for t in THETAS:
        cu, cv = ax + sw / 2.0, ay + sh / 2.0
        tx = w / 2.0 - (math.cos(t) * cu - math.sin(t) * cv) + 0.3
        ty = h / 2.0 - (math.sin(t) * cu + math.cos(t) * cv) - 0.2
        P.append((tx * c, ty * c, t))
    P.append((5000.0 * c, 5000.0 * c, 0.7))
    P.append((0.0, 0.0, 0.0))
    return P


def fill(rep, seed, special=True):
    """Both levels filled with test cells -> the cells per level, (h, w)."""
    out = []
    for l in range(2):
        w, h = rep.Maps[l].Dimensions
        c = A.cells_of(w, h, seed + l, special)
        rep.Maps[l].SetCells(c.ravel())
        out.append(c)
    return out


def cells(rep, level):
    w, h = rep.Maps[level].Dimensions
    return rep.Maps[level].GetCells().reshape(h, w)


def report_eq(got, want, apply=True):
    g, w = A.rep_dict(got), A.rep_dict(want)
    if not apply:
        w["n_changed"] = w["n_clamped"] = 0
    return g == w


def device_prob(rep, level):
    """The probability grid the matcher reads, through the reference's cache turned on for the read (its first fill copies the grid)."""
    w, h = rep.Maps[level].Dimensions
    rep.set_reference_cache(1)
    p = rep.Maps[level].GetCachedProbability(np.arange(w * h, dtype=np.int32))
    rep.set_reference_cache(0)
    return np.asarray(p, F)


@pytest.fixture(scope="module")
def pyramids(hs_mod, ctx):
    reps = {d: hs_mod.MapRepMultiMap(CELL0, d, 2, ctx=ctx) for d in DIMS}
    twin = {d: hs_mod.MapRepMultiMap(CELL0, d, 2, ctx=ctx) for d in DIMS}
    yield reps, twin
    for r in list(reps.values()) + list(twin.values()):
        r.close()


# ---- 1. apply and score against the hook -------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("rule", [ADD, FILL, REPLACE])
@pytest.mark.parametrize("dims", DIMS)
def test_apply_matches_hook(hs_mod, pyramids, dims, rule):
    """Every source at every pose: score before, apply, the cells, the report, level 1 untouched, the probabilities against a second
    pyramid given the merged cells through slamhip_hs_cells_upload."""
    capi = hs_mod.capi
    rep, twin = pyramids[0][dims], pyramids[1][dims]
    stm = stm_of(rep, 0)
    n_changed = 0
    for si, src in enumerate(SOURCES):
        sw, sh, ax, ay = src
        scells = A.cells_of(sw, sh, 40 + si)
        for pi, pose in enumerate(poses_for(dims, src)):
            before = fill(rep, 10 * si + pi)
            rep.merge_set_source(0, ax, ay, scells)
            ck1 = rep.Maps[1].checksum()
            want, wrep = capi.debug_merge(before[0], scells, ax, ay, pose, stm, rule, 2.0)
            rwant, rrep = A.np_merge(before[0], scells, ax, ay, pose, stm, rule, 2.0)
            tag = (dims, src, pose, rule)
            assert A.same_cells(want, rwant) and A.rep_dict(wrep) == rrep, tag   # (hook against restatement at these shapes)
            srep = rep.merge_score([pose])[0]
            assert report_eq(srep, wrep, apply=False), (tag, A.rep_dict(srep), A.rep_dict(wrep))
            assert A.same_cells(cells(rep, 0), before[0]), tag             # score changes no cell
            grep = rep.merge_apply(pose, rule, 2.0)
            got = cells(rep, 0)
            assert A.same_cells(got, want), (tag, np.argwhere(got["value"].view(np.uint32) != want["value"].view(np.uint32))[:4].tolist())
            assert report_eq(grep, wrep), (tag, A.rep_dict(grep), A.rep_dict(wrep))
            assert [int(v) for v in grep["joint"]] == [int(v) for v in srep["joint"]] and int(grep["n_unsourced"]) == int(srep["n_unsourced"])
            assert rep.Maps[1].checksum() == ck1, tag
            n_changed += int(grep["n_changed"])
            if pi in (1, 2):
                twin.Maps[0].SetCells(want.ravel())
                assert np.array_equal(device_prob(rep, 0).view(np.uint32), device_prob(twin, 0).view(np.uint32)), tag
    assert n_changed > 0


@gpu
def test_one_corner_cell_and_nothing(hs_mod, pyramids):
    rep = pyramids[0][(128, 96)]
    before = fill(rep, 77)
    src = np.zeros((1, 1), A.CELL); src["value"][0, 0] = F(1.25)
    rep.merge_set_source(0, 0, 0, src)
    r = rep.merge_apply((0.0, 0.0, 0.0), REPLACE, 1.0)
    assert sum(int(v) for v in r["joint"]) == 1 and int(r["n_unsourced"]) == 128 * 96 - 1
    got = cells(rep, 0)
    assert got["value"][0, 0] == F(1.25) and got["update_index"][0, 0] == before[0]["update_index"][0, 0]
    want = before[0].copy(); want["value"][0, 0] = F(1.25)
    assert A.same_cells(got, want)
    ck = rep.Maps[0].checksum()
    for pose in ((900.0, 0.0, 0.3), (float("nan"), 0.0, 0.0), (0.0, float("inf"), 0.0), (0.0, 0.0, float("-inf"))):
        r = rep.merge_apply(pose, ADD, 1.0)
        assert int(r["n_unsourced"]) == 128 * 96 and int(r["n_changed"]) == 0 and rep.Maps[0].checksum() == ck
        assert int(rep.merge_score([pose])[0]["n_unsourced"]) == 128 * 96


@gpu
def test_level_one_source(hs_mod, pyramids):
    """A source of level 1's cell length goes into level 1; level 0 is untouched."""
    capi = hs_mod.capi
    rep = pyramids[0][(128, 96)]
    before = fill(rep, 91)
    src = (33, 31, -3, 4)
    scells = A.cells_of(33, 31, 92)
    rep.merge_set_source(1, -3, 4, scells)
    ck0 = rep.Maps[0].checksum()
    for pose in poses_for((128, 96), src, level=1)[:3]:
        rep.Maps[1].SetCells(before[1].ravel())
        want, wrep = capi.debug_merge(before[1], scells, -3, 4, pose, stm_of(rep, 1), ADD, 3.0)
        grep = rep.merge_apply(pose, ADD, 3.0)
        assert A.same_cells(cells(rep, 1), want) and report_eq(grep, wrep) and rep.Maps[0].checksum() == ck0
        assert int(wrep["n_changed"]) > 0


@gpu
@pytest.mark.parametrize("B", [1, 2, 65, 257, 4096])
def test_score_batches(hs_mod, pyramids, B):
    """Each pose's report against the hook's; the checksum is equal before and after."""
    capi = hs_mod.capi
    dims = (128, 96)
    rep = pyramids[0][dims]
    before = fill(rep, 300 + B)
    sw, sh, ax, ay = SOURCES[2]
    scells = A.cells_of(sw, sh, 301)
    rep.merge_set_source(0, ax, ay, scells)
    rng = np.random.default_rng(B)
    poses = np.stack([rng.uniform(-6.0, 18.0, B), rng.uniform(-6.0, 14.0, B), rng.uniform(-3.5, 3.5, B)], 1).astype(F)
    base = poses_for(dims, SOURCES[2])
    poses[:min(B, len(base))] = np.asarray(base, F)[:min(B, len(base))]
    if B > 20:
        poses[11] = (np.nan, 0.0, 0.0); poses[12] = (0.0, 0.0, np.inf)
    ck = [rep.Maps[l].checksum() for l in range(2)]
    got = rep.merge_score(poses)
    assert [rep.Maps[l].checksum() for l in range(2)] == ck
    stm = stm_of(rep, 0)
    n_sourced = 0
    for i in range(B):
        _, wrep = capi.debug_merge(before[0], scells, ax, ay, poses[i], stm, FILL, 1.0)
        assert report_eq(got[i], wrep, apply=False), (B, i, poses[i].tolist(), A.rep_dict(got[i]), A.rep_dict(wrep))
        n_sourced += sum(int(v) for v in wrep["joint"])
    assert n_sourced > 0


@gpu
def test_match_after_apply(hs_mod, pyramids):
    """slamhip_hs_match on the merged pyramid and on a second pyramid given the merged cells through the upload: equal bits."""
    dims = (128, 96)
    rep, twin = pyramids[0][dims], pyramids[1][dims]
    rng = np.random.default_rng(5)
    base = []
    for l in range(2):
        w, h = rep.Maps[l].Dimensions
        v = np.zeros((h, w), F)
        v[h // 5:4 * h // 5, w // 5:4 * w // 5] = -0.6
        v[h // 5, w // 5:4 * w // 5] = 1.4; v[4 * h // 5, w // 5:4 * w // 5] = 1.4
        v[h // 5:4 * h // 5, w // 5] = 1.4; v[h // 5:4 * h // 5 + 1, 4 * w // 5] = 1.4
        c = np.zeros((h, w), A.CELL); c["value"] = v; c["update_index"] = -1
        base.append(c)
        rep.Maps[l].SetCells(c.ravel())
    src = base[0][10:80, 20:110].copy()
    src["value"] = src["value"] + rng.normal(0, 0.1, src["value"].shape).astype(F)
    rep.merge_set_source(0, 20, 10, src)
    r = rep.merge_apply((0.13, -0.07, 0.02), ADD, 5.0)
    assert int(r["n_changed"]) > 1000
    merged = cells(rep, 0)
    twin.Maps[0].SetCells(merged.ravel()); twin.Maps[1].SetCells(base[1].ravel())
    a = np.linspace(-math.pi, math.pi, 180, endpoint=False)
    xy = np.stack([3.0 * np.cos(a), 2.4 * np.sin(a)], 1).astype(F)
    scan = hs_mod.ScanCloud(xy)
    m = hs_mod.ScanMatcher()
    p1 = m.MatchData(rep, scan, (6.2, 4.9, 0.05))
    p2 = m.MatchData(twin, scan, (6.2, 4.9, 0.05))
    assert np.array_equal(np.asarray(p1, F).view(np.uint32), np.asarray(p2, F).view(np.uint32)) and np.isfinite(p1).all()
    assert A.same_cells(cells(rep, 0), merged)


# ---- 2. both paths -----------------------------------------------------------------------------------------------------------------
@gpu
def test_apply_under_the_switches():
    """test_apply_matches_hook again in fresh interpreters with the tile box staged in LDS (SLAMHIP_K14_STAGED=1) and with the
    32 x 32 tile (SLAMHIP_K14_TILE32=1), direct and staged: the same maps as the default's, each == the hook's."""
    here = os.path.abspath(__file__)
    for extra in ({"SLAMHIP_K14_STAGED": "1"}, {"SLAMHIP_K14_TILE32": "1"}, {"SLAMHIP_K14_TILE32": "1", "SLAMHIP_K14_STAGED": "1"}):
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "pytest", here, "-m", "gpu", "-x", "-q", "-k",
                            "apply_matches_hook or level_one_source or one_corner"],
                           env=dict(os.environ, **extra), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        out = r.stdout.decode(errors="replace")
        assert r.returncode == 0 and " passed" in out and "skipped" not in out, (extra, out[-3000:])


# ---- 3. state ----------------------------------------------------------------------------------------------------------------------
@gpu
def test_after_shift_and_with_backing(hs_mod, ctx):
    """A non-zero origin, poses in the window's frame; with backing on, what lies outside the window is unchanged by an apply."""
    capi = hs_mod.capi
    rep = hs_mod.MapRepMultiMap(CELL0, (64, 48), 2, ctx=ctx)
    try:
        rep.set_backing(16, 8 << 20)
        fill(rep, 500, special=False)
        rep.shift(8, -6)
        assert rep.origin() == (8, -6)
        outside = rep.world_cells(0, -8, -16, 96, 80)
        before = cells(rep, 0)
        assert (outside["value"][:, :16] != 0).any()                       # (the evicted strip lives in tiles)
        scells = A.cells_of(33, 31, 501)
        rep.merge_set_source(0, -5, -5, scells)
        pose = (2.1, 1.7, 0.3)
        want, wrep = capi.debug_merge(before, scells, -5, -5, pose, stm_of(rep, 0), ADD, 2.0)
        grep = rep.merge_apply(pose, ADD, 2.0)
        assert A.same_cells(cells(rep, 0), want) and report_eq(grep, wrep) and int(grep["n_changed"]) > 0
        after = rep.world_cells(0, -8, -16, 96, 80)
        win = np.zeros(after.shape, bool); win[10:58, 16:80] = True           # the window: world cells [8, 72) x [-6, 42)
        assert A.same_cells(after[win].reshape(48, 64), want)
        assert np.array_equal(after[~win].view(np.uint64), outside[~win].view(np.uint64))
        assert rep.origin() == (8, -6)
    finally:
        rep.close()


@gpu
def test_source_lifetime(hs_mod, pyramids):
    """The source survives a grid update and a match; set_source twice keeps the second; it is gone after Reset and clear_source."""
    capi = hs_mod.capi
    rep = pyramids[0][(128, 96)]
    fill(rep, 600, special=False)
    first = A.cells_of(33, 31, 601); second = A.cells_of(5, 3, 602)
    rep.merge_set_source(0, 0, 0, first)
    rep.merge_set_source(0, 2, 1, second)
    a = np.linspace(-math.pi, math.pi, 90, endpoint=False)
    scan = hs_mod.ScanCloud(np.stack([2.0 * np.cos(a), 2.0 * np.sin(a)], 1).astype(F))
    rep.UpdateByScan(scan, np.array([6.0, 4.5, 0.1], F))
    hs_mod.ScanMatcher().MatchData(rep, scan, (6.0, 4.5, 0.1))
    before = cells(rep, 0)
    pose = (3.0, 2.0, 0.3)
    want, wrep = capi.debug_merge(before, second, 2, 1, pose, stm_of(rep, 0), REPLACE, 1.0)
    assert report_eq(rep.merge_score([pose])[0], wrep, apply=False)
    grep = rep.merge_apply(pose, REPLACE, 1.0)
    assert A.same_cells(cells(rep, 0), want) and report_eq(grep, wrep)
    rep.merge_clear_source()
    for call in (lambda: rep.merge_score([pose]), lambda: rep.merge_apply(pose, ADD, 1.0)):
        with pytest.raises(capi.SlamhipError) as e:
            call()
        assert e.value.code == capi.ERR_STATE
    rep.merge_set_source(0, 2, 1, second)
    rep.Reset()
    ck = rep.Maps[0].checksum()
    for call in (lambda: rep.merge_score([pose]), lambda: rep.merge_apply(pose, ADD, 1.0)):
        with pytest.raises(capi.SlamhipError) as e:
            call()
        assert e.value.code == capi.ERR_STATE
    assert rep.Maps[0].checksum() == ck


@gpu
def test_through_the_processor(hs_mod, ctx):
    """slamhip_hsproc_merge_*: world poses, the window moved -- equal to the hs calls at the poses minus (float)origin * cell0."""
    capi = hs_mod.capi
    proc = hs_mod.HectorSLAMProcessor(CELL0, (64, 48), [3.2, 2.4, 0.0], 2, ctx=ctx, scrollTrigger=4)
    try:
        rep = proc.MapRep
        fill(rep, 700, special=False)
        scells = A.cells_of(33, 31, 701)
        world = np.array([[2.9, 1.1, 0.3], [3.4, 0.2, -3.0], [1.0, 1.0, math.pi / 4]], F)
        proc.merge_set_source(0, -5, -5, scells)
        assert np.array_equal(proc.merge_score(world).view(np.int64), rep.merge_score(world).view(np.int64))   # the origin at (0, 0): every bit passes
        proc.shift(8, -6)
        assert proc.get_origin() == (8, -6)
        off = np.array([F(8) * F(CELL0), F(-6) * F(CELL0)], F)
        win = world.copy(); win[:, 0] = world[:, 0] - off[0]; win[:, 1] = world[:, 1] - off[1]
        before = cells(rep, 0)
        got = proc.merge_score(world)
        assert np.array_equal(got.view(np.int64), rep.merge_score(win).view(np.int64))
        want, wrep = capi.debug_merge(before, scells, -5, -5, win[0], stm_of(rep, 0), FILL, 1.0)
        assert report_eq(got[0], wrep, apply=False)
        grep = proc.merge_apply(world[0], FILL, 1.0)
        assert A.same_cells(cells(rep, 0), want) and report_eq(grep, wrep) and int(grep["n_changed"]) > 0
    finally:
        proc.Dispose()


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------
@gpu
def test_refusals(hs_mod, pyramids):
    """Each refusal leaves the map's checksum equal and the source that was set."""
    capi = hs_mod.capi
    rep = pyramids[0][(128, 96)]
    before = fill(rep, 800, special=False)
    scells = A.cells_of(33, 31, 801)
    rep.merge_set_source(0, 1, 2, scells)
    pose = (4.0, 3.0, 0.3)
    ck = [rep.Maps[l].checksum() for l in range(2)]
    one = np.zeros((1, 1), A.CELL)
    refused = [
        (lambda: rep.merge_set_source(-1, 0, 0, one), capi.ERR_INVALID), (lambda: rep.merge_set_source(2, 0, 0, one), capi.ERR_INVALID),
        (lambda: rep.merge_set_source(0, 2 ** 30 + 1, 0, one), capi.ERR_INVALID), (lambda: rep.merge_set_source(0, 0, -2 ** 30 - 1, one), capi.ERR_INVALID),
        (lambda: capi.call("slamhip_hs_merge_set_source", rep._h, 0, 0, 0, 0, 1, one.ctypes.data), capi.ERR_INVALID),
        (lambda: capi.call("slamhip_hs_merge_set_source", rep._h, 0, 0, 0, 1, 0, one.ctypes.data), capi.ERR_INVALID),
        (lambda: capi.call("slamhip_hs_merge_set_source", rep._h, 0, 0, 0, 8193, 8192, one.ctypes.data), capi.ERR_INVALID),   # 2^26 + 8192 cells
        (lambda: rep.merge_score(np.zeros((0, 3), F)), capi.ERR_INVALID), (lambda: rep.merge_score(np.zeros((4097, 3), F)), capi.ERR_INVALID),
        (lambda: rep.merge_apply(pose, -1, 1.0), capi.ERR_INVALID), (lambda: rep.merge_apply(pose, 3, 1.0), capi.ERR_INVALID),
        (lambda: rep.merge_apply(pose, ADD, 0.0), capi.ERR_INVALID), (lambda: rep.merge_apply(pose, FILL, -1.0), capi.ERR_INVALID),
        (lambda: rep.merge_apply(pose, REPLACE, float("nan")), capi.ERR_INVALID), (lambda: rep.merge_apply(pose, ADD, float("inf")), capi.ERR_INVALID),
    ]
    for i, (call, code) in enumerate(refused):
        with pytest.raises(capi.SlamhipError) as e:
            call()
        assert e.value.code == code, i
        assert [rep.Maps[l].checksum() for l in range(2)] == ck, i
    rep.set_reference_cache(1)
    with pytest.raises(capi.SlamhipError) as e:
        rep.merge_apply(pose, ADD, 1.0)
    assert e.value.code == capi.ERR_INVALID and "cache" in str(e.value)
    assert [rep.Maps[l].checksum() for l in range(2)] == ck
    rep.merge_score([pose])                                                # (rating changes nothing and is allowed)
    rep.set_reference_cache(0)
    # the source that was set is still there, and with the cache off again the apply goes through
    want, wrep = capi.debug_merge(before[0], scells, 1, 2, pose, stm_of(rep, 0), ADD, 1.0)
    assert report_eq(rep.merge_apply(pose, ADD, 1.0), wrep) and A.same_cells(cells(rep, 0), want)


@gpu
def test_poisoned_context_refuses(hs_mod):
    """A context poisoned by a blocking wait that timed out (1 ms against a trace of 4096 poses x 1024 long beams) refuses
    set_source, score and apply at once with SLAMHIP_ERR_TIMEOUT."""
    import time
    capi = hs_mod.capi
    own = hs_mod.Context(0)
    rep = hs_mod.MapRepMultiMap(0.05, (1024, 1024), 1, ctx=own)
    try:
        a = np.linspace(-math.pi, math.pi, 1024, endpoint=False)
        rep.set_scan(hs_mod.ScanCloud(np.stack([25.0 * np.cos(a), 25.0 * np.sin(a)], 1).astype(F)))
        poses = np.tile(np.array([25.6, 25.6, 0.0], F), (4096, 1))
        rep.trace(poses[:2], 0)
        src = A.cells_of(5, 3, 900)
        rep.merge_set_source(0, 0, 0, src)
        assert int(rep.merge_score([(1.0, 1.0, 0.3)])[0]["n_unsourced"]) < 1024 * 1024
        own.set_wait_timeout(1)
        with pytest.raises(capi.SlamhipError) as e:
            rep.trace(poses, 0)
        assert e.value.code == capi.ERR_TIMEOUT and own.poisoned
        t0 = time.perf_counter()
        for call in (lambda: rep.merge_score([(1.0, 1.0, 0.3)]), lambda: rep.merge_apply((1.0, 1.0, 0.3), ADD, 1.0),
                     lambda: rep.merge_set_source(0, 0, 0, src)):
            with pytest.raises(capi.SlamhipError) as e1:
                call()
            assert e1.value.code == capi.ERR_TIMEOUT
        assert time.perf_counter() - t0 < 0.05
    finally:
        rep.close(); own.close()                                           # (destroy waits for the queue to drain: no bound there)
