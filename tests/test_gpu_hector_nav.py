"""The cost-to-go field (slamhip_hs_nav_field, slamhip_hsproc_nav_field) on the device, against the restatement of the definition in
tests/test_hs_nav_abi.py (brute-force clearance, shifted arrays for the moves, a heapq Dijkstra, literal loops for dir, goals and
paths) and against the hook's sequential Dijkstra, fed from cells_download / world_cells_download.  Everything is compared with ==
on integers; there is no tolerance anywhere.

Shapes are the smallest at which each path can go wrong: the 80 x 48 x 2 pyramid (one and two relaxation tiles across, rows of 2.5
and 1.25 traversable words), a level of (3 T + 16) x (2 T + 8) cells -- 4 x 3 tiles, no multiple of the tile or of a word either way
-- for everything that must cross a tile seam, and a window whose level-1 origin is odd over backing tiles of 16 cells."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import test_gpu_hector_frontier as FG
import test_gpu_hector_lattice as L
import test_gpu_hector_shift as S
import test_gpu_hector_trace as TR
import test_hs_nav_abi as NV
from test_gpu_hector_frontier import small                                 # noqa: F401 (fixture)
from test_gpu_hector_shift import hs_mod, ctx                              # noqa: F401 (fixtures)

gpu = pytest.mark.gpu
F = np.float32
POOL = 64 << 20
_SRC = open(os.path.join(NV.ROOT, "slam.net_amd", "csrc", "hs_nav.hip")).read()
T = int(re.search(r"#define K11_TILE (\d+)", _SRC).group(1))               # cells per side of a relaxation tile
SEAM_W, SEAM_H = 3 * T + 16, 2 * T + 8
SEAM_TILES = 4 * 3


def assert_nav(hs_mod, rep, level, cls, m, sources, c=0, site_mask=2, max_cost=0, goals=(), n_paths=0, max_path_cells=1, world=False, grow=3,
               hook=True, tag=None):
    """One call with the rectangle M grown by `grow` cells against the restatement over cls (the classes of M = m), and against the
    hook on the same classes.  -> the call's result."""
    rect = (m[0] - grow, m[1] - grow, m[2] + 2 * grow, m[3] + 2 * grow)
    got = rep.nav_field(level, sources, c, site_mask, max_cost, world, goals, n_paths, max_path_cells, rect)
    want = NV.np_nav(cls, sources, c, site_mask, max_cost, goals, n_paths, max_path_cells, m[0], m[1], rect)
    NV.check(got, want, tag)
    if grow:
        assert (got["cost"][:grow] == NV.UNREACHED).all() and (got["dir"][:, -grow:] == 255).all()
    if hook:                                                               # the hook works in M's own cells
        off = np.array([m[0], m[1]])
        g4 = np.asarray(goals, np.int64).reshape(-1, 4) - np.tile(off, 2)
        hk = hs_mod.capi.debug_nav_field(cls, np.asarray(sources, np.int64).reshape(-1, 2) - off, site_mask, c, max_cost, g4, n_paths, max_path_cells,
                                         rect=(-grow, -grow, rect[2], rect[3]))
        assert np.array_equal(hk["cost"], got["cost"]) and np.array_equal(hk["dir"], got["dir"]), tag
        assert [int(v) for v in hk["path_cells"]] == [int(v) for v in got["path_cells"]]
        assert [int(r["cost"]) for r in hk["goals"]] == [int(r["cost"]) for r in got["goals"]]
        for a, b in zip(hk["paths"], got["paths"]):
            assert np.array_equal(a + off, b), tag
    return got


# ---- 1. small pyramid, all classes -------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("site_mask", [2, 3])
@pytest.mark.parametrize("c", [0, 2])
def test_small_pyramid(hs_mod, small, c, site_mask):
    rep, cls = small
    for level in (0, 1):
        h, w = cls[level].shape
        free = np.argwhere(NV.np_traversable(cls[level], c, site_mask))
        if c == 0:
            assert len(free) > 4
        else:                                                              # (a fifth of the cells is free: a clearance of 2 may leave nothing)
            free = np.concatenate([free, np.argwhere(cls[level] == 2)])
        src = [tuple(int(v) for v in free[len(free) // 2][::-1]), (w + 3, 2), tuple(int(v) for v in free[0][::-1])]
        goals = [(0, 0, w - 1, h - 1), (-4, -4, 6, 6), (w // 2, h // 2, w // 2 + 5, h // 2 + 4), (w - 3, h - 3, w + 5, h + 5), (w + 1, 0, w + 4, 4),
                 tuple(int(v) for v in free[-1][::-1]) * 2]
        got = assert_nav(hs_mod, rep, level, cls[level], (0, 0, w, h), src, c, site_mask, 0, goals, 2, 64, tag=(level, c, site_mask))
        s = got["summary"]
        assert s["n_sources_used"] + s["n_sources_blocked"] == 3 and s["n_sources_blocked"] >= 1 and s["rounds"] >= 1
        if c == 0:
            assert s["n_sources_used"] == 2 and s["n_reached"] >= 2 and tuple(got["goals"][0])[0] == 0 and got["path_cells"][0] == 1


# ---- 2. tile seams -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seam_rep(hs_mod, ctx):
    assert SEAM_W % T and SEAM_W % 32 and SEAM_H % T and SEAM_H % 32
    rep = hs_mod.MapRepMultiMap(0.1, (SEAM_W, SEAM_H), 1, ctx=ctx)
    yield rep
    rep.close()


M_SEAM = (0, 0, SEAM_W, SEAM_H)


@gpu
def test_wave_crosses_every_seam(hs_mod, seam_rep):
    """All free, the source in one corner: the wave crosses every seam and the corners where four tiles meet."""
    c = np.full((SEAM_H, SEAM_W), 2, np.uint8)
    FG.put_classes(hs_mod, seam_rep, 0, c)
    goals = [(SEAM_W - 1, SEAM_H - 1) * 2, (T - 1, T - 1, T, T), (2 * T - 1, 2 * T - 1, 2 * T, 2 * T)]
    got = assert_nav(hs_mod, seam_rep, 0, c, M_SEAM, [(0, 0)], goals=goals, n_paths=3, max_path_cells=512)
    a, b = SEAM_W - 1, SEAM_H - 1
    assert tuple(got["goals"][0]) == (5 * (a - b) + 7 * b, a, b, 1) and got["path_cells"][0] == a + 1
    assert tuple(got["goals"][1]) == (7 * (T - 1), T - 1, T - 1, 4)
    assert got["summary"]["n_reached"] == SEAM_W * SEAM_H and got["summary"]["rounds"] >= 4


@gpu
@pytest.mark.parametrize("blocked", [0, 1])
@pytest.mark.parametrize("row", [T - 1, T, 2 * T - 1, 2 * T])
def test_door_on_a_seam(hs_mod, seam_rep, row, blocked):
    """A wall along column T, the first column of the second tile, with a single door at `row` -- the last row of a tile, the first of
    the next, on the corners where four tiles meet.  blocked: the cell left of the door is occupied, so the door could be entered
    from the left only by a diagonal that would cut the wall's corner: everything right of the wall is unreached."""
    c = np.full((SEAM_H, SEAM_W), 2, np.uint8)
    c[:, T] = 1
    c[row, T] = 2
    if blocked:
        c[row, T - 1] = 1
    FG.put_classes(hs_mod, seam_rep, 0, c)
    goals = [(T + 1, 0, SEAM_W - 1, SEAM_H - 1), (T, row, T, row)]
    got = assert_nav(hs_mod, seam_rep, 0, c, M_SEAM, [(3, 5)], goals=goals, n_paths=1, max_path_cells=400, tag=(row, blocked))
    left = T * SEAM_H
    if blocked:
        assert got["summary"]["n_reached"] == left - 1 and tuple(got["goals"][0]) == (NV.UNREACHED, 0, 0, 0) and got["path_cells"][0] == 0
        assert got["cost"][3 + row, 3 + T] == NV.UNREACHED and got["dir"][3 + row, 3 + T] == 255
    else:
        assert got["summary"]["n_reached"] == SEAM_W * SEAM_H - (SEAM_H - 1)
        a, b = T - 4, abs(row - 5)                                         # to the cell left of the door, then one straight step: no diagonal enters it
        door = 5 * abs(a - b) + 7 * min(a, b) + 5
        assert tuple(got["goals"][1]) == (door, T, row, 1)
        assert tuple(got["goals"][0])[:3] == (door + 5, T + 1, row) and got["goals"][0]["n_reached"] == (SEAM_W - T - 1) * SEAM_H


@gpu
@pytest.mark.parametrize("across", [False, True])
def test_serpentine_over_the_whole_level(hs_mod, seam_rep, across):
    """One-cell corridors over the whole level, and the transpose: the path crosses the seams again and again, every tile is
    re-activated many times, and the only path's length is known in closed form."""
    c = np.ones((SEAM_H, SEAM_W), np.uint8)
    if across:
        w, h = SEAM_H, SEAM_W - 1                                          # (the serpentine needs an odd number of rows)
        c[:, :h] = NV.serpentine(w, h).T
    else:
        w, h = SEAM_W, SEAM_H - 1
        c[:h] = NV.serpentine(w, h)
    far = 0 if ((h - 1) // 2) % 2 else w - 1                               # the last corridor is entered through gap (h - 1) / 2 - 1: at w - 1 if that is even
    end = (h - 1, far) if across else (far, h - 1)
    FG.put_classes(hs_mod, seam_rep, 0, c)
    n = (h + 1) // 2 * w + (h - 1) // 2
    got = assert_nav(hs_mod, seam_rep, 0, c, M_SEAM, [(0, 0)], goals=[end * 2], n_paths=1, max_path_cells=16384, tag=across)
    assert got["path_cells"][0] == n == got["summary"]["n_reached"] and tuple(got["goals"][0]) == (5 * (n - 1),) + end + (1,)
    assert got["summary"]["rounds"] > SEAM_TILES and got["paths"][0].shape == (n, 2)
    cut = seam_rep.nav_field(0, [(0, 0)], max_cost=5 * 1000, goals=[end * 2], n_paths=1)
    assert cut["summary"]["n_reached"] == 1001 and cut["path_cells"][0] == 0 and cut["goals"][0]["cost"] == NV.UNREACHED


@gpu
def test_sources_either_side_of_a_seam(hs_mod, seam_rep):
    rng = np.random.default_rng(23)
    c = rng.choice(np.array([0, 1, 2], np.uint8), size=(SEAM_H, SEAM_W), p=[0.01, 0.03, 0.96])   # (sparse: a clearance of 1 from the unknown too must leave the map connected)
    src = [(T - 1, 5), (T, 70), (3, T - 1), (100, T), (2 * T - 1, 2 * T - 1), (2 * T, 2 * T), (3 * T, 20), (3 * T - 1, 100)]
    for x, y in src:
        c[y, x] = 2
    FG.put_classes(hs_mod, seam_rep, 0, c)
    goals = [(x - 2, y - 2, x + 2, y + 2) for x, y in ((T, T), (2 * T, T), (3 * T, 2 * T), (SEAM_W - 1, SEAM_H - 1))]
    for clearance, mask in ((0, 2), (1, 2), (1, 3)):
        got = assert_nav(hs_mod, seam_rep, 0, c, M_SEAM, src, clearance, mask, goals=goals, n_paths=4, max_path_cells=300, tag=(clearance, mask))
        assert got["summary"]["n_sources_used"] + got["summary"]["n_sources_blocked"] == len(src) and got["summary"]["n_reached"] > SEAM_W * SEAM_H // 2


# ---- 3. max_cost -------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("cells", [20, T // 2 - 1, T // 2, T // 2 + 1])
def test_max_cost_cuts_the_wave(hs_mod, seam_rep, cells):
    """From the middle of the first tile a cap of 5 * cells ends the wave inside the tile, on its last column, on the first column of
    the next tile, and one further."""
    c = np.full((SEAM_H, SEAM_W), 2, np.uint8)
    c[T + 10, :] = 1
    FG.put_classes(hs_mod, seam_rep, 0, c)
    s = T // 2
    got = assert_nav(hs_mod, seam_rep, 0, c, M_SEAM, [(s, s)], max_cost=5 * cells, goals=[(s + cells, s, SEAM_W - 1, s)], tag=cells)
    assert tuple(got["goals"][0]) == (5 * cells, s + cells, s, 1) and got["summary"]["max_cost_reached"] == 5 * cells
    assert got["cost"][3 + s, 3 + s + cells + 1] == NV.UNREACHED
    assert_nav(hs_mod, seam_rep, 0, c, M_SEAM, [(s, s)], max_cost=5 * cells + 4, hook=False, tag=("not a multiple of 5", cells))


# ---- 4. the world ------------------------------------------------------------------------------------------------------------------
def world_nav(hs_mod, rep, level, sources, goals=None, **kw):
    s = rep.nav_field(level, sources, world=True)["summary"]
    m = (int(s["mx0"]), int(s["my0"]), int(s["mw"]), int(s["mh"]))
    W, H = rep.Maps[level].Dimensions
    assert m[0] <= 0 and m[1] <= 0 and m[0] + m[2] >= W and m[1] + m[3] >= H           # R holds the window
    if goals is None:                                                      # the four strips of M outside the window
        goals = [g for g in ((m[0], m[1], -1, m[1] + m[3] - 1), (W, m[1], m[0] + m[2] - 1, m[1] + m[3] - 1), (0, m[1], W - 1, -1),
                             (0, H, W - 1, m[1] + m[3] - 1)) if g[0] <= g[2] and g[1] <= g[3]]
    got = assert_nav(hs_mod, rep, level, FG.world_classes(rep, level, m), m, sources, goals=goals, world=True, tag=("world", level), **kw)
    return m, goals, got


@gpu
@pytest.mark.parametrize("level", [0, 1])
def test_world_variant(hs_mod, ctx, level):
    rng = np.random.default_rng(17)
    rep = hs_mod.MapRepMultiMap(0.1, (80, 48), 2, ctx=ctx)
    rep.set_backing(16, POOL)
    FG.free_fill(hs_mod, rep, rng)
    rep.shift(34, -22)
    FG.free_fill(hs_mod, rep, rng)
    rep.shift(-68, 30)                                                     # part of what was mapped now lies in tiles alone
    ox, oy = rep.origin()
    assert (ox, oy) == (-34, 8) and (ox >> 1) % 2 == 1 and rep.backing_stats()["tiles"] > 3
    W, H = rep.Maps[level].Dimensions
    free = np.argwhere(FG.window_classes(rep, level) == 2)
    src = [tuple(int(v) for v in free[len(free) // 2][::-1])]             # a source in the window
    m, goals, got = world_nav(hs_mod, rep, level, src, n_paths=2, max_path_cells=200, c=0)
    assert m[2] * m[3] > W * H and len(goals) >= 1
    out = [r for r in got["goals"] if r["cost"] != NV.UNREACHED]
    assert out, "no goal outside the window is reached: the construction does not test the world"
    for r in out:                                                          # reached only through evicted cells: the cell lies outside the window
        assert not (0 <= r["bx"] < W and 0 <= r["by"] < H)
    assert max(int(v) for v in got["path_cells"]) > 1
    world_nav(hs_mod, rep, level, src, c=1, site_mask=3)
    win = assert_nav(hs_mod, rep, level, FG.window_classes(rep, level), (0, 0, W, H), src, goals=goals, n_paths=2, max_path_cells=200, tag=("window", level))
    assert all(r["cost"] == NV.UNREACHED and r["n_reached"] == 0 for r in win["goals"]) and list(win["path_cells"]) == [0, 0]
    rep.close()


@gpu
def test_world_is_the_window_without_tiles(hs_mod, small):
    rep, cls = small
    for level in (0, 1):
        h, w = cls[level].shape
        free = np.argwhere(cls[level] == 2)
        src = [tuple(int(v) for v in free[3][::-1])]
        kw = dict(clearance=1, goals=[(0, 0, w - 1, h - 1), (-9, -9, 3, 3)], n_paths=2, max_path_cells=50, rect=(-5, -4, w + 9, h + 11))
        a = rep.nav_field(level, src, world=False, **kw)
        b = rep.nav_field(level, src, world=True, **kw)
        assert tuple(a["summary"])[:9] == tuple(b["summary"])[:9] and tuple(a["summary"])[:4] == (0, 0, w, h)
        assert np.array_equal(a["cost"], b["cost"]) and np.array_equal(a["dir"], b["dir"]) and np.array_equal(a["goals"], b["goals"])
        assert all(np.array_equal(x, y) for x, y in zip(a["paths"], b["paths"]))


@gpu
def test_after_shift(hs_mod, ctx):
    rng = np.random.default_rng(5)
    rep = hs_mod.MapRepMultiMap(0.1, (80, 48), 2, ctx=ctx)
    rep.set_backing(16, POOL)
    FG.free_fill(hs_mod, rep, rng)
    rep.shift(34, -22)
    FG.free_fill(hs_mod, rep, rng)
    rep.shift(-20, 14)
    for l in (0, 1):
        W, H = rep.Maps[l].Dimensions
        free = np.argwhere(FG.window_classes(rep, l) == 2)
        src = [tuple(int(v) for v in free[len(free) // 3][::-1])]
        win = assert_nav(hs_mod, rep, l, FG.window_classes(rep, l), (0, 0, W, H), src, goals=[(0, 0, W - 1, H - 1)], tag=("window after shift", l))
        assert tuple(win["summary"])[:4] == (0, 0, W, H)
        m, goals, got = world_nav(hs_mod, rep, l, src)
        assert got["summary"]["n_reached"] >= win["summary"]["n_reached"]
    rep.close()


# ---- 5. the processor --------------------------------------------------------------------------------------------------------------
@pytest.fixture
def scrolled(hs_mod, sim):
    own = hs_mod.Context(0)
    proc = hs_mod.HectorSLAMProcessor(0.1, (64, 64), (3.0, 3.0, 0.0), 3, ctx=own, scrollTrigger=6)
    for i in range(8):
        true = np.array([3.0 + 0.18 * i, 3.0 + 0.05 * i, 0.04 * i], np.float32)
        proc.Update(hs_mod.ScanCloud(TR.room_scan(sim, true, 120)), true)
    assert proc.get_origin() != (0, 0)                                     # the window has scrolled
    yield proc
    proc.Dispose(); own.close()


@gpu
def test_processor_nav_field_after_a_scroll(hs_mod, scrolled):
    proc = scrolled
    ox, oy = proc.get_origin()
    match, last = proc.MatchPose.copy(), proc.LastMapUpdatePose.copy()
    for level in (0, 1, 2):
        W, H = proc.MapRep.Maps[level].Dimensions
        kx, ky = ox >> level, oy >> level
        k2, k4 = np.array([kx, ky]), np.array([kx, ky, kx, ky])
        px, py = proc.PoseCell(level)
        src_w = np.array([(px, py), (kx - 7, ky + 2)])                     # world cells: the robot's, and one outside the window
        goals_w = np.array([(kx, ky, kx + W - 1, ky + H - 1), (px - 6, py - 6, px - 2, py + 6), (kx - 9, ky - 9, kx - 1, ky + 5)])
        w = proc.NavField(level, src_w, clearance=1, goals=goals_w, n_paths=3, max_path_cells=128, rect=(kx - 2, ky - 1, W + 5, H + 3))
        cls = FG.window_classes(proc.MapRep, level)
        got = assert_nav(hs_mod, proc.MapRep, level, cls, (0, 0, W, H), src_w - k2, 1, goals=goals_w - k4, n_paths=3, max_path_cells=128, grow=0, tag=level)
        win = proc.MapRep.nav_field(level, src_w - k2, 1, goals=goals_w - k4, n_paths=3, max_path_cells=128, rect=(-2, -1, W + 5, H + 3))
        assert np.array_equal(win["cost"][1:1 + H, 2:2 + W], got["cost"])
        assert (w["summary"]["mx0"], w["summary"]["my0"]) == (kx, ky) and tuple(w["summary"])[2:9] == tuple(win["summary"])[2:9]
        assert np.array_equal(w["cost"], win["cost"]) and np.array_equal(w["dir"], win["dir"])
        assert w["summary"]["n_sources_used"] == 1 and w["summary"]["n_sources_blocked"] == 1 and w["summary"]["n_reached"] > 20
        for a, b in zip(w["goals"], win["goals"]):
            assert (a["cost"], a["n_reached"]) == (b["cost"], b["n_reached"])
            assert (a["bx"], a["by"]) == ((b["bx"] + kx, b["by"] + ky) if b["cost"] != NV.UNREACHED else (0, 0))
        assert np.array_equal(w["path_cells"], win["path_cells"]) and w["path_cells"][0] == 1
        for a, b in zip(w["paths"], win["paths"]):
            assert np.array_equal(a, b + k2)
    assert S.same_bits(proc.MatchPose, match) and S.same_bits(proc.LastMapUpdatePose, last) and proc.get_origin() == (ox, oy)


@gpu
def test_explore_goals(hs_mod, scrolled):
    proc = scrolled
    level, clearance, grow = 0, 1, 2
    fr = proc.Frontiers(level, min_cells=2, max_clusters=40)[1]
    rec, res, nav = proc.ExploreGoals(level, clearance, site_mask=2, min_cells=2, max_clusters=40, grow=grow, n_paths=2, max_path_cells=256)
    assert rec.shape[0] == fr.shape[0] >= 1 and np.array_equal(rec, fr[nav["order"]]) and sorted(nav["order"].tolist()) == list(range(fr.shape[0]))
    src = [proc.PoseCell(level)]
    for c, r in zip(rec, res):                                             # every cluster's result is a direct call's with its grown box
        one = proc.NavField(level, src, clearance, goals=[(c["x_min"] - grow, c["y_min"] - grow, c["x_max"] + grow, c["y_max"] + grow)])
        assert tuple(one["goals"][0]) == tuple(r)
    cost = res["cost"].astype(np.int64)
    n_ok = int((cost != NV.UNREACHED).sum())
    assert n_ok >= 1 and (np.diff(cost) >= 0).all() and (cost[n_ok:] == NV.UNREACHED).all()
    order = nav["order"]
    for i in range(len(order) - 1):
        if cost[i] == cost[i + 1]:
            assert order[i] < order[i + 1]                                 # equal costs, and the unreachable ones, keep Frontiers' order
    assert len(nav["paths"]) == 2 and all(tuple(p[-1]) == src[0] for p, g in zip(nav["paths"], nav["goals"]) if g["cost"] != NV.UNREACHED)


# ---- 6. refusals, and no side effects ----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kw", NV.refusal_cases() + [dict(level=-1), dict(level=2), dict(world=2), dict(world=-1)],
                         ids=lambda kw: ",".join("%s=%s" % i for i in kw.items()).replace(" ", ""))
def test_refusals(hs_mod, small, kw):
    capi = hs_mod.capi
    rep, cls = small
    kw = dict(kw)
    spec = capi.nav_spec(kw.pop("level", 0), False, kw.pop("site_mask", 2), kw.pop("clearance", 0), 0)
    spec["world"] = kw.pop("world", 0)
    bufs = NV.refusal_buffers(**{k: v for k, v in kw.items() if k in ("S", "G", "n_paths", "max_path_cells", "inverted")})
    rc = capi.lib().slamhip_hs_nav_field(rep._h, spec.ctypes.data_as(C.c_void_p), *NV.refusal_args(bufs, **kw))
    assert rc == capi.ERR_INVALID and NV.untouched(bufs), kw
    h, w = cls[0].shape
    ok = rep.nav_field(0, [(w // 2, h // 2)], rect=(0, 0, w, h))             # the hs goes on working
    assert tuple(ok["summary"])[:4] == (0, 0, w, h)


@gpu
def test_large_arguments_go_through(hs_mod, small):
    rep, cls = small
    h, w = cls[0].shape
    free = np.argwhere(cls[0] == 2)[:, ::-1]
    src = np.resize(free, (4096, 2))
    goals = np.tile(np.array([(0, 0, w - 1, h - 1)]), (4096, 1))
    got = rep.nav_field(0, src, goals=goals, n_paths=64, max_path_cells=16384, rect=(0, 0, 4096, 4096))
    assert got["summary"]["n_sources_used"] == 4096 and got["cost"].shape == (4096, 4096) and (got["goals"]["cost"] == 0).all()
    assert (got["path_cells"] == 1).all() and (got["cost"][h:] == NV.UNREACHED).all()
    assert np.array_equal(got["cost"][:h, :w], NV.np_nav(cls[0], src, rect=(0, 0, w, h))["cost"])


@gpu
def test_nothing_else_moved(hs_mod, ctx):
    rng = np.random.default_rng(4)
    rep = hs_mod.MapRepMultiMap(0.1, (80, 48), 2, ctx=ctx)
    rep.set_backing(16, POOL)
    TR.fill(hs_mod, rep, rng)
    rep.shift(34, -22)
    TR.fill(hs_mod, rep, rng)
    rep.set_scan(hs_mod.ScanCloud(L.small_points(np.random.default_rng(11), 97)))
    lat = (1, (1.0, 1.0, 0.0), 2, 2, 3, 0.1)

    scan = hs_mod.ScanCloud(L.small_points(np.random.default_rng(11), 97))
    matcher = hs_mod.ScanMatcher()
    idx = np.arange(0, 40 * 24, 7)

    def state():
        k, v = rep.world_lattice_search(None, *lat, scores=True)
        return ([rep.Maps[l].checksum() for l in range(2)], rep.distance_field(1, (-3, -3, 50, 40), site_mask=3, radius=9, world=True), k, v,
                [rep.Maps[l].GetCells().copy() for l in range(2)], [rep.Maps[l].GetCachedProbability(idx) for l in range(2)],
                rep.frontiers(1, 1, 64, world=True, labels_rect=(-8, -8, 100, 70)), matcher.MatchData(rep, scan, (1.0, 1.0, 0.0)))

    def calls():
        return [rep.nav_field(l, [(20, 12), (5, 5)], c, 2 + (c > 0), world=bool(wd), goals=[(0, 0, 30, 30)], n_paths=1, max_path_cells=64, rect=(-8, -8, 100, 70))
                for l in (0, 1) for wd in (0, 1) for c in (0, 2)]
    a = state()
    first = calls()
    b = state()
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    assert all(S.raw(x).tobytes() == S.raw(y).tobytes() for x, y in zip(a[4], b[4]))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[5], b[5])) and S.same_bits(a[7], b[7])
    FG.FR.check(a[6], b[6])
    for x, y in zip(first, calls()):                                       # ... and the call repeats itself
        assert tuple(x["summary"])[:9] == tuple(y["summary"])[:9] and np.array_equal(x["cost"], y["cost"]) and np.array_equal(x["dir"], y["dir"])
        assert np.array_equal(x["goals"], y["goals"]) and np.array_equal(x["paths"][0], y["paths"][0])
    rep.set_reference_cache(1)                                             # cell values only: the reference's cache plays no part
    for x, y in zip(first, calls()):
        assert np.array_equal(x["cost"], y["cost"]) and np.array_equal(x["dir"], y["dir"])
    rep.close()


@gpu
def test_poisoned_context_refuses(hs_mod):
    """A context poisoned by a blocking wait that timed out (the trace of tests/test_gpu_hector_trace.py: 1 ms against 4096 poses x
    1024 long beams) refuses the call at once with SLAMHIP_ERR_TIMEOUT, nothing launched."""
    import time
    capi = hs_mod.capi
    own = hs_mod.Context(0)
    rep = hs_mod.MapRepMultiMap(0.05, (1024, 1024), 1, ctx=own)
    try:
        a = np.linspace(-math.pi, math.pi, 1024, endpoint=False)
        rep.set_scan(hs_mod.ScanCloud(np.stack([25.0 * np.cos(a), 25.0 * np.sin(a)], 1).astype(np.float32)))
        poses = np.tile(np.array([25.6, 25.6, 0.0], np.float32), (4096, 1))
        rep.trace(poses[:2], 0)
        s = rep.nav_field(0, [(5, 5)])["summary"]                          # nothing mapped yet: nothing is free
        assert (s["n_traversable"], s["n_reached"], s["n_sources_blocked"], s["rounds"]) == (0, 0, 1, 1)
        own.set_wait_timeout(1)
        with pytest.raises(capi.SlamhipError) as e:
            rep.trace(poses, 0)
        assert e.value.code == capi.ERR_TIMEOUT and own.poisoned
        t0 = time.perf_counter()
        with pytest.raises(capi.SlamhipError) as e1:
            rep.nav_field(0, [(5, 5)])
        assert e1.value.code == capi.ERR_TIMEOUT and time.perf_counter() - t0 < 0.05
    finally:
        rep.close(); own.close()                                           # (destroy waits for the queue to drain: no bound there)
