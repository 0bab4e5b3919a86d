"""The command rollouts (slamhip_hs_rollouts, slamhip_hsproc_rollouts) on the device, against the restatement of the definition in
tests/test_hs_rollout_abi.py (np.float32 operations one by one, np.rint, np_oracle.det_sincos, the field from test_hs_nav_abi's
restatement) and against the hook, both fed from cells_download / world_cells_download.  Everything is compared with == on integers
and on the bit patterns of the floats; there is no tolerance anywhere.

Shapes are those of tests/test_gpu_hector_nav.py, whose fixtures are imported: the 80 x 48 x 2 pyramid, the (3 T + 16) x (2 T + 8)
seam level and the odd-origin window over 16-cell backing tiles.  P runs over both sides of every sub-group width (1, 2, 4, 32, 64
lanes), B over both sides of a wavefront's and a workgroup's worth of rollouts.  The product's form is a lane per rollout; the two
developer experiments that stay in the library behind environment switches -- a sub-group of lanes per rollout, the traversable
words of a square around the start staged in LDS -- must give the same bytes, and are run at every width, with rollouts that
leave the square and with a start outside M."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_hector_frontier as FG
import test_gpu_hector_nav as GN
import test_gpu_hector_shift as S
import test_hs_nav_abi as NV
import test_hs_rollout_abi as RO
from test_gpu_hector_frontier import small                                 # noqa: F401 (fixture)
from test_gpu_hector_nav import scrolled, seam_rep                         # noqa: F401 (fixtures)
from test_gpu_hector_shift import hs_mod, ctx                              # noqa: F401 (fixtures)

gpu = pytest.mark.gpu
F = np.float32
T = GN.T
SEAM_W, SEAM_H = GN.SEAM_W, GN.SEAM_H


def stm_of(rep, level):
    return F(1.0) / F(rep.Maps[level].CellLength)


def assert_rollouts(hs_mod, rep, level, cls, m, sources, start, dt, body, cmds, hold=1, c=0, site_mask=2, world=False, tag=None):
    """One call against the restatement over cls (the classes of M = m), and, where M starts at the window's first cell, against the
    hook on the same classes.  -> (the call's result, the restatement's)."""
    stm = stm_of(rep, level)
    got = rep.rollouts(level, sources, start, dt, cmds, hold, body, c, site_mask, 0, world)
    cost, trav, nav = RO.np_field(cls, sources, c, site_mask, 0, m[0], m[1])
    want = RO.np_rollouts(cost, trav, (m[0], m[1]), stm, start, dt, body, cmds, hold)
    RO.check(got, want, nav, tag)
    assert got[1]["nav"]["rounds"] >= 1
    if (m[0], m[1]) == (0, 0):
        hk = hs_mod.capi.debug_rollouts(cls, sources, stm, start, dt, body, cmds, hold, site_mask, c, 0)
        assert hk[0].tobytes() == got[0].tobytes(), tag
        assert hk[1].tobytes()[40:] == got[1].tobytes()[40:] and tuple(hk[1]["nav"])[:9] == tuple(got[1]["nav"])[:9], tag
    return got, want


def fan(B, n_cmd, cell, seed=5, v_cells=1.5):
    """B sequences of n_cmd pairs: up to v_cells cells per unit dt forwards, a little backwards, |w| <= 0.5; command 1 stands still."""
    rng = np.random.default_rng([seed, B, n_cmd])
    out = np.stack([rng.uniform(-0.2, 1.0, (B, n_cmd)) * float(cell) * v_cells, rng.uniform(-0.5, 0.5, (B, n_cmd))], 2).astype(F)
    if B > 1:
        out[1] = 0.0
    return out


def at_cell(cell, x, y, th=0.0):
    return (F(x * float(cell)), F(y * float(cell)), F(th))


# ---- 1. small pyramid, all classes -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_open(hs_mod, ctx, small):
    """The small pyramid's classes (a fifth free, in specks: a clearance of 2 leaves next to nothing) with an open block of 15 x 15
    cells planted in the middle of either level, so that rollouts under a clearance have somewhere to go."""
    rep = hs_mod.MapRepMultiMap(0.1, (80, 48), 2, ctx=ctx)
    cls = []
    for l, c in enumerate(small[1]):
        c = c.copy()
        h, w = c.shape
        c[h // 2 - 7:h // 2 + 8, w // 2 - 7:w // 2 + 8] = 2
        FG.put_classes(hs_mod, rep, l, c)
        assert np.array_equal(FG.window_classes(rep, l), c)
        c.setflags(write=False)
        cls.append(c)
    yield rep, cls
    rep.close()


@gpu
@pytest.mark.parametrize("c", [0, 2])
def test_small_pyramid(hs_mod, small_open, c):
    rep, cls = small_open
    for level in (0, 1):
        h, w = cls[level].shape
        cell = F(rep.Maps[level].CellLength)
        free = np.argwhere(NV.np_traversable(cls[level], c, 2))
        sx, sy = w // 2, h // 2                                            # the middle of the open block: traversable under a clearance of 2
        assert NV.np_traversable(cls[level], c, 2)[sy, sx]
        src = [(sx, sy), (w + 3, 2), tuple(int(v) for v in free[0][::-1])]
        for P, hold in ((0, 1), (3, 3)):
            got, want = assert_rollouts(hs_mod, rep, level, cls[level], (0, 0, w, h), src, at_cell(cell, sx, sy, 0.7), 1.0,
                                        RO.body_points(P, 0.6 * float(cell)), fan(65, 4, cell), hold, c, tag=(level, c, P, hold))
            n_free = got[0]["n_free"]
            assert got[1]["start_cost"] == 0 and n_free[1] == 4 * hold + 1 and got[1]["n_complete"] >= 1
            assert (n_free > 1).sum() > 30, n_free                         # not an all-blocked case, under the clearance either
            if hold == 3:
                assert len(set(n_free.tolist())) >= 3 and got[1]["n_complete"] < 65, n_free       # ... and the block's edge cuts some


# ---- 2. the seam level: P, B, hold, T ----------------------------------------------------------------------------------------------
M_SEAM = (0, 0, SEAM_W, SEAM_H)
MID = (SEAM_W // 2, SEAM_H // 2)
SEAM_SRC = (MID[0] + 4, MID[1] - 3)


@pytest.fixture(scope="module")
def seam_random():
    """Sparse obstacles and a little unknown, an open block around the middle that holds the start and the source, and a wall eight
    columns ahead of the start: beyond it nothing is reached, so a rollout that drives on is cut."""
    rng = np.random.default_rng(23)
    c = rng.choice(np.array([0, 1, 2], np.uint8), size=(SEAM_H, SEAM_W), p=[0.01, 0.03, 0.96])
    c[MID[1] - 5:MID[1] + 6, MID[0] - 5:MID[0] + 6] = 2
    c[:, MID[0] + 8] = 1
    c.setflags(write=False)
    return c


def seam_case(hs_mod, seam_rep, cls, P, B, hold, n_cmd=6, tag=None):
    FG.put_classes(hs_mod, seam_rep, 0, cls)
    cell = F(seam_rep.Maps[0].CellLength)
    return assert_rollouts(hs_mod, seam_rep, 0, cls, M_SEAM, [SEAM_SRC], at_cell(cell, MID[0], MID[1], 0.4), 1.0,
                           RO.body_points(P, 3.0 * float(cell)), fan(B, n_cmd, cell), hold, tag=tag)


@gpu
@pytest.mark.parametrize("hold", [1, 3])
@pytest.mark.parametrize("P", [0, 1, 3, 31, 32])
def test_body_points_either_side_of_a_subgroup(hs_mod, seam_rep, seam_random, P, hold):
    got, want = seam_case(hs_mod, seam_rep, seam_random, P, 65, hold, tag=(P, hold))
    n_free = got[0]["n_free"]
    assert (n_free >= 1).all() and n_free.max() == 6 * hold + 1
    if hold == 3:
        assert n_free.min() < 6 * hold + 1                                 # 18 steps of up to 1.5 cells: some reach the wall


@gpu
@pytest.mark.parametrize("hold", [1, 3])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 1025])
def test_rollouts_either_side_of_a_wavefront_and_a_workgroup(hs_mod, seam_rep, seam_random, B, hold):
    got, want = seam_case(hs_mod, seam_rep, seam_random, 3, B, hold, n_cmd=3, tag=(B, hold))
    assert got[0].shape == (B,) and got[1]["n_complete"] == sum(r[0] == 3 * hold + 1 for r in want[0])


# ---- 2b. the developer experiments behind their switches give the same bytes ------------------------------------------------------
@gpu
@pytest.mark.parametrize("lds", [0, 1])
@pytest.mark.parametrize("sg", [0, 1, 2, 4, 8, 16, 32, 64])
def test_experiment_switches_change_nothing(hs_mod, seam_rep, seam_random, monkeypatch, sg, lds):
    """SLAMHIP_ROLLOUT_SG (lanes per rollout; 0: a lane per item) and SLAMHIP_ROLLOUT_LDS (the staged square) against the
    restatement, with P on both sides of the width."""
    monkeypatch.setenv("SLAMHIP_ROLLOUT_SG", str(sg))
    monkeypatch.setenv("SLAMHIP_ROLLOUT_LDS", str(lds))
    for P in sorted({min(max(v, 0), 32) for v in (0, sg - 2, sg - 1, sg, 3, 32)}):      # P + 1 = sg - 1, sg, sg + 1
        seam_case(hs_mod, seam_rep, seam_random, P, 65, 2, n_cmd=3, tag=(sg, lds, P))


@gpu
@pytest.mark.parametrize("sg", [0, 1])
def test_staged_square_left_and_a_start_outside_the_map(hs_mod, seam_rep, monkeypatch, sg):
    """All free.  From (10, 68) the staged square covers columns -128 .. 127 (its first column rounded down to a word) and rows
    -60 .. 195: a drive along +x with a body of three cells' reach leaves it through its right edge at column 128 and goes on over
    global memory to the level's last column; one along -x leaves M inside the square.  A start outside M, and one far outside."""
    c = np.full((SEAM_H, SEAM_W), 2, np.uint8)
    FG.put_classes(hs_mod, seam_rep, 0, c)
    cell = F(seam_rep.Maps[0].CellLength)
    cmds = np.zeros((4, 210, 2), F)
    cmds[0, :, 0] = float(cell); cmds[1, :, 0] = -float(cell)
    cmds[2, :, 0] = float(cell); cmds[2, :, 1] = 0.004                     # a slow turn downwards: leaves the square, then M through the last row
    cmds[3, :100, 0] = float(cell)                                         # into the part beyond the square, and stays
    body = RO.body_points(5, 3.0 * float(cell))
    monkeypatch.setenv("SLAMHIP_ROLLOUT_SG", str(sg))
    out = {}
    for lds in (0, 1):
        monkeypatch.setenv("SLAMHIP_ROLLOUT_LDS", str(lds))
        got, _ = assert_rollouts(hs_mod, seam_rep, 0, c, M_SEAM, [(SEAM_W - 5, 68)], at_cell(cell, 10, 68), 1.0, body, cmds, 1, tag=("leaves", sg, lds))
        n = got[0]["n_free"]
        assert 190 < n[0] < 211 and n[1] < 12 and n[3] == 211 and float(got[0]["x"][3]) * float(stm_of(seam_rep, 0)) > 105
        out[lds] = got
        for start in (at_cell(cell, -3, 68), at_cell(cell, SEAM_W + 400, -900), at_cell(cell, 10, SEAM_H + 2, -1.0)):
            g, _ = assert_rollouts(hs_mod, seam_rep, 0, c, M_SEAM, [(SEAM_W - 5, 68)], start, 1.0, body, cmds, 1, tag=("outside", sg, lds))
            assert (g[0]["n_free"] == 0).all() and g[1]["start_cost"] == NV.UNREACHED
    assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1].tobytes()[40:] == out[1][1].tobytes()[40:]


@gpu
def test_one_step_and_1024_steps(hs_mod, seam_rep):
    c = np.full((SEAM_H, SEAM_W), 2, np.uint8)
    FG.put_classes(hs_mod, seam_rep, 0, c)
    cell = F(seam_rep.Maps[0].CellLength)
    start = at_cell(cell, MID[0], MID[1] - 30, 0.0)
    one = np.array([[[float(cell), 0.0]], [[0.0, 0.3]], [[400.0 * float(cell), 0.0]]], F)
    got, _ = assert_rollouts(hs_mod, seam_rep, 0, c, M_SEAM, [MID], start, 1.0, RO.body_points(1, 0.2), one, 1, tag="T = 1")
    assert list(got[0]["n_free"]) == [2, 2, 1] and got[1]["n_complete"] == 2
    # 1024 steps of half a cell on a circle of 25 cells' radius (three laps) around the middle; a straight drive that leaves M
    long = np.zeros((3, 256, 2), F)
    long[:, :, 0] = 0.5 * float(cell)
    long[0, :, 1] = 0.02; long[2, :, 1] = 0.02
    long[2, 200:, 1] = -0.5
    got, _ = assert_rollouts(hs_mod, seam_rep, 0, c, M_SEAM, [MID], start, 1.0, RO.body_points(3, 0.3), long, 4, tag="T = 1024")
    assert got[0]["n_free"][0] == 1025 and 100 < got[0]["n_free"][1] < 1025 and got[1]["n_complete"] >= 1


@gpu
def test_rollout_crosses_every_tile_seam(hs_mod, seam_rep):
    """All free, the goal in the far corner: a diagonal drive of 480 half-cell steps from (2, 2) crosses the seams at x = T, 2 T, 3 T and
    y = T, 2 T; the cost at its end and the least cost along it come from tiles the wave reached across every seam."""
    c = np.full((SEAM_H, SEAM_W), 2, np.uint8)
    FG.put_classes(hs_mod, seam_rep, 0, c)
    cell = F(seam_rep.Maps[0].CellLength)
    th = float(np.arctan2(SEAM_H - 6.0, SEAM_W - 6.0))
    cmds = np.zeros((2, 240, 2), F)
    cmds[:, :, 0] = 0.5 * float(cell)
    cmds[1, 120:, 0] = 0.0                                                 # stops half-way
    got, want = assert_rollouts(hs_mod, seam_rep, 0, c, M_SEAM, [(SEAM_W - 1, SEAM_H - 1)], at_cell(cell, 2, 2, th), 1.0, RO.body_points(3, 0.25), cmds, 2)
    r = got[0]
    assert list(r["n_free"]) == [481, 481] and r["min_cost"][0] == r["end_cost"][0] < r["end_cost"][1] < got[1]["start_cost"]
    assert float(r["x"][0]) * float(stm_of(seam_rep, 0)) > 3 * T and float(r["y"][0]) * float(stm_of(seam_rep, 0)) > 2 * T
    assert hs_mod.capi.rollout_key(got[1]["key_end"]) == (int(r["end_cost"][0]), 0)


# ---- 3. the world ------------------------------------------------------------------------------------------------------------------
def all_free(hs_mod, rep):
    for l, m in enumerate(rep.Maps):
        w, h = m.Dimensions
        FG.put_classes(hs_mod, rep, l, np.full((h, w), 2, np.uint8))


def shifted_rep(hs_mod, ctx, back):
    rep = hs_mod.MapRepMultiMap(0.1, (80, 48), 2, ctx=ctx)
    rep.set_backing(16, GN.POOL)
    all_free(hs_mod, rep)
    rep.shift(34, -22)
    all_free(hs_mod, rep)
    rep.shift(*back)
    return rep


@gpu
@pytest.mark.parametrize("level", [0, 1])
def test_world_variant(hs_mod, ctx, level):
    """Two all-free windows' worth of map, the window then moved so that part of it lies in tiles alone (odd level-1 origin): a
    drive along +x leaves the window onto a backing tile -- free there with world = 1, cut at the window's edge with world = 0."""
    rep = shifted_rep(hs_mod, ctx, (-68, 30))
    ox, oy = rep.origin()
    assert (ox, oy) == (-34, 8) and (ox >> 1) % 2 == 1 and rep.backing_stats()["tiles"] > 3
    W, H = rep.Maps[level].Dimensions
    cell = F(rep.Maps[level].CellLength)
    sx, sy = W - 6, (12 >> level)                                          # world row 20: free in both earlier windows
    src = [(sx - 3, sy)]
    cmds = np.zeros((2, 20, 2), F)
    cmds[:, :, 0] = float(cell)
    cmds[1, :, 1] = 0.01
    body = RO.body_points(3, 1.2 * float(cell))
    s = rep.nav_field(level, src, world=True)["summary"]
    m = (int(s["mx0"]), int(s["my0"]), int(s["mw"]), int(s["mh"]))
    assert m[2] * m[3] > W * H
    start = at_cell(cell, sx, sy)
    out, _ = assert_rollouts(hs_mod, rep, level, FG.world_classes(rep, level, m), m, src, start, 1.0, body, cmds, 1, world=True, tag=("world", level))
    win, _ = assert_rollouts(hs_mod, rep, level, FG.window_classes(rep, level), (0, 0, W, H), src, start, 1.0, body, cmds, 1, tag=("window", level))
    assert tuple(out[1]["nav"])[:4] == m and tuple(win[1]["nav"])[:4] == (0, 0, W, H)
    assert out[0]["n_free"][0] == 21 and float(out[0]["x"][0]) > float(cell) * W       # complete: it ends outside the window
    assert win[0]["n_free"][0] <= 6 and win[1]["n_complete"] == 0                       # cut where the body reaches the window's edge
    rep.close()


@gpu
def test_after_shift_with_the_reference_cache_on(hs_mod, ctx):
    rng = np.random.default_rng(5)
    rep = hs_mod.MapRepMultiMap(0.1, (80, 48), 2, ctx=ctx)
    rep.set_backing(16, GN.POOL)
    FG.free_fill(hs_mod, rep, rng)
    rep.shift(34, -22)
    FG.free_fill(hs_mod, rep, rng)
    rep.shift(-20, 14)
    rep.set_reference_cache(1)                                             # cell values only: the reference's cache plays no part
    for l in (0, 1):
        W, H = rep.Maps[l].Dimensions
        cell = F(rep.Maps[l].CellLength)
        cls = FG.window_classes(rep, l)
        free = np.argwhere(cls == 2)
        sx, sy = (int(v) for v in free[len(free) // 3][::-1])
        got, _ = assert_rollouts(hs_mod, rep, l, cls, (0, 0, W, H), [(sx, sy)], at_cell(cell, sx, sy, -0.3), 1.0, RO.body_points(1, 0.5 * float(cell)),
                                 fan(65, 4, cell), 2, tag=("after shift", l))
        assert got[1]["start_cost"] == 0
        s = rep.nav_field(l, [(sx, sy)], world=True)["summary"]
        m = (int(s["mx0"]), int(s["my0"]), int(s["mw"]), int(s["mh"]))
        assert_rollouts(hs_mod, rep, l, FG.world_classes(rep, l, m), m, [(sx, sy)], at_cell(cell, sx, sy, -0.3), 1.0, None, fan(65, 4, cell), 2, world=True,
                        tag=("world after shift", l))
    rep.close()


# ---- 4. the processor --------------------------------------------------------------------------------------------------------------
@gpu
def test_processor_rollouts_after_a_scroll(hs_mod, scrolled):
    proc = scrolled
    ox, oy = proc.get_origin()
    match, last = proc.MatchPose.copy(), proc.LastMapUpdatePose.copy()
    cell0 = F(proc.MapRep.Maps[0].CellLength)
    off = (F(ox) * cell0, F(oy) * cell0)
    for level in (0, 1):
        cell = F(proc.MapRep.Maps[level].CellLength)
        kx, ky = ox >> level, oy >> level
        px, py = proc.PoseCell(level)
        src_w = np.array([(px, py), (kx - 7, ky + 2)])
        pose_w = np.array([match[0], match[1], 0.5], F)
        pose_win = (F(pose_w[0] - off[0]), F(pose_w[1] - off[1]), pose_w[2])
        cmds = fan(65, 3, cell, v_cells=1.0)
        body = RO.body_points(3, 1.5 * float(cell))
        w_res, w_sm = proc.Rollouts(level, src_w, 1.0, cmds, 2, body, start_pose=pose_w, clearance=1)
        r, sm = proc.MapRep.rollouts(level, src_w - np.array([kx, ky]), pose_win, 1.0, cmds, 2, body, clearance=1)
        for f in ("n_free", "min_step", "end_cost", "min_cost", "theta"):
            assert w_res[f].tobytes() == r[f].tobytes(), (level, f)
        assert w_res["x"].tobytes() == (r["x"] + off[0]).astype(F).tobytes() and w_res["y"].tobytes() == (r["y"] + off[1]).astype(F).tobytes()
        assert (w_sm["nav"]["mx0"], w_sm["nav"]["my0"]) == (kx, ky) and tuple(w_sm["nav"])[2:9] == tuple(sm["nav"])[2:9]
        assert w_sm.tobytes()[40:] == sm.tobytes()[40:]
        assert w_sm["nav"]["n_sources_used"] == 1 and w_sm["nav"]["n_sources_blocked"] == 1 and (r["n_free"] >= 1).any()
        W, H = proc.MapRep.Maps[level].Dimensions                          # ... and the window call is the restatement's
        assert_rollouts(hs_mod, proc.MapRep, level, FG.window_classes(proc.MapRep, level), (0, 0, W, H), src_w - np.array([kx, ky]), pose_win, 1.0, body,
                        cmds, 2, 1, tag=("processor", level))
        d_res, d_sm = proc.Rollouts(level, src_w, 1.0, cmds, 2, body, clearance=1)          # start_pose None: MatchPose
        assert d_res.shape == (65,) and tuple(d_sm["nav"])[:9] == tuple(w_sm["nav"])[:9]
    assert S.same_bits(proc.MatchPose, match) and S.same_bits(proc.LastMapUpdatePose, last) and proc.get_origin() == (ox, oy)


@gpu
def test_drive_command(hs_mod, scrolled):
    proc = scrolled
    level, clearance, steps = 0, 1, 8
    cell = float(F(proc.MapRep.Maps[level].CellLength))
    px, py = proc.PoseCell(level)
    v_values = [0.0, 0.5 * cell, 1.0 * cell, 40.0 * cell]
    w_values = [-0.3, -0.1, 0.0, 0.1, 0.3]
    body = RO.body_points(3, 1.5 * cell)
    near = proc.NavField(level, [(px, py)], clearance, rect=(px - 8, py - 8, 17, 17))["cost"]
    reached = np.argwhere(near != NV.UNREACHED)                            # cells the robot's cell reaches: as goals they reach the robot
    assert len(reached) > 20
    first, far = ((int(px - 8 + x), int(py - 8 + y)) for y, x in (reached[0], reached[-1]))
    for goal in ([first], [far], [(px, py)]):
        v, w, which, rec, sm = proc.DriveCommand(level, goal, clearance, v_values, w_values, 1.0, steps, body)
        cmds = np.array([[(a, b)] for a in v_values for b in w_values], F)
        res, sm2 = proc.Rollouts(level, goal, 1.0, cmds, steps, body, clearance=clearance)
        assert sm.tobytes() == sm2.tobytes()
        done = np.flatnonzero(res["n_free"] == steps + 1)
        some = np.flatnonzero(res["n_free"] >= 1)
        assert len(some) >= 1 and len(some) > len(done)                     # the 40-cell commands do not complete
        if len(done):
            b = int(done[np.lexsort((done, res["end_cost"][done]))[0]]); want = "end"
        else:
            b = int(some[np.lexsort((some, res["min_cost"][some]))[0]]); want = "min"
        assert which == want and (F(v), F(w)) == (cmds[b, 0, 0], cmds[b, 0, 1]) and rec.tobytes() == res[b].tobytes()
    assert which == "end" and rec["end_cost"] == 0 and v == 0.0             # the goal under the robot: stand still (the lowest b of cost 0)


# ---- 5. repeatability, no side effects, refusals -----------------------------------------------------------------------------------
@gpu
def test_identical_calls_and_an_unchanged_nav_field(hs_mod, small):
    rep, cls = small
    h, w = cls[0].shape
    cell = F(rep.Maps[0].CellLength)
    free = np.argwhere(cls[0] == 2)
    sx, sy = (int(v) for v in free[len(free) // 2][::-1])
    kw = dict(clearance=1, goals=[(0, 0, w - 1, h - 1), (-9, -9, 3, 3)], n_paths=2, max_path_cells=50, rect=(-5, -4, w + 9, h + 11))
    before = rep.nav_field(0, [(sx, sy)], **kw)
    sums = [rep.Maps[l].checksum() for l in range(2)]
    args = (0, [(sx, sy)], at_cell(cell, sx, sy, 0.2), 1.0, fan(1025, 4, cell), 2, RO.body_points(1, 0.03))
    a = rep.rollouts(*args)
    b = rep.rollouts(*args)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    after = rep.nav_field(0, [(sx, sy)], **kw)
    assert before["summary"].tobytes() == after["summary"].tobytes() and before["goals"].tobytes() == after["goals"].tobytes()
    assert np.array_equal(before["cost"], after["cost"]) and np.array_equal(before["dir"], after["dir"])
    assert all(np.array_equal(x, y) for x, y in zip(before["paths"], after["paths"]))
    assert sums == [rep.Maps[l].checksum() for l in range(2)]


@gpu
@pytest.mark.parametrize("kw", RO.refusal_cases() + [dict(level=-1), dict(level=2), dict(world=2), dict(world=-1)],
                         ids=lambda kw: ",".join("%s=%s" % i for i in kw.items()).replace(" ", ""))
def test_refusals(hs_mod, small, kw):
    capi = hs_mod.capi
    rep, cls = small
    kw = dict(kw)
    spec = capi.nav_spec(kw.pop("level", 0), False, kw.pop("site_mask", 2), kw.pop("clearance", 0), 0)
    spec["world"] = kw.pop("world", 0)
    bufs = RO.refusal_buffers(**{k: v for k, v in kw.items() if k in ("start", "bad_body", "P")})
    head, tail = RO.refusal_args(bufs, **kw)
    rc = capi.lib().slamhip_hs_rollouts(rep._h, spec.ctypes.data_as(C.c_void_p), *head, *tail)
    assert rc == capi.ERR_INVALID and RO.untouched(bufs), kw
    h, w = cls[0].shape
    ok = rep.rollouts(0, [(w // 2, h // 2)], (1.0, 1.0, 0.0), 1.0, np.zeros((1, 1, 2), F))    # the hs goes on working
    assert tuple(ok[1]["nav"])[:4] == (0, 0, w, h)
