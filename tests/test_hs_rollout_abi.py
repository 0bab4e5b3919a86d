"""CPU-side checks of the command rollouts' interface (slamhip_hs_rollouts, slamhip_hsproc_rollouts, slamhip_debug_rollouts) and the
restatement of their definition (include/slamhip.h, slamhip_hs_rollouts, steps 2 - 6) that tests/test_gpu_hector_rollout.py compares
the device with.

The restatement: np.float32 operations one by one, np.rint for the cells, oracle/np_oracle.det_sincos for the trigonometry, and
the field -- costs and traversable cells as plain 2-D arrays -- from test_hs_nav_abi's restatement.  It shares nothing with
hs_rollout.h, whose text the hook and the kernel run.  Every comparison is == on integers and on the bit patterns of the floats."""
import ctypes as C
import os
import re

import np_oracle
import numpy as np
import pytest

import test_hs_nav_abi as NV

ROOT = NV.ROOT

F = np.float32
UNREACHED = NV.UNREACHED
NO_KEY = 0xFFFFFFFFFFFFFFFF
SYMBOLS = ("slamhip_hs_rollouts", "slamhip_hsproc_rollouts", "slamhip_debug_rollouts")
RESULT_FIELDS = ["n_free", "min_step", "end_cost", "min_cost", "x", "y", "theta"]
CELL = F(0.125)                                                            # cell length of the closed forms: v * dt = one cell is exact
STM = F(1.0) / CELL


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def np_field(cls, sources, c=0, site_mask=2, max_cost=0, x0=0, y0=0):
    """Steps 1 - 4 of slamhip_hs_nav_field over cls, the classes of M whose first cell is (x0, y0): (cost, traversable, summary)."""
    h, w = cls.shape
    nav = NV.np_nav(cls, sources, c, site_mask, max_cost, x0=x0, y0=y0, rect=(x0, y0, w, h))
    return nav["cost"], NV.np_traversable(cls, c, site_mask), nav["summary"]


def np_cell(m, stm):
    """Step 3 for one coordinate: the cell, or None."""
    with np.errstate(all="ignore"):
        f = F(m) * F(stm)
    if not (np.abs(f) < F(16777216.0)):                                    # a NaN fails
        return None
    return int(np.rint(f))


def np_sincos(th):
    with np.errstate(all="ignore"):
        if not (np.abs(F(th)) <= F(65536.0)):                              # outside the deterministic contract: not finite in these tests
            return F(np.sin(F(th))), F(np.cos(F(th)))
        s, c = np_oracle.det_sincos(np.array([th], F))
    return F(s[0]), F(c[0])


def np_rollouts(cost, trav, m0, stm, start, dt, body, cmds, hold):
    """Steps 2 - 6 over the field (cost, trav) of M whose first cell is m0 = (x0, y0) -> (records as a list of tuples in RESULT_FIELDS'
    order with the floats as np.float32, dict(start_cost, n_complete, key_end, key_min))."""
    h, w = cost.shape
    cmds = np.asarray(cmds, F)
    B, n_cmd = cmds.shape[:2]
    T = n_cmd * hold
    dt = F(dt)
    body = np.asarray(body if body is not None else np.zeros((0, 2)), F).reshape(-1, 2)

    def at(mx, my):
        cx, cy = np_cell(mx, stm), np_cell(my, stm)
        if cx is None or cy is None:
            return None
        x, y = cx - m0[0], cy - m0[1]
        return (x, y) if 0 <= x < w and 0 <= y < h else None

    def centre_cost(p):
        q = at(p[0], p[1])
        return int(cost[q[1], q[0]]) if q else UNREACHED

    out = []
    key_end = key_min = NO_KEY
    n_complete = 0
    with np.errstate(all="ignore"):
        for b in range(B):
            x, y, th = F(start[0]), F(start[1]), F(start[2])
            rec = [0, -1, UNREACHED, UNREACHED, x, y, th]
            for i in range(T + 1):
                s, c = np_sincos(th)
                k = centre_cost((x, y))
                ok = k != UNREACHED
                for bx, by in body:
                    if not ok:
                        break
                    wx = F(F(F(c * bx) - F(s * by)) + x)
                    wy = F(F(F(s * bx) + F(c * by)) + y)
                    q = at(wx, wy)
                    ok = bool(q is not None and trav[q[1], q[0]])
                if not ok:
                    break
                rec[0] = i + 1
                if k < rec[3]:
                    rec[3], rec[1] = k, i
                rec[2] = k
                rec[4:] = [x, y, th]
                if i < T:
                    v, wv = cmds[b, i // hold]
                    d = F(v * dt)
                    x, y, th = F(x + F(d * c)), F(y + F(d * s)), F(th + F(wv * dt))
            out.append(tuple(rec))
            if rec[0] == T + 1:
                n_complete += 1
                key_end = min(key_end, (rec[2] << 32) | b)
            if rec[0] >= 1:
                key_min = min(key_min, (rec[3] << 32) | b)
    return out, dict(start_cost=centre_cost(start), n_complete=n_complete, key_end=key_end, key_min=key_min)


def bits(v):
    return int(np.array(v, F).view(np.uint32))


def check(got, want, nav=None, tag=None):
    """(results, summary) of capi.rollouts_call against np_rollouts' pair (and the field's summary dict)."""
    res, summary = got
    recs, sm = want
    assert res.shape[0] == len(recs), tag
    for b, (g, r) in enumerate(zip(res, recs)):
        assert tuple(int(g[f]) for f in RESULT_FIELDS[:4]) == r[:4], (tag, b, g, r)
        assert tuple(bits(g[f]) for f in RESULT_FIELDS[4:]) == tuple(bits(v) for v in r[4:]), (tag, b, g, r)
    for f in ("start_cost", "n_complete", "key_end", "key_min"):
        assert int(summary[f]) == sm[f], (tag, f, summary, sm)
    if nav is not None:
        for f in NV.SUMMARY_FIELDS:
            assert int(summary["nav"][f]) == nav[f], (tag, f, summary["nav"], nav)


def fan(B, n_cmd, seed, v_cell=1.0):
    """B command sequences of n_cmd pairs: |v| up to about v_cell cells per unit dt at CELL, w up to 0.6."""
    rng = np.random.default_rng([seed, B, n_cmd])
    v = rng.uniform(-0.2, 1.0, (B, n_cmd)) * float(CELL) * v_cell
    w = rng.uniform(-0.6, 0.6, (B, n_cmd))
    return np.stack([v, w], 2).astype(F)


def body_points(P, reach=0.3):
    """P points on a spiral around the centre, the farthest `reach` metres out."""
    k = np.arange(P)
    r = reach * (k + 1) / max(P, 1)
    return np.stack([r * np.cos(2.4 * k), r * np.sin(2.4 * k)], 1).astype(F)


def hook_vs_restatement(capi, cls, sources, start, dt, body, cmds, hold, c=0, site_mask=2, max_cost=0, stm=STM, tag=None):
    cost, trav, nav = np_field(cls, sources, c, site_mask, max_cost)
    want = np_rollouts(cost, trav, (0, 0), stm, start, dt, body, cmds, hold)
    got = capi.debug_rollouts(cls, sources, stm, start, dt, body, cmds, hold, site_mask, c, max_cost)
    check(got, want, nav, tag)
    assert got[1]["nav"]["rounds"] == 0
    return got, want


@pytest.fixture(scope="module")
def capi():
    import slam.net_amd.build as b
    b.build()
    import slam.net_amd.capi as capi
    return capi


# ---- the surface -------------------------------------------------------------------------------------------------------------------
def test_surface(capi):
    L = capi.lib()
    header = open(os.path.join(ROOT, "include", "slamhip.h")).read()
    for n in SYMBOLS:
        assert hasattr(L, n) and n in L._signatures and re.search(r"\b%s\s*\(" % n, header)
    assert len(L._signatures["slamhip_hs_rollouts"][1]) == 14 == len(L._signatures["slamhip_hsproc_rollouts"][1])
    assert len(L._signatures["slamhip_debug_rollouts"][1]) == 19
    dt = capi.ROLLOUT_RESULT
    assert dt.itemsize == 28 and list(dt.names) == RESULT_FIELDS and [dt.fields[f][1] for f in RESULT_FIELDS] == list(range(0, 28, 4))
    assert dt.fields["end_cost"][0] == np.uint32 and dt.fields["min_cost"][0] == np.uint32 and dt.fields["theta"][0] == np.float32
    sm = capi.ROLLOUT_SUMMARY
    assert sm.itemsize == 64 and list(sm.names) == ["nav", "start_cost", "n_complete", "key_end", "key_min"]
    assert [sm.fields[f][1] for f in sm.names] == [0, 40, 44, 48, 56] and sm.fields["nav"][0] == capi.NAV_SUMMARY
    assert sm.fields["key_end"][0] == np.uint64 and sm.fields["start_cost"][0] == np.uint32
    for name, fields in (("result", RESULT_FIELDS), ("summary", list(sm.names))):
        m = re.search(r"typedef struct slamhip_rollout_%s \{(.*?)\} slamhip_rollout_%s;\s*/\*(.*?)\*/" % (name, name), header, re.S)
        body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        assert re.findall(r"(\w+)\s*[,;]", body) == fields, name           # the header's members, in order
        assert "no padding" in m.group(2) and ("28 bytes" if name == "result" else "64 bytes") in m.group(2)
    native = open(os.path.join(ROOT, "bindings", "csharp", "SlamHip", "SlamHip.Native.cs")).read()
    for n in SYMBOLS:
        assert n in native
    assert "struct RolloutResult" in native and "struct RolloutSummary" in native
    import slam.net_amd.build as b
    import slam.net_amd.hector as hm
    assert hasattr(hm.MapRepMultiMap, "rollouts") and hasattr(hm.HectorSLAMProcessor, "Rollouts") and hasattr(hm.HectorSLAMProcessor, "DriveCommand")
    assert "hs_rollout.hip" in b.SOURCES and "hs_rollout.h" in b.HEADERS


# ---- random class arrays -----------------------------------------------------------------------------------------------------------
# The seed of NV.random_classes per shape, chosen on the CPU so that a free start exists (the one cell of the 1 x 1 array is free
# under it); the three outcomes the test asserts then hold by construction, for every P, hold and B = 67.
CLASS_SEED = {(1, 1): 2, (1, 70): 0, (70, 1): 0, (33, 31): 0, (97, 66): 0}
N_CMD = 5


def random_case(cls, shape, P, B):
    """One parametrisation: the sources, dt, the body, the fan of commands and the start poses the fan is rolled out from -- a free
    one (the middle of the open block of the shapes of NV.BIG; else the first free cell, with a body that stays inside it), one on the
    first cell that is not free (if any) and one outside the array."""
    w, h = shape
    big = shape in NV.BIG
    fx, fy = (w // 2, h // 2) if big else (int(v) for v in np.argwhere(cls == 2)[0][::-1])
    cmds = fan(B, N_CMD, 3, v_cell=1.6)
    if B > 3:
        cmds[1] = 0.0                                                      # stands still: complete wherever the start is free
        cmds[2] = 0.0
        cmds[2, :, 0] = F(200.0 * float(CELL))                             # leaves the array with its first step
    body = body_points(P, reach=0.3 if big else 0.25 * float(CELL))
    starts = [(F(fx * float(CELL)), F(fy * float(CELL)), F(0.3))]
    bad = np.argwhere(cls != 2)
    if len(bad):
        starts.append((F(bad[0][1] * float(CELL)), F(bad[0][0] * float(CELL)), F(-1.2)))
    starts.append((F(-2 * float(CELL)), F(0.0), F(0.0)))
    return [(fx, fy)], F(1.0), body, cmds, starts


@pytest.fixture(scope="module")
def arrays():
    out = {s: NV.random_classes(s, CLASS_SEED[s]) for s in NV.SHAPES}
    for a in out.values():
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("B", [1, 67])
@pytest.mark.parametrize("hold", [1, 3])
@pytest.mark.parametrize("P", [0, 1, 3, 32])
@pytest.mark.parametrize("shape", NV.SHAPES)
def test_random_arrays(capi, arrays, shape, P, hold, B):
    cls = arrays[shape]
    src, dt, body, cmds, starts = random_case(cls, shape, P, B)
    T = N_CMD * hold
    n_free = []
    for k, start in enumerate(starts):
        _, want = hook_vs_restatement(capi, cls, src, start, dt, body, cmds, hold, tag=(shape, P, hold, B, k))
        n_free += [r[0] for r in want[0]]
        if k > 0:                                                          # a start that is not free: nothing of any rollout is
            assert all(r[:4] == (0, -1, UNREACHED, UNREACHED) for r in want[0])
            assert want[1] == dict(start_cost=UNREACHED, n_complete=0, key_end=NO_KEY, key_min=NO_KEY)
    if B == 67:                                                            # a wrong n_free must not be able to hide in an all-blocked case
        assert any(n == T + 1 for n in n_free), "no complete rollout"
        assert any(0 < n < T + 1 for n in n_free), "no rollout that stops early"
        assert any(n == 0 for n in n_free), "no rollout with n_free == 0"


@pytest.mark.parametrize("shape", NV.BIG)
def test_random_fan_is_mixed(arrays, shape):
    """On the larger arrays the random part of the fan itself -- not only the two planted commands -- ends in all ways: some
    rollouts complete, some are cut by a wall or the unknown, at different steps."""
    cls = arrays[shape]
    src, dt, body, cmds, starts = random_case(cls, shape, 3, 67)
    cost, trav, _ = np_field(cls, src)
    recs, _ = np_rollouts(cost, trav, (0, 0), STM, starts[0], dt, body, cmds, 3)
    n_free = [r[0] for r in recs[3:]]
    assert any(n == 3 * N_CMD + 1 for n in n_free) and len({n for n in n_free if n < 3 * N_CMD + 1}) >= 3, n_free


# ---- closed forms (cell length 0.125: a step of one cell is exact) -----------------------------------------------------------------
def drive(n, v_cells=1.0, w=0.0):
    """One command sequence of n pairs, v cells per step with dt = 1."""
    return np.tile(np.array([v_cells * float(CELL), w], F), (1, n, 1))


def at_cell(x, y, th=0.0):
    return (F(x * float(CELL)), F(y * float(CELL)), F(th))


@pytest.mark.parametrize("k", [1, 2, 7])
def test_straight_drive_towards_a_wall(capi, k):
    c = np.full((5, 20), 2, np.uint8)
    c[:, 2 + k] = 1                                                        # the wall, k cells ahead of the start
    src = [(0, 2)]
    (res, sm), _ = hook_vs_restatement(capi, c, src, at_cell(2, 2), 1.0, None, drive(12), 1)
    cost = NV.np_nav(c, src, rect=(0, 0, 20, 5))["cost"]
    assert res[0]["n_free"] == k and res[0]["end_cost"] == cost[2, 2 + k - 1] == 5 * (2 + k - 1)
    assert (res[0]["min_step"], res[0]["min_cost"]) == (0, 10) and sm["start_cost"] == 10
    assert bits(res[0]["x"]) == bits(F((2 + k - 1) * float(CELL))) and bits(res[0]["y"]) == bits(F(2 * float(CELL)))
    assert sm["n_complete"] == 0 and sm["key_end"] == NO_KEY and sm["key_min"] == (10 << 32)


def test_half_cells_round_to_even(capi):
    c = np.full((8, 8), 2, np.uint8)
    (res, sm), _ = hook_vs_restatement(capi, c, [(2, 4)], at_cell(2.5, 3.5), 1.0, None, drive(1, 0.0), 1)
    assert sm["start_cost"] == 0 and res[0]["n_free"] == 2 and res[0]["end_cost"] == 0           # cells (2, 4), not (3, 4), (2, 3) or (3, 3)
    cost = NV.np_nav(c, [(0, 0)], rect=(0, 0, 8, 8))["cost"]
    (res, sm), _ = hook_vs_restatement(capi, c, [(0, 0)], at_cell(2.5, 3.5), 1.0, None, drive(1, 0.0), 1)
    assert sm["start_cost"] == cost[4, 2] == 5 * 2 + 7 * 2
    body = np.array([[1.5 * float(CELL), 0.0]], F)                         # the body point at 4.0 cells: cell 4; the wall at 4 blocks, at 5 does not
    for wall, n in ((4, 0), (5, 2)):
        w = c.copy(); w[:, wall] = 1
        (res, _), _ = hook_vs_restatement(capi, w, [(0, 0)], at_cell(2.5, 3.5), 1.0, body, drive(1, 0.0), 1)
        assert res[0]["n_free"] == n


def test_rotation_in_place_swings_an_arm_into_a_wall(capi):
    c = np.full((21, 21), 2, np.uint8)
    c[14, :] = 1                                                           # four rows below the centre row
    body = np.array([[6.0 * float(CELL), 0.0]], F)
    cmds = drive(40, 0.0, 0.05)
    (res, sm), (recs, _) = hook_vs_restatement(capi, c, [(10, 10)], at_cell(10, 10), 1.0, body, cmds, 1)
    # the arm's end reaches row 14 when rint(10 + 6 sin(theta)) = 14: 6 sin(theta) >= 3.5, theta >= asin(3.5 / 6) = 0.6228: step 13
    assert recs[0][0] == 13 == res[0]["n_free"] and res[0]["end_cost"] == 0 and res[0]["min_step"] == 0
    assert bits(res[0]["x"]) == bits(F(1.25)) and bits(res[0]["theta"]) == bits(recs[0][6])


def test_rollout_leaves_the_map(capi):
    c = np.full((6, 6), 2, np.uint8)
    cmds = np.concatenate([drive(8), drive(8, -1.0), drive(8, 1.0, 0.0)])
    (res, sm), _ = hook_vs_restatement(capi, c, [(2, 2)], at_cell(2, 2), 1.0, None, cmds, 1)
    assert list(res["n_free"]) == [4, 3, 4] and list(res["end_cost"]) == [15, 10, 15] and sm["n_complete"] == 0
    (res, _), _ = hook_vs_restatement(capi, c, [(2, 2)], at_cell(2, 2, np.pi / 2), 1.0, None, drive(8), 1)     # ... and off the last row
    assert res[0]["n_free"] == 4 and res[0]["end_cost"] == 15


def test_commands_that_are_not_finite(capi):
    c = np.full((6, 6), 2, np.uint8)
    cmds = np.zeros((5, 3, 2), F)
    cmds[0, :, 0] = np.nan                                                 # x_1 is NaN: no cell
    cmds[1, 1, 0] = np.inf                                                 # x_2 is inf
    cmds[2, 0, 1] = np.nan                                                 # theta_1 is NaN: pose 1 still has its cell, pose 2 (NaN * 0) none
    cmds[3, 0, 1] = np.inf
    (res, sm), _ = hook_vs_restatement(capi, c, [(2, 2)], at_cell(2, 2), 1.0, None, cmds, 1)
    assert list(res["n_free"]) == [1, 2, 2, 2, 4] and sm["n_complete"] == 1 and sm["key_end"] == 4 and sm["key_min"] == 0
    body = np.array([[float(CELL), 0.0]], F)                               # with a body point a NaN heading is not free at once
    (res, _), _ = hook_vs_restatement(capi, c, [(2, 2)], at_cell(2, 2), 1.0, body, cmds, 1)
    assert list(res["n_free"]) == [1, 2, 1, 1, 4]


def test_coordinate_reaches_two_to_the_24(capi):
    c = np.full((6, 6), 2, np.uint8)
    cmds = np.zeros((3, 2, 2), F)
    cmds[0, 0, 0] = F(2.0 ** 21)                                           # x_1 * stm = 2^24 + 2: no cell
    cmds[1, 0, 0] = F(-(2.0 ** 21)); cmds[1, 1, 0] = F(2.0 ** 21)          # ... and back again: the rollout ended at pose 1
    cmds[2, 0, 0] = F(2.0 ** 20)                                           # a cell, far outside M
    (res, _), _ = hook_vs_restatement(capi, c, [(2, 2)], at_cell(2, 2), 1.0, None, cmds, 1)
    assert list(res["n_free"]) == [1, 1, 1]


def test_pocket_cut_off_from_the_source(capi):
    c = np.full((7, 13), 2, np.uint8)
    c[:, 6] = 1                                                            # a wall: the right half is traversable, not reached
    src = [(1, 3)]
    (res, sm), _ = hook_vs_restatement(capi, c, src, at_cell(9, 3), 1.0, None, drive(3, 0.0), 1)
    assert res[0]["n_free"] == 0 and sm["start_cost"] == UNREACHED and sm["nav"]["n_traversable"] == 84 and sm["nav"]["n_reached"] == 42
    arm = np.array([[2.0 * float(CELL), 0.0]], F)                          # from (5, 3) the arm's end lies at (7, 3), in the pocket: traversable
    (res, _), _ = hook_vs_restatement(capi, c, src, at_cell(5, 3), 1.0, arm, drive(3, 0.0), 1)
    assert res[0]["n_free"] == 4
    (res, _), _ = hook_vs_restatement(capi, c, src, at_cell(4, 3), 1.0, arm, drive(3, 0.0), 1)   # ... and at (6, 3), on the wall
    assert res[0]["n_free"] == 0


def test_no_used_source(capi):
    c = np.full((6, 6), 2, np.uint8)
    c[0, 0] = 1
    for src in ([(0, 0)], [(-1, 2), (6, 6)]):
        (res, sm), _ = hook_vs_restatement(capi, c, src, at_cell(2, 2), 1.0, body_points(3, 0.1), fan(9, 2, 1), 2)
        assert (res["n_free"] == 0).all() and (res["min_step"] == -1).all() and (res["end_cost"] == UNREACHED).all()
        assert sm["key_end"] == NO_KEY == sm["key_min"] and sm["n_complete"] == 0 and sm["nav"]["n_sources_used"] == 0 and sm["nav"]["n_reached"] == 0


def test_identical_commands_go_to_the_lower_b(capi):
    c = np.full((9, 9), 2, np.uint8)
    cmds = np.concatenate([drive(3, -1.0), drive(3), drive(3), drive(3, -1.0)])
    (res, sm), _ = hook_vs_restatement(capi, c, [(7, 4)], at_cell(3, 4), 1.0, None, cmds, 1)
    assert list(res["end_cost"]) == [35, 5, 5, 35] and sm["n_complete"] == 4
    assert capi.rollout_key(sm["key_end"]) == (5, 1) and capi.rollout_key(sm["key_min"]) == (5, 1)


def test_min_step_tie_takes_the_first(capi):
    c = np.full((9, 12), 2, np.uint8)
    (res, sm), _ = hook_vs_restatement(capi, c, [(3, 4), (6, 4)], at_cell(2, 4), 1.0, None, drive(6), 1)
    assert (res[0]["n_free"], res[0]["min_step"], res[0]["min_cost"], res[0]["end_cost"]) == (7, 1, 0, 10)
    (res, _), _ = hook_vs_restatement(capi, c, [(3, 4), (6, 4)], at_cell(2, 4), 1.0, None, drive(2), 3)      # hold = 3: the same six steps
    assert (res[0]["n_free"], res[0]["min_step"]) == (7, 1)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def refusal_cases():
    nan, inf = float("nan"), float("inf")
    return [dict(site_mask=1), dict(site_mask=4), dict(clearance=-1), dict(clearance=255), dict(S=0), dict(S=4097), dict(sources=False),
            dict(B=0), dict(B=65537), dict(n_cmd=0), dict(n_cmd=257), dict(hold=0), dict(hold=257), dict(n_cmd=256, hold=5), dict(n_cmd=33, hold=32),
            dict(B=65536, n_cmd=65), dict(P=-1), dict(P=33), dict(start=(nan, 0.0, 0.0)), dict(start=(0.0, inf, 0.0)), dict(start=(0.0, 0.0, -inf)),
            dict(dt=nan), dict(dt=inf), dict(P=2, bad_body=nan), dict(P=32, bad_body=inf), dict(pose=False), dict(cmds=False), dict(results=False),
            dict(P=1, body=False), dict(summary=False)]


def refusal_buffers(start=(0.25, 0.25, 0.0), bad_body=None, P=0):
    """The arrays of one refused call, the outputs filled with 77."""
    src = np.zeros((4097, 2), np.int32)
    pose = np.array(start, F)
    body = np.zeros((33, 2), F)
    if bad_body is not None:
        body[P - 1, 1] = bad_body
    cmds = np.zeros((64, 2), F)                                            # (a refused call reads no command)
    res = np.full(64, 77, np.dtype([(f, np.int32) for f in RESULT_FIELDS]))
    summary = np.full(16, 77, np.int32)
    return src, pose, body, cmds, res, summary


def refusal_args(bufs, S=1, dt=1.0, P=0, B=2, n_cmd=2, hold=2, sources=True, pose=True, body=True, cmds=True, results=True, summary=True,
                 start=None, bad_body=None):
    p = lambda a, on=True: a.ctypes.data_as(C.c_void_p) if on else None
    src, ps, bd, cm, res, sm = bufs
    return [p(src, sources), S], [p(ps, pose), C.c_float(dt), p(bd, body), P, p(cm, cmds), B, n_cmd, hold, p(res, results), p(sm, summary)]


def untouched(bufs):
    return all((b.view(np.int32) == 77).all() for b in bufs[4:])


@pytest.mark.parametrize("kw", refusal_cases(), ids=lambda kw: ",".join("%s=%s" % i for i in kw.items()).replace(" ", ""))
def test_refusals_leave_the_outputs_untouched(capi, kw):
    lib = capi.lib()
    kw = dict(kw)
    c = np.full((8, 8), 2, np.uint8)
    spec = dict(site_mask=kw.pop("site_mask", 2), clearance=kw.pop("clearance", 0))
    bufs = refusal_buffers(**{k: v for k, v in kw.items() if k in ("start", "bad_body", "P")})
    head, tail = refusal_args(bufs, **kw)
    rc = lib.slamhip_debug_rollouts(c.ctypes.data_as(C.c_void_p), 8, 8, spec["site_mask"], spec["clearance"], 0, *head, C.c_float(float(STM)), *tail)
    assert rc == capi.ERR_INVALID and lib.slamhip_last_error(), kw
    assert untouched(bufs), kw


def test_refusals_of_the_class_array(capi):
    lib = capi.lib()
    c = np.full((8, 8), 2, np.uint8)
    for cw, ch, stm in ((0, 8, 8.0), (8, 0, 8.0), (-1, 8, 8.0), (1 << 13, (1 << 12) + 1, 8.0), (8, 8, 0.0), (8, 8, -8.0), (8, 8, float("nan")),
                        (8, 8, float("inf"))):
        bufs = refusal_buffers()
        head, tail = refusal_args(bufs)
        assert lib.slamhip_debug_rollouts(c.ctypes.data_as(C.c_void_p), cw, ch, 2, 0, 0, *head, C.c_float(stm), *tail) == capi.ERR_INVALID
        assert untouched(bufs)
    bufs = refusal_buffers()
    head, tail = refusal_args(bufs)
    assert lib.slamhip_debug_rollouts(c.ctypes.data_as(C.c_void_p), 8, 8, 2, 0, 0, *head, C.c_float(8.0), *tail) == 0 and not untouched(bufs)   # the call itself is fine
    bufs = refusal_buffers()
    head, tail = refusal_args(bufs, B=1, n_cmd=32, hold=32)                # T = 1024 exactly is allowed
    assert lib.slamhip_debug_rollouts(c.ctypes.data_as(C.c_void_p), 8, 8, 2, 0, 0, *head, C.c_float(8.0), *tail) == 0
    assert bufs[4][0]["n_free"] == 1025
