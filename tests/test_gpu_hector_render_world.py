"""K25 on the device: slamhip_hs_render_world through MapRepMultiMap.RenderWorld / HectorSLAMProcessor.RenderKeyframesWorld.  Every case
of tests/render_world_cases.py (each checked on the CPU by tests/test_hs_render_world_abi.py) for tile sides 8, 16 and 32: the world
download of the hook's rectangle == the hook's cells on every level, and once more after one further ordinary UpdateByScan, whose
marks show where the render left the levels' indices.  The tie to K20 without the hook: a 256 x 256 pyramid drawn by slamhip_hs_render
== the world of a 64 x 64 window drawn by slamhip_hs_render_world, cells and -- after the window has been shifted onto rendered tiles
-- probabilities.  Capacity, the refusals, a range over two launches (SLAMHIP_K20_CHUNK=4, a fresh interpreter), and the lap end to
end through close_loops(render="world")."""
import os
import subprocess
import sys

import numpy as np
import pytest

import k5_cases as kc
import render_cases as rc
import render_world_cases as wc
from test_gpu_hector import hs_mod, ctx                                  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu
POOL = 1 << 24


@pytest.fixture(scope="module")
def capi():
    import slam.net_amd.capi as capi
    return capi


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_cells(got, ref, what):
    for field in ("update_index", "value"):
        g, r = bits(got[field]), bits(ref[field])
        bad = np.flatnonzero(g != r)
        assert bad.size == 0, (what, field, bad.size, bad[:8], got[field][bad[:8]], ref[field][bad[:8]])


_hooked = {}


def hooked(capi, name):
    """The case through the hook, and one further scan drawn over it with KEEP (computed once, shared, not changed)."""
    if name not in _hooked:
        c = wc.CASES[name]()
        cells, ui, ci = wc.hook_calls(capi, c)
        more, _, _ = capi.debug_render_world([wc.rect_of(l) for l in range(wc.LEVELS)], wc.CELL_LEN, cells, ui, ci, [ONE_MORE[0]], [ONE_MORE[1]], [ONE_MORE[2]],
                                             keep=True, factors=c.factors or (0.4, 0.9))
        _hooked[name] = (cells, more)
    return _hooked[name]


ONE_MORE = wc.from_to((30, 34), [(35, 36), (27, 38), (32, 28), (60, 3)])       # inside the window: an ordinary update draws all of it


def make(hs_mod, ctx, c, T, pool=POOL):
    rep = hs_mod.MapRepMultiMap(wc.CELL_LEN, wc.WIN, wc.LEVELS, ctx=ctx)
    if c.factors:
        rep.SetUpdateFactorFree(c.factors[0]); rep.SetUpdateFactorOccupied(c.factors[1])
    rep.set_backing(T, pool)
    if c.shift != (0, 0):
        rep.shift(*c.shift)
    for xy, origin, _ in c.scans:
        rep.ScansAdd(hs_mod.ScanCloud(xy, (origin[0], origin[1], 0.0)))
    return rep


def run_calls(rep, c):
    poses = np.array([s[2] for s in c.scans], np.float32).reshape(-1, 3)
    for first, last, keep in c.calls:
        rep.RenderWorld(poses[first:last], first, last, keep=keep)


def world(rep, level):
    x0, y0, w, h = wc.rect_of(level)
    ox, oy = rep.origin()
    return rep.world_cells(level, (ox >> level) + x0, (oy >> level) + y0, w, h).reshape(-1)


@pytest.mark.parametrize("T", wc.TILES)
@pytest.mark.parametrize("name", list(wc.CASES))
def test_case(hs_mod, ctx, capi, name, T):
    c = wc.CASES[name]()
    want, want_more = hooked(capi, name)
    rep = make(hs_mod, ctx, c, T)
    try:
        st0 = rep.backing_stats()                                         # (the case's own shift has moved the counts)
        run_calls(rep, c)
        for l in range(wc.LEVELS):
            same_cells(world(rep, l), want[l], (name, T, l))
        st = rep.backing_stats()
        assert all(st[k] == st0[k] for k in ("evicted_cells", "restored_cells", "dropped_cells")), (st0, st)
        rep.UpdateByScan(hs_mod.ScanCloud(ONE_MORE[0]), ONE_MORE[2])     # its marks are the levels' indices + 1 and + 2
        for l in range(wc.LEVELS):
            same_cells(world(rep, l), want_more[l], (name, T, l, "one more update"))
    finally:
        rep.close()


def test_two_launches():
    """Ranges of 6 to 10 scans in launches of 4 (SLAMHIP_K20_CHUNK, read once per process: a fresh interpreter)."""
    here = os.path.abspath(__file__)
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-m", "pytest", here, "-m", "gpu", "-x", "-q", "-k",
                        "test_case and (ends_outside or keep_existing or origin_off_tile or empty_scan or sub_range)"],
                       env=dict(os.environ, SLAMHIP_K20_CHUNK="4"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and " passed" in out and "failed" not in out, out[-3000:]


def tie_scans():
    return [wc.rand_scan(200 + k, (30 + 25 * k, 220 - 27 * k), 2, 253, 90) for k in range(8)]


def test_tie_to_k20_cells_and_probabilities(hs_mod, ctx, capi):
    """Pyramid A, 256 x 256 x 2 without backing, drawn by slamhip_hs_render; pyramid B, a 64 x 64 window at origin (0, 0) with
    backing, drawn by slamhip_hs_render_world at the same poses: B's world [0, 256)^2 == A's cells on both levels.  Then B's
    window is shifted onto rendered tiles: its cells AND probabilities == A's same region."""
    scans = tie_scans()
    poses = np.array([s[2] for s in scans], np.float32)
    A = hs_mod.MapRepMultiMap(wc.CELL_LEN, (256, 256), 2, ctx=ctx)
    B = hs_mod.MapRepMultiMap(wc.CELL_LEN, wc.WIN, 2, ctx=ctx)
    try:
        B.set_backing(16, POOL)
        for xy, origin, _ in scans:
            for r in (A, B):
                r.ScansAdd(hs_mod.ScanCloud(xy, (origin[0], origin[1], 0.0)))
        A.Render(poses)
        B.RenderWorld(poses)
        a = [A.Maps[l].GetCells().reshape(256 >> l, 256 >> l) for l in range(2)]
        for l in range(2):
            assert (a[l]["value"] != 0).sum() > 1000
            same_cells(B.world_cells(l, 0, 0, 256 >> l, 256 >> l).reshape(-1), a[l].reshape(-1), ("tie", l))
        for dx, dy in ((96, 128), (-64, -96)):                            # onto tiles (no multiple of 64: the window straddles them), and half way back
            B.shift(dx, dy)
            ox, oy = B.origin()
            for l in range(2):
                w = 64 >> l
                X, Y = ox >> l, oy >> l
                same_cells(B.Maps[l].GetCells(), np.ascontiguousarray(a[l][Y:Y + w, X:X + w]).reshape(-1), ("shifted", dx, l))
                idx_b = np.arange(w * w, dtype=np.int32)
                yy, xx = np.divmod(idx_b, w)
                idx_a = ((Y + yy) * (256 >> l) + X + xx).astype(np.int32)
                assert (bits(B.Maps[l].GetCachedProbability(idx_b)) == bits(A.Maps[l].GetCachedProbability(idx_a))).all(), ("probability", dx, l)
    finally:
        A.close(); B.close()


def test_capacity_is_a_refusal(hs_mod, ctx, capi):
    """max_bytes one slot short of what the render needs: SLAMHIP_ERR_NOMEM, and the window, the directory, the stats and the indices
    are what they were -- shown against a twin that was never asked."""
    c = wc.CASES["ends_outside"]()
    T = 16
    slot = T * T * 12
    pre = wc.rand_scan(7, (30, 30), 2, 61)

    def start(pool):
        r = make(hs_mod, ctx, c, T, pool=pool)
        r.UpdateByScan(hs_mod.ScanCloud(pre[0]), pre[2])
        r.shift(16, 8)                                                    # tiles exist, the window is not at the origin
        return r
    probe = start(POOL)
    try:
        run_calls(probe, c)
        n = probe.backing_stats()["tiles"]                                # what the render needs from this state (the old tiles are dropped)
    finally:
        probe.close()
    assert n > 20
    reps = [start((n - 1) * slot) for _ in range(2)]
    try:
        before = reps[0].backing_stats()
        assert before["tiles"] > 0
        poses = np.array([s[2] for s in c.scans], np.float32)
        for keep in (False, True):
            with pytest.raises(capi.SlamhipError) as e:
                reps[0].RenderWorld(poses, keep=keep)
            assert e.value.code == capi.ERR_NOMEM
            assert reps[0].backing_stats() == before
        reps[0].set_backing(T, (n + 8) * slot)                            # (more room under the same tile side: the pool stays)
        reps[1].set_backing(T, (n + 8) * slot)
        for r in reps:
            r.UpdateByScan(hs_mod.ScanCloud(ONE_MORE[0]), ONE_MORE[2])
        for l in range(wc.LEVELS):
            same_cells(world(reps[0], l), world(reps[1], l), ("after NOMEM", l))
        reps[0].RenderWorld(poses)                                        # ... and with room it is drawn
        assert reps[0].backing_stats()["tiles"] > 20
    finally:
        for r in reps:
            r.close()


def test_refusals(hs_mod, ctx, capi):
    """Backing off; K20's list; the world bound; a line of more than 32767 cells: SLAMHIP_ERR_INVALID, nothing changed."""
    c = wc.CASES["ends_outside"]()
    rep = make(hs_mod, ctx, c, 16)
    try:
        poses = np.array([s[2] for s in c.scans], np.float32)
        rep.RenderWorld(poses)
        before = [world(rep, l).tobytes() for l in range(wc.LEVELS)], rep.backing_stats()

        def refused(first, last, p, flags=0):
            with pytest.raises(capi.SlamhipError) as e:
                capi.call("slamhip_hs_render_world", rep._h, first, last, capi._vp(np.ascontiguousarray(p, np.float32)), flags)
            assert e.value.code == capi.ERR_INVALID
            assert ([world(rep, l).tobytes() for l in range(wc.LEVELS)], rep.backing_stats()) == before
        refused(-1, 2, poses[:3])
        refused(3, 2, poses[:1])
        refused(0, 7, np.zeros((7, 3), np.float32))
        refused(0, 6, poses, 2)
        for flags in (0, capi.RENDER_KEEP):
            p = poses.copy(); p[4, 1] = np.nan
            refused(0, 6, p, flags)
            p = poses.copy(); p[2, 0] = np.float32((2 ** 20 + 9) * wc.CELL_LEN)       # the begin cell beyond the world bound
            refused(0, 6, p, flags)
        rep.set_reference_cache(True)
        refused(0, 6, poses)
        rep.set_reference_cache(False)
        # a line of more than 32767 cells needs a point that far away
        far = wc.from_to((10, 10), [(10 + 32768, 10)])
        k = rep.ScansAdd(hs_mod.ScanCloud(far[0]))
        refused(k, k + 1, np.array([far[2]], np.float32), capi.RENDER_KEEP)
        rep.set_backing(0, 0)
        with pytest.raises(capi.SlamhipError) as e:
            rep.RenderWorld(poses, 0, 6)
        assert e.value.code == capi.ERR_INVALID and b"slamhip_hs_render" in capi.lib().slamhip_last_error()
    finally:
        rep.close()


def test_end_to_end_lap(hs_mod, ctx, capi):
    """The lap of tests/test_gpu_hector_render.py::test_end_to_end_lap in a window of 128 x 128 cells of 0.1 m, which the lap leaves,
    with scrollBacking on: keyframes with keep_scan=True at the drifted poses (a heading bias of 0.2 degrees per step), then
    close_loops(render="world").  Over the world rectangle the render at the relaxed poses differs from the render at the true poses
    in fewer cells than the render at the drifted poses does -- an ordering, not a threshold.  And RenderKeyframes, the old path,
    leaves the world outside the window all Reset: the gap K25 closes."""
    import scanmatch_cases as sc
    L = rc.lap()
    N = len(L["scans"])
    proc = hs_mod.HectorSLAMProcessor(rc.LAP_CELL, (128, 128), (0.0, 0.0, 0.0), rc.LAP_LEVELS, ctx=ctx, scrollBacking=(16, 1 << 26))
    try:
        rep = proc.MapRep
        proc.shift(140, 136)                                              # the window round the first keyframe
        rep.SigConfigure(*rc.LAP_SIG)
        for i in range(N):
            proc.AddKeyframe(hs_mod.ScanCloud(L["scans"][i], (0.0, 0.0, 0.0)), L["drifted"][i], keep_scan=True)
        R = (-100, -100, 600, 600)                                        # world cells of level 0: the field and what the drift adds

        def cells():
            return rep.world_cells(0, *R)
        proc.RenderKeyframesWorld(L["true"])
        c_true = cells()
        proc.RenderKeyframesWorld()                                       # the store's poses: the drifted ones
        c_drift = cells()
        out = proc.close_loops(sc.LAP_MIN_GAP, capi.scanmatch_spec(**sc.LAP_SPEC), sc.accept, odom_w=rc.LAP_ODOM_W, render="world")
        assert out["poses"] is not None and int(out["accepted"].sum()) >= 1
        c_relax = cells()
        d_drift, d_relax = rc.sym_diff(c_drift, c_true), rc.sym_diff(c_relax, c_true)
        inside = np.zeros((R[3], R[2]), bool)
        inside[136 - R[1]:136 - R[1] + 128, 140 - R[0]:140 - R[0] + 128] = True
        n_out = int((c_relax["value"][~inside] > 0).sum())
        print("occupied at the true poses %d (outside the window %d); symmetric difference: drifted %d, relaxed %d; tiles %d" %
              (int((c_true["value"] > 0).sum()), n_out, d_drift, d_relax, rep.backing_stats()["tiles"]))
        assert n_out > 0 and d_relax < d_drift
        assert proc.get_origin() == (140, 136)
        proc.RenderKeyframes()                                            # K20: the window alone, the tiles dropped
        c_old = cells()
        assert (c_old["update_index"][~inside] == -1).all() and (bits(c_old["value"][~inside]) == 0).all()
        assert (c_old["value"][inside] != 0).any()
    finally:
        proc.Dispose()
