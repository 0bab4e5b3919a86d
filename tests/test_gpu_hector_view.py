"""GPU checks of the view gain (K15: slamhip_hs_view_gain, _view_select, the covered layer, the processor wrappers) against the host
hook slamhip_debug_view -- the header text the kernels run, in plain loops -- and the NumPy restatement of
tests/test_hs_view_abi.py.  Everything is compared with ==; nothing has a tolerance.

Shapes: two-level pyramids of 40 x 24, 64 x 64 and 96 x 72 (a row of two seen words of which one is partial, two whole, three),
reaches 1 .. 255 (all on the LDS path here), scans of 1 .. 1080 points, B of 1, 2, 11, 65 and 4096; a 544 x 520 pyramid whose
slot at reach 256 (513 rows x 17 words) is the first above the LDS budget, so it takes the global-scratch path unforced.  The
tests named *_paths run a second time in one fresh interpreter under SLAMHIP_K15_GLOBAL=1."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import test_hs_view_abi as A
from test_gpu_hector_shift import hs_mod, ctx                              # noqa: F401 (fixtures)

gpu = pytest.mark.gpu
F = np.float32
CELL0, STM, ORIGIN = A.CELL0, A.STM, A.ORIGIN


def put(hs_mod, rep, values, level=0):
    cells = np.zeros(values.shape, hs_mod.capi.CELL_DTYPE)
    cells["value"] = values
    cells["update_index"] = 3
    rep.Maps[level].SetCells(cells.ravel())


def scan_cloud(hs_mod, xy):
    return hs_mod.ScanCloud(xy, (ORIGIN[0], ORIGIN[1], 0.0))


def hook_views(capi, values, poses, xy, reach, cov_bits):
    """The hook at every pose -> (bitmaps (B, h, wpr), summaries as dicts)."""
    out = [capi.debug_view(values, STM, p, ORIGIN, xy, reach, cov_bits) for p in poses]
    return np.stack([b for b, _ in out]), [A.sdict(s) for _, s in out]


def sets_of(capi, bits, w):
    return [{(int(x), int(y)) for y, x in np.argwhere(capi.view_unpack(b, w))} for b in bits]


@pytest.fixture(scope="module")
def pyramids(hs_mod, ctx):
    reps = {d: hs_mod.MapRepMultiMap(CELL0, d, 2, ctx=ctx) for d in A.DIMS}
    yield reps
    for r in reps.values():
        r.close()


# ---- 1. gain, commit and the layer against the hook ----------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dims", A.DIMS)
def test_gain_and_commit_paths(hs_mod, pyramids, dims):
    """Every map kind, reach and scan size at all eleven poses in one call: the summaries == the hook's against the layer as it was
    before the call; commit rotates through -1, -2 and an index and the layer == the union afterwards; the layer is set from a random
    bitmap with its padding bits set, set empty, or left as the last call committed it."""
    capi = hs_mod.capi
    w, h = dims
    rep = pyramids[dims]
    poses = A.poses_of(w, h)
    it = 0
    for kind in A.KINDS:
        values = A.map_of(w, h, kind)
        put(hs_mod, rep, values)
        ck = [rep.Maps[l].checksum() for l in range(2)]
        for reach in A.REACHES:
            for n in A.SCAN_SIZES:
                xy = A.scan_of(n)
                rep.set_scan(scan_cloud(hs_mod, xy))
                if it % 3 == 0:
                    raw, _ = A.covered_of(w, h, it)
                    layer = rep.covered(0, bits=raw)
                    assert np.array_equal(layer, raw & capi.view_pack(np.ones((h, w), bool)))      # padding: ignored in, zero out
                elif it % 3 == 1:
                    layer = rep.covered(0, clear=True)
                    assert not layer.any()
                else:
                    layer = rep.covered(0)
                commit = (-1, -2, it % len(poses))[it % 3] if it % 2 else (-2, it % len(poses), -1)[it % 3]
                want_bits, want = hook_views(capi, values, poses, xy, reach, layer)
                got = rep.view_gain(poses, 0, reach, commit=commit)
                tag = (dims, kind, reach, n, commit)
                for p in range(len(poses)):
                    assert A.sdict(got[p]) == want[p], (tag, p, A.sdict(got[p]), want[p])
                after = layer | (np.bitwise_or.reduce(want_bits, 0) if commit == -2 else want_bits[commit] if commit >= 0 else 0)
                assert np.array_equal(rep.covered(0), after), tag
                it += 1
        assert [rep.Maps[l].checksum() for l in range(2)] == ck               # the map is read, never written


@gpu
def test_gain_matches_restatement_paths(hs_mod, pyramids):
    """A thin sample of tests/test_hs_view_abi.py's cases, device against the NumPy restatement itself."""
    n = 0
    for (w, h, kind, reach, pi, npts, with_cov) in A.sampled_cases():
        if pi not in (0, 6, 10) or reach not in (2, 33, 255):
            continue
        rep = pyramids[(w, h)]
        values = A.map_of(w, h, kind)
        put(hs_mod, rep, values)
        xy = A.scan_of(npts)
        bits, mask = A.covered_of(w, h, 7 * npts + reach) if with_cov else (None, None)
        rep.covered(0, bits=bits, clear=bits is None)
        V, s, _ = A.np_view(values, STM, A.poses_of(w, h)[pi], ORIGIN, xy, reach, mask)
        got = rep.view_gain([A.poses_of(w, h)[pi]], 0, reach, commit=0, scan=scan_cloud(hs_mod, xy))
        assert A.sdict(got[0]) == s, (w, h, kind, reach, pi, npts)
        want = A.mask_of(V, w, h) | (mask if mask is not None else False)
        assert np.array_equal(hs_mod.capi.view_unpack(rep.covered(0), w), want)
        n += 1
    assert n >= 50


@gpu
@pytest.mark.parametrize("B", [1, 2, 65, 4096])
def test_many_poses_paths(hs_mod, pyramids, B):
    """B poses on the 64 x 64 rooms at reach 8, in, at and around the window; commit -2 ORs B overlapping slots into the layer."""
    capi = hs_mod.capi
    w, h = 64, 64
    rep = pyramids[(w, h)]
    values = A.map_of(w, h, "rooms")
    put(hs_mod, rep, values)
    rng = np.random.default_rng(B)
    poses = np.stack([rng.uniform(-0.9, 7.3, B), rng.uniform(-0.9, 7.3, B), rng.uniform(-4, 4, B)], 1).astype(F)
    xy = A.scan_of(63)
    layer = rep.covered(0, bits=A.covered_of(w, h, B)[0])
    want_bits, want = hook_views(capi, values, poses, xy, 8, layer)
    got = rep.view_gain(poses, 0, 8, commit=-2, scan=scan_cloud(hs_mod, xy))
    assert [A.sdict(g) for g in got] == want
    assert np.array_equal(rep.covered(0), layer | np.bitwise_or.reduce(want_bits, 0))
    assert sum(s["n_new"] for s in want) > 0


@gpu
def test_contention_on_one_word_paths(hs_mod, pyramids):
    """1080 beams of three cells from one sensor cell: every lane ORs into the same few words."""
    capi = hs_mod.capi
    w, h = 64, 64
    rep = pyramids[(w, h)]
    values = A.map_of(w, h, "unknown")
    put(hs_mod, rep, values)
    a = np.linspace(-math.pi, math.pi, 1080, endpoint=False)
    xy = (np.stack([0.3 * np.cos(a), 0.3 * np.sin(a)], 1) + ORIGIN).astype(F)
    poses = [(3.2, 3.2, 0.0), (0.31, 3.2, 1.0), (3.2, 3.2, 0.0)]
    rep.covered(0, clear=True)
    want_bits, want = hook_views(capi, values, poses, xy, 255, None)
    got = rep.view_gain(poses, 0, 255, commit=1, scan=scan_cloud(hs_mod, xy))
    assert [A.sdict(g) for g in got] == want and 20 < want[0]["n_seen"] <= 49 and want[0]["n_walked"] == 1080
    assert np.array_equal(rep.covered(0), want_bits[1])


# ---- 2. the greedy choice ------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dims", A.DIMS)
def test_select_paths(hs_mod, pyramids, dims):
    """out_order, out_gain and the layer == the literal greedy loop over the hook's views: both modes, k below, at and above B, k = 64,
    the same pose twice (the second gains 0 and is never chosen), min_gain stopping the choice at round 1 and mid-way."""
    capi = hs_mod.capi
    w, h = dims
    rep = pyramids[dims]
    values = A.map_of(w, h, "rooms")
    cls = A.np_class_bits(values)
    put(hs_mod, rep, values)
    base = A.poses_of(w, h)
    poses = base[:5] + [base[0], base[3]] + base[5:] + [((w / 4) * CELL0, (h / 2) * CELL0, 1.0), ((3 * w / 4) * CELL0, (h / 2) * CELL0, -2.0)]
    B = len(poses)
    xy = A.scan_of(257)
    rep.set_scan(scan_cloud(hs_mod, xy))
    stopped = [0, 0, 0]
    for reach in (2, 33, 255):
        views = sets_of(capi, hook_views(capi, values, poses, xy, reach, None)[0], w)
        full = A.np_select(views, cls, np.zeros((h, w), bool), 0, 1, 64)[1]
        for mode in (0, 1):
            for k, min_gain, with_cov in ((1, 1, False), (3, 1, True), (B, 1, False), (64, 1, True), (64, 10 ** 6, False),
                                          (64, max(full[min(2, len(full) - 1)], 1), False), (5, 2, True)):
                bits, mask = A.covered_of(w, h, reach + k) if with_cov else (None, np.zeros((h, w), bool))
                rep.covered(0, bits=bits, clear=bits is None)
                order, gains, C = A.np_select(views, cls, mask, mode, min_gain, k)
                got_o, got_g = rep.view_select(poses, 0, reach, k, mode=mode, min_gain=min_gain)
                tag = (dims, reach, mode, k, min_gain, with_cov)
                assert (got_o.tolist(), got_g.tolist()) == (order, gains), (tag, got_o.tolist(), got_g.tolist(), order, gains)
                assert np.array_equal(capi.view_unpack(rep.covered(0), w), A.mask_of(C, w, h)), tag
                assert 5 not in order or 0 not in order                       # poses[5] == poses[0]
                stopped[0 if not order else 1 if len(order) < min(k, B) else 2] += 1
    assert all(stopped), stopped                                              # stopped at round 1, mid-way, and ran to k or B


# ---- 3. the path above the LDS budget, and the forced one ----------------------------------------------------------------------------
@gpu
def test_reach_above_the_lds_budget(hs_mod, ctx):
    """544 x 520: reach 255 is 511 rows x 17 words = 8687 words, in LDS; reach 256 is 513 x 17 = 8721, the first above K15_LDS_WORDS,
    in global scratch without the switch.  Both == the hook; and the scratch bound refuses B = 4096 at reach 256."""
    capi = hs_mod.capi
    w, h = 544, 520
    assert 511 * 17 <= capi.VIEW_LDS_WORDS < 513 * 17
    rep = hs_mod.MapRepMultiMap(CELL0, (w, h), 2, ctx=ctx)
    try:
        values = A.map_of(w, h, "rooms")
        put(hs_mod, rep, values)
        xy = A.scan_of(65)
        poses = [((w / 2 + 20.3) * CELL0, (h / 2) * CELL0, 0.4), (1.0 * CELL0, 2.0 * CELL0, 1.0), ((w - 3) * CELL0, (h - 2) * CELL0, 2.5)]
        rep.set_scan(scan_cloud(hs_mod, xy))
        layer = rep.covered(0, clear=True)
        for reach in (255, 256, 300):
            want_bits, want = hook_views(capi, values, poses, xy, reach, layer)
            got = rep.view_gain(poses, 0, reach, commit=-2)
            assert [A.sdict(g) for g in got] == want, reach
            layer = layer | np.bitwise_or.reduce(want_bits, 0)
            assert np.array_equal(rep.covered(0), layer), reach
            assert reach != 256 or (want[0]["n_cut"] > 0 and want[0]["n_seen"] > 300), want[0]   # (the far walls lie 257 and 258 cells up and down)
        many = np.tile(np.asarray(poses[:1], F), (4096, 1))
        with pytest.raises(capi.SlamhipError) as e:
            rep.view_gain(many, 0, 256)                                       # 4096 x 8721 words > 2^25
        assert e.value.code == capi.ERR_INVALID
        assert np.array_equal(rep.covered(0), layer)
    finally:
        rep.close()


@gpu
def test_under_the_global_switch():
    """The *_paths tests again in one fresh interpreter with every slot in global scratch (SLAMHIP_K15_GLOBAL=1)."""
    here = os.path.abspath(__file__)
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-m", "pytest", here, "-m", "gpu", "-x", "-q", "-k", "paths"],
                       env=dict(os.environ, SLAMHIP_K15_GLOBAL="1"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and " passed" in out and "skipped" not in out, out[-3000:]


# ---- 4. state ------------------------------------------------------------------------------------------------------------------------
@gpu
def test_refusals_and_state(hs_mod, ctx):
    capi = hs_mod.capi
    w, h = 64, 48
    rep = hs_mod.MapRepMultiMap(CELL0, (w, h), 2, ctx=ctx)
    try:
        values = A.map_of(w, h, "rooms")
        put(hs_mod, rep, values)
        poses = np.asarray(A.poses_of(w, h)[:4], F)

        def refused(code, fn, *a, **kw):
            with pytest.raises(capi.SlamhipError) as e:
                fn(*a, **kw)
            assert e.value.code == code, (a, kw, e.value)

        refused(capi.ERR_STATE, rep.view_gain, poses, 0, 8)                   # no scan
        refused(capi.ERR_STATE, rep.view_select, poses, 0, 8, 2)
        assert not rep.covered(0).any()                                       # no layer: empty, nothing allocated
        rep.set_scan(scan_cloud(hs_mod, A.scan_of(65)))
        for level in (-1, 2):
            refused(capi.ERR_INVALID, rep.view_gain, poses, level, 8)
            refused(capi.ERR_INVALID, rep.view_select, poses, level, 8, 2)
            buf = np.zeros((h, 2), np.uint32)
            assert capi.lib().slamhip_hs_view_get_covered(rep._h, level, buf.ctypes.data_as(C.c_void_p)) == capi.ERR_INVALID
            assert capi.lib().slamhip_hs_view_set_covered(rep._h, level, None) == capi.ERR_INVALID
        for reach in (0, -1, 4097):
            refused(capi.ERR_INVALID, rep.view_gain, poses, 0, reach)
            refused(capi.ERR_INVALID, rep.view_select, poses, 0, reach, 2)
        for B in (0, 4097):
            refused(capi.ERR_INVALID, rep.view_gain, np.zeros((B, 3), F), 0, 8)
            refused(capi.ERR_INVALID, rep.view_select, np.zeros((B, 3), F), 0, 8, 2)
        for commit in (-3, 4, 100):
            refused(capi.ERR_INVALID, rep.view_gain, poses, 0, 8, commit=commit)
        for k in (0, 65):
            refused(capi.ERR_INVALID, rep.view_select, poses, 0, 8, k)
        for mode in (-1, 2):
            refused(capi.ERR_INVALID, rep.view_select, poses, 0, 8, 2, mode=mode)
        for mg in (0, -5):
            refused(capi.ERR_INVALID, rep.view_select, poses, 0, 8, 2, min_gain=mg)
        assert not rep.covered(0).any()                                       # no refusal made or changed a layer
        # the limits themselves are taken
        assert rep.view_gain(poses, 0, 4096)[0]["n_walked"] > 0 and len(rep.view_select(poses, 1, 1, 64)[0]) >= 1
        # a layer of another level
        refused(capi.ERR_STATE, rep.view_gain, poses, 0, 8)
        refused(capi.ERR_STATE, rep.view_select, poses, 0, 8, 2)
        refused(capi.ERR_STATE, rep.covered, 0)
        assert rep.covered(1).any()
        rep.covered(0, clear=True)                                            # set_covered replaces it
        want_bits, want = hook_views(capi, values, poses, A.scan_of(65), 8, None)
        assert [A.sdict(g) for g in rep.view_gain(poses, 0, 8, commit=2)] == want
        assert np.array_equal(rep.covered(0), want_bits[2])
        # the window moves: the layer's stamp no longer holds until the layer is set again
        rep.shift(2, -4)
        refused(capi.ERR_STATE, rep.view_gain, poses, 0, 8)
        refused(capi.ERR_STATE, rep.view_select, poses, 0, 8, 2)
        refused(capi.ERR_STATE, rep.covered, 0)
        try:
            rep.view_gain(poses, 0, 8)
        except capi.SlamhipError as e:
            assert "set the layer again" in str(e)
        shifted = rep.Maps[0].GetCells().reshape(h, w)["value"]
        rep.covered(0, clear=True)
        want_bits, want = hook_views(capi, shifted, poses, A.scan_of(65), 8, None)
        assert [A.sdict(g) for g in rep.view_gain(poses, 0, 8, commit=-2)] == want
        # clear frees everything; the next call makes it anew
        rep.view_clear(); rep.view_clear()
        assert not rep.covered(0).any()
        assert [A.sdict(g) for g in rep.view_gain(poses, 0, 8, commit=0)] == want
        assert np.array_equal(rep.covered(0), want_bits[0])
        rep.Reset()                                                           # leaves the layer alone (the origin returns to 0: the stamp differs)
        refused(capi.ERR_STATE, rep.covered, 0)
    finally:
        rep.close()


@gpu
def test_map_and_search_untouched_with_cache_on(hs_mod, ctx):
    """Checksums of both levels and a K7 search are the same bits before and after gain, commit and select; the calls work with the
    reference's cache on (backing is off throughout)."""
    capi = hs_mod.capi
    w, h = 96, 72
    rep = hs_mod.MapRepMultiMap(CELL0, (w, h), 2, ctx=ctx)
    try:
        values = A.map_of(w, h, "rooms")
        put(hs_mod, rep, values)
        xy = A.scan_of(257)
        scan = scan_cloud(hs_mod, xy)
        poses = A.poses_of(w, h)
        centre = poses[0]

        def state():
            keys, _ = rep.lattice_search(scan, 0, centre, 3, 3, 4, 0.1)
            return [rep.Maps[l].checksum() for l in range(2)], np.asarray(keys).tobytes()
        s0 = state()
        want_bits, want = hook_views(capi, values, poses, xy, 33, None)
        for cache in (0, 1):
            rep.set_reference_cache(cache)
            rep.covered(0, clear=True)
            assert [A.sdict(g) for g in rep.view_gain(poses, 0, 33, commit=-2, scan=scan)] == want
            order, _ = rep.view_select(poses, 0, 33, 4, mode=1)
            assert len(order) <= 4
            assert state() == s0
        rep.set_reference_cache(0)
    finally:
        rep.close()


@gpu
def test_through_the_processor(hs_mod, ctx):
    """slamhip_hsproc_view_*: world poses, the window moved -- equal to the hs calls at the poses minus (float)origin * cell0."""
    proc = hs_mod.HectorSLAMProcessor(CELL0, (64, 48), [3.2, 2.4, 0.0], 2, ctx=ctx, scrollTrigger=4)
    try:
        rep = proc.MapRep
        put(hs_mod, rep, A.map_of(64, 48, "rooms"))
        scan = scan_cloud(hs_mod, A.scan_of(257))
        world = np.array([[2.9, 1.1, 0.3], [3.4, 0.2, -3.0], [1.0, 1.0, math.pi / 4], [5.5, 4.0, 2.0]], F)
        a = proc.ViewGain(scan, world, 0, 33)
        assert np.array_equal(a.view(np.int32), rep.view_gain(world, 0, 33).view(np.int32))      # the origin at (0, 0): every bit passes
        proc.shift(8, -6)
        assert proc.get_origin() == (8, -6)
        off = np.array([F(8) * F(CELL0), F(-6) * F(CELL0)], F)
        win = world.copy(); win[:, 0] = world[:, 0] - off[0]; win[:, 1] = world[:, 1] - off[1]
        rep.covered(0, clear=True)
        got = proc.ViewGain(scan, world, 0, 33, commit=-2)
        layer = rep.covered(0)
        rep.covered(0, clear=True)
        assert np.array_equal(got.view(np.int32), rep.view_gain(win, 0, 33, commit=-2).view(np.int32)) and got["n_seen"].sum() > 0
        assert np.array_equal(rep.covered(0), layer)
        rep.covered(0, clear=True)
        o1, g1 = proc.ViewSelect(scan, world, 0, 33, 3, mode=1)
        l1 = rep.covered(0)
        rep.covered(0, clear=True)
        o2, g2 = rep.view_select(win, 0, 33, 3, mode=1)
        assert o1.tolist() == o2.tolist() and g1.tolist() == g2.tolist() and len(o1) >= 1 and np.array_equal(rep.covered(0), l1)
        with pytest.raises(hs_mod.capi.SlamhipError) as e:
            proc.ViewGain(scan, world, 0, 0)
        assert e.value.code == hs_mod.capi.ERR_INVALID
    finally:
        proc.Dispose()
