"""What the Hector units K7 .. K27 share on the host (hs_blocks.h): blocks that grow and are then reused while larger than the call
needs, the one event every blocking call of an hs records and waits on, units made on first use and freed with the hs or by their
*_clear entry point -- every block of theirs, by the count of live blocks (slamhip_debug_live_blocks) -- and a unit whose first
call is refused.  Every result is compared with == (field by field, floats by their bits) against the SAME call on a
fresh hs that holds the same map; nothing is compared with an earlier result of the object under test.

Shapes: the 80 x 48 x 2 pyramid of the K9 tests' `small` fixture, holding a room -- walls, a free inside with a pillar, the unknown
around it, a gap in the wall where free cells touch the unknown -- and a scan of 65 points, a wavefront and one lane more."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_hector_lattice as L
from test_gpu_hector_shift import hs_mod, ctx                              # noqa: F401 (fixtures)

gpu = pytest.mark.gpu
F = np.float32
W0, H0, LEVELS, CELL = 80, 48, 2, 0.1
FULL = (0, 0, W0, H0)


def room_values(level):
    w, h = W0 >> level, H0 >> level
    k = 1 if level else 2                                                  # level 1 halves every coordinate
    v = np.zeros((h, w), F)
    v[3 * k:21 * k, 4 * k:36 * k] = 1.0                                    # the walls ...
    v[3 * k + 1:21 * k - 1, 4 * k + 1:36 * k - 1] = -1.0                   # ... and the free inside
    v[10 * k:12 * k, 15 * k:17 * k] = 1.0                                  # a pillar
    v[3 * k, 20 * k:22 * k] = -1.0                                         # a gap: free cells that touch the unknown
    return v.ravel()


_RNG = np.random.default_rng(19)
_ANG = np.linspace(-math.pi, math.pi, 65, endpoint=False)
SCAN_XY = (np.stack([np.cos(_ANG), np.sin(_ANG)], 1) * _RNG.uniform(0.3, 2.5, (65, 1))).astype(F)


def poses(n):
    """n poses inside the room, the same first ones for every n."""
    rng = np.random.default_rng(23)
    return np.stack([rng.uniform(1.0, 7.0, n), rng.uniform(0.8, 4.0, n), rng.uniform(-math.pi, math.pi, n)], 1).astype(F)


def make(hs_mod, ctx):
    rep = hs_mod.MapRepMultiMap(CELL, (W0, H0), LEVELS, ctx=ctx)
    for level in range(LEVELS):
        L.put_values(hs_mod, rep, level, room_values(level))
    rep.set_scan(hs_mod.ScanCloud(SCAN_XY))
    return rep


# ---- the calls: name -> f(hs_mod, rep, level), one per size the tests use -------------------------------------------------------------
SOURCES = [(60, 30)]
GOALS = [(12, 10, 14, 12), (40, 30, 44, 34), (66, 8, 70, 12), (0, 0, 3, 3)]   # three in the room, one in the unknown
START, DT, BODY = (2.0, 2.0, 0.3), 0.1, [(0.15, 0.0), (-0.1, 0.1)]


def cmds(B):
    rng = np.random.default_rng(29)
    return np.stack([rng.uniform(0.0, 1.5, (B, 4)), rng.uniform(-1.0, 1.0, (B, 4))], 2).astype(F)


def mcl_spec(hs_mod, level, N):
    return hs_mod.capi.mcl_spec(level, 8, (0.05, 0.0, 0.01), (0.02, 0.02, 0.01), hs_mod.capi.mcl_beta(2.0), N, seed=5, stream=N)


def mcl(hs_mod, rep, level, N):
    rep.mcl_set(poses(N))
    return rep.mcl_step(mcl_spec(hs_mod, level, N)), rep.mcl_get()


CALLS = {
    "k7_1": lambda m, r, l: r.lattice_search(None, l, (2.0, 2.0, 0.1), 3, 2, 1, 0.2, scores=False),
    "k7_8s": lambda m, r, l: r.lattice_search(None, l, (2.0, 2.0, 0.1), 3, 2, 8, 0.2, scores=True),
    "k10": lambda m, r, l: r.frontiers(l),
    "k10_labels": lambda m, r, l: r.frontiers(l, labels_rect=FULL),
    "k11": lambda m, r, l: r.nav_field(l, SOURCES, clearance=1),
    "k11_full": lambda m, r, l: r.nav_field(l, SOURCES, clearance=1, goals=GOALS, n_paths=2, max_path_cells=64, rect=FULL),
    "k12_1": lambda m, r, l: r.rollouts(l, SOURCES, START, DT, cmds(1), hold=2, body=BODY, clearance=1),
    "k12_4096": lambda m, r, l: r.rollouts(l, SOURCES, START, DT, cmds(4096), hold=2, body=BODY, clearance=1),
    "k13_1": lambda m, r, l: mcl(m, r, l, 1),
    "k13_300": lambda m, r, l: mcl(m, r, l, 300),
    "k13_2": lambda m, r, l: mcl(m, r, l, 2),
}
for _B in (1, 300, 2):
    for _rec in (False, True):
        CALLS["k8_%d%s" % (_B, "r" if _rec else "")] = lambda m, r, l, B=_B, rec=_rec: r.trace(poses(B), l, beams=rec)
        CALLS["k9_%d%s" % (_B, "r" if _rec else "")] = lambda m, r, l, B=_B, rec=_rec: r.distance_score(poses(B), l, radius=8, points=rec)
ORDER = ["k7_8s", "k8_300r", "k9_300r", "k10_labels", "k11_full", "k12_4096", "k13_300"]   # the seven units, K7 .. K13


def same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is b
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.names:
        return all(a[n].tobytes() == b[n].tobytes() for n in a.dtype.names)
    return a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def ref(hs_mod, ctx):
    """ref(name): the call on an hs of its own, made for it and destroyed behind it; computed once per name."""
    memo = {}

    def get(name):
        if name not in memo:
            rep = make(hs_mod, ctx)
            memo[name] = CALLS[name](hs_mod, rep, 0)
            rep.close()
        return memo[name]
    return get


def check(hs_mod, rep, ref, names, reset_scan=False):
    for name in names:
        if reset_scan:
            rep.set_scan(hs_mod.ScanCloud(SCAN_XY))                       # (the other device block of the scan: its books follow the calls' waits)
        assert same(CALLS[name](hs_mod, rep, 0), ref(name)), name


def test_the_yardstick_tells_results_apart():
    a = np.zeros(2, [("n", np.int32), ("x", F)])
    b = a.copy(); b["x"][1] = F(-0.0)
    assert same((a, None, {"k": [a]}), (a.copy(), None, {"k": [a.copy()]}))
    assert not same(a, b) and not same(a, None) and not same((a,), (a, a)) and not same(a, a.astype([("n", np.int32), ("x", np.float64)]))


# ---- 1. grow, then reuse a larger block ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("names", [("k8_1", "k8_300", "k8_2"), ("k8_1r", "k8_300r", "k8_2r"), ("k9_1", "k9_300", "k9_2"), ("k9_1r", "k9_300r", "k9_2r"),
                                   ("k7_1", "k7_8s", "k7_1"), ("k10", "k10_labels", "k10"), ("k11", "k11_full", "k11"),
                                   ("k12_1", "k12_4096", "k12_1"), ("k13_1", "k13_300", "k13_2")], ids=lambda n: n[1])
def test_small_large_small(hs_mod, ctx, ref, names):
    rep = make(hs_mod, ctx)
    check(hs_mod, rep, ref, names)
    rep.close()


@gpu
def test_results_are_worth_comparing(ref):
    sums, beams = ref("k8_300r")
    assert beams.shape == (300, 65) and (sums["n_walked"] > 0).all() and len(np.unique(beams["first"])) > 4
    sums, pts = ref("k9_300r")
    assert pts.shape == (300, 65) and len(np.unique(pts)) > 8
    keys, vol = ref("k7_8s")
    assert vol.shape == (8, 5, 7) and len(np.unique(vol)) > 4
    summary, clusters, labels = ref("k10_labels")
    assert summary["n_frontier_cells"] > 0 and len(clusters) >= 1 and (labels >= 0).sum() == summary["n_frontier_cells"]
    nav = ref("k11_full")
    assert nav["summary"]["n_reached"] > 1000 and len(nav["paths"][0]) > 10 and nav["goals"]["n_reached"][3] == 0
    res, summary = ref("k12_4096")
    assert 0 < summary["n_complete"] < 4096 and len(np.unique(res["n_free"])) > 2
    s, (p, acc, anc) = ref("k13_300")
    assert s["n_particles"] == 300 and s["cost_max"] > s["cost_min"] and p.shape == (300, 3)


# ---- 2. the seven units on one event ---------------------------------------------------------------------------------------------------
@gpu
def test_interleaved_units(hs_mod, ctx, ref):
    rep = make(hs_mod, ctx)
    check(hs_mod, rep, ref, ORDER, reset_scan=True)
    check(hs_mod, rep, ref, ORDER[::-1], reset_scan=True)
    # K12 directly after K13 and K11 directly after K9: the pairs share the field's and the class map's blocks
    check(hs_mod, rep, ref, ["k13_300", "k12_4096", "k9_300r", "k11_full", "k13_2", "k12_1", "k9_1", "k11"])
    rep.close()


# ---- 3. create and destroy -------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("used", [[], ["k13_300"], ORDER], ids=["none", "k13", "all"])
def test_create_and_destroy(hs_mod, ctx, ref, used):
    for name in used:
        ref(name)                                                          # (its own hs is gone before the baseline is read)
    base = hs_mod.capi.live_blocks()
    rep = make(hs_mod, ctx)
    check(hs_mod, rep, ref, used)
    live = hs_mod.capi.live_blocks()
    assert (live[0] > base[0] and live[1] > base[1]) if used else live == base, (base, live)
    rep.close()
    assert hs_mod.capi.live_blocks() == base
    rep = make(hs_mod, ctx)
    check(hs_mod, rep, ref, ["k8_300r"])
    rep.close()


# ---- 4. a unit whose first call is refused ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", ORDER)
def test_refused_first_use(hs_mod, ctx, ref, name):
    ref(name)                                                              # (its own hs is gone before the baseline is read)
    base = hs_mod.capi.live_blocks()
    rep = make(hs_mod, ctx)
    # level = n_levels; K13's set takes no level, so its first use is the refused step itself
    refused = CALLS[name] if name != "k13_300" else lambda m, r, l: r.mcl_step(mcl_spec(m, l, 300))
    with pytest.raises(hs_mod.capi.SlamhipError) as e:
        refused(hs_mod, rep, LEVELS)
    assert e.value.code == hs_mod.capi.ERR_INVALID and "level %d of %d" % (LEVELS, LEVELS) in str(e.value)
    check(hs_mod, rep, ref, [name])
    rep.close()
    assert hs_mod.capi.live_blocks() == base


@gpu
@pytest.mark.parametrize("name", ORDER)
def test_refused_first_use_then_close(hs_mod, ctx, name):
    base = hs_mod.capi.live_blocks()
    rep = make(hs_mod, ctx)
    refused = CALLS[name] if name != "k13_300" else lambda m, r, l: r.mcl_step(mcl_spec(m, l, 300))
    with pytest.raises(hs_mod.capi.SlamhipError):
        refused(hs_mod, rep, LEVELS)
    rep.close()
    assert hs_mod.capi.live_blocks() == base


# ---- 5. the *_clear entry points -------------------------------------------------------------------------------------------------------
# name -> (the unit used once at its smallest accepted input, its clear, the calls that warm what the unit shares with another one:
# K15 and K17 pack K7's class map, whose blocks are K7's and stay)
def _pg(m, r, l):
    r.PgSet([[0.0, 0.0, 0.0], [1.0, 0.1, 0.05]], None, [[0, 1]], [[1.1, 0.0, 0.0]], [[400.0, 400.0, 2500.0]])
    it, fin = r.PgRelax(m.capi.pg_spec(1, 3))
    return it, fin, r.PgGet()


def _scans(m, r, l):
    k = r.ScansAdd()
    return (k,) + tuple(r.ScansGet(k))


def _loops(m, r, l):
    return r.LoopsConsistent([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]], [[0, 1]], [[1.0, 0.0, 0.0]], [[400.0, 400.0, 2500.0]], m.capi.loops_spec(11.34, 1e-3, 1e-4))


CLEARS = {
    "hough": (lambda m, r, l: r.hough(l, T=4), lambda r: r.hough_clear(), ["k7_1"]),
    "pg": (_pg, lambda r: r.PgClear(), []),
    "scans": (_scans, lambda r: r.ScansClear(), []),
    "view": (lambda m, r, l: r.view_gain(poses(1), l, 8), lambda r: r.view_clear(), ["k7_1"]),
    "loops": (_loops, lambda r: r.LoopsClear(), []),
}


@gpu
@pytest.mark.parametrize("name", sorted(CLEARS))
def test_clear_frees_the_unit(hs_mod, ctx, ref, name):
    use, clear, warm = CLEARS[name]
    fresh = make(hs_mod, ctx)
    want = use(hs_mod, fresh, 0)
    fresh.close()
    rep = make(hs_mod, ctx)
    check(hs_mod, rep, ref, warm)
    before = hs_mod.capi.live_blocks()
    assert same(use(hs_mod, rep, 0), want)
    used = hs_mod.capi.live_blocks()
    assert used[0] > before[0] and used[1] > before[1], (before, used)
    clear(rep)
    assert hs_mod.capi.live_blocks() == before
    assert same(use(hs_mod, rep, 0), want)                                 # the unit works again
    assert hs_mod.capi.live_blocks() == used
    rep.close()


# ---- 6. the two stores that grow by a new allocation: K18's keyframes, K20's scan pool ---------------------------------------------------
POOL_ENV = {"SLAMHIP_K20_POOL_POINTS": "64"}                              # (read once per process: the pool of 65 points doubles at the second scan)


@gpu
def test_stores_regrow_child(hs_mod, ctx):
    """Run by test_stores_regrow_and_close with POOL_ENV set; on its own the scan pool has room and only the keyframe store grows."""
    capi = hs_mod.capi
    base = capi.live_blocks()
    rep = make(hs_mod, ctx)
    rep.SigConfigure(3.0, 5, 2)
    rep.SigAdd((0.0, 0.0, 0.0))
    rep.SigConfigure(3.0, 7, 2)                                            # another n_ring: the store is dropped and laid out anew
    _, sig0, _ = rep.SigAdd((1.0, 2.0, 3.0))
    live = capi.live_blocks()
    B = 16 * 64 + 6                                                        # past the first store of 16 blocks of 64 keyframes
    rep.SigAddScans([SCAN_XY[:3]] * B, np.zeros((B, 3), F))
    grown = capi.live_blocks()
    assert rep.SigCount() == B + 1 and grown[1] > live[1]
    sig, p = rep.SigDownload(0, 1)
    assert same(sig[0], sig0) and same(p[0], np.array([1.0, 2.0, 3.0], F))  # the old store is the new one's front
    for k in range(3):
        assert rep.ScansAdd() == k
        if k == 0:
            blocks = capi.live_blocks()[0]
    assert capi.live_blocks()[0] == blocks                                  # a larger pool replaces the old one
    for k in range(3):
        xy, org = rep.ScansGet(k)
        assert same(xy, SCAN_XY)
    rep.close()
    assert capi.live_blocks() == base


@gpu
def test_stores_regrow_and_close():
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-k", "stores_regrow_child"],
                       env=dict(os.environ, **POOL_ENV), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and "1 passed" in out and "failed" not in out, out[-3000:]
