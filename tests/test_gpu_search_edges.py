"""K1, the scan-to-map distance and its arg-min, at its edges -- the cases of tests/k1_cases.py (each checked on the CPU against both
oracles and for what it claims about the tile steps: tests/test_k1_cases_cpu.py) on the device.  Every comparison is ==: all
distances, the index and the minimum through distance_pxcs (mode 0); distance_poses (mode 2) and search (mode 1) where the case has a pose
form (POSE_NAMES says which have none, and why); search_shard over uneven splits (every shard's key, and their minimum); search_shard_enqueue + key_read five launches back to
back (the ring of four wraps).  selfcheck_failures == 0 at the end of every test.

The kernel's environment switches are read once per process, so the whole file runs once more in a fresh interpreter under each of
VARIANTS.  Under SLAMHIP_K1_VERIFY=1 alone the per-kind counters (slamhip_cs_selfcheck_counts) are taken before and after the mode-0
launch of every case that claims step kinds: > 0 for a claimed kind, == 0 for the others.  Without VERIFY the counters do not move and
nothing is asserted on them; the variants that change the tile budget, the group size, the padding, the split or force global gathers
assert no kind (CLAIMS_HOLD_UNDER says which do).  Left out of the variant runs: VARIANT_SKIP (the 8192^2 map; the 513-group cases
but under VERIFY alone), nothing else.
"""
import os
import subprocess
import sys
import time
import zlib

import numpy as np
import pytest

import k1_cases as kc
from test_gpu_coreslam import cs_mod, ctx, det                           # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

VARIANTS = [{"SLAMHIP_K1_VERIFY": "1"}, {"SLAMHIP_K1_GLOBAL": "1"}, {"SLAMHIP_K1_TILE_KB": "1", "SLAMHIP_K1_VERIFY": "1"},
            {"SLAMHIP_K1_TILE_KB": "16", "SLAMHIP_K1_VERIFY": "1"}, {"SLAMHIP_K1_NODEN": "1"},
            {"SLAMHIP_K1_GROUP": "2048"},         # (SLAMHIP_K1_GROUP=512 is not run: every list here has at most 12 288 candidates, whose mode-1 groups are 512 by default)
            {"SLAMHIP_K1_NOPAD": "1"}, {"SLAMHIP_K1_NOSPLIT": "1"}, {"SLAMHIP_K1_NOBOUNDS": "1"},
            {"SLAMHIP_K1_PLAN_ALWAYS": "1"}]
VARIANT_KEYS = sorted({k for v in VARIANTS for k in v})
IN_VARIANT = any(k in os.environ for k in VARIANT_KEYS)
# the step kinds a case claims hold at the default budget, padding and split, for explicit lists (always 1024-candidate groups): the
# counters are asserted in the run whose only switch is VERIFY
CLAIMS_HOLD_UNDER = [{"SLAMHIP_K1_VERIFY": "1"}]
COUNTERS_ASSERTED = {k: os.environ[k] for k in VARIANT_KEYS if k in os.environ} in CLAIMS_HOLD_UNDER
HUGE_MAP = [c.name for c in kc.CASES if c.name.startswith("i_address_8192")]           # a 128 MiB upload each
MANY_GROUPS = [c.name for c in kc.CASES if c.claims.get("many_groups")]                  # 525 312 candidates: 2.5 s of reference each
# left out of the variant runs, and nothing else: the 8192^2 map everywhere; the 513-group cases everywhere but in the run whose only
# switch is VERIFY (their point is the piece length, which only the counters of that run confirm)
VARIANT_SKIP = (HUGE_MAP + ([] if COUNTERS_ASSERTED else MANY_GROUPS)) if IN_VARIANT else []
NAMES = [c.name for c in kc.CASES if c.name not in VARIANT_SKIP]
# no pose form: rotations (seeded, quarter turns), -0.0, a single candidate; the 513-group cases are explicit lists only (a mode-1 list of
# that size takes 2048-candidate groups and many ranges: not the piece they are built for)
POSE_NAMES = [n for n in NAMES if kc.by_name(n).group != "S" and not n.startswith(("a_turn", "a_negzero")) and n != "g_count_1" and n not in MANY_GROUPS]


def same(got, ref, what):
    got, ref = np.asarray(got).ravel(), np.asarray(ref).ravel()
    bad = np.flatnonzero(got != ref)
    assert bad.size == 0, (what, bad.size, bad[:8], got[bad[:8]], ref[bad[:8]])


@pytest.fixture(scope="module")
def devs(cs_mod, ctx):
    """One device object per HoleMap size, one pixel per metre; the map last uploaded is remembered by the case that built it."""
    cache = {}

    def get(size):
        if size not in cache:
            if size >= 4096:                                             # (one large map at a time)
                for s in [s for s in cache if s >= 4096]:
                    cache.pop(s)[0].close()
            d = cs_mod.CoreSlamDevice(ctx, float(size), size, 64)
            assert d.hole_scale == 1.0
            cache[size] = [d, None]
        return cache[size]
    yield get
    for d, _ in cache.values():
        d.close()


_EXP = {}


def reference(name):
    """(built, (distances, index, minimum)) by the restated rule, computed once and left unchanged (the big cases: not kept)."""
    if name in _EXP:
        return _EXP[name]
    b = kc.by_name(name).build()
    out = (b, kc.expected(b))
    if name in HUGE_MAP + MANY_GROUPS:                                   # (only the last of these is kept)
        for n in [n for n in _EXP if n in HUGE_MAP + MANY_GROUPS]:
            del _EXP[n]
    _EXP[name] = out
    return out


def prepared(devs, name, b):
    """The case's map and scan on the device object of its size."""
    slot = devs(b[0])
    dev = slot[0]
    map_key = zlib.crc32(np.ascontiguousarray(b[1]).data)
    if slot[1] != map_key:
        dev.holemap_upload(b[1])
        slot[1] = map_key
    dev.set_scan(b[2])
    return dev


def shard_cuts(K):
    return sorted({0, 1, K // 3, min(K, 1023), min(K, 1025), K - 1, K} - {-1})


def shard_keys(dist, a, b):
    return min(kc.key_of(dist[j], j) for j in range(a, b))


# ---- mode 0: every case ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_pxcs(devs, name):
    b, (dist, idx, best) = reference(name)
    dev = prepared(devs, name, b)
    claims = kc.by_name(name).claims
    before = dev.selfcheck_counts if COUNTERS_ASSERTED and "kinds" in claims else None
    got, gi, gd = dev.distance_pxcs(b[3])
    same(got, dist, name)
    assert (gi, gd) == (idx, best), name
    if before is not None:
        after = dev.selfcheck_counts
        for kind, word in kc.COUNTER_WORD.items():
            moved = after[word] - before[word]
            assert (moved > 0) if kind in claims["kinds"] else (moved == 0), (name, kind, moved, claims["kinds"])
            if "one_piece_of" in claims and kind in claims["kinds"]:     # one step of that many rays in every workgroup, 4 units per ray
                assert moved == 4 * claims["one_piece_of"] * (b[3].shape[0] // 1024), (name, moved)
    gi2, gd2 = dev.distance_pxcs(b[3], want_all=False)[1:]               # (the same scan searched again: ray ranges may be cut by cost)
    assert (gi2, gd2) == (idx, best), name
    assert dev.selfcheck_failures == 0


# ---- modes 2 and 1: the pose form ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", POSE_NAMES)
def test_poses_and_search(devs, name):
    b, (dist, idx, best) = reference(name)
    pose, offs, poses = kc.pose_form(b)
    dev = prepared(devs, name, b)
    got, gi, gd = dev.distance_poses(poses)
    same(got, dist, (name, "poses"))
    assert (gi, gd) == (idx, best), name
    dev.set_offsets(offs)
    for k in range(2):
        gpose, gd, gi = dev.search(pose)
        assert (gi, gd) == (idx, best) and (gpose == poses[idx]).all(), (name, k, gi, gd, idx, best)
    rpose, rep = dev.search_report(pose)
    assert (int(rep["best_index"]), int(rep["best_dist"])) == (idx, best)
    same(dev.search_distances(), dist, (name, "search"))
    assert dev.selfcheck_failures == 0


@pytest.mark.parametrize("name", POSE_NAMES)
def test_shards(devs, name):
    """search_shard over uneven splits: every shard's key is the minimum of its candidates' keys, and their minimum the search's."""
    b, (dist, idx, best) = reference(name)
    pose, offs, poses = kc.pose_form(b)
    dev = prepared(devs, name, b)
    dev.set_offsets(offs)
    K = poses.shape[0]
    cuts = shard_cuts(K)
    keys = []
    for a, e in zip(cuts[:-1], cuts[1:]):
        keys.append(dev.search_shard(pose, a, e - a))
        assert keys[-1] == shard_keys(dist, a, e), (name, a, e)
    assert min(keys) == kc.key_of(best, idx)
    assert dev.selfcheck_failures == 0


@pytest.mark.parametrize("name", POSE_NAMES)
def test_enqueue_ring(devs, name):
    """Five enqueue-only launches back to back (the ring has four slots), read afterwards and one at a time."""
    b, (dist, idx, best) = reference(name)
    pose, offs, poses = kc.pose_form(b)
    dev = prepared(devs, name, b)
    dev.set_offsets(offs)
    K = poses.shape[0]
    parts = [(0, K), (0, K), (K // 3, K - K // 3), (0, max(K // 3, 1)), (0, K)]
    slots = [dev.search_shard_enqueue(pose, a, n) for a, n in parts]
    assert len(set(slots)) == 4 and slots[4] == slots[0]
    for i in (2, 3, 4):                                                  # (launch 4 took slot 0 again and rested slot 1)
        assert dev.key_read(slots[i]) == shard_keys(dist, parts[i][0], parts[i][0] + parts[i][1]), (name, i)
    for a, n in parts:
        assert dev.key_read(dev.search_shard_enqueue(pose, a, n)) == shard_keys(dist, a, a + n), (name, a, n)
    assert dev.search_shard(pose, 0, K) == kc.key_of(best, idx)
    assert dev.selfcheck_failures == 0


# ---- mode-1 ties: equal minima whose headings sort the later flat index first ------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in kc.T_CASES])
def test_mode1_ties(devs, name):
    """The device evaluates mode-1 candidates in theta order; the winner among equal minima is still the smallest FLAT index -- through
    search, the report and its distances, the shards and the ring."""
    tc = kc.t_by_name(name)
    b, pose, offs = kc.tie_heading_form(tc)
    dist, idx, best = kc.expected(b)                                     # (== the C oracle's search with these jitters: the CPU test)
    dev = prepared(devs, tc.base, b)
    dev.set_offsets(offs)
    want = np.array([pose[0], pose[1], pose[2]], np.float32) + (np.concatenate([np.zeros((1, 3), np.float32), offs])[idx])
    for k in range(2):
        gpose, gd, gi = dev.search(pose)
        assert (gi, gd) == (idx, best) and (gpose == want.astype(np.float32)).all(), (name, k, gi, gd, idx, best)
    rpose, rep = dev.search_report(pose)
    assert (int(rep["best_index"]), int(rep["best_dist"])) == (idx, best) and int(rep["n_ties"]) == int((dist == best).sum())
    same(dev.search_distances(), dist, name)
    K = offs.shape[0] + 1
    cuts = shard_cuts(K)
    keys = [dev.search_shard(pose, a, e - a) for a, e in zip(cuts[:-1], cuts[1:])]
    assert keys == [shard_keys(dist, a, e) for a, e in zip(cuts[:-1], cuts[1:])] and min(keys) == kc.key_of(best, idx)
    slots = [dev.search_shard_enqueue(pose, 0, K) for _ in range(5)]
    assert [dev.key_read(slots[i]) for i in (2, 3, 4)] == [kc.key_of(best, idx)] * 3
    assert dev.selfcheck_failures == 0


# ---- G: candidate counts back to back on ONE handle ------------------------------------------------------------------------------------
def test_counts_back_to_back(devs):
    """Descending then ascending K on one handle: an accumulator or minimum word that the clamped lanes of a partly filled group left
    unrested shows in the next launch.  Mode 0, then mode 1 (512-candidate groups by default), then the ring."""
    order = sorted(kc.G_COUNTS, reverse=True) + sorted(kc.G_COUNTS)
    dev = None
    for K in order:
        name = "g_count_%d" % K
        b, (dist, idx, best) = reference(name)
        dev = prepared(devs, name, b)
        got, gi, gd = dev.distance_pxcs(b[3])
        same(got, dist, (name, "pxcs"))
        assert (gi, gd) == (idx, best) and idx == K - 1, name
        if K >= 2:
            pose, offs, poses = kc.pose_form(b)
            dev.set_offsets(offs)
            gpose, gd, gi = dev.search(pose)
            assert (gi, gd) == (idx, best), (name, "search")
            assert dev.key_read(dev.search_shard_enqueue(pose, 0, K)) == kc.key_of(best, idx), (name, "ring")
    assert dev.selfcheck_failures == 0


# ---- H: bounds from the jitter ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hdev(cs_mod, ctx):
    d = cs_mod.CoreSlamDevice(ctx, 256.0, 256, 64)
    assert d.hole_scale == 1.0
    d.holemap_upload(kc.pattern(256))
    yield d
    d.close()


@pytest.mark.parametrize("name", [c.name for c in kc.H_CASES])
def test_jitter_bounds(hdev, det, name):
    """Mode 1 against the C oracle under deterministic trigonometry: the winner, every distance, and the shards' keys."""
    c = kc.h_by_name(name)
    assert c.size == 256
    pix = kc.pattern(c.size).reshape(-1)
    bi, bpose, bd, all_d = det.search(pix, c.size, 1.0, c.xy, c.pose, c.offs)
    hdev.set_scan(c.xy)
    hdev.set_offsets(c.offs)
    for k in range(2):
        gpose, gd, gi = hdev.search(c.pose)
        assert (gi, gd) == (bi, bd) and (gpose == bpose).all(), (name, k)
    hdev.search_report(c.pose)
    same(hdev.search_distances(), all_d, name)
    K = c.offs.shape[0] + 1
    keys = [hdev.search_shard(c.pose, a, e - a) for a, e in ((0, 1), (1, K // 2), (K // 2, K))]
    assert min(keys) == kc.key_of(bd, bi)
    assert hdev.selfcheck_failures == 0


if not IN_VARIANT:                                                       # (a variant run starts no variant runs)
    def test_variants():
        """The whole file in fresh interpreters, one after the other, under each of VARIANTS; stops at the first that does not exit 0."""
        here = os.path.abspath(__file__)
        for env in VARIANTS:
            t0 = time.time()
            r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-m", "pytest", here, "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider"],
                               env=dict(os.environ, **env), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
            out = r.stdout.decode(errors="replace")
            print(env, "%.1f s" % (time.time() - t0), out.strip().splitlines()[-1:] if out.strip() else "")
            assert r.returncode == 0 and " passed" in out and "failed" not in out, (env, out[-3000:])
