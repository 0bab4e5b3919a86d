"""Consecutive enqueue-only searches (slamhip_cs_search_shard_enqueue) overlap on the device: every other one runs in the context's
side stream (csrc/distance.hip, cs_launch_distance).  What that can break -- a result word written across streams, accumulator sets
that meet, an input rewritten under a search that still reads it, a join that is missing in one direction, a plan slot reused too
early -- is checked here against the C oracle under deterministic trigonometry, == everywhere, on 64^2 / 256^2 maps with 90 / 360
rays and 2049 candidates.

The ring has four result words, each valid until three further ring launches have been enqueued (slamhip.h: in ring mode the third
one rests it).  The overlapping launches store their key and rest nothing, so of a queue that was never synchronised the last FOUR
words are read -- the fourth from the end is the one a launch that wrongly rested a word would destroy -- and the last THREE under
SLAMHIP_K1_OVERLAP=0 (ring mode).  Queues of 9, 8, 7 and 6 launches put every depth and both streams last.

The switches are read once per process: the file runs once more in a fresh interpreter under each of VARIANTS -- SLAMHIP_K1_OVERLAP=0
(every launch in the operator's stream, the path of before), SLAMHIP_K1_PLAN_ALWAYS=1 (a plan for every launch: most arrive late) and
SLAMHIP_K1_VERIFY=1 (every end point checked against its tile).  selfcheck_failures == 0 at the end of every test.
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import k1_cases as kc
from test_gpu_coreslam import cs_mod, ctx, det                           # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

VARIANTS = [{"SLAMHIP_K1_OVERLAP": "0"}, {"SLAMHIP_K1_PLAN_ALWAYS": "1"}, {"SLAMHIP_K1_VERIFY": "1"}]
VARIANT_KEYS = sorted({k for v in VARIANTS for k in v})
IN_VARIANT = any(k in os.environ for k in VARIANT_KEYS)
K = 2049
LIVE = 3 if os.environ.get("SLAMHIP_K1_OVERLAP") == "0" else 4         # words of an unread queue that still hold their keys (the module docstring)
PLAN_SLOTS = 8                                                           # K1_PLAN_SLOTS (csrc/cs_internal.h)
SHAPES = [(64, 90), (256, 360)]                                          # (map size, rays)
COUNTS = (1, 1025, 512, 2049, 3)                                         # partly filled last groups of 512 candidates


class World:
    """One map size: pattern map, two scans, two jitter lists, nine poses; the oracle's distances per (map, scan, list, pose), made
    once and kept."""

    def __init__(self, size, rays):
        rng = np.random.default_rng(7000 + size)
        self.size, self.rays = size, rays
        self.pix = kc.pattern(size)
        reach = size * 0.08
        self.scans = []
        for _ in range(2):
            ang = rng.uniform(0, 2 * np.pi, rays)
            rad = rng.uniform(0.2 * reach, reach, rays)
            self.scans.append(np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1).astype(np.float32))
        d = size / 85.0
        self.lists = [np.stack([rng.uniform(-d, d, K - 1), rng.uniform(-d, d, K - 1), rng.uniform(-0.3, 0.3, K - 1)], 1).astype(np.float32)
                      for _ in range(2)]
        c = size / 2.0
        self.poses = [np.array([c + 0.37 * i, c - 0.21 * i, 0.4 + 0.11 * i], np.float32) for i in range(9)]
        self._d = {}

    def dist(self, oc, pix, tag, si, li, pi):
        key = (tag, si, li, pi)
        if key not in self._d:
            self._d[key] = oc.search(pix.reshape(-1), self.size, 1.0, self.scans[si], self.poses[pi], self.lists[li])[3]
        return self._d[key]

    def key(self, oc, si, li, pi, count=K, pix=None, tag="pattern"):
        d = self.dist(oc, self.pix if pix is None else pix, tag, si, li, pi)
        return min(kc.key_of(d[j], j) for j in range(count))


_WORLDS = {}


def world(size, rays):
    if size not in _WORLDS:
        _WORLDS[size] = World(size, rays)
    return _WORLDS[size]


def fresh(cs_mod, ctx, w, si=0, li=0):
    dev = cs_mod.CoreSlamDevice(ctx, float(w.size), w.size, 64)
    assert dev.hole_scale == 1.0
    dev.holemap_upload(w.pix)
    dev.set_scan(w.scans[si])
    dev.set_offsets(w.lists[li])
    return dev


@pytest.mark.parametrize("size,rays", SHAPES)
def test_queue_of_different_poses(cs_mod, ctx, det, size, rays):
    """Queues of 9, 8, 7, 6 launches, a different pose for every launch, no synchronise in between: after ONE synchronise the last LIVE
    words hold the keys of their own poses; then a blocking search on the same handle (accumulator set 0 at rest, join taken)."""
    w = world(size, rays)
    dev = fresh(cs_mod, ctx, w)
    for n in (9, 8, 7, 6):
        slots = [dev.search_shard_enqueue(w.poses[i], 0, K) for i in range(n)]
        ctx.synchronize()
        for i in range(n - LIVE, n):
            assert dev.key_read(slots[i]) == w.key(det, 0, 0, i), (n, i)
    assert dev.search_shard(w.poses[4], 0, K) == w.key(det, 0, 0, 4)
    slots = [dev.search_shard_enqueue(w.poses[i], 0, K) for i in range(3)]     # (unread launches in flight behind a blocking call)
    assert dev.search_shard(w.poses[5], 0, K) == w.key(det, 0, 0, 5)
    assert [dev.key_read(s) for s in slots] == [w.key(det, 0, 0, i) for i in range(3)]
    assert dev.selfcheck_failures == 0
    dev.close()


@pytest.mark.parametrize("size,rays", SHAPES)
def test_queue_of_changing_counts(cs_mod, ctx, det, size, rays):
    """The same queues with K alternating 1, 1025, 512, 2049, 3 from launch to launch (every change regathers the evaluation list in the
    operator's stream under the searches of the side stream): both accumulator sets must come back to rest."""
    w = world(size, rays)
    dev = fresh(cs_mod, ctx, w)
    for n in (9, 8):
        counts = [COUNTS[(i + n) % len(COUNTS)] for i in range(n)]
        slots = [dev.search_shard_enqueue(w.poses[i], 0, counts[i]) for i in range(n)]
        ctx.synchronize()
        for i in range(n - LIVE, n):
            assert dev.key_read(slots[i]) == w.key(det, 0, 0, i, counts[i]), (n, i, counts[i])
    assert dev.search_shard(w.poses[2], 0, K) == w.key(det, 0, 0, 2)
    assert dev.selfcheck_failures == 0
    dev.close()


@pytest.mark.parametrize("lead", (0, 1))
def test_joins_in_both_directions(cs_mod, ctx, det, lead):
    """A new list, a new scan and a map update between enqueues, nothing synchronised by the test: the launch before each change saw
    the old input and the one after it the new -- with the launch before the change in the side stream (lead = 1) and in the
    operator's (lead = 0).  A HoleMap download right behind an enqueue and an update equals the oracle's map."""
    w = world(256, 360)
    dev = fresh(cs_mod, ctx, w)
    for i in range(lead):
        dev.search_shard_enqueue(w.poses[8], 0, K)
    a = dev.search_shard_enqueue(w.poses[0], 0, K)
    dev.set_offsets(w.lists[1])
    b = dev.search_shard_enqueue(w.poses[1], 0, K)
    assert (dev.key_read(a), dev.key_read(b)) == (w.key(det, 0, 0, 0), w.key(det, 0, 1, 1))
    a = dev.search_shard_enqueue(w.poses[2], 0, K)
    dev.set_scan(w.scans[1])
    b = dev.search_shard_enqueue(w.poses[3], 0, K)
    c = dev.search_shard_enqueue(w.poses[4], 0, K)
    assert (dev.key_read(a), dev.key_read(b), dev.key_read(c)) == (w.key(det, 0, 1, 2), w.key(det, 1, 1, 3), w.key(det, 1, 1, 4))
    ref = w.pix.copy().reshape(-1)
    det.update_holemap(ref, w.size, 1.0, w.scans[1], w.poses[6])
    a = dev.search_shard_enqueue(w.poses[5], 0, K)
    dev.update_holemap(w.poses[6])
    got_map = dev.holemap_download()
    b = dev.search_shard_enqueue(w.poses[7], 0, K)
    c = dev.search_shard_enqueue(w.poses[8], 0, K)
    assert (np.asarray(got_map).reshape(-1) == ref).all()
    assert dev.key_read(a) == w.key(det, 1, 1, 5)
    assert (dev.key_read(b), dev.key_read(c)) == (w.key(det, 1, 1, 7, pix=ref, tag="updated"), w.key(det, 1, 1, 8, pix=ref, tag="updated"))
    assert dev.selfcheck_failures == 0
    dev.close()


def test_two_handles_interleaved(cs_mod, ctx, det):
    """Two handles of one context (one side stream): interleaved queues, each handle's words hold its own keys."""
    w1, w2 = world(64, 90), world(256, 360)
    d1, d2 = fresh(cs_mod, ctx, w1), fresh(cs_mod, ctx, w2, 1, 1)
    s1, s2 = [], []
    for i in range(7):
        s1.append(d1.search_shard_enqueue(w1.poses[i], 0, K))
        s2.append(d2.search_shard_enqueue(w2.poses[8 - i], 0, K))
        if i == 3:
            s2.append(d2.search_shard_enqueue(w2.poses[0], 0, K))          # (the handles' ring positions part ways)
    ctx.synchronize()
    assert [d1.key_read(s) for s in s1[-LIVE:]] == [w1.key(det, 0, 0, i) for i in (3, 4, 5, 6)[-LIVE:]]
    assert [d2.key_read(s) for s in s2[-LIVE:]] == [w2.key(det, 1, 1, p) for p in (0, 4, 3, 2)[-LIVE:]]   # (the extra launch, then i = 4, 5, 6)
    assert d1.selfcheck_failures == 0 and d2.selfcheck_failures == 0
    d1.close(); d2.close()


def test_destroy_with_launches_in_flight(cs_mod, ctx, det):
    """A handle destroyed with its last two launches (one per stream) unread; a new one on the same context searches right."""
    w = world(256, 360)
    dev = fresh(cs_mod, ctx, w)
    for i in range(6):
        dev.search_shard_enqueue(w.poses[i], 0, K)
    dev.close()
    dev = fresh(cs_mod, ctx, w, 1, 0)
    s = [dev.search_shard_enqueue(w.poses[i], 0, K) for i in (1, 2)]
    assert [dev.key_read(x) for x in s] == [w.key(det, 1, 0, 1), w.key(det, 1, 0, 2)]
    assert dev.search_shard(w.poses[3], 0, K) == w.key(det, 1, 0, 3)
    assert dev.selfcheck_failures == 0
    dev.close()


def test_plans_keep_coming(cs_mod, ctx, det):
    """40 launches back to back (16 384 candidates and 1080 rays on the 256^2 map: a launch outlasts the host's two launch calls, so the
    host runs ahead).  A launch gets a plan when the search launch before it -- in whichever stream, by the started word of THAT stream
    -- has not started and a slot is free; a slot is free when a later launch of the stream of the launch that read it has started.
    Wrong bookkeeping per stream shows as plans skipped, as slots never free, or as one stream's launches going without.  Under
    SLAMHIP_K1_PLAN_ALWAYS=1 every one of the 40 gets a plan.  Otherwise all but the first few: the launches without a plan are the
    first of the queue (the device is idle) and those the device catches up with, and the host cannot be further ahead than the
    PLAN_SLOTS records allow -- as many launches as there are plan slots may go without: at least 40 - PLAN_SLOTS = 32 plans."""
    w = world(256, 360)
    dev = fresh(cs_mod, ctx, w)
    rng = np.random.default_rng(5)
    big = np.stack([rng.uniform(-3, 3, 16383), rng.uniform(-3, 3, 16383), rng.uniform(-0.3, 0.3, 16383)], 1).astype(np.float32)
    dev.set_offsets(big)
    ang, rad = rng.uniform(0, 2 * np.pi, 1080), rng.uniform(4.0, 20.0, 1080)
    xy = np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1).astype(np.float32)
    dev.set_scan(xy)
    want = det.search(w.pix.reshape(-1), w.size, 1.0, xy, w.poses[0], big)
    want = kc.key_of(want[2], want[0])
    assert dev.key_read(dev.search_shard_enqueue(w.poses[0], 0, 16384)) == want      # (the list is gathered, its launches have finished)
    before = dev.plan_stats
    slots = [dev.search_shard_enqueue(w.poses[0], 0, 16384) for _ in range(40)]
    after = dev.plan_stats
    ctx.synchronize()
    assert [dev.key_read(s) for s in slots[-LIVE:]] == [want] * LIVE
    moved = [int(a) - int(b) for a, b in zip(after, before)]
    print("plan_stats moved by", moved)
    assert moved[0] + moved[1] == 40 and moved[3] == 0, moved
    if os.environ.get("SLAMHIP_K1_PLAN_ALWAYS"):
        assert moved[0] == 40, moved
    elif os.environ.get("SLAMHIP_K1_PLAN", "1") != "0":
        assert moved[0] >= 40 - PLAN_SLOTS, moved
    assert dev.selfcheck_failures == 0
    dev.close()


if not IN_VARIANT:                                                       # (a variant run starts no variant runs)
    def test_variants():
        """The whole file in fresh interpreters, one after the other, under each of VARIANTS; stops at the first that does not exit 0."""
        here = os.path.abspath(__file__)
        for env in VARIANTS:
            t0 = time.time()
            r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-m", "pytest", here, "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider"],
                               env=dict(os.environ, **env), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
            out = r.stdout.decode(errors="replace")
            print(env, "%.1f s" % (time.time() - t0), out.strip().splitlines()[-1:] if out.strip() else "")
            assert r.returncode == 0 and " passed" in out and "failed" not in out, (env, out[-3000:])
