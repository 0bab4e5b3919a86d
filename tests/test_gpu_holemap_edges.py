"""K2, the HoleMap update, at its edges -- the cases of tests/k2_cases.py (each checked on the CPU for the property it claims and
against both oracles: tests/test_k2_cases_cpu.py) on the device.  After every step the blended pixel count and the whole downloaded
map are compared with the literal loop of the C oracle; every comparison is == on the whole uint16 map.

A subset spanning every group runs three more ways: fused (search_and_update with all-zero jitters -- the kernel decodes the winner's
key and forms (px, py, c, s) itself), with a host mirror kept (no arcs, k2_row_spans; the mirror must equal the download), and back
to back with another case on one device object.  The kernel's environment switches are read once per process, so the whole file
runs once more in a fresh interpreter under each of VARIANTS.  Left out of the variant runs: BIG_NAMES, the two cases on a map of
16 384^2 pixels, and nothing else.  Geometry claims are asserted on the CPU only; here only equality with the oracle is.
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import k2_cases as kc
from test_gpu_coreslam import cs_mod, ctx, det                           # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

VARIANTS = [{"SLAMHIP_K2_NCORE": "0"}, {"SLAMHIP_K2_ZONE": "48", "SLAMHIP_K2_RB": "5"}, {"SLAMHIP_K2_ZONE": "200", "SLAMHIP_K2_RB": "30"},
            {"SLAMHIP_K2_GRID": "16"}, {"SLAMHIP_K2_GRID": "64"}, {"SLAMHIP_K2_TWO_LAUNCHES": "1"}]
IN_VARIANT = any(k in os.environ for v in VARIANTS for k in v)
BIG_NAMES = [c.name for c in kc.CASES if "big" in c.claims]              # division_16384, arc_sane_16384
NAMES = [c.name for c in kc.CASES if not (IN_VARIANT and c.name in BIG_NAMES)]
SUBSET = ["rays_2048", "rays_2049", "central_inside_v_shuffled", "count_q255", "mixed_47_48_mid", "mixq_overflow", "cand_65", "far_c5_h3_o1",
          "fan_c1_shuffled", "diagonal_shared_q2", "arc_margin", "own_849", "v_derrorv_65501", "borders_300"]
K = 64                                                                   # candidates of the fused scans: all the base pose


def same(got, ref, what):
    got, ref = np.asarray(got).ravel(), np.asarray(ref).ravel()
    bad = np.flatnonzero(got != ref)
    assert bad.size == 0, (what, bad.size, bad[:8], got[bad[:8]], ref[bad[:8]])


@pytest.fixture(scope="module")
def devs(cs_mod, ctx):
    """One device object per HoleMap size, one pixel per metre."""
    cache = {}

    def get(size):
        if size not in cache:
            if size >= kc.BIG:                                           # (half a gigabyte each: one at a time)
                for s in [s for s in cache if s >= 2048]:
                    cache.pop(s).close()
            d = cs_mod.CoreSlamDevice(ctx, float(size), size, 64)
            assert d.hole_scale == 1.0
            d.set_offsets(np.zeros((K - 1, 3), np.float32))
            cache[size] = d
        return cache[size]
    yield get
    for d in cache.values():
        d.close()


_REF = {}


def reference(name, oc):
    """The C oracle's pixel count and map after every step of the case, computed once and left unchanged (the 16 384^2 cases: not
    kept, half a gigabyte a step -- test_case walks them step by step)."""
    if name not in _REF:
        b = kc.by_name(name).build()
        pix = np.full(b.size * b.size, kc.START, np.uint16) if b.start is None else b.start.copy()
        out = []
        for st in b.steps:
            n = oc.update_holemap_pxcs(pix, b.size, 1.0, *st)
            out.append((n, pix.copy()))
        _REF[name] = (b, out)
    return _REF[name]


def upload(dev, b):
    dev.holemap_upload(np.full(b.size * b.size, kc.START, np.uint16) if b.start is None else b.start)


@pytest.mark.parametrize("name", NAMES)
def test_case(devs, det, name):
    if name in BIG_NAMES:
        b = kc.by_name(name).build()
        dev = devs(b.size)
        want = np.full(b.size * b.size, kc.START, np.uint16)
        upload(dev, b)
        for k, st in enumerate(b.steps):
            dev.set_scan(st[0])
            dev.update_holemap_pxcs(st[1], st[2], st[3])
            assert dev.last_holemap_pixels == det.update_holemap_pxcs(want, b.size, 1.0, *st), (name, k)
            assert np.array_equal(dev.holemap_download(), want), (name, k)
        return
    b, ref = reference(name, det)
    dev = devs(b.size)
    upload(dev, b)
    for k, (st, (n, want)) in enumerate(zip(b.steps, ref)):
        dev.set_scan(st[0])
        dev.update_holemap_pxcs(st[1], st[2], st[3])
        assert dev.last_holemap_pixels == n, (name, k)
        same(dev.holemap_download(), want, (name, k))


@pytest.mark.parametrize("name", SUBSET)
def test_fused(devs, det, name):
    """The same steps through search_and_update: the winner is the base pose (x1, y1, 0), whose (px, py, c, s) are the case's."""
    b, ref = reference(name, det)
    dev = devs(b.size)
    upload(dev, b)
    for k, (st, (n, want)) in enumerate(zip(b.steps, ref)):
        pose = np.array([float(st[1][0]) - 0.5, float(st[1][1]) - 0.5, 0.0], np.float32)
        assert (det.pose_to_pxcs(pose, 1.0) == st[1]).all()
        dev.set_scan(st[0])
        got, _, idx = dev.search_and_update(pose, st[2], st[3], 10)
        assert idx == 0 and (got == pose).all(), (idx, got, pose)
        assert dev.last_holemap_pixels == n, (name, k)
        same(dev.holemap_download(), want, (name, k))


@pytest.mark.parametrize("name", SUBSET)
def test_mirror(devs, det, name):
    """With a host mirror kept (asynchronous: the updates keep row spans, and no arcs): the mirror equals the download after every
    step, and a synchronous refresh at the end does."""
    b, ref = reference(name, det)
    dev = devs(b.size)
    upload(dev, b)
    mirror = np.zeros(b.size * b.size, np.uint16)
    try:
        dev.holemap_mirror_async(mirror)
        dev.holemap_mirror_wait()
        for k, (st, (n, want)) in enumerate(zip(b.steps, ref)):
            dev.set_scan(st[0])
            dev.update_holemap_pxcs(st[1], st[2], st[3])
            dev.holemap_mirror_async(mirror)
            dev.holemap_mirror_wait()
            got = dev.holemap_download()
            same(mirror, got, (name, k, "mirror"))
            same(got, want, (name, k))
        dev.set_scan(b.steps[0][0])
        dev.update_holemap_pxcs(*b.steps[0][1:])
        dev.holemap_mirror(mirror)
        same(mirror, dev.holemap_download(), (name, "synchronous mirror"))
    finally:
        dev.holemap_mirror_release()


@pytest.mark.parametrize("a,b_", list(zip(SUBSET, SUBSET[1:] + SUBSET[:1])))
def test_back_to_back(devs, det, a, b_):
    """Two different cases on one device object, the second case's steps right behind the first one's last."""
    ba, _ = reference(a, det)
    bb, ref = reference(b_, det)
    dev = devs(bb.size)
    # the first case's last scan on the second case's map: only the device object's state at rest matters
    dev.set_scan(ba.steps[-1][0])
    dev.update_holemap_pxcs(kc.pxcs_at(bb.size // 2, bb.size // 3), ba.steps[-1][2], ba.steps[-1][3])
    upload(dev, bb)
    for k, (st, (n, want)) in enumerate(zip(bb.steps, ref)):
        dev.set_scan(st[0])
        dev.update_holemap_pxcs(st[1], st[2], st[3])
        assert dev.last_holemap_pixels == n, (b_, k)
        same(dev.holemap_download(), want, (a, b_, k))


if not IN_VARIANT:                                                       # (a variant run starts no variant runs)
    def test_variants():
        """The whole file in fresh interpreters, one after the other, under each of VARIANTS; stops at the first that does not exit 0."""
        here = os.path.abspath(__file__)
        for env in VARIANTS:
            t0 = time.time()
            r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "pytest", here, "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider"],
                               env=dict(os.environ, **env), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
            out = r.stdout.decode(errors="replace")
            print(env, "%.1f s" % (time.time() - t0), out.strip().splitlines()[-1:] if out.strip() else "")
            assert r.returncode == 0 and " passed" in out and "failed" not in out, (env, out[-3000:])
