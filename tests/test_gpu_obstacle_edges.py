"""K3, the ObstacleMap update, at its edges -- the cases of tests/k3_cases.py (each checked on the CPU for the property it claims:
tests/test_k3_cases_cpu.py) on the device, in both places the update runs: stand-alone (k3_rays + k3_apply, through
update_obstaclemap_pxcs) and riding inside the wavefronts of the HoleMap update's launch (k2_ride_tail, through the fused
search_and_update).  Every comparison is == on the whole int8 map against the literal loop of the C oracle; no tolerance anywhere.

The riding path: only the fused search + update carries the ride (update_maps_pxcs and search_and_update_pxcs are compositions of
the stand-alone operators), so the cases ride through search_and_update with all-zero jitters -- the winner is the base pose -- on
a map of one cell per metre and the pose (x1, y1, 0), which gives exactly the case's (px, py, c, s) (asserted on the CPU).  Two
scans in a row each: the first scan's cell pass is pending when the second rides and is applied by it; the download applies the
second's.

Out of scope: the `i < 65536` half of the walk's width condition (k3_walk_iter) needs an ObstacleMap of 65 536^2 cells.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import k3_cases as kc
from test_gpu_coreslam import cs_mod, ctx, det                           # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

K = 64                                                                   # candidates of the fused scans: all the base pose
NAMES = [c.name for c in kc.CASES if "beyond_first_stride" not in c.claims]


def same(got, ref, what):
    got, ref = np.asarray(got).ravel(), np.asarray(ref).ravel()
    bad = np.flatnonzero(got != ref)
    assert bad.size == 0, (what, bad.size, bad[:8], got[bad[:8]], ref[bad[:8]])


@pytest.fixture(scope="module")
def devs(cs_mod, ctx):
    """One device object per (HoleMap size, ObstacleMap size, metres), one cell of the ObstacleMap per metre unless told otherwise."""
    cache = {}

    def get(osize, hsize=64, metres=None):
        key = (hsize, osize, metres)
        if key not in cache:
            d = cs_mod.CoreSlamDevice(ctx, float(osize if metres is None else metres), hsize, osize)
            if metres is None:
                assert d.obst_scale == 1.0
            d.set_offsets(np.zeros((K - 1, 3), np.float32))
            cache[key] = d
        return cache[key]
    yield get
    for d in cache.values():
        d.close()


def fused(dev, oc, ref, xy, pose, max_hits=10, set_scan=True):
    """One fused scan (the ObstacleMap update rides, its cell pass stays pending) and the oracle's update of `ref`."""
    if set_scan:
        dev.set_scan(xy)
    got, _, idx = dev.search_and_update(np.asarray(pose, np.float32), 0.6, 50, max_hits)
    want = np.array([pose[0], pose[1], oc.normalize_angle(pose[2])], np.float32)
    assert idx == 0 and (got == want).all(), (idx, got, want)
    oc.update_obstaclemap(ref, dev.obst_size, dev.obst_scale, xy, got, max_hits)


def random_scan(seed, R, reach):
    return np.random.default_rng(seed).integers(-reach, reach + 1, (R, 2)).astype(np.float32)


# ---- the cases, stand-alone and riding ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_standalone(devs, det, name):
    """k3_rays + k3_apply; two updates in a row (the scratch the first pass cleared is clear)."""
    oc = det
    size, start, xy, pxcs, max_hits = kc.by_name(name).build()
    dev = devs(size)
    dev.obstaclemap_upload(start)
    dev.set_scan(xy)
    ref = start.copy()
    for k in range(2):
        dev.update_obstaclemap_pxcs(pxcs, max_hits)
        oc.update_obstaclemap_pxcs(ref, size, xy, pxcs, max_hits)
        same(dev.obstaclemap_download(), ref, (name, k))


@pytest.mark.parametrize("name", NAMES)
def test_ride(devs, det, name):
    """The same case riding on the HoleMap update's launch, twice: the second scan's ride applies the first one's pending pass."""
    oc = det
    size, start, xy, pxcs, max_hits = kc.by_name(name).build()
    dev = devs(size)
    dev.obstaclemap_upload(start)
    dev.set_scan(xy)
    ref = start.copy()
    pose = [float(pxcs[0]) - 0.5, float(pxcs[1]) - 0.5, 0.0]
    for k in range(2):
        fused(dev, oc, ref, xy, pose, max_hits, set_scan=False)
    same(dev.obstaclemap_download(), ref, name)


@pytest.mark.parametrize("name", ["saturation_max_10", "octants_65", "width_pp"])
def test_update_maps_pxcs(devs, det, name):
    """Both updates from the caller's (px, py, c, s) in one call, twice -- behind a fused scan, so that a pass is pending."""
    oc = det
    size, start, xy, pxcs, max_hits = kc.by_name(name).build()
    dev = devs(size)
    dev.obstaclemap_upload(start)
    ref = start.copy()
    fused(dev, oc, ref, xy, [size // 2, size // 3, 0.0], 7)
    for k in range(2):
        dev.update_maps_pxcs(pxcs, pxcs, 0.6, 50, max_hits)
        oc.update_obstaclemap_pxcs(ref, size, xy, pxcs, max_hits)
    same(dev.obstaclemap_download(), ref, name)


@pytest.mark.parametrize("max_hits", [128, 200, 255, -129])
def test_max_hits_beyond_sbyte_is_refused(cs_mod, devs, det, max_hits):
    """MaxObstacleHits is an sbyte (:101): a value outside it is refused by every entry point and the map -- a pending pass
    included -- is what it was."""
    import slam.net_amd.capi as capi
    oc = det
    size, start, xy, pxcs, _ = kc.by_name("saturation_max_127").build()
    dev = devs(size)
    dev.obstaclemap_upload(start)
    ref = start.copy()
    fused(dev, oc, ref, xy, [2.0, 2.0, 0.0], 127)
    for call in (lambda: dev.update_obstaclemap_pxcs(pxcs, max_hits), lambda: dev.update_obstaclemap([2.0, 2.0, 0.0], max_hits),
                 lambda: dev.update_maps_pxcs(pxcs, pxcs, 0.6, 50, max_hits), lambda: dev.search_and_update([2.0, 2.0, 0.0], 0.6, 50, max_hits),
                 lambda: dev.search_and_update_pxcs(pxcs, pxcs, pxcs, 0.6, 50, max_hits)):
        with pytest.raises(capi.SlamhipError):
            call()
    same(dev.obstaclemap_download(), ref, max_hits)


# ---- ObstacleMaps of more cells than the launch's wavefronts take in one stride ---------------------------------------------
@pytest.fixture(scope="module")
def cus(ctx):
    """The compute units of device 0, which the context launches one k2_pixels workgroup each on."""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    v = C.c_int(0)
    assert hip.hipDeviceGetAttribute(C.byref(v), 63, 0) == 0             # hipDeviceAttributeMultiprocessorCount (hip_runtime_api.h)
    assert 8 <= v.value <= 4096, v.value
    return v.value


@pytest.mark.parametrize("which,hsize", [(0, 64), (1, 256), (2, 64)])
def test_ride_beyond_the_first_stride(devs, det, cus, which, hsize):
    """513^2, 520^2 and 1024^2 cells on 256 CUs (by the reported count otherwise): the cell pass's stride loop (k2_ride_tail) owns
    every cell from 64 * 16 * CUs on.  Random int8 start map; robot, end points and crossed cells in the last rows; the second
    scan's ride applies the first one's pass, hits there included."""
    oc = det
    size = kc.big_sizes(cus)[which]
    stride = 64 * 16 * cus
    assert size * size > stride
    _, start, xy_a, pxcs_a, _ = kc.big_case(size, 0)
    _, _, xy_b, pxcs_b, _ = kc.big_case(size, 1)
    hits, crossed, _ = kc.trace((size, start, xy_a, pxcs_a, 10))
    assert any(y * size + x >= stride for x, y in hits) and any(y * size + x >= stride for x, y in crossed)
    dev = devs(size, hsize)
    dev.obstaclemap_upload(start)
    ref = start.copy()
    fused(dev, oc, ref, xy_a, [float(pxcs_a[0]) - 0.5, float(pxcs_a[1]) - 0.5, 0.0])
    changed_a = np.flatnonzero(ref.ravel() != start.ravel())
    assert (changed_a >= stride).sum() >= 20
    fused(dev, oc, ref, xy_b, [float(pxcs_b[0]) - 0.5, float(pxcs_b[1]) - 0.5, 0.0])
    print("ObstacleMap %d^2 = %d cells, %d CUs, stride %d cells" % (size, size * size, cus, stride))
    same(dev.obstaclemap_download(), ref, (size, cus))


@pytest.mark.parametrize("osize,R", [(128, 90), (128, 300), (192, 300)])
def test_ride_scans(devs, det, osize, R):
    """Three fused scans of R rays from three places on a random map.  Under SLAMHIP_K2_GRID = 8 / 16 (test_ride_small_grid) the
    launch has 128 / 256 wavefronts: several strides of cells each and, from 129 / 257 rays on, several rays."""
    oc = det
    grid = int(os.environ.get("SLAMHIP_K2_GRID", "0"))
    if grid and (osize, grid) != (128, 16):
        assert osize * osize > grid * 16 * 64                            # (128^2 is exactly one stride of 256 wavefronts)
    if grid and R == 300:
        assert R > grid * 16
    dev = devs(osize)
    start = kc.random_map(osize, osize + R)
    dev.obstaclemap_upload(start)
    ref = start.copy()
    for k, (x, y) in enumerate([(osize // 2, osize // 2), (3, osize - 2), (osize - 1, 0)]):
        fused(dev, oc, ref, random_scan(R + k, R, osize), [x, y, 0.0], 10 - 4 * k)
    same(dev.obstaclemap_download(), ref, (osize, R, grid))


@pytest.mark.parametrize("grid", [8, 16])
def test_ride_small_grid(grid):
    """test_ride_scans in a fresh interpreter with a launch of 8 / 16 workgroups: the ride's stride loops over cells and rays run."""
    here = os.path.abspath(__file__)
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-m", "pytest", here, "-m", "gpu", "-x", "-q", "-k", "test_ride_scans"],
                       env=dict(os.environ, SLAMHIP_K2_GRID=str(grid)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and "3 passed" in out, (grid, out[-3000:])


# ---- the pending pass: everything that may come behind a fused scan ---------------------------------------------------------
SM = 64                                                                  # both maps 64^2, one cell per metre


def _pending(devs, oc, seed, max_hits=10):
    """A device whose last fused scan's cell pass is pending, and the reference map behind that scan."""
    dev = devs(SM)
    start = kc.random_map(SM, seed)
    dev.obstaclemap_upload(start)
    ref = start.copy()
    fused(dev, oc, ref, random_scan(seed, 300, 40), [20.0 + seed % 7, 30.0, 0.0], max_hits)
    assert (ref != start).sum() > 100
    return dev, ref


def test_pending_then_upload(devs, det):
    oc = det
    dev, _ = _pending(devs, oc, 1)
    fresh = kc.random_map(SM, 101)
    dev.obstaclemap_upload(fresh)                                        # the pending pass lands BEFORE the upload, not on it
    ref = fresh.copy()
    same(dev.obstaclemap_download(), ref, "upload")
    fused(dev, oc, ref, random_scan(2, 200, 40), [40.0, 11.0, 0.0])      # ... and left its scratch clear
    fused(dev, oc, ref, random_scan(3, 200, 40), [12.0, 50.0, 0.0])
    same(dev.obstaclemap_download(), ref, "upload, two scans")


def test_pending_then_reset(devs, det):
    oc = det
    dev, _ = _pending(devs, oc, 2)
    dev.reset(-7)
    ref = np.full((SM, SM), -7, np.int8)
    same(dev.obstaclemap_download(), ref, "reset")
    fused(dev, oc, ref, random_scan(4, 200, 40), [33.0, 31.0, 0.0])
    fused(dev, oc, ref, random_scan(5, 200, 40), [30.0, 35.0, 0.0])
    same(dev.obstaclemap_download(), ref, "reset, two scans")


def test_pending_then_checksum(devs, det, checksum_np):
    oc = det
    dev, ref = _pending(devs, oc, 3)
    assert dev.maps_checksum()[1] == checksum_np(ref)
    same(dev.obstaclemap_download(), ref, "checksum")


def test_pending_then_standalone_update(devs, det):
    oc = det
    dev, ref = _pending(devs, oc, 4)
    xy = random_scan(6, 250, 40)
    pxcs = kc.pxcs_at(25, 28)
    dev.set_scan(xy)
    dev.update_obstaclemap_pxcs(pxcs, 3)
    oc.update_obstaclemap_pxcs(ref, SM, xy, pxcs, 3)
    same(dev.obstaclemap_download(), ref, "stand-alone")


def test_pending_then_fused_with_another_max_hits(devs, det):
    """The pending pass is applied with ITS scan's MaxObstacleHits, not with that of the scan it rides on."""
    oc = det
    dev = devs(SM)
    start = np.tile(np.arange(-4, 12, dtype=np.int8), (SM, SM // 16))
    dev.obstaclemap_upload(start)
    ref = start.copy()
    xy = np.array([(x, y) for y in range(-20, 21, 2) for x in range(-20, 21, 2)], np.float32)
    for max_hits in (10, 3, 127, -2, 10):
        fused(dev, oc, ref, xy, [30.0, 30.0, 0.0], max_hits)
    same(dev.obstaclemap_download(), ref, "max_hits")


def test_pending_then_robot_outside_obstaclemap_only(cs_mod, devs, det):
    """Robot on the HoleMap's last column but -- (int)(x * scale + 0.5) at the coarser scale -- past the ObstacleMap's: the walk is
    refused (:557-560), the launch is made all the same and carries the pending pass, which is applied exactly once."""
    oc = det
    dev = devs(SM, 128, metres=64.0)
    pose_out = [63.625, 20.0, 0.0]
    assert int(oc.pose_to_pxcs(pose_out, dev.obst_scale)[0]) == SM and int(oc.pose_to_pxcs(pose_out, dev.hole_scale)[0]) == 127
    start = kc.random_map(SM, 7)
    dev.obstaclemap_upload(start)
    ref = start.copy()
    fused(dev, oc, ref, random_scan(7, 300, 40), [30.0, 30.0, 0.0])
    before = ref.copy()
    fused(dev, oc, ref, random_scan(8, 300, 40), pose_out)
    fused(dev, oc, ref, random_scan(9, 300, 40), pose_out)
    assert (ref == before).all()
    fused(dev, oc, ref, random_scan(10, 300, 40), [31.0, 29.0, 0.0])
    same(dev.obstaclemap_download(), ref, "robot outside the ObstacleMap")


def test_pending_then_two_launch_scan(devs, det):
    """2100 rays (> K2_LDS_RAYS): the HoleMap update takes k2_prepare + the pixel kernel and the ObstacleMap update its own launches,
    behind the pending pass."""
    oc = det
    dev, ref = _pending(devs, oc, 5)
    fused(dev, oc, ref, random_scan(11, 2100, 40), [22.0, 41.0, 0.0], 5)
    fused(dev, oc, ref, random_scan(12, 300, 40), [41.0, 22.0, 0.0])
    same(dev.obstaclemap_download(), ref, "two-launch form")


def test_pending_then_empty_scan(cs_mod, devs, det):
    """No scan: the fused call is a state error and touches nothing; the pending pass is still applied afterwards."""
    import slam.net_amd.capi as capi
    oc = det
    dev, ref = _pending(devs, oc, 6)
    dev.set_scan(np.zeros((0, 2), np.float32))
    with pytest.raises(capi.SlamhipError):
        dev.search_and_update([30.0, 30.0, 0.0], 0.6, 50, 10)
    dev.update_obstaclemap_pxcs(kc.pxcs_at(30, 30), 10)                  # (an empty scan: nothing to do, nothing flushed)
    same(dev.obstaclemap_download(), ref, "empty scan")
    fused(dev, oc, ref, random_scan(13, 300, 40), [30.0, 30.0, 0.0])
    same(dev.obstaclemap_download(), ref, "empty scan, one more")
