"""CPU-side checks of the scrolling window's backing store (slamhip_hs_set_backing, slamhip_hs_backing_stats,
slamhip_hs_world_cells_download, slamhip_debug_backing_plan): exported, declared, stated in the header, mirrored in Python and in
the C# shim; and the planner -- pure host code -- against a brute-force NumPy model that paints every cell of the old and the new
window with its world coordinate and groups the cells by np.floor_divide.  No compute calls."""
import ctypes as C
import hashlib
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("slamhip_hs_set_backing", "slamhip_hs_backing_stats", "slamhip_hs_world_cells_download", "slamhip_debug_backing_plan")
LEVELS = 3
G = 1 << (LEVELS - 1)


@pytest.fixture(scope="module")
def capi():
    import slam.net_amd.build as b
    b.build()
    import slam.net_amd.capi as capi
    return capi


def header_text():
    return open(os.path.join(ROOT, "include", "slamhip.h")).read()


def test_symbols_exported_and_declared(capi):
    L = capi.lib()
    declared = set(capi.declared_symbols())
    for name in SYMBOLS:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in L._signatures, name
    h = re.sub(r"\s+", " ", header_text())
    assert "int32_t slamhip_hs_set_backing(slamhip_hs *hs, int32_t tile_cells, uint64_t max_bytes);" in h
    assert "int32_t slamhip_hs_backing_stats(slamhip_hs *hs, slamhip_backing_stats *out);" in h
    assert ("int32_t slamhip_hs_world_cells_download(slamhip_hs *hs, int32_t level, int64_t x0, int64_t y0, "
            "int32_t w, int32_t h, slamhip_cell *out);") in h
    assert ("int32_t slamhip_debug_backing_plan(int32_t levels, int32_t w0, int32_t h0, int64_t ox, int64_t oy, "
            "int32_t dx, int32_t dy, int32_t tile, slamhip_backing_job *jobs, int32_t cap, int32_t *n_jobs);") in h
    assert "int64_t tiles, bytes, capacity_bytes;" in h and "int64_t evicted_cells, restored_cells, dropped_cells;" in h
    assert "int32_t tile, on; } slamhip_backing_stats;" in h


def test_header_states_the_contract():
    h = re.sub(r"[\s*/]+", " ", header_text())
    assert "12 tile^2 bytes" in h                                          # the slot
    assert "A shift NEVER fails for capacity" in h and "dropped_cells" in h
    assert "a power of two in [8, 256]" in h
    assert "The setting survives slamhip_hs_reset; the tiles do not" in h
    assert "slamhip_hs_cells_upload touches the window only" in h
    assert "the window wins" in h and "w h <= 2^26 cells" in h             # the download: precedence and its bound
    assert "While the reference's cache is on (slamhip_hs_set_reference_cache) slamhip_hs_shift refuses as before" in h
    assert "With backing off nothing is allocated, no extra launch is issued" in h


def test_null_handles_are_refused(capi):
    """Argument checks run before anything touches a device: a null handle is SLAMHIP_ERR_INVALID, not a crash."""
    L = capi.lib()
    st = capi.BackingStats()
    st.tiles = 7
    cell = np.zeros(4, capi.CELL_DTYPE)
    assert L.slamhip_hs_set_backing(None, 16, 1 << 20) == capi.ERR_INVALID
    assert L.slamhip_hs_set_backing(None, 16, 0) == capi.ERR_INVALID
    assert L.slamhip_hs_backing_stats(None, C.byref(st)) == capi.ERR_INVALID
    assert st.tiles == 7
    assert L.slamhip_hs_world_cells_download(None, 0, 0, 0, 2, 2, cell.ctypes.data_as(C.c_void_p)) == capi.ERR_INVALID
    n = C.c_int32(-5)
    assert L.slamhip_debug_backing_plan(3, 64, 64, 0, 0, 4, 0, 16, None, 0, None) == capi.ERR_INVALID
    for tile in (0, 4, 12, 512):                                           # not a power of two in [8, 256]
        assert L.slamhip_debug_backing_plan(3, 64, 64, 0, 0, 4, 0, tile, None, 0, C.byref(n)) == capi.ERR_INVALID
    assert L.slamhip_debug_backing_plan(0, 64, 64, 0, 0, 4, 0, 16, None, 0, C.byref(n)) == capi.ERR_INVALID
    assert L.slamhip_debug_backing_plan(3, 64, 4, 0, 0, 4, 0, 16, None, 0, C.byref(n)) == capi.ERR_INVALID   # 4 >> 2 < 2
    assert n.value == -5


def test_python_mirror_exposes_the_methods(capi):
    import slam.net_amd.hector as hs
    for name in ("set_backing", "backing_stats", "world_cells"):
        assert callable(getattr(hs.MapRepMultiMap, name)), name
    assert callable(hs.HectorSLAMProcessor.set_backing)
    p = inspect.signature(hs.HectorSLAMProcessor.__init__).parameters
    assert "scrollBacking" in p and p["scrollBacking"].default is None
    assert C.sizeof(capi.BackingStats) == 56 and C.sizeof(capi.BackingJob) == 48


def test_csharp_shim_declares_the_imports():
    shim = os.path.join(ROOT, "bindings", "csharp", "SlamHip")
    native = open(os.path.join(shim, "SlamHip.Native.cs")).read()
    for name in SYMBOLS[:3]:
        assert re.search(r"\[DllImport\(Lib\)\] internal static extern int %s\(" % name, native), name
    assert "public struct BackingStats" in native
    rep = open(os.path.join(shim, "HectorSLAM", "MapRepMultiMap.Hip.cs")).read()
    assert "public void SetBacking(int tileCells, ulong maxBytes)" in rep and "Native.slamhip_hs_set_backing(" in rep
    assert "public BackingStats BackingStats" in rep and "Native.slamhip_hs_backing_stats(" in rep
    assert re.search(r"public unsafe LogOddsCell\[\] WorldCells\(int level, long x0, long y0, int w, int h\)", rep)
    assert "Native.slamhip_hs_world_cells_download(" in rep
    proc = open(os.path.join(shim, "HectorSLAM", "HectorSLAMProcessor.Hip.cs")).read()
    assert "ScrollBacking" in proc and "MapRep.SetBacking(" in proc


# ---- the planner against a brute-force model -------------------------------------------------------------------------------------
def plan_cases():
    out = []
    for w0, h0 in ((64, 64), (70, 46)):
        shifts = [(G, 0), (0, -G), (-2 * G, 3 * G), (w0, 0), (0, -h0 - G), (-w0 - G, h0 + G)]    # the last three: at or beyond the window
        for T in (8, 16):
            for origin in ((0, 0), (-52, -36), (4 * 10 ** 6, -4 * 10 ** 6)):
                for d in shifts:
                    out.append((w0, h0, T, origin, d))
    return out


def model_regions(w, h, sx, sy):
    """(departing mask in the OLD window's coordinates, arriving mask in the NEW window's), cell by cell."""
    y, x = np.mgrid[0:h, 0:w]
    dep = ~((x - sx >= 0) & (x - sx < w) & (y - sy >= 0) & (y - sy < h))
    arr = ~((x + sx >= 0) & (x + sx < w) & (y + sy >= 0) & (y + sy < h))
    return dep, arr


@pytest.mark.parametrize("case", plan_cases(), ids=lambda c: "%dx%d-T%d-o%d_%d-d%d_%d" % (c[0], c[1], c[2], c[3][0], c[3][1], c[4][0], c[4][1]))
def test_planner_against_brute_force(capi, case):
    w0, h0, T, (ox, oy), (dx, dy) = case
    jobs = capi.backing_plan(LEVELS, w0, h0, ox, oy, dx, dy, T)
    assert len(jobs) > 0
    # the order: level, then evict before restore, then row-major by tile
    keys = [(int(j["level"]), int(j["kind"]), int(j["ty"]), int(j["tx"])) for j in jobs]
    assert keys == sorted(keys)
    w, h = w0, h0
    for l in range(LEVELS):
        sx, sy = dx >> l, dy >> l
        dep, arr = model_regions(w, h, sx, sy)
        if abs(dx) >= w0 or abs(dy) >= h0:
            assert dep.all() and arr.all()
        for kind, mask, OX, OY in ((capi.BACKING_EVICT, dep, ox >> l, oy >> l), (capi.BACKING_RESTORE, arr, (ox >> l) + sx, (oy >> l) + sy)):
            yy, xx = np.mgrid[0:h, 0:w]
            X, Y = xx.astype(np.int64) + OX, yy.astype(np.int64) + OY     # every window cell painted with its world coordinate
            TX, TY = np.floor_divide(X, T), np.floor_divide(Y, T)
            LX, LY = X - T * TX, Y - T * TY
            cover = np.zeros((h, w), np.int32)
            for j in jobs[(jobs["level"] == l) & (jobs["kind"] == kind)]:
                wx, wy, nx, ny = int(j["wx"]), int(j["wy"]), int(j["nx"]), int(j["ny"])
                assert nx >= 1 and ny >= 1 and 0 <= wx and wx + nx <= w and 0 <= wy and wy + ny <= h, j
                sl = (slice(wy, wy + ny), slice(wx, wx + nx))
                cover[sl] += 1
                assert (TX[sl] == j["tx"]).all() and (TY[sl] == j["ty"]).all(), j          # no job crosses a tile
                assert LX[wy, wx] == j["lx"] and LY[wy, wx] == j["ly"], j
                assert 0 <= j["lx"] and j["lx"] + nx <= T and 0 <= j["ly"] and j["ly"] + ny <= T, j
            assert np.array_equal(cover, mask.astype(np.int32)), (l, kind)                 # the region exactly once, nothing else
        w //= 2; h //= 2


def test_planner_cap_too_small(capi):
    L = capi.lib()
    jobs = capi.backing_plan(LEVELS, 70, 46, -52, -36, -2 * G, 3 * G, 8)
    need = len(jobs)
    assert need > 4
    n = C.c_int32(0)
    buf = np.zeros(need, capi.BACKING_JOB_DTYPE)
    buf["level"] = 99
    ptr = buf.ctypes.data_as(C.POINTER(capi.BackingJob))
    assert L.slamhip_debug_backing_plan(LEVELS, 70, 46, -52, -36, -2 * G, 3 * G, 8, ptr, need - 1, C.byref(n)) == capi.ERR_INVALID
    assert n.value == need and (buf["level"] == 99).all()                  # the needed count, nothing written
    assert L.slamhip_debug_backing_plan(LEVELS, 70, 46, -52, -36, -2 * G, 3 * G, 8, ptr, need, C.byref(n)) == capi.OK
    assert n.value == need and np.array_equal(buf, jobs)
    assert len(capi.backing_plan(LEVELS, 64, 64, 0, 0, 0, 0, 16)) == 0     # no move, no jobs


# ---- the plans, byte for byte ----------------------------------------------------------------------------------------------------
# The brute-force test pins coverage and order; this pins the bytes -- the byte order deals the slots and so decides what a full
# pool drops.  SHA-256 over the raw job arrays (jobs.tobytes()) of plan_cases() and then DIGEST_EXTRA, concatenated in that order,
# as the library of commit 920e200 (the last one with a tile cutter of its own in backing_plan.h) produced them.
DIGEST_EXTRA = [(128, 128, 64, (0, 0), (-68, 72)), (128, 128, 64, (-52, -36), (-68, 72))]   # test_gpu_hector_backing.py's two-piece jobs
PLAN_SHA256 = "7687dc55f29f1489d72c0048840d56b35a7573fac9c043ebb0bef3d4ad51263a"


def test_plans_are_byte_identical(capi):
    h = hashlib.sha256()
    for w0, h0, T, (ox, oy), (dx, dy) in plan_cases() + DIGEST_EXTRA:
        h.update(capi.backing_plan(LEVELS, w0, h0, ox, oy, dx, dy, T).tobytes())
    first = capi.backing_plan(LEVELS, *DIGEST_EXTRA[0][:2], *DIGEST_EXTRA[0][3], *DIGEST_EXTRA[0][4], DIGEST_EXTRA[0][2])
    areas = sorted((first["nx"] * first["ny"]).tolist())
    assert len(first) == 24 and areas[-1] == 4096 and 3584 in areas        # (jobs of more than 2048 cells: two pieces each)
    assert h.hexdigest() == PLAN_SHA256
