"""CPU-side checks of loading a saved world back (slamhip_hs_world_cells_upload, slamhip_hs_world_extends,
slamhip_debug_world_plan): exported, declared, stated in the header, mirrored in Python and in the C# shim; and the planner -- pure
host code -- against a brute-force NumPy model that paints every cell of the rectangle with its world coordinate, classifies it as
inside or outside the window and groups the outside cells by np.floor_divide.  No compute calls."""
import ctypes as C
import hashlib
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("slamhip_hs_world_cells_upload", "slamhip_hs_world_extends", "slamhip_debug_world_plan")


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
    for name in SYMBOLS + ("slamhip_hsproc_shift",):
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in L._signatures, name
    h = re.sub(r"\s+", " ", header_text())
    assert ("int32_t slamhip_hs_world_cells_upload(slamhip_hs *hs, int32_t level, int64_t x0, int64_t y0, "
            "int32_t w, int32_t h, const slamhip_cell *cells, int64_t *out_dropped);") in h
    assert "int32_t slamhip_hs_world_extends(slamhip_hs *hs, int32_t level, int64_t extends[4], int32_t *found);" in h
    assert ("typedef struct slamhip_world_job { int32_t kind, sx, sy, nx, ny, lx, ly, pad; int64_t tx, ty; } "
            "slamhip_world_job;") in h
    assert ("int32_t slamhip_debug_world_plan(int32_t w, int32_t h, int64_t OX, int64_t OY, int64_t x0, int64_t y0, int32_t rw, "
            "int32_t rh, int32_t tile, slamhip_world_job *jobs, int32_t cap, int32_t *n_jobs);") in h
    assert "int32_t slamhip_hsproc_shift(slamhip_hsproc *p, int32_t dx, int32_t dy);" in h
    # the stats struct is as it was
    assert "int64_t tiles, bytes, capacity_bytes;" in h and "int64_t evicted_cells, restored_cells, dropped_cells;" in h
    assert "int32_t tile, on; } slamhip_backing_stats;" in h
    assert C.sizeof(capi.BackingStats) == 56 and C.sizeof(capi.WorldJob) == capi.WORLD_JOB_DTYPE.itemsize == 48


def test_header_states_the_contract():
    h = re.sub(r"[\s*/]+", " ", header_text())
    assert "OVERWRITE: every cell of the rectangle replaces what the world holds at that place" in h
    assert "The part of a tile that lies under the window is NOT written: the window wins" in h
    assert "an all-Reset piece takes no slot" in h and "An all-Reset piece over an EXISTING tile is written" in h
    assert "An upload never fails for capacity" in h and "evicted_cells and restored_cells do not move" in h
    assert "counted into dropped_cells of slamhip_hs_backing_stats and into out_dropped" in h and "out_dropped may be NULL" in h
    assert "it becomes at least (mx 3 + 1) 3" in h                         # the update-index rule: (mx / 3 + 1) * 3
    assert "w h <= 2^26 cells, |x0|, |y0| < 2^60" in h
    assert "The cache epoch, the reference's cache and the origin are left as they are" in h
    # the extents
    assert "extends = {xMax, yMax, xMin, yMin} in WORLD cells" in h and "a NaN counts" in h
    assert "EXCLUDING the part of a tile that lies under the window" in h
    assert "found = 0 and extends is zeroed" in h and "does not apply here" in h
    assert "Works with backing off: the window only" in h


def test_null_handles_and_ranges_are_refused(capi):
    """Argument checks run before anything touches a device: a null handle is SLAMHIP_ERR_INVALID, not a crash."""
    L = capi.lib()
    cell = np.zeros(4, capi.CELL_DTYPE)
    dropped = C.c_int64(-9)
    ext = (C.c_int64 * 4)(7, 7, 7, 7)
    found = C.c_int32(-3)
    assert L.slamhip_hs_world_cells_upload(None, 0, 0, 0, 2, 2, cell.ctypes.data_as(C.c_void_p), C.byref(dropped)) == capi.ERR_INVALID
    assert L.slamhip_hs_world_cells_upload(None, 0, 0, 0, 2, 2, None, None) == capi.ERR_INVALID
    assert dropped.value == -9
    assert L.slamhip_hs_world_extends(None, 0, ext, C.byref(found)) == capi.ERR_INVALID
    assert list(ext) == [7, 7, 7, 7] and found.value == -3
    assert L.slamhip_hsproc_shift(None, 4, 0) == capi.ERR_INVALID
    n = C.c_int32(-5)
    plan = lambda *a: L.slamhip_debug_world_plan(*a, None, 0, C.byref(n))
    assert L.slamhip_debug_world_plan(16, 12, 0, 0, 0, 0, 4, 4, 8, None, 0, None) == capi.ERR_INVALID
    for tile in (4, 12, 512, -8):                                          # neither 0 nor a power of two in [8, 256]
        assert plan(16, 12, 0, 0, 0, 0, 4, 4, tile) == capi.ERR_INVALID
    assert plan(16, 12, 0, 0, 0, 0, 0, 4, 8) == capi.ERR_INVALID           # w, h >= 1
    assert plan(16, 12, 0, 0, 0, 0, 4, -1, 8) == capi.ERR_INVALID
    assert plan(16, 12, 0, 0, 0, 0, 1 << 14, (1 << 12) + 1, 8) == capi.ERR_INVALID   # w * h <= 2^26
    assert plan(16, 12, 0, 0, 1 << 60, 0, 4, 4, 8) == capi.ERR_INVALID     # |x0|, |y0| < 2^60
    assert plan(16, 12, 0, 0, 0, -(1 << 60), 4, 4, 8) == capi.ERR_INVALID
    assert plan(0, 12, 0, 0, 0, 0, 4, 4, 8) == capi.ERR_INVALID
    assert n.value == -5


def test_python_mirror_exposes_the_methods(capi):
    import slam.net_amd.hector as hs
    for name in ("world_put", "world_extends", "save_world", "load_world"):
        assert callable(getattr(hs.MapRepMultiMap, name)), name
    assert list(inspect.signature(hs.MapRepMultiMap.world_put).parameters) == ["self", "level", "x0", "y0", "cells"]
    for name in ("SaveWorld", "LoadWorld"):
        assert callable(getattr(hs.HectorSLAMProcessor, name)), name
    assert callable(capi.world_plan)


def test_csharp_shim_declares_and_uses_the_stubs():
    shim = os.path.join(ROOT, "bindings", "csharp", "SlamHip")
    native = open(os.path.join(shim, "SlamHip.Native.cs")).read()
    for name in SYMBOLS[:2] + ("slamhip_hsproc_shift",):
        assert re.search(r"\[DllImport\(Lib\)\] internal static extern int %s\(" % name, native), name
    rep = open(os.path.join(shim, "HectorSLAM", "MapRepMultiMap.Hip.cs")).read()
    assert re.search(r"public unsafe long WorldPut\(int level, long x0, long y0, int w, int h, LogOddsCell\[\] cells\)", rep)
    assert "Native.slamhip_hs_world_cells_upload(" in rep
    assert re.search(r"public unsafe bool WorldExtends\(int level, out long xMax, out long yMax, out long xMin, out long yMin\)", rep)
    assert "Native.slamhip_hs_world_extends(" in rep
    assert "public void SaveWorld(string path)" in rep and "public long LoadWorld(string path" in rep
    proc = open(os.path.join(shim, "HectorSLAM", "HectorSLAMProcessor.Hip.cs")).read()
    assert "public void SaveWorld(string path)" in proc and "public long LoadWorld(string path)" in proc
    assert "MapRep.SaveWorld(" in proc and "MapRep.LoadWorld(" in proc and "Native.slamhip_hsproc_shift(" in proc
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "Resume from a saved map" in doc and "slamhip_hs_world_cells_upload" in doc and "little-endian" in doc


# ---- the planner against a brute-force model -------------------------------------------------------------------------------------
WINDOWS = [(64, 48), (16, 12), (18, 14)]                                   # level 0 and level 2 of 64 x 48; level 2 of 72 x 56


def rect_shapes(w, h, OX, OY):
    """(name, x0, y0, rw, rh) relative to the window at (OX, OY)."""
    return [("inside", OX + 3, OY + 2, 5, 4),
            ("outside", OX + w + 9, OY - 20, 11, 7),
            ("left_edge", OX - 7, OY + 1, 12, 5),                          # (x0 odd for an even OX and even for an odd one: both occur)
            ("all_four", OX - 9, OY - 10, w + 19, h + 21),                 # the window inside the rectangle
            ("rw1", OX + w - 1, OY - 3, 1, h + 6),
            ("rh1", OX - 11, OY + h - 1, w + 20, 1),
            ("corner", OX + w - 4, OY + h - 3, 13, 9)]


def plan_cases():
    out = []
    for w, h in WINDOWS:
        for OX, OY in ((0, 0), (-5, 3), (9, -7), (10 ** 6 + 1, -10 ** 6)):
            for name, x0, y0, rw, rh in rect_shapes(w, h, OX, OY):
                for T in (8, 16, 0):
                    out.append((w, h, OX, OY, name, x0, y0, rw, rh, T))
    return out


@pytest.mark.parametrize("case", plan_cases(), ids=lambda c: "%dx%d-o%d_%d-%s-T%d" % (c[0], c[1], c[2], c[3], c[4], c[9]))
def test_planner_against_brute_force(capi, case):
    w, h, OX, OY, name, x0, y0, rw, rh, T = case
    jobs = capi.world_plan(w, h, OX, OY, x0, y0, rw, rh, T)
    yy, xx = np.mgrid[0:rh, 0:rw]
    X, Y = xx.astype(np.int64) + x0, yy.astype(np.int64) + y0              # every cell of the rectangle painted with its world coordinate
    inwin = (X >= OX) & (X < OX + w) & (Y >= OY) & (Y < OY + h)
    assert inwin.any() == (name != "outside") and (~inwin).any() == (name != "inside")
    # the window in rectangle coordinates: what the order of one tile's jobs is stated in
    kx0, kx1, ky0, ky1 = max(0, OX - x0), min(rw, OX + w - x0), max(0, OY - y0), min(rh, OY + h - y0)
    cover = np.zeros((rh, rw), np.int32)
    n_window, keys = 0, []
    for k, j in enumerate(jobs):
        sx, sy, nx, ny, lx, ly = (int(j[f]) for f in ("sx", "sy", "nx", "ny", "lx", "ly"))
        assert nx >= 1 and ny >= 1 and 0 <= sx and sx + nx <= rw and 0 <= sy and sy + ny <= rh, j     # inside the rectangle
        sl = (slice(sy, sy + ny), slice(sx, sx + nx))
        cover[sl] += 1
        if j["kind"] == capi.WORLD_WINDOW:
            assert k == 0, "the window job comes first"
            n_window += 1
            assert inwin[sl].all(), j
            assert lx == X[sy, sx] - OX and ly == Y[sy, sx] - OY, j
            assert 0 <= lx and lx + nx <= w and 0 <= ly and ly + ny <= h, j                            # inside the window
        else:
            assert j["kind"] == capi.WORLD_TILE and T > 0, j
            assert not inwin[sl].any(), j
            TX, TY = np.floor_divide(X[sl], T), np.floor_divide(Y[sl], T)
            assert (TX == j["tx"]).all() and (TY == j["ty"]).all(), j                                  # no job crosses a tile
            assert lx == X[sy, sx] - T * int(j["tx"]) and ly == Y[sy, sx] - T * int(j["ty"]), j
            assert 0 <= lx and lx + nx <= T and 0 <= ly and ly + ny <= T, j                            # inside the tile
            band = 0 if sy < ky0 or not inwin.any() else 1 if sy >= ky1 else 2 if sx < kx0 else 3      # above, below, left, right
            keys.append((int(j["ty"]), int(j["tx"]), band))
    assert n_window == (1 if inwin.any() else 0)
    assert keys == sorted(keys)                                            # row-major by tile, one tile's jobs in rectangle order
    if T > 0:
        assert (cover == 1).all()                                          # every cell of the rectangle exactly once
        tiles = {(a, b) for a, b, _ in keys}
        want = set(zip(np.floor_divide(Y[~inwin], T).tolist(), np.floor_divide(X[~inwin], T).tolist()))
        assert tiles == want
    else:
        assert np.array_equal(cover, inwin.astype(np.int32))               # backing off: exactly the window's cells


def test_planner_cap_too_small(capi):
    L = capi.lib()
    args = (16, 12, -5, 3, -14, -7, 35, 33, 8)
    jobs = capi.world_plan(*args)
    need = len(jobs)
    assert need > 8 and jobs[0]["kind"] == capi.WORLD_WINDOW
    n = C.c_int32(0)
    buf = np.zeros(need, capi.WORLD_JOB_DTYPE)
    buf["kind"] = 99
    ptr = buf.ctypes.data_as(C.POINTER(capi.WorldJob))
    assert L.slamhip_debug_world_plan(*args, ptr, need - 1, C.byref(n)) == capi.ERR_INVALID
    assert n.value == need and (buf["kind"] == 99).all()                   # the needed count, nothing written
    assert L.slamhip_debug_world_plan(*args, ptr, need, C.byref(n)) == capi.OK
    assert n.value == need and np.array_equal(buf, jobs)
    # a tile in the window's corner gives more than one job, in rectangle order
    t = jobs[jobs["kind"] == capi.WORLD_TILE]
    per_tile = {}
    for j in t:
        per_tile.setdefault((int(j["ty"]), int(j["tx"])), []).append(j)
    assert max(len(v) for v in per_tile.values()) >= 2


# ---- the plans, byte for byte ----------------------------------------------------------------------------------------------------
# The brute-force test pins coverage and order; this pins the bytes -- the byte order deals the slots and so decides what a full
# pool drops.  SHA-256 over the raw job arrays (jobs.tobytes()) of plan_cases() and then DIGEST_EXTRA, concatenated in that order,
# as the library of commit 920e200 (the last one with a tile cutter of its own in world_plan.h) produced them.
DIGEST_EXTRA = [(2304, 8, 0, 0, "wide", -3, -2, 2310, 12, 8), (2304, 8, 0, 0, "wide", -3, -2, 2310, 12, 0)]   # test_gpu_hector_world.py's wide put
PLAN_SHA256 = "785823b00c208b54205141d70fd0f786f183453687113fa4410429c389c833e2"


def test_plans_are_byte_identical(capi):
    h = hashlib.sha256()
    for w, hh, OX, OY, _, x0, y0, rw, rh, T in plan_cases() + DIGEST_EXTRA:
        h.update(capi.world_plan(w, hh, OX, OY, x0, y0, rw, rh, T).tobytes())
    wide = capi.world_plan(2304, 8, 0, 0, -3, -2, 2310, 12, 8)
    assert len(wide) == 583 and wide[0]["kind"] == capi.WORLD_WINDOW and wide[0]["nx"] == 2304   # (wider than one piece of 2048 cells)
    assert h.hexdigest() == PLAN_SHA256
