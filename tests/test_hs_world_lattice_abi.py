"""CPU-side checks of the world search's interface (slamhip_hs_world_lattice_search, slamhip_hs_relocalise_world,
slamhip_hsproc_relocalise_world, slamhip_debug_world_pack_plan), its planner against a brute-force ownership map, and the NumPy
restatement of the world definition (include/slamhip.h, THE WORLD SEARCH) that tests/test_gpu_hector_world_lattice.py compares the
device with: test_hs_lattice_abi's point cells, integer indexing into a cell array that covers more than the window.  Everything is
compared with == on integers.  No compute calls on a device."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import test_hs_lattice_abi as A
from test_hs_lattice_abi import capi                                       # noqa: F401 (fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("slamhip_hs_world_lattice_search", "slamhip_hs_relocalise_world", "slamhip_hsproc_relocalise_world",
           "slamhip_debug_world_pack_plan")
F = np.float32


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def np_world_volume(values, ax0, ay0, cell, centre, nx, ny, n_theta, dtheta, xy):
    """The score volume of the world definition.  values: an (H, W) float32 array of cell Values whose element [0, 0] is
    WINDOW-FRAME cell (ax0, ay0) of the level -- the window over the tiles, Reset (0.0) where nothing is; every cell outside the
    array is Reset as well, so the array must hold everything of the world that is not.  (ax0, ay0) = (0, 0) and the window's own
    values: the window search."""
    values = np.asarray(values, np.float32)
    H, W = values.shape
    cls = A.np_classes(values, W, H)
    stm = F(1.0) / F(cell)
    ixs = np.arange(-nx, nx + 1, dtype=np.int64)
    out = np.zeros((n_theta, 2 * ny + 1, 2 * nx + 1), np.int32)
    for k in range(n_theta):
        gx, gy, valid = A.np_point_cells(stm, centre, A.np_theta(centre, k, dtheta), xy)
        gx, gy = gx[valid] - ax0, gy[valid] - ay0                          # integers: exact
        X = gx[None, :] + ixs[:, None]
        okx = (X >= 0) & (X < W)
        Xc = np.clip(X, 0, W - 1)
        for iy in range(-ny, ny + 1):
            Y = gy + iy
            ok = okx & ((Y >= 0) & (Y < H))[None, :]
            vals = cls[np.clip(Y, 0, H - 1)[None, :], Xc]
            out[k, iy + ny] = np.where(ok, vals, 0).sum(axis=1, dtype=np.int64).astype(np.int32)
    return out


def test_restatement_equals_the_window_restatement():
    rng = np.random.default_rng(5)
    w, h = 40, 24
    pick = rng.integers(0, 5, w * h)
    mag = rng.uniform(0.1, 3.0, w * h).astype(np.float32)
    v = np.select([pick == 0, pick == 1, pick == 2, pick == 3], [mag, -mag, F(0.0), F(-0.0)], F(np.nan)).astype(np.float32)
    xy = np.stack([rng.uniform(-1.0, 9.0, 61), rng.uniform(-1.0, 6.0, 61)], 1).astype(np.float32)
    xy[3] = (np.nan, 0.5)
    xy[11] = (1.0e6, -2.0e6)
    args = (F(0.2), np.array([0.27, 0.13, 0.3], np.float32), 9, 7, 4, F(0.4), xy)
    want = A.np_volume(v, w, h, *args)
    assert np.array_equal(np_world_volume(v.reshape(h, w), 0, 0, *args), want) and len(np.unique(want)) > 8
    # a frame of Reset cells around the window changes nothing; a frame of occupied cells does
    pad = np.zeros((h + 11, w + 9), np.float32)
    pad[6:6 + h, 5:5 + w] = v.reshape(h, w)
    assert np.array_equal(np_world_volume(pad, -5, -6, *args), want)
    pad[:6] = 1.0
    assert not np.array_equal(np_world_volume(pad, -5, -6, *args), want)


# ---- the interface -----------------------------------------------------------------------------------------------------------------
def header_text():
    return open(os.path.join(ROOT, "include", "slamhip.h")).read()


def test_symbols_exported_and_declared(capi):
    L = capi.lib()
    declared = set(capi.declared_symbols())
    for name in SYMBOLS:
        assert name in declared and hasattr(L, name) and name in L._signatures, name
    h = re.sub(r"[\s*/]+", " ", header_text())
    assert "THE WORLD SEARCH" in h and "only; slamhip_hs_world_lattice_search covers the world behind it" in h
    assert "SLAMHIP_K_HS_LATTICE_PACK_WORLD = 9" in h and "SLAMHIP_K_COUNT = 10" in h
    assert "SLAMHIP_K_HS_LATTICE_PACK = 7" in h and "SLAMHIP_K_HS_LATTICE = 8" in h          # the existing ids keep their values
    assert capi.K_HS_LATTICE_PACK_WORLD == 9 and (capi.K_HS_LATTICE_PACK, capi.K_HS_LATTICE) == (7, 8)


def test_struct_matches_the_header(capi):
    h = header_text()
    assert "sizeof(slamhip_world_reloc_info) == 40, no padding" in h
    names = [n for n, _ in capi.WorldRelocInfo._fields_]
    assert names == list(capi.RELOC_INFO.names) + ["dx", "dy", "n_far"]
    assert C.sizeof(capi.WorldRelocInfo) == capi.WORLD_RELOC_INFO.itemsize == 40
    for i, n in enumerate(names):
        assert getattr(capi.WorldRelocInfo, n).offset == 4 * i == capi.WORLD_RELOC_INFO.fields[n][1], n
        assert getattr(capi.WorldRelocInfo, n).size == 4
    body = re.search(r"typedef struct slamhip_world_reloc_info \{(.*?)\} slamhip_world_reloc_info;", h, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b([a-z_]+)\s*[,;]", body) == names
    assert all(t == "int32_t" for t in re.findall(r"^\s*(\w+)\s", body, re.M))


def test_null_handles_are_refused(capi):
    L = capi.lib()
    spec = capi.lattice_spec(0, (0, 0, 0), 1, 1, 1, 0.1)
    keys = (C.c_uint64 * 1)(7)
    pose = (C.c_float * 3)(1, 2, 3)
    rep, info = capi.MatchReport(), capi.WorldRelocInfo()
    assert L.slamhip_hs_world_lattice_search(None, C.byref(spec), keys, None) == capi.ERR_INVALID
    assert L.slamhip_hs_relocalise_world(None, C.byref(spec), 4, pose, C.byref(rep), C.byref(info)) == capi.ERR_INVALID
    assert L.slamhip_hsproc_relocalise_world(None, None, 0, None, C.byref(spec), 4, 1, pose, C.byref(rep), C.byref(info)) == capi.ERR_INVALID
    assert keys[0] == 7 and list(pose) == [1, 2, 3]


def test_python_mirror_exposes_the_methods(capi):
    import slam.net_amd.hector as hs
    p = inspect.signature(hs.MapRepMultiMap.world_lattice_search).parameters
    assert list(p) == list(inspect.signature(hs.MapRepMultiMap.lattice_search).parameters)
    assert callable(hs.ScanMatcher.RelocaliseWorld)
    p = inspect.signature(hs.HectorSLAMProcessor.RelocaliseWorld).parameters
    assert list(p)[1:] == ["scan", "centreWorld", "level", "nx", "ny", "n_theta", "dtheta", "B", "adopt"]
    assert p["B"].default == 16 and p["adopt"].default is True


def test_csharp_shim_declares_the_imports():
    shim = os.path.join(ROOT, "bindings", "csharp", "SlamHip")
    native = open(os.path.join(shim, "SlamHip.Native.cs")).read()
    for name in SYMBOLS[:3]:
        assert re.search(r"\[DllImport\(Lib\)\] internal static extern int %s\(" % name, native), name
    assert re.search(r"\[StructLayout\(LayoutKind\.Sequential\)\]\s*public struct WorldRelocInfo", native)
    for f, call in (("MapRepMultiMap", "slamhip_hs_world_lattice_search"), ("ScanMatcher", "slamhip_hs_relocalise_world"),
                    ("HectorSLAMProcessor", "slamhip_hsproc_relocalise_world")):
        assert "Native.%s(" % call in open(os.path.join(shim, "HectorSLAM", f + ".Hip.cs")).read(), f


# ---- the planner against a brute-force ownership map -------------------------------------------------------------------------------
def brute_owner(w, h, OX, OY, T, tiles, rect):
    """Per cell of R: kind (-1 nobody, 0 the window, 1 a tile), the tile and the local coordinates -- from the definition alone."""
    x0, y0, rw, rh = rect
    X = np.arange(rw, dtype=np.int64)[None, :] + x0 + np.zeros((rh, 1), np.int64)      # window-frame coordinates
    Y = np.arange(rh, dtype=np.int64)[:, None] + y0 + np.zeros((1, rw), np.int64)
    in_win = (X >= 0) & (X < w) & (Y >= 0) & (Y < h)
    kind = np.where(in_win, 0, -1)
    tx = np.zeros((rh, rw), np.int64); ty = np.zeros((rh, rw), np.int64)
    lx = np.where(in_win, X, 0); ly = np.where(in_win, Y, 0)
    if T:
        WX, WY = X + OX, Y + OY                                                         # world coordinates
        ctx_, cty = np.floor_divide(WX, T), np.floor_divide(WY, T)
        have = np.zeros((rh, rw), bool)
        for t_y, t_x in tiles:
            have |= (ctx_ == t_x) & (cty == t_y)
        t = have & ~in_win
        kind = np.where(t, 1, kind)
        tx = np.where(t, ctx_, tx); ty = np.where(t, cty, ty)
        lx = np.where(t, WX - ctx_ * T, lx); ly = np.where(t, WY - cty * T, ly)
    return kind, tx, ty, lx, ly


PLAN_CASES = [
    # w, h, OX, OY, T, tiles (ty, tx): tiles on every side, under the window, straddling its edges, far corners, holes
    (40, 24, -18, 4, 8, [(-2, -4), (-1, -3), (0, -3), (0, -2), (0, 0), (1, -1), (1, 2), (2, 3), (3, -3), (4, 0), (5, 5)]),
    (40, 24, 17, -11, 8, [(-3, 1), (-2, 2), (-2, 3), (-1, 7), (0, 0), (0, 4), (1, 8), (2, 1)]),      # odd origin
    (80, 48, -36, 8, 16, [(0, -3), (0, -1), (1, 0), (2, 2), (3, -3), (4, 4)]),
    (33, 17, -7, -5, 8, [(-1, -1), (-1, 0), (0, -1), (0, 0), (1, 3)]),                             # negative origin, odd sizes
    (20, 20, 3, 5, 32, [(0, 0)]),                                                                  # the window inside one tile
    (20, 20, 0, 0, 8, [(0, 0), (0, 1), (1, 0), (1, 1)]),                                            # every tile under the window
    (24, 10, 1000001, -999999, 8, [(-125000, 125000), (-124999, 125003)]),                         # far from the world's origin
    (40, 24, 5, 5, 0, []),                                                                         # backing off
]


@pytest.mark.parametrize("case", range(len(PLAN_CASES)))
def test_pack_plan_against_brute_force(capi, case):
    w, h, OX, OY, T, tiles = PLAN_CASES[case]
    rect, jobs = capi.world_pack_plan(w, h, OX, OY, T, tiles)
    x0, y0, rw, rh = rect
    # R: the bounding box of the window and the tiles, in window-frame cells
    xs = [0, w] + [tx * T - OX for _, tx in tiles] + [tx * T + T - OX for _, tx in tiles]
    ys = [0, h] + [ty * T - OY for ty, _ in tiles] + [ty * T + T - OY for ty, _ in tiles]
    assert rect == (min(xs), min(ys), max(xs) - min(xs), max(ys) - min(ys))
    want = brute_owner(w, h, OX, OY, T, tiles, rect)
    kind = np.full((rh, rw), -1, np.int64)
    tx = np.zeros((rh, rw), np.int64); ty = np.zeros((rh, rw), np.int64); lx = np.zeros((rh, rw), np.int64); ly = np.zeros((rh, rw), np.int64)
    assert len(jobs) >= 1 and int(jobs[0]["kind"]) == capi.WORLD_WINDOW
    assert [int(jobs[0][n]) for n in ("sx", "sy", "nx", "ny", "lx", "ly", "tx", "ty")] == [-x0, -y0, w, h, 0, 0, 0, 0]
    for i, j in enumerate(jobs):
        sx, sy, nx, ny = int(j["sx"]), int(j["sy"]), int(j["nx"]), int(j["ny"])
        assert nx >= 1 and ny >= 1 and sx >= 0 and sy >= 0 and sx + nx <= rw and sy + ny <= rh, i
        assert (int(j["kind"]) == capi.WORLD_WINDOW) == (i == 0), i            # window cells are owned by the window job only
        side = (w, h) if i == 0 else (T, T)
        assert 0 <= int(j["lx"]) and int(j["lx"]) + nx <= side[0] and 0 <= int(j["ly"]) and int(j["ly"]) + ny <= side[1], i
        sl = (slice(sy, sy + ny), slice(sx, sx + nx))
        assert (kind[sl] == -1).all(), ("a cell in two jobs", i)
        kind[sl] = int(j["kind"])
        tx[sl] = int(j["tx"]); ty[sl] = int(j["ty"])
        lx[sl] = int(j["lx"]) + np.arange(nx)[None, :]; ly[sl] = int(j["ly"]) + np.arange(ny)[:, None]
    for got, exp, name in zip((kind, tx, ty, lx, ly), want, ("kind", "tx", "ty", "lx", "ly")):
        assert np.array_equal(got, exp), (name, np.argwhere(got != exp)[:4].tolist())
    if T and tiles:
        outside = [(t_y, t_x) for t_y, t_x in tiles if not (t_x * T >= OX and t_x * T + T <= OX + w and t_y * T >= OY and t_y * T + T <= OY + h)]
        assert {(int(j["ty"]), int(j["tx"])) for j in jobs[1:]} == set(outside)
        # tiles in the order given, one tile's jobs together
        seen = [(int(j["ty"]), int(j["tx"])) for j in jobs[1:]]
        assert [t for k, t in enumerate(seen) if k == 0 or seen[k - 1] != t] == outside


def test_pack_plan_refusals(capi):
    L = capi.lib()
    rect = (C.c_int64 * 4)(9, 9, 9, 9)
    n = C.c_int32(5)
    far = (C.c_int64 * 2)(1 << 20, 1 << 20)                                 # 8 * 2^20 cells away on both axes: 2^46 cells
    assert L.slamhip_debug_world_pack_plan(40, 24, 0, 0, 8, far, 1, rect, None, 0, C.byref(n)) == capi.ERR_INVALID
    assert n.value == 0 and list(rect) == [0, 0, 8 * (1 << 20) + 8, 8 * (1 << 20) + 8]
    assert b"8388616 x 8388616" in L.slamhip_last_error()
    with pytest.raises(capi.SlamhipError):
        capi.world_pack_plan(40, 24, 0, 0, 8, [(1 << 20, 1 << 20)])
    # 2^28 cells is the bound on R with its rows padded to whole words: 16384 x 16384 fits, one more row of tiles does not
    side = (C.c_int64 * 2)(16384 // 8 - 1, 16384 // 8 - 1)
    assert L.slamhip_debug_world_pack_plan(40, 24, 0, 0, 8, side, 1, rect, None, 0, C.byref(n)) == capi.ERR_INVALID and n.value == 2
    assert list(rect) == [0, 0, 16384, 16384]
    side = (C.c_int64 * 2)(16384 // 8, 16384 // 8 - 1)
    assert L.slamhip_debug_world_pack_plan(40, 24, 0, 0, 8, side, 1, rect, None, 0, C.byref(n)) == capi.ERR_INVALID and n.value == 0
    for bad in ((0, 24, 0, 0, 8), (40, 32769, 0, 0, 8), (40, 24, 0, 0, 12), (40, 24, 0, 0, 4), (40, 24, 1 << 60, 0, 8)):
        assert L.slamhip_debug_world_pack_plan(*bad, None, 0, rect, None, 0, C.byref(n)) == capi.ERR_INVALID, bad
    assert L.slamhip_debug_world_pack_plan(40, 24, 0, 0, 0, side, 1, rect, None, 0, C.byref(n)) == capi.ERR_INVALID      # tiles without backing
    assert L.slamhip_debug_world_pack_plan(40, 24, 0, 0, 8, None, 0, None, None, 0, C.byref(n)) == capi.ERR_INVALID
