"""CPU-side checks of the pose-lattice search's interface (slamhip_hs_lattice_search, slamhip_hs_lattice_node_pose,
slamhip_hs_relocalise, slamhip_hsproc_relocalise, slamhip_debug_lattice_cells), and the NumPy restatement of its definition
(include/slamhip.h, slamhip_lattice_spec) that tests/test_gpu_hector_lattice.py compares the device with: np.float32 operations
one at a time, np_oracle.det_sincos for the trigonometry, integer fancy-indexing for the correlation.  Everything is compared with
== on integers and on bit patterns.  No compute calls on a device."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest

import np_oracle as npo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("slamhip_hs_lattice_search", "slamhip_hs_lattice_node_pose", "slamhip_hs_relocalise", "slamhip_hsproc_relocalise",
           "slamhip_debug_lattice_cells")
F = np.float32
I32_MIN = -2 ** 31
LIMIT = F(16777216.0)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def np_theta(centre, k, dtheta):
    """theta_k = centre[2] + (float)k * dtheta, product and sum each rounded to binary32."""
    return F(F(centre[2]) + F(F(k) * F(dtheta)))


def np_point_cells(stm, centre, theta, xy):
    """-> (gx, gy, valid): the cells of the points for one heading; gx, gy are int64 and meaningless where valid is False."""
    stm = F(stm); xy = np.asarray(xy, np.float32).reshape(-1, 2)
    s, c = npo.det_sincos(F(theta))
    s, c = F(s), F(c)
    cxm, cym = F(F(centre[0]) * stm), F(F(centre[1]) * stm)
    px, py = xy[:, 0], xy[:, 1]
    with np.errstate(invalid="ignore", over="ignore"):
        rx = (c * px) - (s * py)                                           # (float32 arrays: every operation rounds on its own)
        ry = (s * px) + (c * py)
        fx = (rx * stm) + cxm
        fy = (ry * stm) + cym
        assert fx.dtype == np.float32 and fy.dtype == np.float32
        valid = (np.abs(fx) < LIMIT) & (np.abs(fy) < LIMIT)
        gx = np.where(valid, np.floor(fx), 0).astype(np.int64)
        gy = np.where(valid, np.floor(fy), 0).astype(np.int64)
    return gx, gy, valid


def np_classes(values, w, h):
    """cls of every cell: +1 where Value > 0, -1 where Value < 0, 0 for +0, -0 and NaN."""
    v = np.asarray(values, np.float32).reshape(h, w)
    with np.errstate(invalid="ignore"):
        return (v > 0).astype(np.int32) - (v < 0).astype(np.int32)


def np_volume(values, w, h, cell, centre, nx, ny, n_theta, dtheta, xy):
    """The whole score volume (n_theta, 2 ny + 1, 2 nx + 1), int32."""
    cls = np_classes(values, w, h)
    stm = F(1.0) / F(cell)
    ixs = np.arange(-nx, nx + 1, dtype=np.int64)
    out = np.zeros((n_theta, 2 * ny + 1, 2 * nx + 1), np.int32)
    for k in range(n_theta):
        gx, gy, valid = np_point_cells(stm, centre, np_theta(centre, k, dtheta), xy)
        gx, gy = gx[valid], gy[valid]
        X = gx[None, :] + ixs[:, None]                                     # (ix, point)
        okx = (X >= 0) & (X < w)
        Xc = np.clip(X, 0, w - 1)
        for iy in range(-ny, ny + 1):
            Y = gy + iy
            ok = okx & ((Y >= 0) & (Y < h))[None, :]
            vals = cls[np.clip(Y, 0, h - 1)[None, :], Xc]
            out[k, iy + ny] = np.where(ok, vals, 0).sum(axis=1, dtype=np.int64).astype(np.int32)
    return out


def np_keys(vol):
    """key[k] = max over the nodes of ((uint32)score ^ 0x80000000) << 32 | (0xFFFFFFFF - flat)."""
    n_theta = vol.shape[0]
    flat = np.arange(vol.shape[1] * vol.shape[2], dtype=np.uint64)
    sc = (vol.reshape(n_theta, -1).astype(np.int64) & 0xFFFFFFFF).astype(np.uint64) ^ np.uint64(0x80000000)
    keys = (sc << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - flat)[None, :]
    return keys.max(axis=1)


def np_node_pose(cell, centre, nx, ny, dtheta, k, flat):
    cell = F(cell); stm = F(1.0) / cell
    NX = 2 * nx + 1
    ix, iy = flat % NX - nx, flat // NX - ny
    cxm, cym = F(F(centre[0]) * stm), F(F(centre[1]) * stm)
    return np.array([F(F(cxm + F(ix)) * cell), F(F(cym + F(iy)) * cell), np_theta(centre, k, dtheta)], np.float32)


# ---- the interface -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def capi():
    import slam.net_amd.build as b
    b.build()
    import slam.net_amd.capi as capi
    return capi


def header_text():
    return open(os.path.join(ROOT, "include", "slamhip.h")).read()


def test_struct_sizes_match_the_header(capi):
    h = header_text()
    assert "sizeof(slamhip_lattice_spec) == 32" in h and "sizeof(slamhip_reloc_info) == 28" in h
    assert C.sizeof(capi.LATTICE_SPEC) == 32
    assert [n for n, _ in capi.LATTICE_SPEC._fields_] == ["level", "nx", "ny", "n_theta", "centre", "dtheta"]
    assert capi.LATTICE_SPEC.centre.offset == 16 and capi.LATTICE_SPEC.dtheta.offset == 28
    assert C.sizeof(capi.RelocInfo) == capi.RELOC_INFO.itemsize == 28
    assert list(capi.RELOC_INFO.names) == ["n_hints", "best_hint", "k", "ix", "iy", "score", "top_score"]
    body = re.search(r"typedef struct slamhip_reloc_info \{(.*?)\} slamhip_reloc_info;", h, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b([a-z_]+)\s*[,;]", body) == list(capi.RELOC_INFO.names)


def test_symbols_exported_and_declared(capi):
    L = capi.lib()
    declared = set(capi.declared_symbols())
    for name in SYMBOLS:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in L._signatures, name
    h = re.sub(r"[\s*/]+", " ", header_text())
    assert "no reference counterpart" in h
    assert "The search covers the window only" in h


def test_null_handles_are_refused(capi):
    L = capi.lib()
    spec = capi.lattice_spec(0, (0, 0, 0), 1, 1, 1, 0.1)
    keys = (C.c_uint64 * 1)(7)
    pose = (C.c_float * 3)(1, 2, 3)
    rep, info = capi.MatchReport(), capi.RelocInfo()
    assert L.slamhip_hs_lattice_search(None, C.byref(spec), keys, None) == capi.ERR_INVALID
    assert L.slamhip_hs_lattice_node_pose(None, C.byref(spec), 0, 0, pose) == capi.ERR_INVALID
    assert L.slamhip_hs_relocalise(None, C.byref(spec), 4, pose, C.byref(rep), C.byref(info)) == capi.ERR_INVALID
    assert L.slamhip_hsproc_relocalise(None, None, 0, None, C.byref(spec), 4, 1, pose, C.byref(rep), C.byref(info)) == capi.ERR_INVALID
    assert keys[0] == 7 and list(pose) == [1, 2, 3]


def test_python_mirror_exposes_the_methods(capi):
    import slam.net_amd.hector as hs
    assert callable(hs.MapRepMultiMap.lattice_search) and callable(hs.ScanMatcher.Relocalise)
    p = inspect.signature(hs.HectorSLAMProcessor.Relocalise).parameters
    assert "adopt" in p and p["adopt"].default is True
    p = inspect.signature(hs.MapRepMultiMap.lattice_search).parameters
    assert list(p)[1:] == ["scan", "level", "centre", "nx", "ny", "n_theta", "dtheta", "scores"] and p["scores"].default is False
    for score, flat in ((0, 0), (-1, 15), (-2 ** 31, 0), (2 ** 31 - 1, 2 ** 26 - 1), (5, 7)):
        key = (((score & 0xFFFFFFFF) ^ 0x80000000) << 32) | (0xFFFFFFFF - flat)
        assert hs.decode_lattice_key(key) == (score, flat)
        assert hs.decode_lattice_key(np.uint64(key)) == (score, flat)
    assert hs.decode_lattice_key(0x80000000FFFFFFFF) == (0, 0)


def test_csharp_shim_declares_the_imports():
    shim = os.path.join(ROOT, "bindings", "csharp", "SlamHip")
    native = open(os.path.join(shim, "SlamHip.Native.cs")).read()
    for name in SYMBOLS:
        assert re.search(r"\[DllImport\(Lib\)\] internal static extern int %s\(" % name, native), name
    assert re.search(r"\[StructLayout\(LayoutKind\.Sequential\)\]\s*(?:public|internal) struct LatticeSpec", native)
    proc = open(os.path.join(shim, "HectorSLAM", "HectorSLAMProcessor.Hip.cs")).read()
    assert "Relocalise(" in proc and "Native.slamhip_hsproc_relocalise(" in proc


# ---- slamhip_debug_lattice_cells against the restatement ---------------------------------------------------------------------------
def _next(v, up):
    return np.nextafter(F(v), F(np.inf) if up else F(-np.inf))


def lattice_cases():
    """(cell, centre, theta, xy) cases: random points x headings, with the headings at and next to 0, +-pi/2 and pi (where
    Matrix3x2.CreateRotation, and hs_rotation_sc after it, snap sine and cosine -- the lattice does not), NaN points, points that
    land at |f| >= 2^24 and just below, and negative coordinates, where floorf and truncation differ."""
    rng = np.random.default_rng(20240611)
    pi = F(math.pi)
    special = []
    for a in (F(0.0), pi / F(2), -pi / F(2), pi, -pi):
        special += [a, _next(a, True), _next(a, False), F(a + F(1e-5)), F(a - F(1e-5))]
    thetas = special + [F(v) for v in rng.uniform(-7.0, 7.0, 15)]
    cases = []
    for i, th in enumerate(thetas):
        cell = F([0.025, 0.05, 0.1, 0.2, 0.4][i % 5])
        centre = np.array([rng.uniform(-3, 20), rng.uniform(-3, 20), rng.uniform(-3, 3)], np.float32)
        xy = rng.uniform(-25.0, 25.0, (12, 2)).astype(np.float32)
        xy[0] = (np.nan, 1.0)
        xy[1] = (2.0, np.nan)
        xy[2] = (F(2.0 ** 24) * cell, 0.0)                                  # |f| >= 2^24 at heading 0; far off at any heading
        xy[3] = (-1e30, 1e30)
        xy[4] = (np.inf, 0.0)
        xy[5] = (-0.3 * float(cell), -0.7 * float(cell))                    # negative map coordinates near zero
        xy[6] = (0.0, -0.0)
        cases.append((cell, centre, th, xy))
    # exactly at the limit: centre 0, heading 0 (s = 0, c = 1), stm = 1 / cell exact in binary32
    lim = np.array([[2.0 ** 23, 0.0], [_next(2.0 ** 23, False), 0.0], [-2.0 ** 23, 0.0], [0.0, 2.0 ** 23], [0.0, -_next(2.0 ** 23, False)]], np.float32)
    cases.append((F(0.5), np.zeros(3, np.float32), F(0.0), lim))
    return cases


def test_debug_lattice_cells_equals_the_restatement(capi):
    total = ignored = negative = 0
    for cell, centre, th, xy in lattice_cases():
        got = capi.lattice_cells(cell, centre, th, xy)
        gx, gy, valid = np_point_cells(F(1.0) / F(cell), centre, th, xy)
        want = np.where(valid[:, None], np.stack([gx, gy], 1), I32_MIN)
        assert np.array_equal(got.astype(np.int64), want), (cell, centre, th, got, want)
        total += len(xy); ignored += int((~valid).sum()); negative += int((want[valid] < 0).sum())
    assert total >= 300 and ignored >= 100 and negative >= 20
    # the limit case itself: 2^23 / 0.5 = 2^24 is ignored, the float below it is not
    cell, centre, th, xy = lattice_cases()[-1]
    got = capi.lattice_cells(cell, centre, th, xy)
    assert got[0].tolist() == [I32_MIN, I32_MIN] and got[2].tolist() == [I32_MIN, I32_MIN] and got[3].tolist() == [I32_MIN, I32_MIN]
    assert got[1].tolist() == [2 ** 24 - 1, 0] and got[4].tolist() == [0, -(2 ** 24 - 1)]
    # the lattice does not snap: next to pi / 2 the cosine is the routine's own small number, not 0
    s, c = npo.det_sincos(F(math.pi) / F(2))
    assert c != 0 and capi.lattice_cells(F(1.0), (0.0, 0.0, 0.0), F(math.pi) / F(2), [[1.0e6, 0.0]])[0, 0] == int(np.floor(F(c) * F(1.0e6)))


def test_debug_lattice_cells_refuses_bad_arguments(capi):
    L = capi.lib()
    out = (C.c_int32 * 2)(5, 5)
    xy = (C.c_float * 2)(1, 1)
    c = (C.c_float * 3)(0, 0, 0)
    assert L.slamhip_debug_lattice_cells(0.1, None, 0.0, xy, 1, out) == capi.ERR_INVALID
    assert L.slamhip_debug_lattice_cells(0.1, c, 0.0, None, 1, out) == capi.ERR_INVALID
    assert L.slamhip_debug_lattice_cells(0.1, c, 0.0, xy, -1, out) == capi.ERR_INVALID
    assert L.slamhip_debug_lattice_cells(0.0, c, 0.0, xy, 1, out) == capi.ERR_INVALID
    assert list(out) == [5, 5]
    assert L.slamhip_debug_lattice_cells(0.1, c, 0.0, None, 0, None) == 0


def test_restatement_on_a_hand_made_map():
    """The correlation itself on a map small enough to check by eye: 4 x 3 cells of 1 m, two points, heading 0."""
    values = np.array([[1, -1, 0, np.nan], [-0.0, 2, -3, 0.0], [5, 5, -1, -1]], np.float32)
    xy = np.array([[0.5, 0.5], [2.5, 1.5]], np.float32)                    # cells (0, 0) and (2, 1)
    vol = np_volume(values, 4, 3, 1.0, (0.0, 0.0, 0.0), 1, 1, 1, 0.0, xy)
    # node (ix, iy): cls(0 + ix, 0 + iy) + cls(2 + ix, 1 + iy)
    assert vol[0].tolist() == [[0 - 1, 0 + 0, 0 + 0], [0 + 1, 1 - 1, -1 + 0], [0 + 1, 0 - 1, 1 - 1]]
    keys = np_keys(vol)
    assert int(keys[0]) == ((1 ^ 0x80000000) << 32) | (0xFFFFFFFF - 3)    # score 1 first at flat 3 (iy = 0, ix = -1)
    assert np_node_pose(1.0, (0.25, 0.5, 0.1), 1, 1, 0.2, 3, 3).tolist() == [F(-0.75), F(0.5), F(F(0.1) + F(F(3) * F(0.2)))]
