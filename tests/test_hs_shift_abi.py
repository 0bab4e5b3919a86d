"""CPU-side checks of the scrolling map window's interface (slamhip_hs_shift, slamhip_hs_origin, slamhip_hsproc_set_scroll,
slamhip_hsproc_get_origin): exported, declared, stated in the header, mirrored in Python and in the C# shim.  No compute calls."""
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("slamhip_hs_shift", "slamhip_hs_origin", "slamhip_hsproc_set_scroll", "slamhip_hsproc_get_origin")


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
    assert "int32_t slamhip_hs_shift(slamhip_hs *hs, int32_t dx, int32_t dy);" in h
    assert "int32_t slamhip_hs_origin(slamhip_hs *hs, int64_t *ox, int64_t *oy);" in h
    assert "int32_t slamhip_hsproc_set_scroll(slamhip_hsproc *p, int32_t trigger_cells);" in h
    assert "int32_t slamhip_hsproc_get_origin(slamhip_hsproc *p, int64_t *ox, int64_t *oy);" in h


def test_header_states_the_contract():
    h = re.sub(r"[\s*/]+", " ", header_text())
    assert "multiple of g = 1 << (levels - 1)" in h                       # the multiple-of-g rule
    assert "p - origin cell_length(level 0)" in h                          # where a world point lies in the window's frame
    assert "12 bytes per cell and level" in h                              # what the first shift allocates
    assert "min(w0, h0) 2 - g" in h                                        # the trigger's valid range
    assert re.search(r"slamhip_hsproc_get_report.{0,40}", h) and "pose_map stays in the WINDOW's frame" in h


def test_null_handles_are_refused(capi):
    """Argument checks run before anything touches a device: a null handle is SLAMHIP_ERR_INVALID, not a crash."""
    import ctypes as C
    L = capi.lib()
    ox, oy = C.c_int64(7), C.c_int64(7)
    assert L.slamhip_hs_shift(None, 4, 0) == capi.ERR_INVALID
    assert L.slamhip_hs_origin(None, C.byref(ox), C.byref(oy)) == capi.ERR_INVALID
    assert L.slamhip_hsproc_set_scroll(None, 8) == capi.ERR_INVALID
    assert L.slamhip_hsproc_get_origin(None, C.byref(ox), C.byref(oy)) == capi.ERR_INVALID
    assert (ox.value, oy.value) == (7, 7)


def test_python_mirror_exposes_the_methods(capi):
    import slam.net_amd.hector as hs
    for name in ("shift", "origin"):
        assert callable(getattr(hs.MapRepMultiMap, name)), name
    for name in ("set_scroll", "get_origin"):
        assert callable(getattr(hs.HectorSLAMProcessor, name)), name
    p = inspect.signature(hs.HectorSLAMProcessor.__init__).parameters
    assert "scrollTrigger" in p and p["scrollTrigger"].default == 0


def test_csharp_shim_declares_the_imports():
    shim = os.path.join(ROOT, "bindings", "csharp", "SlamHip")
    native = open(os.path.join(shim, "SlamHip.Native.cs")).read()
    for name in SYMBOLS:
        assert re.search(r"\[DllImport\(Lib\)\] internal static extern int %s\(" % name, native), name
    rep = open(os.path.join(shim, "HectorSLAM", "MapRepMultiMap.Hip.cs")).read()
    assert "public void Shift(int dx, int dy)" in rep and "Native.slamhip_hs_shift(" in rep
    assert re.search(r"public \(long X, long Y\) Origin", rep) and "Native.slamhip_hs_origin(" in rep
    proc = open(os.path.join(shim, "HectorSLAM", "HectorSLAMProcessor.Hip.cs")).read()
    assert "public int ScrollTrigger" in proc and "Native.slamhip_hsproc_set_scroll(" in proc
    assert "Native.slamhip_hsproc_get_origin(" in proc
    # the reference's own `offset` stays unsupported, and says where to go instead
    grid = open(os.path.join(shim, "HectorSLAM", "GridMap.Hip.cs")).read()
    for txt in (rep, grid):
        m = re.search(r"throw new NotSupportedException\(\"the device maps have no offset[^\"]*\"\)", txt)
        assert m and "Shift" in m.group(0)
