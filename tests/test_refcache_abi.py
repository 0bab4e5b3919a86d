"""CPU-side checks of the opt-in reference probability cache (deviation D5) through every layer: the C-ABI declaration
and export, the C# stub and its callers, the Python mirror.  No compute calls."""
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CS = os.path.join(ROOT, "bindings", "csharp", "SlamHip")
NAME = "slamhip_hs_set_reference_cache"


@pytest.fixture(scope="module")
def capi():
    import slam.net_amd.build as b
    b.build()
    import slam.net_amd.capi as capi
    return capi


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def test_header_declares_setter(capi):
    assert NAME in capi.declared_symbols()
    assert re.search(r"int32_t\s+%s\s*\(\s*slamhip_hs\s*\*\s*\w+\s*,\s*int32_t\s+\w+\s*\)\s*;" % NAME, _read(capi.HEADER))


def test_library_exports_setter(capi):
    L = capi.lib()
    assert hasattr(L, NAME)
    assert L._signatures[NAME][1] == [capi.C.c_void_p, capi.C.c_int32]


def test_null_handle_is_refused(capi):
    """The argument check runs before anything touches a device: a null pyramid is SLAMHIP_ERR_INVALID for every value."""
    L = capi.lib()
    for on in (0, 1, 2):
        assert getattr(L, NAME)(None, on) == capi.ERR_INVALID, on


def test_csharp_stub_and_callers():
    m = re.search(r"static\s+extern\s+int\s+%s\s*\(([^)]*)\)" % NAME, _read(CS, "SlamHip.Native.cs"))
    assert m, "no DllImport stub"
    assert len([a for a in m.group(1).split(",") if a.strip()]) == 2
    rep = _read(CS, "HectorSLAM", "MapRepMultiMap.Hip.cs")
    assert "Native.%s(" % NAME in rep
    assert re.search(r"public\s+bool\s+ReferenceCache\b", rep)
    proc = _read(CS, "HectorSLAM", "HectorSLAMProcessor.Hip.cs")
    assert re.search(r"public\s+bool\s+ReferenceCache\b", proc)
    assert "MapRep.ReferenceCache" in proc


def test_python_mirror_surface(capi):
    import slam.net_amd.hector as h
    p = inspect.signature(h.HectorSLAMProcessor.__init__).parameters
    assert "referenceCache" in p and p["referenceCache"].default is False
    assert callable(getattr(h.MapRepMultiMap, "set_reference_cache", None))


def test_python_mirror_passes_the_value(capi, monkeypatch):
    """set_reference_cache hands its value to the C-ABI unchanged (so 2 reaches the library's check), and the processor
    turns the mode on only when asked."""
    import slam.net_amd.hector as h
    log = []
    monkeypatch.setattr(h.capi, "call", lambda name, *a: log.append((name, a)))

    class Rep(h.MapRepMultiMap):
        def __init__(self):
            self._h = "pyramid"

    rep = Rep()
    for v, want in ((True, 1), (False, 0), (1, 1), (2, 2)):
        log.clear()
        rep.set_reference_cache(v)
        assert log == [(NAME, ("pyramid", want))], log
