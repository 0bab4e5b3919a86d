"""CPU-side checks of the matcher's reference summation order through every layer: the C-ABI declaration and export, the
C# stub and its callers, the Python mirror.  No compute calls."""
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CS = os.path.join(ROOT, "bindings", "csharp", "SlamHip")
NAME = "slamhip_hs_set_match_threads"


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


def test_csharp_stub_and_callers():
    m = re.search(r"static\s+extern\s+int\s+%s\s*\(([^)]*)\)" % NAME, _read(CS, "SlamHip.Native.cs"))
    assert m, "no DllImport stub"
    assert len([a for a in m.group(1).split(",") if a.strip()]) == 2
    for f in ("ScanMatcher.Hip.cs", "HectorSLAMProcessor.Hip.cs"):
        assert "Native.%s(" % NAME in _read(CS, "HectorSLAM", f), f
    sm = _read(CS, "HectorSLAM", "ScanMatcher.Hip.cs")
    assert re.search(r"public\s+ScanMatcher\s*\(\s*int\s+numThreads\s*,\s*ILogger\s+logger\s*,\s*bool\s+referenceSummation\s*\)", sm)
    assert re.search(r"public\s+bool\s+ReferenceSummation\b", _read(CS, "HectorSLAM", "HectorSLAMProcessor.Hip.cs"))


def test_python_mirror_accepts_reference_summation(capi):
    import slam.net_amd.hector as h
    for cls in (h.ScanMatcher, h.HectorSLAMProcessor):
        p = inspect.signature(cls.__init__).parameters
        assert "referenceSummation" in p and p["referenceSummation"].default is False, cls
    assert callable(getattr(h.MapRepMultiMap, "set_match_threads", None))


def test_python_matcher_sets_order_before_every_match(capi, monkeypatch):
    """ScanMatcher sets numThreads (referenceSummation) or 0 (default) on the target pyramid before each native match."""
    import slam.net_amd.hector as h
    log = []
    monkeypatch.setattr(h.capi, "call", lambda name, *a: log.append((name, a[1] if name == NAME else None)))

    class Rep(h.MapRepMultiMap):
        def __init__(self):
            self._h = None
            self.Maps = []

    rep = Rep()
    grid = h.OccGridMap.__new__(h.OccGridMap)
    grid._rep, grid.level, grid._iters = rep, 1, 3
    scan = h.ScanCloud([[1.0, 2.0]])
    for ref, want in ((True, 7), (False, 0)):
        m = h.ScanMatcher(7, referenceSummation=ref)
        for call in (lambda: m.MatchData(rep, scan, [0, 0, 0]), lambda: m.MatchData(grid, scan, [0, 0, 0]),
                     lambda: m.MatchDataBatch(rep, scan, [[0, 0, 0], [1, 1, 0]])):
            log.clear()
            call()
            assert log[0] == (NAME, want), log
            assert log[-1][0] in ("slamhip_hs_match", "slamhip_hs_match_level", "slamhip_hs_match_batch"), log
