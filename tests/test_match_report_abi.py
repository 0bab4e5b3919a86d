"""CPU-side checks of the match report (slamhip_match_report) and best-of-batch through every layer: the C-ABI declarations and
exports, the struct's size in the header, ctypes and C#, the argument checks that run before anything touches a device, the C#
stubs and their callers, the Python mirror.  No compute calls."""
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CS = os.path.join(ROOT, "bindings", "csharp", "SlamHip")
NAMES = ("slamhip_hs_match_report", "slamhip_hs_match_level_report", "slamhip_hs_match_batch_report", "slamhip_hs_match_best",
         "slamhip_hsproc_set_match_report", "slamhip_hsproc_get_report")
FIELDS = [("pose_map", 3), ("H", 9), ("dTr", 3), ("residual", 1), ("n_in_map", 1), ("n_points", 1), ("level", 1)]


@pytest.fixture(scope="module")
def capi():
    import slam.net_amd.build as b
    b.build()
    import slam.net_amd.capi as capi
    return capi


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def test_header_declares_and_library_exports(capi):
    C = capi.C
    vp, i32, fp, ip, rp = C.c_void_p, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(capi.MatchReport)
    want = {
        "slamhip_hs_match_report": [vp, fp, fp, rp],
        "slamhip_hs_match_level_report": [vp, i32, fp, i32, fp, rp],
        "slamhip_hs_match_batch_report": [vp, fp, i32, fp, rp],
        "slamhip_hs_match_best": [vp, fp, i32, fp, ip, rp],
        "slamhip_hsproc_set_match_report": [vp, i32],
        "slamhip_hsproc_get_report": [vp, rp, ip],
    }
    assert set(want) == set(NAMES)
    header = _read(capi.HEADER)
    L = capi.lib()
    for name, args in want.items():
        assert name in capi.declared_symbols(), name
        proto = re.search(r"int32_t\s+%s\s*\(([^;]*?)\)\s*;" % name, header, re.S)
        assert proto and len(proto.group(1).split(",")) == len(args), name
        assert hasattr(L, name), name
        assert L._signatures[name] == (i32, args), name


def test_struct_size_agrees_everywhere(capi):
    """sizeof(slamhip_match_report) as the header states it, the header's field list, the ctypes structure, the NumPy dtype and
    the C# struct's field list: 19 four-byte fields, 76 bytes, in one order."""
    header = _read(capi.HEADER)
    body = re.search(r"typedef struct slamhip_match_report \{(.*?)\}\s*slamhip_match_report;\s*/\*(.*?)\*/", header, re.S)
    assert body
    stated = int(re.search(r"sizeof\(slamhip_match_report\) == (\d+)", body.group(2)).group(1))
    decl = re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S)
    fields = [(m.group(2), int(m.group(3) or 1)) for m in re.finditer(r"(float|int32_t)\s+(\w+)(?:\[(\d+)\])?\s*;", decl)]
    assert fields == FIELDS
    assert stated == 4 * sum(n for _, n in fields) == 76
    assert capi.C.sizeof(capi.MatchReport) == stated and capi.REPORT_DTYPE.itemsize == stated
    assert [f[0] for f in capi.MatchReport._fields_] == [f for f, _ in FIELDS] == list(capi.REPORT_DTYPE.names)
    for name, n in FIELDS:
        assert getattr(capi.MatchReport, name).offset == capi.REPORT_DTYPE.fields[name][1], name
        assert getattr(capi.MatchReport, name).size == 4 * n, name
    cs = re.search(r"\[StructLayout\(LayoutKind\.Sequential[^\]]*\)\]\s*public struct MatchReport\s*\{(.*?)\n    \}", _read(CS, "SlamHip.Native.cs"), re.S)
    assert cs
    cs_fields = []
    for m in re.finditer(r"public (float|int) ([\w, ]+);", cs.group(1)):
        cs_fields += [(m.group(1), n.strip()) for n in m.group(2).split(",")]
    assert len(cs_fields) == 19 and [t for t, _ in cs_fields] == ["float"] * 16 + ["int"] * 3


def test_bad_arguments_are_refused_before_any_device_work(capi):
    L = capi.lib()
    C = capi.C
    f3 = (C.c_float * 3)(); o3 = (C.c_float * 3)(); r = capi.MatchReport(); idx = C.c_int32(); valid = C.c_int32()
    fp = lambda a: C.cast(a, C.POINTER(C.c_float))
    assert L.slamhip_hs_match_report(None, fp(f3), fp(o3), C.byref(r)) == capi.ERR_INVALID
    assert L.slamhip_hs_match_level_report(None, 0, fp(f3), 3, fp(o3), C.byref(r)) == capi.ERR_INVALID
    for B in (0, -1, 4):
        assert L.slamhip_hs_match_batch_report(None, fp(f3), B, fp(o3), C.byref(r)) == capi.ERR_INVALID
        assert L.slamhip_hs_match_best(None, fp(f3), B, fp(o3), C.byref(idx), C.byref(r)) == capi.ERR_INVALID
    for on in (0, 1, 2):
        assert L.slamhip_hsproc_set_match_report(None, on) == capi.ERR_INVALID
    assert L.slamhip_hsproc_get_report(None, C.byref(r), C.byref(valid)) == capi.ERR_INVALID


def test_csharp_stubs_and_callers():
    native = _read(CS, "SlamHip.Native.cs")
    counts = {"slamhip_hs_match_report": 4, "slamhip_hs_match_level_report": 6, "slamhip_hs_match_batch_report": 5,
              "slamhip_hs_match_best": 6, "slamhip_hsproc_set_match_report": 2, "slamhip_hsproc_get_report": 3}
    for name, n in counts.items():
        m = re.search(r"static\s+extern\s+int\s+%s\s*\(([^)]*)\)" % name, native)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == n, name
    sm = _read(CS, "HectorSLAM", "ScanMatcher.Hip.cs")
    for name in NAMES[:4]:
        assert "Native.%s(" % name in sm, name
    assert len(re.findall(r"public (?:unsafe )?Vector3 MatchData\([^)]*out MatchReport report\)", sm)) == 2
    assert re.search(r"public unsafe Vector3 MatchDataBest\(", sm)
    proc = _read(CS, "HectorSLAM", "HectorSLAMProcessor.Hip.cs")
    assert re.search(r"public\s+bool\s+MatchReport\b", proc) and re.search(r"public\s+SlamHip\.MatchReport\?\s+LastMatchReport\b", proc)
    for name in NAMES[4:]:
        assert "Native.%s(" % name in proc, name


def test_python_mirror_passes_arguments_through(capi, monkeypatch):
    import slam.net_amd.hector as h
    p = inspect.signature(h.HectorSLAMProcessor.__init__).parameters
    assert "matchReport" in p and p["matchReport"].default is False
    assert isinstance(h.HectorSLAMProcessor.LastMatchReport, property)
    log = []
    monkeypatch.setattr(h.capi, "call", lambda name, *a: log.append((name, a)))

    class Rep(h.MapRepMultiMap):
        def __init__(self):
            self._h = "pyramid"

        def set_scan(self, scan):
            log.append(("set_scan", scan))

    class Level:
        def __init__(self, rep):
            self._rep, self.level, self.EstimateIterations = rep, 2, 5

    rep = Rep()
    m = h.ScanMatcher(4, referenceSummation=True)
    scan = h.ScanCloud(np.zeros((3, 2), np.float32))
    hint = np.array([1, 2, 3], np.float32)

    def floats(ptr, n):
        return [ptr[i] for i in range(n)]

    pose, r = m.MatchDataReport(rep, scan, hint)
    assert [c[0] for c in log] == ["slamhip_hs_set_match_threads", "set_scan", "slamhip_hs_match_report"]
    assert log[0][1] == ("pyramid", 4)
    a = log[2][1]
    assert a[0] == "pyramid" and floats(a[1], 3) == [1, 2, 3] and len(a) == 4
    assert pose.shape == (3,) and r.dtype == capi.REPORT_DTYPE
    log.clear()
    m.MatchDataReport(Level(rep), scan, hint)
    a = log[2][1]
    assert log[2][0] == "slamhip_hs_match_level_report" and a[0] == "pyramid" and a[1] == 2 and a[3] == 5 and len(a) == 6
    hints = np.arange(15, dtype=np.float32).reshape(5, 3)
    log.clear()
    poses, reps = m.MatchDataBatchReport(rep, scan, hints)
    a = log[2][1]
    assert log[2][0] == "slamhip_hs_match_batch_report" and a[2] == 5 and floats(a[1], 15) == list(range(15))
    assert poses.shape == (5, 3) and reps.shape == (5,) and reps.dtype == capi.REPORT_DTYPE
    log.clear()
    pose, idx, r = m.MatchDataBest(rep, scan, hints)
    a = log[2][1]
    assert log[2][0] == "slamhip_hs_match_best" and a[2] == 5 and floats(a[1], 15) == list(range(15)) and len(a) == 6
    assert isinstance(idx, int)


def test_hint_lattice():
    import slam.net_amd.hector as h
    lat = h.hint_lattice((1.0, 2.0, 0.5), 0.2, 0.1, 0.05, 0.05)
    assert lat.dtype == np.float32 and lat.shape == (5 * 5 * 3, 3)
    assert (lat[0] == np.array([1.0, 2.0, 0.5], np.float32)).all()
    assert len({tuple(r) for r in lat.tolist()}) == lat.shape[0]           # every hint once
    assert np.isclose(lat[:, 0].min(), 0.8) and np.isclose(lat[:, 0].max(), 1.2) and np.isclose(lat[:, 2].max(), 0.55)
    one = h.hint_lattice((3, 4, 5), 0.0, 0.1, 0.0, 0.1)
    assert one.shape == (1, 3) and one.tolist() == [[3.0, 4.0, 5.0]]
    with pytest.raises(ValueError):
        h.hint_lattice((0, 0, 0), 1.0, 0.0, 0.1, 0.1)
