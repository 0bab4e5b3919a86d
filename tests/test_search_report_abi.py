"""CPU-side checks of the CoreSLAM search report (slamhip_search_report) through every layer: the struct's size and field
offsets in the header (compiled with the host C compiler), ctypes and NumPy; the C-ABI declarations, exports and bindings; the
argument checks that run before anything touches a device; the C# stubs and their callers; the Python mirror.  No compute calls."""
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CS = os.path.join(ROOT, "bindings", "csharp", "SlamHip")
ARGS = {"slamhip_cs_search_report": 5, "slamhip_cs_search_distances": 3, "slamhip_cs_search_and_update_report": 8,
        "slamhip_cs_scan_search_and_update_report": 10, "slamhip_csproc_set_search_report": 3, "slamhip_csproc_get_report": 3}
FIELDS = [("sum_off", "double", 3), ("sum_off2", "double", 6), ("best_dist", "int32_t", 1), ("best_index", "int32_t", 1),
          ("runner_dist", "int32_t", 1), ("runner_index", "int32_t", 1), ("dist0", "int32_t", 1), ("n_candidates", "int32_t", 1),
          ("n_unscored", "int32_t", 1), ("n_ties", "int32_t", 1), ("band", "int32_t", 1), ("n_band", "int32_t", 1),
          ("n_in_map", "int32_t", 1), ("n_points", "int32_t", 1)]


@pytest.fixture(scope="module")
def capi():
    import slam.net_amd.build as b
    b.build()
    import slam.net_amd.capi as capi
    return capi


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def test_dtype_is_120_bytes_in_the_header_s_order(capi):
    assert capi.SEARCH_REPORT_DTYPE.itemsize == 120 and capi.C.sizeof(capi.SearchReport) == 120
    body = re.search(r"typedef struct slamhip_search_report \{(.*?)\}\s*slamhip_search_report;\s*/\*(.*?)\*/", _read(capi.HEADER), re.S)
    assert body and int(re.search(r"sizeof\(slamhip_search_report\) == (\d+)", body.group(2)).group(1)) == 120
    decl = re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S)
    fields = []
    for m in re.finditer(r"(double|int32_t)\s+([^;]+);", decl):
        for item in m.group(2).split(","):
            n = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", item)
            fields.append((n.group(1), m.group(1), int(n.group(2) or 1)))
    assert fields == FIELDS
    assert list(capi.SEARCH_REPORT_DTYPE.names) == [f for f, _, _ in FIELDS] == [f[0] for f in capi.SearchReport._fields_]
    for name, typ, n in FIELDS:
        assert capi.SEARCH_REPORT_DTYPE.fields[name][0].base == (np.float64 if typ == "double" else np.int32), name
        assert getattr(capi.SearchReport, name).offset == capi.SEARCH_REPORT_DTYPE.fields[name][1], name
        assert getattr(capi.SearchReport, name).size == (8 if typ == "double" else 4) * n, name


def test_field_offsets_equal_the_c_struct_s(capi, tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a host C compiler is needed"
    src = tmp_path / "offsets.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "slamhip.h"', 'int main(void) {',
             '    printf("sizeof %zu\\n", sizeof(slamhip_search_report));']
    lines += ['    printf("%s %%zu\\n", offsetof(slamhip_search_report, %s));' % (f, f) for f, _, _ in FIELDS]
    lines += ['    return 0;', '}']
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "offsets"
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(capi.HEADER), str(src), "-o", str(exe)])
    out = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(out["sizeof"]) == 120
    for f, _, _ in FIELDS:
        assert int(out[f]) == capi.SEARCH_REPORT_DTYPE.fields[f][1] == getattr(capi.SearchReport, f).offset, f


def test_header_declares_library_exports_capi_binds(capi):
    C = capi.C
    vp, i32, f, fp, ip, srp = C.c_void_p, C.c_int32, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(capi.SearchReport)
    want = {
        "slamhip_cs_search_report": [vp, fp, i32, fp, srp],
        "slamhip_cs_search_distances": [vp, ip, i32],
        "slamhip_cs_search_and_update_report": [vp, fp, i32, f, i32, i32, fp, srp],
        "slamhip_cs_scan_search_and_update_report": [vp, fp, i32, fp, i32, f, i32, i32, fp, srp],
        "slamhip_csproc_set_search_report": [vp, i32, i32],
        "slamhip_csproc_get_report": [vp, srp, ip],
    }
    assert set(want) == set(ARGS)
    header = _read(capi.HEADER)
    L = capi.lib()
    for name, args in want.items():
        assert name in capi.declared_symbols(), name
        proto = re.search(r"int32_t\s+%s\s*\(([^;]*?)\)\s*;" % name, header, re.S)
        assert proto and len(proto.group(1).split(",")) == len(args) == ARGS[name], name
        assert hasattr(L, name), name
        assert L._signatures[name] == (i32, args), name
    # the header says what the report forms give up, and that the library sets no threshold
    assert "no threshold" in header and "ordinary launch order" in header


def test_null_handles_are_refused_and_nothing_crashes(capi):
    L = capi.lib()
    C = capi.C
    f3 = (C.c_float * 3)(); o3 = (C.c_float * 3)(); r = capi.SearchReport(); valid = C.c_int32(); d = (C.c_int32 * 4)()
    fp = lambda a: C.cast(a, C.POINTER(C.c_float))
    ipt = lambda a: C.cast(a, C.POINTER(C.c_int32))
    for band in (0, 5, -1):
        assert L.slamhip_cs_search_report(None, fp(f3), band, fp(o3), C.byref(r)) < 0
        assert L.slamhip_cs_search_and_update_report(None, fp(f3), band, C.c_float(0.6), 50, 10, fp(o3), C.byref(r)) < 0
        assert L.slamhip_cs_scan_search_and_update_report(None, fp(f3), 1, fp(f3), band, C.c_float(0.6), 50, 10, fp(o3), C.byref(r)) < 0
    assert L.slamhip_cs_search_report(None, fp(f3), 0, fp(o3), None) == capi.ERR_INVALID
    assert L.slamhip_cs_search_distances(None, ipt(d), 4) == capi.ERR_INVALID
    for on, band in ((0, 0), (1, 0), (2, 0), (1, -1)):
        assert L.slamhip_csproc_set_search_report(None, on, band) == capi.ERR_INVALID
    assert L.slamhip_csproc_get_report(None, C.byref(r), C.byref(valid)) == capi.ERR_INVALID
    assert L.slamhip_last_error()


def test_csharp_stubs_struct_and_callers():
    native = _read(CS, "SlamHip.Native.cs")
    for name, n in ARGS.items():
        if name.startswith("slamhip_csproc_"):
            continue                                       # (the C# CoreSLAMProcessor keeps its own state machine on slamhip_cs: no slamhip_csproc_* stub)
        m = re.search(r"static\s+extern\s+int\s+%s\s*\(([^)]*)\)" % name, native)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == n, name
    cs = re.search(r"\[StructLayout\(LayoutKind\.Sequential[^\]]*\)\]\s*public (?:unsafe )?struct SearchReport\s*\{(.*?)\n    \}", native, re.S)
    assert cs
    cs_fields = []
    for m in re.finditer(r"public (double|int) ([\w, ]+);", cs.group(1)):
        cs_fields += [(m.group(1), n.strip()) for n in m.group(2).split(",")]
    assert [t for t, _ in cs_fields] == ["double"] * 9 + ["int"] * 12                 # blittable: 9 doubles + 12 ints, 120 bytes
    proc = _read(CS, "CoreSLAM", "CoreSLAMProcessor.Hip.cs")
    assert re.search(r"public\s+SlamHip\.SearchReport\?\s+LastSearchReport\b", proc)
    assert re.search(r"public\s+bool\s+SearchReport\b", proc) and re.search(r"public\s+int\s+ReportBand\b", proc)
    assert "Native.slamhip_cs_scan_search_and_update_report(" in proc and "Native.slamhip_cs_search_distances(" in proc


def test_python_mirror(capi, monkeypatch):
    import slam.net_amd.coreslam as m
    p = inspect.signature(m.CoreSLAMProcessor.__init__).parameters
    assert p["searchReport"].default is False and p["reportBand"].default == 0
    assert isinstance(m.CoreSLAMProcessor.LastSearchReport, property)
    log = []
    monkeypatch.setattr(m.capi, "call", lambda name, *a: log.append((name, a)))
    dev = m.CoreSlamDevice.__new__(m.CoreSlamDevice)
    dev._h, dev.n_offsets = "cs", 7
    pose, rep = dev.search_report((1, 2, 3), 9)
    assert log[-1][0] == "slamhip_cs_search_report" and log[-1][1][0] == "cs" and log[-1][1][2] == 9 and len(log[-1][1]) == 5
    assert pose.shape == (3,) and rep.dtype == capi.SEARCH_REPORT_DTYPE
    d = dev.search_distances()
    assert log[-1][0] == "slamhip_cs_search_distances" and log[-1][1][2] == 8 and d.shape == (8,) and d.dtype == np.int32
    dev.search_and_update_report((1, 2, 3), 4, 0.5, 40, 9)
    assert log[-1][0] == "slamhip_cs_search_and_update_report" and log[-1][1][2] == 4 and len(log[-1][1]) == 8
    dev.search_and_update_report((1, 2, 3), 4, 0.5, 40, 9, xy=np.zeros((6, 2), np.float32))
    assert log[-1][0] == "slamhip_cs_scan_search_and_update_report" and log[-1][1][2] == 6 and log[-1][1][4] == 4 and len(log[-1][1]) == 10
