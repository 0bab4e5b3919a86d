"""CPU-side checks of the branch-and-bound pose-lattice search's interface (K24: slamhip_hs_lattice_search_bnb,
slamhip_hs_relocalise_bnb, slamhip_hsproc_relocalise_bnb, slamhip_debug_lattice_bnb) and of its host arithmetic: the hook runs rules
1 - 6 from the text the kernels share (hs_bnb.h) and is compared, with == on integers, against K7's exhaustive definition
(test_hs_lattice_abi.np_volume / np_keys -- the proof that nothing is pruned wrongly) and against the NumPy restatement of the rules
(bnb_cases.np_bnb).  No compute calls on a device."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import bnb_cases as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("slamhip_hs_lattice_search_bnb", "slamhip_hs_relocalise_bnb", "slamhip_hsproc_relocalise_bnb", "slamhip_debug_lattice_bnb")


@pytest.fixture(scope="module")
def capi():
    import slam.net_amd.build as b
    b.build()
    import slam.net_amd.capi as capi
    return capi


def hook(capi, case, **change):
    c = dict(case, **change)
    values, w, h, cell = B.level_of(c)
    spec = capi.bnb_spec(c["level"], c["centre"], c["nx"], c["ny"], c["n_theta"], c["dtheta"], c["top"], max_blocks=c.get("max_blocks", 0))
    keys, info = capi.bnb_call(values, w, h, cell, spec, c["xy"])
    return keys, B.info_dict(info)


def test_struct_sizes_match_the_header(capi):
    h = open(os.path.join(ROOT, "include", "slamhip.h")).read()
    assert "sizeof(slamhip_bnb_spec) == 48" in h and "sizeof(slamhip_bnb_info) == 88" in h
    assert C.sizeof(capi.BNB_SPEC) == 48 and C.sizeof(capi.BnbInfo) == capi.BNB_INFO.itemsize == 88
    assert [n for n, _ in capi.BNB_SPEC._fields_] == ["lattice", "top", "world", "max_blocks", "reserved"]
    assert (capi.BNB_SPEC.top.offset, capi.BNB_SPEC.world.offset, capi.BNB_SPEC.max_blocks.offset, capi.BNB_SPEC.reserved.offset) == (32, 36, 40, 44)
    assert [n for n, _ in capi.BnbInfo._fields_] == list(capi.BNB_INFO.names) == list(B.INFO_FIELDS)
    assert (capi.BnbInfo.evaluated.offset, capi.BnbInfo.blocks.offset, capi.BnbInfo.kept.offset) == (8, 16, 52)
    assert [capi.BNB_INFO.fields[n][1] for n in B.INFO_FIELDS] == [0, 4, 8, 16, 52]
    for rec, names in (("slamhip_bnb_spec", ["lattice", "top", "world", "max_blocks", "reserved"]), ("slamhip_bnb_info", list(B.INFO_FIELDS))):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (rec, rec), h, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        assert re.findall(r"\b([a-z_]+)(?:\[\d+\])?\s*;", body) == names


def test_symbols_exported_and_bound(capi):
    L = capi.lib()
    declared = set(capi.declared_symbols())
    for name in SYMBOLS:
        assert name in declared and hasattr(L, name) and name in L._signatures, name
    h = re.sub(r"[\s*/]+", " ", open(os.path.join(ROOT, "include", "slamhip.h")).read())
    for rule in ("1. Refusals", "2. Pooled maps", "3. Blocks", "4. The levels", "5. Capacity", "6. Results", "7. Blocking and memory"):
        assert rule in h, rule


def test_python_mirror_exposes_the_methods_and_keywords(capi):
    import slam.net_amd.hector as hs
    p = inspect.signature(hs.MapRepMultiMap.lattice_search_bnb).parameters
    assert list(p)[1:] == ["scan", "level", "centre", "nx", "ny", "n_theta", "dtheta", "top", "world", "max_blocks"]
    assert p["world"].default is False and p["max_blocks"].default == 0
    for fn in (hs.ScanMatcher.Relocalise, hs.ScanMatcher.RelocaliseWorld, hs.HectorSLAMProcessor.Relocalise, hs.HectorSLAMProcessor.VerifyLoop):
        p = inspect.signature(fn).parameters
        assert p["search"].default == "lattice" and p["top"].default is None, fn
    # (the processor's RelocaliseWorld keeps its pinned parameter list: the bnb form is a method of its own)
    p = inspect.signature(hs.HectorSLAMProcessor.RelocaliseWorldBnb).parameters
    assert list(p)[1:] == ["scan", "centreWorld", "level", "nx", "ny", "n_theta", "dtheta", "B", "adopt", "top"] and p["top"].default is None
    assert hs.BNB_DEFAULT_TOP == 3 and "top=None: 3, measured" in hs.ScanMatcher.Relocalise.__doc__   # profiles/r30_hs_bnb.json
    with pytest.raises(ValueError):
        hs.ScanMatcher(1).Relocalise(None, None, 0, (0, 0, 0), 1, 1, 1, 0.1, search="exhaustive")


def test_null_handles_are_refused(capi):
    L = capi.lib()
    spec = capi.bnb_spec(0, (0, 0, 0), 1, 1, 1, 0.1, 1)
    keys = (C.c_uint64 * 1)(7)
    pose = (C.c_float * 3)(1, 2, 3)
    rep, info, bnb = capi.MatchReport(), capi.RelocInfo(), capi.BnbInfo()
    bnb.top = 77
    assert L.slamhip_hs_lattice_search_bnb(None, C.byref(spec), keys, C.byref(bnb)) == capi.ERR_INVALID
    assert L.slamhip_hs_relocalise_bnb(None, C.byref(spec), 4, pose, C.byref(rep), C.byref(info), C.byref(bnb)) == capi.ERR_INVALID
    assert L.slamhip_hsproc_relocalise_bnb(None, None, 0, None, C.byref(spec), 4, 1, pose, C.byref(rep), C.byref(info), C.byref(bnb)) == capi.ERR_INVALID
    assert keys[0] == 7 and list(pose) == [1, 2, 3] and bnb.top == 77


def test_rule_1_refusals_write_nothing(capi):
    L = capi.lib()
    c = B.CASES["corner_top2"]
    values, w, h, cell = B.level_of(c)
    v = capi.f32(values); xy = capi.f32(c["xy"])
    good = dict(level=0, centre=c["centre"], nx=5, ny=3, n_theta=7, dtheta=0.4, top=2, world=0, max_blocks=0, reserved=0)
    bad = [dict(top=-1), dict(top=9), dict(world=1), dict(world=2), dict(world=-1), dict(reserved=1), dict(max_blocks=-1),
           dict(max_blocks=41),                                            # 3 * 2 * 7 = 42 top blocks
           dict(nx=-1), dict(nx=4097), dict(ny=-1), dict(ny=4097), dict(n_theta=0), dict(n_theta=4097),
           dict(nx=4096, ny=4096, n_theta=4096, top=0),                    # 2.7e11 blocks
           dict(centre=(np.nan, 0.0, 0.0)), dict(centre=(0.0, np.inf, 0.0)), dict(centre=(0.0, 0.0, -np.inf)), dict(dtheta=np.nan)]
    for change in bad:
        a = dict(good, **change)
        spec = capi.bnb_spec(a["level"], a["centre"], a["nx"], a["ny"], a["n_theta"], a["dtheta"], a["top"], a["world"], a["max_blocks"], a["reserved"])
        keys = np.full(4097, 7, np.uint64)
        info = capi.BnbInfo(); info.top = 77; info.evaluated = 5
        rc = L.slamhip_debug_lattice_bnb(capi.fptr(v), w, h, cell, C.byref(spec), capi.fptr(xy), xy.shape[0], keys.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(info))
        assert rc == capi.ERR_INVALID, change
        assert (keys == 7).all() and info.top == 77 and info.evaluated == 5, change
    with pytest.raises(capi.SlamhipError) as e:                            # exactly the top grid: rule 1 passes, rule 5 ends the search one level down
        hook(capi, c, max_blocks=42)
    assert e.value.code == capi.ERR_INVALID and "height 1" in str(e.value)


@pytest.mark.parametrize("name", list(B.CASES))
def test_hook_keys_equal_the_exhaustive_definition(capi, name):
    keys, _ = hook(capi, B.CASES[name])
    assert np.array_equal(keys, B.exhaustive_keys(name)), name


@pytest.mark.parametrize("name", list(B.CASES))
def test_hook_equals_the_restatement(capi, name):
    keys, info = hook(capi, B.CASES[name])
    want_keys, want_info = B.reference(name)
    assert np.array_equal(keys, want_keys), name
    for f in B.INFO_FIELDS:
        assert info[f] == want_info[f], (name, f, info[f], want_info[f])
    c = B.CASES[name]
    assert info["blocks"][c["top"] + 1:] == [0] * (8 - c["top"]) and info["kept"][0] == 0 and info["evaluated"] == sum(info["blocks"])


def test_what_the_catalogue_holds():
    """The properties the cases were chosen for, on the restatement alone."""
    keys, info = B.reference("empty")
    assert (keys == np.uint64(B.EMPTY_KEY)).all()
    assert info["blocks"][:3] == [11 * 7 * 7, 6 * 4 * 7, 3 * 2 * 7] and info["kept"][1:3] == info["blocks"][1:3]   # nothing pruned
    _, info = B.reference("one_peak")
    assert info["evaluated"] < B.nodes_of(B.CASES["one_peak"]) / 2
    assert any(info["kept"][h] < info["blocks"][h] for h in range(1, 3))
    k, ix, iy = B.PEAK_NODE
    c = B.CASES["one_peak"]
    top_k = max(range(c["n_theta"]), key=lambda i: int(B.reference("one_peak")[0][i]))
    assert top_k == k and 0xFFFFFFFF - (int(B.reference("one_peak")[0][k]) & 0xFFFFFFFF) == (iy + c["ny"]) * (2 * c["nx"] + 1) + ix + c["nx"]
    _, info = B.reference("corner_top4")
    assert info["blocks"][4] == 7                                          # one block per heading
    _, info = B.reference("corner_top0")
    assert info["blocks"][0] == info["evaluated"] == 539
    _, info = B.reference("wide")
    assert min(info["blocks"][:5]) > 256 * 4 // 4 and info["blocks"][0] > 4 * 256   # lower frontiers of more than one workgroup per heading
    assert len(B.CASES["many_points"]["xy"]) == 5000


# which case catches which wrong copy of the restatement
WRONG = [("corner_top2", dict(strict=True)),          # survive on U > best: a tie that holds a lower flat is pruned -- the keys differ
         ("empty", dict(strict=True)),                # ... and on the empty map everything ties: the counts collapse
         ("corner_top2", dict(short_window=True)),    # a window of 2^h - 1 cells misses the block's last row and column of nodes
         ("corner_top2", dict(outside=-1))]           # outside the map taken as free: the bound falls below scores of nodes off the map


@pytest.mark.parametrize("name,kw", WRONG)
def test_wrong_copies_differ_from_the_hook(capi, name, kw):
    c = B.CASES[name]
    keys, info = hook(capi, c)
    values, w, h, cell = B.level_of(c)
    wrong_keys, wrong_info = B.np_bnb(values, w, h, cell, c["centre"], c["nx"], c["ny"], c["n_theta"], c["dtheta"], c["top"], c["xy"], **kw)
    assert not np.array_equal(wrong_keys, keys) or wrong_info != info, (name, kw)
    if name == "corner_top2":
        assert not np.array_equal(wrong_keys, keys), (name, kw)            # wrong RESULTS, not only other counts


def test_rule_5_capacity_on_the_empty_map(capi):
    """max_blocks = 4 on the empty map: with top = 4 and one heading the top grid is 1 block (rule 1 passes); it survives, and so do its
    2 children in the 11 x 7 lattice (a in {0, 8}, b = 0); their 6 children (a in {0, 4, 8}, b in {0, 4}) are more than 4."""
    L = capi.lib()
    c = dict(B.CASES["empty"], top=4, n_theta=1)
    values, w, h, cell = B.level_of(c)
    assert B.np_bnb(values, w, h, cell, c["centre"], c["nx"], c["ny"], 1, c["dtheta"], 4, c["xy"], max_blocks=4) is None
    assert B.np_bnb(values, w, h, cell, c["centre"], c["nx"], c["ny"], 1, c["dtheta"], 4, c["xy"], max_blocks=77) is not None
    v = capi.f32(values); xy = capi.f32(c["xy"])
    spec = capi.bnb_spec(0, c["centre"], c["nx"], c["ny"], 1, c["dtheta"], 4, max_blocks=4)
    keys = np.full(1, 7, np.uint64)
    info = capi.BnbInfo(); info.top = 77
    rc = L.slamhip_debug_lattice_bnb(capi.fptr(v), w, h, cell, C.byref(spec), capi.fptr(xy), xy.shape[0], keys.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(info))
    assert rc == capi.ERR_INVALID and keys[0] == 7 and info.top == 77
    msg = L.slamhip_last_error().decode()
    assert "max_blocks" in msg and "top" in msg and "height 2" in msg and "6 blocks" in msg
    keys, info = hook(capi, c, max_blocks=77)
    assert info["blocks"][:5] == [77, 24, 6, 2, 1]
