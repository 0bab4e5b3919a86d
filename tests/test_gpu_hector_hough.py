"""The Hough transform of a map, the rotation scores and the row correlations (slamhip_hs_hough, _hough_rotation, _hough_shifts,
_hough_clear, the slamhip_hsproc_hough* calls and HectorSLAMProcessor.AlignMaps) on the device, against the host hooks and the NumPy
restatement of the definition in tests/test_hs_hough_abi.py, fed from cells_download / world_cells_download.  Everything is compared
with == on integers; there is no tolerance anywhere.

Shapes are the smallest at which each path can go wrong: maps below, at and above k17_vote's 64 x 64 tile in both axes and with a
width that is no multiple of 16, angle counts below and above its 64-angle chunk (4, 8, 12, 180), one 512 x 512 level whose sites fill
many tiles per chunk and whose rows take several 256-shift blocks of k17_xcorr.  (A window is at least 2 x 2 cells: the 1-cell-wide
shapes of the CPU file run as merge sources, slot 1.)"""
import math

import numpy as np
import pytest

import test_gpu_hector_dfield as G
import test_gpu_hector_lattice as L
import test_gpu_hector_trace as TR
import test_hs_dfield_abi as D
import test_hs_hough_abi as A
from test_gpu_hector_shift import hs_mod, ctx                              # noqa: F401 (fixtures)

gpu = pytest.mark.gpu
F = np.float32
POOL = 64 << 20


def values_of(cls):
    return np.select([cls == 1, cls == 2], [F(1.5), F(-0.7)], F(0.0)).astype(np.float32)


def rep_of(hs_mod, ctx, cls, levels=1):
    h, w = cls.shape
    rep = hs_mod.MapRepMultiMap(0.1, (w, h), levels, ctx=ctx)
    L.put_values(hs_mod, rep, 0, values_of(cls).ravel())
    return rep


def cells_of(hs_mod, cls):
    c = np.zeros(cls.shape, hs_mod.capi.CELL_DTYPE)
    c["value"] = values_of(cls); c["update_index"] = -1
    return c


def slot_equals(hs_mod, rep, slot, cls, origin, mask, T, q, level=0, world=False):
    """The device's H, spectrum and info of one fill == the restatement == the hook."""
    info, HS, H = rep.hough(level, slot, world, mask, T, q, H=True)
    wH, wHS, n = A.np_hough(cls, mask, T, q)
    Dd, N = A.np_bins(cls.shape[1], cls.shape[0], q)
    assert info == {"w": cls.shape[1], "h": cls.shape[0], "x0": origin[0], "y0": origin[1], "D": Dd, "N": N, "n_sites": n}, info
    assert H.dtype == np.uint32 and H.shape == wH.shape and np.array_equal(H, wH), (cls.shape, slot, mask, T, q, np.argwhere(H != wH)[:5].tolist())
    assert HS.dtype == np.uint64 and np.array_equal(HS, wHS)
    gH, gS = hs_mod.capi.debug_hough(cls, mask, T, q)
    assert np.array_equal(H, gH) and np.array_equal(HS, gS)
    info2, HS2, none = rep.hough(level, slot, world, mask, T, q)           # without out_H: the same spectrum
    assert none is None and info2 == info and np.array_equal(HS2, HS)
    return info, HS, H


def shape_map(w, h):
    c = A.class_map(w, h, 17)
    c[0, 0] = c[h - 1, w - 1] = c[0, w - 1] = c[h - 1, 0] = 1
    return c


# ---- 1. the CPU file's shapes and masks ----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("w,h", [s for s in A.SHAPES if min(s) >= 2])
def test_shapes_window(hs_mod, ctx, w, h):
    c = shape_map(w, h)
    rep = rep_of(hs_mod, ctx, c)
    for T in A.TS:
        for q in A.QS:
            slot_equals(hs_mod, rep, 0, c, (0, 0), 2, T, q)
    for mask in (1, 4, 7, 3):
        slot_equals(hs_mod, rep, 0, c, (0, 0), mask, 12, 1)
    slot_equals(hs_mod, rep, 0, c, (0, 0), 2, 180, 0, world=True)          # backing off: the world is the window
    rep.close()


@gpu
@pytest.mark.parametrize("w,h", A.SHAPES)
def test_shapes_source(hs_mod, ctx, w, h):
    """Slot 1 after merge_set_source with (ax, ay) negative and large."""
    c = shape_map(w, h)
    rep = hs_mod.MapRepMultiMap(0.1, (16, 16), 1, ctx=ctx)
    ax, ay = -(1 << 29) - 7, (1 << 30)
    rep.merge_set_source(0, ax, ay, cells_of(hs_mod, c))
    for T, q in ((4, 0), (8, 3), (12, 1), (180, 0), (180, 1)):
        slot_equals(hs_mod, rep, 1, c, (ax, ay), 2, T, q)
    for mask in (1, 4, 7):
        slot_equals(hs_mod, rep, 1, c, (ax, ay), mask, 12, 1)
    rep.close()


@gpu
def test_known_answers(hs_mod, ctx):
    w, h, Lw, T = 90, 31, 70, 180
    c = np.zeros((h, w), np.uint8); c[11, 5:5 + Lw] = 1
    rep = rep_of(hs_mod, ctx, c)
    _, HS, H = slot_equals(hs_mod, rep, 0, c, (0, 0), 2, T, 0)
    assert H[T // 2, 11 + w + h] == Lw and HS[T // 2] == Lw * Lw and int(np.argmax(HS)) == T // 2
    rep.close()
    for c in (np.full((37, 70), 2, np.uint8), np.ones((37, 70), np.uint8)):   # an empty map (every tile leaves at once), an all-sites map
        rep = rep_of(hs_mod, ctx, c)
        for q in A.QS:
            info, HS, H = slot_equals(hs_mod, rep, 0, c, (0, 0), 2, 12, q)
            assert info["n_sites"] == (0 if c[0, 0] == 2 else 37 * 70) and (H.sum(1, dtype=np.int64) == info["n_sites"]).all()
        rep.close()


# ---- 2. the world, a pyramid, a shifted and an updated window --------------------------------------------------------------------------
@gpu
def test_world_variant(hs_mod, ctx):
    level = 1
    rng = np.random.default_rng(7)
    rep = hs_mod.MapRepMultiMap(0.1, (80, 48), 2, ctx=ctx)
    rep.set_backing(16, POOL)
    TR.fill(hs_mod, rep, rng)
    rep.shift(34, -22)
    TR.fill(hs_mod, rep, rng)
    rep.shift(-68, 30)                                                     # part of what was mapped now lies in tiles alone: a ring round the window
    assert rep.origin() == (-34, 8) and rep.backing_stats()["tiles"] > 3
    ox, oy = rep.origin()
    info, _, _ = rep.hough(level, 0, True, 2, 12, 1)
    assert info["w"] > 40 and info["h"] > 24 and info["x0"] <= 0 and info["y0"] <= 0   # the world rectangle holds the window and its tiles
    cells = rep.world_cells(level, info["x0"] + (ox >> level), info["y0"] + (oy >> level), info["w"], info["h"])
    cls = D.np_class_bits(cells["value"])
    for mask, T, q in ((2, 12, 1), (3, 180, 0), (4, 8, 3)):
        slot_equals(hs_mod, rep, 0, cls, (info["x0"], info["y0"]), mask, T, q, level=level, world=True)
    _, HSw, _ = rep.hough(level, 0, True, 2, 12, 1)
    wcls = G.window_classes(rep, level)
    _, HS0, _ = slot_equals(hs_mod, rep, 0, wcls, (0, 0), 2, 12, 1, level=level)
    assert not np.array_equal(HS0, HSw)                                    # the tiles outside the window count in the world alone
    rep.close()


@gpu
def test_three_level_pyramid(hs_mod, ctx):
    rng = np.random.default_rng(11)
    rep = hs_mod.MapRepMultiMap(0.1, (136, 72), 3, ctx=ctx)
    TR.fill(hs_mod, rep, rng)
    for level in (0, 2):
        c = G.window_classes(rep, level)
        for mask, T, q in ((2, 180, 0), (6, 12, 1)):
            slot_equals(hs_mod, rep, 0, c, (0, 0), mask, T, q, level=level)
    rep.close()


@gpu
def test_after_a_shift_and_an_update(hs_mod, ctx):
    rng = np.random.default_rng(5)
    rep = hs_mod.MapRepMultiMap(0.1, (80, 48), 2, ctx=ctx)
    TR.fill(hs_mod, rep, rng)
    _, before, _ = slot_equals(hs_mod, rep, 0, G.window_classes(rep, 0), (0, 0), 2, 12, 0)
    rep.shift(6, -4)
    for level in (0, 1):
        _, after, _ = slot_equals(hs_mod, rep, 0, G.window_classes(rep, level), (0, 0), 2, 12, 0, level=level)
    _, after, _ = slot_equals(hs_mod, rep, 0, G.window_classes(rep, 0), (0, 0), 2, 12, 0)
    assert not np.array_equal(before, after)
    a = np.linspace(-math.pi, math.pi, 90, endpoint=False)
    scan = hs_mod.ScanCloud((1.5 * np.stack([np.cos(a), np.sin(a)], 1)).astype(np.float32))
    rep.UpdateByScan(scan, (4.0, 2.4, 0.3))
    _, updated, _ = slot_equals(hs_mod, rep, 0, G.window_classes(rep, 0), (0, 0), 2, 12, 0)
    assert not np.array_equal(updated, after)                              # the grid update changed the sites; the refilled slot follows
    rep.close()


# ---- 3. rotation scores and row correlations ----------------------------------------------------------------------------------------
def both_slots(hs_mod, ctx, d, s, T, q, ax=-40, ay=1000):
    rep = rep_of(hs_mod, ctx, d)
    rep.merge_set_source(0, ax, ay, cells_of(hs_mod, s))
    _, hs_d, Hd = slot_equals(hs_mod, rep, 0, d, (0, 0), 2, T, q)
    _, hs_s, Hs = slot_equals(hs_mod, rep, 1, s, (ax, ay), 2, T, q)
    return rep, hs_d, hs_s, Hd, Hs


def shifts_equal(rep, Hd, Hs, T, pairs):
    want = A.np_shifts(Hd, Hs, T, pairs)
    rec, xc = rep.hough_shifts(pairs, xc=True)
    assert xc.shape == (len(pairs), Hd.shape[1] + Hs.shape[1] - 1)
    for i, (wxc, wrec) in enumerate(want):
        assert A.rec_tuple(rec[i]) == wrec, (i, pairs[i].tolist(), A.rec_tuple(rec[i]), wrec)
        assert np.array_equal(xc[i], wxc), (i, pairs[i].tolist())
    rec2, none = rep.hough_shifts(pairs)                                   # the record without out_xc
    assert none is None and np.array_equal(rec2, rec)
    return rec


@gpu
@pytest.mark.parametrize("q", [0, 1])
def test_rotation_and_shifts(hs_mod, ctx, q):
    d, s, T, pairs = A.pairs_case()
    rep, hs_d, hs_s, Hd, Hs = both_slots(hs_mod, ctx, d, s, T, q)
    cc = rep.hough_rotation()
    assert cc.dtype == np.uint64 and np.array_equal(cc, A.np_rotation(hs_d, hs_s)[0]) and np.array_equal(cc, hs_mod.capi.debug_hough_rotation(hs_d, hs_s))
    rec = shifts_equal(rep, Hd, Hs, T, pairs)
    nd, ns = int(Hd[0].sum()), int(Hs[0].sum())
    assert all(int(r["sum"]) == nd * ns for r in rec)
    shifts_equal(rep, Hd, Hs, T, pairs[2:3])                               # P = 1
    rng = np.random.default_rng(3)
    many = np.stack([rng.integers(0, 2 * T, 256), rng.integers(0, T, 256)], 1).astype(np.int32)
    shifts_equal(rep, Hd, Hs, T, many)                                     # P = 256
    rep.close()


@gpu
def test_empty_rows(hs_mod, ctx):
    """An all-zero XC: -(N_s - 1), N_d + N_s - 1, 0 -- a source without a site, then a destination without one."""
    d = A.class_map(40, 30, 4); z = np.full((20, 25), 2, np.uint8)
    for dst, src in ((d, z), (np.full((30, 40), 2, np.uint8), A.class_map(25, 20, 4))):
        rep, _, _, Hd, Hs = both_slots(hs_mod, ctx, dst, src, 8, 1)
        rec = shifts_equal(rep, Hd, Hs, 8, np.array([[0, 0], [9, 3]], np.int32))
        assert [A.rec_tuple(r) for r in rec] == [(-(Hs.shape[1] - 1), Hd.shape[1] + Hs.shape[1] - 1, 0, 0)] * 2
        assert not rep.hough_rotation().any()
        rep.close()


@gpu
def test_large_level(hs_mod, ctx):
    """One 512 x 512 level with a few thousand sites at T = 180: many non-empty tiles per angle chunk, three chunks, and rows of
    2049 and 1401 bins -- 14 blocks of shifts per pair."""
    rng = np.random.default_rng(8)
    d = np.full((512, 512), 2, np.uint8)
    for _ in range(40):                                                    # wall pieces of both directions and a scatter
        x, y, n = rng.integers(0, 440), rng.integers(0, 512), rng.integers(20, 70)
        if rng.random() < 0.5:
            d[y, x:x + n] = 1
        else:
            d[x:x + n, y] = 1
    d[rng.random(d.shape) < 0.004] = 1
    assert 2000 < int((d == 1).sum()) < 6000
    s = d[100:400, 60:460].copy()
    T = 180
    rep, hs_d, hs_s, Hd, Hs = both_slots(hs_mod, ctx, d, s, T, 0)
    assert Hd.shape[1] == 2049 and Hs.shape[1] == 1401
    assert np.array_equal(rep.hough_rotation(), A.np_rotation(hs_d, hs_s)[0])
    rec = shifts_equal(rep, Hd, Hs, T, np.array([[0, 0], [0, 90], [180, 45], [359, 179], [7, 3]], np.int32))
    # the source is the destination's cells [60, 460) x [100, 400): rows 0 and T/2 peak at the shift that says so (D_d - D_s + offset)
    assert int(rec[0]["best_shift"]) == 60 + 1024 - 700 and int(rec[1]["best_shift"]) == 100 + 1024 - 700
    rep.close()


# ---- 4. the refusals -----------------------------------------------------------------------------------------------------------------
def refused(capi, call, code):
    with pytest.raises(capi.SlamhipError) as e:
        call()
    assert e.value.code == code, (e.value.code, code, str(e.value))


@gpu
def test_refusals_and_slot_state(hs_mod, ctx):
    capi = hs_mod.capi
    d = A.class_map(40, 30, 4); s = A.class_map(25, 20, 5)
    rep = hs_mod.MapRepMultiMap(0.1, (40, 30), 2, ctx=ctx)
    L.put_values(hs_mod, rep, 0, values_of(d).ravel())
    pairs = np.array([[0, 0]], np.int32)
    INV, STATE = capi.ERR_INVALID, capi.ERR_STATE
    # nothing filled: both slot-state errors
    refused(capi, lambda: capi.call("slamhip_hs_hough_rotation", rep._h, np.zeros(8, np.uint64).ctypes.data), STATE)
    refused(capi, lambda: capi.hough_shifts_call("slamhip_hs_hough_shifts", rep._h, pairs, None), STATE)
    refused(capi, lambda: rep.hough(0, 1, False, 2, 8, 0), STATE)          # slot 1 without a source
    for kw in (dict(level=2), dict(level=-1), dict(slot=2), dict(slot=-1), dict(world=2), dict(site_mask=0), dict(site_mask=8), dict(T=0), dict(T=6),
               dict(T=1028), dict(q=-1), dict(q=4)):
        a = dict(level=0, slot=0, world=0, site_mask=2, T=8, q=0); a.update(kw)
        refused(capi, lambda: rep.hough(a["level"], a["slot"], a["world"], a["site_mask"], a["T"], a["q"]), INV)
    rep.hough(0, 0, False, 2, 8, 0)
    refused(capi, lambda: rep.hough_rotation(), STATE)                     # slot 0 alone
    rep.merge_set_source(0, 3, -2, cells_of(hs_mod, s))
    refused(capi, lambda: rep.hough(0, 1, True, 2, 8, 0), INV)             # slot 1 has no world
    refused(capi, lambda: rep.hough(1, 1, False, 2, 8, 0), INV)            # ... and is of the source's level
    rep.hough(0, 1, False, 2, 12, 0)
    refused(capi, lambda: rep.hough_rotation(), STATE)                     # T differs
    refused(capi, lambda: rep.hough_shifts(pairs), STATE)
    rep.hough(0, 1, False, 2, 8, 1)
    refused(capi, lambda: rep.hough_rotation(), STATE)                     # q differs
    rep.hough(0, 1, False, 2, 8, 0)
    cc = rep.hough_rotation()
    rec, _ = rep.hough_shifts(pairs)
    for bad in ([[16, 0]], [[-1, 0]], [[0, 8]], [[0, -1]]):
        refused(capi, lambda: rep.hough_shifts(np.array(bad, np.int32)), INV)
    refused(capi, lambda: rep.hough_shifts(np.zeros((257, 2), np.int32)), INV)
    refused(capi, lambda: capi.call("slamhip_hs_hough_shifts", rep._h, pairs.ctypes.data, 0, np.zeros(1, capi.HOUGH_SHIFT).ctypes.data, None), INV)
    # a refused fill leaves the slots as they were
    refused(capi, lambda: rep.hough(0, 0, False, 9, 8, 0), INV)
    assert np.array_equal(rep.hough_rotation(), cc) and np.array_equal(rep.hough_shifts(pairs)[0], rec)
    # slot 1 emptied by set_source, clear_source and reset; reset empties slot 0 too
    rep.merge_set_source(0, 3, -2, cells_of(hs_mod, s))
    refused(capi, lambda: rep.hough_rotation(), STATE)
    rep.hough(0, 1, False, 2, 8, 0)
    assert np.array_equal(rep.hough_rotation(), cc)
    rep.merge_clear_source()
    refused(capi, lambda: rep.hough_shifts(pairs), STATE)
    refused(capi, lambda: rep.hough(0, 1, False, 2, 8, 0), STATE)
    rep.merge_set_source(0, 3, -2, cells_of(hs_mod, s))
    rep.hough(0, 1, False, 2, 8, 0)
    rep.Reset()
    refused(capi, lambda: rep.hough_rotation(), STATE)
    rep.merge_set_source(0, 3, -2, cells_of(hs_mod, s))
    rep.hough(0, 1, False, 2, 8, 0)
    refused(capi, lambda: rep.hough_rotation(), STATE)                     # slot 0 went with the reset
    rep.hough(0, 0, False, 2, 8, 0)
    assert not rep.hough_rotation().any()                                  # (the reset map has no site)
    rep.hough_clear()
    refused(capi, lambda: capi.call("slamhip_hs_hough_rotation", rep._h, np.zeros(8, np.uint64).ctypes.data), STATE)
    rep.hough_clear()                                                      # never fails for an hs without blocks
    rep.hough(0, 0, False, 2, 8, 0)                                        # ... and the unit comes back on the next call
    rep.close()
    # out_xc above 2^22 entries: N_d + N_s - 1 = 2 * 8193 - 1 at 2048 x 2048, q = 0; 256 pairs fit, 257 are refused as P
    big = hs_mod.MapRepMultiMap(0.1, (2048, 2048), 1, ctx=ctx)
    big.merge_set_source(0, 0, 0, cells_of(hs_mod, np.ones((2048, 2048), np.uint8)))
    big.hough(0, 0, False, 2, 4, 0); big.hough(0, 1, False, 2, 4, 0)
    refused(capi, lambda: big.hough_shifts(np.zeros((256, 2), np.int32), xc=True), INV)
    big.hough_shifts(np.zeros((256, 2), np.int32))
    big.close()


# ---- 5. AlignMaps --------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case,q", [(1, 1), (3, 0)])
def test_align_maps_equals_the_cpu_composition(hs_mod, ctx, case, q):
    capi = hs_mod.capi
    theta, t = A.CASES[case]
    dst, src, ax, ay, truth = A.synthetic_case(capi, theta, t)
    want = A.cpu_align(capi, dst, src, ax, ay, 360, q)
    proc = hs_mod.HectorSLAMProcessor(A.CELL, (A.W, A.H), (0.0, 0.0, 0.0), 1, ctx=ctx)
    proc.MapRep.Maps[0].SetCells(dst.ravel())
    proc.merge_set_source(0, ax, ay, src)
    got = proc.AlignMaps(0, T=360, q=q)
    assert [h["m"] for h in got] == [h["m"] for h in want]
    for g, w in zip(got, want):
        assert np.array_equal(g["pose"].view(np.uint32), w["pose"].view(np.uint32))
        assert [A.rec_tuple(r) for r in g["shifts"]] == [A.rec_tuple(r) for r in w["shifts"]]
        assert g["report"]["joint"].tolist() == w["report"]["joint"].tolist() and int(g["report"]["n_unsourced"]) == int(w["report"]["n_unsourced"])
    dth, dt = A.pose_errors(got[0]["pose"], truth)
    assert dth <= math.pi / 360 and dt <= (1 << q) + 2
    # through the processor's own calls: the same slots
    cc = proc.hough_rotation()
    assert np.array_equal(cc, proc.MapRep.hough_rotation())
    proc.Dispose()
