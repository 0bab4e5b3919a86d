"""CPU-side checks of the map merge's interface (slamhip_hs_merge_set_source / _score / _apply / _clear_source, the three
slamhip_hsproc_merge_* calls, slamhip_debug_merge, slamhip_debug_merge_box) and the restatement of its definition (include/slamhip.h,
slamhip_hs_merge_apply, steps 1 - 4) that tests/test_gpu_hector_merge.py compares the device with.

The restatement: np.float32 operations one by one, oracle/np_oracle's Matrix3x2 rotation (IEEERemainder, the snapped angles, the
deterministic sine and cosine), np.rint for the cells.  It shares no text with hs_merge.h, whose text the hook and the kernels run.
Every comparison is == on integers and on the bit patterns of the Values."""
import math
import os
import re

import np_oracle as npo
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
LIMIT = F(16777216.0)
QNAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]
SYMBOLS = ("slamhip_hs_merge_set_source", "slamhip_hs_merge_score", "slamhip_hs_merge_apply", "slamhip_hs_merge_clear_source",
           "slamhip_hsproc_merge_set_source", "slamhip_hsproc_merge_score", "slamhip_hsproc_merge_apply", "slamhip_debug_merge",
           "slamhip_debug_merge_box")
ADD, FILL, REPLACE = 0, 1, 2
THETAS = [F(0.3), F(math.pi / 4), F(-math.pi / 4), F(math.pi / 2), F(math.pi), F(-3.0)]
CELL = np.dtype([("update_index", np.int32), ("value", np.float32)])


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def np_xf(stm, pose):
    """Step 1 -> (txc, tyc, c, s) as float32."""
    tx, ty, th = (F(v) for v in np.asarray(pose, F).reshape(3))
    with np.errstate(over="ignore", invalid="ignore"):
        txc, tyc = tx * F(stm), ty * F(stm)
    if not np.isfinite(th):
        return txc, tyc, F(np.nan), F(np.nan)                              # (IEEERemainder of an infinity or a NaN is NaN, and so are its sine and cosine)
    r = npo.M32.rotation(th)
    return txc, tyc, r.m[0], r.m[1]


def np_source(dw, dh, sw, sh, ax, ay, pose, stm, x0=0, y0=0):
    """Step 2 for the destination cells [x0, x0 + dw) x [y0, y0 + dh) -> (sourced (dh, dw) bool, su, sv int64; 0 where not sourced)."""
    txc, tyc, c, s = np_xf(stm, pose)
    x = np.broadcast_to(np.arange(x0, x0 + dw).astype(F)[None, :], (dh, dw))
    y = np.broadcast_to(np.arange(y0, y0 + dh).astype(F)[:, None], (dh, dw))
    with np.errstate(over="ignore", invalid="ignore"):
        dxf = x - txc; dyf = y - tyc
        u = (c * dxf) + (s * dyf)
        v = (c * dyf) - (s * dxf)
        assert u.dtype == np.float32 and v.dtype == np.float32
        ok = (np.abs(u) < LIMIT) & (np.abs(v) < LIMIT)
        su = np.where(ok, np.rint(u), 0).astype(np.int64) - int(ax)
        sv = np.where(ok, np.rint(v), 0).astype(np.int64) - int(ay)
    sourced = ok & (su >= 0) & (su < sw) & (sv >= 0) & (sv < sh)
    return sourced, np.where(sourced, su, 0), np.where(sourced, sv, 0)


def np_class(v):
    with np.errstate(invalid="ignore"):
        return np.where(v > F(0.0), 1, np.where(v < F(0.0), 2, 0)).astype(np.int64)


def np_merge(dst, src, ax, ay, pose, stm, rule, limit):
    """Steps 1 - 4 -> (merged cells, report dict)."""
    dst = np.asarray(dst, CELL); src = np.asarray(src, CELL)
    dh, dw = dst.shape; sh, sw = src.shape
    limit = F(limit)
    sourced, su, sv = np_source(dw, dh, sw, sh, ax, ay, pose, stm)
    d = dst["value"].copy()
    s = src["value"][sv, su]
    cd, cs = np_class(d), np_class(s)
    joint = [int((sourced & (cd == a) & (cs == b)).sum()) for a in range(3) for b in range(3)]
    t = d.copy()
    clamped = np.zeros(d.shape, bool)
    with np.errstate(over="ignore", invalid="ignore"):
        if rule == ADD:
            m = sourced & (cs != 0) & ~np.isnan(d)
            a = d + s
            assert a.dtype == np.float32
            a = np.where(np.isnan(a), QNAN, a)
            hi = a > limit
            a = np.where(hi, limit, a)
            lo = a < -limit
            a = np.where(lo, -limit, a)
            t = np.where(m, a, d)
            clamped = m & (hi | lo)
        elif rule == FILL:
            t = np.where(sourced & (cd == 0) & (cs != 0), s, d)
        else:
            t = np.where(sourced & (cs != 0), s, d)
    changed = t.view(np.uint32) != d.view(np.uint32)
    out = dst.copy()
    out["value"] = np.where(changed, t, d)
    rep = dict(joint=joint, n_unsourced=int((~sourced).sum()), n_changed=int(changed.sum()), n_clamped=int(clamped.sum()))
    return out, rep


def rep_dict(r):
    return dict(joint=[int(v) for v in r["joint"]], n_unsourced=int(r["n_unsourced"]), n_changed=int(r["n_changed"]), n_clamped=int(r["n_clamped"]))


def same_cells(a, b):
    return (np.array_equal(a["update_index"], b["update_index"]) and np.array_equal(a["value"].view(np.uint32), b["value"].view(np.uint32)))


# ---- the maps ----------------------------------------------------------------------------------------------------------------------
TINY = F(1e-45)                                                            # the smallest subnormal
SPECIAL = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, TINY, -TINY, 1.5, -0.75, 2.25, -3.0, 0.4], F)


def cells_of(w, h, seed, special=True):
    """An (h, w) cell array: a spread of log-odds of both signs and zeros; with `special`, the special values salted in."""
    rng = np.random.default_rng([seed, w, h])
    c = np.zeros((h, w), CELL)
    v = rng.normal(0.0, 2.0, (h, w)).astype(F)
    v[rng.random((h, w)) < 0.3] = F(0.0)
    if special:
        k = rng.random((h, w)) < 0.35
        v[k] = SPECIAL[rng.integers(0, len(SPECIAL), int(k.sum()))]
    c["value"] = v
    c["update_index"] = rng.integers(-1, 50, (h, w)).astype(np.int32)
    return c


DESTS = [(8, 8), (33, 17)]
SOURCES = [(1, 1), (5, 3), (40, 40)]


def poses_for(stm):
    """The poses of the issue's list, in metres for ScaleToMap stm."""
    c = 1.0 / float(stm)
    P = [(0.0, 0.0, 0.0), (3 * c, 2 * c, 0.0), (-2 * c, 5 * c, 0.0),       # the identity; integer translations
         (0.5 * c, 0.0, 0.0), (1.5 * c, 2.5 * c, 0.0), (-0.5 * c, -1.5 * c, 0.0),   # dxf on k + 0.5, even and odd k
         (1000.0 * c, -1000.0 * c, 0.7)]                                   # the source wholly outside
    P += [(4 * c, 3 * c, float(t)) for t in THETAS] + [(0.3 * c, -0.2 * c, float(t)) for t in THETAS]
    for bad in (np.nan, np.inf, -np.inf):
        for k in range(3):
            p = [2 * c, 1 * c, 0.3]; p[k] = bad
            P.append(tuple(p))
    return P


@pytest.fixture(scope="module")
def capi():
    import slam.net_amd.build as b
    b.build()
    import slam.net_amd.capi as capi
    return capi


# ---- the surface -------------------------------------------------------------------------------------------------------------------
def test_surface(capi):
    L = capi.lib()
    header = open(os.path.join(ROOT, "include", "slamhip.h")).read()
    native = open(os.path.join(ROOT, "bindings", "csharp", "SlamHip", "SlamHip.Native.cs")).read()
    bare = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for n in SYMBOLS:
        assert hasattr(L, n) and n in L._signatures, n
        proto = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % n, bare, re.S)
        stub = re.search(r"static extern int %s\(([^;]*?)\);" % n, native, re.S)
        assert proto and stub, n
        n_c = len([a for a in proto.group(1).split(",") if a.strip()])
        assert n_c == len([a for a in stub.group(1).split(",") if a.strip()]) == len(L._signatures[n][1]), n
    assert [len(L._signatures[n][1]) for n in SYMBOLS] == [7, 4, 5, 1, 7, 4, 5, 14, 12]
    R = capi.MERGE_REPORT
    assert R.itemsize == 96 and list(R.names) == ["joint", "n_unsourced", "n_changed", "n_clamped"]
    assert [R.fields[f][1] for f in R.names] == [0, 72, 80, 88]
    m = re.search(r"typedef struct slamhip_merge_report \{(.*?)\} slamhip_merge_report;\s*/\*(.*?)\*/", header, re.S)
    body = re.sub(r"\[\d+\]", "", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert re.findall(r"(\w+)\s*[,;]", body) == list(R.names) and "96 bytes" in m.group(2) and "no padding" in m.group(2)
    assert "struct MergeReport" in native
    assert "SLAMHIP_K_COUNT = 10" in header                                 # no new timing class
    import slam.net_amd.build as b
    import slam.net_amd.hector as hm
    for n in ("merge_set_source", "merge_score", "merge_apply", "merge_clear_source"):
        assert hasattr(hm.MapRepMultiMap, n) and hasattr(hm.HectorSLAMProcessor, n), n
    assert "hs_merge.hip" in b.SOURCES and "hs_merge.h" in b.HEADERS
    shim = os.path.join(ROOT, "bindings", "csharp", "SlamHip", "HectorSLAM")
    used = set(re.findall(r"Native\.(slamhip_\w+)", open(os.path.join(shim, "MapRepMultiMap.Hip.cs")).read()
                          + open(os.path.join(shim, "HectorSLAMProcessor.Hip.cs")).read()))
    assert set(SYMBOLS) <= used


# ---- hook against restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stm", [1.0, 20.0])
@pytest.mark.parametrize("src_wh", SOURCES)
@pytest.mark.parametrize("dst_wh", DESTS)
def test_hook_equals_restatement(capi, dst_wh, src_wh, stm):
    dst = cells_of(dst_wh[0], dst_wh[1], 1)
    src = cells_of(src_wh[0], src_wh[1], 2)
    n_sourced = 0
    for ax, ay in ((0, 0), (-3, 2)):
        for pose in poses_for(stm):
            for rule in (ADD, FILL, REPLACE):
                got, grep = capi.debug_merge(dst, src, ax, ay, pose, stm, rule, 2.0)
                want, wrep = np_merge(dst, src, ax, ay, pose, stm, rule, 2.0)
                tag = (dst_wh, src_wh, ax, ay, pose, rule)
                assert same_cells(got, want), tag
                assert rep_dict(grep) == wrep, tag
                assert sum(wrep["joint"]) + wrep["n_unsourced"] == dst_wh[0] * dst_wh[1], tag
                if not np.isfinite(np.asarray(pose, F)).all() or abs(pose[0]) > 100:
                    assert wrep["n_unsourced"] == dst_wh[0] * dst_wh[1] and wrep["n_changed"] == 0, tag
                n_sourced += sum(wrep["joint"])
    assert n_sourced > 0


def test_integer_translation_is_an_array_shift(capi):
    """theta = 0 and a whole number of cells: destination cell (x, y) reads source-frame cell (x - 3, y - 2) -- written down as slices."""
    dw, dh, sw, sh, ax, ay = 33, 17, 40, 40, -1, 4
    dst = cells_of(dw, dh, 3, special=False)
    src = cells_of(sw, sh, 4, special=False)
    src["value"][src["value"] == 0] = F(0.5)                               # (every source cell has a class: REPLACE takes them all)
    got, rep = capi.debug_merge(dst, src, ax, ay, (3.0, 2.0, 0.0), 1.0, REPLACE, 1.0)
    want = dst.copy()
    # source array index (x - 3 - ax, y - 2 - ay) = (x - 2, y - 6): x in [2, 33), y in [6, 17)
    want["value"][6:17, 2:33] = src["value"][0:11, 0:31]
    assert same_cells(got, want)
    assert int(rep["n_unsourced"]) == dw * dh - 11 * 31 and int(rep["n_clamped"]) == 0


def test_half_cells_round_to_even(capi):
    """txc = 0.5 at theta = 0: dxf = x - 0.5 = k + 0.5 for k = x - 1, which rintf takes to the even neighbour."""
    src = np.zeros((1, 12), CELL)
    src["value"][0] = np.arange(1, 13, dtype=F)                            # source cell su holds su + 1
    dst = np.zeros((1, 8), CELL)
    got, _ = capi.debug_merge(dst, src, -2, 0, (0.5, 0.0, 0.0), 1.0, REPLACE, 1.0)
    rounded = [int(np.rint(F(x) - F(0.5))) for x in range(8)]
    assert rounded == [0, 0, 2, 2, 4, 4, 6, 6]                             # -0.5 -> -0, 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, ...
    assert got["value"][0].tolist() == [float(r + 2 + 1) for r in rounded]


def test_add_at_the_limit(capi):
    """ADD at limit - ulp, limit and limit + ulp on both signs, n_clamped counted; d = 1 everywhere, the source carries the rest."""
    limit = F(2.0)
    below, above = np.nextafter(limit, F(0.0)), np.nextafter(limit, F(4.0))
    for sign in (F(1.0), F(-1.0)):
        sums = [below, limit, above]
        dst = np.zeros((1, 3), CELL); dst["value"][0] = sign * F(1.0)
        src = np.zeros((1, 3), CELL); src["value"][0] = [sign * (t - F(1.0)) for t in sums]
        assert [F(1.0) + (t - F(1.0)) for t in sums] == sums               # (the sums are exact)
        got, rep = capi.debug_merge(dst, src, 0, 0, (0.0, 0.0, 0.0), 1.0, ADD, float(limit))
        want, wrep = np_merge(dst, src, 0, 0, (0.0, 0.0, 0.0), 1.0, ADD, float(limit))
        assert same_cells(got, want) and rep_dict(rep) == wrep
        assert got["value"][0].tolist() == [float(sign * below), float(sign * limit), float(sign * limit)]
        assert int(rep["n_clamped"]) == 1 and int(rep["n_changed"]) == 3
    # a cell already at the limit: the cut applies, no bit changes
    dst = np.zeros((1, 1), CELL); dst["value"][0, 0] = limit
    src = np.zeros((1, 1), CELL); src["value"][0, 0] = F(1.0)
    got, rep = capi.debug_merge(dst, src, 0, 0, (0.0, 0.0, 0.0), 1.0, ADD, float(limit))
    assert same_cells(got, dst) and int(rep["n_clamped"]) == 1 and int(rep["n_changed"]) == 0


def test_special_values_pairwise(capi):
    """Every special destination value against every special source value under the three rules; inf + -inf is the quiet NaN."""
    n = len(SPECIAL)
    dst = np.zeros((n, n), CELL); src = np.zeros((n, n), CELL)
    dst["value"] = SPECIAL[:, None]; src["value"] = SPECIAL[None, :]
    dst["update_index"] = 7
    for rule in (ADD, FILL, REPLACE):
        got, rep = capi.debug_merge(dst, src, 0, 0, (0.0, 0.0, 0.0), 1.0, rule, 2.0)
        want, wrep = np_merge(dst, src, 0, 0, (0.0, 0.0, 0.0), 1.0, rule, 2.0)
        assert same_cells(got, want) and rep_dict(rep) == wrep, rule
    got, _ = capi.debug_merge(dst, src, 0, 0, (0.0, 0.0, 0.0), 1.0, ADD, 2.0)
    i_pinf, i_ninf, i_nan = 3, 4, 2
    assert got["value"].view(np.uint32)[i_pinf, i_ninf] == 0x7FC00000 and got["value"].view(np.uint32)[i_ninf, i_pinf] == 0x7FC00000
    assert np.array_equal(got["value"].view(np.uint32)[i_nan], dst["value"].view(np.uint32)[i_nan])   # a NaN d stays
    assert np.array_equal(got["value"].view(np.uint32)[:, i_nan], dst["value"].view(np.uint32)[:, i_nan])   # a NaN source has no class


def test_replace_twice_changes_nothing(capi):
    dst = cells_of(33, 17, 5); src = cells_of(40, 40, 6)
    pose = (0.4, -0.1, 0.3)
    once, r1 = capi.debug_merge(dst, src, -4, -6, pose, 10.0, REPLACE, 1.0)
    twice, r2 = capi.debug_merge(once, src, -4, -6, pose, 10.0, REPLACE, 1.0)
    assert int(r1["n_changed"]) > 0 and int(r2["n_changed"]) == 0 and same_cells(once, twice)


def test_known_answer_doubling(capi):
    """Independent of the restatement: a map merged with its own download at the identity pose under ADD with a large limit has every
    Value doubled and every index unchanged."""
    m = cells_of(33, 17, 7, special=False)
    got, rep = capi.debug_merge(m, m, 0, 0, (0.0, 0.0, 0.0), 20.0, ADD, 1.0e30)
    assert np.array_equal(got["update_index"], m["update_index"])
    assert np.array_equal(got["value"].view(np.uint32), (m["value"] * F(2.0)).view(np.uint32))
    assert int(rep["n_unsourced"]) == 0 and int(rep["n_clamped"]) == 0 and int(rep["n_changed"]) == int((m["value"] != 0).sum())
    assert [int(v) for v in rep["joint"]][1:4] == [0, 0, 0] and int(rep["joint"][4]) == int((m["value"] > 0).sum())


def test_refusals_of_the_hook(capi):
    d = np.zeros((2, 2), CELL)
    for rule, limit in ((-1, 1.0), (3, 1.0), (0, 0.0), (0, -1.0), (1, float("nan")), (2, float("inf"))):
        with pytest.raises(capi.SlamhipError) as e:
            capi.debug_merge(d, d, 0, 0, (0, 0, 0), 1.0, rule, limit)
        assert e.value.code == capi.ERR_INVALID
    with pytest.raises(capi.SlamhipError):
        capi.debug_merge(d, d, 2 ** 30 + 1, 0, (0, 0, 0), 1.0, 0, 1.0)


# ---- the box -----------------------------------------------------------------------------------------------------------------------
def check_box(capi, pose, stm, ax, ay, sw, sh, x0, y0, tw, th):
    box = capi.debug_merge_box(pose, stm, ax, ay, sw, sh, x0, y0, x0 + tw - 1, y0 + th - 1)
    sourced, su, sv = np_source(tw, th, sw, sh, ax, ay, pose, stm, x0, y0)
    tag = (pose, stm, ax, ay, sw, sh, x0, y0, tw, th, box)
    if box is None:
        assert not sourced.any(), tag
        return 0
    u0, v0, u1, v1 = box
    assert 0 <= u0 <= u1 < sw and 0 <= v0 <= v1 < sh, tag
    assert ((su[sourced] >= u0) & (su[sourced] <= u1) & (sv[sourced] >= v0) & (sv[sourced] <= v1)).all(), tag
    return int(sourced.sum())


def test_box_holds_every_source_cell(capi):
    """20 000 sampled (pose, tile position, tile size) triples, and the listed angles and the poses that are not finite at every
    tile of a window: every cell of the tile has its source cell inside the box.  The box of the kernels' own tile stays within
    what their LDS block holds."""
    rng = np.random.default_rng(14)
    n = n_sourced = 0
    for _ in range(200):
        stm = float(rng.choice([1.0, 10.0, 20.0]))
        sw, sh = int(rng.integers(1, 300)), int(rng.integers(1, 300))
        ax, ay = int(rng.integers(-200, 50)), int(rng.integers(-200, 50))
        th = float(rng.uniform(-7.0, 7.0)) if rng.random() < 0.8 else float(rng.choice(THETAS))
        pose = (float(rng.uniform(-100, 300)) / stm, float(rng.uniform(-100, 300)) / stm, th)
        for _ in range(100):
            tw, tt = ((32, 32), (64, 32), (64, 16), (int(rng.integers(1, 65)), int(rng.integers(1, 33))))[int(rng.integers(0, 4))]
            x0, y0 = int(rng.integers(0, 400)), int(rng.integers(0, 400))
            n_sourced += check_box(capi, pose, stm, ax, ay, sw, sh, x0, y0, tw, tt)
            n += 1
    assert n == 20000 and n_sourced > 100000
    for t in [F(0.0)] + THETAS:
        for tx, ty in ((0.0, 0.0), (3.3, -1.7), (40.25, 12.5)):
            for tw, tt, cap in ((32, 32, 2560), (64, 32, 5120)):
                for y0 in range(0, 96, tt):
                    for x0 in range(0, 128, tw):
                        check_box(capi, (tx, ty, float(t)), 1.0, -10, -20, 200, 150, x0, y0, tw, tt)
                        box = capi.debug_merge_box((tx, ty, float(t)), 1.0, -1000, -1000, 3000, 3000, x0, y0, x0 + tw - 1, y0 + tt - 1)
                        assert box is not None and (box[2] - box[0] + 1) * (box[3] - box[1] + 1) <= cap, (t, tx, ty, tw, tt, box)
    for bad in (np.nan, np.inf, -np.inf):
        for k in range(3):
            p = [2.0, 1.0, 0.3]; p[k] = bad
            assert check_box(capi, tuple(p), 1.0, 0, 0, 40, 40, 0, 0, 32, 32) == 0
    # far out: |u| reaches 2^24 inside the tile's interval
    assert check_box(capi, (-16777000.0, 0.0, 0.0), 1.0, 16777000, 0, 300, 40, 200, 0, 64, 32) > 0
