"""K20 (slamhip_hs_render) on the CPU, no GPU: the host hook slamhip_debug_render -- the reference's own walk per line, from the header
text the kernels run -- against the C oracle's sequential Hector grid update with == on every cell of every level and on the indices,
over the cases of tests/render_cases.py and every case of tests/k5_cases.py that is a plain sequence of updates; the tile rule of
k20_render restated in NumPy (the clip interval of a line to a tile, the smallest crossing and ending line index per cell, the two
transitions) against the hook on the same cases; the clip interval against a literal walk; three wrong copies of the rule, each of
which must fail a named case; the hook's refusals.  (The refusals of slamhip_hs_render and slamhip_hs_scans_* need a context:
tests/test_gpu_hector_render.py.)"""
import numpy as np
import pytest

import k5_cases as kc
import render_cases as rc

F = np.float32
INF = 0x7fffffff


@pytest.fixture(scope="module")
def capi():
    import slam.net_amd.build as b
    b.build()
    import slam.net_amd.capi as capi
    return capi


@pytest.fixture(scope="module")
def det(oc):
    oc.set_trig_mode(oc.TRIG_DET)
    yield oc
    oc.set_trig_mode(oc.TRIG_LIBM)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_cells(got, ref, what):
    for field in ("update_index", "value"):
        g, r = bits(got[field]), bits(ref[field])
        bad = np.flatnonzero(g != r)
        assert bad.size == 0, (what, field, bad.size, bad[:8], got[field][bad[:8]], ref[field][bad[:8]])


def reset_cells(dims):
    out = []
    for w, h in dims:
        c = np.empty(w * h, kc.CELL)
        c["update_index"] = -1
        c["value"] = 0
        out.append(c)
    return out


def hook(capi, b, cells=None, ui=None, keep=False):
    dims = kc.level_dims(b.size, b.levels)
    return capi.debug_render(dims, b.cell_len, reset_cells(dims) if cells is None else cells, [0] * b.levels if ui is None else ui, [0] * b.levels,
                             [s[0] for s in b.steps], [s[1] for s in b.steps], [s[2] for s in b.steps], keep=keep, factors=b.factors or (0.4, 0.9))


def oracle(oc, b):
    """The C oracle's pyramid after the case's start (uploaded; the oracle follows an upload's index with empty scans, as
    tests/test_gpu_grid_update_edges.py does) and its scans -> (cells per level, update index per level)."""
    ref = oc.make_pyramid(b.cell_len, b.size[0], b.size[1], b.levels)
    try:
        cur = [0] * b.levels
        for l, g in enumerate(ref):
            if b.factors:
                g.set_factors(*b.factors)
            if b.start is not None:
                g.cells[:] = b.start[l]
                cur[l] = kc.index_after_upload(b.start[l], 0)
                for _ in range(cur[l] // 3):
                    g.update_by_scan(np.zeros((0, 2), np.float32), (0.0, 0.0, 0.0))
            for xy, origin, pose in b.steps:
                g.update_by_scan(xy, pose, origin=origin)
            cur[l] += 3 * len(b.steps)
        return [g.cells.copy() for g in ref], cur
    finally:
        for g in ref:
            g.close()



def test_hook_against_oracle_render_cases(capi, det):
    for name, fn in rc.CASES.items():
        b = fn()
        got, ui, ci = hook(capi, b)
        want, cur = oracle(det, b)
        for l in range(b.levels):
            same_cells(got[l], want[l], (name, l))
        assert ui == cur and ci == [len(b.steps)] * b.levels, name


def test_hook_against_oracle_k5_cases(capi, det):
    """Every case of k5_cases that is a plain sequence of updates: with a start state the hook runs as a KEEP render over the
    uploaded cells, from the index the upload leaves."""
    n = 0
    for c in kc.CASES:
        b = c.build()
        if not all(kc.is_scan(s) for s in b.steps):
            continue
        dims = kc.level_dims(b.size, b.levels)
        if b.start is None:
            got, ui, _ = hook(capi, b)
        else:
            got, ui, _ = hook(capi, b, [s.copy() for s in b.start], [kc.index_after_upload(b.start[l], 0) for l in range(b.levels)], keep=True)
        want, cur = oracle(det, b)
        for l in range(len(dims)):
            same_cells(got[l], want[l], (c.name, l))
        assert ui == cur, c.name
        n += 1
    assert n >= 20, n


# ---- the tile rule of k20_render, restated -----------------------------------------------------------------------------------
def clip(da, db, A0, A1, B0, B1):
    """hs_line_clip in Python integers."""
    lo, hi, e0 = max(A0, 0), min(A1, da), da // 2
    if B1 < 0 or B0 > db:
        return 1, 0
    if B0 > 0:
        lo = max(lo, -((-(B0 * da - e0)) // db))
    if B1 < db:
        hi = min(hi, ((B1 + 1) * da - e0 - 1) // db)
    return lo, hi


def logodds(capi, factors):
    """lo_free and lo_occ as the library forms them (libm's logf on the host), read off a three-cell map after one line."""
    out, _, _ = capi.debug_render([(3, 1)], 1.0, reset_cells([(3, 1)]), [0], [0], [np.array([[2.0, 0.0]], np.float32)], [(0.0, 0.0)], [(0.0, 0.0, 0.0)],
                                  factors=factors)
    return out[0]["value"][0], out[0]["value"][2]


def tile_rule(capi, b, T, variant=None):
    """All levels by tiles of T x T: per tile the scans in order (variant "reverse": in reverse order); per scan the smallest index of
    a line that crosses each cell and of one that ends in it, from the clip interval of every line; then the two transitions
    (variant "end_is_free": the end cell counts as a free step of its line too; "fixed_order": free, then occupied, whatever touched
    the cell first)."""
    lo_free, lo_occ = logodds(capi, b.factors or (0.4, 0.9))
    geo = kc.geometry(b)
    dims = kc.level_dims(b.size, b.levels)
    out = reset_cells(dims)
    order = list(range(len(b.steps)))
    if variant == "reverse":
        order.reverse()
    for l, (w, h) in enumerate(dims):
        val = out[l]["value"].reshape(h, w)
        idx = out[l]["update_index"].reshape(h, w)
        for ty in range(0, h, T):
            for tx in range(0, w, T):
                x1, y1 = min(tx + T, w) - 1, min(ty + T, h) - 1
                for pos, k in enumerate(order):
                    g = geo[k][l]
                    ff, fo = {}, {}
                    for i in np.flatnonzero(g.valid):
                        da, sdb, mx, smaj = int(g.da[i]), int(g.sdb[i]), bool(g.major_x[i]), int(g.smaj[i])
                        db, smin = abs(sdb), (-1 if sdb < 0 else 1)
                        bM, bm = (g.bx, g.by) if mx else (g.by, g.bx)
                        tM0, tM1, tm0, tm1 = (tx, x1, ty, y1) if mx else (ty, y1, tx, x1)
                        A0, A1 = (tM0 - bM, tM1 - bM) if smaj > 0 else (bM - tM1, bM - tM0)
                        B0, B1 = (tm0 - bm, tm1 - bm) if smin > 0 else (bm - tm1, bm - tm0)
                        i0, i1 = clip(da, db, A0, A1, B0, B1)
                        for s in range(i0, i1 + 1):
                            m = (da // 2 + s * db) // da
                            cM, cm = bM + smaj * s, bm + smin * m
                            c = (cM, cm) if mx else (cm, cM)
                            assert tx <= c[0] <= x1 and ty <= c[1] <= y1
                            if s == da:
                                fo[c] = min(fo.get(c, INF), int(i))
                                if variant == "end_is_free":
                                    ff[c] = min(ff.get(c, INF), int(i))
                            else:
                                ff[c] = min(ff.get(c, INF), int(i))
                    mark_free, mark_occ = 3 * pos + 1, 3 * pos + 2
                    for c in set(ff) | set(fo):
                        f0, o0 = ff.get(c, INF), fo.get(c, INF)
                        v, u = val[c[1], c[0]], int(idx[c[1], c[0]])
                        free_first = f0 != INF if variant == "fixed_order" else (f0 <= o0 if variant == "end_is_free" else f0 < o0)
                        if free_first and f0 != INF and u < mark_free:
                            v = F(v + lo_free); u = mark_free
                        if o0 != INF and u < mark_occ:
                            if u == mark_free:
                                v = F(v - lo_free)
                            if v < F(50.0):
                                v = F(v + lo_occ)
                            u = mark_occ
                        val[c[1], c[0]] = v; idx[c[1], c[0]] = u
    return out


@pytest.mark.parametrize("T", rc.TILES)
def test_tile_rule_against_hook(capi, T):
    """The same cases as the hook runs, every one of them, for both tile sides."""
    for name in rc.CASES:
        b = rc.CASES[name]()
        got, _, _ = hook(capi, b)
        want = tile_rule(capi, b, T)
        for l in range(b.levels):
            same_cells(want[l], got[l], (name, T, l))


@pytest.mark.parametrize("variant,name", [("reverse", "across_mid_end_cross"), ("reverse", "clamp"), ("end_is_free", "within_mid_end_cross"),
                                          ("fixed_order", "within_mid_end_cross"), ("fixed_order", "within_border_end_cross")])
def test_wrong_copies_fail(capi, variant, name):
    """The cases tell the rule from its wrong copies: scans applied in reverse order; the end cell counted as a free step; a fixed
    free-then-occupied order within a scan."""
    b = rc.CASES[name]()
    got, _, _ = hook(capi, b)
    wrong = tile_rule(capi, b, 32, variant)
    differs = any((bits(wrong[l]["value"]) != bits(got[l]["value"])).any() or (wrong[l]["update_index"] != got[l]["update_index"]).any() for l in range(b.levels))
    assert differs, (variant, name)
    right = tile_rule(capi, b, 32)
    for l in range(b.levels):
        same_cells(right[l], got[l], (name, l))


def test_clamp_case_passes_50(capi):
    b = rc.CASES["clamp"]()
    got, _, _ = hook(capi, b)
    assert got[0]["value"].reshape(64, 64)[33, 40] >= 50.0


# ---- the clip interval against a literal walk -----------------------------------------------------------------------------------
def walk_minor(da, db):
    """The minor offset at steps 0 .. da by Bresenham2D's own loop (OccGridMap.cs:220-239)."""
    out = np.empty(da + 1, np.int64)
    err, m = da // 2, 0
    for i in range(da + 1):
        out[i] = m
        err += db
        if err >= da:
            m += 1; err -= da
    return out


def expect_clip(mo, da, a0, b0, T):
    lo = np.maximum(a0, 0); hi = np.minimum(a0 + T - 1, da)
    lo = np.maximum(lo, np.searchsorted(mo, b0, "left")); hi = np.minimum(hi, np.searchsorted(mo, b0 + T - 1, "right") - 1)
    return lo, hi


def check_clip(capi, da, db, T, a0, b0):
    mo = walk_minor(da, db)
    assert mo[da] == db
    i0, i1 = capi.debug_render_clip(da, db, T, a0, b0)
    lo, hi = expect_clip(mo, da, a0.astype(np.int64), b0.astype(np.int64), T)
    empty = lo > hi
    assert ((i0 > i1) == empty).all(), (da, db, T)
    assert (i0[~empty] == lo[~empty]).all() and (i1[~empty] == hi[~empty]).all(), (da, db, T)
    for k in (0, a0.size // 2, a0.size - 1):                      # ... and the Python restatement the tile rule above goes by
        assert (clip(da, db, int(a0[k]), int(a0[k]) + T - 1, int(b0[k]), int(b0[k]) + T - 1)[0] > clip(da, db, int(a0[k]), int(a0[k]) + T - 1, int(b0[k]), int(b0[k]) + T - 1)[1]) == bool(empty[k])


@pytest.mark.parametrize("T", rc.TILES)
def test_clip_interval_small_lines(capi, T):
    """Every (da, db) with db <= da <= 96 and every window offset that can meet the line, and a ring beyond."""
    for da in range(1, 97):
        for db in range(0, da + 1):
            a, bb = np.meshgrid(np.arange(-T, da + 2, dtype=np.int32), np.arange(-T, db + 2, dtype=np.int32), indexing="ij")
            check_clip(capi, da, db, T, a.ravel(), bb.ravel())


@pytest.mark.parametrize("T", rc.TILES)
@pytest.mark.parametrize("da", (2047, 8191, 32767))
def test_clip_interval_long_lines(capi, T, da):
    """db in {0, 1, da - 1, da}, the first, a middle and the last tile along the line, every alignment of the tile grid."""
    for db in (0, 1, da - 1, da):
        mo = walk_minor(da, db)
        a_list, b_list = [], []
        for i in (0, da // 2, da):
            for oa in range(T):
                for ob in (0, 1, T // 2, T - 1):
                    a_list.append(i - oa); b_list.append(int(mo[i]) - ob)
        check_clip(capi, da, db, T, np.array(a_list, np.int32), np.array(b_list, np.int32))


def test_hook_refusals(capi):
    dims = [(16, 16)]
    cells = reset_cells(dims)
    scan = [np.array([[3.0, 1.0]], np.float32)]

    def refused(**kw):
        a = dict(dims=dims, cell_length=1.0, cells=cells, update_index=[0], cache_index=[0], scans=scan, origins=[(0.0, 0.0)], poses=[(4.0, 4.0, 0.0)])
        a.update(kw)
        with pytest.raises(capi.SlamhipError) as e:
            capi.debug_render(**a)
        assert e.value.code == capi.ERR_INVALID
    for bad in (np.nan, np.inf, -np.inf):
        for k in range(3):
            p = [4.0, 4.0, 0.0]
            p[k] = bad
            refused(poses=[tuple(p)])
    refused(update_index=[2 ** 31 - 3], keep=True)                # + 3 passes INT_MAX
    capi.debug_render(dims, 1.0, cells, [2 ** 31 - 4], [0], scan, [(0.0, 0.0)], [(4.0, 4.0, 0.0)], keep=True)      # ... and this does not
    capi.debug_render(dims, 1.0, cells, [2 ** 31 - 3], [0], scan, [(0.0, 0.0)], [(4.0, 4.0, 0.0)])                 # without KEEP the index starts at 0
    refused(flags=2)
    refused(dims=[(0, 16)], cells=[np.zeros(0, kc.CELL)])
    with pytest.raises(capi.SlamhipError):
        capi.debug_render_clip(0, 0, 32, [0], [0])
    with pytest.raises(capi.SlamhipError):
        capi.debug_render_clip(8, 9, 32, [0], [0])


def test_hook_keep_and_empty(capi):
    """Without KEEP and without scans the hook clears; with KEEP and without scans it changes nothing; a scan of 0 points advances
    the indices by 3 and 1."""
    dims = [(8, 8)]
    c = reset_cells(dims)
    c[0]["value"][5] = 1.5; c[0]["update_index"][5] = 4
    out, ui, ci = capi.debug_render(dims, 1.0, c, [6], [2], [], [], [], keep=True)
    same_cells(out[0], c[0], "keep")
    assert (ui, ci) == ([6], [2])
    out, ui, ci = capi.debug_render(dims, 1.0, c, [6], [2], [], [], [])
    same_cells(out[0], reset_cells(dims)[0], "clear")
    assert (ui, ci) == ([0], [0])
    out, ui, ci = capi.debug_render(dims, 1.0, c, [6], [2], [np.zeros((0, 2), np.float32)], [(0.0, 0.0)], [(1.0, 1.0, 0.0)], keep=True)
    same_cells(out[0], c[0], "empty scan")
    assert (ui, ci) == ([9], [3])



def test_lap_ordering_on_the_cpu(capi):
    """The end-to-end lap of tests/test_gpu_hector_render.py with the hooks alone: renders at the true, the drifted and the relaxed
    poses (slamhip_debug_pg_relax over the graph RelaxKeyframes forms); the level-0 set of cells with value > 0 of the relaxed
    render differs from the true render's in fewer cells than the drifted render's does.  An ordering, not a threshold.  The counts
    (DESIGN.md section 4 "K20"): 1704 cells occupied at the true poses; 6006 differ for the drifted poses, 77 for the relaxed ones."""
    L = rc.lap()
    N = len(L["scans"])
    p0, ij, z, w = rc.lap_graph(capi, L["drifted"], L["loop"])
    relaxed = capi.debug_pg_relax(p0, None, ij, z, w, capi.pg_spec(5, 4 * N, tol=1e-8))[0].astype(np.float32)
    r_true, r_drift, r_relax = (rc.lap_hook_render(capi, L, p)[0] for p in (L["true"], L["drifted"], relaxed))
    d_drift, d_relax = rc.sym_diff(r_drift, r_true), rc.sym_diff(r_relax, r_true)
    print("occupied at the true poses %d; symmetric difference: drifted %d, relaxed %d" % (int((r_true["value"] > 0).sum()), d_drift, d_relax))
    assert d_relax < d_drift
