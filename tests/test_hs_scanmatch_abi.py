"""CPU-side checks of K21, stored scans matched pairwise (slamhip_hs_scans_match, slamhip_hs_scans_edges, slamhip_debug_scans_match;
include/slamhip.h): the host hook -- the header text the kernel runs, in plain loops -- against an elementwise NumPy restatement of
rules 1 - 5 on every case of tests/scanmatch_cases.py, rule 6 against a binary64 restatement, the layouts, every refusal, wrong copies
of the rule that must each fail a named case, and the end-to-end lap with the hooks alone.  Everything is compared with == on
integers and on bit patterns.  No compute calls on a device."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import np_oracle as npo
import render_cases as rc
import scanmatch_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SYMBOLS = ("slamhip_hs_scans_match", "slamhip_hs_scans_edges", "slamhip_debug_scans_match", "slamhip_hsproc_scans_match")
SUMS = ("sum_x", "sum_y", "sum_k", "sum_xx", "sum_yy", "sum_kk", "sum_xy", "sum_xk", "sum_yk")


@pytest.fixture(scope="module")
def capi():
    import slam.net_amd.build as b
    b.build()
    import slam.net_amd.capi as capi
    return capi


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def np_floor(f, variant):
    return (np.trunc(f) if variant == "trunc" else np.floor(f)).astype(np.int64)


def np_raster(ref_xy, scale, H, variant=None):
    """Rule 1 -> (val (2H, 2H) int64 indexed [y, x], n_ref)."""
    xy = np.asarray(ref_xy, np.float32).reshape(-1, 2)
    with np.errstate(invalid="ignore", over="ignore"):
        fx = xy[:, 0] * F(scale); fy = xy[:, 1] * F(scale)
        assert fx.dtype == np.float32
        ok = (np.abs(fx) < F(16384.0)) & (np.abs(fy) < F(16384.0))
    cx = np_floor(fx[ok], variant) + H; cy = np_floor(fy[ok], variant) + H
    inside = (cx >= 0) & (cx < 2 * H) & (cy >= 0) & (cy < 2 * H)
    hit = np.zeros((2 * H, 2 * H), bool)
    hit[cy[inside], cx[inside]] = True
    near = np.zeros_like(hit)
    if variant == "wrap":                                                  # the dilation NOT clipped at the grid's edge: the flat array's neighbours
        flat = hit.reshape(-1)
        for d in (-2 * H - 1, -2 * H, -2 * H + 1, -1, 0, 1, 2 * H - 1, 2 * H, 2 * H + 1):
            near |= np.roll(flat, d).reshape(hit.shape)
    else:
        pad = np.zeros((2 * H + 2, 2 * H + 2), bool)
        pad[1:-1, 1:-1] = hit
        for dy in (0, 1, 2):
            for dx in (0, 1, 2):
                near |= pad[dy:dy + 2 * H, dx:dx + 2 * H]
    val = np.where(hit, 1 if variant == "hit1" else 2, np.where(near, 1, 0)).astype(np.int64)
    return val, int(ok.sum())


def np_theta(guess, k, dtheta):
    return F(F(guess[2]) + F(F(k) * F(dtheta)))


def np_query_cells(scale, H, guess, theta, xy, variant=None):
    """Rule 2 -> (gx, gy) int64 of the points used."""
    scale = F(scale); xy = np.asarray(xy, np.float32).reshape(-1, 2)
    s, c = npo.det_sincos(F(theta))
    s, c = F(s), F(c)
    cxm, cym = F(F(guess[0]) * scale), F(F(guess[1]) * scale)
    px, py = xy[:, 0], xy[:, 1]
    with np.errstate(invalid="ignore", over="ignore"):
        rx = (c * px) - (s * py)
        ry = (s * px) + (c * py)
        fx = (rx * scale) + cxm
        fy = (ry * scale) + cym
        assert fx.dtype == np.float32 and fy.dtype == np.float32
        valid = (np.abs(fx) < F(16777216.0)) & (np.abs(fy) < F(16777216.0))
    return np_floor(fx[valid], variant) + H, np_floor(fy[valid], variant) + H


def np_match(scans, sp, pair, variant=None):
    """Rules 1 - 5 for one pair -> a dict with the fields of slamhip_scanmatch_result."""
    ref, query, guess = pair
    if variant == "swap":
        ref, query = query, ref
    H, nx, ny, nt = sp["half"], sp["nx"], sp["ny"], sp["nt"]
    val, n_ref = np_raster(scans[ref], sp["scale"], H, variant)
    ixs = np.arange(-nx, nx + 1, dtype=np.int64)
    vol = np.zeros((2 * nt + 1, 2 * ny + 1, 2 * nx + 1), np.int64)
    used = []
    for k in range(-nt, nt + 1):
        gx, gy = np_query_cells(sp["scale"], H, guess, np_theta(guess, k, sp["dtheta"]), scans[query], variant)
        used.append(gx.shape[0])
        X = gx[None, :] + ixs[:, None]
        okx = (X >= 0) & (X < 2 * H)
        Xc = np.clip(X, 0, 2 * H - 1)
        for iy in range(-ny, ny + 1):
            Y = gy + iy
            ok = okx & ((Y >= 0) & (Y < 2 * H))[None, :]
            vol[k + nt, iy + ny] = np.where(ok, val[np.clip(Y, 0, 2 * H - 1)[None, :], Xc], 0).sum(axis=1)
    flat = np.arange(vol.size, dtype=np.uint64).reshape(vol.shape)
    keys = ((vol.astype(np.uint64) ^ np.uint64(0x80000000)) << np.uint64(32)) | (flat if variant == "tie_high" else np.uint64(0xFFFFFFFF) - flat)
    best = int(keys.max())
    b = (best >> 32) ^ 0x80000000
    bflat = (best & 0xFFFFFFFF) if variant == "tie_high" else 0xFFFFFFFF - (best & 0xFFFFFFFF)
    NX, NY = 2 * nx + 1, 2 * ny + 1
    out = dict(k=bflat // (NX * NY) - nt, iy=(bflat // NX) % NY - ny, ix=bflat % NX - nx, score=b, n_ref=n_ref, reserved=0)
    out["n_query"] = used[out["k"] + nt]
    inN = vol >= b - sp["margin"]
    if variant != "no_positive":
        inN &= vol > 0
    K, IY, IX = np.meshgrid(np.arange(-nt, nt + 1), np.arange(-ny, ny + 1), np.arange(-nx, nx + 1), indexing="ij")
    k_, y_, x_ = K[inN].astype(object), IY[inN].astype(object), IX[inN].astype(object)   # (Python integers: no width to overflow)
    out["cnt"] = int(inN.sum())
    for name, v in zip(SUMS, (x_, y_, k_, x_ * x_, y_ * y_, k_ * k_, x_ * y_, x_ * k_, y_ * k_)):
        out[name] = int(v.sum()) if out["cnt"] else 0
    return out


def same(got, want, what):
    for name in got.dtype.names:
        assert int(got[name]) == int(want[name]), (what, name, int(got[name]), int(want[name]))


def run_hook(capi, case):
    return capi.debug_scans_match(case["scans"], capi.scanmatch_spec(**case["spec"]), case["pairs"])


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_hook_against_restatement(capi, name):
    case = sc.CASES[name]()
    got = run_hook(capi, case)
    for i, pair in enumerate(case["pairs"]):
        want = np_match(case["scans"], case["spec"], pair)
        for f in got.dtype.names:
            assert int(got[i][f]) == want[f], (name, i, f, int(got[i][f]), want[f])
        assert int(got[i]["score"]) <= 2 * int(got[i]["n_query"])


def test_cases_do_what_they_say(capi):
    """What the case builders promise, by construction and from the hook's own output."""
    got = run_hook(capi, sc.CASES["empty_query_and_reference"]())
    for r in got:
        assert (int(r["score"]), int(r["cnt"]), int(r["k"]), int(r["iy"]), int(r["ix"])) == (0, 0, -1, -2, -1)      # invalid, best flat 0
        assert all(int(r[s]) == 0 for s in SUMS)
    assert [int(r["n_ref"]) for r in got] == [20, 0, 0] and [int(r["n_query"]) for r in got] == [0, 20, 0]
    r = run_hook(capi, sc.CASES["all_nodes_tie"]())[0]
    assert (int(r["score"]), int(r["k"]), int(r["iy"]), int(r["ix"]), int(r["cnt"])) == (2, -2, -2, -2, 5 * 25)
    r = run_hook(capi, sc.CASES["tie_across_heading_blocks"]())[0]
    assert (int(r["k"]), int(r["iy"]), int(r["ix"]), int(r["cnt"])) == (-2, 0, 0, 5) and int(r["score"]) == 2 * int(r["n_query"])
    r = run_hook(capi, sc.CASES["reference_edges_H16"]())[0]
    assert int(r["n_ref"]) == 16 + 8 + 6 + 2                                # the grid's, the six beside it, the two below 2^14; two at 2^14 and two NaN ignored
    c = sc.CASES["margin_everything"]()
    r = run_hook(capi, c)[0]
    assert int(r["sum_xx"]) > 2 ** 24 and int(r["cnt"]) > 10000             # sums of tens of thousands of nodes, past what a binary32 holds exactly
    assert int(run_hook(capi, sc.CASES["margin_zero"]())[0]["cnt"]) < int(r["cnt"])
    for name, n in (("query_1023", sc.CHUNK - 1), ("query_1024", sc.CHUNK), ("query_1025", sc.CHUNK + 1), ("scans_2049", 2 * sc.CHUNK + 1)):
        assert sc.CASES[name]()["scans"][1].shape[0] == n
    for name, nt in (("tile_255", 255), ("tile_259", 259), ("tile_511", 511), ("tile_513", 513)):
        s = sc.CASES[name]()["spec"]
        assert (2 * s["nx"] + 1) * (2 * s["ny"] + 1) == nt and abs(nt - round(nt / sc.TILE) * sc.TILE) <= 3
    assert len(sc.CASES["pairs_65_one_reference"]()["pairs"]) == 65


WRONG = [("wrap", "reference_edges_H16"), ("hit1", "self_pair"), ("tie_high", "all_nodes_tie"), ("no_positive", "empty_query_and_reference"),
         ("trunc", "cell_borders"), ("swap", "one_one")]


@pytest.mark.parametrize("variant,name", WRONG)
def test_wrong_copies_fail(capi, variant, name):
    """Each wrong copy of the rule -- the dilation not clipped at the grid's edge, val = 1 for hit cells, ties to the highest flat,
    score >= b - margin without score > 0, truncation instead of floor, the ref / query roles swapped -- differs from the hook on
    its named case (on which the right copy agrees: test_hook_against_restatement)."""
    case = sc.CASES[name]()
    got = run_hook(capi, case)
    differs = False
    for i, pair in enumerate(case["pairs"]):
        want = np_match(case["scans"], case["spec"], pair, variant)
        differs |= any(int(got[i][f]) != want[f] for f in got.dtype.names)
    assert differs, (variant, name)


# ---- rule 6 ------------------------------------------------------------------------------------------------------------------------
def np_edge(sp, pair, r):
    D = np.float64
    scale = F(sp["scale"]); g = [F(v) for v in pair[2]]
    cxm, cym = F(g[0] * scale), F(g[1] * scale)
    z = [(D(cxm) + D(int(r["ix"]))) / D(scale), (D(cym) + D(int(r["iy"]))) / D(scale), D(np_theta(g, int(r["k"]), sp["dtheta"]))]
    cnt = int(r["cnt"])
    if cnt <= 0:
        return z, [D(0.0)] * 3, False
    u = D(1.0) / D(scale)
    ut = D(6.283185307179586) / D(64.0) if sp["nt"] == 0 or F(sp["dtheta"]) == 0 else abs(D(F(sp["dtheta"])))
    w = []
    for s1, s2, uu in ((r["sum_x"], r["sum_xx"], u), (r["sum_y"], r["sum_yy"], u), (r["sum_k"], r["sum_kk"], ut)):
        m = D(int(s1)) / D(cnt)
        v = D(int(s2)) / D(cnt) - m * m
        v = v if v > 0 else D(0.0)
        u2 = uu * uu
        w.append(D(1.0) / ((v * u2) + (u2 / D(12.0))))
    return z, w, True


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_edge_rule_against_restatement(capi, name):
    case = sc.CASES[name]()
    sp = capi.scanmatch_spec(**case["spec"])
    res = run_hook(capi, case)
    z, w, valid = capi.scans_edges(sp, case["pairs"], res)
    for i, pair in enumerate(case["pairs"]):
        wz, ww, wv = np_edge(case["spec"], pair, res[i])
        assert bool(valid[i]) == wv == (int(res[i]["cnt"]) > 0)
        assert [float(v).hex() for v in z[i]] == [float(v).hex() for v in wz], (name, i)
        assert [float(v).hex() for v in w[i]] == [float(v).hex() for v in ww], (name, i)
        if wv:
            assert all(math.isfinite(v) and v > 0 for v in w[i])


def test_edge_rule_weights_finite_at_the_extremes(capi):
    """scale and dtheta at the ends of binary32, nt = 0 and dtheta = 0: every weight of a valid result is finite and > 0."""
    r = np.zeros(1, capi.SCANMATCH_RESULT)
    r["cnt"] = 2; r["sum_x"] = 64; r["sum_xx"] = 64 * 64; r["sum_k"] = 0; r["sum_kk"] = 2 * 8 * 8
    for scale in (1e-45, 1e-38, 1.0, 3.4e38):
        for nt, dth in ((0, 0.5), (8, 0.0), (8, 1e-45), (8, -1e-38), (8, 3.4e38)):
            sp = capi.scanmatch_spec(scale, 16, 64, 64, min(nt, 8), dth)
            r["k"] = 0
            z, w, valid = capi.scans_edges(sp, [(0, 0, (0.0, 0.0, 0.0))], r)
            assert valid[0] and all(math.isfinite(v) and v > 0 for v in w[0]), (scale, nt, dth, w)


# ---- layouts, symbols, refusals ----------------------------------------------------------------------------------------------------
def test_layouts_and_symbols(capi):
    L = capi.lib()
    for s in SYMBOLS:
        assert hasattr(L, s) and s in capi.declared_symbols(), s
    assert [capi.SCANMATCH_SPEC.fields[n][1] for n in ("scale", "half", "nx", "ny", "nt", "dtheta", "margin", "reserved")] == [0, 4, 8, 12, 16, 20, 24, 28]
    assert capi.SCANMATCH_SPEC.itemsize == 32
    assert [capi.SCAN_PAIR.fields[n][1] for n in ("ref", "query", "guess")] == [0, 4, 8] and capi.SCAN_PAIR.itemsize == 20
    R = capi.SCANMATCH_RESULT
    assert [R.fields[n][1] for n in ("k", "ix", "iy", "score", "n_ref", "n_query", "cnt", "reserved")] == [0, 4, 8, 12, 16, 20, 24, 28]
    assert [R.fields[n][1] for n in SUMS] == [32, 40, 48, 56, 64, 72, 80, 88, 96] and R.itemsize == 104
    h = open(os.path.join(ROOT, "include", "slamhip.h")).read()
    for text in ("slamhip_scanmatch_spec;              /* 32 bytes */", "slamhip_scan_pair;                   /* 20 bytes */",
                 "slamhip_scanmatch_result;            /* 104 bytes */", "offsets 80, 88, 96"):
        assert text in h, text
    import slam.net_amd.build as b
    assert "hs_scanmatch.hip" in b.SOURCES and "hs_scanmatch.h" in b.HEADERS and "hs_scans.h" in b.HEADERS


def raw_hook(capi, scans, sp, pairs, n_pairs=None, N=None):
    """The hook through ctypes alone -> (status, the out array it was given, filled with 0x55 beforehand)."""
    pts = [capi.f32(s, (-1, 2)) for s in scans]
    off = np.zeros(len(pts) + 1, np.int32)
    off[1:] = np.cumsum([p.shape[0] for p in pts])
    xy = np.ascontiguousarray(np.concatenate(pts, axis=0)) if pts and off[-1] else np.zeros((1, 2), np.float32)
    pr = capi.scan_pairs(pairs) if len(pairs) else np.zeros(1, capi.SCAN_PAIR)
    n = len(pairs) if n_pairs is None else n_pairs
    out = np.full(max(len(pairs), 1) * capi.SCANMATCH_RESULT.itemsize, 0x55, np.uint8)
    rc_ = capi.lib().slamhip_debug_scans_match(xy.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p), len(pts) if N is None else N,
                                               sp.ctypes.data_as(C.c_void_p), pr.ctypes.data_as(C.c_void_p), n, out.ctypes.data_as(C.c_void_p))
    return rc_, out


def test_refusals_write_nothing(capi):
    scans = [sc.walls(10, 1, 4), sc.walls(10, 2, 4)]
    good = dict(scale=1.0, half=16, nx=1, ny=1, nt=1, dtheta=0.1, margin=0)
    pairs = [(0, 1, (0.0, 0.0, 0.0))]
    assert raw_hook(capi, scans, capi.scanmatch_spec(**good), pairs)[0] == 0
    bad_specs = [dict(scale=0.0), dict(scale=-1.0), dict(scale=float("inf")), dict(scale=float("nan")), dict(half=0), dict(half=8), dict(half=24),
                 dict(half=208), dict(nx=-1), dict(nx=65), dict(ny=-1), dict(ny=65), dict(nt=-1), dict(nt=65), dict(dtheta=float("inf")),
                 dict(dtheta=float("nan")), dict(margin=-1), dict(reserved=1)]
    for d in bad_specs:
        rc_, out = raw_hook(capi, scans, capi.scanmatch_spec(**dict(good, **d)), pairs)
        assert rc_ == capi.ERR_INVALID and (out == 0x55).all(), d
    sp = capi.scanmatch_spec(**good)
    for n in (0, -1, 4097):
        rc_, out = raw_hook(capi, scans, sp, pairs, n_pairs=n)
        assert rc_ == capi.ERR_INVALID and (out == 0x55).all(), n
    for p in ((-1, 0), (0, -1), (2, 0), (0, 2)):
        rc_, out = raw_hook(capi, scans, sp, [(p[0], p[1], (0.0, 0.0, 0.0))])
        assert rc_ == capi.ERR_INVALID and (out == 0x55).all(), p
    for a in range(3):
        for bad in (float("nan"), float("inf"), float("-inf")):
            g = [0.0, 0.0, 0.0]; g[a] = bad
            rc_, out = raw_hook(capi, scans, sp, [(0, 1, tuple(g))])
            assert rc_ == capi.ERR_INVALID and (out == 0x55).all(), (a, bad)
    # more than 2^20 nodes per pair: 129 * 129 * 65 = 1081665; more than 2^26 in the call: 129 * 129 * 5 = 83205 nodes x 807 pairs
    rc_, out = raw_hook(capi, scans, capi.scanmatch_spec(1.0, 16, 64, 64, 32, 0.1), pairs)
    assert rc_ == capi.ERR_INVALID and (out == 0x55).all()
    assert 129 * 129 * 63 <= 2 ** 20 < 129 * 129 * 65 and 83205 * 806 <= 2 ** 26 < 83205 * 807
    many = [(0, 1, (0.0, 0.0, 0.0))] * 807
    rc_, out = raw_hook(capi, scans, capi.scanmatch_spec(1.0, 16, 64, 64, 2, 0.1), many)
    assert rc_ == capi.ERR_INVALID and (out == 0x55).all()
    # no store
    rc_, out = raw_hook(capi, [], sp, pairs)
    assert rc_ == capi.ERR_STATE and (out == 0x55).all()
    # slamhip_hs_scans_edges: the spec, n, the guesses, a node outside the lattice
    r = np.zeros(1, capi.SCANMATCH_RESULT); r["cnt"] = 1
    z = np.full(3, 7.0); w = np.full(3, 7.0); v = np.full(1, 7, np.int32)
    pr = capi.scan_pairs(pairs)

    def edges(spx, n, res=r, prx=pr):
        return capi.lib().slamhip_hs_scans_edges(spx.ctypes.data_as(C.c_void_p), prx.ctypes.data_as(C.c_void_p), res.ctypes.data_as(C.c_void_p), n,
                                                 z.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p))
    assert edges(sp, 1) == 0 and v[0] == 1
    z[:] = 7.0; w[:] = 7.0; v[:] = 7
    assert edges(capi.scanmatch_spec(**dict(good, half=8)), 1) == capi.ERR_INVALID and edges(sp, 0) == capi.ERR_INVALID
    for f, bad in (("k", 2), ("k", -2), ("ix", 2), ("iy", -2), ("cnt", -1)):
        rr = r.copy(); rr[f] = bad
        assert edges(sp, 1, rr) == capi.ERR_INVALID, f
    bad_pr = capi.scan_pairs([(0, 1, (float("nan"), 0.0, 0.0))])
    assert edges(sp, 1, r, bad_pr) == capi.ERR_INVALID
    assert (z == 7.0).all() and (w == 7.0).all() and v[0] == 7


def test_invalid_pair_is_no_edge(capi):
    case = sc.CASES["empty_query_and_reference"]()
    sp = capi.scanmatch_spec(**case["spec"])
    z, w, valid = capi.scans_edges(sp, case["pairs"], run_hook(capi, case))
    assert not valid.any() and (w == 0.0).all()


# ---- the end-to-end lap with the hooks alone -----------------------------------------------------------------------------------------
def lap_edges(capi, L, match):
    """The loop edges of the lap's true loop pairs by `match` (the hook, or the device call) -> (pairs, results, loops for lap_graph)."""
    true = L["true"].astype(np.float64)
    ij = sc.lap_true_pairs(true)
    pairs = [(i, j, sc.lap_sector_guess(true, i, j)) for (i, j) in ij]
    sp = capi.scanmatch_spec(**sc.LAP_SPEC)
    res = match(sp, pairs)
    z, w, valid = capi.scans_edges(sp, pairs, res)
    loops = [(i, j, z[n], w[n]) for n, (i, j) in enumerate(ij) if valid[n] and sc.accept(res[n])]
    return pairs, res, z, loops


def lap_relax(capi, L, loops):
    p0 = np.asarray(L["drifted"], np.float32).astype(np.float64)
    N = p0.shape[0]
    ij = [(k, k + 1) for k in range(N - 1)] + [(int(l[0]), int(l[1])) for l in loops]
    z = [capi.pg_edge_between(p0[k], p0[k + 1]) for k in range(N - 1)] + [tuple(float(v) for v in l[2]) for l in loops]
    w = [rc.LAP_ODOM_W] * (N - 1) + [tuple(float(v) for v in l[3]) for l in loops]
    return capi.debug_pg_relax(p0, None, np.array(ij, np.int32), np.array(z, np.float64), np.array(w, np.float64), capi.pg_spec(5, 4 * N, tol=1e-8))[0]


def max_position_error(poses, true):
    d = np.asarray(poses, np.float64)[:, :2] - np.asarray(true, np.float64)[:, :2]
    return float(np.hypot(d[:, 0], d[:, 1]).max())


def test_lap_on_the_cpu(capi):
    """The end-to-end lap of tests/test_gpu_hector_scanmatch.py with the hooks alone: render_cases.lap() (tools/scenario.py's world,
    a keyframe every metre, odometry drifting by 0.2 degrees and 2 mm per step), loop edges for the TRUE loop pairs (keyframes at
    least 40 apart whose true positions lie within 2.5 m) from slamhip_debug_scans_match + slamhip_hs_scans_edges with K18's knowledge
    as the guess (no translation, the heading to the nearest sector), relaxed by slamhip_debug_pg_relax.  No ground-truth edge.
    Measured here (cells of 0.125 m, heading steps of 2 pi / 1024; DESIGN.md section 4 "K21"): 3 true loop pairs -- (47, 0), (48, 0),
    (48, 1) -- all accepted, each with a score of about 1180 for 720 points and cnt = 1; z lies at most 0.33 cells and 0.39 heading
    steps from the ground-truth relative pose; the largest keyframe position error is 1.361 m drifted and 0.074 m relaxed.  Asserted:
    every true pair is accepted, and the ordering relaxed < drifted."""
    L = rc.lap()
    true = L["true"].astype(np.float64)
    pairs, res, z, loops = lap_edges(capi, L, lambda sp, pr: capi.debug_scans_match(L["scans"], sp, pr))
    assert len(pairs) >= 1 and len(loops) == len(pairs)
    worst_c, worst_t = 0.0, 0.0
    for n, (i, j, _) in enumerate(pairs):
        t = rc._rel(true[i], true[j])
        dc = max(abs(z[n][0] - t[0]), abs(z[n][1] - t[1])) * sc.LAP_SCALE
        dt = abs(math.remainder(z[n][2] - t[2], 2 * math.pi)) / sc.LAP_SPEC["dtheta"]
        print("pair (%d, %d): score %d of %d points, cnt %d, %.2f cells and %.2f heading steps from the truth" %
              (i, j, res[n]["score"], res[n]["n_query"], res[n]["cnt"], dc, dt))
        worst_c, worst_t = max(worst_c, dc), max(worst_t, dt)
    relaxed = lap_relax(capi, L, loops)
    e_drift, e_relax = max_position_error(L["drifted"], true), max_position_error(relaxed, true)
    print("%d true loop pairs; worst %.2f cells, %.2f heading steps; largest keyframe error: drifted %.3f m, relaxed %.3f m" %
          (len(pairs), worst_c, worst_t, e_drift, e_relax))
    assert e_relax < e_drift
