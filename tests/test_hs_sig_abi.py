"""CPU-side checks of the scan signatures' interface (the slamhip_hs_sig_* calls, the three slamhip_hsproc_sig_* calls and the
slamhip_debug_sig* hooks) and the NumPy restatement of their definition (include/slamhip.h, slamhip_hs_sig_add) that
tests/test_gpu_hector_sig.py compares the device with.

The restatement (np_table, np_cells, np_ring, np_sector, np_sig, np_match, np_query, np_self) shares no text with hs_sig.h: the table
is a whole-array cosine extended by slicing, rings are a searchsorted on the squared boundaries, the sector is found from the crosses
with all 64 directions at once, signatures are filled by bitwise_or.at, matches are np.roll on unpacked bit arrays.  The library's
hooks run hs_sig.h (a square root with a fix-up, the quadrant and four steps, rotates and popcounts on words, a packed key).
Everything is compared with == on integers.  No compute calls on a device."""
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("slamhip_hs_sig_configure", "slamhip_hs_sig_add", "slamhip_hs_sig_add_scans", "slamhip_hs_sig_query", "slamhip_hs_sig_self",
           "slamhip_hs_sig_count", "slamhip_hs_sig_download", "slamhip_hs_sig_upload", "slamhip_hs_sig_clear", "slamhip_hsproc_sig_add",
           "slamhip_hsproc_sig_query", "slamhip_hsproc_sig_self", "slamhip_debug_sig_table", "slamhip_debug_sig", "slamhip_debug_sig_ring",
           "slamhip_debug_sig_sector", "slamhip_debug_sig_search")
F = np.float32
U64 = np.uint64
SECTORS = 64


@pytest.fixture(scope="module")
def capi():
    import slam.net_amd.build as b
    b.build()
    import slam.net_amd.capi as capi
    return capi


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def np_table():
    """Rule 1 -> (C, S) int64."""
    a = np.arange(16, dtype=np.float64) * np.pi / 32.0
    c = np.rint(16384.0 * np.cos(a)).astype(np.int64); s = np.rint(16384.0 * np.sin(a)).astype(np.int64)
    return np.concatenate([c, -s, -c, s]), np.concatenate([s, c, -s, -c])


def np_cells(xy, scale, wrong=None):
    """Rule 2 -> (keep mask, u, v) over the (n, 2) points."""
    p = np.asarray(xy, np.float32).reshape(-1, 2)
    f = p * F(scale)                                                       # (binary32 products, each rounded on its own)
    assert f.dtype == np.float32
    with np.errstate(invalid="ignore"):
        keep = (np.abs(f) < F(16384.0)).all(axis=1)
    g = np.where(keep[:, None], f, F(0.0)).astype(np.float64)
    cell = (np.trunc(g) if wrong == "trunc" else np.floor(g)).astype(np.int64)
    uv = 2 * cell + (0 if wrong == "no_plus_one" else 1)
    return keep, uv[:, 0], uv[:, 1]


def np_ring(d2, n_ring, ring_cells, wrong=None):
    """Rule 3: how many squared boundaries are <= d2."""
    bounds = (2 * ring_cells * np.arange(1, n_ring + 1, dtype=np.int64)) ** 2
    return np.searchsorted(bounds, np.asarray(d2, np.int64), side="left" if wrong == "ring_lt" else "right")


def np_sector(u, v, wrong=None):
    """Rule 4: the crosses with all 64 directions at once; the sector is where a non-negative cross is followed by a negative one."""
    u = np.asarray(u, np.int64); v = np.asarray(v, np.int64)
    if wrong == "atan2":
        return np.rint(np.arctan2(v.astype(np.float64), u.astype(np.float64)) * 32.0 / np.pi).astype(np.int64) % SECTORS
    C, S = np_table()
    cross = C[None, :] * v[:, None] - S[None, :] * u[:, None]
    last = (cross >= 0) & (np.roll(cross, -1, axis=1) < 0)
    assert (last.sum(axis=1) == 1).all()
    return np.argmax(last, axis=1)


def np_sig(xy, scale, n_ring, ring_cells, wrong=None):
    """Rules 2 - 5 -> (sig (n_ring,) uint64, info dict)."""
    keep, u, v = np_cells(xy, scale, wrong)
    u, v = u[keep], v[keep]
    ring = np_ring(u * u + v * v, n_ring, ring_cells, wrong)
    near = ring < n_ring
    sig = np.zeros(n_ring, U64)
    if near.any():
        np.bitwise_or.at(sig, ring[near], U64(1) << np_sector(u[near], v[near], wrong).astype(U64))
    return sig, {"n_points": int(keep.shape[0]), "n_ignored": int((~keep).sum()), "n_far": int((~near).sum()), "n_set": int(np_bits(sig).sum())}


def np_bits(sig):
    """Words -> bits: (..., n_ring) uint64 -> (..., n_ring, 64) bool, bit k in column k."""
    s = np.asarray(sig, U64)
    return ((s[..., None] >> np.arange(SECTORS, dtype=U64)) & U64(1)).astype(bool)


def np_match(q, keys, wrong=None):
    """Rule 6 of one query (n_ring,) against keys (N, n_ring) -> (shift, inter, uni, score, n_set_key), each (N,) int64."""
    Q = np_bits(q); K = np_bits(np.asarray(keys, U64).reshape(-1, Q.shape[0]))
    sgn = -1 if wrong == "sign" else 1
    inter = np.stack([(Q[None] & np.roll(K, sgn * s, axis=2)).sum(axis=(1, 2)) for s in range(SECTORS)], axis=1).astype(np.int64)
    shift = SECTORS - 1 - np.argmax(inter[:, ::-1], axis=1) if wrong == "tie_larger" else np.argmax(inter, axis=1)
    best = inter[np.arange(inter.shape[0]), shift]
    nk = K.sum(axis=(1, 2)).astype(np.int64)
    uni = int(Q.sum()) + nk - best
    score = best.copy() if wrong == "score_inter" else np.where(uni > 0, (best << 16) // np.maximum(uni, 1), 0)
    return shift, best, uni, score, nk


def np_hits(capi, index, shift, inter, uni, score, nk):
    h = np.zeros(len(index), capi.SIG_HIT_DTYPE)
    h["score"] = score; h["index"] = index; h["shift"] = shift; h["inter"] = inter; h["uni"] = uni; h["n_set_key"] = nk
    return h


def np_query(capi, q, store, first, last, B, wrong=None):
    """Rule 7 -> SIG_HIT_DTYPE records."""
    store = np.asarray(store, U64)
    if last <= first:
        return np.zeros(0, capi.SIG_HIT_DTYPE)
    shift, inter, uni, score, nk = np_match(q, store[first:last], wrong)
    idx = np.arange(first, last)
    order = np.lexsort((idx, -score))[:B]
    return np_hits(capi, idx[order], shift[order], inter[order], uni[order], score[order], nk[order])


def np_self(capi, store, first, last, min_gap):
    """Rule 8 -> one record per keyframe of [first, last)."""
    store = np.asarray(store, U64)
    out = np.zeros(max(last - first, 0), capi.SIG_HIT_DTYPE)
    out["index"] = -1
    for i in range(first, last):
        if i - min_gap >= first:
            out[i - first] = np_query(capi, store[i], store, first, i - min_gap + 1, 1)[0]
    return out


def random_store(seed, N, n_ring, density=0.15):
    g = np.random.Generator(np.random.Philox(seed))
    bits = g.random((N, n_ring, SECTORS)) < density
    return (bits.astype(U64) << np.arange(SECTORS, dtype=U64)).sum(axis=2).astype(U64)


def rotl(w, s):
    w = np.asarray(w, U64); s = int(s) % SECTORS
    return w if s == 0 else (w << U64(s)) | (w >> U64(SECTORS - s))


def hook_sig(capi, xy, scale, n_ring, ring_cells):
    sig, info = capi.debug_sig(np.asarray(xy, np.float32).reshape(-1, 2), capi.sig_spec(scale, n_ring, ring_cells))
    return sig, {k: int(info[k]) for k in ("n_points", "n_ignored", "n_far", "n_set")}


def same_sig(capi, xy, scale, n_ring, ring_cells):
    """hook == restatement for one scan -> the signature."""
    got, ginfo = hook_sig(capi, xy, scale, n_ring, ring_cells)
    want, winfo = np_sig(xy, scale, n_ring, ring_cells)
    assert np.array_equal(got, want), (got, want)
    assert ginfo == winfo, (ginfo, winfo)
    return got, ginfo


# ---- 1. the interface ----------------------------------------------------------------------------------------------------------------
def test_symbols_and_struct_sizes(capi):
    L = capi.lib()
    declared = set(capi.declared_symbols())
    for name in SYMBOLS:
        assert name in declared and hasattr(L, name) and name in L._signatures, name
    assert capi.SIG_SPEC.itemsize == 12 and capi.SIG_INFO.itemsize == 16 and capi.SIG_HIT_DTYPE.itemsize == 16
    header = open(os.path.join(ROOT, "include", "slamhip.h")).read()
    for text in ("#define SLAMHIP_SIG_SECTORS 64", "} slamhip_sig_spec;", "} slamhip_sig_info;", "} slamhip_sig_hit;", "theta_k - s * 2 pi / 64"):
        assert text in header, text
    assert (capi.SIG_SECTORS, capi.SIG_MAX_RINGS, capi.SIG_MAX_HITS, capi.SIG_MAX_KEYS) == (64, 32, 16, 1 << 20)
    for macro, value in (("SLAMHIP_SIG_MAX_RINGS", "32"), ("SLAMHIP_SIG_MAX_HITS", "16"), ("SLAMHIP_SIG_MAX_KEYS", "(1 << 20)")):
        assert re.search(r"#define %s %s\n" % (macro, re.escape(value)), header), macro


def test_csharp_and_build_list():
    native = open(os.path.join(ROOT, "bindings", "csharp", "SlamHip", "SlamHip.Native.cs")).read()
    for name in SYMBOLS:
        if not name.startswith("slamhip_debug"):
            assert re.search(r"static extern int %s\(" % name, native), name
    import slam.net_amd.build as b
    assert "hs_sig.hip" in b.SOURCES and os.path.exists(os.path.join(b.CSRC, "hs_sig.h"))


@pytest.mark.parametrize("scale,n_ring,rc", [(0.0, 4, 1), (-1.0, 4, 1), (float("nan"), 4, 1), (float("inf"), 4, 1), (1.0, 0, 1), (1.0, 33, 1),
                                              (1.0, 4, 0), (1.0, 32, 513), (1.0, 1, 16385), (1.0, -1, 1)])
def test_bad_specs_refused(capi, scale, n_ring, rc):
    with pytest.raises(capi.SlamhipError) as e:
        capi.debug_sig(np.zeros((1, 2), F), capi.sig_spec(scale, n_ring, rc))
    assert e.value.code == capi.ERR_INVALID


def test_largest_specs_accepted(capi):
    for n_ring, rc in ((32, 512), (1, 16384), (31, 528)):
        same_sig(capi, [[0.5, 0.5], [16383.5, 0.5]], 1.0, n_ring, rc)
    same_sig(capi, [[1e-30, 1.0]], np.finfo(np.float32).max, 2, 1)
    same_sig(capi, [[1e30, 1.0]], np.finfo(np.float32).tiny, 2, 1)


def test_search_refusals(capi):
    store = random_store(3, 8, 3)
    q = store[0].copy()
    bad = [dict(B=0), dict(B=17), dict(first=-1), dict(first=5, last=4), dict(last=9)]
    for kw in bad:
        a = dict(first=0, last=8, B=1); a.update(kw)
        with pytest.raises(capi.SlamhipError) as e:
            capi.debug_sig_search(q, store, a["first"], a["last"], 1, a["B"])
        assert e.value.code == capi.ERR_INVALID, kw
    for gap in (0, -3):
        with pytest.raises(capi.SlamhipError) as e:
            capi.debug_sig_search(None, store, 0, 8, gap)
        assert e.value.code == capi.ERR_INVALID
    ns = capi.sig_popcounts(store)
    assert np.array_equal(ns, np_bits(store).sum(axis=(1, 2)))
    ns[5] += 1                                                             # a popcount that disagrees with its words
    for query in (q, None):
        with pytest.raises(capi.SlamhipError) as e:
            capi.debug_sig_search(query, store, 0, 8, 1, 1, n_set=ns)
        assert e.value.code == capi.ERR_INVALID
    assert len(capi.debug_sig_search(q, store, 0, 5, 1, 1, n_set=ns)) == 1  # ... outside the range it is not looked at
    with pytest.raises(capi.SlamhipError):
        capi.debug_sig_search(q, np.zeros((8, 33), U64), 0, 8, 1, 1)       # n_ring = 33


# ---- 2. the table and the partition ------------------------------------------------------------------------------------------------
def test_table(capi):
    C, S = capi.debug_sig_table()
    wC, wS = np_table()
    assert np.array_equal(C, wC) and np.array_equal(S, wS)
    C = C.astype(np.int64); S = S.astype(np.int64)
    assert C[0] == 16384 and S[0] == 0 and C[16] == 0 and S[16] == 16384
    assert np.array_equal(np.roll(C, -16), -S) and np.array_equal(np.roll(S, -16), C)      # a quarter turn is exact
    assert np.array_equal(np.roll(C, -32), -C) and np.array_equal(np.roll(S, -32), -S)
    cross = C * np.roll(S, -1) - S * np.roll(C, -1)                         # cross(d_k, d_{k+1}) > 0: strictly ordered round the circle
    assert (cross > 0).all()
    assert (np.diff(S[:17]) > 0).all() and (np.diff(C[:17]) < 0).all()
    assert np.abs(C).max() == 16384 and np.abs(S).max() == 16384


def test_partition_on_a_box(capi):
    """Exactly one k for every odd (u, v) in [-129, 129]^2 (np_sector asserts it), and the kernel's quadrant + four steps finds it."""
    o = np.arange(-129, 130, 2)
    u, v = [a.ravel() for a in np.meshgrid(o, o)]
    want = np_sector(u, v)
    got = capi.debug_sig_sector(np.stack([u, v], axis=1))
    assert np.array_equal(got, want)
    assert set(want.tolist()) == set(range(64))
    far = np.array([[32767, 1], [32767, -1], [-32767, 1], [1, 32767], [-1, -32767], [32767, 32767], [-32767, 32765], [3277, 32767]])
    assert np.array_equal(capi.debug_sig_sector(far), np_sector(far[:, 0], far[:, 1]))
    for bad in ([[2, 1]], [[1, 0]], [[32769, 1]]):
        with pytest.raises(capi.SlamhipError):
            capi.debug_sig_sector(np.array(bad))


@pytest.mark.parametrize("rc", [1, 3, 512])
@pytest.mark.parametrize("n_ring", [1, 2, 31, 32])
def test_ring_at_every_boundary(capi, rc, n_ring):
    b = (2 * rc * np.arange(1, n_ring + 1, dtype=np.int64)) ** 2
    d2 = np.unique(np.clip(np.concatenate([b - 1, b, b + 1, [0, 1, 2, 2 ** 31 - 1, 2 * 32767 ** 2]]), 0, 2 ** 31 - 1))
    got = capi.debug_sig_ring(d2, n_ring, rc)
    assert np.array_equal(got, np_ring(d2, n_ring, rc))
    assert got[0] == 0 and got.max() == n_ring
    # the wrong copy: `<` in place of `<=` differs exactly on the boundaries
    wrong = np_ring(d2, n_ring, rc, "ring_lt")
    assert np.array_equal(got != wrong, np.isin(d2, b))


def test_ring_dense(capi):
    d2 = np.arange(0, 70000, dtype=np.int64)
    for n_ring, rc in ((32, 4), (5, 7), (1, 1)):
        assert np.array_equal(capi.debug_sig_ring(d2, n_ring, rc), np_ring(d2, n_ring, rc))


# ---- 3. signatures -----------------------------------------------------------------------------------------------------------------
def test_edges_of_rule_2(capi):
    big = F(16384.0)
    below = np.nextafter(big, F(0.0))
    pts = np.array([[below, 0.5], [0.5, below], [-below, 0.5], [big, 0.5], [0.5, -big], [-big, -big], [np.nan, 1.0], [1.0, np.nan],
                    [np.inf, 1.0], [1.0, -np.inf], [-0.0, 0.5], [0.5, -0.0], [-0.0, -0.0], [16383.0, 16383.0], [-16383.0, -16384.0 + 0.5]], F)
    sig, info = same_sig(capi, pts, 1.0, 32, 512)
    assert info["n_points"] == 15 and info["n_ignored"] == 7 and info["n_far"] == 2
    _, u, v = np_cells(pts[10:13], 1.0)
    assert u.tolist() == [1, 1, 1] and v.tolist() == [1, 1, 1]             # -0.0 lies in the cell of +0.0
    # scale is applied in binary32 before the floor
    same_sig(capi, [[0.1, 0.7], [-0.3, 2.9], [1e-3, -1e-3]], 10.0, 8, 2)
    same_sig(capi, [[3.0, 3.0]], F(1.0) / F(3.0), 8, 1)


def test_empty_and_one_cell(capi):
    sig, info = same_sig(capi, np.zeros((0, 2), F), 2.0, 5, 3)
    assert not sig.any() and info == {"n_points": 0, "n_ignored": 0, "n_far": 0, "n_set": 0}
    pts = np.full((300, 2), 0.0, F)
    pts[:, 0] = np.linspace(4.01, 4.99, 300); pts[:, 1] = np.linspace(-2.99, -2.01, 300)
    sig, info = same_sig(capi, pts, 1.0, 8, 1)
    assert info["n_set"] == 1 and info["n_points"] == 300


@pytest.mark.parametrize("n_ring,rc", [(1, 64), (7, 64), (32, 64), (32, 512)])
def test_a_point_in_every_cell(capi, n_ring, rc):
    """A point at the polar centre of each of the 64 * n_ring cells.  The rings are wide enough (rc >= 64) for the grid cell's centre,
    at most 0.71 cells from the point, to stay in the polar cell: half a ring is 32 cells, half a sector's arc at radius 32 is 1.57."""
    r = (np.arange(n_ring) + 0.5) * rc
    a = (np.arange(64) + 0.5) * (2.0 * np.pi / 64.0)
    pts = np.stack([np.outer(r, np.cos(a)).ravel(), np.outer(r, np.sin(a)).ravel()], axis=1).astype(F)
    sig, info = same_sig(capi, pts, 1.0, n_ring, rc)
    assert (sig == U64(0xFFFFFFFFFFFFFFFF)).all() and info["n_set"] == 64 * n_ring and info["n_far"] == 0
    sig, info = same_sig(capi, pts, 1.0, n_ring, rc // 2)                  # rings of half the width: the outer points are FAR
    assert info["n_far"] >= 64 * (n_ring // 2)


def test_random_scans(capi):
    g = np.random.Generator(np.random.Philox(18))
    for n, scale, n_ring, rc in ((1, 1.0, 1, 1), (255, 3.0, 9, 2), (257, 20.0, 32, 4), (1080, 10.0, 20, 5), (4000, 0.5, 3, 1)):
        pts = (g.standard_normal((n, 2)) * (n_ring * rc * 0.7 / scale)).astype(F)
        same_sig(capi, pts, scale, n_ring, rc)


# ---- 4. matches --------------------------------------------------------------------------------------------------------------------
def same_query(capi, q, store, first, last, B):
    got = capi.debug_sig_search(q, store, first, last, 1, B)
    want = np_query(capi, q, store, first, last, B)
    assert got.tobytes() == want.tobytes(), (got, want)
    return got


def same_self(capi, store, first, last, min_gap):
    got = capi.debug_sig_search(None, store, first, last, min_gap)
    want = np_self(capi, store, first, last, min_gap)
    assert got.tobytes() == want.tobytes(), (first, last, min_gap, np.flatnonzero(got != want)[:5])
    return got


def quarter_scan(n=200, seed=7):
    """Points whose scaled coordinates (scale 4) are all k + 1/4, within 30 cells."""
    g = np.random.Generator(np.random.Philox(seed))
    return ((g.integers(-30, 30, (n, 2)) + 0.25) / 4.0).astype(F)


def test_quarter_turn(capi):
    """The scan and its turn by +90 degrees, (-y, x): every cell's centre turns exactly, and the table's quarter turn is exact, so the
    signature is rotated by exactly 16 bits.  The turned scan is what the robot sees after turning by -90 degrees: the query's heading
    is theta_k - 16 * 2 pi / 64, the sign rule 6 states."""
    scale, n_ring, rc = 4.0, 16, 2
    p = quarter_scan()
    t = np.stack([-p[:, 1], p[:, 0]], axis=1)
    sp, ip = same_sig(capi, p, scale, n_ring, rc)
    st, it = same_sig(capi, t, scale, n_ring, rc)
    assert np.array_equal(st, rotl(sp, 16)) and ip == it and ip["n_set"] > 100
    store = np.stack([random_store(1, 1, n_ring)[0], sp, random_store(2, 1, n_ring)[0]])
    h = same_query(capi, st, store, 0, 3, 3)
    assert h[0]["index"] == 1 and h[0]["score"] == 65536 and h[0]["shift"] == 16
    assert h[0]["inter"] == h[0]["uni"] == h[0]["n_set_key"] == ip["n_set"]
    x, y, th = capi.sig_pose_guess((3.0, -2.0, 0.3), h[0]["shift"])
    assert (x, y) == (3.0, -2.0) and th == math.remainder(0.3 - 16 * 2.0 * math.pi / 64.0, 2.0 * math.pi)
    # the wrong copy with the heading's sign flipped puts the shift on the other side
    assert np_query(capi, st, store, 0, 3, 1, "sign")[0]["shift"] == 48
    back = same_query(capi, sp, np.stack([st]), 0, 1, 1)                   # ... and the other way round
    assert back[0]["shift"] == 48 and back[0]["score"] == 65536
    # one point ON an integer coordinate.  On the axis the turn keeps (x -> y') the cell still turns into the turned cell ...
    p2 = p.copy(); p2[0] = (F(5.0 / 4.0), F(7.25 / 4.0))
    t2 = np.stack([-p2[:, 1], p2[:, 0]], axis=1)
    s2, _ = same_sig(capi, p2, scale, n_ring, rc)
    st2, _ = same_sig(capi, t2, scale, n_ring, rc)
    _, u, v = np_cells(p2[:1], scale); _, ut, vt = np_cells(t2[:1], scale)
    assert (int(u[0]), int(v[0])) == (11, 15) and (int(ut[0]), int(vt[0])) == (-15, 11)
    # ... on the axis the turn negates (y -> -x') it does not: floor(-k) is -k, not -(k + 1)
    p3 = p.copy(); p3[0] = (F(7.25 / 4.0), F(5.0 / 4.0))
    t3 = np.stack([-p3[:, 1], p3[:, 0]], axis=1)
    _, u, v = np_cells(p3[:1], scale); _, ut, vt = np_cells(t3[:1], scale)
    assert (int(u[0]), int(v[0])) == (15, 11) and (int(ut[0]), int(vt[0])) == (-9, 15)      # -v would be -11
    s3, _ = same_sig(capi, p3, scale, n_ring, rc)
    st3, _ = same_sig(capi, t3, scale, n_ring, rc)
    same_query(capi, st3, np.stack([s3]), 0, 1, 1)                         # whatever the restatement says
    same_query(capi, st2, np.stack([s2]), 0, 1, 1)


def test_ties(capi):
    n_ring = 3
    full = np.full(n_ring, 0xFFFFFFFFFFFFFFFF, U64)
    sym = np.array([0x0001000100010001, 0, 0x8000800080008000], U64)       # period 16: shifts 0, 16, 32, 48 tie
    store = np.stack([sym, full, sym, rotl(sym, 5), np.zeros(n_ring, U64), sym])
    h = same_query(capi, sym, store, 0, 6, 6)
    assert h["index"].tolist() == [0, 2, 3, 5, 1, 4] and h["shift"].tolist() == [0, 0, 11, 0, 0, 0]     # equal scores: the lower index first
    assert h["score"][:4].tolist() == [65536] * 4 and h["score"][5] == 0
    assert np_query(capi, sym, store, 0, 6, 1, "tie_larger")[0]["shift"] == 48            # the wrong copy: the tie to the larger shift
    assert same_query(capi, full, store, 1, 2, 1)[0]["shift"] == 0                         # every shift ties
    assert np_query(capi, full, store, 1, 2, 1, "tie_larger")[0]["shift"] == 63
    part = same_query(capi, sym, store, 1, 2, 1)[0]                                        # the wrong copy: score = inter
    assert part["score"] == (8 << 16) // 192 and part["inter"] == 8 and np_query(capi, sym, store, 1, 2, 1, "score_inter")[0]["score"] == 8
    same_self(capi, store, 0, 6, 1)
    assert same_self(capi, store, 0, 6, 1)["index"].tolist() == [-1, 0, 0, 0, 0, 0]


def test_empty_signatures_and_ranges(capi):
    n_ring = 4
    z = np.zeros(n_ring, U64)
    store = np.concatenate([random_store(5, 3, n_ring), z[None], random_store(6, 2, n_ring)])
    h = same_query(capi, z, store, 0, 6, 16)                               # an empty query: every score 0, the order is the index
    assert len(h) == 6 and h["index"].tolist() == list(range(6)) and not h["score"].any() and not h["shift"].any()
    assert h["uni"].tolist() == capi.sig_popcounts(store).tolist()
    h = same_query(capi, store[0], store, 3, 4, 1)                         # an empty key
    assert h[0]["score"] == 0 and h[0]["uni"] == capi.sig_popcounts(store)[0] and h[0]["n_set_key"] == 0
    h = same_query(capi, z, store, 3, 4, 2)                                # both empty: uni = 0, score 0
    assert len(h) == 1 and h[0]["uni"] == 0 and h[0]["score"] == 0
    assert len(same_query(capi, store[0], store, 2, 2, 4)) == 0            # first = last
    assert len(same_query(capi, store[0], store, 6, 6, 4)) == 0
    assert len(same_query(capi, store[0], store, 1, 4, 16)) == 3           # B larger than the range
    assert len(capi.debug_sig_search(store[0], np.zeros((0, n_ring), U64), 0, 0, 1, 3)) == 0
    assert len(capi.debug_sig_search(None, store, 4, 4, 1)) == 0


@pytest.mark.parametrize("N", [1, 63, 64, 65, 129])
def test_self_search(capi, N):
    store = random_store(100 + N, N, 2, 0.3)
    store[N // 2] = store[0]                                               # a revisit
    for gap in (1, 64, 65, N):
        h = same_self(capi, store, 0, N, gap)
        assert (h["index"][:gap] == -1).all() and (h["index"][gap:] >= 0).all() and (h["index"][gap:] <= np.arange(gap, N) - gap).all()
    if N > 4:
        same_self(capi, store, 3, N - 1, 1)
        assert same_self(capi, store, 0, N, 1)[N // 2]["score"] == 65536 or N // 2 == 0


def test_query_random(capi):
    for n_ring, N in ((1, 70), (8, 40), (9, 40), (20, 33), (32, 20)):
        store = random_store(n_ring, N, n_ring)
        q = rotl(store[N // 3], 37)
        q[0] ^= U64(0x10)
        h = same_query(capi, q, store, 0, N, 16)
        assert h[0]["index"] == N // 3 and h[0]["shift"] == 37
        same_query(capi, q, store, 5, N - 3, 2)


def test_packed_key_at_its_limits(capi):
    """The self search's key: index 2^20 - 1 and 2^20 - 2, shift 63, score 65536 -- every field at its largest."""
    N = capi.SIG_MAX_KEYS
    store = np.zeros((N, 1), U64)
    w = U64(0x00000000DEADBEEF)
    store[N - 3, 0] = w; store[N - 2, 0] = rotl(w, 1); store[N - 1, 0] = w
    ns = np.zeros(N, np.uint16); ns[N - 3:] = 24
    h = capi.debug_sig_search(None, store, N - 3, N, 1, 1, n_set=ns)
    assert h.tobytes() == np_self(capi, store, N - 3, N, 1).tobytes()
    assert h["index"].tolist() == [-1, N - 3, N - 3] and h["shift"].tolist() == [0, 1, 0] and h["score"].tolist() == [0, 65536, 65536]
    h = capi.debug_sig_search(None, store, N - 2, N, 1, 1, n_set=ns)       # only N - 2 is left as a key: q == rotl(k, 63)
    assert (h[1]["index"], h[1]["shift"], h[1]["score"]) == (N - 2, 63, 65536)
    q = capi.debug_sig_search(w.reshape(1), store, N - 3, N, 1, 2, n_set=ns)
    assert q["index"].tolist() == [N - 3, N - 2] and q["shift"].tolist() == [0, 63] and q["score"].tolist() == [65536, 65536]
    with pytest.raises(capi.SlamhipError):
        capi.debug_sig_search(None, np.zeros((N + 1, 1), U64), 0, 1, 1)


# ---- 5. wrong copies of the rules, each failing a named case -----------------------------------------------------------------------
def test_wrong_copies_fail(capi):
    # floor replaced by truncation: a negative coordinate
    pts = np.array([[-0.5, 0.5]], F)
    got, _ = same_sig(capi, pts, 1.0, 4, 1)
    assert not np.array_equal(got, np_sig(pts, 1.0, 4, 1, "trunc")[0])
    # u = 2 floor without the + 1: the cell (3, 0), whose centre is off the axis
    pts = np.array([[3.25, 0.25]], F)
    got, _ = same_sig(capi, pts, 1.0, 4, 1)
    assert got[3] == U64(2) and np_sig(pts, 1.0, 4, 1, "no_plus_one")[0][3] != U64(2)
    # ring by `<`: test_ring_at_every_boundary (no odd (u, v) lies on a boundary: u^2 + v^2 = 2 mod 8)
    b = np.array([36], np.int64)
    assert capi.debug_sig_ring(b, 4, 3)[0] == 1 and np_ring(b, 4, 3, "ring_lt")[0] == 0
    # sector by a rounded atan2: a direction in the upper half of sector 0
    pts = np.array([[7.5, 0.5]], F)
    got, _ = same_sig(capi, pts, 1.0, 8, 1)
    assert got[7] == U64(1) and np_sig(pts, 1.0, 8, 1, "atan2")[0][7] == U64(2)
    # the tie to the larger shift, score = inter: test_ties; the heading sign flipped: test_quarter_turn


# ---- 6. end to end on the simulator's field ----------------------------------------------------------------------------------------
SIM_SCALE, SIM_RINGS, SIM_RC = 2.0, 32, 1          # cells of 0.5 m, 32 rings of one cell: 16 m of reach
SIM_STEP_M, SIM_RAYS = 1.0, 720
SIM_ALPHA = 0.7                                    # radians: 7.13 sectors
SIM_OFFSET = (0.10, -0.05)                         # metres from the keyframe's position at the revisit


def sim_lap():
    from slam.net_amd import sim
    segs = sim.default_field()
    poses, _ = sim.lap_trajectory(step=SIM_STEP_M)
    scans = [sim.make_scan(segs, p, SIM_RAYS, noise=False)[1] for p in poses]
    return sim, segs, poses, scans


def revisit(sim, segs, pose, alpha, offset):
    """The scan taken again at the keyframe's position (+ offset), the robot turned by -alpha: everything is seen alpha further round."""
    p = (float(pose[0]) + offset[0], float(pose[1]) + offset[1], float(pose[2]) - alpha)
    return sim.make_scan(segs, p, SIM_RAYS, rng=sim.PCG32(99), noise=True)[1]


def test_end_to_end_lap(capi):
    sim, segs, poses, scans = sim_lap()
    store = np.stack([np_sig(s, SIM_SCALE, SIM_RINGS, SIM_RC)[0] for s in scans])
    for j, s in enumerate(scans[::7]):
        assert np.array_equal(capi.debug_sig(s, capi.sig_spec(SIM_SCALE, SIM_RINGS, SIM_RC))[0], store[7 * j])
    N = len(scans)
    want_shift = SIM_ALPHA * 64.0 / (2.0 * math.pi)
    for j in (3, N // 3, N // 2, N - 5):
        q_xy = revisit(sim, segs, poses[j], SIM_ALPHA, SIM_OFFSET)
        q, _ = np_sig(q_xy, SIM_SCALE, SIM_RINGS, SIM_RC)
        want = np_query(capi, q, store, 0, N, 4)
        assert want[0]["index"] == j, (j, want)                            # the restatement first ...
        d = (int(want[0]["shift"]) - want_shift) % 64.0
        assert min(d, 64.0 - d) <= 1.0, (j, want[0])
        got = capi.debug_sig_search(capi.debug_sig(q_xy, capi.sig_spec(SIM_SCALE, SIM_RINGS, SIM_RC))[0], store, 0, N, 1, 4)
        assert got.tobytes() == want.tobytes()                             # ... then the library is held to it
        x, y, th = capi.sig_pose_guess(poses[j], got[0]["shift"])
        assert abs(math.remainder(th - (float(poses[j][2]) - SIM_ALPHA), 2.0 * math.pi)) <= 2.0 * math.pi / 64.0
