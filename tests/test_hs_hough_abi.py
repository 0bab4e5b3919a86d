"""CPU-side checks of the Hough transform's interface (slamhip_hs_hough, _hough_rotation, _hough_shifts, _hough_clear, the three
slamhip_hsproc_hough* calls and the four slamhip_debug_hough* hooks) and the NumPy restatement of its definition (include/slamhip.h,
slamhip_hs_hough) that tests/test_gpu_hector_hough.py compares the device with.

The restatement (np_table, np_hough, np_rotation, np_xcorr) shares no text with hs_hough.h: the table is formed with NumPy's cosine
over whole arrays and mirrored by slicing, the votes are one bincount over a sites x angles array of int64 bins, the correlation
is np.convolve on uint64.  The library's hooks run hs_hough.h (site bits by word, ctz, a 32-bit bin, the arg-max kept as a running
record).  Everything is compared with == on integers.  No compute calls on a device."""
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("slamhip_hs_hough", "slamhip_hs_hough_rotation", "slamhip_hs_hough_shifts", "slamhip_hs_hough_clear", "slamhip_hsproc_hough",
           "slamhip_hsproc_hough_rotation", "slamhip_hsproc_hough_shifts", "slamhip_debug_hough_table", "slamhip_debug_hough",
           "slamhip_debug_hough_rotation", "slamhip_debug_hough_xcorr")
F = np.float32
SHAPES = [(1, 1), (1, 37), (37, 1), (16, 16), (33, 65), (64, 64), (65, 64), (130, 70)]     # (w, h)
TS = (4, 8, 12, 180)
QS = (0, 1, 3)


@pytest.fixture(scope="module")
def capi():
    import slam.net_amd.build as b
    b.build()
    import slam.net_amd.capi as capi
    return capi


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def np_table(T):
    """Step 1 -> (C, S) int64."""
    k = np.arange(1, T // 2, dtype=np.float64)
    a = (k * np.pi) / np.float64(T)
    ch = np.rint(16384.0 * np.cos(a)).astype(np.int64); sh = np.rint(16384.0 * np.sin(a)).astype(np.int64)
    C = np.concatenate([[16384], ch, [0], -ch[::-1]]); S = np.concatenate([[0], sh, [16384], sh[::-1]])
    assert C.shape == S.shape == (T,)
    return C, S


def np_bins(w, h, q):
    D = w + h
    return D, ((2 * D) >> q) + 1


def np_hough(cls, site_mask, T, q, late_offset=False):
    """Steps 2 and 3 -> (H (T, N) uint32, HS (T,) uint64, n_sites).  late_offset: a WRONG copy of the rule -- the bin formed without
    + D * 16384 under the floor shift, D >> q added afterwards."""
    cls = np.asarray(cls)
    h, w = cls.shape
    D, N = np_bins(w, h, q)
    C, S = np_table(T)
    j, i = np.nonzero((site_mask >> cls.astype(np.int64)) & 1)
    arg = i[:, None].astype(np.int64) * C[None, :] + j[:, None].astype(np.int64) * S[None, :]
    if late_offset:
        p = (arg >> (14 + q)) + (D >> q)
    else:
        arg = arg + D * 16384
        assert arg.size == 0 or (arg.min() >= 0 and arg.max() < 2 ** 31)
        p = arg >> (14 + q)
    assert p.size == 0 or (p.min() >= 0 and p.max() < N)
    flat = (np.arange(T, dtype=np.int64)[None, :] * N + p).ravel()
    H = np.bincount(flat, minlength=T * N).reshape(T, N)
    HS = (H.astype(np.uint64) ** 2).sum(1, dtype=np.uint64)
    return H.astype(np.uint32), HS, int(i.shape[0])


def np_rotation(hd, hs):
    """Step 4 -> (CC (T,) uint64, sh_d, sh_s)."""
    sh = []
    for s in (hd, hs):
        mx, n = int(np.max(s)), 0
        while (mx >> n) >= 2 ** 26:
            n += 1
        sh.append(n)
    a = np.asarray(hd, np.uint64) >> np.uint64(sh[0]); b = np.asarray(hs, np.uint64) >> np.uint64(sh[1])
    return np.array([int((a * np.roll(b, m)).sum(dtype=np.uint64)) for m in range(a.shape[0])], np.uint64), sh[0], sh[1]


def np_pair(T, m, k):
    """Step 5's source row and flip."""
    kk = k - m
    n = 0
    while kk < 0:
        kk += T; n += 1
    return kk, n & 1, n


def np_xcorr(A, B, flip, wrong_flip=False):
    """Step 5 over a destination row A and a source ROW B -> (XC uint64, (best_shift, n_ties, best_value, sum)).  wrong_flip: a WRONG
    copy of the rule -- the flip as N_s - p' (p' = 0 then reads nothing)."""
    A = np.asarray(A, np.uint64); B = np.asarray(B, np.uint64)
    Ns = B.shape[0]
    if flip:
        Bp = np.concatenate([[0], B[:0:-1]]).astype(np.uint64) if wrong_flip else B[::-1]
    else:
        Bp = B
    xc = np.convolve(A, Bp[::-1])                                          # entry n: sum_p' A[n - (Ns - 1) + p'] B'[p']
    assert xc.dtype == np.uint64 and xc.shape[0] == A.shape[0] + Ns - 1
    best = xc.max()
    at = np.nonzero(xc == best)[0]
    return xc, (int(at[0]) - (Ns - 1), int(at.shape[0]), int(best), int(xc.sum(dtype=np.uint64)))


def rec_tuple(r):
    return (int(r["best_shift"]), int(r["n_ties"]), int(r["best_value"]), int(r["sum"]))


def class_map(w, h, seed, p=(0.6, 0.15, 0.25)):
    return np.random.default_rng([seed, w, h]).choice(3, (h, w), p=list(p)).astype(np.uint8)


def hook_equals(capi, cls, mask, T, q):
    H, HS = capi.debug_hough(cls, mask, T, q)
    wH, wHS, n = np_hough(cls, mask, T, q)
    assert H.dtype == np.uint32 and H.shape == wH.shape and np.array_equal(H, wH), (cls.shape, mask, T, q, np.argwhere(H != wH)[:5].tolist())
    assert np.array_equal(HS, wHS)
    assert (H.sum(1, dtype=np.int64) == n).all()
    return H, HS, n


# ---- the surface -------------------------------------------------------------------------------------------------------------------
def test_surface(capi):
    L = capi.lib()
    header = open(os.path.join(ROOT, "include", "slamhip.h")).read()
    native = open(os.path.join(ROOT, "bindings", "csharp", "SlamHip", "SlamHip.Native.cs")).read()
    bare = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for n in SYMBOLS:
        assert hasattr(L, n) and n in L._signatures, n
        proto = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % n, bare, re.S)
        assert proto, n
        assert len([a for a in proto.group(1).split(",") if a.strip()]) == len(L._signatures[n][1]), n
        if not n.startswith("slamhip_debug"):
            stub = re.search(r"static extern int %s\(([^;]*?)\);" % n, native, re.S)
            assert stub and len([a for a in stub.group(1).split(",") if a.strip()]) == len(L._signatures[n][1]), n
    assert [len(L._signatures[n][1]) for n in SYMBOLS] == [10, 2, 5, 1, 10, 2, 5, 2, 8, 4, 7]
    R = capi.HOUGH_SHIFT
    assert R.itemsize == 24 and list(R.names) == ["best_shift", "n_ties", "best_value", "sum"] and [R.fields[f][1] for f in R.names] == [0, 4, 8, 16]
    m = re.search(r"typedef struct slamhip_hough_shift \{(.*?)\} slamhip_hough_shift;\s*/\*(.*?)\*/", header, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert re.findall(r"(\w+)\s*[,;]", body) == list(R.names) and "24 bytes" in m.group(2)
    assert "struct HoughShift" in native
    assert "SLAMHIP_K_COUNT = 10" in header                                 # no new timing class
    import slam.net_amd.build as b
    import slam.net_amd.hector as hm
    for n in ("hough", "hough_rotation", "hough_shifts"):
        assert hasattr(hm.MapRepMultiMap, n) and hasattr(hm.HectorSLAMProcessor, n), n
    assert hasattr(hm.HectorSLAMProcessor, "AlignMaps") and hasattr(hm.MapRepMultiMap, "hough_clear")
    assert "hs_hough.hip" in b.SOURCES and "hs_hough.h" in b.HEADERS
    shim = os.path.join(ROOT, "bindings", "csharp", "SlamHip", "HectorSLAM")
    used = set(re.findall(r"Native\.(slamhip_\w+)", open(os.path.join(shim, "MapRepMultiMap.Hip.cs")).read()
                          + open(os.path.join(shim, "HectorSLAMProcessor.Hip.cs")).read()))
    assert {n for n in SYMBOLS if not n.startswith("slamhip_debug")} <= used
    assert "AlignMaps" in open(os.path.join(shim, "HectorSLAMProcessor.Hip.cs")).read()


# ---- the table ---------------------------------------------------------------------------------------------------------------------
def test_table_every_T(capi):
    """Hook (libm's cos and sin) against restatement (NumPy's) for every multiple of 4 up to 1024, which holds every T of both files.
    No disagreement across a rounding boundary was found; if one ever appears it shows here, on the CPU."""
    for T in range(4, 1025, 4):
        C, S = capi.debug_hough_table(T)
        wC, wS = np_table(T)
        assert C.dtype == np.int32 and np.array_equal(C, wC) and np.array_equal(S, wS), T
        assert C[0] == 16384 and S[0] == 0 and C[T // 2] == 0 and S[T // 2] == 16384
        assert (S >= 0).all() and np.array_equal(C[1:], -C[:0:-1]) and np.array_equal(S[1:], S[:0:-1])
        assert (np.abs(C) + np.abs(S)).max() <= 23172                      # what k17_vote's 96-bin span rests on: 63 * 23172 >> 14 = 89


def test_table_refusals(capi):
    out = np.zeros(4096, np.int32)
    for T in (0, 2, 3, 6, 1028, -4):
        assert capi.lib().slamhip_debug_hough_table(T, out.ctypes.data) == capi.ERR_INVALID, T


# ---- known answers worked out by hand ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", QS)
def test_one_site(capi, q):
    w, h, i, j, T = 23, 17, 9, 13, 12
    c = np.zeros((h, w), np.uint8); c[j, i] = 1
    H, HS, n = hook_equals(capi, c, 2, T, q)
    D = w + h
    assert n == 1 and (HS == 1).all()
    assert np.nonzero(H[0])[0].tolist() == [(i + D) >> q] and np.nonzero(H[T // 2])[0].tolist() == [(j + D) >> q]


@pytest.mark.parametrize("q", QS)
@pytest.mark.parametrize("T", TS)
def test_four_corners_reach_both_end_bins(capi, T, q):
    w, h = 40, 25
    c = np.zeros((h, w), np.uint8); c[0, 0] = c[0, w - 1] = c[h - 1, 0] = c[h - 1, w - 1] = 1
    H, HS, n = hook_equals(capi, c, 2, T, q)                               # (np_hough asserts that nothing lies outside [0, N))
    D, N = np_bins(w, h, q)
    assert n == 4 and H.shape[1] == N
    # bin N - 1 = (2 D) >> q holds the argument 2 D 16384 alone, bin 0 the arguments below 2^(14 + q): both are reachable by the rule
    # (the last by no cell of a map, whose argument stays below (2 D - 1) 16384), and a 1 x 1 map at q = 3 reaches bin 0 ...
    one = np.ones((1, 1), np.uint8)
    H1, _, _ = hook_equals(capi, one, 2, T, 3)
    assert H1.shape[1] == 1 and (H1[:, 0] == 1).all()                      # ... which there is bin N - 1 too
    lo = int(np.nonzero(H.sum(0))[0].min()); hi = int(np.nonzero(H.sum(0))[0].max())
    assert 0 <= lo and hi <= N - 1


def test_horizontal_wall(capi):
    # (L - 1) * |C[T/2 +- 1]| = 69 * 286 > 16384: at the neighbouring angles the wall crosses a bin border, so T/2 alone holds it in one bin
    w, h, L, T = 90, 31, 70, 180
    c = np.zeros((h, w), np.uint8); c[11, 5:5 + L] = 1
    H, HS, n = hook_equals(capi, c, 2, T, 0)
    assert n == L and H[T // 2].max() == L and np.count_nonzero(H[T // 2]) == 1 and H[T // 2, 11 + w + h] == L
    assert HS[T // 2] == L * L and int(np.argmax(HS)) == T // 2 and (HS[np.arange(T) != T // 2] < L * L).all()


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("w,h", SHAPES)
def test_empty_and_full_maps(capi, w, h, T):
    for q in QS:
        H, HS, n = hook_equals(capi, np.full((h, w), 2, np.uint8), 2, T, q)
        assert n == 0 and not H.any() and not HS.any()
        H, HS, n = hook_equals(capi, np.ones((h, w), np.uint8), 2, T, q)
        assert n == w * h and (H.sum(1, dtype=np.int64) == w * h).all()
        assert H.max() <= (2 * (1 << q) + 1) * max(w, h)                   # step 2's bound on an entry


@pytest.mark.parametrize("mask", [1, 2, 4, 7, 3, 5, 6])
def test_site_masks_on_one_map(capi, mask):
    c = class_map(70, 45, 3)                                               # 70: the last packed word holds 6 cells, the last site word 6
    _, _, n = hook_equals(capi, c, mask, 12, 1)
    assert n == sum(int((c == k).sum()) for k in range(3) if mask >> k & 1)
    # class 3 (both bits) is no class of the map: no mask makes it a site
    c3 = c.copy(); c3[c3 == 0] = 3
    H3, _ = capi.debug_hough(c3, mask, 12, 1)
    assert int(H3[0].sum()) == sum(int((c3 == k).sum()) for k in (1, 2) if mask >> k & 1)


@pytest.mark.parametrize("q", QS)
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("w,h", SHAPES)
def test_shapes(capi, w, h, T, q):
    c = class_map(w, h, 17)
    c[0, 0] = c[h - 1, w - 1] = c[0, w - 1] = c[h - 1, 0] = 1
    for mask in (2, 1):                                                    # (bit 0: the row's padding and the cells right of M are no sites)
        hook_equals(capi, c, mask, T, q)


def test_hook_refusals(capi):
    c = np.ones((4, 5), np.uint8); H = np.zeros(1 << 16, np.uint32); S = np.zeros(2048, np.uint64)
    L = capi.lib()

    def rc(cw=5, ch=4, mask=2, T=8, q=0):
        return L.slamhip_debug_hough(c.ctypes.data, cw, ch, mask, T, q, H.ctypes.data, S.ctypes.data)
    assert rc() == 0
    for kw in ({"mask": 0}, {"mask": 8}, {"T": 6}, {"T": 0}, {"T": 1028}, {"q": -1}, {"q": 4}, {"cw": 0}, {"ch": 0}, {"cw": 16385}):
        assert rc(**kw) == capi.ERR_INVALID, kw
    assert L.slamhip_debug_hough(c.ctypes.data, 16384, 16384, 2, 1024, 0, H.ctypes.data, S.ctypes.data) == capi.ERR_INVALID   # T N > 2^24


# ---- the two wrong copies ----------------------------------------------------------------------------------------------------------
def test_wrong_copy_late_offset_fails_a_named_case(capi):
    """w + h = 7 and q = 1: the site (1, 0) at k = 0 has the argument 16384 + 7 * 16384 = 8 * 16384 -> bin 4; without the offset under
    the shift, 16384 >> 15 = 0 and 7 >> 1 = 3 -> bin 3.  At q = 0 the two rules agree everywhere."""
    c = np.zeros((3, 4), np.uint8); c[0, 1] = 1
    H, _ = capi.debug_hough(c, 2, 4, 1)
    right, _, _ = np_hough(c, 2, 4, 1); wrong, _, _ = np_hough(c, 2, 4, 1, late_offset=True)
    assert np.nonzero(right[0])[0].tolist() == [4] and np.nonzero(wrong[0])[0].tolist() == [3]
    assert np.array_equal(H, right) and not np.array_equal(H, wrong)
    r0, _, _ = np_hough(class_map(33, 20, 1), 2, 12, 0); w0, _, _ = np_hough(class_map(33, 20, 1), 2, 12, 0, late_offset=True)
    assert np.array_equal(r0, w0)


def test_wrong_copy_flip_fails_a_named_case(capi):
    Nd, Ns, pa, pb = 11, 7, 6, 2
    A = np.zeros(Nd, np.uint32); B = np.zeros(Ns, np.uint32); A[pa] = 3; B[pb] = 5
    xc, rec = capi.debug_hough_xcorr(A, B, 1)
    right = np_xcorr(A, B, 1); wrong = np_xcorr(A, B, 1, wrong_flip=True)
    assert right[1][0] == pa - (Ns - 1 - pb) and wrong[1][0] == pa - (Ns - pb)
    assert rec_tuple(rec) == right[1] == (pa - (Ns - 1 - pb), 1, 15, 15) and np.array_equal(xc, right[0]) and not np.array_equal(xc, wrong[0])


# ---- the row correlation -----------------------------------------------------------------------------------------------------------
def xcorr_equals(capi, A, B, flip):
    xc, rec = capi.debug_hough_xcorr(A, B, flip)
    wxc, wrec = np_xcorr(A, B, flip)
    assert xc.dtype == np.uint64 and np.array_equal(xc, wxc) and rec_tuple(rec) == wrec, (len(A), len(B), flip, rec_tuple(rec), wrec)
    assert wrec[3] == int(np.asarray(A, np.uint64).sum()) * int(np.asarray(B, np.uint64).sum())
    return wrec


@pytest.mark.parametrize("flip", [0, 1])
def test_single_bins_and_extreme_shifts(capi, flip):
    for Nd, Ns in ((9, 9), (12, 5), (5, 12), (1, 1), (1, 6), (6, 1)):
        for pa, pb in ((Nd // 2, Ns // 2), (0, Ns - 1), (Nd - 1, 0), (0, 0), (Nd - 1, Ns - 1)):
            A = np.zeros(Nd, np.uint32); B = np.zeros(Ns, np.uint32); A[pa] = 7; B[pb] = 11
            want = pa - (Ns - 1 - pb) if flip else pa - pb
            assert xcorr_equals(capi, A, B, flip) == (want, 1, 77, 77), (Nd, Ns, pa, pb)
    # both extreme shifts: d = -(Ns - 1) and d = Nd - 1
    A = np.zeros(8, np.uint32); B = np.zeros(5, np.uint32); A[0] = 1; B[0 if flip else 4] = 1
    assert xcorr_equals(capi, A, B, flip)[0] == -4
    A[:] = 0; B[:] = 0; A[7] = 1; B[4 if flip else 0] = 1
    assert xcorr_equals(capi, A, B, flip)[0] == 7


def test_ties_and_zero(capi):
    A = np.zeros(20, np.uint32); B = np.zeros(6, np.uint32)
    A[4] = A[13] = 9; B[2] = 2
    assert xcorr_equals(capi, A, B, 0) == (2, 2, 18, 36)                   # two equal peaks: the smaller d, n_ties = 2
    assert xcorr_equals(capi, A, B, 1) == (4 - 3, 2, 18, 36)
    for Nd, Ns in ((20, 6), (1, 1), (3, 9)):
        z = xcorr_equals(capi, np.zeros(Nd, np.uint32), np.zeros(Ns, np.uint32), 0)
        assert z == (-(Ns - 1), Nd + Ns - 1, 0, 0)
    assert xcorr_equals(capi, A, np.zeros(6, np.uint32), 1) == (-5, 25, 0, 0)


def test_random_rows_and_large_entries(capi):
    rng = np.random.default_rng(5)
    for Nd, Ns in ((64, 64), (257, 100), (100, 257), (513, 1)):
        for flip in (0, 1):
            A = (rng.integers(0, 50, Nd) * (rng.random(Nd) < 0.3)).astype(np.uint32)
            B = (rng.integers(0, 50, Ns) * (rng.random(Ns) < 0.3)).astype(np.uint32)
            xcorr_equals(capi, A, B, flip)
    A = np.full(300, (1 << 19) - 1, np.uint32); B = np.full(300, (1 << 19) - 1, np.uint32)   # step 2's bound on an entry: sums of 2^46
    assert xcorr_equals(capi, A, B, 0)[2] == 300 * ((1 << 19) - 1) ** 2


def test_pair_wraps(capi):
    """kk wrapping 0, 1 and 2 times: f toggles per addition."""
    T = 12
    assert np_pair(T, 3, 7) == (4, 0, 0) and np_pair(T, 7, 3) == (8, 1, 1) and np_pair(T, 12, 0) == (0, 1, 1)
    assert np_pair(T, 23, 0) == (1, 0, 2) and np_pair(T, 13, 0) == (11, 0, 2) and np_pair(T, 12, 11) == (11, 1, 1) and np_pair(T, 0, 0) == (0, 0, 0)
    got = {np_pair(T, m, k)[2] for m in range(2 * T) for k in range(T)}
    assert got == {0, 1, 2}


def pairs_case():
    """A destination and a source map, T, q and pairs whose kk wraps 0, 1 and 2 times -- shared with the GPU file."""
    d = class_map(70, 45, 21, (0.7, 0.08, 0.22)); s = class_map(52, 61, 22, (0.7, 0.08, 0.22))
    T = 12
    pairs = np.array([[0, 0], [3, 7], [7, 3], [12, 0], [23, 0], [13, 0], [12, 11], [5, 5], [18, 6], [23, 11]], np.int32)
    return d, s, T, pairs


def np_shifts(Hd, Hs, T, pairs):
    out = []
    for m, k in np.asarray(pairs).tolist():
        kk, f, _ = np_pair(T, m, k)
        out.append(np_xcorr(Hd[k], Hs[kk], f))
    return out


@pytest.mark.parametrize("q", [0, 1])
def test_pairs_of_two_maps(capi, q):
    d, s, T, pairs = pairs_case()
    Hd, _, nd = np_hough(d, 2, T, q); Hs, _, ns = np_hough(s, 2, T, q)
    assert Hd.shape[1] != Hs.shape[1]                                      # N_d != N_s
    assert {np_pair(T, m, k)[2] for m, k in pairs.tolist()} == {0, 1, 2}
    for (m, k), (wxc, wrec) in zip(pairs.tolist(), np_shifts(Hd, Hs, T, pairs)):
        kk, f, _ = np_pair(T, m, k)
        xc, rec = capi.debug_hough_xcorr(Hd[k], Hs[kk], f)
        assert np.array_equal(xc, wxc) and rec_tuple(rec) == wrec and wrec[3] == nd * ns, (m, k)


# ---- rotation scores ---------------------------------------------------------------------------------------------------------------
def test_rotation_scores(capi):
    rng = np.random.default_rng(9)
    T = 36
    small = rng.integers(1, 1 << 20, T).astype(np.uint64)                  # sh = 0
    big = (rng.integers(1, 1 << 30, T).astype(np.uint64) << np.uint64(17)) | np.uint64(0x1FFFF)   # up to 2^47: sh = 21 or so
    edge = np.full(T, (1 << 26) - 1, np.uint64); edge2 = edge.copy(); edge2[5] = 1 << 26            # sh 0 and 1, on both sides of 2^26
    for a, b in ((small, small[::-1].copy()), (big, small), (small, big), (big, big[::-1].copy()), (edge, edge2), (edge2, edge)):
        cc, sa, sb = np_rotation(a, b)
        assert np.array_equal(capi.debug_hough_rotation(a, b), cc), (sa, sb)
    assert np_rotation(small, big)[1:] == (0, 21) and np_rotation(edge, edge2)[1:] == (0, 1)
    # a source spectrum that is a circular shift of the destination's by m0 peaks at m0: HS_s[k - m0] = HS_d[k]
    for hd in (small, big):
        for m0 in (0, 1, 17, T - 1):
            hs = np.roll(hd, -m0)
            cc = capi.debug_hough_rotation(hd, hs)
            assert int(np.argmax(cc)) == m0 and np.count_nonzero(cc == cc.max()) == 1, m0
    for T_bad in (6, 0, 1028):
        assert capi.lib().slamhip_debug_hough_rotation(small.ctypes.data, small.ctypes.data, T_bad, small.ctypes.data) == capi.ERR_INVALID


def test_peaks(capi):
    assert capi.hough_peaks([1, 5, 5, 2, 9, 3], 4) == [4, 1]               # > the left, >= the right: a plateau's first cell
    assert capi.hough_peaks([7, 7, 7, 7], 4) == [0]                        # none: m = 0
    assert capi.hough_peaks([9, 1, 1, 8], 4) == [0]                        # circular: 9 > 8; 8 is not >= 9
    assert capi.hough_peaks([3, 1, 3, 1], 1) == [0] and capi.hough_peaks([3, 1, 3, 1], 4) == [0, 2]


# ---- end to end on the CPU ---------------------------------------------------------------------------------------------------------
W, H = 160, 120
CELL = 0.5                                                                 # metres per cell: stm = 2
SRC = 224                                                                  # the source array is SRC x SRC cells
OCC, FREE = F(1.5), F(-0.7)
CASES = [(0.0, (31.0, -22.0)), (0.3, (-40.0, 25.0)), (math.pi / 2 + 0.2, (55.0, 38.0)), (-2.5, (-27.0, -61.0))]   # theta, t in cells


def synthetic_map():
    """160 x 120 cells: an outer room and inner rooms of axis-aligned walls 2 cells thick, doorways, and ONE oblique wall, so that
    the spectrum is not symmetric under a quarter turn; free inside, unknown outside."""
    v = np.zeros((H, W), F)
    v[12:108, 10:150] = FREE
    for y0, y1, x0, x1 in ((12, 14, 10, 150), (106, 108, 10, 150), (12, 108, 10, 12), (12, 108, 148, 150),        # the outer room
                           (12, 70, 60, 62), (68, 70, 10, 40), (68, 70, 50, 62), (50, 108, 110, 112), (50, 52, 112, 135)):
        v[y0:y1, x0:x1] = OCC
    for s in range(46):                                                    # the oblique wall, about 27 degrees
        x, y = 66 + s, 100 - s // 2
        v[y:y + 2, x:x + 2] = OCC
    return v


def cells_of(capi, values):
    c = np.zeros(values.shape, capi.CELL_DTYPE)
    c["value"] = values; c["update_index"] = -1
    return c


def synthetic_case(capi, theta, t):
    """The map resampled as a source by K14's step 2 (slamhip_debug_merge, REPLACE into an empty SRC x SRC array) such that the source
    frame lies at pose (t, theta) in the map's frame: destination = R(theta) source + t in cells.  The source array's first cell
    (ax, ay) is chosen so that the map's centre falls on the array's.  -> (dst cells, src cells, ax, ay, the true pose in metres)."""
    stm = 1.0 / CELL
    dst = cells_of(capi, synthetic_map())
    c, s = math.cos(theta), math.sin(theta)
    inv = lambda x, y: (c * x + s * y, -s * x + c * y)                     # R(-theta)
    mx, my = inv(W / 2 - t[0], H / 2 - t[1])
    ax, ay = int(round(mx - SRC / 2)), int(round(my - SRC / 2))
    qx, qy = inv(-t[0], -t[1])
    q = ((qx - ax) / stm, (qy - ay) / stm, -theta)                         # array = R(-theta) map + q: the pose of the MAP in the array's frame
    src, rep = capi.debug_merge(cells_of(capi, np.zeros((SRC, SRC), F)), dst, 0, 0, q, stm, capi.MERGE_REPLACE, 50.0)
    assert int(rep["joint"][1]) > 600 and int(rep["n_unsourced"]) > 0      # the walls arrived; the array is larger than the map
    return dst, src, ax, ay, (t[0] / stm, t[1] / stm, theta)


def np_class_of(values):
    return np.where(values > 0, 1, np.where(values < 0, 2, 0)).astype(np.uint8)


def cpu_align(capi, dst, src, ax, ay, T, q, n_rot=4, site_mask=2):
    """HectorSLAMProcessor.AlignMaps' composition (capi.align_maps) with the restatement, the hooks and slamhip_debug_merge standing
    in for the device; restatement and hooks are held to == on the way."""
    stm = 1.0 / CELL
    cd, cs = np_class_of(dst["value"]), np_class_of(src["value"])
    Hd, hs_d, nd = np_hough(cd, site_mask, T, q); Hs, hs_s, ns = np_hough(cs, site_mask, T, q)
    for c_, H_, S_ in ((cd, Hd, hs_d), (cs, Hs, hs_s)):
        gH, gS = capi.debug_hough(c_, site_mask, T, q)
        assert np.array_equal(gH, H_) and np.array_equal(gS, S_)
    info = lambda c_, x0, y0, n: dict(zip(("w", "h", "x0", "y0", "D", "N", "n_sites"), (c_.shape[1], c_.shape[0], x0, y0) + np_bins(c_.shape[1], c_.shape[0], q) + (n,)))

    def rotation():
        cc = np_rotation(hs_d, hs_s)[0]
        assert np.array_equal(cc, capi.debug_hough_rotation(hs_d, hs_s))
        return cc

    def shifts(pairs):
        out = np.zeros(len(pairs), capi.HOUGH_SHIFT)
        for i, ((m, k), (_, wrec)) in enumerate(zip(pairs.tolist(), np_shifts(Hd, Hs, T, pairs))):
            kk, f, _ = np_pair(T, m, k)
            out[i] = capi.debug_hough_xcorr(Hd[k], Hs[kk], f)[1]
            assert rec_tuple(out[i]) == wrec
        return out

    def score(poses):
        return np.array([capi.debug_merge(dst, src, ax, ay, p, stm, capi.MERGE_ADD, 50.0)[1] for p in poses], capi.MERGE_REPORT)
    return capi.align_maps(T, q, n_rot, hs_d, hs_s, info(cd, 0, 0, nd), info(cs, ax, ay, ns), stm, rotation, shifts, score)


def pose_errors(pose, truth):
    stm = 1.0 / CELL
    dth = abs(math.remainder(float(pose[2]) - truth[2], 2 * math.pi))
    return dth, math.hypot((float(pose[0]) - truth[0]) * stm, (float(pose[1]) - truth[1]) * stm)


@pytest.mark.parametrize("q", [0, 1])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_align_end_to_end(capi, case, q):
    """The composition's FIRST hypothesis lies within pi / T of theta and within 2^q + 2 cells of t, at T = 360.  The bound is the
    issue's condition, not a measurement.  Two candidate maps were tried, each with the four transforms of CASES at q = 0 and 1:
    this one, and the same rooms with walls ONE cell thick.  Both meet the bound in all eight runs (largest errors: 0.0080 rad and
    1.44 cells here, 0.0054 rad and 1.11 cells with thin walls), so none had to be dropped; the thick walls are kept because under a
    rotation the nearest-neighbour resampling breaks a thin wall into steps and the occupied-on-occupied counts that rank the
    hypotheses fall to a few hundred (196 against 158 for the runner-up in the worst run, 881 against 627 here).  No other transforms
    were tried.  The figures are printed before the assertion."""
    theta, t = CASES[case]
    T = 360
    dst, src, ax, ay, truth = synthetic_case(capi, theta, t)
    hyp = cpu_align(capi, dst, src, ax, ay, T, q)
    assert 2 <= len(hyp) <= 8 and all(int(a["report"]["joint"][4]) >= int(b["report"]["joint"][4]) for a, b in zip(hyp, hyp[1:]))
    dth, dt = pose_errors(hyp[0]["pose"], truth)
    print("case %d q %d: m = %d, pose %s, truth %s, |dtheta| = %.5f rad (bound %.5f), |dt| = %.3f cells (bound %d), joint[4] = %s"
          % (case, q, hyp[0]["m"], hyp[0]["pose"].tolist(), truth, dth, math.pi / T, dt, (1 << q) + 2, [int(h["report"]["joint"][4]) for h in hyp]))
    assert dth <= math.pi / T and dt <= (1 << q) + 2
