"""CPU-side checks of the frontier clusters' interface (slamhip_hs_frontiers, slamhip_hsproc_frontiers, slamhip_debug_frontiers) and
the NumPy restatement of their definition (include/slamhip.h, slamhip_hs_frontiers, steps 2 - 7) that
tests/test_gpu_hector_frontier.py compares the device with.

The restatement: the frontier mask from four shifted comparisons on a class array padded with zeros, the components from a plain
Python flood fill over the eight neighbours in row-major order (so a component's first cell is its seed), the records and their
order from np.lexsort.  It shares nothing with hs_frontier.h, whose text -- frontier words, runs by ctz / clz, a union-find over run
starts -- the library's hook runs.  Everything is compared with == on integers.  No compute calls on a device."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("slamhip_hs_frontiers", "slamhip_hsproc_frontiers", "slamhip_debug_frontiers")
CLUSTER = np.dtype([("seed_x", np.int32), ("seed_y", np.int32), ("n_cells", np.int32), ("n_runs", np.int32), ("x_min", np.int32),
                    ("y_min", np.int32), ("x_max", np.int32), ("y_max", np.int32), ("sum_x", np.int64), ("sum_y", np.int64)])
SUMMARY = np.dtype([(n, np.int32) for n in ("mx0", "my0", "mw", "mh", "n_frontier_cells", "n_runs", "n_clusters", "n_kept", "n_returned",
                                            "kept_cells")])
MAX_CLUSTERS = 65536
SHAPES = [(80, 48), (40, 24), (33, 5), (32, 1), (1, 32), (97, 31)]         # (w, h): both sides of the 16-cell packed word and the 32-cell frontier word


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def np_frontier_mask(cls):
    """Step 2: free, and one of the four edge neighbours of class 0; everything outside the array is class 0."""
    c = np.pad(np.asarray(cls).astype(np.int64) & 3, 1)
    unknown = c == 0
    near = unknown[1:-1, :-2] | unknown[1:-1, 2:] | unknown[:-2, 1:-1] | unknown[2:, 1:-1]
    return (c[1:-1, 1:-1] == 2) & near


def np_labels(mask):
    """Step 3: the label of every frontier cell, -1 elsewhere.  The cells are visited in row-major order, so the first cell of a
    component that the flood fill meets is its seed."""
    h, w = mask.shape
    lab = np.full((h, w), -1, np.int64)
    m = mask.tolist()
    out = lab.tolist()
    for y in range(h):
        for x in range(w):
            if not m[y][x] or out[y][x] >= 0:
                continue
            seed = y * w + x
            out[y][x] = seed
            stack = [(x, y)]
            while stack:
                cx, cy = stack.pop()
                for ny in (cy - 1, cy, cy + 1):
                    if ny < 0 or ny >= h:
                        continue
                    for nx in (cx - 1, cx, cx + 1):
                        if 0 <= nx < w and m[ny][nx] and out[ny][nx] < 0:
                            out[ny][nx] = seed
                            stack.append((nx, ny))
    return np.array(out, np.int64).reshape(h, w)


def np_frontiers(cls, min_cells, max_clusters, x0=0, y0=0):
    """Steps 2 - 7 for M = (x0, y0, w, h) holding `cls` -> (summary, records, labels): a SUMMARY record, the returned CLUSTER records in
    window-frame cells, the (h, w) label array."""
    mask = np_frontier_mask(cls)
    h, w = mask.shape
    lab = np_labels(mask)
    starts = mask & ~np.pad(mask, ((0, 0), (1, 0)))[:, :-1]                # step 4: a frontier cell whose left neighbour is none
    ys, xs = np.nonzero(mask)
    l = lab[ys, xs]
    labels, inv, n_cells = np.unique(l, return_inverse=True, return_counts=True)
    k = labels.shape[0]
    rec = np.zeros(k, CLUSTER)
    if k:
        rec["seed_x"] = labels % w + x0; rec["seed_y"] = labels // w + y0
        rec["n_cells"] = n_cells
        rec["n_runs"] = np.bincount(inv, weights=starts[ys, xs], minlength=k).astype(np.int64)
        for name, src, fn, off in (("x_min", xs, np.minimum, x0), ("x_max", xs, np.maximum, x0), ("y_min", ys, np.minimum, y0),
                                   ("y_max", ys, np.maximum, y0)):
            acc = np.full(k, (1 << 40) if fn is np.minimum else -(1 << 40), np.int64)
            fn.at(acc, inv, src)
            rec[name] = acc + off
        rec["sum_x"] = np.bincount(inv, weights=xs + x0, minlength=k).astype(np.int64)   # (far below 2^53: exact)
        rec["sum_y"] = np.bincount(inv, weights=ys + y0, minlength=k).astype(np.int64)
    kept = rec[rec["n_cells"] >= min_cells]
    kl = labels[rec["n_cells"] >= min_cells]
    kept = kept[np.lexsort((kl, -kept["n_cells"].astype(np.int64)))]       # step 6: n_cells descending, equal sizes by label ascending
    n_ret = min(kept.shape[0], max_clusters)
    s = np.zeros(1, SUMMARY)[0]
    for name, v in zip(SUMMARY.names, (x0, y0, w, h, int(mask.sum()), int(starts.sum()), k, kept.shape[0], n_ret, int(kept["n_cells"].sum()))):
        s[name] = v
    return s, kept[:n_ret].copy(), lab.astype(np.int32)


def check(got, want, what=None):
    """A call's (summary, clusters[, labels]) against the restatement's, field by field."""
    assert got[0].dtype == SUMMARY and got[0] == want[0], (what, got[0], want[0])
    assert got[1].dtype == CLUSTER and got[1].shape == want[1].shape, (what, got[1].shape, want[1].shape)
    assert np.array_equal(got[1], want[1]), (what, [(a, b) for a, b in zip(got[1], want[1]) if a != b][:3])
    if len(got) > 2:
        assert got[2].dtype == np.int32 and np.array_equal(got[2], want[2]), (what, np.argwhere(got[2] != want[2])[:5].tolist())


# ---- the maps of the hand cases, shared with the GPU file (class arrays of (h, w) uint8) -------------------------------------------
def serpentine(w, h):
    """A one-cell-wide free path through unknown space: every even row whole, the odd rows one cell at alternating ends."""
    c = np.zeros((h, w), np.uint8)
    c[0::2] = 2
    for y in range(1, h, 2):
        c[y, w - 1 if (y // 2) % 2 == 0 else 0] = 2
    return c


def comb(w, h):
    """One-cell-wide vertical teeth on every even column, joined only by the last row."""
    c = np.zeros((h, w), np.uint8)
    c[:, 0::2] = 2
    c[h - 1] = 2
    return c


def seam_cases(w, h, bx, y):
    """The three run-seam cases around column bx (a word or workgroup boundary: bx - 1 is the last cell left of it) in rows y, y + 1 of
    an unknown w x h array -> [(name, class array, clusters, runs)]."""
    out = []
    c = np.zeros((h, w), np.uint8); c[y, bx - 3:bx + 4] = 2
    out.append(("a run across the boundary", c, 1, 1))
    c = np.zeros((h, w), np.uint8); c[y, bx - 1] = 2; c[y + 1, bx] = 2
    out.append(("the diagonal pair", c, 1, 2))
    c = np.zeros((h, w), np.uint8); c[y, bx - 1] = 2; c[y + 1, bx + 1] = 2
    out.append(("two cells apart", c, 2, 2))
    return out


def random_classes(rng, h, w):
    """Classes drawn from {0, 1, 2}, free the most frequent so that clusters of many sizes form."""
    return rng.choice(np.array([0, 1, 2], np.uint8), size=(h, w), p=[0.25, 0.15, 0.6])


# ---- the interface -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def capi():
    import slam.net_amd.build as b
    b.build()
    import slam.net_amd.capi as capi
    return capi


def test_surface(capi):
    h = open(os.path.join(ROOT, "include", "slamhip.h")).read()
    native = open(os.path.join(ROOT, "bindings", "csharp", "SlamHip", "SlamHip.Native.cs")).read()
    assert capi.FRONTIER_CLUSTER == CLUSTER and capi.FRONTIER_CLUSTER.itemsize == 48
    assert [CLUSTER.fields[n][1] for n in CLUSTER.names] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 40]   # 8 int32 + 2 int64: no padding
    assert capi.FRONTIER_SUMMARY == SUMMARY and SUMMARY.itemsize == 40
    assert "SLAMHIP_K_COUNT = 10" in h and "#define SLAMHIP_FRONTIER_MAX_CLUSTERS 65536" in h   # no new timing class
    assert capi.FRONTIER_MAX_CLUSTERS == MAX_CLUSTERS
    L = capi.lib()
    for name in SYMBOLS:
        assert hasattr(L, name) and name in L._signatures and name in capi.declared_symbols() and name in native, name
    assert "struct FrontierCluster" in native and "struct FrontierSummary" in native
    assert len(L._signatures["slamhip_hs_frontiers"][1]) == 12 == len(L._signatures["slamhip_hsproc_frontiers"][1])
    assert len(L._signatures["slamhip_debug_frontiers"][1]) == 8
    import slam.net_amd.build as b
    import slam.net_amd.hector as hm
    assert hasattr(hm.MapRepMultiMap, "frontiers") and hasattr(hm.HectorSLAMProcessor, "Frontiers")
    assert "hs_frontier.hip" in b.SOURCES and "hs_frontier.h" in b.HEADERS


# ---- random class arrays -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def arrays():
    rng = np.random.default_rng(10)
    out = {s: random_classes(rng, s[1], s[0]) for s in SHAPES}
    for c in out.values():
        c.setflags(write=False)
    return out


_WANT = {}


def want_of(arrays, shape, min_cells, max_clusters):
    key = (shape, min_cells, max_clusters)
    if key not in _WANT:
        _WANT[key] = np_frontiers(arrays[shape], min_cells, max_clusters)
    return _WANT[key]


@pytest.mark.parametrize("max_clusters", [0, 3, MAX_CLUSTERS])
@pytest.mark.parametrize("min_cells", [1, 2, 5])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_random_arrays(capi, arrays, shape, min_cells, max_clusters):
    want = want_of(arrays, shape, min_cells, max_clusters)
    got = capi.debug_frontiers(arrays[shape], min_cells, max_clusters)
    check(got, want, (shape, min_cells, max_clusters))
    s = got[0]
    assert s["n_returned"] == min(s["n_kept"], max_clusters) and s["n_kept"] <= s["n_clusters"] <= s["n_runs"] <= s["n_frontier_cells"]
    if shape == (80, 48):
        assert s["n_clusters"] > 20 and got[1].shape[0] in (0, 3, s["n_kept"]) and (min_cells == 1) == (s["n_kept"] == s["n_clusters"])
    without = capi.debug_frontiers(arrays[shape], min_cells, max_clusters, labels=False)
    assert len(without) == 2
    check(without, want[:2])


def test_random_arrays_hold_what_they_should(arrays):
    for shape in ((80, 48), (97, 31)):
        assert set(np.unique(arrays[shape]).tolist()) == {0, 1, 2}
        s, rec, _ = np_frontiers(arrays[shape], 1, MAX_CLUSTERS)
        assert (rec["n_cells"] == 1).any() and (rec["n_cells"] >= 5).any() and (rec["n_runs"] > 1).any()
        assert (np.diff(rec["n_cells"]) <= 0).all()


# ---- hand cases, each named for what it can break ----------------------------------------------------------------------------------
W, H = 80, 48


@pytest.mark.parametrize("bx", [16, 32, 64])
def test_run_seams(capi, bx):
    """Cells either side of a word boundary (bx = 32, 64: the frontier word's; 16: the packed word's): a run across it is ONE run, the
    diagonal pair across it is one cluster, two columns apart it is two."""
    for name, c, clusters, runs in seam_cases(W, H, bx, 7):
        got = capi.debug_frontiers(c)
        check(got, np_frontiers(c, 1, 256), name)
        assert (got[0]["n_clusters"], got[0]["n_runs"]) == (clusters, runs), (bx, name)
        assert got[1][0]["seed_y"] == 7 and got[1][0]["seed_x"] == (bx - 3 if runs == 1 else bx - 1)


def test_serpentine(capi):
    for c, seed_runs in ((serpentine(W, H), 48), (serpentine(H, W).T.copy(), None)):
        got = capi.debug_frontiers(c)
        check(got, np_frontiers(c, 1, 256), "serpentine")
        s, r = got[0], got[1]
        assert s["n_clusters"] == 1 and s["n_frontier_cells"] == int((c == 2).sum()) == r[0]["n_cells"]
        assert (r[0]["seed_x"], r[0]["seed_y"]) == (0, 0) and (got[2][c == 2] == 0).all()
        assert (r[0]["x_min"], r[0]["y_min"], r[0]["x_max"], r[0]["y_max"]) == (0, 0, W - 1, H - 1)
        assert seed_runs is None or r[0]["n_runs"] == seed_runs


def test_comb(capi):
    c = comb(W, H)
    got = capi.debug_frontiers(c)
    check(got, np_frontiers(c, 1, 256), "comb")
    assert got[0]["n_clusters"] == 1 and got[0]["n_runs"] == 40 * 47 + 1 == got[1][0]["n_runs"]
    assert got[1][0]["n_cells"] == 40 * 47 + 80 and (got[2][c == 2] == 0).all()


def test_walled_block_has_no_frontier(capi):
    c = np.zeros((H, W), np.uint8)
    c[10:30, 20:60] = 1
    c[11:29, 21:59] = 2
    got = capi.debug_frontiers(c)
    check(got, np_frontiers(c, 1, 256))
    assert got[0]["n_frontier_cells"] == 0 == got[0]["n_clusters"] and (got[2] == -1).all()
    c[10, 40] = 0                                                          # one stone out of the wall: the free cell below it sees the unknown
    got = capi.debug_frontiers(c)
    check(got, np_frontiers(c, 1, 256))
    assert got[0]["n_frontier_cells"] == 1 and got[2][11, 40] == 11 * W + 40


def test_free_array_is_its_border_ring(capi):
    for w, h in ((W, H), (33, 5), (32, 1), (1, 32), (2, 2)):
        c = np.full((h, w), 2, np.uint8)
        got = capi.debug_frontiers(c)
        check(got, np_frontiers(c, 1, 256), (w, h))
        ring = w * h - max(w - 2, 0) * max(h - 2, 0)
        assert got[0]["n_clusters"] == 1 and got[1][0]["n_cells"] == ring == (got[2] == 0).sum()
        assert (got[2][1:-1, 1:-1] == -1).all()


@pytest.mark.parametrize("value", [0, 1])
def test_nothing_free(capi, value):
    c = np.full((H, W), value, np.uint8)
    got = capi.debug_frontiers(c)
    assert tuple(got[0]) == (0, 0, W, H, 0, 0, 0, 0, 0, 0) and got[1].shape == (0,) and (got[2] == -1).all()


def lone_cells(w, h, cells):
    c = np.zeros((h, w), np.uint8)
    for x, y in cells:
        c[y, x] = 2
    return c


def test_ties_come_back_in_label_order(capi):
    cells = [(70, 1), (3, 1), (31, 9), (33, 9), (0, 40), (79, 47)]
    c = lone_cells(W, H, cells)
    c[20, 10:13] = 2                                                       # and one larger: first
    got = capi.debug_frontiers(c)
    check(got, np_frontiers(c, 1, 256))
    lab = got[1]["seed_y"].astype(np.int64) * W + got[1]["seed_x"]
    assert got[1]["n_cells"].tolist() == [3] + [1] * 6 and lab[0] == 20 * W + 10 and (np.diff(lab[1:]) > 0).all()
    assert lab[1:].tolist() == sorted(y * W + x for x, y in cells)


def test_truncation_keeps_n_kept(capi):
    c = lone_cells(W, H, [(2 * i, 2 * (i % 20)) for i in range(40)])
    full = capi.debug_frontiers(c, 1, 256)
    assert full[0]["n_kept"] == 40 == full[0]["n_returned"]
    for m in (0, 1, 39, 40, 41):
        got = capi.debug_frontiers(c, 1, m)
        assert got[0]["n_kept"] == 40 and got[0]["n_returned"] == min(m, 40) and got[0]["kept_cells"] == 40
        assert np.array_equal(got[1], full[1][:m]) and np.array_equal(got[2], full[2])


def test_hook_refuses(capi):
    L = capi.lib()
    cls = np.zeros((4, 6), np.uint8); cls[1, 1] = 2
    s = np.full(1, 77, SUMMARY); rec = np.zeros(4, CLUSTER); rec["n_cells"] = 77
    lab = np.full((4, 6), 77, np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)                             # noqa: E731

    def rc(cw=6, ch=4, min_cells=1, max_clusters=4, clusters=rec):
        return L.slamhip_debug_frontiers(vp(cls), cw, ch, min_cells, max_clusters, vp(s), vp(clusters) if clusters is not None else None, vp(lab))
    for kw in (dict(cw=0), dict(ch=0), dict(cw=-1), dict(cw=8192, ch=4097), dict(min_cells=0), dict(min_cells=-3), dict(max_clusters=-1),
               dict(max_clusters=MAX_CLUSTERS + 1), dict(clusters=None)):
        assert rc(**kw) == capi.ERR_INVALID, kw
        assert L.slamhip_last_error()
    assert (s["mw"] == 77).all() and (rec["n_cells"] == 77).all() and (lab == 77).all()
    assert rc(max_clusters=0, clusters=None) == 0 and s[0]["n_kept"] == 1 and s[0]["n_returned"] == 0 and (rec["n_cells"] == 77).all()
    assert rc() == 0 and s[0]["n_returned"] == 1 and rec[0]["n_cells"] == 1 and lab[1, 1] == 7 and (lab != 77).all()


def test_too_many_kept_clusters(capi):
    """A free cell at every (even x, even y) of 528 x 512: 67 584 isolated clusters.  Kept with min_cells = 1 they exceed the record
    block: refused AFTER the labelling, the summary filled; with min_cells = 2 none is kept and every free cell is its own label."""
    w, h = 528, 512
    c = np.zeros((h, w), np.uint8)
    c[0::2, 0::2] = 2
    L = capi.lib()
    s = np.zeros(1, SUMMARY)
    rc = L.slamhip_debug_frontiers(c.ctypes.data_as(C.c_void_p), w, h, 1, 0, s.ctypes.data_as(C.c_void_p), None, None)
    assert rc == capi.ERR_INVALID and b"67584" in L.slamhip_last_error() and b"min_cells" in L.slamhip_last_error()
    assert tuple(s[0]) == (0, 0, w, h, 67584, 67584, 67584, 67584, 0, 67584)
    got = capi.debug_frontiers(c, 2, 16)
    assert tuple(got[0]) == (0, 0, w, h, 67584, 67584, 67584, 0, 0, 0) and got[1].shape == (0,)
    flat = np.arange(w * h, dtype=np.int32).reshape(h, w)
    assert np.array_equal(got[2], np.where(c == 2, flat, -1))
