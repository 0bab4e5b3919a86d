"""The branch-and-bound pose-lattice search (K24, slamhip_bnb_spec in include/slamhip.h): a NumPy restatement of rules 2 - 6, written
from the rules and not from the C, and the catalogue of cases that tests/test_hs_bnb_abi.py (host hook, no GPU) and
tests/test_gpu_hector_bnb.py (device) share.

The restatement forms P_h by sliding maxima over an explicitly zero-padded class array -- 2^h - 1 shifted copies per axis, no
doubling, no packed words -- and takes its point cells from test_hs_lattice_abi.np_point_cells.  Three deliberately wrong copies of
it (np_bnb's keyword arguments) show that the catalogue can tell the rules from their nearest mistakes."""
import numpy as np

import test_hs_lattice_abi as A

F = np.float32
EMPTY_KEY = 0x80000000FFFFFFFF
INFO_FIELDS = ("top", "n_levels", "evaluated", "blocks", "kept")


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def np_pooled(cls, top, short_window=False, outside=0):
    """-> (maps, m): maps[h][y + m, x + m] = P_h(x, y) for -m <= x < w + m, -m <= y < h + m, m = 2^top; P_h is `outside` beyond.
    short_window (a wrong copy): windows of 2^h - 1 cells.  outside = -1 (a wrong copy): cells outside the map count as free."""
    m = 1 << top
    base = np.full((cls.shape[0] + 2 * m, cls.shape[1] + 2 * m), outside, np.int8)
    base[m:m + cls.shape[0], m:m + cls.shape[1]] = cls
    maps = [base]
    for h in range(1, top + 1):
        s = (1 << h) - (1 if short_window else 0)
        rows = base.copy()
        for u in range(1, s):                                              # max over x .. x + s - 1 (a window cut by the array's end holds padding only)
            np.maximum(rows[:, :-u], base[:, u:], out=rows[:, :-u])
        both = rows.copy()
        for v in range(1, s):
            np.maximum(both[:-v, :], rows[v:, :], out=both[:-v, :])
        maps.append(both)
    return maps, m


def np_lookup(P, m, outside, X, Y):
    ok = (X >= -m) & (X < P.shape[1] - m) & (Y >= -m) & (Y < P.shape[0] - m)
    vals = P[np.clip(Y + m, 0, P.shape[0] - 1), np.clip(X + m, 0, P.shape[1] - 1)]
    return np.where(ok, vals, outside).sum(axis=1, dtype=np.int64)


def np_key(score, flat):
    return ((int(score) & 0xFFFFFFFF) ^ 0x80000000) << 32 | (0xFFFFFFFF - int(flat))


def np_bnb(values, w, h, cell, centre, nx, ny, n_theta, dtheta, top, xy, max_blocks=0, strict=False, short_window=False, outside=0):
    """Rules 2 - 6 -> (keys (n_theta,) uint64, info dict), or None where rule 5 ends the search.  strict, short_window, outside: the
    three wrong copies (survive on U > best; windows of 2^h - 1 cells; outside the map taken as free when bounding)."""
    cap = max_blocks or 1 << 26
    cls = A.np_classes(values, w, h).astype(np.int8)
    exact, m = np_pooled(cls, top)
    pooled = exact if not (short_window or outside) else np_pooled(cls, top, short_window, outside)[0]
    stm = F(1.0) / F(cell)
    NX = 2 * nx + 1
    s = 1 << top
    ga, gb = np.meshgrid(np.arange(0, NX, s), np.arange(0, 2 * ny + 1, s))
    fronts = [(ga.ravel().astype(np.int64), gb.ravel().astype(np.int64)) for _ in range(n_theta)]
    cells = []
    for k in range(n_theta):
        gx, gy, valid = A.np_point_cells(stm, centre, A.np_theta(centre, k, dtheta), xy)
        cells.append((gx[valid], gy[valid]))
    keys = [0] * n_theta
    blocks, kept = [0] * 9, [0] * 9
    for lvl in range(top, -1, -1):
        blocks[lvl] = sum(len(a) for a, _ in fronts)
        if blocks[lvl] > cap:
            return None                                                    # rule 5 (rule 1 at the top)
        Us = []
        for k, (a, b) in enumerate(fronts):
            gx, gy = cells[k]
            U = np.zeros(len(a), np.int64); E = np.zeros(len(a), np.int64)
            for i in range(0, len(a), 4096):                               # (blocks x points, in slices)
                X = gx[None, :] + (a[i:i + 4096] - nx)[:, None]
                Y = gy[None, :] + (b[i:i + 4096] - ny)[:, None]
                E[i:i + 4096] = np_lookup(exact[0], m, 0, X, Y)
                U[i:i + 4096] = np_lookup(pooled[lvl], m, outside, X, Y) if lvl else E[i:i + 4096]
            Us.append(U)
            if len(a):
                keys[k] = max(keys[k], max(np_key(e, bb * NX + aa) for e, aa, bb in zip(E, a, b)))
        if lvl == 0:
            break
        d = 1 << (lvl - 1)
        nxt = []
        for k, (a, b) in enumerate(fronts):
            best = (keys[k] >> 32) ^ 0x80000000                            # the score in key[k] ...
            best -= (best >> 31) << 32                                     # ... signed
            live = (Us[k] > best) if strict else (Us[k] >= best)
            kept[lvl] += int(live.sum())
            a, b = a[live], b[live]
            ca = np.concatenate([a, a + d, a, a + d]); cb = np.concatenate([b, b, b + d, b + d])
            ok = (ca <= 2 * nx) & (cb <= 2 * ny)
            nxt.append((ca[ok], cb[ok]))
        fronts = nxt
    info = dict(top=top, n_levels=top + 1, evaluated=sum(blocks), blocks=blocks, kept=kept)
    return np.array(keys, np.uint64), info


def info_dict(rec):
    """A capi.BNB_INFO record as np_bnb's dict."""
    return dict(top=int(rec["top"]), n_levels=int(rec["n_levels"]), evaluated=int(rec["evaluated"]),
                blocks=[int(v) for v in rec["blocks"]], kept=[int(v) for v in rec["kept"]])


# ---- the maps ----------------------------------------------------------------------------------------------------------------------
def class_values(rng, n):
    """Cell values drawn from {positive, negative, +0, -0, NaN} (test_gpu_hector_lattice.class_values, same draws)."""
    pick = rng.integers(0, 5, n)
    mag = rng.uniform(0.1, 3.0, n).astype(np.float32)
    return np.select([pick == 0, pick == 1, pick == 2, pick == 3], [mag, -mag, F(0.0), F(-0.0)], F(np.nan)).astype(np.float32)


def small_points(rng, n):
    xy = np.stack([rng.uniform(-1.0, 7.0, n), rng.uniform(-1.0, 4.0, n)], 1).astype(np.float32)
    xy[3] = (np.nan, 0.5)
    xy[11] = (1.0e6, -2.0e6)                                               # far away: off every map, still a valid point
    return xy


def peak_values(w, h, cell, centre, nx, ny, dtheta, xy, node):
    """Every cell free, except the end cells of the scan at lattice node (k, ix, iy), which are occupied."""
    k, ix, iy = node
    v = np.full((h, w), -1.0, np.float32)
    gx, gy, ok = A.np_point_cells(F(1.0) / F(cell), centre, A.np_theta(centre, k, dtheta), xy)
    x, y = gx[ok] + ix, gy[ok] + iy
    inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
    v[y[inside], x[inside]] = 1.0
    return v.ravel(), int(inside.sum())


_MAPS = {}


def map_of(name):
    """-> dict(cell0, dims (w0, h0), levels, values [per level]): what a test uploads, or hands to the hook level by level."""
    if name not in _MAPS:
        if name == "small":                                                # test_gpu_hector_lattice's: 80 x 48 of 0.1 m, 2 levels, level 1 a row of 2.5 words
            rng = np.random.default_rng(7)
            _MAPS[name] = dict(cell0=0.1, dims=(80, 48), levels=2, values=[class_values(rng, 80 * 48), class_values(rng, 40 * 24)])
        elif name == "empty":
            _MAPS[name] = dict(cell0=0.1, dims=(80, 48), levels=2, values=[np.zeros(80 * 48, np.float32), np.zeros(40 * 24, np.float32)])
        elif name == "peak":
            c = CASES["one_peak"]
            v, n_in = peak_values(80, 48, 0.1, c["centre"], c["nx"], c["ny"], c["dtheta"], c["xy"], PEAK_NODE)
            assert n_in > 40
            _MAPS[name] = dict(cell0=0.1, dims=(80, 48), levels=2, values=[v, np.zeros(40 * 24, np.float32)])
        elif name == "big":                                                # one level of 1024 x 1024
            _MAPS[name] = dict(cell0=0.05, dims=(1024, 1024), levels=1, values=[class_values(np.random.default_rng(23), 1024 * 1024)])
        else:
            raise KeyError(name)
    return _MAPS[name]


def level_of(case):
    """-> (values, w, h, cell) of the level a case searches."""
    mp = map_of(case["map"])
    l = case["level"]
    w, h = mp["dims"][0] >> l, mp["dims"][1] >> l
    return mp["values"][l], w, h, F(F(mp["cell0"]) * F(1 << l))


# ---- the catalogue -----------------------------------------------------------------------------------------------------------------
CORNER = np.array([0.27, 0.13, 0.3], np.float32)                            # near the map's corner: nodes fall off on two sides
PEAK_NODE = (1, 4, -4)                                                      # (k, ix, iy): ix + nx = 12, iy + ny = 4 -- an origin at every height up to 2


def _case(map, level, centre, nx, ny, n_theta, dtheta, top, xy):
    return dict(map=map, level=level, centre=np.asarray(centre, np.float32), nx=nx, ny=ny, n_theta=n_theta, dtheta=F(dtheta), top=top, xy=xy)


def _big_points():
    rng = np.random.default_rng(23)
    rng.random(1024 * 1024 * 3)                                            # (past the draws of the map's values)
    xy = rng.uniform(-22.5, 22.5, (200, 2)).astype(np.float32)
    xy[5] = (np.nan, np.nan)
    xy[6] = (27.0, 0.0)                                                    # off the map at some headings
    return xy


_P97 = small_points(np.random.default_rng(11), 97)
CASES = {
    # the 11 x 7 x 7 lattice at the corner
    "corner_top2": _case("small", 0, CORNER, 5, 3, 7, 0.4, 2, _P97),        # blocks of 4 that divide neither 11 nor 7
    "corner_top2_l1": _case("small", 1, CORNER, 5, 3, 7, 0.4, 2, _P97),     # rows of 2.5 packed words
    "corner_top0": _case("small", 1, CORNER, 5, 3, 7, 0.4, 0, _P97),        # every node a block, nothing pooled
    "corner_top4": _case("small", 0, CORNER, 5, 3, 7, 0.4, 4, _P97),        # one block per heading
    "empty": _case("empty", 0, (2.0, 2.0, 0.0), 5, 3, 7, 0.4, 2, _P97),     # all scores tie: nothing may be pruned
    "one_peak": _case("peak", 0, (0.3, 0.3, -0.05), 8, 8, 7, 0.05, 2, _P97),   # must prune
    "many_points": _case("small", 0, (0.9, 0.4, -1.0), 1, 1, 2, 2.0, 1, small_points(np.random.default_rng(13), 5000)),   # several LDS chunks
    "big_level": _case("big", 0, (25.6, 25.6, -0.2), 20, 20, 4, 0.9, 5, _big_points()),   # windows of 32 cross many words and rows
    "wide": _case("small", 0, (4.0, 2.4, 0.2), 128, 128, 4, 0.7, 5, _P97),  # 257 x 257 x 4: lower frontiers of more than one workgroup per heading
}


def nodes_of(case):
    return (2 * case["nx"] + 1) * (2 * case["ny"] + 1) * case["n_theta"]


_REF = {}


def reference(name):
    """np_bnb of a case, computed once."""
    if name not in _REF:
        c = CASES[name]
        values, w, h, cell = level_of(c)
        _REF[name] = np_bnb(values, w, h, cell, c["centre"], c["nx"], c["ny"], c["n_theta"], c["dtheta"], c["top"], c["xy"])
    return _REF[name]


_VOL = {}


def exhaustive_keys(name):
    """np_keys(np_volume(...)) of a case -- K7's definition -- computed once."""
    if name not in _VOL:
        c = CASES[name]
        values, w, h, cell = level_of(c)
        _VOL[name] = A.np_keys(A.np_volume(values, w, h, cell, c["centre"], c["nx"], c["ny"], c["n_theta"], c["dtheta"], c["xy"]))
    return _VOL[name]
