"""Case builders for the K4 (Hector scan matcher) edge tests: tests/test_k4_cases_cpu.py checks every case on the CPU (both oracles,
the matcher's rule restated here, and the property the case claims to exercise), tests/test_gpu_match_edges.py runs them on the
device.

A case is one pyramid with cell_len = 1, the cell values of every level (uploaded with SetCells), the pose (tx, ty, 0) with dyadic
tx, ty and a list of scans: `build()` returns Built(size, levels, cells, pose, scans, iters, family, Ts, batch).  The heading is
exactly 0, so Matrix3x2.CreateRotation snaps to the identity, sinRot = 0 and cosRot = 1 / cell length are exact, and a point (x, y)
lies at ((x + tx) / 2^l, (y + ty) / 2^l) on level l.  Cell values are drawn from VALUES only: their probabilities exp(v) / (exp(v) + 1)
are 0.5, 1.0 and 0.0 exactly whatever the expf (0, 50 and -inf: tests/test_gpu_hector_rawparity.py::test_probability_ladder), and NaN
for 100 (expf overflows: inf / inf), which only the NaN-tap cases use.

`geometry()` restates, per level, ScanMatcher.cs:139-180 and :211-249 -- cx, cy, the in-map test of MapProperties.cs:83-87, floor,
the four taps, P, gx, gy and the nine terms plus funVal^2 -- in the arithmetic it is asked for: binary32 with the reference's own
roundings, or binary64.  Two families:
  "exact": every term and every partial sum is exactly representable (the CPU test proves it per case: binary64 and binary32 agree
           term for term, every term is a multiple of 2^-g and the sum of the |terms| lies below 2^(24 - g)), so the binary32 sum is
           the same in EVERY order: the default order (T = 0), every T and the report must equal `expected()` bit for bit;
  "order": fx, fy carry many bits, the binary32 sum depends on the order (the CPU test asserts that the oracle's sums at two T
           differ): compared in the reference order only, against the oracle at T.
"""
import collections
import fractions

import numpy as np

F = np.float32
VALUES = {"half": F(0.0), "one": F(50.0), "zero": F(-np.inf), "nan": F(100.0)}
PROB = {0.0: 0.5, 50.0: 1.0, -np.inf: 0.0, 100.0: np.nan}
LDS_PTS = 2048                         # HS_LDS_PTS (csrc/hs_internal.h)
MAX_T = 64                             # HS_REF_MAX_T
W_SINGLE, W_BATCH = 512 * 3, 256 * 5   # points per pass / window: hs_shape<512>, hs_shape<256> (csrc/hs_match.hip)
WIDE_FROM = 9                          # batches of more than 8 hints run 256 lanes per hint

Case = collections.namedtuple("Case", "name build claims")
Built = collections.namedtuple("Built", "size levels cells pose scans iters family Ts batch")
Geo = collections.namedtuple("Geo", "w h cx cy inmap ix iy idx P gx gy rot terms")
CASES = []


def case(name, *claims):
    def deco(fn):
        CASES.append(Case(name, fn, claims))
        return fn
    return deco


def by_name(name):
    return next(c for c in CASES if c.name == name)


def level_dims(size, levels):
    return [(size[0] >> l, size[1] >> l) for l in range(levels)]       # MapRepMultiMap.cs:40-58


def pts(p):
    return np.array(p, np.float64).reshape(-1, 2).astype(np.float32)


def built(size, levels, cells, pose, scans, iters=None, family="exact", Ts=(1, 3, 64), batch=()):
    scans = [pts(s) for s in scans]
    return Built(size, levels, cells, (float(pose[0]), float(pose[1]), 0.0), scans, list(iters or [1] * levels), family, tuple(Ts), tuple(batch))


def prob_of(values):
    """The probability of every cell, exact on both sides for VALUES."""
    out = np.empty(values.shape, np.float32)
    for v, p in PROB.items():
        out[values == F(v)] = p
    assert np.isin(values, np.array(list(PROB), np.float32)).all()
    return out


def batch_hints(b, B):
    """B distinct dyadic hints around the case's pose: steps of 1/4 (of 4 on a pyramid of several levels: the fractions of every
    level stay what they are), eight to a row."""
    step = 0.25 if b.levels == 1 else 4.0
    return np.array([(b.pose[0] + step * (k % 8), b.pose[1] - step * (k // 8), 0.0) for k in range(B)], np.float32)


# ---- the matcher's rule ----------------------------------------------------------------------------------------------------------
def map_pose(pose, l):
    """GetMapCoordsPose on level l (GridMap.cs:133-137): a scale by 2^-l, exact for dyadic poses."""
    stm = F(1.0) / F(2 ** l)
    return np.array([F(pose[0]) * stm, F(pose[1]) * stm, F(pose[2])], np.float32)


def geometry(cells, size, l, pose_map, xy, dtype=np.float32, rule=None):
    """One level's view of a scan at the map pose (x, y, 0).  dtype float32: every operation rounded as the reference rounds it;
    float64: the same expressions in binary64 (exact for the "exact" family).  rule: None, or a deliberately wrong copy --
    "ge" (cx >= w - 2 is outside), "w1" (limit w - 1), "limy_w" (limy from w), "idx_h" (idx = iy * h + ix), "trunc" (cx truncated
    to an integer before the range test), "out_zero" (a point outside the map adds 0 to the residual)."""
    assert pose_map[2] == 0.0
    D = dtype
    w, h = level_dims(size, l + 1)[l]
    cell = D(2 ** l)
    stm = D(1.0) / cell
    x, y = xy[:, 0].astype(D), xy[:, 1].astype(D)
    z = D(0.0)
    with np.errstate(all="ignore"):
        # rotation(0) * translation(pose * cell) * scale(stm), Matrix3x2 products term by term (:139-142)
        tx, ty = D(pose_map[0]) * cell, D(pose_map[1]) * cell
        m31, m32 = (tx * stm + ty * z) + z, (tx * z + ty * stm) + z
        cx, cy = (x * stm + y * z) + m31, (x * z + y * stm) + m32       # :161
        limx, limy = D(w) - D(2.0), D(h) - D(2.0)
        if rule == "w1":
            limx, limy = D(w) - D(1.0), D(h) - D(1.0)
        if rule == "limy_w":
            limy = limx
        tcx, tcy = (np.trunc(cx), np.trunc(cy)) if rule == "trunc" else (cx, cy)
        out = np.isnan(cx) | np.isnan(cy) | (tcx < 0) | (tcy < 0)
        out |= ((tcx >= limx) | (tcy >= limy)) if rule == "ge" else ((tcx > limx) | (tcy > limy))
        fxx, fyy = np.floor(np.where(out, z, cx)), np.floor(np.where(out, z, cy))
        ix, iy = fxx.astype(np.int64), fyy.astype(np.int64)
        fx, fy = np.where(out, z, cx) - fxx, np.where(out, z, cy) - fyy
        idx = iy * (h if rule == "idx_h" else w) + ix
        p = prob_of(cells[l]).astype(D)
        tap = lambda k: np.take(p, idx + k, mode="wrap")               # (wrap: only a wrong copy can leave the grid)
        i0, i1, i2, i3 = tap(0), tap(1), tap(w), tap(w + 1)
        xi, yi = D(1.0) - fx, D(1.0) - fy
        P = ((i0 * xi + i1 * fx) * yi) + ((i2 * xi + i3 * fx) * fy)
        gx = -(((i0 - i1) * xi) + ((i2 - i3) * fx))
        gy = -(((i0 - i2) * yi) + ((i1 - i3) * fy))
        P, gx, gy = np.where(out, z, P), np.where(out, z, gx), np.where(out, z, gy)
        fun = D(1.0) - P
        sinRot, cosRot = z * stm, D(1.0) * stm
        rot = ((-sinRot * x - cosRot * y) * gx + (cosRot * x - sinRot * y) * gy)
        res = fun * fun
        if rule == "out_zero":
            res = np.where(out, z, res)
        terms = np.stack([gx * fun, gy * fun, rot * fun, gx * gx, gy * gy, rot * rot, gx * gy, gx * rot, gy * rot, res]).astype(D)
    return Geo(w, h, cx, cy, ~out, ix, iy, idx, P, gx, gy, rot, terms)


def chunks(n, T, floor=False):
    """ScanMatcher.cs:149,159: T chunks of ceil(n / T) points (floor: the wrong copy).  -> [(lo, hi)], empty ones as (n, n)."""
    c = n // T if floor else (n + T - 1) // T
    return [(min(n, t * c), min(n, (t + 1) * c)) for t in range(T)]


def ref_sum(row, T, floor=False):
    """One sum in the reference's order: every chunk from +0 point after point in binary32, the partials in thread order."""
    tot = F(0.0)
    with np.errstate(all="ignore"):
        for lo, hi in chunks(row.shape[0], T, floor):
            part = np.add.accumulate(row[lo:hi], dtype=np.float32)[-1] if hi > lo else F(0.0)
            tot = F(tot + part)
    return tot


def sums_ref(g, T, floor=False):
    return np.array([ref_sum(g.terms[k].astype(np.float32), T, floor) for k in range(10)], np.float32)


def exact_sums(g):
    """The ten sums in exact rational arithmetic; a row with a NaN term (a NaN or infinite point: rotDeriv = NaN * 0) sums to NaN
    in every order."""
    out = []
    for k in range(10):
        if not np.isfinite(g.terms[k]).all():
            assert not np.isinf(g.terms[k]).any()
            out.append(float("nan"))
            continue
        nz = g.terms[k][g.terms[k] != 0]
        out.append(sum((fractions.Fraction(float(t)) for t in nz), fractions.Fraction(0)))
    return out


def expected(g, pad=0):
    """H, dTr, residual, n_in_map of an "exact" case: the rational sums, which binary32 holds (asserted by the CPU test).
    pad: the wrong copy in which every padding lane of the device's passes adds 1 to the residual."""
    s = [F(float(v)) for v in exact_sums(g)]                            # (lossless: asserted by the CPU test's exactness())
    H = np.array([[s[3], s[6], s[7]], [s[6], s[4], s[8]], [s[7], s[8], s[5]]], np.float32)
    return H, np.array(s[0:3], np.float32), F(s[9] + F(pad)), int(g.inmap.sum())


def padding_lanes(n, per_pass):
    return (-n) % per_pass if n else 0


def pack(s):
    """H (3 x 3), dTr from ten sums in the kernel's order."""
    return np.array([[s[3], s[6], s[7]], [s[6], s[4], s[8]], [s[7], s[8], s[5]]], np.float32), np.array(s[0:3], np.float32)


def invert_h(H):
    """sh_invert_h (csrc/m3x2.h; Matrix4x4.Invert's cofactor formulas with the last row and column of the identity) in binary32."""
    a, b, c, e, f, g, i, j, k = [F(v) for v in np.asarray(H, np.float32).ravel()]
    p, z = F(1.0), F(0.0)
    with np.errstate(all="ignore"):
        kp_lo, jp_ln, jo_kn = k * p - z * z, j * p - z * z, j * z - k * z
        ip_lm, io_km, in_jm = i * p - z * z, i * z - k * z, i * z - j * z
        a11 = +(f * kp_lo - g * jp_ln + z * jo_kn)
        a12 = -(e * kp_lo - g * ip_lm + z * io_km)
        a13 = +(e * jp_ln - f * ip_lm + z * in_jm)
        a14 = -(e * jo_kn - f * io_km + g * in_jm)
        det = a * a11 + b * a12 + c * a13 + z * a14
        if abs(det) < F(1.401298464e-45):
            return None
        inv = F(1.0) / det
        gp_ho, fp_hn, fo_gn = g * p - z * z, f * p - z * z, f * z - g * z
        ep_hm, eo_gm, en_fm = e * p - z * z, e * z - g * z, e * z - f * z
        R = [a11 * inv, -(b * kp_lo - c * jp_ln + z * jo_kn) * inv, +(b * gp_ho - c * fp_hn + z * fo_gn) * inv,
             a12 * inv, +(a * kp_lo - c * ip_lm + z * io_km) * inv, -(a * gp_ho - c * ep_hm + z * eo_gm) * inv,
             a13 * inv, -(a * jp_ln - b * ip_lm + z * in_jm) * inv, +(a * fp_hn - b * ep_hm + z * en_fm) * inv]
    return np.array(R, np.float32)


def step(H, dTr, est, variant=None):
    """EstimateTransformationLogLh (:93-125) / hs_step.  -> (new estimate, branch): branch in "h_zero", "singular", "clamp+",
    "clamp-", "inside".  variant: "no_clamp", "no_h_test" (the wrong copies)."""
    H = np.asarray(H, np.float32).ravel()
    est = np.array(est, np.float32)
    if variant != "no_h_test" and not (H[0] != 0 and H[4] != 0):
        return est, "h_zero"
    R = invert_h(H)
    if R is None:
        return est, "singular"
    d0, d1, d2 = [F(v) for v in dTr]
    with np.errstate(all="ignore"):
        sx = (d0 * R[0]) + (d1 * R[3]) + (d2 * R[6]) + F(0.0)
        sy = (d0 * R[1]) + (d1 * R[4]) + (d2 * R[7]) + F(0.0)
        sz = (d0 * R[2]) + (d1 * R[5]) + (d2 * R[8]) + F(0.0)
        branch = "inside"
        if sz > F(0.2):
            branch = "clamp+"
        elif sz < F(-0.2):
            branch = "clamp-"
        if variant != "no_clamp":
            sz = F(0.2) if branch == "clamp+" else F(-0.2) if branch == "clamp-" else sz
        return np.array([est[0] + sx, est[1] + sy, est[2] + sz], np.float32), branch


def chain_paths(lo, hi):
    """Which loops of hs_chain add elements of row[lo, hi): "head" (scalar, up to a multiple of 4), "body" (blocks of 32 in two
    register sets), "tail4", "tail1"."""
    out, i = set(), lo
    while i < hi and (i & 3):
        out.add("head"); i += 1
    if i + 32 <= hi:
        out.add("body")
        i += 32 * ((hi - i) // 32)
    if i + 4 <= hi:
        out.add("tail4")
        i += 4 * ((hi - i) // 4)
    if i < hi:
        out.add("tail1")
    return out


def segments(n, T, W):
    """hs_hessian_ref: per window of W points, the part [lo, hi) of every chunk that lies in it, relative to the window's base.
    -> [(chunk, window, lo - base, hi - base)]"""
    out = []
    for wi, base in enumerate(range(0, n, W)):
        end = min(n, base + W)
        for c, (clo, chi) in enumerate(chunks(n, T)):
            lo, hi = max(clo, base), min(chi, end)
            if lo < hi:
                out.append((c, wi, lo - base, hi - base))
    return out


# ---- maps --------------------------------------------------------------------------------------------------------------------------
def flat(size, levels):
    return [np.zeros(w * h, np.float32) for w, h in level_dims(size, levels)]


CALM = ((0, 1), (1, 1), (0, 2), (1, 2), (1, 0), (2, 0), (2, 1))


def speckled(size, levels, nan_at=None, calm=False):
    """Every level: 50 where (3 x + 5 y) % 7 == 0, -inf where it is 3, else 0 -- gradients in both directions everywhere, the last
    row and column included, and no symmetry between x and y.  calm: the cells under the two denormal border points are 0, so that
    a denormal fx or fy meets no gradient along its own axis (its products would not be multiples of any 2^-g)."""
    out = []
    for w, h in level_dims(size, levels):
        y, x = np.divmod(np.arange(w * h), w)
        k = (3 * x + 5 * y) % 7
        v = np.where(k == 0, VALUES["one"], np.where(k == 3, VALUES["zero"], VALUES["half"])).astype(np.float32)
        if calm:
            for cx_, cy_ in CALM:
                v[cy_ * w + cx_] = VALUES["half"]
        out.append(v)
    if nan_at is not None:
        out[0][nan_at[1] * size[0] + nan_at[0]] = VALUES["nan"]
    return out


def patch(size, levels, at=(10, 10)):
    """A flat map with one corner of gradient around cell `at` on level 0: (x + 1, y) occupied, (x, y + 1) free."""
    out = flat(size, levels)
    w = size[0]
    out[0][at[1] * w + at[0] + 1] = VALUES["one"]
    out[0][(at[1] + 1) * w + at[0]] = VALUES["zero"]
    return out


def informative(i, at=(10, 10)):
    """The i-th informative point: inside cell `at`, fx and fy in quarters, different for neighbouring indices."""
    return (at[0] + (i % 3 + 1) * 0.25, at[1] + ((i // 3 + i // 64) % 3 + 1) * 0.25)


# ---- A. border -----------------------------------------------------------------------------------------------------------------------
DEN = float(np.nextafter(F(0.0), F(1.0)))
SPECIAL = [(np.nan, 1.0), (1.0, np.nan), (np.inf, 1.0), (1.0, -np.inf), (-np.inf, np.inf), (1e30, 1.0), (1.0, -1e30), (1e30, 1e30)]


def border_points(w, h, scale=1.0, shift=(0.0, 0.0), denormal=True):
    """Scan points that land on level coordinates cx in {-0.0, 0, smallest denormal, 0.5, w - 2.5, w - 2, nextafter(w - 2), w - 1}
    at an interior cy, the same for cy, the four corners, and NaN / inf / 1e30 points, on a level of w x h cells whose cell is
    `scale` long, for the pose `shift`."""
    def along(m):
        lim = F(m - 2.0)
        v = [-0.0, 0.0, 0.5, float(lim) - 0.5, float(lim), float(np.nextafter(lim, F(np.inf))), float(lim) + 1.0, -0.5, -1.0]
        return v + ([DEN] if denormal else [])
    mx, my = (min(1.5, w - 2.0), min(1.5, h - 2.0))
    p = [(c, my) for c in along(w)] + [(mx, c) for c in along(h)]
    p += [(0.0, 0.0), (w - 2.0, 0.0), (0.0, h - 2.0), (w - 2.0, h - 2.0)]
    out = [(F(F(a) * F(scale)) - F(shift[0]), F(F(b) * F(scale)) - F(shift[1])) for a, b in p]
    return out + SPECIAL


BORDER_MAPS = {"16x16": (16, 16), "24x16": (24, 16), "16x24": (16, 24), "17x16": (17, 16), "2x2": (2, 2), "3x2": (3, 2), "2x3": (2, 3)}
for _name, _size in BORDER_MAPS.items():
    def _mk(name=_name, size=_size):
        @case("border_" + name, "border:0")
        def _b():
            """All finite border points together, then with the NaN / inf / 1e30 points (whose rotDeriv is NaN), then one at a time."""
            big = min(size) >= 4                                        # (the smallest maps have no room for a calm patch)
            p = border_points(size[0], size[1], denormal=big)
            return built(size, 1, speckled(size, 1, calm=big), (0, 0), [p[:-len(SPECIAL)], p] + [[q] for q in p], Ts=(1, 4))
    _mk()


@case("border_16x16_posed", "border:0")
def _border_posed():
    """The same with a pose that is not zero (no denormal target: x + tx must be exact)."""
    p = border_points(16, 16, shift=(0.5, -0.25), denormal=False)
    return built((16, 16), 1, speckled((16, 16), 1), (0.5, -0.25), [p[:-len(SPECIAL)], p], Ts=(1, 4))


def speckled_end(size, band=16):
    """A flat map whose last `band` columns (w > h) or rows are speckled: a point there is informative, and with the pose at the
    band its x, y -- which rotDeriv multiplies -- stay small."""
    w, h = size
    v = speckled(size, 1)[0]
    y, x = np.divmod(np.arange(w * h), w)
    v[(x < w - band) if w > h else (y < h - band)] = VALUES["half"]
    return [v]


for _size in ((32768, 8), (8, 32768)):
    def _mk(size=_size):
        @case("border_thin_%dx%d" % size, "border:0", "last_idx")
        def _b():
            """The far end of a long thin map: the last valid idx, (w - 2, h - 2)."""
            w, h = size
            shift = (w - 15.5, 0.5) if w > h else (0.5, h - 15.5)
            p = border_points(w, h, shift=shift, denormal=False)
            fin = p[:-len(SPECIAL)] + [(w - 2.75 - shift[0], h - 2.25 - shift[1]), (w - 3.0 - shift[0], h - 3.5 - shift[1])]
            return built(size, 1, speckled_end(size), shift, [fin, fin + SPECIAL], Ts=(1, 4))
    _mk()


for _l in (1, 2):
    def _mk(l=_l):
        @case("border_level%d_96x64" % l, "border:%d" % l)
        def _b():
            """The border of level l of a three-level pyramid of 96 x 64, 48 x 32, 24 x 16 cells: stm and the limits per level."""
            w, h = level_dims((96, 64), 3)[l]
            p = border_points(w, h, scale=2 ** l)
            cells = flat((96, 64), 3)                                  # (the other levels flat: there the same points have other fractions)
            cells[l] = speckled((96, 64), 3, calm=True)[l]
            return built((96, 64), 3, cells, (0, 0), [p[:-len(SPECIAL)], p], iters=[1, 1, 1], Ts=(1, 4))
    _mk()


# ---- B. counts -----------------------------------------------------------------------------------------------------------------------
COUNTS = (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1279, 1280, 1281, 1535, 1536, 1537, 2047, 2048, 2049, 2559, 2560, 2561,
          3071, 3072, 3073, 4097)
STRIDES = (64, 256, 512, 1280, 1536, 2048)


def informative_indices(n):
    s = {0, n - 1}
    for m in STRIDES:
        for k in range(m, n + 1, m):
            s |= {k - 1, k}
    return sorted(i for i in s if 0 <= i < n)


def count_scan(n):
    p = [(1000.0 + i % 7, -5.0 - i % 3) for i in range(n)]            # outside the map: terms zero, residual exactly 1
    for i in informative_indices(n):
        p[i] = informative(i)
    return p


for _n in COUNTS:
    def _mk(n=_n):
        @case("count_%d" % n, "count:%d" % n)
        def _c():
            """n points, the informative ones at 0, n - 1 and either side of every multiple of 64 .. 2048, the rest outside."""
            return built((64, 64), 1, patch((64, 64), 1), (0, 0), [count_scan(n)], Ts=(1, 7, 64), batch=(2, 9) if n in (1281, 1537, 2049, 4097) else ())
    _mk()


@case("count_0", "count:0")
def _count_0():
    """An empty scan: the hint comes back."""
    return built((64, 64), 1, patch((64, 64), 1), (3.5, -2.25), [np.zeros((0, 2))], Ts=(1, 64), batch=(2, 9))


@case("batch_sizes", "batch")
def _batch_sizes():
    """Group C: batches of 1 .. 65 distinct dyadic hints, every entry equal to its single match."""
    return built((64, 64), 1, patch((64, 64), 1), (0, 0), [count_scan(300)], Ts=(1, 7), batch=(1, 2, 7, 8, 9, 12, 65))


# ---- D. chunks (order-sensitive) --------------------------------------------------------------------------------------------------------
def rough_scan(n, seed):
    """Points with many bits all over a 64 x 64 speckled map, a few outside."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(1.0, 61.0, (n, 2)).astype(np.float32)
    p[rng.random(n) < 0.05] += F(70.0)
    return p


# (T, n): chunk = ceil(n / T) takes the lengths 1, 3, 4, 5, 31, 32, 33, 35, 63, 64, 65, 96, 97; starts take every residue mod 4;
# T > n; the last chunk short (190) or empty (130); a chunk across the window boundary (1400, 1700 at T = 3); n = W and W + 1
CHUNKS = [(1, n) for n in (3, 4, 5, 31, 32, 33, 35, 63, 64, 65, 96, 97)]
CHUNKS += [(2, 66), (2, 193), (3, 105), (3, 13), (4, 20), (4, 131), (7, 679), (7, 28), (16, 496), (16, 1021), (63, 4095), (64, 4032),
           (64, 64), (64, 192), (64, 190), (64, 130), (64, 1), (64, 5), (64, 63), (3, 1400), (3, 1700), (7, 1280), (7, 1281),
           (7, 1536), (7, 1537), (64, 2049)]
SEED_BUMP = {(1, 4): 1}               # (a seed whose four terms do round differently in two orders)
for _T, _n in CHUNKS:
    def _mk(T=_T, n=_n):
        @case("chunk_T%d_n%d" % (T, n), "chunks:%d:%d" % (T, n))
        def _c():
            return built((64, 64), 1, speckled((64, 64), 1), (0.5, 0.25), [rough_scan(n, 100 * T + n + SEED_BUMP.get((T, n), 0))], family="order", Ts=(T,),
                         batch=(9,) if n >= 1280 else ())
    _mk()


# ---- E. the step ----------------------------------------------------------------------------------------------------------------------
def stripes(size, axis):
    """A map constant along x (axis 0: rows of 50 at y % 5 == 0) or along y."""
    w, h = size
    y, x = np.divmod(np.arange(w * h), w)
    return [np.where((y if axis == 0 else x) % 5 == 0, VALUES["one"], VALUES["half"]).astype(np.float32)]


QUARTERS = [(6.25 + 1.5 * k, 7.75 + 1.25 * ((3 * k) % 7)) for k in range(24)]


@case("step_all_out", "step:h_zero")
def _step_all_out():
    return built((32, 32), 1, speckled((32, 32), 1), (1.5, 2.25), [[(100.0 + k, -40.0) for k in range(70)]])


@case("step_const_x", "step:h_zero", "h11_zero")
def _step_const_x():
    return built((48, 48), 1, stripes((48, 48), 0), (0.25, 0.5), [QUARTERS])


@case("step_const_y", "step:h_zero", "h22_zero")
def _step_const_y():
    return built((48, 48), 1, stripes((48, 48), 1), (0.25, 0.5), [[(b, a) for a, b in QUARTERS]])


@case("step_const_x_nan_point", "step:h_zero", "h11_zero", "nan_sums")
def _step_const_x_nan_point():
    """H11 = 0 and H13 = NaN (a NaN point: rotDeriv = NaN * 0): only the H11 test keeps the pose."""
    return built((48, 48), 1, stripes((48, 48), 0), (0.25, 0.5), [QUARTERS + [(np.nan, 1.0)]])


@case("step_collinear", "step:singular")
def _step_collinear():
    """One informative point three times: H = 3 v v^T has rank one, every cofactor and the determinant are exactly zero."""
    return built((64, 64), 1, patch((64, 64), 1), (0, 0), [[informative(1)] * 3 + [(500.0, 2.0)] * 5])


def step_scan(seed, n=12):
    """Twelve points in halves on a 32 x 32 speckled map."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(4, 56, n) / 2.0, rng.integers(4, 56, n) / 2.0], 1)


# seeds whose first step has sz > 0.2, sz < -0.2 and 0 < |sz| < 0.2 (found by trying seeds 0, 1, 2, ... through kc.step; the CPU
# test asserts the branch with kc.step and Grid.estimate_step before the device is looked at)
STEP_SEEDS = {"clamp+": 42, "clamp-": 200, "inside": 0}


def _step_case(branch):
    @case("step_" + {"clamp+": "clamp_pos", "clamp-": "clamp_neg", "inside": "inside"}[branch], "step:" + branch)
    def _s():
        return built((32, 32), 1, speckled((32, 32), 1), (0.5, -0.5), [step_scan(STEP_SEEDS[branch])])


for _b in STEP_SEEDS:
    _step_case(_b)


@case("step_nan_tap", "nan_tap")
def _step_nan_tap():
    """One cell whose probability is NaN under one point's taps: every sum is NaN, and so is the pose after a step."""
    p = [(4.5 + 2.25 * k, 5.25 + 1.5 * k) for k in range(20)] + [(20.25, 20.5)]
    return built((64, 64), 1, speckled((64, 64), 1, nan_at=(21, 20)), (0, 0), [p], Ts=(1, 4))


# ---- F. levels -----------------------------------------------------------------------------------------------------------------------
# (whole numbers and a pose in halves: fx, fy are 1/2 on level 0 and eighths on level 2, and the products still fit binary32)
LEVEL_POINTS = [(1.0 + 3 * (k % 13) + (k % 4), 6.0 + 3 * (k // 13) + (k % 2)) for k in range(130)]
for _levels, _iters in ((1, [1]), (2, [0, 1]), (3, [1, 0, 2])):
    def _mk(levels=_levels, iters=_iters):
        @case("levels_%d" % levels, "levels:%d" % levels)
        def _l():
            """Pyramids of 1, 2, 3 levels with iteration counts per level (finest first); the single-level pyramid's single match
            brings helper workgroups that have no finer level to touch."""
            return built((64, 48), levels, speckled((64, 48), levels), (4.5, -3.5), [LEVEL_POINTS], iters=iters, Ts=(1, 4, 64), batch=(2, 9))
    _mk()
