"""Case builders for the K2 (HoleMap update) edge tests: tests/test_k2_cases_cpu.py checks every case on the CPU (both oracles, the
kernel's rule restated in NumPy, and the property the case claims to exercise), tests/test_gpu_holemap_edges.py runs them on the
device.  No device and no oracle here.

A case is `Case(name, build, claims)`; `build()` returns `Built(size, start, steps)`: the map's side, the start map (uint16, or None
for all 32750) and a short list of steps (xy, pxcs, hole_width, quality).  All cases use one pixel per metre, c = 1, s = 0,
integer-valued points and px = x1 + 0.5, py = y1 + 0.5: xp, yp (:521-522) are x1 + X, y1 + Y exactly, and the extended end x2, y2
and derrorv follow from the float operations of k2_make_ray (:524-530), which `geometry()` restates in float32 NumPy.  `touches()`
lists every (pixel, ray, step, value) of a step by the two closed forms that tests/test_closed_forms.py pins against the literal
loops: the minor offset m(x) and the V profile.
"""
import collections

import numpy as np

F = np.float32
INT_MIN = -(2 ** 31)
NO_OBSTACLE = 65500                    # TS_NO_OBSTACLE (holemap.hip; CoreSLAMProcessor.cs:21)
START = 32750                          # a fresh HoleMap's pixel (HoleMap.cs)

# mirrored from the source
ZONE_MIN, ZONE_MAX = 48, 192           # K2_ZONE_MIN, K2_ZONE_MAX (holemap.hip); zone = clamp(R // 8): k2_zone_radius
RB_NUM = 12                            # SLAMHIP_K2_RB's default (cs_launch_holemap_update): rB = clamp((12 R + 1079) // 1080, 1, 48)
MAXHIT = 4                             # K2_MAXHIT: hits a step lane orders in registers
MIXQ = 192                             # K2_MIXQ: a workgroup's LDS queue of mixed zone pixels
OWN_CAP = 848                          # K2_OWN_CAP: own rays whose records lie side by side (direct own list)
LDS_RAYS = 2048                        # K2_LDS_RAYS: the largest scan of the one-launch form
NBUCK = 1024                           # RS_NBUCK (raster.h): slope buckets per direction class
WAVE_CAND = 64                         # k2_wave_pixel: more candidates than lanes -> the all-rays scan
ALONE_REACH = 11                       # buckets either side that the lone-ray rule looks at (k2_pixels, table phase)
ARC_SANE = 16000.0                     # k2_arc_member / k2_pixels: |pose|, |point| beyond it select every ray
HW_PX_MAX = 8000.0                     # cs_launch_holemap_update: hole half widths from here on (or negative) turn arcs off
QUALITIES = (0, 1, 2, 50, 128, 254, 255, 256)      # the API admits 0 .. 256 (slamhip_cs_update_holemap_pxcs); the reference's
#                                                    Quality is a byte, "1 to 255, DO NOT USE 0 OR 256" (:74-80): alpha as it is
START_VALUES = (0, 1, 255, 256, 32750, 65499, 65500, 65501, 65535)

Case = collections.namedtuple("Case", "name build claims")
Built = collections.namedtuple("Built", "size start steps")
CASES = []
BIG = 16384                            # the two cases on a map of this side are left out of the variant runs


def case(name, *claims):
    def deco(fn):
        CASES.append(Case(name, fn, claims))
        return fn
    return deco


def by_name(name):
    return next(c for c in CASES if c.name == name)


def zone_radius(R):
    return min(max(R // 8, ZONE_MIN), ZONE_MAX)


def rb_radius(R, num=RB_NUM):
    return min(max((num * R + 1079) // 1080, 1), ZONE_MIN)


def pxcs_at(x1, y1):
    return np.array([x1 + 0.5, y1 + 0.5, 1.0, 0.0], np.float32)


def pts(deltas):
    return np.array(deltas, np.float64).reshape(-1, 2).astype(np.float32)


def step(deltas, x1, y1, hw=2.0, quality=50):
    return (pts(deltas), pxcs_at(x1, y1), float(hw), int(quality))


def start_pattern(size):
    """Every start value of the issue's list on every row, column and diagonal."""
    y, x = np.mgrid[0:size, 0:size]
    return np.array(START_VALUES, np.uint16)[(x + 4 * y) % len(START_VALUES)].ravel()


# ---- what the integers of a step imply -----------------------------------------------------------------------------------------
def _wrap32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v & 0x80000000 else v


def _cdiv(a, b):
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


def _f2i(a):
    """cvttss2si on a float32 array: truncation, int.MinValue for what does not fit."""
    a = np.asarray(a, np.float32)
    bad = ~np.isfinite(a) | (a >= F(2147483648.0)) | (a <= F(-2147483904.0))
    out = np.where(bad, 0, np.trunc(a)).astype(np.int64)
    out[bad] = INT_MIN
    return out


def _clip(size, xyc, yxc, xy, yx):
    """ClipRay (:320-345) in Python integers with 32-bit wrapping."""
    for low in (True, False):
        if (xyc < 0) if low else (xyc >= size):
            if xyc == xy:
                return False, xyc, yxc
            num = _wrap32(_wrap32(yxc - yx) * _wrap32((0 if low else size - 1) - xyc))
            den = _wrap32(xyc - xy)
            if den == -1 and num == INT_MIN:
                return False, xyc, yxc
            yxc = _wrap32(yxc + _cdiv(num, den))
            xyc = 0 if low else size - 1
    return True, xyc, yxc


GEO = np.dtype([(n, np.int64) for n in ("valid", "x1", "y1", "xp", "yp", "x2", "y2", "major_x", "smaj", "smin", "dx", "dxc", "dyc",
                                         "d", "lim2", "lim1")])


def geometry(size, st):
    """Per ray of the step what k2_make_ray makes of it (holemap.hip, :505-530 and :361-408), as a structured array; `valid` 0: the
    ray draws nothing.  None: the robot is outside the map."""
    xy, pxcs, hw, _ = st
    px, py, c, s = [F(v) for v in pxcs]
    x1, y1 = int(_f2i(px)), int(_f2i(py))
    if not (0 <= x1 < size and 0 <= y1 < size):
        return None
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    X, Y = xy[:, 0], xy[:, 1]
    with np.errstate(all="ignore"):
        x2p = c * X - s * Y                                             # :519
        y2p = s * X + c * Y                                             # :520
        xp, yp = _f2i(px + x2p), _f2i(py + y2p)                          # :521-522
        dist = np.sqrt(x2p * x2p + y2p * y2p)                           # :524
        add = ((F(hw) * F(1.0)) * F(0.5)) / dist                        # :525 (scale = 1)
        x2 = _f2i(px + x2p * (F(1.0) + add))                            # :527, :529
        y2 = _f2i(py + y2p * (F(1.0) + add))                            # :528, :530
    g = np.zeros(len(xy), GEO)
    for i in range(len(xy)):
        r = g[i]
        r["x1"], r["y1"] = x1, y1
        if INT_MIN in (int(xp[i]), int(yp[i]), int(x2[i]), int(y2[i])):
            continue                                                    # (deviation D1)
        ok, x2c, y2c = _clip(size, int(x2[i]), int(y2[i]), x1, y1)       # :365
        if ok:
            ok, y2c, x2c = _clip(size, y2c, x2c, y1, x1)                 # :366
        if not ok or not (0 <= x2c < size and 0 <= y2c < size):         # (deviation D4)
            continue
        ddx, ddy = _wrap32(int(x2[i]) - x1), _wrap32(int(y2[i]) - y1)
        if INT_MIN in (ddx, ddy):
            continue                                                    # (deviation D2)
        dx, dy, dxc, dyc = abs(ddx), abs(ddy), abs(x2c - x1), abs(y2c - y1)      # :368-371
        smaj, smin, major_x = (ddx > 0) - (ddx < 0), (ddy > 0) - (ddy < 0), 1
        if dx > dy:                                                     # :377
            t = _wrap32(int(xp[i]) - int(x2[i]))                        # :379
        else:
            dx, dxc, dyc, smaj, smin, major_x = dy, dyc, dxc, smin, smaj, 0      # :383-385 (the axis swap)
            t = _wrap32(int(yp[i]) - int(y2[i]))                        # :386
        if t == INT_MIN or t == 0:                                      # (D2), :389-392
            continue
        d = abs(t)
        r["valid"], r["xp"], r["yp"], r["x2"], r["y2"] = 1, xp[i], yp[i], x2[i], y2[i]
        r["major_x"], r["smaj"], r["smin"], r["dx"], r["dxc"], r["dyc"], r["d"] = major_x, smaj, smin, dx, dxc, dyc, d
        r["lim2"], r["lim1"] = _wrap32(dx - 2 * d), _wrap32(dx - d)     # :406, :408
    return g


def minor_offset(x, dxc, dyc):
    """m(x) = min(x, max(0, ceil((2 dyc x - dxc) / (2 dxc)))), the closed form of the error recurrence (:394-396, :433-441)."""
    x = np.asarray(x, np.int64)
    if dxc == 0:
        return np.zeros_like(x)
    N = 2 * dyc * x - dxc
    return np.minimum(x, np.maximum(0, -((-N) // (2 * dxc))))


def pixval(d, lim2, lim1, x, float_incv=False):
    """The V profile at step x (array): k2_pixval_closed (holemap.hip), for derrorv <= 2^24."""
    x = np.asarray(x, np.int64)
    incv = -(NO_OBSTACLE // d)                                          # :398 (truncating division)
    incerrorv = -NO_OBSTACLE - d * incv                                 # :399
    xs = 0 if lim2 < 0 else lim2 + 1
    n1 = np.maximum(np.minimum(x, lim1) - xs + 1, 0)
    j = (x - xs + 1) - n1
    u0, g = d // 2 + n1 * incerrorv, -incerrorv
    J = np.where((j > 0) & (d - u0 > 0), (d - u0 + (g + d) - 1) // (g + d) - 1, 0)
    v = NO_OBSTACLE + (n1 - j) * incv + np.minimum(j, J)
    if float_incv:                                                      # (a wrong copy for the CPU test: the slope -65500 / derrorv as a float, no error term)
        v = np.trunc(F(NO_OBSTACLE) + (n1 - j).astype(np.float32) * (F(-NO_OBSTACLE) / F(d))).astype(np.int64)
    return np.where(x <= lim2, NO_OBSTACLE, v)


TOUCH = np.dtype([("ptr", np.int64), ("ray", np.int64), ("x", np.int64), ("b", np.int64), ("value", np.int64), ("inv", np.int64)])


def touches(size, geo, float_incv=False):
    """Every (pixel, ray, step, signed minor offset, value, inside the ray's V) of a step, rays in index order, steps in walk order."""
    out = []
    for i in np.flatnonzero(geo["valid"]):
        r = geo[i]
        dxc, dyc, d, lim2, lim1 = int(r["dxc"]), int(r["dyc"]), int(r["d"]), int(r["lim2"]), int(r["lim1"])
        x = np.arange(dxc + 1, dtype=np.int64)
        m = minor_offset(x, dxc, dyc)
        a, b = r["smaj"] * x, r["smin"] * m
        ox, oy = (a, b) if r["major_x"] else (b, a)
        t = np.zeros(dxc + 1, TOUCH)
        t["ptr"] = (r["y1"] + oy) * size + (r["x1"] + ox)
        t["ray"], t["x"], t["b"] = i, x, b
        t["value"] = pixval(d, lim2, lim1, x, float_incv)
        t["inv"] = x > lim2
        out.append(t)
    return np.concatenate(out) if out else np.zeros(0, TOUCH)


# ---- the sorted table (raster.h) and what goes by it -----------------------------------------------------------------------------
def rs_bucket(t):
    k = np.floor((np.asarray(t, np.float32) + F(1.0)) * F(NBUCK // 2)).astype(np.int64)
    return np.clip(k, 0, NBUCK - 1)


def ray_class(geo):
    return np.where(geo["major_x"] == 1, np.where(geo["smaj"] >= 0, 0, 1), np.where(geo["smaj"] >= 0, 2, 3))


def ray_slope(geo):
    """The slope a ray is bucketed with: (float)sdyc / (float)dxc (k2_ray_bucket)."""
    with np.errstate(all="ignore"):
        return np.where(geo["dxc"] > 0, (geo["smin"] * geo["dyc"]).astype(np.float32) / np.maximum(geo["dxc"], 1).astype(np.float32), F(0.0)).astype(np.float32)


def ray_bucket(geo):
    return rs_bucket(ray_slope(geo))


def rs_window(a, b, narrow=0):
    """The buckets [blo, bhi] of a pixel's candidate range (rs_range; the hardware's reciprocal is within 1 ulp of this one)."""
    ra = F(1.0) / F(a)
    m = F(4.0e-6)
    blo, bhi = int(rs_bucket((F(b) - F(0.5)) * ra - m)), int(rs_bucket((F(b) + F(0.5)) * ra + m))
    return blo + narrow, bhi - narrow


def rs_classes(dx, dy):
    """[(class, a, b)] of the pixel at offset (dx, dy): two on a diagonal, none for the robot's pixel."""
    adx, ady = abs(dx), abs(dy)
    out = []
    if adx >= ady and adx > 0:
        out.append((0 if dx > 0 else 1, adx, dy))
    if ady >= adx and ady > 0:
        out.append((2 if dy > 0 else 3, ady, dx))
    return out


def candidates(geo, dx, dy, narrow=0):
    """Indices of the rays in the candidate range of the pixel at (dx, dy)."""
    cls, bk, ok = ray_class(geo), ray_bucket(geo), geo["valid"] == 1
    out = []
    for c, a, b in rs_classes(dx, dy):
        blo, bhi = rs_window(a, b, narrow)
        out.append(np.flatnonzero(ok & (cls == c) & (bk >= blo) & (bk <= bhi)))
    return np.concatenate(out) if out else np.zeros(0, np.int64)


def xalone(geo, plus=2):
    """Per ray the step from which the lone-ray rule lets its lanes blend without a lookup (k2_pixels, table phase), from the slopes
    of ALL valid rays of its class (a sector workgroup holds a subset: its g is no smaller); 2047: never."""
    cls, bk, sl, ok = ray_class(geo), ray_bucket(geo), ray_slope(geo), geo["valid"] == 1
    out = np.full(len(geo), 2047, np.int64)
    for i in np.flatnonzero(ok):
        near = ok & (cls == cls[i]) & (bk >= max(bk[i] - ALONE_REACH, 0)) & (bk <= min(bk[i] + ALONE_REACH, NBUCK - 1))
        dd = np.abs(sl[near] - sl[i]).astype(np.float32)
        same = int((dd == 0).sum())
        g = F(10.0) * (F(2.0) / F(NBUCK))
        if (dd > 0).any():
            g = min(g, dd[dd > 0].min())
        out[i] = xalone_of_gap(g, plus) if same == 1 else 2047
    return out


def xalone_of_gap(g, plus=2, rcp_ulps=0):
    """min((int)(rcp(g - 4e-7) * 1.0001) + 2, 2047) for g > 1e-6, in float32; rcp_ulps moves the reciprocal by that many ulps."""
    g = F(g)
    if not g > F(1.0e-6):
        return 2047
    r = F(1.0) / F(g - F(4.0e-7))
    for _ in range(abs(rcp_ulps)):
        r = np.nextafter(r, F(np.inf) if rcp_ulps > 0 else F(0.0), dtype=np.float32)
    return min(int(F(r * F(1.0001))) + plus, 2047)


def ray_octant(geo):
    """k2_ray_octant: by the exact class and the slope's sign."""
    sd = geo["smin"] * geo["dyc"]
    return np.where(geo["major_x"] == 1, np.where(geo["smaj"] >= 0, np.where(sd < 0, 0, 1), np.where(sd > 0, 4, 5)),
                    np.where(geo["smaj"] >= 0, np.where(sd > 0, 2, 3), np.where(sd < 0, 6, 7)))


def pixel_octant(dx, dy):
    """k2_pixel_octant: a diagonal pixel belongs to the octant that begins there."""
    adx, ady = abs(dx), abs(dy)
    if adx > ady:
        return (0 if dy < 0 else 1) if dx > 0 else (4 if dy > 0 else 5)
    if ady > adx:
        return (2 if dx > 0 else 3) if dy > 0 else (6 if dx < 0 else 7)
    return (2 if dy > 0 else 0) if dx > 0 else (4 if dy > 0 else 6)


def arc_u(xy, pxcs):
    """k2_arc_member's direction coordinate u in [0, 8) of the float end points (exact float32 division for the hardware's
    reciprocal, which is within 1 ulp)."""
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    c, s = F(pxcs[2]), F(pxcs[3])
    X, Y = c * xy[:, 0] - s * xy[:, 1], s * xy[:, 0] + c * xy[:, 1]
    ax, ay = np.abs(X), np.abs(Y)
    with np.errstate(all="ignore"):
        ux = np.where(X > 0, F(1.0) + Y / ax, F(5.0) - Y / ax)
        uy = np.where(Y > 0, F(3.0) - X / ay, F(7.0) + X / ay)
    return np.where(ax > ay, ux, uy).astype(np.float32), (ax < F(ARC_SANE)) & (ay < F(ARC_SANE))


def arc_member(xy, pxcs, octant, rB, margin_num=8.0):
    u, sane = arc_u(xy, pxcs)
    halfw = F(0.5) + F(margin_num) / F(rB) + F(0.02)
    d = (u - F(octant + 0.5)).astype(np.float32)
    d = d - F(8.0) * np.rint(d * F(0.125))
    with np.errstate(invalid="ignore"):
        return ~sane | ~(np.abs(d) > halfw)


def arcs_on(size, st):
    """Whether the default build selects rays by octant for this step (cs_launch_holemap_update, k2_pixels)."""
    xy, pxcs, hw, _ = st
    hw_px = F(F(hw) * F(1.0)) * F(0.5)
    return bool(0 < len(xy) <= LDS_RAYS and hw_px >= 0 and hw_px < F(HW_PX_MAX) and size <= 16384
                and abs(pxcs[0]) < ARC_SANE and abs(pxcs[1]) < ARC_SANE)


# ---- building blocks ---------------------------------------------------------------------------------------------------------------
DIRS8 = ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))


def ring(r):
    """End points at Chebyshev radius r: the four axes, the four diagonals, and one slope inside each of the eight octants."""
    h = max(r // 2, 1) if r > 1 else 0
    out = [(ux * r, uy * r) for ux, uy in DIRS8]
    out += [(sx * r, sy * h) for sx in (1, -1) for sy in (1, -1)] + [(sx * h, sy * r) for sx in (1, -1) for sy in (1, -1)]
    return out


def filler(n, rng, lo=2, hi=9):
    """n short rays in every direction (they pad a scan to its ray count and cross the central rings)."""
    out = []
    while len(out) < n:
        x, y = int(rng.integers(-hi, hi + 1)), int(rng.integers(-hi, hi + 1))
        if max(abs(x), abs(y)) >= lo:
            out.append((x, y))
    return out


# ---- ray-count edges ---------------------------------------------------------------------------------------------------------------
RAY_COUNTS = (1, 63, 64, 65, 90, 91, 383, 384, 392, 1023, 1024, 1025, 1536, 1544, 2047, 2048, 2049)


def rim_radii(R):
    z, rb = zone_radius(R), rb_radius(R)
    return sorted({r for r in (z - 1, z, z + 1, rb - 1, rb, rb + 1) if r >= 2}, reverse=True)       # (the zone's rim first: scans of fewer rays than these take cut the list short)


for _R in RAY_COUNTS:
    def _mk(R=_R):
        @case("rays_%d" % R, "ray_count", "rim")
        def _rays():
            """R rays (hole width 2: the clipped length is the end point's radius + 1): ends on, one short of and one past the
            zone's rim and the rB ring, on the axes, the diagonals and inside every octant; short rays pad the count.  Shuffled."""
            rng = np.random.default_rng(R)
            size = 128 if zone_radius(R) <= 49 else 512
            d = [p for r in rim_radii(R) for p in ring(max(r - 1, 1))]
            d = (d + filler(max(R - len(d), 0), rng))[:R] if R > 1 else [(zone_radius(R) - 1, 0)]
            d = [d[k] for k in rng.permutation(len(d))]
            return Built(size, None, [step(d, size // 2, size // 2, 2.0, 50), step(d[::-1], size // 2 + 1, size // 2 - 2, 2.0, 200)])
    _mk()


# ---- central pixels ----------------------------------------------------------------------------------------------------------------
for _n in (1, 2, 300, 1080):
    def _mk(n=_n):
        @case("central_cross_%d" % n, "central")
        def _cross():
            """1080 rays (rB = 12): n of them run east over the central pixels (1 .. 11, 0), the rest west; every ray is step 0
            on the robot's own pixel."""
            return Built(64, start_pattern(64), [step([(20, 0)] * n + [(-20, 0)] * (1080 - n), 32, 32, 2.0, 50)])
    _mk()


@case("central_adjacent_octant", "central", "adjacent_octant")
def _adjacent():
    """Rays whose first steps lie in the octant next to their own: just off an axis (the axis' pixels belong to the octant beyond
    it) and just off a diagonal (a diagonal pixel belongs to the octant that begins there), all eight ways; 300 rays: rB = 4."""
    d = []
    for a, b in ((20, 1), (20, 19)):
        d += [(sx * a, sy * b) for sx in (1, -1) for sy in (1, -1)] + [(sx * b, sy * a) for sx in (1, -1) for sy in (1, -1)]
    d = (d * 19)[:300]
    return Built(64, None, [step(d, 32, 32, 2.0, 50)])


@case("central_inside_v", "central", "central_marked")
def _inside_v():
    """Obstacles at distance 1 .. 12 = rB in every direction with a hole of half width 20: lim2 < 0, every step is inside its ray's
    V, every central pixel is marked and drawn in ray order by the all-rays scan."""
    d = [p for r in range(1, 13) for p in ring(r)]
    d = (d * 6)[:1080]
    return Built(64, start_pattern(64), [step(d, 32, 32, 40.0, 50), step(d, 31, 33, 40.0, 256)])


@case("central_inside_v_shuffled", "central", "central_marked", "index_not_angle")
def _inside_v_shuffled():
    b = _inside_v()
    rng = np.random.default_rng(5)
    st = []
    for xy, pxcs, hw, q in b.steps:
        st.append((xy[rng.permutation(len(xy))], pxcs, hw, q))
    return Built(b.size, b.start, st)


for _n in (50, 300):
    def _mk(n=_n):
        @case("identical_%d" % n, "identical")
        def _identical():
            """n identical rays with a V of half width 2; 300 rays: rB = 4, the ray ends in the central rings' neighbourhood."""
            return Built(64, start_pattern(64), [step([(6, 2)] * n, 30, 30, 4.0, 50), step([(-3, 5)] * n, 30, 30, 4.0, 255)])
    _mk()


# ---- the counting shortcut and the blend's fixed point ----------------------------------------------------------------------------
COUNTS = ((1, (40, 0)), (2, (0, 40)), (7, (-40, 0)), (40, (0, -40)), (300, (40, 20)))


for _q in QUALITIES:
    def _mk(q=_q):
        @case("count_q%d" % q, "counting")
        def _count():
            """350 rays (rB = 4, zone 48): 1, 2, 7, 40 and 300 rays over the same zone pixels, all below every V (hole width 2, the
            obstacles at radius 40), on a start map that holds every start value of the list on each of the lines."""
            d = [p for n, p in COUNTS for _ in range(n)]
            return Built(128, start_pattern(128), [step(d, 64, 64, 2.0, q)])
    _mk()


# ---- mixed zone pixels ---------------------------------------------------------------------------------------------------------------
for _where in ("lo", "mid", "hi"):
    def _mk(where=_where):
        @case("mixed_47_48_%s" % where, "mixed", "mixed_47_48")
        def _mixed():
            """800 rays (zone 100, rB 9).  Nine long rays run along each axis and each diagonal below their V; one ray per direction
            ends at radius 50 with a hole of half width 5: its V covers the pixels at radius 47 (queued) and 48 (the lane's own
            ordered draw), and its index is the lowest, a middle or the highest of its direction's rays."""
            d = []
            for ux, uy in DIRS8:
                long_ = [(ux * 120, uy * 120)] * 9
                k = {"lo": 0, "mid": 4, "hi": 9}[where]
                d += long_[:k] + [(ux * 50, uy * 50)] + long_[k:]
            d += filler(800 - len(d), np.random.default_rng(8))
            return Built(512, None, [step(d, 256, 256, 10.0, 128)])
    _mk()


@case("mixq_overflow", "mixed", "mixq")
def _mixq():
    """1080 rays (rB 12, zone 135).  Obstacles at radius 20 with a hole of half width 10: 300 of them spread over octant 1 put more
    than 192 mixed pixels below radius 48 there, three in octant 5 fewer than 192; long rays below their V cross both."""
    d = [(20, j % 20) for j in range(300)] + [(60, j % 60) for j in range(200)]
    d += [(-20, -3), (-20, -9), (-20, -15)] + [(-60, -(j % 60)) for j in range(200)]
    d += filler(1080 - len(d), np.random.default_rng(9))
    d = [d[k] for k in np.random.default_rng(10).permutation(len(d))]
    return Built(256, None, [step(d, 128, 128, 20.0, 90)])


# ---- candidate counts ------------------------------------------------------------------------------------------------------------
for _n in (64, 65):
    def _mk(n=_n):
        @case("cand_%d" % n, "candidates", "wave_cand")
        def _cand():
            """200 rays.  n rays of slope 0 run east (n - 1 of them long, below their V); one of them, of a middle index, ends at
            radius 30 with a V of half width 2: the pixels (29 .. 32, 0) are mixed and have exactly n candidates."""
            d = [(60, 0)] * (n - 1)
            d.insert(n // 2, (30, 0))
            d += [(-30 - (j % 20), (j % 7) - 3) for j in range(200 - n)]
            return Built(128, None, [step(d, 64, 64, 4.0, 100)])
    _mk()


def _far_rays(c, h):
    """c candidates of the far pixel (60, 0), h of which draw it: slope 0 or 1 / 128 draws it, 1 / 110 is in its range but passes by."""
    hitting = [(59, 0), (127, 1), (127, -1), (100, 0), (90, 0)][:h]       # (the first one ends there: its V covers the pixel)
    passing = [(109, 1), (109, -1), (108, 1), (108, -1)][:c - h]
    return hitting + passing


for _c in (4, 5):
    for _h in range(1, _c + 1):
        for _o in range(3):
            def _mk(c=_c, h=_h, o=_o):
                @case("far_c%d_h%d_o%d" % (c, h, o), "candidates", "far_cand")
                def _far():
                    """The far pixel (60, 0) (zone 48) with exactly c candidates, h of them hits; the ray whose V covers
                    the pixel has the lowest (o = 0), the middle (o = 1) or the highest (o = 2) index among the hits."""
                    d = _far_rays(c, h)
                    hits, passing = d[1:h], d[h:]
                    hits.insert({0: 0, 1: h // 2, 2: h - 1}[o], d[0])      # (the ray whose V covers the pixel: first, middle, last of the hits)
                    d = passing[:1] + hits + passing[1:]
                    d += [(-5, 3), (2, -7), (-60, -60)]
                    return Built(256, None, [step(d, 128, 128, 2.0, 200)])
            _mk()


# ---- the lone-ray bound --------------------------------------------------------------------------------------------------------------
CLASS_DIR = {0: (1, 0), 1: (-1, 0), 2: (0, 1), 3: (0, -1)}
PAIR_MINORS = (0, 1, 2, 5, 6, 7, 12, 20)         # partner's minor end offset; 0: a duplicate (same slope: never alone)


def _class_point(cls, major, minor):
    ux, uy = CLASS_DIR[cls]
    return (ux * major + abs(uy) * minor, uy * major + abs(ux) * minor)


for _cls in range(4):
    for _m in PAIR_MINORS:
        for _ord in ("fwd", "rev"):
            def _mk(cls=_cls, m=_m, order=_ord):
                @case("pair_c%d_m%d_%s" % (cls, m, order), "lone", "pair")
                def _pair():
                    """Two rays of one class: a long one along the axis, below its V out to 210, and a partner towards (200, m)
                    with a hole of half width 150, inside its V from step 51 on: where they share a pixel beyond the zone the
                    blend order shows.  Robot in the middle of the border the class points away from (512^2)."""
                    ux, uy = CLASS_DIR[cls]
                    x1 = 0 if ux > 0 else 511 if ux < 0 else 256
                    y1 = 0 if uy > 0 else 511 if uy < 0 else 256
                    d = [_class_point(cls, 360, 0), _class_point(cls, 200, m)]
                    return Built(512, None, [step(d if order == "fwd" else d[::-1], x1, y1, 300.0, 256)])
            _mk()


for _cls in range(4):
    for _ord in ("fwd", "rev", "shuffled"):
        def _mk(cls=_cls, order=_ord):
            @case("fan_c%d_%s" % (cls, order), "lone", "fan")
            def _fan():
                """A fan of one class: minor end offsets -40 .. 40 in uneven steps at major distances 150 .. 250, holes of half
                width 100: neighbours a fraction of a bucket to a dozen buckets apart, the outermost in the first and the last
                bucket any ray of the fan has."""
                ux, uy = CLASS_DIR[cls]
                x1 = 0 if ux > 0 else 511 if ux < 0 else 256
                y1 = 0 if uy > 0 else 511 if uy < 0 else 256
                minors = [-40, -39, -30, -29, -28, -12, -11, -10, -3, -2, -1, 0, 0, 1, 2, 4, 7, 11, 16, 22, 29, 37, 40]
                d = [_class_point(cls, 150 + 9 * (k % 12), m) for k, m in enumerate(minors)]
                if order == "rev":
                    d = d[::-1]
                elif order == "shuffled":
                    d = [d[k] for k in np.random.default_rng(cls).permutation(len(d))]
                return Built(512, None, [step(d, x1, y1, 200.0, 256)])
        _mk()


for _q, (_sx, _sy) in enumerate(((1, 1), (-1, 1), (-1, -1), (1, -1))):
    def _mk(q=_q, sx=_sx, sy=_sy):
        @case("diagonal_shared_q%d" % q, "lone", "diagonal")
        def _diag():
            """The two classes of a quadrant on its diagonal: (201, 200) and (200, 201) draw the diagonal's pixels out to step 100,
            far beyond the step from which either is alone in its class; the same in the opposite quadrant."""
            d = [(sx * 201, sy * 200), (sx * 200, sy * 201), (-sx * 200, -sy * 201), (-sx * 201, -sy * 200)]
            return Built(512, None, [step(d, 256, 256, 60.0, 128)])
    _mk()


GAP_POINTS = {1: (430, 1), 10: (300, 6), 11: (281, 6), 12: (300, 7), 40: (293, 23)}     # partner end points for exact bucket gaps (hole half width 211)


for _cls in range(4):
    for _k in sorted(GAP_POINTS):
        for _ord in ("fwd", "rev"):
            def _mk(cls=_cls, k=_k, order=_ord):
                @case("gap_c%d_b%d_%s" % (cls, k, order), "lone", "bucket_gap")
                def _gap():
                    """Two rays of one class exactly k slope buckets apart -- 1, 10 and 11 are inside the eleven buckets the lone-ray
                    rule looks at (ALONE_REACH), 12 and 40 outside: the partner is not seen and the gap counts as ten buckets.  The
                    axis ray (200, 0) is inside its V all along (hole half width 211), the partner from step 90 or 212 on: where
                    they share a pixel the order shows (quality 128)."""
                    ux, uy = CLASS_DIR[cls]
                    x1 = 0 if ux > 0 else 511 if ux < 0 else 256
                    y1 = 0 if uy > 0 else 511 if uy < 0 else 256
                    d = [_class_point(cls, 200, 0), _class_point(cls, *GAP_POINTS[k])]
                    return Built(512, None, [step(d if order == "fwd" else d[::-1], x1, y1, 422.0, 128)])
            _mk()


@case("gap_above_inverse", "lone", "above_inverse")
def _gap_above_inverse():
    """Slopes 0 and 5 / 495 = 1 / 99: just above 1 / 100 -- the two rays share no pixel at offset 100 or beyond, and from step 102 on
    each is alone."""
    return Built(512, None, [step([(510, 0), (494, 5)], 0, 256, 2.0, 128), step([(494, 5), (510, 0)], 0, 200, 2.0, 128)])


for _name, _pts in (("below", ((999, 1), (1000, 1))), ("above", ((998, 1), (999, 1)))):
    def _mk(name=_name, p=_pts):
        @case("cutoff_%s" % name, "lone", "cutoff")
        def _cutoff():
            """Slopes 1 / 1000 and 1 / 1001 (gap 0.999e-6, below the rule's 1e-6 cut-off: never alone) and 1 / 999 and 1 / 1000 (gap
            1.001e-6, above it: alone from 1 / g on, which the 11-bit field holds as 'never' too); 2048^2 map."""
            return Built(2048, None, [step(list(p), 0, 1024, 2.0, 128), step(list(p)[::-1], 0, 1000, 2.0, 128)])
    _mk()


@case("bucket_ends", "lone", "bucket_ends")
def _bucket_ends():
    """Rays in bucket 0 and bucket 1023 of each class, where the rule's window of eleven buckets either side is clamped to the class:
    the exact diagonals (y major, slope -1 and +1) and x-major rays of slope -+1198 / 1199, each with a neighbour a few buckets in;
    2048^2 map, robot in the centre."""
    d = []
    for sx in (1, -1):
        for sy in (1, -1):
            d += [(sx * 1198, sy * 1197), (sx * 1198, sy * 1190), (sx * 800, sy * 800), (sx * 790, sy * 800)]
    return Built(2048, None, [step(d, 1024, 1024, 2.0, 128), step(d[::-1], 1024, 1024, 2.0, 200)])


@case("pair_plus_2", "lone", "plus_2")
def _pair_plus_2():
    """Clipped lengths 510 and 365, both of minor length 11 (slopes 0.0216 and 0.0301: 1 / g = 116.6): the two rays share the pixel at
    step 116, which is the very step from which they would be alone without the rule's + 2; both below their V there, quality 128:
    one blend and two differ.  In both orders, from column 0 of a 512^2 map."""
    d = [(509, 11), (364, 11)]
    return Built(512, None, [step(d, 0, 256, 2.0, 128), step(d[::-1], 0, 200, 2.0, 128)])


@case("pair_dxc_2047", "lone", "xalone_field")
def _pair_2047():
    """dxc = 2047 and slopes one unit of sdyc apart: 1 / g is 2047, the 11-bit field's 'never'; robot in column 0 of a 2048^2 map."""
    d = [(2046, 0), (2046, 1), (2046, 3)]
    return Built(2048, None, [step(d, 0, 1024, 2.0, 256), step(d[::-1], 0, 1000, 1000.0, 256)])


# ---- arcs ---------------------------------------------------------------------------------------------------------------------------
@case("arc_margin", "arcs", "arc_margin")
def _arc_margin():
    """1080 rays (rB 12: margin 1/2 + 8/12 + 0.02 octants): from a robot twelve pixels from the east border and fourteen from the
    north one, long rays in every direction -- the clip cuts them to a dozen pixels and moves their class and slope away from the
    float direction the selection goes by."""
    rng = np.random.default_rng(12)
    d = [(int(x), int(y)) for x, y in rng.integers(-200, 201, (1080, 2)) if max(abs(x), abs(y)) > 20][:1000]
    d += [(150, k) for k in range(-40, 40)]
    return Built(256, None, [step(d[:1080], 243, 241, 30.0, 77)])


def direction_point(u, D):
    """An integer end point at major distance D whose direction coordinate is about u (the inverse of k2_arc_member's u)."""
    u = u % 8.0
    if u < 2:
        return (D, int(round((u - 1) * D)))
    if u < 4:
        return (int(round((3 - u) * D)), D)
    if u < 6:
        return (-D, int(round((5 - u) * D)))
    return (int(round((u - 7) * D)), -D)


@case("arc_edge", "arcs", "arc_edge")
def _arc_edge():
    """1080 rays (rB 12: an octant's sector workgroups select the rays within 1/2 + 8/12 + 0.02 = 1.18667 octants of its centre).  For
    every octant and either side: five rays of major length 150 whose float direction steps across the margin's edge, one minor pixel
    (1/150 octant) at a time -- some selected, some not, none of the latter draws a pixel of the octant from offset rB on; and rays from
    the octant before that do draw its pixel at offset exactly rB (the axis' and the diagonal's pixels belong to the octant that
    begins there)."""
    d = []
    for k in range(8):
        for side in (-1, 1):
            edge = k + 0.5 + side * (0.5 + 8.0 / 12.0 + 0.02)
            d += [direction_point(edge + e / 150.0, 150) for e in (-2, -1, 0, 1, 2)]
        d += [direction_point(k - 1.0 / 40.0, 40), direction_point(k - 1.0 / 13.0, 13)]
    d += filler(1080 - len(d), np.random.default_rng(16), 3, 60)
    return Built(512, None, [step(d, 256, 256, 2.0, 128)])


@case("arc_need", "arcs", "arc_need")
def _arc_need():
    """The ray that needs the widest margin an enumeration of clipped rays found (tests/test_k2_cases_cpu.py): robot 31 pixels from
    the east border in the top row of a 64^2 map, end point (-31, -29), hole half width 4.5 -- the truncations put the integer ray
    1.42 / x octants from its float direction at step x (the clipped ray is the exact diagonal, whose pixels are octant 6's; the float
    direction lies in octant 5).  Scans of 1981, 2000 and 2048 rays (rB = 23, the only one of the default build at which the ray needs more than 1 / rB), the ray first, last and
    in the middle; the other rays are short and point east."""
    st = []
    for R, k in ((1981, 0), (2000, 1000), (2048, 2047)):
        f = [(2 + j % 5, (j % 3) - 1) for j in range(R - 1)]
        st.append(step(f[:k] + [(-31, -29)] + f[k:], 32, 63, 9.0, 128))
    return Built(64, None, st)


@case("arc_class_border", "arcs", "class_border")
def _arc_border():
    """Rays whose float direction lies a hair from a diagonal or an axis, so that the truncations (:529-530) and the clip put them
    into the other class; 400 rays, rB 5."""
    d = []
    for a in (13, 30, 57, 100):
        for e in (-1, 0, 1):
            d += [(sx * a, sy * (a + e)) for sx in (1, -1) for sy in (1, -1)] + [(sx * a, e) for sx in (1, -1)] + [(e, sy * a) for sy in (1, -1)]
    d = (d * 5)[:400]
    return Built(128, None, [step(d, 64, 64, 3.0, 77), step(d, 120, 9, 3.0, 77)])


for _hw, _name in ((15998.0, "below"), (16000.0, "at"), (-2.0, "negative")):
    def _mk(hw=_hw, name=_name):
        @case("arc_hole_%s" % name, "arcs", "hole_width")
        def _hole():
            """Hole half width just below 8000 pixels (arcs on), at 8000 and negative (arcs off); 200 rays."""
            d = filler(200, np.random.default_rng(13), 3, 40)
            return Built(128, None, [step(d, 64, 64, hw, 77)])
    _mk()


for _n in (848, 849):
    def _mk(n=_n):
        @case("own_%d" % n, "arcs", "own_cap")
        def _own():
            """Exactly n rays of octant 1 reach beyond the zone (zone 128 at 1030 rays): the own list's records lie side by side
            up to 848 rays."""
            d = [(140 + (j % 50), 1 + (j * 7) % 120) for j in range(n)]
            d += filler(1030 - n, np.random.default_rng(14))
            return Built(512, None, [step(d, 256, 256, 2.0, 77)])
    _mk()


@case("octants_empty", "arcs", "empty_octants")
def _octants_empty():
    """Rays in octants 1 and 6 only."""
    d = [(100 + j % 20, 3 + j % 60) for j in range(150)] + [(-(3 + j % 60), -(100 + j % 20)) for j in range(150)]
    return Built(256, None, [step(d, 128, 128, 2.0, 77)])


# ---- the V profile ---------------------------------------------------------------------------------------------------------------
DERRORV = (1, 2, 32750, 32751, 65499, 65500, 65501)


@case("v_derrorv_small", "vprofile", "derrorv")
def _v_small():
    """derrorv 1 and 2 (hole widths 2 and 4 along the axes) with lim2 = -1, 0, 1 (obstacles at derrorv - 1, derrorv, derrorv + 1)."""
    st = []
    for h in (1, 2):
        d = [(ux * r, uy * r) for r in (h - 1, h, h + 1, 9) if r > 0 for ux, uy in DIRS8]
        st.append(step(d, 16, 16, 2.0 * h, 128))
    return Built(32, start_pattern(32), st)


for _d in DERRORV[2:]:
    def _mk(dv=_d):
        @case("v_derrorv_%d" % dv, "vprofile", "derrorv")
        def _v_large():
            """derrorv = dv along the four axes (hole width 2 dv: within the range the closed form is used for); the whole clipped
            ray lies in the descending half, where incv = -65500 / dv is -2, -1 or 0 -- a flat V at 65501."""
            d = [(5, 0), (-5, 0), (0, 5), (0, -7), (3, 0)]
            return Built(64, start_pattern(64), [step(d, 31, 33, 2.0 * dv, 128)])
    _mk()


@case("v_lim1_clipped", "vprofile", "lim1")
def _v_lim1():
    """lim1 (the obstacle's step) before, at and beyond the clipped end: obstacles 3 short of the border, on it and 3 past it."""
    d = []
    for ux, uy in DIRS8:
        for r in (17, 20, 23):
            d.append((ux * r, uy * r))
    return Built(41, None, [step(d, 20, 20, 8.0, 128)])


@case("v_ties", "vprofile", "ties")
def _v_ties():
    """dx == dy ties and dx = dy +- 1 in every quadrant, at three lengths."""
    d = []
    for a in (3, 10, 25):
        for e in (-1, 0, 1):
            d += [(sx * a, sy * (a + e)) for sx in (1, -1) for sy in (1, -1)]
    return Built(64, None, [step(d, 32, 32, 4.0, 128)])


for _S in (8, 63, 64, 65, 300):
    def _mk(S=_S):
        @case("borders_%d" % S, "vprofile", "borders", "sizes")
        def _borders():
            """From the centre, from every corner and from the middle of every border (rows and columns 0 and size - 1): end points
            on, one past and far past each border and corner.  300: rows that are not whole 16-byte units."""
            st = []
            for rx, ry in ((S // 2, S // 2), (0, 0), (S - 1, 0), (0, S - 1), (S - 1, S - 1), (S // 2, 0), (S // 2, S - 1), (0, S // 2), (S - 1, S // 2)):
                d = []
                for ux, uy in DIRS8:
                    room = min([S - 1 - rx if ux > 0 else rx if ux < 0 else S] + [S - 1 - ry if uy > 0 else ry if uy < 0 else S])
                    for n in (room - 1, room, room + 1, room + 1000):
                        if n > 0:
                            d.append((ux * n, uy * n))
                    d.append((ux * (room + 1000) + uy * 333, uy * (room + 1000) - ux * 333))
                st.append(step(d, rx, ry, 2.0, 128))
            return Built(S, None, st)
    _mk()


# ---- division width ----------------------------------------------------------------------------------------------------------------
def division_minors(dxc):
    """Minor lengths dyc for which N = 2 dyc x - dxc lands on, one below or one above a multiple of 2 dxc at some step x <= dxc
    (dxc odd: N is odd and never on one)."""
    out = []
    for dyc in (1, 2, 3, dxc // 3, dxc // 2, dxc // 2 + 1, dxc - 2, dxc - 1):
        x = np.arange(1, dxc + 1, dtype=np.int64)
        r = (2 * dyc * x - dxc) % (2 * dxc)
        if ((r == 1) | (r == 2 * dxc - 1) | (r == 0)).any():
            out.append(dyc)
    return out


def division_residues(geo):
    """Per valid ray the set of residues N mod 2 dxc, N = 2 dyc x - dxc over its steps, restricted to {0, 1, 2 dxc - 1}."""
    out = []
    for r in geo[geo["valid"] == 1]:
        dxc, dyc = int(r["dxc"]), int(r["dyc"])
        x = np.arange(1, dxc + 1, dtype=np.int64)
        res = (2 * dyc * x - dxc) % (2 * dxc)
        out.append({("on" if v == 0 else "above" if v == 1 else "below") for v in np.unique(res[(res <= 1) | (res == 2 * dxc - 1)])})
    return out


@case("division_16384", "division", "big")
def _division():
    """A 16 384^2 map (arcs on, int arithmetic): rays of dxc = 16383 (N odd: one below and one above multiples of 2 dxc) and 16382 (on
    them) from the four corners, both major axes.  The end points are tried at the chosen minor length and one short of it (the hole's
    extension adds a pixel to steep rays only); the rays whose dyc is the chosen one are kept."""
    S = BIG
    st = []
    for cx, cy in ((0, 0), (S - 1, 0), (0, S - 1), (S - 1, S - 1)):
        sx, sy = (1 if cx == 0 else -1), (1 if cy == 0 else -1)
        d, want = [], []
        for major in (S - 2, S - 3):
            for m in division_minors(major + 1):
                for y in (m, m - 1):
                    d += [(sx * major, sy * y), (sx * y, sy * major)]
                    want += [(major + 1, m)] * 2
        g = geometry(S, step(d, cx, cy, 2.0, 128))
        keep = [p for p, w, r in zip(d, want, g) if r["valid"] and (int(r["dxc"]), int(r["dyc"])) == w]
        st.append(step(keep, cx, cy, 2.0, 128))
    return Built(S, None, st)


@case("arc_sane_16384", "arcs", "sane", "big")
def _arc_sane():
    """|pose| and |point| either side of 16 000 on a 16 384^2 map: robot at 15 999 / 16 001, points of 15 999 and 16 001."""
    S = BIG
    d = [(-15999, -100), (-16001, -100), (-100, -15999), (-100, -16001), (50, 60), (-300, 20), (-15999, -15999), (-16001, -16001)]
    d += filler(100, np.random.default_rng(15), 3, 200)
    return Built(S, None, [step(d, 15999, 15999, 2.0, 128), step(d, 16001, 16001, 2.0, 128), step(d, 16001, 15999, 2.0, 128)])
