"""CPU-side checks of the localisation step's interface (slamhip_hs_mcl_set / _step / _get, slamhip_hsproc_mcl_step,
slamhip_debug_mcl_step, slamhip_debug_mcl_table) and the restatement of its definition (include/slamhip.h, slamhip_hs_mcl_step,
steps 1 - 7) that tests/test_gpu_hector_mcl.py compares the device with.

The restatement: np.float32 operations one by one, oracle/np_oracle for Philox, the deterministic sin / cos and the Matrix3x2
product, np.rint for the cells, Python integers for costs, weights, sums, the prefix sum and the comb, bisect for the ancestors, and
a field handed in as a plain array (here the brute-force field of test_hs_dfield_abi).  It shares nothing with hs_mcl.h, whose text
the hook and the kernels run.  Every comparison is == on integers and on the bit patterns of the floats."""
import bisect
import ctypes as C
import math
import os
import re

import np_oracle as npo
import numpy as np
import pytest

import test_hs_dfield_abi as D
import test_hs_trace_abi as T

ROOT = D.ROOT
F = np.float32
LIMIT = F(16777216.0)
ZS = F(math.sqrt(3.0 / (2 ** 32 - 1)))                                     # (the binary32 nearest to the real root)
SYMBOLS = ("slamhip_hs_mcl_set", "slamhip_hs_mcl_step", "slamhip_hs_mcl_get", "slamhip_hsproc_mcl_step", "slamhip_debug_mcl_step",
           "slamhip_debug_mcl_table")
SUMMARY_FIELDS = ["W", "A", "Q", "key_best", "sum_hx", "sum_hy", "sum_hc", "sum_hs", "cost_min", "cost_max", "resampled", "n_distinct",
                  "n_unplaced", "n_particles"]
M32_MASK = 0xFFFFFFFF


def iroot64(n):
    """floor(n ** (1 / 64)) for a Python integer."""
    lo, hi = 0, 1 << (n.bit_length() // 64 + 1)
    while lo < hi:
        m = (lo + hi + 1) // 2
        if m ** 64 <= n:
            lo = m
        else:
            hi = m - 1
    return lo


TABLE = [min(2 ** 32 - 1, iroot64(2 ** (2048 - f))) for f in range(64)]


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def np_noise(N, seed, stream):
    """Step 1 -> (N, 3) float32."""
    i = np.arange(N, dtype=np.uint64)
    key = (seed & M32_MASK, (seed >> 32) & M32_MASK)
    words = []
    for j in (0, 1):
        ctr = np.stack([i, np.full(N, j, np.uint64), np.full(N, stream & M32_MASK, np.uint64), np.full(N, (stream >> 32) & M32_MASK, np.uint64)], -1)
        words.append(npo.philox4x32_10(ctr, key).astype(np.int64))
    b = np.concatenate(words, 1)                                           # (N, 8)
    halves = np.stack([b & 0xFFFF, b >> 16], 2).reshape(N, 16)             # word 0 low, word 0 high, word 1 low, ...
    return np.stack([(halves[:, 4 * m:4 * m + 4].sum(1) - 131070).astype(F) * ZS for m in range(3)], 1)


def np_predict(particles, spec, z):
    """Step 2 -> (N, 3) float32."""
    p = np.asarray(particles, F).reshape(-1, 3)
    d, sg, fo = (np.asarray(spec[k], F) for k in ("delta", "sigma", "frame_offset"))
    ex = d[0] + sg[0] * z[:, 0]; ey = d[1] + sg[1] * z[:, 1]; eth = d[2] + sg[2] * z[:, 2]
    s, c = npo.det_sincos(p[:, 2])
    x = (p[:, 0] + fo[0]) + (c * ex - s * ey)
    y = (p[:, 1] + fo[1]) + (s * ex + c * ey)
    out = np.stack([x, y, p[:, 2] + eth], 1)
    assert out.dtype == np.float32 and ex.dtype == np.float32
    return out


def np_cost(field, rect, const, stm, pose, xy, r):
    """Step 3 for one pose: `field` covers rect = (x0, y0, w, h), which contains E; `const` holds outside."""
    xy = np.asarray(xy, F).reshape(-1, 2)
    t = T.np_transform(stm, pose)
    if t is None:
        return xy.shape[0] * r * r
    with np.errstate(over="ignore", invalid="ignore"):
        exf, eyf = t.transform(xy[:, 0], xy[:, 1])
        assert exf.dtype == np.float32
        ok = (np.abs(exf) < LIMIT) & (np.abs(eyf) < LIMIT)
        ex = np.where(ok, np.rint(exf), 0).astype(np.int64); ey = np.where(ok, np.rint(eyf), 0).astype(np.int64)
    x0, y0, w, h = rect
    inside = ok & (ex >= x0) & (ex < x0 + w) & (ey >= y0) & (ey < y0 + h)
    v = np.full(xy.shape[0], const, np.int64)
    v[inside] = field[ey[inside] - y0, ex[inside] - x0]
    v[~ok] = r * r
    return int(v.sum())


def np_weight(accp, beta):
    e = (min(accp, 2 ** 32 - 1) * beta) >> 16
    k, f = e >> 6, e & 63
    return 0 if k >= 32 else TABLE[f] >> k


def np_mcl_step(field, rect, const, stm, xy, particles, acc, spec):
    """Steps 1 - 7 -> (particles (N, 3) float32, acc list, ancestors list, summary dict, costs list).  spec: a dict, or a
    capi.MCL_SPEC record."""
    p = np.asarray(particles, F).reshape(-1, 3)
    N = p.shape[0]
    r, beta, n_eff_min = int(spec["radius"]), int(spec["beta"]), int(spec["n_eff_min"])
    z = np_noise(N, int(spec["seed"]), int(spec["stream"]))
    with np.errstate(over="ignore", invalid="ignore"):
        pred = np_predict(p, spec, z)
        cost = [np_cost(field, rect, const, stm, pred[i], xy, r) for i in range(N)]
        a = [(int(acc[i]) if acc is not None else 0) + cost[i] for i in range(N)]
        min_a = min(a)
        accp = [v - min_a for v in a]
        w = [np_weight(v, beta) for v in accp]
        h = [v >> 20 for v in w]
        fx, fy = pred[:, 0] * F(1024.0), pred[:, 1] * F(1024.0)
        s2, c2 = npo.det_sincos(pred[:, 2])
        placed = (np.abs(fx) < F(2147483648.0)) & (np.abs(fy) < F(2147483648.0)) & np.isfinite(c2) & np.isfinite(s2)
        ix, iy = np.rint(fx), np.rint(fy)
        ic, is_ = np.rint(c2 * F(16384.0)), np.rint(s2 * F(16384.0))
    S = dict(W=sum(w), A=sum(h), Q=sum(v * v for v in h), key_best=min((a[i] << 16) | i for i in range(N)), cost_min=min(cost), cost_max=max(cost),
             n_unplaced=int((~placed).sum()), n_particles=N)
    for name, arr in (("sum_hx", ix), ("sum_hy", iy), ("sum_hc", ic), ("sum_hs", is_)):
        S[name] = sum(h[i] * int(arr[i]) for i in range(N) if placed[i])
    S["resampled"] = int(S["A"] * S["A"] < n_eff_min * S["Q"])
    if not S["resampled"]:
        S["n_distinct"] = N
        return pred, accp, list(range(N)), S, cost
    Cs, run = [], 0
    for v in w:
        run += v
        Cs.append(N * run)
    seed, stream = int(spec["seed"]), int(spec["stream"])
    rr = int(npo.philox4x32_10(np.array([0, 2, stream & M32_MASK, (stream >> 32) & M32_MASK], np.uint64), (seed & M32_MASK, (seed >> 32) & M32_MASK))[0])
    u = ((S["W"] >> 16) * rr) >> 16
    anc = [bisect.bisect_right(Cs, k * S["W"] + u) for k in range(N)]       # the least i with N * C_i > T_k
    assert max(anc) < N
    S["n_distinct"] = len(set(anc))
    return pred[anc], [0] * N, anc, S, cost


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def check(got, want, tag=None):
    """(particles, acc, ancestors, summary) of the library against np_mcl_step's first four."""
    gp, ga, gk, gs = got
    wp, wa, wk, ws = want[:4]
    for f in SUMMARY_FIELDS:
        assert int(gs[f]) == ws[f], (tag, f, int(gs[f]), ws[f])
    assert gk.tolist() == wk, (tag, "ancestors")
    assert [int(v) for v in ga] == wa, (tag, "acc")
    assert np.array_equal(bits(gp), bits(wp)), (tag, "particles", np.argwhere(bits(gp) != bits(wp))[:4].tolist())


def spec_dict(rec):
    r = rec[0] if rec.shape else rec
    return {k: (np.array(r[k]) if k in ("delta", "sigma", "frame_offset") else int(r[k])) for k in rec.dtype.names}


# ---- the map and the scan ----------------------------------------------------------------------------------------------------------
CW, CH = 96, 80
CELL = F(0.1)
STM = F(1.0) / CELL
TRUTH = np.array([4.6, 4.1, 0.3], F)
ROOM = (12, 9, 83, 69)                                                     # the walls' cells: x0, y0, x1, y1


def room_classes():
    """96 x 80: unknown space, a room of free cells with walls of occupied cells, a pillar, a stretch of wall not yet seen."""
    c = np.zeros((CH, CW), np.uint8)
    x0, y0, x1, y1 = ROOM
    c[y0:y1 + 1, x0:x1 + 1] = 1
    c[y0 + 1:y1, x0 + 1:x1] = 2
    c[30:34, 50:54] = 1
    c[y0, 40:52] = 0
    return c


def room_scan(n, pose=TRUTH, room_m=None):
    """n points on the room's walls (room_m = (x0, y0, x1, y1) in metres; None: ROOM), evenly along the perimeter, in the robot's frame
    at `pose` (float64 geometry, rounded once)."""
    x0, y0, x1, y1 = room_m if room_m is not None else tuple(v * float(CELL) for v in ROOM)
    per = 2 * ((x1 - x0) + (y1 - y0))
    s = (np.arange(n) + 0.37) * per / n
    wx = np.where(s < x1 - x0, x0 + s, np.where(s < x1 - x0 + y1 - y0, x1, np.where(s < 2 * (x1 - x0) + y1 - y0, x1 - (s - (x1 - x0) - (y1 - y0)), x0)))
    wy = np.where(s < x1 - x0, y0, np.where(s < x1 - x0 + y1 - y0, y0 + s - (x1 - x0), np.where(s < 2 * (x1 - x0) + y1 - y0, y1, y1 - (s - 2 * (x1 - x0) - (y1 - y0)))))
    dx, dy, th = wx - float(pose[0]), wy - float(pose[1]), float(pose[2])
    return np.stack([math.cos(th) * dx + math.sin(th) * dy, -math.sin(th) * dx + math.cos(th) * dy], 1).astype(F)


def cloud(N, seed, spread=(0.5, 0.5, math.radians(20.0)), centre=TRUTH, outliers=True):
    """N particles around `centre`; from N = 63 on, three that leave the map: far outside E, past 2^24 cells, past 2^31 / 1024 m."""
    rng = np.random.default_rng([seed, N])
    p = (np.asarray(centre, np.float64) + rng.uniform(-1.0, 1.0, (N, 3)) * np.asarray(spread)).astype(F)
    if outliers and N >= 63:
        p[5] = (500.0, -300.0, 1.0); p[17] = (2.0e6, 4.0, -2.0); p[40] = (4.0, -3.0e6, 0.5)
    return p


@pytest.fixture(scope="module")
def capi():
    import slam.net_amd.build as b
    b.build()
    import slam.net_amd.capi as capi
    return capi


@pytest.fixture(scope="module")
def fields():
    """The brute-force field of the room over E and a margin, per (site_mask, r): computed once, read-only."""
    cls = room_classes()
    cls.setflags(write=False)
    out = {}
    for mask in (2, 3):
        for r in (1, 8):
            rect = (-r - 2, -r - 2, CW + 2 * r + 4, CH + 2 * r + 4)
            f = D.np_field_brute(cls, mask, r, rect)
            f.setflags(write=False)
            out[mask, r] = (f, rect, 0 if mask & 1 else r * r)
    return cls, out


# ---- the surface -------------------------------------------------------------------------------------------------------------------
def test_surface(capi):
    L = capi.lib()
    header = open(os.path.join(ROOT, "include", "slamhip.h")).read()
    native = open(os.path.join(ROOT, "bindings", "csharp", "SlamHip", "SlamHip.Native.cs")).read()
    for n in SYMBOLS:
        assert hasattr(L, n) and n in L._signatures and re.search(r"\b%s\s*\(" % n, header) and n in native, n
    assert [len(L._signatures[n][1]) for n in SYMBOLS] == [3, 3, 5, 6, 14, 1]
    sp, sm = capi.MCL_SPEC, capi.MCL_SUMMARY
    assert sp.itemsize == 72 and [sp.fields[f][1] for f in sp.names] == [0, 4, 8, 12, 16, 28, 40, 48, 52, 56, 64]
    assert sm.itemsize == 96 and list(sm.names) == SUMMARY_FIELDS and [sm.fields[f][1] for f in sm.names] == list(range(0, 80, 8)) + [80, 84, 88, 92]
    for name, fields_ in (("spec", list(sp.names)), ("summary", SUMMARY_FIELDS)):
        m = re.search(r"typedef struct slamhip_mcl_%s \{(.*?)\} slamhip_mcl_%s;\s*/\*(.*?)\*/" % (name, name), header, re.S)
        body = re.sub(r"\[\d+\]", "", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
        assert re.findall(r"(\w+)\s*[,;]", body) == fields_, name           # the header's members, in order
        assert "no padding" in m.group(2) and ("72 bytes" if name == "spec" else "96 bytes") in m.group(2)
    assert "struct MclSpec" in native and "struct MclSummary" in native
    assert "SLAMHIP_K_COUNT = 10" in header                                 # no new timing class
    import slam.net_amd.build as b
    import slam.net_amd.hector as hm
    for n in ("mcl_set", "mcl_step", "mcl_get"):
        assert hasattr(hm.MapRepMultiMap, n)
    assert hasattr(hm.HectorSLAMProcessor, "LocaliseInit") and hasattr(hm.HectorSLAMProcessor, "LocaliseStep")
    assert "hs_mcl.hip" in b.SOURCES and "hs_mcl.h" in b.HEADERS and "philox.h" in b.HEADERS
    assert float(ZS) == float.fromhex("0x1.bb67aep-16") and "0x1.bb67aep-16f" in header
    assert "0x1.bb67aep-16f" in open(os.path.join(b.CSRC, "hs_mcl.h")).read()
    assert capi.mcl_beta(2.0, 1.0) == round(65536 * 64 * math.log2(math.e) / 8.0)


def test_weight_table(capi):
    t = capi.debug_mcl_table()
    assert t.dtype == np.uint32 and t.tolist() == TABLE
    assert TABLE[0] == 2 ** 32 - 1 and TABLE[32] == math.isqrt(2 ** 63) and all(a > b for a, b in zip(TABLE, TABLE[1:])) and TABLE[63] > 2 ** 31


# ---- hook against restatement ------------------------------------------------------------------------------------------------------
def run_both(capi, cls, field, stm, xy, particles, acc, spec, tag):
    got = capi.debug_mcl_step(cls, stm, xy, particles, spec, acc)
    want = np_mcl_step(field[0], field[1], field[2], stm, xy, particles, acc, spec_dict(spec))
    check(got, want, tag)
    return got, want


@pytest.mark.parametrize("r", [1, 8])
@pytest.mark.parametrize("mask", [2, 3])
@pytest.mark.parametrize("n_points", [1, 37, 360])
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 257, 1000])
def test_hook_equals_restatement(capi, fields, N, n_points, mask, r):
    """Three consecutive steps, each from what the last one left, with n_eff_min = 0 (never resample), N + 1 (always) and a middle
    value, in an order that turns with the case: accumulated costs and resampled particles both go through a later step."""
    cls, fs = fields
    case = N + n_points + mask + r
    xy = room_scan(n_points)
    p = cloud(N, case)
    beta = capi.mcl_beta(2.0 if r == 8 else 0.7, max(1.0, n_points / 8.0))
    outcomes = set()
    acc = None
    order = (0, N + 1, N // 2 + 1)
    for step, n_eff_min in enumerate(order[case % 3:] + order[:case % 3]):
        spec = capi.mcl_spec(0, r, (0.05, -0.01, 0.02), (0.02, 0.01, 0.01), beta, n_eff_min, seed=0x1234567890ABCDEF + case, stream=(7 << 32) + step,
                             site_mask=mask)
        got, want = run_both(capi, cls, fs[mask, r], STM, xy, p, acc, spec, (N, n_points, mask, r, step))
        outcomes.add(int(got[3]["resampled"]))
        assert got[3]["resampled"] == (0 if n_eff_min == 0 else 1 if n_eff_min == N + 1 else got[3]["resampled"])
        p, acc = got[0], got[1]
    assert outcomes == {0, 1}                                               # both branches in every case


def test_cases_reach_what_they_are_for(capi, fields):
    """The parametrised cases would prove little if every particle cost the same or no weight ever vanished: on one of them, the
    costs differ, some weights are 0, some lie strictly between, ignored points and unplaced particles occur, and the resampled set
    has fewer distinct ancestors than particles but more than one."""
    cls, fs = fields
    xy = room_scan(360)
    p = cloud(257, 1)
    spec = capi.mcl_spec(0, 8, (0.05, -0.01, 0.02), (0.02, 0.01, 0.01), capi.mcl_beta(2.0, 45.0), 258, seed=5, stream=1)
    got, want = run_both(capi, cls, fs[2, 8], STM, xy, p, None, spec, "reach")
    cost = want[4]
    assert len(set(cost)) > 200 and cost[17] == 360 * 64 and cost[5] == 360 * 64 and min(cost) < 360 * 8
    w = [np_weight(c - min(cost), int(spec["beta"][0])) for c in cost]
    assert w.count(0) >= 3 and sum(1 for v in w if 0 < v < 2 ** 31) > 50
    assert got[3]["n_unplaced"] == 1 and got[3]["resampled"] == 1 and 1 < got[3]["n_distinct"] < 200
    assert 40 not in got[2].tolist() and 17 not in got[2].tolist()


# ---- closed forms ------------------------------------------------------------------------------------------------------------------
def test_equal_costs_resample_to_the_identity(capi, fields):
    """Equal costs: every w is 2^32 - 1 = w, W = N w, C_i = (i + 1) w, T_k = k N w + u with u < N w: N C_i > T_k first holds at
    i = k.  n_eff_min = N + 1 forces the resampling."""
    cls, _ = fields
    for N in (1, 100):
        p = np.tile(TRUTH, (N, 1))
        spec = capi.mcl_spec(0, 8, (0.1, 0.0, 0.0), (0.0, 0.0, 0.0), 1000, N + 1, seed=3, stream=9)
        gp, ga, gk, gs = capi.debug_mcl_step(cls, STM, room_scan(37), p, spec)
        assert gs["resampled"] == 1 and gk.tolist() == list(range(N)) and gs["n_distinct"] == N and gs["W"] == N * (2 ** 32 - 1)
        assert gs["cost_min"] == gs["cost_max"] and not ga.any() and (bits(gp) == bits(gp[0])).all() and gs["A"] == 4095 * N


def test_one_good_particle_takes_all(capi, fields):
    cls, _ = fields
    N, best = 50, 31
    p = np.tile(np.array([500.0, 500.0, 0.0], F), (N, 1))                   # 5000 cells off the map: every point capped
    p[best] = TRUTH
    spec = capi.mcl_spec(0, 8, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 0xFFFFFFFF, N + 1, seed=1, stream=2)
    gp, ga, gk, gs = capi.debug_mcl_step(cls, STM, room_scan(360), p, spec)
    assert gs["cost_max"] == 360 * 64 and gs["cost_min"] < 360 * 2 and gs["W"] == 2 ** 32 - 1 and gs["key_best"] == (int(gs["cost_min"]) << 16) | best
    assert gk.tolist() == [best] * N and gs["n_distinct"] == 1 and gs["resampled"] == 1 and (bits(gp) == bits(TRUTH)).all()


def test_no_resampling_accumulates_renormalised_costs(capi, fields):
    cls, _ = fields
    N = 40
    p = cloud(N, 77, outliers=False)
    xy = room_scan(37)
    kw = dict(seed=11, site_mask=2)
    s1 = capi.mcl_spec(0, 8, (0.03, 0.0, 0.01), (0.01, 0.01, 0.01), 300, 0, stream=1, **kw)
    s2 = capi.mcl_spec(0, 8, (0.03, 0.0, 0.01), (0.01, 0.01, 0.01), 300, 0, stream=2, **kw)
    p1, a1, k1, m1 = capi.debug_mcl_step(cls, STM, xy, p, s1)
    c1 = a1.astype(object) + int(m1["cost_min"])                            # from zero costs: acc' = cost - cost_min
    p2, a2, k2, m2 = capi.debug_mcl_step(cls, STM, xy, p1, s2)              # the second step's own costs, again from zero
    c2 = a2.astype(object) + int(m2["cost_min"])
    q2, b2, j2, n2 = capi.debug_mcl_step(cls, STM, xy, p1, s2, acc=a1)      # ... and chained
    tot = c1 + c2
    assert m1["resampled"] == 0 == n2["resampled"] and k1.tolist() == list(range(N)) == j2.tolist() and n2["n_distinct"] == N
    assert [int(v) for v in b2] == [int(v - min(tot)) for v in tot] and len(set(tot.tolist())) > 5 and np.array_equal(bits(q2), bits(p2))
    assert n2["cost_min"] == m2["cost_min"] and n2["key_best"] >> 16 == min(int(x) + int(y) for x, y in zip(a1, c2))


def test_all_points_ignored_costs_n_r_squared(capi, fields):
    cls, _ = fields
    for n, r in ((37, 8), (360, 1), (1, 255)):
        spec = capi.mcl_spec(0, r, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 100, 0)
        gp, ga, gk, gs = capi.debug_mcl_step(cls, STM, room_scan(n), [[2.0e6, 2.0e6, 0.0]], spec)   # 2e7 cells: past 2^24
        assert gs["cost_min"] == n * r * r == gs["cost_max"] and ga[0] == 0 and gs["W"] == 2 ** 32 - 1 and gs["n_unplaced"] == 0


def test_sigma_zero_is_the_odometry_composition(capi, fields):
    cls, _ = fields
    p = cloud(30, 4, outliers=False)
    d = np.array([0.21, -0.04, 0.11], F); fo = np.array([-1.6, 0.8], F)
    s, c = npo.det_sincos(p[:, 2])
    want = np.stack([(p[:, 0] + fo[0]) + (c * d[0] - s * d[1]), (p[:, 1] + fo[1]) + (s * d[0] + c * d[1]), p[:, 2] + d[2]], 1)
    for seed in (0, 99, 2 ** 63 + 5):
        spec = capi.mcl_spec(0, 8, d, (0.0, 0.0, 0.0), 100, 0, seed=seed, stream=seed * 3, frame_offset=fo)
        gp = capi.debug_mcl_step(cls, STM, room_scan(37), p, spec)[0]
        assert np.array_equal(bits(gp), bits(want)), seed


def test_stream_changes_the_noise_and_repeats(capi, fields):
    cls, _ = fields
    p = cloud(30, 4, outliers=False)
    run = lambda seed, stream: capi.debug_mcl_step(cls, STM, room_scan(37), p, capi.mcl_spec(0, 8, (0.1, 0.0, 0.0), (0.05, 0.05, 0.02), 100, 0,
                                                                                              seed=seed, stream=stream))[0]
    a, b, c, d = run(5, 1), run(5, 2), run(5, 1), run(6, 1)
    assert np.array_equal(bits(a), bits(c)) and (bits(a) != bits(b)).all(1).all() and (bits(a) != bits(d)).all(1).all()
    z = np_noise(4096, 5, 1).astype(np.float64)                             # the variate is what the header says it is
    assert abs(z.mean()) < 0.05 and abs(z.var() - 1.0) < 0.05 and np.abs(z).max() <= 131070 * float(ZS) < 3.47


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(capi, fields):
    cls, _ = fields
    L = capi.lib()
    vp = C.c_void_p
    N = 5
    xy = room_scan(9)
    good = cloud(N, 1, outliers=False)

    def attempt(N=N, n_points=9, cw=CW, ch=CH, stm=float(STM), particles=good, null=None, **kw):
        spec = capi.mcl_spec(0, 8, (0.1, 0.0, 0.0), (0.01, 0.01, 0.01), 100, 2)
        for k, v in kw.items():
            if k in ("delta", "sigma", "frame_offset"):
                spec[k][0][v[0]] = v[1]
            else:
                spec[k] = v
        out_p = np.full((8, 3), 7.0, F); out_a = np.full(8, 7, np.uint64); out_k = np.full(8, 7, np.int32); sm = np.full(96, 7, np.uint8)
        args = dict(cls=cls.ctypes.data_as(vp), pts=xy.ctypes.data_as(vp), part=particles.ctypes.data_as(vp), spec=spec.ctypes.data_as(vp),
                    out_p=out_p.ctypes.data_as(vp), out_a=out_a.ctypes.data_as(vp), out_k=out_k.ctypes.data_as(vp), sm=sm.ctypes.data_as(vp))
        if null:
            args[null] = None
        rc = L.slamhip_debug_mcl_step(args["cls"], cw, ch, C.c_float(stm), args["pts"], n_points, args["part"], None, N, args["spec"], args["out_p"],
                                      args["out_a"], args["out_k"], args["sm"])
        assert (out_p == 7.0).all() and (out_a == 7).all() and (out_k == 7).all() and (sm == 7).all()
        return rc

    bad = good.copy(); bad[3, 1] = np.inf
    nanp = good.copy(); nanp[0, 2] = np.nan
    cases = [dict(level=1), dict(level=-1), dict(world=2), dict(world=-1), dict(site_mask=0), dict(site_mask=8), dict(radius=0), dict(radius=256),
             dict(beta=0), dict(n_eff_min=-1), dict(n_eff_min=N + 2), dict(N=0), dict(N=65537), dict(n_points=0), dict(n_points=7681),
             dict(cw=0), dict(ch=0), dict(stm=0.0), dict(stm=-1.0), dict(stm=float("nan")), dict(stm=float("inf")), dict(particles=bad),
             dict(particles=nanp)]
    cases += [dict([(name, (i, v))]) for name, n in (("delta", 3), ("sigma", 3), ("frame_offset", 2)) for i in range(n) for v in (np.nan, np.inf, -np.inf)]
    cases += [dict(null=k) for k in ("cls", "pts", "part", "spec", "out_p", "out_a", "out_k", "sm")]
    for kw in cases:
        assert attempt(**kw) == capi.ERR_INVALID, kw
        assert L.slamhip_last_error()
    # the same arguments without a fault go through (n_eff_min = N + 1 is the last allowed value)
    spec = capi.mcl_spec(0, 8, (0.1, 0.0, 0.0), (0.01, 0.01, 0.01), 100, N + 1)
    assert capi.debug_mcl_step(cls, STM, xy, good, spec)[3]["resampled"] == 1
    assert L.slamhip_debug_mcl_table(None) == capi.ERR_INVALID
