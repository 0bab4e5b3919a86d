"""CPU-side checks of the pose-graph relaxation's interface (the slamhip_hs_pg_* calls, slamhip_hs_sig_set_poses and the hooks
slamhip_debug_pg_relax / _pg_sum / _sincos) and the NumPy restatement of its definition (include/slamhip.h, slamhip_hs_pg_relax) that
tests/test_gpu_hector_pg.py compares the device with through the hook.

The restatement (np_sincos, np_wrap, np_sum, np_edges, np_lists, np_relax) shares no text with hs_pg.h and uses elementwise NumPy
operations only -- no einsum, dot or @, which may fuse or reorder: the trig is whole-array Cody-Waite, the tree sum a reshape and
sliced adds, the sums over a node's edges run rank by rank over all nodes at once (the r-th incident edge of every node in one
fancy-indexed add), Jacobians are (E, 3, 3) arrays.  The hook runs hs_pg.h in plain loops.  hook == restatement is asserted with == on
every output; the hook against an independent dense Gauss-Newton (libm trig, numpy.linalg.solve) within the issue's bounds.  No
compute calls on a device."""
import ctypes as C
import itertools
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("slamhip_hs_pg_set", "slamhip_hs_pg_relax", "slamhip_hs_pg_get", "slamhip_hs_pg_residuals", "slamhip_hs_pg_clear",
           "slamhip_hs_sig_set_poses", "slamhip_debug_pg_relax", "slamhip_debug_pg_sum", "slamhip_debug_sincos")
D = np.float64
TWO_PI = D(6.283185307179586)


@pytest.fixture(scope="module")
def capi():
    import slam.net_amd.build as b
    b.build()
    import slam.net_amd.capi as capi
    return capi


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def np_sincos(x):
    """Rule 2 -> (sin, cos), binary64, whole arrays."""
    x = np.asarray(x, D)
    k = np.rint(x * D(6.36619772367581382433e-01))
    r = ((x - k * D(1.57079632673412561417e+00)) - k * D(6.07710050630396597660e-11)) - k * D(2.02226624879595063154e-21)
    z = r * r
    ps = D(8.33333333332248946124e-03) + z * (D(-1.98412698298579493134e-04) + z * (D(2.75573137070700676789e-06) + z * (
        D(-2.50507602534068634195e-08) + z * D(1.58969099521155010221e-10))))
    sn = r + (z * r) * (D(-1.66666666666666324348e-01) + z * ps)
    pc = z * (D(4.16666666666666019037e-02) + z * (D(-1.38888888888741095749e-03) + z * (D(2.48015872894767294178e-05) + z * (
        D(-2.75573143513906633035e-07) + z * (D(2.08757232129817482790e-09) + z * D(-1.13596475577881948265e-11))))))
    cs = D(1.0) - (D(0.5) * z - z * pc)
    q = k.astype(np.int64) & 3
    return np.choose(q, [sn, cs, -sn, -cs]), np.choose(q, [cs, -sn, -cs, sn])


def np_wrap(a):
    return a - TWO_PI * np.rint(a / TWO_PI)


def np_sum(v):
    """Rule 6: reshape to blocks of 256 and add halves."""
    t = np.asarray(v, D).ravel()
    while True:
        nb = max(-(-t.shape[0] // 256), 1)
        a = np.zeros(nb * 256, D)
        a[:t.shape[0]] = t
        a = a.reshape(nb, 256)
        h = 128
        while h >= 1:
            a[:, :h] = a[:, :h] + a[:, h:2 * h]
            h //= 2
        t = a[:, 0].copy()
        if t.shape[0] == 1:
            return t[0]


def np_dot(u, v):
    return np_sum((u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]) + u[:, 2] * v[:, 2])


def np_edges(poses, ij, z, w, wrong=None):
    """Rule 3 over all edges -> (A (E, 3, 3), B (E, 3, 3), r (E, 3), chi2_e (E,))."""
    pi, pj = poses[ij[:, 0]], poses[ij[:, 1]]
    s, c = np_sincos(pi[:, 2])
    dx, dy = pj[:, 0] - pi[:, 0], pj[:, 1] - pi[:, 1]
    ux, uy = c * dx + s * dy, c * dy - s * dx
    dth = (pj[:, 2] - pi[:, 2]) - z[:, 2]
    r = np.stack([ux - z[:, 0], uy - z[:, 1], dth if wrong == "no_wrap" else np_wrap(dth)], axis=1)
    E = ij.shape[0]
    A = np.zeros((E, 3, 3), D); B = np.zeros((E, 3, 3), D)
    A[:, 0, 0] = -c; A[:, 0, 1] = -s; A[:, 0, 2] = -uy if wrong == "uy_sign" else uy
    A[:, 1, 0] = s; A[:, 1, 1] = -c; A[:, 1, 2] = -ux
    A[:, 2, 2] = -1.0
    B[:, 0, 0] = c; B[:, 0, 1] = s
    B[:, 1, 0] = -s; B[:, 1, 1] = c
    B[:, 2, 2] = 1.0
    chi2 = (w[:, 0] * (r[:, 0] * r[:, 0]) + w[:, 1] * (r[:, 1] * r[:, 1])) + w[:, 2] * (r[:, 2] * r[:, 2])
    return A, B, r, chi2


def np_lists(N, ij, wrong=None):
    """Rule 4's order: the incident (edge, side) entries of every node, as a list over the rank r of (nodes, edges, sides) arrays -- the
    r-th entry of every node that has one."""
    E = ij.shape[0]
    node = np.concatenate([ij[:, 0], ij[:, 1]]); edge = np.concatenate([np.arange(E), np.arange(E)]); side = np.concatenate([np.zeros(E, int), np.ones(E, int)])
    order = np.lexsort((side, -edge if wrong == "order" else edge, node))
    node, edge, side = node[order], edge[order], side[order]
    first = np.searchsorted(node, node, side="left")
    rank = np.arange(node.shape[0]) - first
    return [(node[rank == r], edge[rank == r], side[rank == r]) for r in range(int(rank.max()) + 1 if rank.size else 0)]


def np_jtv(J, v):
    """(J^T v)[a] = (J[0][a] v0 + J[1][a] v1) + J[2][a] v2 over a batch."""
    return (J[:, 0, :] * v[:, 0:1] + J[:, 1, :] * v[:, 1:2]) + J[:, 2, :] * v[:, 2:3]


def np_mul(M, v):
    """M v for a batch of symmetric 3 x 3 (n, 3, 3)."""
    return (M[:, :, 0] * v[:, 0:1] + M[:, :, 1] * v[:, 1:2]) + M[:, :, 2] * v[:, 2:3]


def np_relax(poses, fixed, ij, z, w, n_outer, n_cg, lam=0.0, tol=1e-6, wrong=None):
    """Rules 3 - 8 -> (poses, iters as a list of dicts, chi2_final, r, chi2_e)."""
    poses = np.array(poses, D).reshape(-1, 3); ij = np.asarray(ij, np.int64).reshape(-1, 2)
    z = np.asarray(z, D).reshape(-1, 3); w = np.asarray(w, D).reshape(-1, 3)
    N = poses.shape[0]
    fx = np.zeros(N, bool)
    if fixed is None:
        fx[0] = True
    else:
        fx[:] = np.asarray(fixed).astype(bool)
    free = ~fx
    lists = np_lists(N, ij, wrong)
    lam = D(lam); tol = D(tol)
    iters = []
    for _ in range(n_outer):
        A, B, r, chi2e = np_edges(poses, ij, z, w, wrong)
        Dn = np.zeros((N, 3, 3), D); g = np.zeros((N, 3), D)
        Dn[:, 0, 0] = lam; Dn[:, 1, 1] = lam; Dn[:, 2, 2] = lam
        wr = w * r
        for nodes, edges, sides in lists:
            keep = free[nodes]
            nodes, edges, sides = nodes[keep], edges[keep], sides[keep]
            J = np.where((sides == 0)[:, None, None], A[edges], B[edges])
            we = w[edges]
            for a in range(3):
                for b in range(a, 3):
                    T = ((J[:, 0, a] * we[:, 0]) * J[:, 0, b] + (J[:, 1, a] * we[:, 1]) * J[:, 1, b]) + (J[:, 2, a] * we[:, 2]) * J[:, 2, b]
                    Dn[nodes, a, b] = Dn[nodes, a, b] + T
            g[nodes] = g[nodes] + np_jtv(J, wr[edges])
        d00, d01, d02, d11, d12, d22 = Dn[:, 0, 0], Dn[:, 0, 1], Dn[:, 0, 2], Dn[:, 1, 1], Dn[:, 1, 2], Dn[:, 2, 2]
        c00 = d11 * d22 - d12 * d12; c01 = d02 * d12 - d01 * d22; c02 = d01 * d12 - d02 * d11
        c11 = d00 * d22 - d02 * d02; c12 = d01 * d02 - d00 * d12; c22 = d00 * d11 - d01 * d01
        det = (d00 * c00 + d01 * c01) + d02 * c02
        ok = free & (det > 0)
        safe = np.where(ok, det, D(1.0))
        M = np.zeros((N, 3, 3), D)
        for (a, b), cab in (((0, 0), c00), ((0, 1), c01), ((0, 2), c02), ((1, 1), c11), ((1, 2), c12), ((2, 2), c22)):
            M[:, a, b] = np.where(ok, cab / safe, D(0.0)); M[:, b, a] = M[:, a, b]
        g[fx] = 0.0
        x = np.zeros((N, 3), D); res = -g; zv = np_mul(M, res); p = zv.copy()
        rz = np_dot(res, zv); rz0 = rz
        k = 0
        while True:
            if rz <= (tol * tol) * rz0 or rz <= 0:
                stopped = 0
                break
            if k == n_cg:
                stopped = 1
                break
            t = w * (np_mul(A, p[ij[:, 0]]) + np_mul(B, p[ij[:, 1]]))
            q = lam * p
            for nodes, edges, sides in lists:
                J = np.where((sides == 0)[:, None, None], A[edges], B[edges])
                q[nodes] = q[nodes] + np_jtv(J, t[edges])
            q[fx] = 0.0
            pq = np_dot(p, q)
            if not pq > 0:
                stopped = 2
                break
            alpha = rz / pq
            x = x + alpha * p; res = res - alpha * q
            zv = np_mul(M, res)
            rzn = np_dot(res, zv)
            beta = rzn / rz
            p = zv + beta * p
            rz = rzn
            k += 1
        iters.append({"chi2": np_sum(chi2e), "rz0": rz0, "rz": rz, "cg_iters": k, "stopped": stopped})
        new = poses + x
        new[:, 2] = np_wrap(new[:, 2])
        poses = np.where(free[:, None], new, poses)
    _, _, r, chi2e = np_edges(poses, ij, z, w, wrong)
    return poses, iters, np_sum(chi2e), r, chi2e


def same_as_hook(capi, poses, fixed, ij, z, w, n_outer, n_cg, lam=0.0, tol=1e-6, wrong=None):
    """hook == restatement on every output -> the hook's outputs (with wrong: whether they are all equal)."""
    hp, hit, hfin, hr, hc = capi.debug_pg_relax(poses, fixed, ij, z, w, capi.pg_spec(n_outer, n_cg, lam=lam, tol=tol))
    wp, wit, wfin, wr, wc = np_relax(poses, fixed, ij, z, w, n_outer, n_cg, lam, tol, wrong)
    eq = np.array_equal(hp, wp) and hfin == wfin and np.array_equal(hr, wr) and np.array_equal(hc, wc)
    for o in range(n_outer):
        eq = eq and all(hit[o][f] == wit[o][f] for f in ("chi2", "rz0", "rz", "cg_iters", "stopped"))
    if wrong is not None:
        return eq
    assert eq, (hp - wp, hit, wit, hfin, wfin)
    return hp, hit, hfin, hr, hc


# ---- graphs ----------------------------------------------------------------------------------------------------------------------
def rel(pi, pj):
    """The exact relative pose of j in i's frame, libm trig."""
    c, s = np.cos(pi[2]), np.sin(pi[2])
    dx, dy = pj[0] - pi[0], pj[1] - pi[1]
    return np.array([c * dx + s * dy, c * dy - s * dx, np_wrap(pj[2] - pi[2])])


def compose(pi, zz):
    c, s = np.cos(pi[2]), np.sin(pi[2])
    return np.array([pi[0] + c * zz[0] - s * zz[1], pi[1] + s * zz[0] + c * zz[1], pi[2] + zz[2]])


SIGMA = np.array([0.02, 0.02, 0.01])


def ring(N, seed=7, turn=0.0, wrap=True):
    """The issue's ring: N poses at spacing 0.25 m heading along the tangent, edges (k, k + 1 mod N) = true relative pose + Gaussian
    noise, weights 1 / sigma^2, initial poses by chaining the noisy edges from node 0 -> (poses, ij, z, w)."""
    g = np.random.Generator(np.random.Philox(seed))
    R = 0.25 / (2.0 * np.sin(np.pi / N))
    phi = 2.0 * np.pi * np.arange(N) / N
    true = np.stack([R * np.cos(phi), R * np.sin(phi), phi + np.pi / 2], axis=1)
    ij = np.stack([np.arange(N), (np.arange(N) + 1) % N], axis=1).astype(np.int32)
    z = np.stack([rel(true[i], true[j]) for i, j in ij]) + g.standard_normal((N, 3)) * SIGMA
    w = np.tile(1.0 / SIGMA ** 2, (N, 1))
    start = true[0].copy()
    if turn:
        c, s = np.cos(turn), np.sin(turn)
        start = np.array([c * start[0] - s * start[1], s * start[0] + c * start[1], start[2] + turn])
    poses = [start]
    for k in range(N - 1):
        poses.append(compose(poses[-1], z[k]))
    poses = np.stack(poses)
    if wrap:
        poses[:, 2] = np_wrap(poses[:, 2])
    return poses, ij, z, w


def dense_gauss_newton(poses, ij, z, w, steps=10):
    """The independent solver: dense binary64 Gauss-Newton, libm trig, numpy.linalg.solve, node 0 fixed -> (poses, chi2)."""
    p = np.array(poses, D)
    N, E = p.shape[0], ij.shape[0]

    def residuals(p):
        r = np.zeros((E, 3)); J = np.zeros((3 * E, 3 * N))
        for e, (i, j) in enumerate(ij):
            c, s = np.cos(p[i, 2]), np.sin(p[i, 2])
            dx, dy = p[j, 0] - p[i, 0], p[j, 1] - p[i, 1]
            ux, uy = c * dx + s * dy, c * dy - s * dx
            r[e] = (ux - z[e, 0], uy - z[e, 1], np.arctan2(np.sin(p[j, 2] - p[i, 2] - z[e, 2]), np.cos(p[j, 2] - p[i, 2] - z[e, 2])))
            J[3 * e:3 * e + 3, 3 * i:3 * i + 3] = [[-c, -s, uy], [s, -c, -ux], [0, 0, -1]]
            J[3 * e:3 * e + 3, 3 * j:3 * j + 3] = [[c, s, 0], [-s, c, 0], [0, 0, 1]]
        return r, J
    W = w.reshape(-1)
    for _ in range(steps):
        r, J = residuals(p)
        Jf = J[:, 3:]
        H = Jf.T @ (Jf * W[:, None]); b = -Jf.T @ (W * r.reshape(-1))
        p[1:] += np.linalg.solve(H, b).reshape(-1, 3)
    r, _ = residuals(p)
    return p, float((w * r * r).sum())


def tiny_graph(seed, N, edges):
    g = np.random.Generator(np.random.Philox(seed))
    poses = g.standard_normal((N, 3)) * np.array([2.0, 2.0, 1.0])
    ij = np.array(edges, np.int32).reshape(-1, 2)
    truth = poses + g.standard_normal((N, 3)) * 0.05
    z = np.stack([rel(truth[i], truth[j]) for i, j in ij]) if len(ij) else np.zeros((0, 3))
    w = g.uniform(0.5, 50.0, (ij.shape[0], 3))
    return poses, ij, z, w


# ---- 1. the interface ----------------------------------------------------------------------------------------------------------------
def test_symbols_and_struct_layout(capi):
    L = capi.lib()
    declared = set(capi.declared_symbols())
    for name in SYMBOLS:
        assert name in declared and hasattr(L, name) and name in L._signatures, name
    header = open(os.path.join(ROOT, "include", "slamhip.h")).read()
    for text in ("} slamhip_pg_spec;                     /* 32 bytes */", "} slamhip_pg_iter;                     /* 32 bytes */",
                 "#define SLAMHIP_PG_MAX_NODES (1 << 20)", "#define SLAMHIP_PG_MAX_EDGES (1 << 22)", "increasing EDGE INDEX"):
        assert text in header, text
    assert capi.PG_SPEC.itemsize == 32 and capi.PG_ITER.itemsize == 32
    assert [capi.PG_SPEC.fields[n][1] for n in ("n_outer", "n_cg", "check_every", "reserved", "lambda", "tol")] == [0, 4, 8, 12, 16, 24]
    assert [capi.PG_ITER.fields[n][1] for n in ("chi2", "rz0", "rz", "cg_iters", "stopped")] == [0, 8, 16, 24, 28]
    for n, off in (("n_outer", 0), ("n_cg", 4), ("check_every", 8), ("reserved", 12), ("lambda", 16), ("tol", 24)):
        assert re.search(r"%s;\s*/\* offset %d:" % (n, off), header), n
    # the library's own view of the spec: a record whose check_every is 0 is refused, one whose tol sits at offset 24 is used
    poses, ij, z, w = tiny_graph(1, 2, [(0, 1)])
    raw = np.zeros(32, np.uint8)
    raw[0:4] = np.array([1], np.int32).view(np.uint8); raw[4:8] = np.array([3], np.int32).view(np.uint8); raw[8:12] = np.array([1], np.int32).view(np.uint8)
    raw[24:32] = np.array([2.0], D).view(np.uint8)                        # tol = 2: rz0 <= 4 rz0 stops before iteration 0
    spec = raw.view(capi.PG_SPEC)
    _, it, _, _, _ = capi.debug_pg_relax(poses, None, ij, z, w, spec)
    assert it[0]["cg_iters"] == 0 and it[0]["stopped"] == 0


def test_csharp_and_build_list():
    native = open(os.path.join(ROOT, "bindings", "csharp", "SlamHip", "SlamHip.Native.cs")).read()
    for name in SYMBOLS:
        if not name.startswith("slamhip_debug"):
            assert re.search(r"static extern int %s\(" % name, native), name
    proc = open(os.path.join(ROOT, "bindings", "csharp", "SlamHip", "HectorSLAM", "HectorSLAMProcessor.Hip.cs")).read()
    assert "RelaxKeyframes(" in proc
    import slam.net_amd.build as b
    assert "hs_pg.hip" in b.SOURCES and "hs_pg.h" in b.HEADERS


def raw_relax(capi, poses, fixed, ij, z, w, spec):
    """The hook called with sentinel-filled outputs -> (return code, whether anything was written)."""
    p = np.array(poses, D).reshape(-1, 3); before = p.copy()
    e = np.array(ij, np.int32).reshape(-1, 2); zz = np.array(z, D).reshape(-1, 3); ww = np.array(w, D).reshape(-1, 3)
    fx = None if fixed is None else np.asarray(fixed, np.uint8)
    iters = np.full(64 * 4, -7.25, D); fin = np.full(1, -7.25, D); r = np.full(3 * max(len(e), 1), -7.25, D); c2 = np.full(max(len(e), 1), -7.25, D)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)     # noqa: E731
    rc = capi.lib().slamhip_debug_pg_relax(vp(p), vp(fx), p.shape[0], vp(e), vp(zz), vp(ww), e.shape[0], vp(spec), vp(iters), vp(fin), vp(r), vp(c2))
    written = not (np.array_equal(p, before, equal_nan=True) and (iters == -7.25).all() and fin[0] == -7.25 and (r == -7.25).all() and (c2 == -7.25).all())
    return rc, written


def test_refusals_write_nothing(capi):
    poses, ij, z, w = tiny_graph(2, 3, [(0, 1), (1, 2)])
    good = capi.pg_spec(2, 5)
    rc, written = raw_relax(capi, poses, None, ij, z, w, good)
    assert rc == 0 and written
    bad_graphs = []
    for e in ([(0, 3), (1, 2)], [(-1, 1), (1, 2)], [(1, 1), (1, 2)]):
        bad_graphs.append((poses, None, e, z, w))
    for v in (np.nan, np.inf):
        zz = z.copy(); zz[1, 2] = v; bad_graphs.append((poses, None, ij, zz, w))
        pp = poses.copy(); pp[2, 0] = v; bad_graphs.append((pp, None, ij, z, w))
        ww = w.copy(); ww[0, 1] = v; bad_graphs.append((poses, None, ij, z, ww))
    for v in (0.0, -1.0):
        ww = w.copy(); ww[1, 2] = v; bad_graphs.append((poses, None, ij, z, ww))
    pp = poses.copy(); pp[1, 2] = 65537.0; bad_graphs.append((pp, None, ij, z, w))
    bad_graphs.append((poses, np.zeros(3, np.uint8), ij, z, w))           # no fixed node
    for gr in bad_graphs:
        rc, written = raw_relax(capi, *gr, good)
        assert rc == capi.ERR_INVALID and not written, gr
    for kw in (dict(n_outer=0), dict(n_outer=65), dict(n_cg=0), dict(n_cg=(1 << 20) + 1), dict(check_every=0), dict(reserved=1), dict(lam=-1.0),
               dict(lam=np.nan), dict(tol=-1e-3), dict(tol=np.inf)):
        a = dict(n_outer=2, n_cg=5); a.update(kw)
        rc, written = raw_relax(capi, poses, None, ij, z, w, capi.pg_spec(**a))
        assert rc == capi.ERR_INVALID and not written, kw
    with pytest.raises(capi.SlamhipError) as e:
        capi.debug_pg_relax(np.zeros((0, 3)), None, np.zeros((0, 2)), np.zeros((0, 3)), np.zeros((0, 3)), good)      # N = 0
    assert e.value.code == capi.ERR_INVALID
    rc, written = raw_relax(capi, poses, None, ij, z, w, capi.pg_spec(64, 1 << 20, check_every=1 << 30, tol=0.5))   # the largest spec
    assert rc == 0


# ---- 2. rule 6 and rule 2 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [0, 1, 255, 256, 257, 65536, 65537])
def test_tree_sum(capi, L):
    g = np.random.Generator(np.random.Philox(100 + L))
    v = g.standard_normal(L) * np.exp(g.uniform(-20, 20, L))
    got = capi.debug_pg_sum(v)
    assert got == np_sum(v)
    if L == 65537:
        left = D(0.0)
        for t in v.tolist():
            left += t
        assert got != left                                                 # a sequence where the plain left-to-right sum differs
        assert abs(got - left) <= 1e-9 * np.abs(v).sum()
    if L == 1:
        assert got == v[0]
    if L == 0:
        assert got == 0.0


def test_sincos(capi):
    """Largest error measured against NumPy's binary64 sin / cos on these 10^5 angles: 2 ulp in each (an ulp: np.spacing of NumPy's
    value).  Asserted: twice that."""
    a = np.random.Generator(np.random.Philox(2025)).uniform(-65536.0, 65536.0, 100000)
    a[:5] = (0.0, 65536.0, -65536.0, np.pi, -np.pi / 2)
    s, c = capi.debug_sincos(a)
    ws, wc = np_sincos(a)
    assert np.array_equal(s, ws) and np.array_equal(c, wc)
    us = np.abs(s - np.sin(a)) / np.spacing(np.abs(np.sin(a))); uc = np.abs(c - np.cos(a)) / np.spacing(np.abs(np.cos(a)))
    print("largest ulp error: sin %g cos %g" % (us.max(), uc.max()))
    assert us.max() <= 4.0 and uc.max() <= 4.0


def test_sincosf_unchanged(capi):
    """sh_det_sincosf itself, on the same 10^5 angles rounded to binary32, through a hook that hands its bits back: a rollout
    (slamhip_debug_rollouts) from (0, 0, 0) with dt = 1 whose first command turns by theta (theta_1 = 0 + theta * 1, exact) and whose
    second drives 1 m (x_2 = 0 + 1 * c, y_2 = 0 + 1 * s, exact) ends at (c, s, theta).  Compared with == against
    oracle/np_oracle.det_sincos, the committed restatement every earlier unit's tests hold the library to."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import np_oracle as npo
    a = np.random.Generator(np.random.Philox(2025)).uniform(-65536.0, 65536.0, 100000)
    a[:5] = (0.0, 65536.0, -65536.0, np.pi, -np.pi / 2)
    af = a.astype(np.float32)
    cls = np.full((4, 4), 2, np.uint8)                                     # all free; at stm = 0.25 every pose lies in cell (0, 0)
    cm = np.zeros((af.shape[0], 2, 2), np.float32); cm[:, 0, 1] = af; cm[:, 1, 0] = 1.0
    res = np.concatenate([capi.debug_rollouts(cls, [(0, 0)], 0.25, (0.0, 0.0, 0.0), 1.0, None, cm[lo:lo + 4096])[0] for lo in range(0, af.shape[0], 4096)])
    ws, wc = npo.det_sincos(af)
    assert (res["n_free"] == 3).all() and np.array_equal(res["theta"], af)
    assert np.array_equal(res["y"].view(np.uint32), ws.view(np.uint32)) and np.array_equal(res["x"].view(np.uint32), wc.view(np.uint32))
    # ... and the binary64 entry point rounded once is the same value
    s64, c64 = capi.debug_sincos(af.astype(D))
    assert np.array_equal(s64.astype(np.float32), ws) and np.array_equal(c64.astype(np.float32), wc)


# ---- 3. restatement against hook -------------------------------------------------------------------------------------------------
def test_two_nodes_one_edge(capi):
    poses = np.array([[0.5, -1.0, 0.3], [2.0, 0.25, -0.4]])
    ij = np.array([[0, 1]], np.int32); z = np.array([[1.25, -0.5, 0.7]]); w = np.array([[4.0, 9.0, 25.0]])
    hp, it, fin, r, c2 = same_as_hook(capi, poses, None, ij, z, w, 1, 3)
    want = compose(poses[0], z[0])                                         # the closed form: the free node lands where z puts it
    assert np.abs(hp[1] - want).max() <= 1e-12 and np.array_equal(hp[0], poses[0])
    assert it[0]["stopped"] == 0 and it[0]["cg_iters"] == 1 and fin <= 1e-20 and it[0]["chi2"] > 1.0
    hp2, it2, fin2, _, _ = same_as_hook(capi, poses, [0, 1], ij, z, w, 4, 3)   # node 1 fixed: node 0 moves (not linear in node 0: several steps)
    assert np.array_equal(hp2[1], poses[1]) and not np.array_equal(hp2[0], poses[0]) and fin2 < it2[0]["chi2"]
    same_as_hook(capi, poses, None, np.zeros((0, 2), np.int32), np.zeros((0, 3)), np.zeros((0, 3)), 1, 3)    # E = 0
    same_as_hook(capi, poses[:1], None, np.zeros((0, 2), np.int32), np.zeros((0, 3)), np.zeros((0, 3)), 2, 1)  # N = 1


@pytest.mark.parametrize("lam", [0.0, 0.5])
def test_three_nodes_duplicated_edge(capi, lam):
    poses, ij, z, w = tiny_graph(11, 3, [(0, 1), (1, 2), (0, 1), (2, 0), (2, 1)])
    z[2] = z[0] + 0.01                                                     # the duplicate is a second edge with its own measurement
    hp, it, fin, _, c2 = same_as_hook(capi, poses, None, ij, z, w, 3, 12, lam=lam)
    assert fin < it[0]["chi2"] and c2.shape == (5,)
    same_as_hook(capi, poses, [0, 0, 1], ij, z, w, 2, 12, lam=lam)
    same_as_hook(capi, poses, [1, 0, 1], ij, z, w, 2, 12, lam=lam)
    same_as_hook(capi, poses, None, ij, z, w, 2, 1, lam=lam, tol=0.0)     # n_cg reached
    _, it, _, _, _ = capi.debug_pg_relax(poses, None, ij, z, w, capi.pg_spec(2, 1, lam=lam, tol=0.0))
    assert it[0]["stopped"] == 1 and it[0]["cg_iters"] == 1


def test_ring_of_64_against_the_restatement(capi):
    poses, ij, z, w = ring(64)
    same_as_hook(capi, poses, None, ij, z, w, 2, 40)
    # node 300 of a chain of 520 lies in the third block of rule 6
    p2, ij2, z2, w2 = ring(520, seed=3)
    same_as_hook(capi, p2, None, ij2[:-1], z2[:-1], w2[:-1], 1, 6)


@pytest.mark.parametrize("wrong", ["order", "no_wrap", "uy_sign"])
def test_wrong_variants_fail(capi, wrong):
    """The comparison is sharp: each wrong copy of the restatement disagrees with the hook on a graph that exercises it."""
    poses, ij, z, w = tiny_graph(21, 5, [(0, 1), (1, 2), (1, 3), (4, 1), (2, 3), (3, 4), (1, 0)])
    poses[:, 2] = [3.0, -3.0, 2.5, -2.9, 0.1]                             # heading differences beyond pi: the wrap matters
    same_as_hook(capi, poses, None, ij, z, w, 2, 20)
    assert not same_as_hook(capi, poses, None, ij, z, w, 2, 20, wrong=wrong)


def test_edge_order_changes_last_bits(capi):
    """Rule 4 sums in EDGE order: a permutation of the edges that meet at one node may change the last bits, and nothing more."""
    poses, ij, z, w = tiny_graph(31, 5, [(0, 1), (1, 2), (1, 3), (4, 1), (2, 3), (3, 4)])
    spec = capi.pg_spec(1, 4, tol=0.0)
    base = capi.debug_pg_relax(poses, None, ij, z, w, spec)[0]
    found = None
    for perm in itertools.permutations(range(4)):                          # the four edges that meet at node 1
        order = list(perm) + [4, 5]
        if order == list(range(6)):
            continue
        got = capi.debug_pg_relax(poses, None, ij[order], z[order], w[order], spec)[0]
        assert np.abs(got - base).max() <= 1e-9
        wp = np_relax(poses, None, ij[order], z[order], w[order], 1, 4, tol=0.0)[0]
        assert np.array_equal(got, wp)
        if found is None and not np.array_equal(got, base):
            found = order
    assert found is not None


# ---- 4. convergence against the independent solver -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ring_cases(capi):
    """The hook's and the dense solver's results on the rings, computed once."""
    out = {}
    for N in (64, 257):
        poses, ij, z, w = ring(N)
        hook = capi.debug_pg_relax(poses, None, ij, z, w, capi.pg_spec(6, 4 * N, tol=1e-6))
        out[N] = (hook, dense_gauss_newton(poses, ij, z, w, 10))
    return out


@pytest.mark.parametrize("N", [64, 257])
def test_ring_converges_to_the_dense_solution(ring_cases, N):
    (hp, it, fin, _, _), (dp, dchi2) = ring_cases[N]
    err_xy = np.abs(hp[:, :2] - dp[:, :2]).max(); err_th = np.abs(np_wrap(hp[:, 2] - dp[:, 2])).max()
    print("N = %d: %g m, %g rad, chi2 %.12g against %.12g, PCG iterations %s" % (N, err_xy, err_th, fin, dchi2, it["cg_iters"].tolist()))
    assert err_xy <= 1e-8 and err_th <= 1e-9
    assert abs(fin - dchi2) <= 1e-9 * dchi2
    assert it[-1]["stopped"] == 0 and (it["cg_iters"] < 4 * N).all()
    assert fin < it[0]["chi2"]


def test_wrap_and_turn(capi):
    """A ring whose headings cross +-pi and the same ring turned by 1 rad relax to the same chi2."""
    N = 64
    a = ring(N); b = ring(N, turn=1.0)
    assert np.abs(a[0][:, 2]).max() > 3.0 and (np.abs(np.diff(a[0][:, 2])) > 6.0).any()      # the stored headings do jump by 2 pi
    assert np.array_equal(a[2], b[2])
    fa = capi.debug_pg_relax(*[a[0], None, a[1], a[2], a[3]], capi.pg_spec(6, 4 * N))[2]
    fb = capi.debug_pg_relax(*[b[0], None, b[1], b[2], b[3]], capi.pg_spec(6, 4 * N))[2]
    fu = capi.debug_pg_relax(ring(N, wrap=False)[0], None, a[1], a[2], a[3], capi.pg_spec(6, 4 * N))[2]   # ... and unwrapped headings
    assert abs(fa - fb) <= 1e-9 * fa and abs(fa - fu) <= 1e-9 * fa


@pytest.mark.parametrize("lam", [0.0, 0.25])
def test_free_node_without_edges_stays(capi, lam):
    poses, ij, z, w = tiny_graph(41, 4, [(0, 1), (1, 2), (0, 2)])       # node 3 has no edge
    hp, it, _, _, _ = same_as_hook(capi, poses, None, ij, z, w, 2, 10, lam=lam)
    assert np.array_equal(hp[3], poses[3]) and not np.array_equal(hp[1], poses[1])
    assert (it["stopped"] != 2).all()
