"""The graphs of the odometry-chain preconditioner's tests (K22: tests/test_hs_pg_tri_abi.py, tests/test_gpu_hector_pg_tri.py) and the
NumPy restatement of its definition (include/slamhip.h, slamhip_hs_pg_relax_tri, rules T1 - T5).

The restatement (np_inv, np_px, np_tri_factor, np_tri_solve, np_relax_tri) shares no text with hs_pg_tri.h and, like the one of
tests/test_hs_pg_abi.py that it builds on, uses elementwise NumPy operations only: a level of the cyclic reduction is one batch of
(n, 3, 3) arrays, every product and sum written with the header's parentheses."""
import numpy as np

import test_hs_pg_abi as A

D = np.float64
TAIL = 1024                                                                # S, HS_TRI_TAIL


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def np_inv(Dn, ok=None):
    """Rule 4's adjugate over the determinant for a batch of symmetric (n, 3, 3) (the entries a <= b are read) -> (P, det > 0)."""
    d00, d01, d02, d11, d12, d22 = Dn[:, 0, 0], Dn[:, 0, 1], Dn[:, 0, 2], Dn[:, 1, 1], Dn[:, 1, 2], Dn[:, 2, 2]
    c00 = d11 * d22 - d12 * d12; c01 = d02 * d12 - d01 * d22; c02 = d01 * d12 - d02 * d11
    c11 = d00 * d22 - d02 * d02; c12 = d01 * d02 - d00 * d12; c22 = d00 * d11 - d01 * d01
    det = (d00 * c00 + d01 * c01) + d02 * c02
    pos = det > 0 if ok is None else (ok & (det > 0))
    safe = np.where(pos, det, D(1.0))
    P = np.zeros_like(Dn)
    for (a, b), cab in (((0, 0), c00), ((0, 1), c01), ((0, 2), c02), ((1, 1), c11), ((1, 2), c12), ((2, 2), c22)):
        P[:, a, b] = np.where(pos, cab / safe, D(0.0)); P[:, b, a] = P[:, a, b]
    return P, pos


def np_px(P, X):
    """W = P X: W[a][b] = (P[a][0] X[0][b] + P[a][1] X[1][b]) + P[a][2] X[2][b]."""
    W = np.zeros_like(X)
    for a in range(3):
        for b in range(3):
            W[:, a, b] = (P[:, a, 0] * X[:, 0, b] + P[:, a, 1] * X[:, 1, b]) + P[:, a, 2] * X[:, 2, b]
    return W


def np_tri_factor(poses, fx, ij, z, w, lam, lists):
    """Rules 3, 4 and T1 - T3 -> (levels: a list of (P, U) per level, live, g, chi2_e, A, B)."""
    N = poses.shape[0]
    free = ~fx
    Aj, Bj, r, chi2e = A.np_edges(poses, ij, z, w)
    Dn = np.zeros((N, 3, 3), D); g = np.zeros((N, 3), D)
    Dn[:, 0, 0] = lam; Dn[:, 1, 1] = lam; Dn[:, 2, 2] = lam
    wr = w * r
    for nodes, edges, sides in lists:
        keep = free[nodes]
        nodes, edges, sides = nodes[keep], edges[keep], sides[keep]
        J = np.where((sides == 0)[:, None, None], Aj[edges], Bj[edges])
        we = w[edges]
        for a in range(3):
            for b in range(a, 3):
                T = ((J[:, 0, a] * we[:, 0]) * J[:, 0, b] + (J[:, 1, a] * we[:, 1]) * J[:, 1, b]) + (J[:, 2, a] * we[:, 2]) * J[:, 2, b]
                Dn[nodes, a, b] = Dn[nodes, a, b] + T
        g[nodes] = g[nodes] + A.np_jtv(J, wr[edges])
    g[fx] = 0.0
    P, live = np_inv(Dn, free)
    Dn[~live] = np.eye(3); P[~live] = np.eye(3)                            # T1
    for a in range(3):
        for b in range(a):
            Dn[:, a, b] = Dn[:, b, a]
    # T2: the chain edges of two live nodes, rank by rank in edge order
    U = np.zeros((N, 3, 3), D)
    lo = np.minimum(ij[:, 0], ij[:, 1]); hi = np.maximum(ij[:, 0], ij[:, 1])
    e = np.nonzero((hi == lo + 1) & live[lo] & live[hi])[0]
    e = e[np.lexsort((e, lo[e]))]
    rank = np.arange(e.shape[0]) - np.searchsorted(lo[e], lo[e], side="left")
    for rr in range(int(rank.max()) + 1 if rank.size else 0):
        ee = e[rank == rr]
        at_i = (ij[ee, 0] == lo[ee])[:, None, None]
        Jn = np.where(at_i, Aj[ee], Bj[ee]); Jm = np.where(at_i, Bj[ee], Aj[ee])
        we = w[ee]
        for a in range(3):
            for b in range(3):
                U[lo[ee], a, b] = U[lo[ee], a, b] + (((Jn[:, 0, a] * we[:, 0]) * Jm[:, 0, b] + (Jn[:, 1, a] * we[:, 1]) * Jm[:, 1, b]) + (Jn[:, 2, a] * we[:, 2]) * Jm[:, 2, b])
    levels = [(P, U)]
    while Dn.shape[0] > 1:                                                 # T3
        n = Dn.shape[0]
        k = 2 * np.arange((n + 1) // 2)
        D1 = Dn[k].copy()
        U1 = np.zeros((k.shape[0], 3, 3), D)
        s = np.nonzero(k >= 1)[0]
        Ul = U[k[s] - 1]; W = np_px(P[k[s] - 1], Ul)
        for a in range(3):
            for b in range(a, 3):
                D1[s, a, b] = D1[s, a, b] - ((Ul[:, 0, a] * W[:, 0, b] + Ul[:, 1, a] * W[:, 1, b]) + Ul[:, 2, a] * W[:, 2, b])
        s = np.nonzero(k + 1 < n)[0]
        Uk = U[k[s]]; W = np_px(P[k[s] + 1], Uk.transpose(0, 2, 1))
        for a in range(3):
            for b in range(a, 3):
                D1[s, a, b] = D1[s, a, b] - ((Uk[:, a, 0] * W[:, 0, b] + Uk[:, a, 1] * W[:, 1, b]) + Uk[:, a, 2] * W[:, 2, b])
        s = np.nonzero(k + 2 < n)[0]
        Uk = U[k[s]]; W = np_px(P[k[s] + 1], U[k[s] + 1])
        for a in range(3):
            for b in range(3):
                U1[s, a, b] = D(0.0) - ((Uk[:, a, 0] * W[:, 0, b] + Uk[:, a, 1] * W[:, 1, b]) + Uk[:, a, 2] * W[:, 2, b])
        for a in range(3):
            for b in range(a):
                D1[:, a, b] = D1[:, b, a]
        Dn, U = D1, U1
        P, _ = np_inv(Dn)
        levels.append((P, U))
    return levels, live, g, chi2e, Aj, Bj


def np_tri_solve(levels, live, r0):
    """Rule T4 -> z."""
    rs = [np.array(r0, D)]
    for P, U in levels[:-1]:
        r = rs[-1]; n = r.shape[0]
        k = 2 * np.arange((n + 1) // 2)
        r1 = r[k].copy()
        s = np.nonzero(k >= 1)[0]
        r1[s] = r1[s] - A.np_jtv(U[k[s] - 1], A.np_mul(P[k[s] - 1], r[k[s] - 1]))
        s = np.nonzero(k + 1 < n)[0]
        r1[s] = r1[s] - A.np_mul(U[k[s]], A.np_mul(P[k[s] + 1], r[k[s] + 1]))
        rs.append(r1)
    zz = A.np_mul(levels[-1][0], rs[-1])
    for l in range(len(levels) - 2, -1, -1):
        P, U = levels[l]
        r = rs[l]; n = r.shape[0]
        out = np.zeros_like(r)
        out[0::2] = zz
        k = np.arange(1, n, 2)
        t = r[k] - A.np_jtv(U[k - 1], zz[(k - 1) // 2])
        s = np.nonzero(k + 1 < n)[0]
        t[s] = t[s] - A.np_mul(U[k[s]], zz[(k[s] + 1) // 2])
        out[k] = A.np_mul(P[k], t)
        zz = out
    zz[~live] = 0.0
    return zz


def np_graph(poses, fixed, ij, z, w):
    poses = np.array(poses, D).reshape(-1, 3); ij = np.asarray(ij, np.int64).reshape(-1, 2)
    z = np.asarray(z, D).reshape(-1, 3); w = np.asarray(w, D).reshape(-1, 3)
    fx = np.zeros(poses.shape[0], bool)
    if fixed is None:
        fx[0] = True
    else:
        fx[:] = np.asarray(fixed).astype(bool)
    return poses, fx, ij, z, w


def np_tri_apply(poses, fixed, ij, z, w, lam, rhs):
    poses, fx, ij, z, w = np_graph(poses, fixed, ij, z, w)
    levels, live = np_tri_factor(poses, fx, ij, z, w, D(lam), A.np_lists(poses.shape[0], ij))[:2]
    return np_tri_solve(levels, live, np.asarray(rhs, D).reshape(-1, 3))


def np_relax_tri(poses, fixed, ij, z, w, n_outer, n_cg, lam=0.0, tol=1e-6):
    """Rules 3, 5, 6, 8 and T1 - T5 -> (poses, iters as a list of dicts, chi2_final, r, chi2_e)."""
    poses, fx, ij, z, w = np_graph(poses, fixed, ij, z, w)
    free = ~fx
    lists = A.np_lists(poses.shape[0], ij)
    lam = D(lam); tol = D(tol)
    iters = []
    for _ in range(n_outer):
        levels, live, g, chi2e, Aj, Bj = np_tri_factor(poses, fx, ij, z, w, lam, lists)
        x = np.zeros_like(poses); res = -g; zv = np_tri_solve(levels, live, res); p = zv.copy()
        rz = A.np_dot(res, zv); rz0 = rz
        k = 0
        while True:
            if rz <= (tol * tol) * rz0 or rz <= 0:
                stopped = 0
                break
            if k == n_cg:
                stopped = 1
                break
            t = w * (A.np_mul(Aj, p[ij[:, 0]]) + A.np_mul(Bj, p[ij[:, 1]]))
            q = lam * p
            for nodes, edges, sides in lists:
                J = np.where((sides == 0)[:, None, None], Aj[edges], Bj[edges])
                q[nodes] = q[nodes] + A.np_jtv(J, t[edges])
            q[fx] = 0.0
            pq = A.np_dot(p, q)
            if not pq > 0:
                stopped = 2
                break
            alpha = rz / pq
            x = x + alpha * p; res = res - alpha * q
            zv = np_tri_solve(levels, live, res)
            rzn = A.np_dot(res, zv)
            beta = rzn / rz
            p = zv + beta * p
            rz = rzn
            k += 1
        iters.append({"chi2": A.np_sum(chi2e), "rz0": rz0, "rz": rz, "cg_iters": k, "stopped": stopped})
        new = poses + x
        new[:, 2] = A.np_wrap(new[:, 2])
        poses = np.where(free[:, None], new, poses)
    _, _, r, chi2e = A.np_edges(poses, ij, z, w)
    return poses, iters, A.np_sum(chi2e), r, chi2e


# ---- graphs ----------------------------------------------------------------------------------------------------------------------
def ring_true(N):
    R = 0.25 / (2.0 * np.sin(np.pi / max(N, 2)))
    phi = 2.0 * np.pi * np.arange(N) / N
    return np.stack([R * np.cos(phi), R * np.sin(phi), phi + np.pi / 2], axis=1)


def rel_many(true, i, j):
    c, s = np.cos(true[i, 2]), np.sin(true[i, 2])
    dx, dy = true[j, 0] - true[i, 0], true[j, 1] - true[i, 1]
    return np.stack([c * dx + s * dy, c * dy - s * dx, A.np_wrap(true[j, 2] - true[i, 2])], axis=1)


def chain_ring(N, loops=(), seed=3, close=True):
    """N poses on a ring 0.25 m apart: the chain edges (k, k + 1), the closing edge (N - 1, 0) to the fixed node 0 (close, N >= 3),
    then `loops` (i, j); measurements = the true relative poses + noise, the poses the truth + noise.  Whole-array operations."""
    g = np.random.Generator(np.random.Philox(seed))
    true = ring_true(N)
    e = [(k, k + 1) for k in range(N - 1)] + ([(N - 1, 0)] if close and N >= 3 else []) + [tuple(l) for l in loops]
    ij = np.array(e, np.int32).reshape(-1, 2)
    z = rel_many(true, ij[:, 0], ij[:, 1]) + g.standard_normal((ij.shape[0], 3)) * A.SIGMA
    w = np.tile(1.0 / A.SIGMA ** 2, (ij.shape[0], 1))
    poses = true + g.standard_normal((N, 3)) * np.array([0.05, 0.05, 0.01])
    poses[:, 2] = A.np_wrap(poses[:, 2])
    return poses, ij, z, w


def level_case(N):
    """The graph of a level-edge size: a closed ring with one loop to the fixed node's neighbourhood and, from 8 nodes on, two loops
    between free nodes."""
    loops = [(N - 2, 1), (N // 2, 2)] if N >= 8 else []
    return chain_ring(N, loops, seed=100 + N)


def structure_cases():
    """name -> (poses, fixed, ij, z, w, lam): the shapes of the chain at which T changes."""
    out = {}
    p, e, z, w = chain_ring(40, [(30, 5), (20, 2)], seed=12)
    out["loops"] = (p, None, e, z, w, 0.0)
    keep = np.array([n for n in range(e.shape[0]) if tuple(e[n]) not in ((19, 20), (39, 0), (20, 2))])
    out["missing_chain_edge"] = (p, None, e[keep], z[keep], w[keep], 0.0)            # nodes 20 .. 39 hang on the loop (30, 5) alone
    mid = np.zeros(40, np.uint8); mid[20] = 1
    out["fixed_mid"] = (p, mid, e, z, w, 0.0)
    ends = np.zeros(40, np.uint8); ends[[0, 39]] = 1
    out["fixed_ends"] = (p, ends, e, z, w, 1e-3)
    er = e.copy(); zr = z.copy()
    true = ring_true(40)
    er[7] = (8, 7); zr[7] = rel_many(true, np.array([8]), np.array([7]))[0]
    out["reversed_chain_edge"] = (p, None, er, zr, w, 0.0)
    # duplicates of the chain edges 3 and 17 (one reversed) behind the loops, a loop between their indices
    ed = np.concatenate([e, [(3, 4), (33, 6), (3, 4), (18, 17)]]).astype(np.int32)
    zd = np.concatenate([z, z[[3]] + 0.005, rel_many(true, np.array([33]), np.array([6])), z[[3]] - 0.004, rel_many(true, np.array([18]), np.array([17]))])
    out["duplicate_chain_edges"] = (p, None, ed, zd, np.tile(1.0 / A.SIGMA ** 2, (ed.shape[0], 1)), 0.0)
    keep = np.array([n for n in range(e.shape[0]) if 10 not in tuple(e[n])])
    out["dead_node"] = (p, None, e[keep], z[keep], w[keep], 0.0)                       # node 10 has no edge: dead
    out["lone_node_lambda"] = (p, None, e[keep], z[keep], w[keep], 0.5)                # ... live, its diagonal alone
    # a star with no chain edge: centre 10, its chain neighbours 9 and 11 fixed, every other node a leaf
    g = np.random.Generator(np.random.Philox(21))
    leaves = np.array([n for n in range(30) if n not in (9, 10, 11)])
    es = np.stack([np.full(leaves.shape[0], 10), leaves], axis=1).astype(np.int32)
    es[::2] = es[::2, ::-1]
    t30 = ring_true(30)
    fs = np.zeros(30, np.uint8); fs[[9, 11]] = 1
    out["star"] = (t30 + g.standard_normal((30, 3)) * 0.05, fs, es, rel_many(t30, es[:, 0], es[:, 1]) + g.standard_normal((es.shape[0], 3)) * 0.01,
                   g.uniform(1.0, 100.0, (es.shape[0], 3)), 0.0)
    # a segment with no anchor and lambda = 0: nodes 20 .. 39 hang on nothing (T and H are singular there)
    keep = np.array([n for n in range(e.shape[0]) if tuple(e[n]) not in ((19, 20), (39, 0), (20, 2), (30, 5))])
    out["floating_segment"] = (p, None, e[keep], z[keep], w[keep], 0.0)
    return out


LEVEL_SIZES = (1, 2, 3, 4, 5, 7, 8, 9, 255, 256, 257, TAIL - 1, TAIL, TAIL + 1, 2 * TAIL + 1)
