"""The graphs and queries of the marginal-covariance tests (K27: tests/test_hs_pg_marg_abi.py, tests/test_gpu_hector_pg_marg.py) and the
NumPy restatement of the definition (include/slamhip.h, slamhip_hs_pg_marginals, rules M1 - M5).

The restatement (np_marginals) shares no text with the library: it stands on the restatements of K19 and K22 (test_hs_pg_abi.py,
pg_tri_cases.py), whole-array NumPy with the header's parentheses, and writes rule 7 once more, per right-hand side, from x = 0 and
res = e.  `wrong` selects one of three wrong copies that the hook must differ from.

The catalogue is the smallest graphs at which the batch can go wrong.  R = 3 C is a multiple of 3, so of the group edges G - 1, G,
G + 1 and 2 G + 1 (G = 1 and G = 4 are instantiated) a QUERY reaches R = 3 (G - 1 for G = 4, 2 G + 1 for G = 1), R = 6, R = 9
(2 G + 1 for G = 4) and R = 12; the others -- 1, 2, 4 and 5 right-hand sides in a launch -- are reached as chunk sizes R_c through
max_bytes (CHUNKS), which the tests run on the cases that have enough right-hand sides."""
import numpy as np

import pg_tri_cases as tc
import test_hs_pg_abi as A

D = np.float64
GROUPS = (1, 4)                                                            # the instantiated G; 1 is the default
CHUNKS = (1, 2, 3, 4, 5, 9)                                                # R_c: G - 1, G, G + 1 and 2 G + 1 for both G


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def rhs_bytes(N, precond):
    """Rule M5's B."""
    tot, n = 0, N
    while True:
        tot += n
        if n == 1:
            break
        n = (n + 1) // 2
    return 120 * N + 16 * (-(-N // 256)) + 40 + (24 * (tot - N) + 24 if precond else 0)


def np_columns(fx, pairs, wrong=None):
    """Rule M1 -> the columns' nodes."""
    ms = [int(m) for m in pairs[:, 1] if not fx[m]]
    if wrong == "first_appearance":
        return list(dict.fromkeys(ms))
    return sorted(set(ms))


class _Solve:
    """One right-hand side's PCG (rule M2): step() is "the tests before iteration k, then iteration k"."""

    def __init__(self, S, node, comp):
        self.S = S
        N = S["N"]
        self.x = np.zeros((N, 3), D); self.res = np.zeros((N, 3), D)
        self.res[node, comp] = 1.0
        self.zv = S["precondition"](self.res); self.p = self.zv.copy()
        self.rz = A.np_dot(self.res, self.zv); self.rz0 = self.rz
        self.k = 0; self.stopped = None
        self.node, self.comp = node, comp

    def step(self):
        S = self.S
        tol, lam, w, ij, fx = S["tol"], S["lam"], S["w"], S["ij"], S["fx"]
        if self.rz <= (tol * tol) * self.rz0 or self.rz <= 0:
            self.stopped = 0
            return
        if self.k == S["n_cg"]:
            self.stopped = 1
            return
        p = self.p
        t = w * (A.np_mul(S["Aj"], p[ij[:, 0]]) + A.np_mul(S["Bj"], p[ij[:, 1]]))
        q = lam * p
        for nodes, edges, sides in S["lists"]:
            J = np.where((sides == 0)[:, None, None], S["Aj"][edges], S["Bj"][edges])
            q[nodes] = q[nodes] + A.np_jtv(J, t[edges])
        q[fx] = 0.0
        pq = A.np_dot(p, q)
        if not pq > 0:
            self.stopped = 2
            return
        alpha = self.rz / pq
        self.x = self.x + alpha * p; self.res = self.res - alpha * q
        self.zv = S["precondition"](self.res)
        rzn = A.np_dot(self.res, self.zv)
        beta = rzn / self.rz
        self.p = self.zv + beta * p
        self.rz = rzn
        self.k += 1


def np_marginals(poses, fixed, ij, z, w, pairs, n_cg, precond, lam=0.0, tol=1e-9, max_bytes=0, group=4, wrong=None):
    """Rules M1 - M5 -> (blocks (P, 3, 3), cols: a list of dicts in M1's order, info: a dict; None for rule M5's R_c = 0)."""
    poses, fx, ij, z, w = tc.np_graph(poses, fixed, ij, z, w)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    N, P = poses.shape[0], pairs.shape[0]
    cols = np_columns(fx, pairs, wrong)
    C = len(cols); R = 3 * C
    Rc = min(R, (max_bytes if max_bytes else 256 << 20) // rhs_bytes(N, precond))
    info = {"n_cols": C, "n_rhs": R, "rhs_per_chunk": Rc, "n_chunks": -(-R // Rc) if Rc else 0, "group": group}
    blocks = np.zeros((P, 3, 3), D)
    if R == 0:
        return blocks, [], info
    if Rc == 0:
        return None
    lam = D(lam); tol = D(tol)
    lists = A.np_lists(N, ij)
    levels, live, _, _, Aj, Bj = tc.np_tri_factor(poses, fx, ij, z, w, lam, lists)
    M = np.where(live[:, None, None], levels[0][0], D(0.0))                # rule 4's M: rule T1's P of a live node, 0 of a dead one
    S = {"N": N, "n_cg": n_cg, "tol": tol, "lam": lam, "w": w, "ij": ij, "fx": fx, "Aj": Aj, "Bj": Bj, "lists": lists,
         "precondition": (lambda res: tc.np_tri_solve(levels, live, res)) if precond else (lambda res: A.np_mul(M, res))}
    sol = [_Solve(S, m, b) for m in cols for b in range(3)]
    if wrong == "shared_stop":                                             # one stop for a group of right-hand sides
        for j0 in range(0, R, group):
            grp = sol[j0:j0 + group]
            while all(s.stopped is None for s in grp):
                for s in grp:
                    s.step()
            first = next(s.stopped for s in grp if s.stopped is not None)
            for s in grp:
                s.stopped = first if s.stopped is None else s.stopped
    else:
        for s in sol:
            while s.stopped is None:
                s.step()
    col_of = {m: c for c, m in enumerate(cols)}
    for pi, (n, m) in enumerate(pairs):
        if fx[n] or fx[m]:
            continue
        for b in range(3):
            blocks[pi, :, b] = sol[3 * col_of[int(m)] + b].x[n]
        if wrong == "transposed":
            blocks[pi] = blocks[pi].T.copy()
    recs = [{"rz0": s.rz0, "rz": s.rz, "cg_iters": s.k, "stopped": s.stopped, "node": s.node, "comp": s.comp} for s in sol]
    return blocks, recs, info


def free_loops(fx, ij):
    """L': the edges that are not chain edges and join two free nodes."""
    ij = np.asarray(ij).reshape(-1, 2)
    return int(sum(1 for i, j in ij if abs(int(i) - int(j)) != 1 and not fx[i] and not fx[j]))


# ---- the catalogue -------------------------------------------------------------------------------------------------------------------
def all_pairs(nodes):
    return [(n, m) for n in nodes for m in nodes]


def chain(N, w=(400.0, 400.0, 2500.0), step=0.25):
    """A straight chain along x, theta = 0 throughout, exact measurements: rule 3's third rows decouple theta."""
    poses = np.zeros((N, 3), D); poses[:, 0] = step * np.arange(N)
    ij = np.array([(k, k + 1) for k in range(N - 1)], np.int32).reshape(-1, 2)
    z = np.tile([step, 0.0, 0.0], (N - 1, 1)); ww = np.tile(np.asarray(w, D), (N - 1, 1))
    return poses, ij, z, ww


def cases():
    """name -> dict(poses, fixed, ij, z, w, lam, pairs, n_cg, tol): n_cg per preconditioner as (jacobi, tri)."""
    out = {}

    def put(name, poses, fixed, ij, z, w, lam, pairs, n_cg, tol=1e-9):
        out[name] = dict(poses=np.asarray(poses, D), fixed=fixed, ij=np.asarray(ij, np.int32).reshape(-1, 2), z=np.asarray(z, D).reshape(-1, 3),
                         w=np.asarray(w, D).reshape(-1, 3), lam=lam, pairs=np.asarray(pairs, np.int32).reshape(-1, 2), n_cg=n_cg, tol=tol)

    put("n1", [[0.3, -0.2, 0.1]], None, np.zeros((0, 2)), np.zeros((0, 3)), np.zeros((0, 3)), 0.0, [(0, 0)], (5, 5))          # only the fixed node: C = 0
    p, e, z, w = tc.chain_ring(2, seed=41)
    put("n2", p, None, e, z, w, 0.0, [(1, 1), (0, 1), (1, 0), (1, 1)], (8, 8))                                              # R = 3
    p, e, z, w = tc.chain_ring(3, seed=42, close=False)
    e = np.concatenate([e, [(1, 2)]]); z = np.concatenate([z, z[[1]] + 0.003]); w = np.concatenate([w, w[[1]] * 0.5])
    put("n3_duplicate", p, None, e, z, w, 0.0, all_pairs(range(3)), (20, 8))                                               # R = 6
    # rule 6's block edge per right-hand side: rings with 1, 2 and 3 loops between free nodes; a column next to the fixed node, one
    # far from it, the last node; many n for one m
    for N, loops in ((255, [(200, 40)]), (256, [(200, 40), (128, 3)]), (257, [(200, 40), (128, 3), (250, 100)])):
        p, e, z, w = tc.chain_ring(N, loops, seed=300 + N)
        pairs = all_pairs((1, N // 2, N - 1)) + [(n, N // 2) for n in (0, 2, 77, 254)]
        put("ring%d" % N, p, None, e, z, w, 0.0, pairs, (12, 6 * len(loops) + 1), 1e-12)                                   # R = 9
    # a pure chain with node 0 fixed, fixed nodes in the middle (segments) and a free node without an edge (dead)
    p, e, z, w = tc.chain_ring(40, seed=44, close=False)
    keep = np.array([k for k in range(e.shape[0]) if 30 not in tuple(e[k])])
    fx = np.zeros(40, np.uint8); fx[[0, 10, 11, 25, 33]] = 1
    pairs = [(5, 5), (5, 5), (18, 5), (5, 18), (12, 18), (10, 18), (18, 10), (30, 30), (31, 30), (31, 31), (32, 31), (32, 32), (34, 39), (39, 39), (1, 1), (26, 1)]
    put("segments", p, fx, e[keep], z[keep], w[keep], 0.0, pairs, (10, 4), 1e-6)                                          # C = 7 (1, 5, 18, 30, 31, 32, 39)
    put("segments_lambda", p, fx, e[keep], z[keep], w[keep], 0.25, pairs, (10, 10), 1e-6)                                  # ... the dead node is live
    sc = tc.structure_cases()
    p, f, e, z, w, _ = sc["duplicate_chain_edges"]
    put("duplicates", p, f, e, z, w, 1e-3, all_pairs((3, 4, 17, 33)), (9, 30), 1e-10)                                      # R = 12
    p, f, e, z, w, _ = sc["reversed_chain_edge"]
    put("reversed", p, f, e, z, w, 0.0, [(7, 8), (8, 7), (8, 8), (39, 8), (7, 39)], (9, 8), 1e-10)                         # R = 9 (7, 8, 39)
    p, f, e, z, w, _ = sc["loops"]
    put("lambda", p, f, e, z, w, 0.5, [(20, 20), (2, 20), (21, 20)], (40, 20), 1e-10)                                      # R = 3
    p, e, z, w = chain(37)
    put("chain37", p, None, e, z, w, 0.0, [(k, k) for k in (1, 2, 18, 36)] + [(36, 1), (1, 36)], (15, 4), 1e-10)           # R = 12
    return out


PRECONDS = (("jacobi", 0), ("tri", 1))
