"""Cases for the consistent set of loop edges (K23) and a NumPy restatement of its definition (include/slamhip.h,
slamhip_hs_loops_consistent, rules 1 - 6).  tests/test_hs_loops_abi.py holds the host hook to the restatement with == on every
field; tests/test_gpu_hector_loops.py holds the device to the hook.

The restatement (np_loops) is written from the header's rules: whole-array NumPy for rules 1 - 3 (the L x L matrix of d2 in one
broadcast, a < b taken from the upper triangle), a plain loop over boolean rows for rules 4 - 6.  It shares the trig and the wrap
with tests/test_hs_pg_abi.py's restatement (rule 2 of slamhip_hs_pg_relax) and no text with hs_loops.h.  brute_max_clique is an
exhaustive search for the cases small enough.  `wrong` selects a deliberately wrong copy of one rule."""
import numpy as np

import test_hs_pg_abi as A

D = np.float64
WRONG = ("swap", "lt", "tie", "nolever", "nowrap")


def np_loops(poses, ij, z, w, gamma, q_t, q_theta, n_starts=8, min_clique=1, use=None, wrong=None):
    p = np.asarray(poses, D).reshape(-1, 3); ij = np.asarray(ij, np.int64).reshape(-1, 2)
    z = np.asarray(z, D).reshape(-1, 3); w = np.asarray(w, D).reshape(-1, 3)
    L = ij.shape[0]
    u = np.ones(L, bool) if use is None else np.asarray(use).astype(bool)
    i, j = ij[:, 0], ij[:, 1]
    pi, pj = p[i], p[j]
    # rule 1
    sI, cI = A.np_sincos(pi[:, 2])
    Wx = pi[:, 0] + (cI * z[:, 0] - sI * z[:, 1])
    Wy = pi[:, 1] + (sI * z[:, 0] + cI * z[:, 1])
    Wt = pi[:, 2] + z[:, 2]
    sW, cW = A.np_sincos(Wt)
    sJ, cJ = A.np_sincos(pj[:, 2])
    vt = D(0.5) * (D(1.0) / w[:, 0] + D(1.0) / w[:, 1])
    vth = D(1.0) / w[:, 2]
    # rule 2 with the ROW in the role of a and the COLUMN in the role of b, then the upper triangle mirrored
    a, b = (slice(None), None), (None, slice(None))
    with np.errstate(all="ignore"):
        dx = pj[:, 0][b] - pj[:, 0][a]; dy = pj[:, 1][b] - pj[:, 1][a]
        ux = cJ[a] * dx + sJ[a] * dy
        uy = cJ[a] * dy - sJ[a] * dx
        ut = pj[:, 2][b] - pj[:, 2][a]
        Tx = Wx[a] + (cW[a] * ux - sW[a] * uy)
        Ty = Wy[a] + (sW[a] * ux + cW[a] * uy)
        Tt = Wt[a] + ut
        ex = Tx - Wx[b]; ey = Ty - Wy[b]
        et = Tt - Wt[b]
        if wrong != "nowrap":
            et = A.np_wrap(et)
        s = (np.abs(j[a] - j[b]) + np.abs(i[a] - i[b])).astype(D)
        rho2 = ux * ux + uy * uy
        Vt = (vt[a] + vt[b]) + s * D(q_t)
        if wrong != "nolever":
            Vt = Vt + vth[a] * rho2
        Vth = (vth[a] + vth[b]) + s * D(q_theta)
        full = (ex * ex + ey * ey) / Vt + (et * et) / Vth
    tri = np.triu(np.ones((L, L), bool), 1)
    if wrong == "swap":
        tri = tri.T
    d2 = np.where(tri, full, D(0.0))
    d2 = d2 + d2.T
    with np.errstate(invalid="ignore"):
        ok = (d2 < D(gamma)) if wrong == "lt" else (d2 <= D(gamma))
    C = ok & u[:, None] & u[None, :] & ~np.eye(L, dtype=bool)
    # rule 3
    deg = C.sum(axis=1).astype(np.int32)
    # rule 4
    n_used = int(u.sum())
    R = min(int(n_starts), n_used)
    order = sorted(np.flatnonzero(u), key=lambda v: (-int(deg[v]), int(v)))[:R]
    # rules 5 and 6
    best = (0, -1, -1, np.zeros(L, bool))
    for r, v0 in enumerate(order):
        Q = np.zeros(L, bool); Q[v0] = True
        S = C[v0].copy()
        while S.any():
            g = (C & S[None, :]).sum(axis=1)
            cand = np.flatnonzero(S)
            top = cand[g[cand] == g[cand].max()]
            v = int(top.max() if wrong == "tie" else top.min())
            Q[v] = True
            S &= C[v]
        if int(Q.sum()) > best[0]:
            best = (int(Q.sum()), r, int(v0), Q)
    size, rank, start, Q = best
    keep = Q if (rank >= 0 and size >= int(min_clique)) else np.zeros(L, bool)
    return dict(keep=keep, deg=deg, adj=pack_rows(C), d2=d2, C=C,
                info=dict(n_pairs=int(C.sum()) // 2, n_used=n_used, size=size, start=start, rank=rank, n_starts=R, reserved=0))


def pack_rows(C):
    """A boolean L x L matrix as L x ceil(L / 64) uint64: bit (b & 63) of word b >> 6."""
    L = C.shape[0]
    Wn = (L + 63) // 64
    padded = np.zeros((L, Wn * 64), np.uint8)
    padded[:, :L] = C
    return np.packbits(padded, axis=1, bitorder="little").view("<u8").astype(np.uint64).reshape(L, Wn)


def unpack_rows(adj, L):
    return np.unpackbits(np.ascontiguousarray(adj).astype("<u8").view(np.uint8).reshape(adj.shape[0], -1), axis=1, bitorder="little")[:, :L].astype(bool)


def brute_max_clique(C):
    """(size, the list of all maximum cliques as sorted tuples) by exhaustive search; L <= 24."""
    L = C.shape[0]
    assert L <= 24
    nb = [sum(1 << b for b in range(L) if C[a, b]) for a in range(L)]
    best = [0, []]

    def grow(Q, cand):
        if not cand:
            n = len(Q)
            if n > best[0]:
                best[0], best[1] = n, [tuple(Q)]
            elif n == best[0]:
                best[1].append(tuple(Q))
            return
        if len(Q) + bin(cand).count("1") < best[0]:
            return
        c = cand
        while c:
            v = (c & -c).bit_length() - 1
            c &= c - 1
            grow(Q + [v], cand & nb[v] & ~((1 << (v + 1)) - 1))          # (members in increasing order: every clique once)
    for v in range(L):
        grow([v], nb[v] & ~((1 << (v + 1)) - 1))
    if L and best[0] == 0:
        best[0], best[1] = 1, [(v,) for v in range(L)]
    return best[0], sorted(set(best[1]))


# ---- geometry ----------------------------------------------------------------------------------------------------------------------
def rel(true, i, j):
    """Node j in node i's frame (libm trig: these are inputs, not the definition)."""
    i = np.asarray(i); j = np.asarray(j)
    c, s = np.cos(true[i, 2]), np.sin(true[i, 2])
    dx, dy = true[j, 0] - true[i, 0], true[j, 1] - true[i, 1]
    return np.stack([c * dx + s * dy, c * dy - s * dx, A.np_wrap(true[j, 2] - true[i, 2])], axis=1)


def ring(N, seed, step=0.25, bias=0.0015, noise=(0.004, 0.004, 0.0008)):
    """A closed ring of N poses `step` apart -> (true, drifted): the drifted chain integrates the true odometry with a heading bias
    per step and noise, from the true pose 0 -- the keyframe chain as it stands before any loop is closed."""
    g = np.random.Generator(np.random.Philox(seed))
    Rr = step / (2.0 * np.sin(np.pi / N))
    phi = 2.0 * np.pi * np.arange(N) / N
    true = np.stack([Rr * np.cos(phi), Rr * np.sin(phi), A.np_wrap(phi + np.pi / 2)], axis=1)
    od = rel(true, np.arange(N - 1), np.arange(1, N)) + g.standard_normal((N - 1, 3)) * np.array(noise)
    od[:, 2] += bias
    drift = np.zeros((N, 3)); drift[0] = true[0]
    for k in range(N - 1):
        c, s = np.cos(drift[k, 2]), np.sin(drift[k, 2])
        drift[k + 1] = (drift[k, 0] + c * od[k, 0] - s * od[k, 1], drift[k, 1] + s * od[k, 0] + c * od[k, 1], drift[k, 2] + od[k, 2])
    drift[:, 2] = A.np_wrap(drift[:, 2])
    return true, drift


W_LOOP = (2500.0, 2500.0, 10000.0)         # a loop edge's weights: 2 cm, 0.01 rad
SPEC = dict(gamma=11.34, q_t=1e-4, q_theta=2e-5, n_starts=8, min_clique=1)


def loops_on_ring(N, n_true, n_false, seed, reverse=(), dup=0, spread=1):
    """n_true loops between the ring's start and its end (i = 3 + spread k, j = N - 14 + k: they share the correction of the one
    place where the ring closes) with measurements from the TRUE poses plus noise, then n_false edges between nodes far from one
    another whose measurement claims a revisit (a small z), shuffled together; `reverse`: indices (after the shuffle) turned round,
    j < i; dup: that many true loops measured twice."""
    g = np.random.Generator(np.random.Philox(seed))
    true, drift = ring(N, seed + 1)
    ti = 3 + spread * (np.arange(n_true) % 12) + (np.arange(n_true) // 12) % 2; tj = N - 14 + (np.arange(n_true) % 12)
    e = [(int(a), int(b)) for a, b in zip(ti, tj)]
    e += e[:dup]
    zt = rel(true, [a for a, _ in e], [b for _, b in e]) + g.standard_normal((len(e), 3)) * np.array([0.005, 0.005, 0.002])
    fi = g.integers(N // 8, N // 2 - N // 8, n_false); fj = g.integers(N // 2 + N // 8, N - N // 8, n_false)
    zf = g.standard_normal((n_false, 3)) * np.array([0.3, 0.3, 0.2])
    ij = np.array(e + [(int(a), int(b)) for a, b in zip(fi, fj)], np.int64).reshape(-1, 2)
    z = np.concatenate([zt, zf]); is_true = np.arange(ij.shape[0]) < len(e)
    perm = g.permutation(ij.shape[0])
    ij, z, is_true = ij[perm], z[perm], is_true[perm]
    for k in reverse:
        a, b = ij[k]
        c, s = np.cos(z[k, 2]), np.sin(z[k, 2])
        z[k] = (-(c * z[k, 0] + s * z[k, 1]), -(c * z[k, 1] - s * z[k, 0]), -z[k, 2])     # the inverse measurement
        ij[k] = (b, a)
    return dict(poses=drift, true=true, ij=ij.astype(np.int32), z=z, w=np.tile(np.array(W_LOOP), (ij.shape[0], 1)), is_true=is_true,
                spec=dict(SPEC), use=None)


def flat(zx, gamma=0.0, w=(1.0, 1.0, 1.0), n_starts=8, min_clique=1, N=3):
    """All poses 0, every edge (0, 1), z = (zx_k, 0, 0): W = z, s = 0, rho2 = 0, so d2 = (zx_a - zx_b)^2 / (2 / w) exactly."""
    zx = np.asarray(zx, D)
    L = zx.shape[0]
    z = np.zeros((L, 3)); z[:, 0] = zx
    return dict(poses=np.zeros((N, 3)), ij=np.tile(np.array([[0, 1]], np.int32), (L, 1)), z=z, w=np.tile(np.array(w, D), (L, 1)),
                spec=dict(gamma=gamma, q_t=0.0, q_theta=0.0, n_starts=n_starts, min_clique=min_clique), use=None)


def first_non_resident(capi):
    """The smallest L whose matrix k23_clique does not keep in LDS (capi.LOOPS_LDS_ADJ_BYTES, hs_loops.h's bound)."""
    L = 1
    while L * (((L + 63) // 64) | 1) * 8 <= capi.LOOPS_LDS_ADJ_BYTES:
        L += 1
    return L


def _ring_case():
    return loops_on_ring(200, 12, 9, seed=11)


def _masked(case, drop):
    use = np.ones(case["ij"].shape[0], bool); use[list(drop)] = False
    return dict(case, use=use)


def _one_ulp():
    c = flat([1.0, 1.0, 1.0, 1.0, 1.0])
    c["z"][3, 0] = np.nextafter(1.0, 2.0)                                  # ex of every pair with edge 3: one ulp of 1.0, its square > 0
    return c


CASES = {
    "L1": lambda: flat([0.5]),
    "L2_consistent": lambda: flat([1.0, 1.0]),
    "L2_inconsistent": lambda: flat([1.0, 2.0]),
    "L63": lambda: loops_on_ring(300, 20, 43, seed=63),
    "L64": lambda: loops_on_ring(300, 24, 40, seed=64),
    "L65": lambda: loops_on_ring(300, 24, 41, seed=65, reverse=(1, 7, 40)),
    "L129": lambda: _masked(loops_on_ring(400, 24, 105, seed=129, dup=0), (0, 5, 64, 65, 128)),
    "ring": _ring_case,
    "ring_masked": lambda: _masked(_ring_case(), (2, 3, 10, 20)),
    "ring_duplicates": lambda: loops_on_ring(200, 8, 6, seed=12, dup=4),
    "ring_reversed": lambda: loops_on_ring(200, 10, 8, seed=13, reverse=(0, 2, 3, 9, 15)),
    "threshold_all_zero": lambda: flat([0.0] * 6),                         # d2 == 0 <= gamma == 0 for every pair
    "threshold_one_ulp": _one_ulp,
    # two disjoint cliques of three, every degree 2: rank 0 is edge 0, and its clique {0, 2, 5} wins the tie of sizes
    "tie_two_cliques": lambda: flat([2.0, 1.0, 2.0, 1.0, 1.0, 2.0]),
    "tie_two_cliques_one_start": lambda: flat([2.0, 1.0, 2.0, 1.0, 1.0, 2.0], n_starts=1),
    # a path 0 - 1 - 2 (d2 = dx^2 / 2 <= 0.5): the one start is edge 1, g(0) = g(2) = 0, the lower index joins: {0, 1}
    "tie_path": lambda: flat([0.0, 1.0, 2.0], gamma=0.5, n_starts=1),
    "min_clique_above": lambda: dict(_ring_case(), spec=dict(SPEC, min_clique=13)),
    "nothing_used": lambda: _masked(flat([1.0, 1.0, 1.0]), (0, 1, 2)),
}
BRUTE = ("L1", "L2_consistent", "L2_inconsistent", "ring", "ring_masked", "ring_duplicates", "ring_reversed", "threshold_all_zero",
         "threshold_one_ulp", "tie_two_cliques", "tie_path")


def big_case(capi):
    """One L above the LDS-resident bound: 48 loops at the ring's seam among false ones."""
    L = first_non_resident(capi)
    return dict(loops_on_ring(600, 48, L - 48, seed=7, spread=2), spec=dict(SPEC, n_starts=3))


def restate(case, wrong=None):
    return np_loops(case["poses"], case["ij"], case["z"], case["w"], use=case["use"], wrong=wrong, **case["spec"])
