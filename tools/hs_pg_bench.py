"""K19, the pose-graph relaxation (slamhip_hs_pg_set, _pg_relax): wall clock per blocking call, each figure beside a host solve FROM
THE SAME RUN.
 * Graphs: the ring of tests/test_hs_pg_abi.py (N nodes, N edges) and a grid of streets (k x k nodes, an edge to the right and the
   upper neighbour: about 2 N edges), at N = 10^3, 10^4, 10^5 and 2^20; true relative poses plus Gaussian noise, node 0 fixed.
 * relax: ONE Gauss-Newton step with tol = 0, so that exactly n_cg PCG iterations run, at n_cg = 10 and 60 with check_every = n_cg;
   median, min and max of 15 blocking calls after a warm-up of 3 (5 after 1 at 2^20), the graph set again before each.  The time per
   PCG iteration is the difference of the two medians over 50.  pg_set is timed on its own.
 * Host: the same Gauss-Newton step (libm trig) as a sparse system solved by scipy.sparse.linalg.spsolve, when scipy is there and
   N <= 10^5, once; and slamhip_debug_pg_relax, the library's own host loops, for the same 60 iterations.
 * The design alternative, a developer build of this tree in slam.net_amd/build/variants/ (`python tools/build_variant.py
   WORK k19_scalar -DK19_SCALAR_LAUNCH=1`: alpha, beta and the stop word by a one-workgroup launch behind k19_apply and behind k19_step,
   five launches per iteration), when it is there: the same relax figures at 10^5 and 2^20 nodes, the library in a fresh interpreter
   (`--variant-only` with SLAMHIP_LIB set), the poses after the 60 iterations hashed and compared with this tree's.
 * Existing path: HectorSLAMProcessor.Update of the trace bench's scan, blocking, median of 35 scans; the new code is never entered on
   it.  With a build of the parent commit at slam.net_amd/build/variants/parent.so (`python tools/build_variant.py HEAD~1 parent`) the
   figure is taken in alternating fresh interpreters, this tree then the parent, three each (`--update-only` with SLAMHIP_LIB set).
`python tools/hs_pg_bench.py [out.json]` writes profiles/r25_hs_pg.json by default.

`python tools/hs_pg_bench.py --precond tri [out.json]` (profiles/r28_hs_pg_tri.json): K22, the odometry-chain preconditioner
(slamhip_hs_pg_relax_tri, _pg_tri_apply) beside block-Jacobi IN THE SAME RUN.  Graphs: the ring with its closing edge (N - 1, 0) alone
("fixed": one loop to the fixed node), with one more loop between free nodes ("free") and with 16 of them ("loops16"), and the street
grid, whose vertical edges -- half of all -- are no chain edges.  Per graph and preconditioner: ONE Gauss-Newton step to tol = 1e-6
(wall clock of the blocking call, the PCG iterations it took; block-Jacobi is capped at 4 N iterations and left out at 2^20 nodes),
the same call with n_cg = 1 (linearise, factorisation, the start's solve, one iteration, the copies), the time per PCG iteration as
the difference of the two over the iterations between them, and for tri one blocking _pg_tri_apply (upload, factorisation, solve,
download) with its backward error |T z - r| / (|T|_1 |z| + |r|) beside scipy's spsolve on the same sparse T.

`python tools/hs_pg_bench.py --lm [out.json]` (profiles/r32_hs_pg_lm.json): K26, one attempt of slamhip_hs_pg_relax_lm beside one step
of slamhip_hs_pg_relax / _relax_tri at equal n_cg, and the large rings' first step with and without damping (lm_main)."""
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import slam.net_amd.hector as hs                                           # noqa: E402
from slam.net_amd import capi                                              # noqa: E402

import hs_dfield_bench as db                                               # noqa: E402

SIGMA = np.array([0.02, 0.02, 0.01])


def rel(pi, pj):
    c, s = np.cos(pi[:, 2]), np.sin(pi[:, 2])
    dx, dy = pj[:, 0] - pi[:, 0], pj[:, 1] - pi[:, 1]
    return np.stack([c * dx + s * dy, c * dy - s * dx, np.remainder(pj[:, 2] - pi[:, 2] + np.pi, 2 * np.pi) - np.pi], axis=1)


def finish(true, ij, seed):
    g = np.random.Generator(np.random.Philox(seed))
    z = rel(true[ij[:, 0]], true[ij[:, 1]]) + g.standard_normal((ij.shape[0], 3)) * SIGMA
    poses = true + g.standard_normal(true.shape) * np.array([0.05, 0.05, 0.01])
    return poses, ij.astype(np.int32), z, np.tile(1.0 / SIGMA ** 2, (ij.shape[0], 1))


def ring(N):
    R = 0.25 / (2.0 * np.sin(np.pi / N))
    phi = 2.0 * np.pi * np.arange(N) / N
    true = np.stack([R * np.cos(phi), R * np.sin(phi), np.remainder(phi + 1.5 * np.pi, 2 * np.pi) - np.pi], axis=1)
    return finish(true, np.stack([np.arange(N), (np.arange(N) + 1) % N], axis=1), N)


def streets(N):
    k = int(round(np.sqrt(N)))
    y, x = np.divmod(np.arange(k * k), k)
    true = np.stack([0.25 * x, 0.25 * y, np.where(y % 2 == 0, 0.0, 3.0)], axis=1)
    idx = np.arange(k * k).reshape(k, k)
    ij = np.concatenate([np.stack([idx[:, :-1].ravel(), idx[:, 1:].ravel()], axis=1), np.stack([idx[:-1].ravel(), idx[1:].ravel()], axis=1)])
    return finish(true, ij, N + 1)


def stats(ts):
    ts = np.array(ts) * 1e6
    return {"median_us": float(np.median(ts)), "min_us": float(ts.min()), "max_us": float(ts.max()), "n": len(ts)}


def scipy_step(poses, ij, z, w):
    """One Gauss-Newton step by a sparse direct solve -> seconds, or None without scipy."""
    try:
        import scipy.sparse as sp
        import scipy.sparse.linalg as spl
    except ImportError:
        return None
    t0 = time.perf_counter()
    N, E = poses.shape[0], ij.shape[0]
    i, j = ij[:, 0], ij[:, 1]
    c, s = np.cos(poses[i, 2]), np.sin(poses[i, 2])
    dx, dy = poses[j, 0] - poses[i, 0], poses[j, 1] - poses[i, 1]
    ux, uy = c * dx + s * dy, c * dy - s * dx
    r = np.stack([ux - z[:, 0], uy - z[:, 1], np.remainder(poses[j, 2] - poses[i, 2] - z[:, 2] + np.pi, 2 * np.pi) - np.pi], axis=1)
    zero, one = np.zeros(E), np.ones(E)
    A = np.stack([np.stack([-c, -s, uy], 1), np.stack([s, -c, -ux], 1), np.stack([zero, zero, -one], 1)], 1)
    B = np.stack([np.stack([c, s, zero], 1), np.stack([-s, c, zero], 1), np.stack([zero, zero, one], 1)], 1)
    rows = (3 * np.arange(E)[:, None, None] + np.arange(3)[None, :, None]) + np.zeros((1, 1, 3), int)
    cols_i = 3 * i[:, None, None] + np.arange(3)[None, None, :] + np.zeros((1, 3, 1), int)
    cols_j = 3 * j[:, None, None] + np.arange(3)[None, None, :] + np.zeros((1, 3, 1), int)
    J = sp.csr_matrix((np.concatenate([A.ravel(), B.ravel()]), (np.concatenate([rows.ravel(), rows.ravel()]), np.concatenate([cols_i.ravel(), cols_j.ravel()]))),
                      shape=(3 * E, 3 * N))[:, 3:]
    W = sp.diags(w.ravel())
    H = (J.T @ W @ J).tocsc()
    x = spl.spsolve(H, -(J.T @ (w.ravel() * r.ravel())))
    assert np.isfinite(x).all()
    return time.perf_counter() - t0


def relax_figures(rep, poses, ij, z, w, reps, warm):
    """relax at n_cg = 10 and 60 -> the record (with the hash of the poses after the last 60-iteration call)."""
    rec = {}
    for n_cg in (10, 60):
        spec = capi.pg_spec(1, n_cg, check_every=n_cg, tol=0.0)
        ts = []
        for k in range(reps + warm):
            rep.PgSet(poses, None, ij, z, w)
            t0 = time.perf_counter(); it, _ = rep.PgRelax(spec); dt = time.perf_counter() - t0
            assert it[0]["cg_iters"] == n_cg, it
            if k >= warm:
                ts.append(dt)
        rec["relax_n_cg_%d" % n_cg] = stats(ts)
    rec["us_per_pcg_iteration"] = (rec["relax_n_cg_60"]["median_us"] - rec["relax_n_cg_10"]["median_us"]) / 50.0
    rec["poses_sha1"] = hashlib.sha1(rep.PgGet().tobytes()).hexdigest()
    return rec


VARIANT_SIZES = (100000, 1 << 20)


def variant_figures():
    """The relax figures of the library that is loaded, at the sizes the design alternatives are compared at."""
    ctx = hs.Context(0)
    rep = hs.MapRepMultiMap(0.1, (64, 64), 1, ctx=ctx)
    out = {}
    for name, make in (("ring", ring), ("streets", streets)):
        for N in VARIANT_SIZES:
            poses, ij, z, w = make(N)
            out["%s_%d" % (name, N)] = relax_figures(rep, poses, ij, z, w, *((5, 1) if N > 100000 else (15, 3)))
    rep.close()
    ctx.close()
    return out


def sparse_T(poses, ij, w):
    """The block-tridiagonal part of H (node 0 fixed: identity), rule 2's trig from the library, as a scipy CSC matrix."""
    import scipy.sparse as sp
    N = poses.shape[0]
    i, j = ij[:, 0].astype(np.int64), ij[:, 1].astype(np.int64)
    sn, c = capi.debug_sincos(poses[i, 2])
    dx, dy = poses[j, 0] - poses[i, 0], poses[j, 1] - poses[i, 1]
    ux, uy = c * dx + sn * dy, c * dy - sn * dx
    zero, one = np.zeros(i.shape[0]), np.ones(i.shape[0])
    A = np.stack([np.stack([-c, -sn, uy], 1), np.stack([sn, -c, -ux], 1), np.stack([zero, zero, -one], 1)], 1)
    B = np.stack([np.stack([c, sn, zero], 1), np.stack([-sn, c, zero], 1), np.stack([zero, zero, one], 1)], 1)
    rows, cols, vals = [], [], []
    for (na, Ja), (nb, Jb) in (((i, A), (i, A)), ((j, B), (j, B)), ((i, A), (j, B)), ((j, B), (i, A))):
        keep = (np.abs(na - nb) <= 1) & (na != 0) & (nb != 0)
        blk = np.einsum("eka,ek,ekb->eab", Ja[keep], w[keep], Jb[keep])
        rows.append((3 * na[keep])[:, None, None] + np.arange(3)[None, :, None] + np.zeros((1, 1, 3), np.int64))
        cols.append((3 * nb[keep])[:, None, None] + np.arange(3)[None, None, :] + np.zeros((1, 3, 1), np.int64))
        vals.append(blk)
    rows.append(np.arange(3)); cols.append(np.arange(3)); vals.append(np.ones(3))
    return sp.csc_matrix((np.concatenate([v.ravel() for v in vals]), (np.concatenate([r.ravel() for r in rows]), np.concatenate([c_.ravel() for c_ in cols]))),
                         shape=(3 * N, 3 * N))


def timed_relax(rep, g, spec, precond, reps):
    ts = []
    for _ in range(reps):
        rep.PgSet(g[0], None, g[1], g[2], g[3])
        t0 = time.perf_counter(); it, fin = rep.PgRelax(spec, precond=precond); ts.append(time.perf_counter() - t0)
    return stats(ts), int(it[0]["cg_iters"]), int(it[0]["stopped"]), float(it[0]["chi2"]), float(fin)


def with_loops(make, N, n_loops):
    """The graph of `make` with n_loops more edges between free nodes, spread over the chain."""
    poses, ij, z, w = make(N)
    if n_loops:
        a = (N // 4 + (N // 2) * np.arange(n_loops) // n_loops).astype(np.int32)
        b = (N // 8 + (N // 16) * np.arange(n_loops) // n_loops + 1).astype(np.int32)
        e = np.stack([a, b], axis=1)
        true = make(N)[0]                                                  # (the noisy poses stand in for the truth: the measurement is what matters)
        zz = rel(true[e[:, 0]], true[e[:, 1]])
        ij = np.concatenate([ij, e]).astype(np.int32); z = np.concatenate([z, zz]); w = np.concatenate([w, np.tile(1.0 / SIGMA ** 2, (n_loops, 1))])
    return poses, ij, z, w


def tri_main(out_path):
    ctx = hs.Context(0)
    rep = hs.MapRepMultiMap(0.1, (64, 64), 1, ctx=ctx)
    out = {"graphs": {}}
    for name, make, n_loops in (("ring_fixed", ring, 0), ("ring_free", ring, 1), ("ring_loops16", ring, 16), ("streets", streets, 0)):
        for N in (1000, 10000, 100000, 1 << 20):
            g = with_loops(make, N, n_loops)
            N = g[0].shape[0]
            reps = 3 if N > 100000 else 7
            rec = {"N": int(N), "E": int(g[1].shape[0])}
            for precond in ("tri", "jacobi"):
                cap = min(4 * N, 1 << 20)
                if precond == "jacobi" and N > 100000:
                    continue
                one, _, _, _, _ = timed_relax(rep, g, capi.pg_spec(1, 1, check_every=1, tol=1e-6), precond, reps)
                full, iters, stopped, chi0, chi1 = timed_relax(rep, g, capi.pg_spec(1, cap, check_every=64, tol=1e-6), precond, 1 if precond == "jacobi" and N > 10000 else reps)
                rec[precond] = {"step_to_tol": full, "cg_iters": iters, "stopped": stopped, "chi2_before": chi0, "chi2_after": chi1, "step_n_cg_1": one,
                                "us_per_pcg_iteration": (full["median_us"] - one["median_us"]) / (iters - 1) if iters > 1 else None}
            rep.PgSet(g[0], None, g[1], g[2], g[3])
            rhs = np.random.Generator(np.random.Philox(N)).standard_normal((N, 3)); rhs[0] = 0.0
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter(); zz = rep.PgTriApply(0.0, rhs); ts.append(time.perf_counter() - t0)
            rec["tri_apply"] = stats(ts)
            try:
                import scipy.sparse.linalg as spl
                T = sparse_T(g[0], g[1], g[3])
                r = rhs.ravel()
                n1 = abs(T).sum(axis=0).max()
                be = lambda v: float(np.linalg.norm(T @ v - r) / (n1 * np.linalg.norm(v) + np.linalg.norm(r)))
                rec["backward_error"] = {"tri_apply": be(zz.ravel()), "scipy_spsolve": be(spl.spsolve(T, r))}
            except ImportError:
                rec["backward_error"] = None
            out["graphs"]["%s_%d" % (name, N)] = rec
            print(name, N, json.dumps(rec), flush=True)
    rep.close()
    ctx.close()
    parent = os.path.join(ROOT, "slam.net_amd", "build", "variants", "parent.so")
    if os.path.exists(parent):
        out["update_alternating"] = {"this_tree": [], "parent": []}
        for _ in range(3):
            out["update_alternating"]["this_tree"].append(child("--update-only", None)["update"])
            out["update_alternating"]["parent"].append(child("--update-only", parent)["update"])
        print(json.dumps(out["update_alternating"]), flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)


def lm_main(out_path):
    """K26 (slamhip_hs_pg_relax_lm) beside K19 / K22 IN THE SAME RUN -- their kernels are the parent commit's, instruction for
    instruction.  Per graph (ring, street grid; 10^3, 10^4, 10^5 nodes) and preconditioner: ONE attempt against ONE step at equal
    n_cg = 60 with tol = 0 and kind NONE (the same PCG iterations, counted), the graph set again before each, medians of 7 blocking calls after a warm-up.
    Then the rings whose first undamped step raises chi2 (DESIGN.md section 4 "K22"), once each with LM: F per attempt."""
    ctx = hs.Context(0)
    rep = hs.MapRepMultiMap(0.1, (64, 64), 1, ctx=ctx)
    out = {"graphs": {}, "first_step": {}}
    for name, make in (("ring", ring), ("streets", streets)):
        for N in (1000, 10000, 100000):
            g = make(N)
            rec = {"N": int(g[0].shape[0]), "E": int(g[1].shape[0])}
            for precond in ("jacobi", "tri"):
                step = capi.pg_spec(1, 60, check_every=60, tol=0.0, lam=1e-3)
                lm = capi.pg_lm_spec(1, 60, check_every=60, precond=precond, kind="none", lambda0=1e-3, tol=0.0)   # (NONE: the step's own arithmetic)
                ts = {"step": [], "lm_attempt": []}
                for k in range(8):
                    rep.PgSet(g[0], None, g[1], g[2], g[3])
                    t0 = time.perf_counter(); it, _ = rep.PgRelax(step, precond=precond); dt = time.perf_counter() - t0
                    rep.PgSet(g[0], None, g[1], g[2], g[3])
                    t1 = time.perf_counter(); lit, _, _ = rep.PgRelaxLM(lm); dl = time.perf_counter() - t1
                    assert len(lit) == 1 and lit[0]["cg_iters"] == it[0]["cg_iters"] and lit[0]["rz"] == it[0]["rz"], (it, lit)
                    if k >= 1:
                        ts["step"].append(dt); ts["lm_attempt"].append(dl)
                rec[precond] = {k: stats(v) for k, v in ts.items()}
                rec[precond]["cg_iters"] = int(it[0]["cg_iters"])              # (tri may end below 60: rz <= 0 stops it whatever tol says)
                rec[precond]["extra_us"] = rec[precond]["lm_attempt"]["median_us"] - rec[precond]["step"]["median_us"]
            out["graphs"]["%s_%d" % (name, N)] = rec
            print(name, N, json.dumps(rec), flush=True)
    for N in (10000, 100000, 1 << 20):
        g = ring(N)
        rep.PgSet(g[0], None, g[1], g[2], g[3])
        it, fin = rep.PgRelax(capi.pg_spec(2, 64, check_every=64, tol=1e-6), precond="tri")
        rep.PgSet(g[0], None, g[1], g[2], g[3])
        t0 = time.perf_counter(); lit, F, _ = rep.PgRelaxLM(capi.pg_lm_spec(12, 64, check_every=64, precond="tri", lambda0=1e-3, tol=1e-6)); dt = time.perf_counter() - t0
        out["first_step"]["ring_%d" % N] = {"gauss_newton_chi2": it["chi2"].tolist() + [fin], "lm_F": lit["F"].tolist() + [F], "lm_accepted": lit["accepted"].tolist(),
                                           "lm_lambda": lit["lambda"].tolist(), "lm_cg_iters": lit["cg_iters"].tolist(), "lm_call_us": dt * 1e6}
        print("first_step", N, json.dumps(out["first_step"]["ring_%d" % N]), flush=True)
    rep.close()
    ctx.close()
    parent = os.path.join(ROOT, "slam.net_amd", "build", "variants", "parent.so")
    if os.path.exists(parent):
        out["update_alternating"] = {"this_tree": [], "parent": []}
        for _ in range(3):
            out["update_alternating"]["this_tree"].append(child("--update-only", None)["update"])
            out["update_alternating"]["parent"].append(child("--update-only", parent)["update"])
        print(json.dumps(out["update_alternating"]), flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)


def child(flag, lib):
    """This script again in a fresh interpreter with `lib` (None: this tree's) -> the JSON object it printed last."""
    env = dict(os.environ)
    env.pop("SLAMHIP_LIB", None)
    if lib:
        env["SLAMHIP_LIB"] = lib
    r = subprocess.run([sys.executable, os.path.abspath(__file__), flag], env=env, stdout=subprocess.PIPE, timeout=300, check=True)
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


def marg_launches(N, precond, cols, info, check_every, n_cg):
    """The launches the driver of slamhip_hs_pg_marginals enqueues, from its rule: once k19_linearise and the preconditioner; per chunk
    k27_begin, the start's solve, k27_begin_state, batches of check_every iterations until every right-hand side of the chunk has
    stopped (three launches each, and the solve's), k27_collect."""
    lt, n = 0, N
    while n > 1024:
        n = (n + 1) // 2; lt += 1
    solve = 2 * lt + 1 if precond else 0
    once = 1 + (2 + lt + 1 if precond else 1)                              # k19_linearise; k22_diag, k22_coupling, k22_reduce per large level, k22_factor_tail
    per_iter = 3 + solve
    total = once
    Rc = int(info["rhs_per_chunk"])
    for r0 in range(0, int(info["n_rhs"]), Rc):
        c = cols[r0:r0 + Rc]
        need = int((c["cg_iters"] + (c["stopped"] == 0)).max())            # a tolerance stop is seen by the iteration after it
        batch = min(check_every, 1024)
        enq = min(n_cg, -(-max(need, 1) // batch) * batch)
        total += 2 + solve + enq * per_iter + 1
    return total


def marg_main(out_path, kres_path):
    """K27 (slamhip_hs_pg_marginals): the ring with 16 loops between free nodes of profiles/r28_hs_pg_tri.json at 10^3 and 10^4 nodes,
    C = 64 columns spread over the ring (the four blocks of 32 pairs), precond = 1, tol = 1e-9, n_cg = 6 * 16 + 1.  Timed, each a blocking
    call by the host clock: the default max_bytes with G = 1 (the default) and with G = 4 (SLAMHIP_K27_GROUP), and max_bytes = one right-hand side per
    chunk -- the same kernels launched per right-hand side, the factorisation still done once.  The three are taken in alternation,
    7 rounds after 2 warm-up rounds (the one-per-chunk call: 3 after 1), medians; every call's blocks are compared with the first's."""
    ctx = hs.Context(0)
    rep = hs.MapRepMultiMap(0.1, (64, 64), 1, ctx=ctx)
    out = {"points": {}}
    n_cg = 6 * 16 + 1
    for N in (1000, 10000):
        g = with_loops(ring, N, 16)
        rep.PgSet(g[0], None, g[1], g[2], g[3])
        nodes = (1 + (N - 2) * np.arange(64) // 64).astype(np.int32)
        pairs = np.array([(a, b) for i, j in zip(nodes[0::2], nodes[1::2]) for a, b in ((i, i), (i, j), (j, i), (j, j))], np.int32)
        B = capi.pg_marg_rhs_bytes(N, "tri")
        runs = {"batched_g1": ("1", 0), "batched_g4": ("4", 0), "one_per_chunk": ("1", B)}
        ts = {k: [] for k in runs}
        ref = None; last = {}
        for rnd in range(9):
            for key, (G, mb) in runs.items():
                if key == "one_per_chunk" and rnd not in (0, 2, 5, 8):
                    continue
                os.environ["SLAMHIP_K27_GROUP"] = G
                spec = capi.pg_marg_spec(n_cg, check_every=32, precond="tri", tol=1e-9, max_bytes=mb)
                t0 = time.perf_counter(); b, cols, info = rep.PgMarginals(pairs, spec); dt = time.perf_counter() - t0
                ref = b if ref is None else ref
                assert b.tobytes() == ref.tobytes()
                last[key] = (cols, info)
                if rnd >= 2 or (key == "one_per_chunk" and rnd > 0):
                    ts[key].append(dt)
        os.environ.pop("SLAMHIP_K27_GROUP", None)
        rec = {"N": N, "E": int(g[1].shape[0]), "columns": 64, "rhs": 192, "n_cg": n_cg, "check_every": 32, "bytes_per_rhs": int(B)}
        for key in runs:
            cols, info = last[key]
            rec[key] = dict(stats(ts[key]), rhs_per_chunk=int(info["rhs_per_chunk"]), n_chunks=int(info["n_chunks"]), group=int(info["group"]),
                            launches=marg_launches(N, 1, cols, info, 32, n_cg), cg_iters_min=int(cols["cg_iters"].min()), cg_iters_max=int(cols["cg_iters"].max()),
                            stopped=sorted(set(cols["stopped"].tolist())))
        rec["one_per_chunk_over_batched_g1"] = rec["one_per_chunk"]["median_us"] / rec["batched_g1"]["median_us"]
        rec["batched_g4_over_batched_g1"] = rec["batched_g4"]["median_us"] / rec["batched_g1"]["median_us"]
        out["points"]["ring_loops16_%d" % N] = rec
        print(json.dumps(rec), flush=True)
    rep.close()
    ctx.close()
    if kres_path and os.path.exists(kres_path):                           # tools/kres.sh hs_pg.hip k27, one kernel per line
        import re
        out["kernel_resources"] = {}
        for line in open(kres_path):
            m = re.search(r"Name: (\S+).*?TotalSGPRs: (\d+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+).*?LDS Size \[bytes/block\]: (\d+)", line)
            if m:
                out["kernel_resources"][m.group(1)] = {"sgprs": int(m.group(2)), "vgprs": int(m.group(3)), "scratch_bytes_per_lane": int(m.group(4)),
                                                      "occupancy_waves_per_simd": int(m.group(5)), "lds_bytes": int(m.group(6))}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)


def main():
    if "--marginals" in sys.argv:
        rest = [a for a in sys.argv[1:] if a != "--marginals"]
        kres = None
        if "--kres" in rest:
            at = rest.index("--kres"); kres = rest[at + 1]; rest = rest[:at] + rest[at + 2:]
        marg_main(rest[0] if rest else os.path.join(ROOT, "profiles", "r34_hs_pg_marg.json"), kres)
        return
    if "--update-only" in sys.argv:
        print(json.dumps({"update": db.update_us(), "lib": os.environ.get("SLAMHIP_LIB", "this tree")}))
        return
    if "--variant-only" in sys.argv:
        print(json.dumps({"figures": variant_figures(), "lib": os.environ.get("SLAMHIP_LIB", "this tree")}))
        return
    if "--lm" in sys.argv:
        rest = [a for a in sys.argv[1:] if a != "--lm"]
        lm_main(rest[0] if rest else os.path.join(ROOT, "profiles", "r32_hs_pg_lm.json"))
        return
    if "--precond" in sys.argv:
        at = sys.argv.index("--precond")
        if sys.argv[at + 1] != "tri":
            raise SystemExit("--precond tri is the one there is (block-Jacobi is the default run)")
        rest = sys.argv[1:at] + sys.argv[at + 2:]
        tri_main(rest[0] if rest else os.path.join(ROOT, "profiles", "r28_hs_pg_tri.json"))
        return
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r25_hs_pg.json")
    ctx = hs.Context(0)
    rep = hs.MapRepMultiMap(0.1, (64, 64), 1, ctx=ctx)
    out = {"graphs": {}}
    for name, make in (("ring", ring), ("streets", streets)):
        for N in (1000, 10000, 100000, 1 << 20):
            poses, ij, z, w = make(N)
            reps, warm = (5, 1) if N > 100000 else (15, 3)
            rec = {"N": int(poses.shape[0]), "E": int(ij.shape[0])}
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter(); rep.PgSet(poses, None, ij, z, w); ts.append(time.perf_counter() - t0)
            rec["pg_set"] = stats(ts)
            rec.update(relax_figures(rep, poses, ij, z, w, reps, warm))
            t0 = time.perf_counter(); capi.debug_pg_relax(poses, None, ij, z, w, capi.pg_spec(1, 60, tol=0.0)); rec["host_hook_n_cg_60_us"] = (time.perf_counter() - t0) * 1e6
            if N <= 100000:
                t = scipy_step(poses, ij, z, w)
                rec["scipy_spsolve_step_us"] = None if t is None else t * 1e6
            out["graphs"]["%s_%d" % (name, N)] = rec
            print(name, N, json.dumps(rec), flush=True)
    rep.close()
    ctx.close()
    variants = os.path.join(ROOT, "slam.net_amd", "build", "variants")
    out["design_alternatives"] = {}
    for tag in ("k19_scalar", "k19_soa"):
        lib = os.path.join(variants, tag + ".so")
        if os.path.exists(lib):
            fig = child("--variant-only", lib)["figures"]
            for key, rec in fig.items():
                rec["same_poses_as_this_tree"] = rec["poses_sha1"] == out["graphs"][key]["poses_sha1"]
                rec["us_per_pcg_iteration_this_tree"] = out["graphs"][key]["us_per_pcg_iteration"]
            out["design_alternatives"][tag] = fig
            print(tag, json.dumps(fig), flush=True)
    parent = os.path.join(variants, "parent.so")
    if os.path.exists(parent):
        out["update_alternating"] = {"this_tree": [], "parent": []}
        for _ in range(3):
            out["update_alternating"]["this_tree"].append(child("--update-only", None)["update"])
            out["update_alternating"]["parent"].append(child("--update-only", parent)["update"])
        print(json.dumps(out["update_alternating"]), flush=True)
    out["update"] = db.update_us()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out["update"]))


if __name__ == "__main__":
    main()
