"""K19, the pose-graph relaxation (slamhip_hs_pg_set, _pg_relax): wall clock per blocking call, each figure beside a host solve FROM
THE SAME RUN.
 * Graphs: the ring of tests/test_hs_pg_abi.py (N nodes, N edges) and a grid of streets (k x k nodes, an edge to the right and the
   upper neighbour: about 2 N edges), at N = 10^3, 10^4, 10^5 and 2^20; true relative poses plus Gaussian noise, node 0 fixed.
 * relax: ONE Gauss-Newton step with tol = 0, so that exactly n_cg PCG iterations run, at n_cg = 10 and 60 with check_every = n_cg;
   median, min and max of 15 blocking calls after a warm-up of 3 (5 after 1 at 2^20), the graph set again before each.  The time per
   PCG iteration is the difference of the two medians over 50.  pg_set is timed on its own.
 * Host: the same Gauss-Newton step (libm trig) as a sparse system solved by scipy.sparse.linalg.spsolve, when scipy is there and
   N <= 10^5, once; and slamhip_debug_pg_relax, the library's own host loops, for the same 60 iterations.
 * The two design alternatives, each a developer build of this tree in slam.net_amd/build/variants/ (`python tools/build_variant.py
   WORK k19_scalar -DK19_SCALAR_LAUNCH=1`: alpha, beta and the stop word by a one-workgroup launch behind k19_apply and behind k19_step,
   five launches per iteration; `... WORK k19_soa -DK19_SOA=1`: the node vectors as three arrays of N doubles), when they are there:
   the same relax figures at 10^5 and 2^20 nodes, each library in a fresh interpreter (`--variant-only` with SLAMHIP_LIB set), the
   poses after the 60 iterations hashed and compared with this tree's.
 * Existing path: HectorSLAMProcessor.Update of the trace bench's scan, blocking, median of 35 scans; the new code is never entered on
   it.  With a build of the parent commit at slam.net_amd/build/variants/parent.so (`python tools/build_variant.py HEAD~1 parent`) the
   figure is taken in alternating fresh interpreters, this tree then the parent, three each (`--update-only` with SLAMHIP_LIB set).
`python tools/hs_pg_bench.py [out.json]` writes profiles/r25_hs_pg.json by default."""
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


def child(flag, lib):
    """This script again in a fresh interpreter with `lib` (None: this tree's) -> the JSON object it printed last."""
    env = dict(os.environ)
    env.pop("SLAMHIP_LIB", None)
    if lib:
        env["SLAMHIP_LIB"] = lib
    r = subprocess.run([sys.executable, os.path.abspath(__file__), flag], env=env, stdout=subprocess.PIPE, timeout=300, check=True)
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


def main():
    if "--update-only" in sys.argv:
        print(json.dumps({"update": db.update_us(), "lib": os.environ.get("SLAMHIP_LIB", "this tree")}))
        return
    if "--variant-only" in sys.argv:
        print(json.dumps({"figures": variant_figures(), "lib": os.environ.get("SLAMHIP_LIB", "this tree")}))
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
