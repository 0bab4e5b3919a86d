"""K23: the consistent set of loop edges on the device (slamhip_hs_loops_consistent) beside the host hook
(slamhip_debug_loops_consistent) on the same inputs, in the same process -> profiles/r29_hs_loops.json.

  python tools/hs_loops_bench.py [--edges 256,1024,4096] [--starts 8] [--reps 9] [--warmup 2] [--hook-reps 1] [--out profiles/r29_hs_loops.json]

Per L two inputs: "all" -- every pair consistent, the worst case of the set search (L rounds per start over all L rows) -- and
"planted" -- one consistent set of L / 4 among edges consistent with nothing.  The edges hang between the two ends of a chain of 2 L
nodes (i = k, j = L + k), the poses on a line, so that s, rho2 and the lever arm take part.  Wall clock per blocking call, median
of `reps` after `warmup`; the hook, plain loops on one host thread, is timed `hook-reps` times.  Both results are compared: a row
with "equal": false is a bug."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import slam.net_amd.capi as capi        # noqa: E402
import slam.net_amd.hector as hs        # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def inputs(L, planted):
    N = 2 * L
    poses = np.zeros((N, 3)); poses[:, 0] = 0.25 * np.arange(N)
    ij = np.stack([np.arange(L), L + np.arange(L)], axis=1).astype(np.int32)
    z = np.zeros((L, 3)); z[:, 0] = 0.25 * L                               # the odometry's own answer: every pair closes exactly
    if planted:
        g = np.random.Generator(np.random.Philox(L))
        out = np.ones(L, bool); out[g.permutation(L)[:L // 4]] = False
        z[out, 1] = 50.0 * (1 + np.arange(int(out.sum())))                 # each 50 m from every other: consistent with nothing
    w = np.tile(np.array([2500.0, 2500.0, 10000.0]), (L, 1))
    return poses, ij, z, w


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); t.append((time.perf_counter() - t0) * 1e3)
    return {"median": float(np.median(t)), "min": float(min(t)), "max": float(max(t))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edges", default="256,1024,4096")
    ap.add_argument("--starts", type=int, default=8)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--hook-reps", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r29_hs_loops.json"))
    a = ap.parse_args()
    ctx = hs.Context(0)
    rep = hs.MapRepMultiMap(0.125, (64, 64), 1, ctx=ctx)
    sp = capi.loops_spec(11.34, 1e-4, 2e-5, n_starts=a.starts)
    rows = []
    for L in (int(v) for v in a.edges.split(",")):
        for planted in (False, True):
            poses, ij, z, w = inputs(L, planted)
            res = {}

            def dev():
                res["d"] = rep.LoopsConsistent(poses, ij, z, w, sp, adj=True)

            def dev_plain():
                res["p"] = rep.LoopsConsistent(poses, ij, z, w, sp)

            def hook():
                res["h"] = capi.debug_loops_consistent(poses, ij, z, w, sp, adj=True)
            t_plain = median_ms(dev_plain, a.reps, a.warmup)
            t_adj = median_ms(dev, a.reps, a.warmup)
            t_hook = median_ms(hook, a.hook_reps, 0)
            d, h = res["d"], res["h"]
            equal = bool(np.array_equal(d["keep"], h["keep"]) and np.array_equal(d["deg"], h["deg"]) and np.array_equal(d["adj"], h["adj"]) and d["info"] == h["info"]
                         and np.array_equal(res["p"]["keep"], h["keep"]))
            row = {"L": L, "input": "planted" if planted else "all", "n_starts": a.starts, "size": int(d["info"]["size"]), "n_pairs": int(d["info"]["n_pairs"]),
                   "device_ms": t_plain, "device_with_matrix_ms": t_adj, "hook_ms": t_hook, "ratio_hook_over_device": t_hook["median"] / t_plain["median"],
                   "equal": equal}
            print(json.dumps(row), flush=True)
            rows.append(row)
    rep.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
