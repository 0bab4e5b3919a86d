"""K21: a list of stored-scan pairs matched in one call (slamhip_hs_scans_match) beside what a caller of the same library had to do
per pair without it, in the same process -> profiles/r27_hs_scanmatch.json.

  python tools/hs_scanmatch_bench.py [--pairs 64,1024,4096] [--reps 15] [--warmup 3] [--rays 1080] [--out profiles/r27_hs_scanmatch.json]

The call: H = 192, a 33 x 33 x 33 lattice, scale 8 cells per metre; wall clock per blocking call, median of `reps` after `warmup`.
A call takes at most 2^26 nodes, 1867 pairs of this lattice: a longer list goes in several calls ("calls"), timed together.
The old way, per pair, on a second small handle (512 x 512 cells of 0.125 m, one level): reset, set_scan(reference),
update_by_scan at the centre, set_scan(query), slamhip_hs_lattice_search with the same lattice -- four blocking calls and a reset;
timed per pair (median of `reps` pairs after `warmup`) and multiplied by the pair count.  The two score different rasters (hit and
near cells against occupied and free cells): times only, no agreement.  The scans are 64 distinct simulated scans of `rays` rays
used in turn.  With slam.net_amd/build/variants/parent.so present -- a build of the parent commit -- it also times the EXISTING
path, HectorSLAMProcessor.Update per scan (hs_dfield_bench.update_us), in alternating fresh interpreters, this tree then the parent,
three each -> "update_alternating"."""
import argparse
import json
import math
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import slam.net_amd.capi as capi        # noqa: E402
import slam.net_amd.hector as hs        # noqa: E402
import slam.net_amd.sim as sim          # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hs_dfield_bench as db            # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE, HALF, NXY, NT, DTHETA = 8.0, 192, 16, 16, 2.0 * math.pi / 1024.0


def child(args, lib=None):
    env = dict(os.environ)
    env.pop("SLAMHIP_LIB", None)
    if lib:
        env["SLAMHIP_LIB"] = lib
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=env, stdout=subprocess.PIPE, timeout=600, check=True)
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(min(t)), float(max(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="64,1024,4096")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rays", type=int, default=1080)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27_hs_scanmatch.json"))
    ap.add_argument("--update-only", action="store_true")
    a = ap.parse_args()
    if a.update_only:
        print(json.dumps({"update": db.update_us(), "lib": os.environ.get("SLAMHIP_LIB", "this tree")}))
        return
    segs = sim.default_field()
    lap, _ = sim.lap_trajectory(step=0.75)
    scans = [sim.make_scan(segs, p, a.rays, noise=False)[1] for p in lap[:64]]
    ctx = hs.Context(0)
    rep = hs.MapRepMultiMap(0.125, (64, 64), 1, ctx=ctx)
    for s in scans:
        rep.ScansAdd(hs.ScanCloud(s, (0.0, 0.0, 0.0)))
    sp = capi.scanmatch_spec(SCALE, HALF, NXY, NXY, NT, DTHETA, margin=8)
    old = hs.MapRepMultiMap(0.125, (512, 512), 1, ctx=ctx)
    centre = (32.0, 32.0, 0.0)
    state = {"i": 0}

    def old_pair():
        i = state["i"]; state["i"] += 1
        ref, qry = scans[i % 64], scans[(i + 1) % 64]
        old.Reset()
        old.UpdateByScan(hs.ScanCloud(ref, (0.0, 0.0, 0.0)), centre)
        old.lattice_search(hs.ScanCloud(qry, (0.0, 0.0, 0.0)), 0, centre, NXY, NXY, 2 * NT + 1, DTHETA)
    old_ms = median_ms(old_pair, a.reps, a.warmup)
    rows = []
    for n in (int(v) for v in a.pairs.split(",")):
        pairs = capi.scan_pairs([(i % 64, (i + 1) % 64, (0.0, 0.0, 0.0)) for i in range(n)])
        res = {}

        per_call = capi.SCANMATCH_MAX_CALL_NODES // ((2 * NXY + 1) ** 2 * (2 * NT + 1))    # 1867 pairs of this lattice: a call takes 2^26 nodes

        def call():
            res["r"] = np.concatenate([rep.scans_match(sp, pairs[i:i + per_call]) for i in range(0, n, per_call)])
        ms = median_ms(call, a.reps, a.warmup)
        row = {"pairs": n, "calls": -(-n // per_call), "points": int(np.mean([s.shape[0] for s in scans])), "half": HALF, "lattice": [2 * NXY + 1, 2 * NXY + 1, 2 * NT + 1],
               "scans_match_ms": {"median": ms[0], "min": ms[1], "max": ms[2]}, "us_per_pair": 1e3 * ms[0] / n,
               "old_way_ms_per_pair": {"median": old_ms[0], "min": old_ms[1], "max": old_ms[2]}, "old_way_ms": old_ms[0] * n,
               "ratio_old_over_new": old_ms[0] * n / ms[0], "valid": int((res["r"]["cnt"] > 0).sum())}
        print(json.dumps(row), flush=True)
        rows.append(row)
    rep.close(); old.close()
    out = {"rows": rows}
    parent = os.path.join(ROOT, "slam.net_amd", "build", "variants", "parent.so")
    if os.path.exists(parent):
        out["update_alternating"] = {"this_tree": [], "parent": []}
        for _ in range(3):
            out["update_alternating"]["this_tree"].append(child(["--update-only"])["update"])
            out["update_alternating"]["parent"].append(child(["--update-only"], parent)["update"])
        print(json.dumps(out["update_alternating"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
