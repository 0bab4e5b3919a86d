"""K20: the render of N stored scans in one call (slamhip_hs_render) beside the same library's sequential loop of set_scan +
update_by_scan in the same process -> one JSON line per (trajectory, N).  The library has no enqueue-only Hector update, so the
loop is what a caller has today: N blocking slamhip_hs_update_by_scan calls, each with its own wait.

  python tools/hs_render_bench.py [--n 64,1024,10000] [--reps 15] [--warmup 3] [--rays 1080] [--out profiles/r26_hs_render.json]

It runs itself once per tile side in a fresh interpreter (SLAMHIP_K20_TILE is read once per process; --rows-only is that child) and
writes {"rows_tile_32": [...], "rows_tile_64": [...]}.  With slam.net_amd/build/variants/parent.so present -- a build of the parent
commit -- it also times the EXISTING path, HectorSLAMProcessor.Update per scan (median of 35 scans, hs_dfield_bench.update_us), in
alternating fresh interpreters, this tree then the parent, three each (--update-only with SLAMHIP_LIB set) -> "update_alternating".

Trajectories: "lap" (the simulator's lap, the keyframes spread evenly over it) and "spot" (every keyframe within a few centimetres
of one place: the worst case for tile balance -- every scan reaches the same tiles).  The scans are 64 distinct simulated scans
of `rays` points used in turn (casting 10^4 scans on the host would take longer than the measurement).  Wall clock per blocking
call, median of `reps` after `warmup`; both forms must leave equal checksums on every level or the run fails.  The tile side is
the library's (SLAMHIP_K20_TILE in the environment selects 64)."""
import argparse
import json
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


def poses_for(kind, n, lap):
    if kind == "lap":
        return lap[(np.arange(n) * len(lap)) // n].astype(np.float32)
    rng = np.random.default_rng(5)
    p = np.tile(lap[0], (n, 1))
    p[:, :2] += rng.normal(0, 0.03, (n, 2))
    p[:, 2] += rng.normal(0, 0.02, n)
    return p.astype(np.float32)


def child(args, env_extra, lib=None):
    """This script again in a fresh interpreter -> the JSON object it printed last."""
    env = dict(os.environ)
    env.pop("SLAMHIP_LIB", None); env.pop("SLAMHIP_K20_TILE", None)
    env.update(env_extra)
    if lib:
        env["SLAMHIP_LIB"] = lib
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=env, stdout=subprocess.PIPE, timeout=600, check=True)
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="64,1024,10000")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rays", type=int, default=1080)
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows-only", action="store_true")
    ap.add_argument("--update-only", action="store_true")
    a = ap.parse_args()
    if a.update_only:
        print(json.dumps({"update": db.update_us(), "lib": os.environ.get("SLAMHIP_LIB", "this tree")}))
        return
    if a.rows_only:
        print(json.dumps({"rows": rows_of(a)}))
        return
    common = ["--n", a.n, "--reps", str(a.reps), "--warmup", str(a.warmup), "--rays", str(a.rays), "--rows-only"]
    out = {"tool": "tools/hs_render_bench.py", "device": "one MI355X", "map": "2048 x 2048 x 3 levels, 0.02 m", "reps": a.reps, "warmup": a.warmup,
           "loop": "N blocking slamhip_hs_set_scan + slamhip_hs_update_by_scan calls of the same library in the same process: a host wait per scan"}
    for tile in (32, 64):
        out["rows_tile_%d" % tile] = child(common, {"SLAMHIP_K20_TILE": str(tile)})["rows"]
        for row in out["rows_tile_%d" % tile]:
            print(json.dumps(row), flush=True)
    parent = os.path.join(ROOT, "slam.net_amd", "build", "variants", "parent.so")
    if os.path.exists(parent):
        out["update_alternating"] = {"this_tree": [], "parent": []}
        for _ in range(3):
            out["update_alternating"]["this_tree"].append(child(["--update-only"], {})["update"])
            out["update_alternating"]["parent"].append(child(["--update-only"], {}, parent)["update"])
        print(json.dumps(out["update_alternating"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


def rows_of(a):
    ctx = hs.Context(0)
    segs = sim.default_field()
    lap, _ = sim.lap_trajectory()
    rng = sim.PCG32(7)
    base = [sim.make_scan(segs, lap[(k * len(lap)) // 64], a.rays, rng)[1] for k in range(64)]
    rows = []
    for kind in ("lap", "spot"):
        for n in [int(v) for v in a.n.split(",")]:
            poses = poses_for(kind, n, lap)
            rep = hs.MapRepMultiMap(0.02, (2048, 2048), 3, ctx=ctx)
            ref = hs.MapRepMultiMap(0.02, (2048, 2048), 3, ctx=ctx)
            clouds = [hs.ScanCloud(s) for s in base]
            for k in range(n):
                rep.ScansAdd(clouds[k % 64])
            org = capi.f32((0.0, 0.0))
            t_render, t_loop = [], []
            for it in range(a.warmup + a.reps):
                t0 = time.perf_counter()
                rep.Render(poses)
                t1 = time.perf_counter()
                ref.Reset()
                ctx.synchronize()
                t2 = time.perf_counter()
                for k in range(n):
                    s = base[k % 64]
                    capi.call("slamhip_hs_set_scan", ref._h, capi.fptr(s), s.shape[0], capi.fptr(org))
                    capi.call("slamhip_hs_update_by_scan", ref._h, capi.fptr(poses[k]))
                t3 = time.perf_counter()
                if it >= a.warmup:
                    t_render.append(t1 - t0); t_loop.append(t3 - t2)
            equal = all(rep.Maps[l].checksum() == ref.Maps[l].checksum() for l in range(3))
            row = {"trajectory": kind, "n_scans": n, "rays": a.rays, "tile": int(os.environ.get("SLAMHIP_K20_TILE", "32")),
                   "render_ms": 1e3 * float(np.median(t_render)), "loop_ms": 1e3 * float(np.median(t_loop)),
                   "loop_over_render": float(np.median(t_loop) / np.median(t_render)), "checksums_equal": bool(equal)}
            print(json.dumps(row), file=sys.stderr, flush=True)
            rows.append(row)
            rep.close(); ref.close()
            if not equal:
                raise SystemExit("the render and the loop left different maps")
    ctx.close()
    return rows


if __name__ == "__main__":
    main()
