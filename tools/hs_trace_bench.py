"""K8, the beam trace of HectorSLAM (slamhip_hs_trace): wall clock per blocking call (median of 15 after a warm-up) and cells
looked up per second, on a 2048^2 x 3 pyramid from the simulator with 1080 rays, levels 0 and 2, B in {1, 64, 4096}, over the
window and over the world (the ring of 64^2 tiles that hs_lattice_bench.py --world builds around the level-2 window).  The cells
a call looks up are counted from its own beam records (first + 1, or da + 1 where the beam meets nothing, plus the extra look-up
of end_class for a blocked beam), fetched outside the timing in pieces of at most 2^20 records.
Yardsticks of the same session: the blocking slamhip_hs_update_by_scan of the same scan (it walks the same lines on all levels,
and writes), and K7's node x points rate from profiles/r12_hs_world_lattice.json.
`python tools/hs_trace_bench.py [out.json]` writes profiles/r13_hs_trace.json by default.  The trace has no timing class: the
kernel's own time comes from a run of its own under `rocprofv3 --kernel-trace --stats -- python tools/hs_trace_bench.py --kernel-run
LEVEL B WORLD`, which issues 10 traces of that one configuration and nothing else after the map is built; `--merge-kernel-us
out.json KEY US` writes such a figure into the profile."""
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import slam.net_amd.capi as capi
import slam.net_amd.hector as hs
import slam.net_amd.sim as sim

SIZE, LEVELS, RAYS = 2048, 3, 1080
CELL = 40.0 / SIZE
PIECE = (1 << 20) // RAYS                                                  # poses per call with beam records


def build_map(world):
    ctx = hs.Context(0)
    rep = hs.MapRepMultiMap(CELL, (SIZE, SIZE), LEVELS, ctx=ctx)
    if world:
        rep.set_backing(64, 512 << 20)
    segs = sim.default_field(); rng = sim.PCG32(1234); traj = sim.trajectory(25)
    for p in traj[:-1]:
        rep.UpdateByScan(hs.ScanCloud(sim.make_scan(segs, p, RAYS, rng)[1]), p)
    truth = traj[-1]
    scan = hs.ScanCloud(sim.make_scan(segs, truth, RAYS, rng)[1])
    if world:                                                              # a ring of 64^2 tiles around the 512^2 window of level 2
        w2 = SIZE >> 2
        g = np.random.default_rng(3)
        for x0, y0, w, h in ((-64, -64, w2 + 128, 64), (-64, w2, w2 + 128, 64), (-64, 0, 64, w2), (w2, 0, 64, w2)):
            cells = np.zeros((h, w), capi.CELL_DTYPE)
            cells["update_index"] = 1
            cells["value"] = g.uniform(-2.0, 2.0, (h, w)).astype(np.float32)
            assert rep.world_put(2, x0, y0, cells) == 0
    rep.set_scan(scan)
    return ctx, rep, scan, truth


def poses_of(truth, B):
    g = np.random.default_rng(B)
    p = np.tile(truth, (B, 1)).astype(np.float64)
    p[1:, 0:2] += g.uniform(-1.0, 1.0, (B - 1, 2)); p[1:, 2] += g.uniform(-0.5, 0.5, B - 1)
    return p.astype(np.float32)


def lookups(rep, poses, level, world):
    n = 0
    for i in range(0, poses.shape[0], PIECE):
        _, b = rep.trace(poses[i:i + PIECE], level, world=world, beams=True)
        walked = b["da"] >= 1
        n += int(np.where(b["first"] >= 0, b["first"] + 1, b["da"] + 1)[walked].sum()) + int((walked & (b["first"] >= 0) & (b["first"] < b["da"])).sum())
    return n


def wall_us(ctx, fn, warm=3, reps=15, spread=False):
    """Median microseconds per call; spread=True: a dict with the median, the least and the greatest."""
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e6)
    if spread:
        return {"median_us": round(float(np.median(out)), 2), "min_us": round(float(np.min(out)), 2), "max_us": round(float(np.max(out)), 2)}
    return float(np.median(out))


def kernel_run(argv):
    level, B, world = int(argv[0]), int(argv[1]), bool(int(argv[2]))
    ctx, rep, scan, truth = build_map(world)
    poses = poses_of(truth, B)
    for _ in range(10):
        rep.trace(poses, level, world=world)
    rep.close(); ctx.close()


def merge(argv):
    path, key, us = argv[0], argv[1], float(argv[2])
    d = json.load(open(path))
    d.setdefault("kernel_us_rocprofv3", {})[key] = us
    with open(path, "w") as f:
        json.dump(d, f, indent=1)
        f.write("\n")


def main():
    if "--kernel-run" in sys.argv:
        return kernel_run(sys.argv[sys.argv.index("--kernel-run") + 1:])
    if "--merge-kernel-us" in sys.argv:
        return merge(sys.argv[sys.argv.index("--merge-kernel-us") + 1:])
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r13_hs_trace.json")
    out = {"map": SIZE, "levels": LEVELS, "cell_m": CELL, "traces": {}}
    for world in (False, True):
        ctx, rep, scan, truth = build_map(world)
        out["points"] = int(scan.Points.shape[0])
        for level in (0, 2):
            for B in (1, 64, 4096):
                poses = poses_of(truth, B)
                n = lookups(rep, poses, level, world)
                us = wall_us(ctx, lambda: rep.trace(poses, level, world=world))
                sums, _ = rep.trace(poses, level, world=world)
                out["traces"]["%s_level%d_B%d" % ("world" if world else "window", level, B)] = {
                    "us_per_blocking_call": round(us, 2), "cells_looked_up": n, "cells_per_s": n / (us * 1e-6),
                    "beams_per_s": B * scan.Points.shape[0] / (us * 1e-6),
                    "pose0": {k: int(sums[0][k]) for k in sums.dtype.names}}
        if not world:                                                      # the yardstick last: it writes the map
            p = capi.f32(truth)                                            # (the scan is set: slamhip_hs_update_by_scan alone, as the trace is timed)
            out["update_by_scan_us_per_blocking_call"] = round(wall_us(ctx, lambda: (capi.call("slamhip_hs_update_by_scan", rep._h, capi.fptr(p)), ctx.synchronize())), 2)
        rep.close(); ctx.close()
    t = out["traces"]["window_level0_B1"]
    out["trace_B1_level0_vs_update"] = round(t["us_per_blocking_call"] / out["update_by_scan_us_per_blocking_call"], 3)
    try:
        r12 = json.load(open(os.path.join(ROOT, "profiles", "r12_hs_world_lattice.json")))
        out["k7_node_points_per_s"] = r12["nodes"] * r12["points"] / (r12["window_search"]["device_us_search"] * 1e-6)
    except (OSError, KeyError) as e:
        out["k7_node_points_per_s"] = "not available: %r" % (e,)
    out["kernel_us_rocprofv3"] = {}
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
