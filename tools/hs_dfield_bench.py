"""K9, the distance field of HectorSLAM (slamhip_hs_distance_field, slamhip_hs_distance_score): wall clock per blocking call (median
of 15 after a warm-up) on a 2048^2 x 3 pyramid from the simulator with 1080 rays.
 * Field build: slamhip_hs_distance_field of a 1 x 1 rectangle -- the class map's pack, k9_rows, k9_cols, a one-cell gather and the
   wait -- on levels 0 and 2 for r = 8, 32, 255 with site_mask 2.  The field has no timing class, so this is the blocking call, not
   the two launches alone; beside it, from the same run: K7's window pack launch of that level (its timing class, device time) and
   a device-to-device copy of the field's bytes (E cells x 2, torch, blocking).
 * Score: B = 1 and B = 4096 at r = 32 as blocking wall clock, beside slamhip_hs_trace of the same poses.
 * Existing path: HectorSLAMProcessor.Update of the trace bench's scan, blocking, median of 15; the new code is never entered on it.
   `SLAMHIP_LIB=<a build of the parent commit> python tools/hs_dfield_bench.py --update-only` prints the same figure for that build.
`python tools/hs_dfield_bench.py [out.json]` writes profiles/r14_hs_dfield.json by default."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import slam.net_amd.capi as capi
import slam.net_amd.hector as hs
import slam.net_amd.sim as sim

import hs_trace_bench as tb

SIZE, LEVELS, RAYS = tb.SIZE, tb.LEVELS, tb.RAYS


def update_us():
    """HectorSLAMProcessor.Update, blocking, over a short drive: median microseconds per scan."""
    ctx = hs.Context(0)
    proc = hs.HectorSLAMProcessor(tb.CELL, (SIZE, SIZE), (20.0, 20.0, 0.0), LEVELS, ctx=ctx)
    segs = sim.default_field(); rng = sim.PCG32(1234); traj = sim.trajectory(40)
    scans = [hs.ScanCloud(sim.make_scan(segs, p, RAYS, rng)[1]) for p in traj]
    out = []
    for i, (s, p) in enumerate(zip(scans, traj)):
        ctx.synchronize()
        t0 = time.perf_counter()
        proc.Update(s, p)
        proc.MatchPose
        ctx.synchronize()
        if i >= 5:
            out.append((time.perf_counter() - t0) * 1e6)
    proc.Dispose(); ctx.close()
    return {"median_us": round(float(np.median(out)), 2), "min_us": round(float(np.min(out)), 2), "max_us": round(float(np.max(out)), 2), "scans": len(out)}


def main():
    if "--update-only" in sys.argv:
        print(json.dumps({"update": update_us(), "lib": os.environ.get("SLAMHIP_LIB", "this tree")}))
        return
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r14_hs_dfield.json")
    import torch
    ctx, rep, scan, truth = tb.build_map(False)
    out = {"map": SIZE, "levels": LEVELS, "points": int(scan.Points.shape[0]), "site_mask": 2, "field": {}, "score": {}}
    for level in (0, 2):
        w, h = rep.Maps[level].Dimensions
        for r in (8, 32, 255):
            us = tb.wall_us(ctx, lambda: rep.distance_field(level, (0, 0, 1, 1), site_mask=2, radius=r))
            e_cells = (w + 2 * r) * (h + 2 * r)
            a = torch.empty(e_cells, dtype=torch.int16, device="cuda"); b = torch.empty_like(a)

            def copy():
                b.copy_(a); torch.cuda.synchronize()
            f = rep.distance_field(level, (0, 0, w, h), site_mask=2, radius=r)
            out["field"]["level%d_r%d" % (level, r)] = {
                "us_per_blocking_call": round(us, 2), "E_cells": e_cells, "cells_per_s": e_cells / (us * 1e-6),
                "d2d_copy_of_F_us_blocking": round(tb.wall_us(ctx, copy), 2),
                "capped_fraction_in_window": float((f == r * r).mean())}
        ctx.timing_enable(1 << capi.K_HS_LATTICE_PACK); ctx.timing_reset()
        for _ in range(10):
            rep.distance_field(level, (0, 0, 1, 1), site_mask=2, radius=8)
        ms, n = ctx.timing_get(capi.K_HS_LATTICE_PACK)
        out["field"]["level%d_k7_pack_device_us" % level] = round(ms * 1e3 / max(n, 1), 2)
        ctx.timing_enable(0)
    for B in (1, 4096):
        poses = tb.poses_of(truth, B)
        for level in (0, 2):
            us = tb.wall_us(ctx, lambda: rep.distance_score(poses, level, site_mask=2, radius=32))
            ut = tb.wall_us(ctx, lambda: rep.trace(poses, level))
            sums, _ = rep.distance_score(poses, level, site_mask=2, radius=32)
            out["score"]["level%d_B%d" % (level, B)] = {"us_per_blocking_call": round(us, 2), "trace_us_per_blocking_call": round(ut, 2),
                                                       "pose0": {k: int(sums[0][k]) for k in sums.dtype.names}}
    rep.close(); ctx.close()
    out["update"] = update_us()
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
