"""K17, the Hough transform of HectorSLAM's map (slamhip_hs_hough, _hough_rotation, _hough_shifts, HectorSLAMProcessor.AlignMaps):
wall clock per blocking call (median of 15 after 3) on a 2048^2 x 3 pyramid from the simulator with 1080 rays, each figure beside
its yardstick FROM THE SAME RUN.
 * Fill: slamhip_hs_hough of slot 0 on levels 0 and 2 for T = 180, 360 and q = 0, 1 with site_mask 2 -- the table's copy, the class
   map's pack, the memset of H, k17_vote, k17_spectrum, the spectrum's copy and the wait.  It has no timing class, so it is the
   blocking call, not the launches alone.
 * The host-side alternative it replaces, per level: slamhip_hs_world_cells_download of the level plus a NumPy Hough of the same
   sites (one bincount over sites x angles), at T = 180, q = 0.
 * Shifts: the source is the level-0 map's own middle (1536 x 1536 cells, first cell (37, -512) in its own frame); hough_shifts at
   P = 2 and 16 for T = 360, q = 1; slamhip_hs_merge_score of 4096 poses for scale; AlignMaps end to end (two fills, the rotation
   scores, one hough_shifts, one merge_score) and the first hypothesis it returns (the truth: theta = 0, t = (219, 768) cells).
 * Existing path: HectorSLAMProcessor.Update of the trace bench's scan, blocking, median of 35 scans; the new code is never entered on
   it.  `SLAMHIP_LIB=<a build of the parent commit> python tools/hs_hough_bench.py --update-only` prints the same figure for that
   build; run the two alternately.
`python tools/hs_hough_bench.py [out.json]` writes profiles/r23_hs_hough.json by default."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import slam.net_amd.hector as hs                                           # noqa: E402
from slam.net_amd import capi                                              # noqa: E402

import hs_dfield_bench as db                                               # noqa: E402
import hs_trace_bench as tb                                                # noqa: E402
import slam.net_amd.sim as sim                                             # noqa: E402


def np_hough(values, T, q):
    """The votes of the occupied cells of `values` by NumPy on the host -> (H, HS)."""
    h, w = values.shape
    D = w + h; N = ((2 * D) >> q) + 1
    C, S = capi.debug_hough_table(T)
    j, i = np.nonzero(values > 0)
    p = (i[:, None].astype(np.int64) * C[None, :] + j[:, None].astype(np.int64) * S[None, :] + D * 16384) >> (14 + q)
    H = np.bincount((np.arange(T, dtype=np.int64)[None, :] * N + p).ravel(), minlength=T * N).reshape(T, N)
    return H, (H.astype(np.uint64) ** 2).sum(1)


def host_us(fn, warm=1, reps=5):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(out))


def main():
    if "--update-only" in sys.argv:
        print(json.dumps({"update": db.update_us(), "lib": os.environ.get("SLAMHIP_LIB", "this tree")}))
        return
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r23_hs_hough.json")
    ctx = hs.Context(0)
    proc = hs.HectorSLAMProcessor(tb.CELL, (tb.SIZE, tb.SIZE), (20.0, 20.0, 0.0), tb.LEVELS, ctx=ctx)
    rep = proc.MapRep
    segs = sim.default_field(); rng = sim.PCG32(1234)
    for p in sim.trajectory(25)[:-1]:
        rep.UpdateByScan(hs.ScanCloud(sim.make_scan(segs, p, tb.RAYS, rng)[1]), p)
    out = {"map": tb.SIZE, "levels": tb.LEVELS, "site_mask": 2, "fill": {}, "host_alternative": {}, "shifts": {}}
    for level in (0, 2):
        w, h = rep.Maps[level].Dimensions
        for T in (180, 360):
            for q in (0, 1):
                rec = tb.wall_us(ctx, lambda: rep.hough(level, 0, False, 2, T, q), spread=True)
                info, _, _ = rep.hough(level, 0, False, 2, T, q)
                rec.update({"n_sites": info["n_sites"], "N": info["N"], "votes": info["n_sites"] * T})
                out["fill"]["level%d_T%d_q%d" % (level, T, q)] = rec
        try:                                                               # (the world download needs no backing store: world = window)
            download, which = (lambda: rep.world_cells(level, 0, 0, w, h)), "slamhip_hs_world_cells_download"
            download()
        except capi.SlamhipError:
            download, which = (lambda: rep.Maps[level].GetCells()), "slamhip_hs_cells_download"
        dl = tb.wall_us(ctx, download)
        values = download()["value"].reshape(h, w)
        nh = host_us(lambda: np_hough(values, 180, 0))
        _, hs_dev, H_dev = rep.hough(level, 0, False, 2, 180, 0, H=True)
        H_np, hs_np = np_hough(values, 180, 0)
        out["host_alternative"]["level%d_T180_q0" % level] = {
            "download": which, "download_us": round(dl, 2), "numpy_hough_us": round(nh, 2), "sum_us": round(dl + nh, 2),
            "equal_to_device": bool(np.array_equal(H_np, H_dev) and np.array_equal(hs_np, hs_dev))}
    # the source: the level-0 map's own middle under another first cell
    cells0 = rep.Maps[0].GetCells().reshape(tb.SIZE, tb.SIZE)
    src = np.ascontiguousarray(cells0[256:1792, 256:1792])
    ax, ay = 37, -512
    proc.merge_set_source(0, ax, ay, src)
    T, q = 360, 1
    rep.hough(0, 0, False, 2, T, q)
    out["fill"]["source_level0_T360_q1"] = tb.wall_us(ctx, lambda: rep.hough(0, 1, False, 2, T, q), spread=True)
    g = np.random.default_rng(2)
    for P in (2, 16):
        pairs = np.stack([g.integers(0, 2 * T, P), g.integers(0, T, P)], 1).astype(np.int32)
        pairs[0] = (0, 0)
        out["shifts"]["P%d" % P] = tb.wall_us(ctx, lambda: rep.hough_shifts(pairs), spread=True)
    out["rotation_host_us"] = round(host_us(rep.hough_rotation), 2)
    poses = np.zeros((4096, 3), np.float32)
    poses[:, 0] = g.uniform(0.0, 40.0, 4096); poses[:, 1] = g.uniform(0.0, 40.0, 4096); poses[:, 2] = g.uniform(-3.1, 3.1, 4096)
    out["merge_score_4096_poses"] = tb.wall_us(ctx, lambda: proc.merge_score(poses), spread=True)
    out["align_maps"] = tb.wall_us(ctx, lambda: proc.AlignMaps(0, T=T, q=q), warm=1, reps=7, spread=True)
    hyp = proc.AlignMaps(0, T=T, q=q)
    stm = 1.0 / tb.CELL
    out["align_maps"]["first"] = {"m": int(hyp[0]["m"]), "pose_cells": [float(hyp[0]["pose"][0]) * stm, float(hyp[0]["pose"][1]) * stm, float(hyp[0]["pose"][2])],
                                  "truth_cells": [256 - ax, 256 - ay, 0.0], "joint4": [int(h_["report"]["joint"][4]) for h_ in hyp]}
    proc.Dispose(); ctx.close()
    out["update"] = db.update_us()
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
