"""K14, the map merge of HectorSLAM (slamhip_hs_merge_score / slamhip_hs_merge_apply): wall clock per blocking call (median of 15
after a warm-up of 3, with min and max for the spread) on the 2048^2 x 3 pyramid from the simulator that the other K-benches use.
The source is the level's own download, set once; the poses turn it about the window's centre.
 * apply: level 1 (1024^2) and level 0 (2048^2) at theta = 0, 0.3 and pi / 4, rule ADD with a limit nothing reaches, so every apply
   changes every sourced cell whose source cell has a class.  Each of the four variants of k14_apply -- the 32 x 32 and the 64 x 32
   tile, staged in LDS and with direct gathers (SLAMHIP_K14_TILE32, SLAMHIP_K14_STAGED) -- runs in a fresh interpreter, one after the
   other.  Beside the time: the bytes the definition moves -- 8 per destination cell read, 12 more per changed cell written (20 per
   changed cell in all), 4 per sourced cell of source -- and the fraction of the 8 TB/s HBM peak that implies.
 * score: B = 1, 64, 1024 poses on both levels: microseconds per blocking call and cells x poses per second.
`python tools/hs_merge_bench.py [out.json]` writes profiles/r20_hs_merge.json by default."""
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import hs_trace_bench as tb

HBM_PEAK = 8.0e12                                                          # bytes per second
THETAS = (("0", 0.0), ("0.3", 0.3), ("pi/4", math.pi / 4))
VARIANTS = (("tile32_staged", {"SLAMHIP_K14_TILE32": "1", "SLAMHIP_K14_STAGED": "1"}), ("tile32_direct", {"SLAMHIP_K14_TILE32": "1"}),
            ("tile64_staged", {"SLAMHIP_K14_STAGED": "1"}), ("tile64_direct", {}))           # the last is what the library runs by default


def wall(ctx, fn):
    return tb.wall_us(ctx, fn, warm=3, reps=15, spread=True)


def pose_about_centre(n, cell, theta):
    """The source frame turned by theta about the window's centre cell (n / 2, n / 2), a fraction of a cell off the grid."""
    c = n / 2.0
    return np.array([(c - (math.cos(theta) * c - math.sin(theta) * c) + 0.3) * cell, (c - (math.sin(theta) * c + math.cos(theta) * c) - 0.2) * cell, theta],
                    np.float32)


def variant_run(out_path, with_score):
    ctx, rep, scan, truth = tb.build_map(False)
    out = {"apply": {}, "score": {}}
    for level in (1, 0):
        n = tb.SIZE >> level
        cell = tb.CELL * (1 << level)
        cells = rep.Maps[level].GetCells().reshape(n, n)
        rep.merge_set_source(level, 0, 0, cells)
        for name, theta in THETAS:
            pose = pose_about_centre(n, cell, theta)
            rec = wall(ctx, lambda: rep.merge_apply(pose, 0, 1.0e30))
            r = rep.merge_apply(pose, 0, 1.0e30)
            sourced = int(sum(int(v) for v in r["joint"]))
            rec["n_changed"] = int(r["n_changed"]); rec["n_sourced"] = sourced
            rec["bytes_definition"] = 8 * n * n + 12 * int(r["n_changed"]) + 4 * sourced
            rec["hbm_fraction_implied"] = round(rec["bytes_definition"] / (rec["median_us"] * 1e-6) / HBM_PEAK, 4)
            out["apply"]["%d_theta_%s" % (n, name)] = rec
            print("apply", n, name, json.dumps(rec), flush=True)
            rep.Maps[level].SetCells(cells.ravel())                        # (the sums grow: back to the map as it was)
        if with_score:
            for B in (1, 64, 1024):
                g = np.random.default_rng(B)
                poses = np.stack([pose_about_centre(n, cell, t) for t in g.uniform(-math.pi, math.pi, B)])
                poses[:, :2] += g.uniform(-2.0, 2.0, (B, 2)).astype(np.float32)
                rec = wall(ctx, lambda: rep.merge_score(poses))
                rec["cell_poses_per_s"] = round(n * n * B / (rec["median_us"] * 1e-6), 0)
                out["score"]["%d_B%d" % (n, B)] = rec
                print("score", n, B, json.dumps(rec), flush=True)
    rep.close(); ctx.close()
    with open(out_path, "w") as f:
        json.dump(out, f)


def main():
    if "--variant-run" in sys.argv:
        i = sys.argv.index("--variant-run")
        return variant_run(sys.argv[i + 1], sys.argv[i + 2] == "1")
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r20_hs_merge.json")
    out = {"map": tb.SIZE, "levels": tb.LEVELS, "warm": 3, "reps": 15, "hbm_peak_bytes_per_s": HBM_PEAK, "rule": "ADD, limit 1e30",
           "source": "the level's own cells", "apply": {}, "score": {}}
    tmp = out_path + ".part"
    for k, (name, env) in enumerate(VARIANTS):
        r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--variant-run", tmp, "1" if k == 0 else "0"],
                           env=dict(os.environ, **env))
        if r.returncode != 0:
            raise SystemExit("variant %s ended with %d" % (name, r.returncode))
        part = json.load(open(tmp))
        os.remove(tmp)
        out["apply"][name] = part["apply"]
        if k == 0:
            out["score"] = part["score"]
    best = {}
    for key in out["apply"][VARIANTS[0][0]]:
        best[key] = min(VARIANTS, key=lambda v: out["apply"][v[0]][key]["median_us"])[0]
    out["fastest_apply_variant"] = best
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(best))


if __name__ == "__main__":
    main()
