"""K13, the particle-filter localisation step of HectorSLAM (slamhip_hs_mcl_step): wall clock per blocking call (median of 15 after a
warm-up of 3, with min and max for the spread) on the 2048^2 x 3 pyramid from the simulator with 1080 rays that the other K-benches
use, for N = 256, 4096, 65536 particles, levels 0 and 2, r = 8 and 32, with resampling forced (n_eff_min = N + 1) and off (0).
In the SAME run, for the same N poses:
 * slamhip_hs_distance_score, blocking: the field build and the score the step contains.  step - score is what predict, weigh, scan and
   resample cost (the score call also moves N x 12 bytes in and N x 24 out, which the step does not).
 * the host-side alternative the step replaces: the score call, then in NumPy the costs, exp weights, the prefix sum and a systematic
   resampling (searchsorted), the gather of the new poses and normal noise for the next prediction -- one filter step done on the
   host around the device's score.
`python tools/hs_mcl_bench.py [out.json]` writes profiles/r18_hs_mcl.json by default.
`python tools/hs_mcl_bench.py --k9-ab out.json parent=a.json this=b.json ...` puts several runs of tools/hs_dfield_bench.py -- this
commit's build and the parent's, alternating -- side by side (profiles/r18_k9_ab.json): hs_dfield.hip changed in linkage only."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import slam.net_amd.capi as capi

import hs_trace_bench as tb


def wall(ctx, fn):
    return tb.wall_us(ctx, fn, warm=3, reps=15, spread=True)


def k9_ab(argv):
    """--k9-ab out.json label=file ...: the figures of several tools/hs_dfield_bench.py runs (label `parent` or `this`, in the order
    they were made) side by side, with the range of each figure per label."""
    runs = []
    for a in argv[1:]:
        label, path = a.split("=", 1)
        e = json.load(open(path))
        fig = {"field_" + k: v["us_per_blocking_call"] for k, v in e["field"].items() if isinstance(v, dict)}
        fig.update({"score_" + k: v["us_per_blocking_call"] for k, v in e["score"].items()})
        fig["update_median"] = e["update"]["median_us"]
        runs.append({"build": label, "us": fig})
    ranges = {}
    for name in runs[0]["us"]:
        ranges[name] = {lab: [min(r["us"][name] for r in runs if r["build"] == lab), max(r["us"][name] for r in runs if r["build"] == lab)]
                        for lab in sorted({r["build"] for r in runs})}
    out = {"tool": "tools/hs_dfield_bench.py, the builds alternating in one session on one machine", "runs_in_order": runs, "range_us": ranges}
    with open(argv[0], "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(ranges))


def host_step(rep, poses, level, r, sigma_cells, rng):
    """One filter step on the host around slamhip_hs_distance_score -> the next poses."""
    sums, _ = rep.distance_score(poses, level, site_mask=2, radius=r)
    cost = sums["sum_d2"].astype(np.float64) + float(r * r) * sums["n_ignored"]
    w = np.exp(-(cost - cost.min()) / (2.0 * sigma_cells ** 2 * 135.0))
    c = np.cumsum(w)
    n = poses.shape[0]
    anc = np.minimum(np.searchsorted(c, (np.arange(n) + rng.random()) * (c[-1] / n), side="right"), n - 1)
    nxt = poses[anc]
    nxt += (rng.standard_normal((n, 3)) * (0.02, 0.02, 0.01)).astype(np.float32)
    return nxt


def main():
    if "--k9-ab" in sys.argv:
        return k9_ab(sys.argv[sys.argv.index("--k9-ab") + 1:])
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r18_hs_mcl.json")
    ctx, rep, scan, truth = tb.build_map(False)
    rep.set_scan(scan)
    out = {"map": tb.SIZE, "levels": tb.LEVELS, "points": int(scan.Points.shape[0]), "site_mask": 2, "warm": 3, "reps": 15, "steps": {}}
    rng = np.random.default_rng(5)
    for N in (256, 4096, 65536):
        poses = tb.poses_of(truth, N)
        for level in (0, 2):
            for r in (8, 32):
                key = "N%d_level%d_r%d" % (N, level, r)
                rec = {}
                beta = capi.mcl_beta(2.0, 135.0)
                for name, n_eff_min in (("resample", N + 1), ("no_resample", 0)):
                    rep.mcl_set(poses)
                    stream = [0]

                    def step():
                        stream[0] += 1
                        return rep.mcl_step(capi.mcl_spec(level, r, (0.02, 0.0, 0.005), (0.02, 0.02, 0.01), beta, n_eff_min, seed=9, stream=stream[0]))
                    rec["step_" + name] = wall(ctx, step)
                    s = step()
                    rec["step_" + name]["last_summary"] = {k: int(s[k]) for k in ("resampled", "n_distinct", "cost_min", "cost_max", "n_unplaced")}
                rec["score"] = wall(ctx, lambda: rep.distance_score(poses, level, site_mask=2, radius=r))
                cur = [poses.copy()]

                def host():
                    cur[0] = host_step(rep, cur[0], level, r, 2.0, rng)
                rec["host_alternative"] = wall(ctx, host)
                rec["step_minus_score_us"] = round(rec["step_resample"]["median_us"] - rec["score"]["median_us"], 2)
                rec["host_minus_step_us"] = round(rec["host_alternative"]["median_us"] - rec["step_resample"]["median_us"], 2)
                out["steps"][key] = rec
                print(key, json.dumps(rec), flush=True)
    rep.close(); ctx.close()
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
