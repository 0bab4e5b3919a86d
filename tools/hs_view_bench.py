"""K15, the view gain of HectorSLAM (slamhip_hs_view_gain / slamhip_hs_view_select): wall clock per blocking call (median of 15
after a warm-up of 3, with min and max) on the 2048^2 x 3 pyramid from the simulator that the other K-benches use, with its 1080-beam
scan, levels 0 and 2.
 * view_gain at reach 64 and 255 (the seen bitmaps in LDS) and 300 on level 0 (513+ rows: the global-scratch path unforced), B = 1, 64
   and 4096 (a configuration the scratch bound refuses is recorded as refused), commit -1.
 * view_select with B = 256 and k = 8 at reach 64 and 255, mode 1, the layer set empty before every call.
 * The yardstick, in the same run: slamhip_hs_trace of the same poses and scan.  It walks the same lines (to their ends, not to
   `reach`) and neither marks nor counts cells.
 * Variants, each in a fresh interpreter: the default; every slot in global scratch (SLAMHIP_K15_GLOBAL=1); and every side build
   slam.net_amd/build/variants/k15_*.so that exists, under its tag -- `python tools/build_variant.py WORK k15_acc_word -DK15_ACC_LDS=1
   -DK15_ACC_GLOBAL=1` keeps a seen word's bits in a register and issues one atomic per word on both paths, `... k15_per_cell
   -DK15_ACC_LDS=0 -DK15_ACC_GLOBAL=0` one atomic per seen cell on both.
 * Existing path: HectorSLAMProcessor.Update per scan over the simulator's drive, median of 35; the new code is never entered on it.
`python tools/hs_view_bench.py [out.json]` writes profiles/r21_hs_view.json by default."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import hs_dfield_bench as db
import hs_trace_bench as tb

VARIANT_DIR = os.path.join(ROOT, "slam.net_amd", "build", "variants")
CONFIGS = [(0, 64), (0, 255), (0, 300), (2, 64), (2, 255)]                  # (level, reach)


def wall(ctx, fn):
    return tb.wall_us(ctx, fn, warm=3, reps=15, spread=True)


def variant_run(out_path, full):
    import slam.net_amd.capi as capi
    ctx, rep, scan, truth = tb.build_map(False)
    out = {"view_gain": {}, "view_select": {}, "trace": {}}
    for level, reach in CONFIGS:
        for B in (1, 64, 4096):
            poses = tb.poses_of(truth, B)
            key = "level%d_reach%d_B%d" % (level, reach, B)
            try:
                rec = wall(ctx, lambda: rep.view_gain(poses, level, reach))
                s = rep.view_gain(poses, level, reach)
                rec["pose0"] = {k: int(s[0][k]) for k in s.dtype.names}
                rec["seen_cells_per_s"] = round(float(s["n_seen"].astype(np.int64).sum()) / (rec["median_us"] * 1e-6), 0)
            except capi.SlamhipError as e:
                rec = {"refused": str(e)}
            out["view_gain"][key] = rec
            print("gain", key, json.dumps(rec), flush=True)
            if full and reach == 64:
                tkey = "level%d_B%d" % (level, B)
                out["trace"][tkey] = wall(ctx, lambda: rep.trace(poses, level))
                print("trace", tkey, json.dumps(out["trace"][tkey]), flush=True)
    for level, reach in ((0, 64), (0, 255)):
        poses = tb.poses_of(truth, 256)

        def select():
            rep.covered(level, clear=True)
            return rep.view_select(poses, level, reach, 8, mode=1, min_gain=1)
        empty = wall(ctx, lambda: rep.covered(level, clear=True))
        rec = wall(ctx, select)
        order, gains = select()
        rec["set_empty_layer_us"] = empty["median_us"]                       # (inside the timed call: the layer set empty and downloaded)
        rec["order"] = order.tolist(); rec["gains"] = gains.tolist()
        out["view_select"]["level%d_reach%d_B256_k8" % (level, reach)] = rec
        print("select", level, reach, json.dumps(rec), flush=True)
    rep.close(); ctx.close()
    with open(out_path, "w") as f:
        json.dump(out, f)


def main():
    if "--variant-run" in sys.argv:
        i = sys.argv.index("--variant-run")
        return variant_run(sys.argv[i + 1], sys.argv[i + 2] == "1")
    if "--update-only" in sys.argv:
        return print(json.dumps({"update": db.update_us(), "lib": os.environ.get("SLAMHIP_LIB", "this tree")}))
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r21_hs_view.json")
    out = {"map": tb.SIZE, "levels": tb.LEVELS, "rays": tb.RAYS, "warm": 3, "reps": 15, "variants": {}}
    variants = [("default", {}), ("global_scratch", {"SLAMHIP_K15_GLOBAL": "1"})]
    if os.path.isdir(VARIANT_DIR):
        for f in sorted(os.listdir(VARIANT_DIR)):
            if f.startswith("k15_") and f.endswith(".so"):
                variants.append((f[:-3], {"SLAMHIP_LIB": os.path.join(VARIANT_DIR, f)}))
    tmp = out_path + ".part"
    for k, (name, env) in enumerate(variants):
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--variant-run", tmp, "1" if k == 0 else "0"],
                           env=dict(os.environ, **env))
        if r.returncode != 0:
            raise SystemExit("variant %s ended with %d" % (name, r.returncode))
        out["variants"][name] = json.load(open(tmp))
        os.remove(tmp)
    d = out["variants"]["default"]
    out["view_gain_over_trace"] = {k: round(d["view_gain"]["level%s_reach64_B%s" % tuple(k.replace("level", "").split("_B"))]["median_us"] / v["median_us"], 3)
                                   for k, v in d["trace"].items()}
    out["update"] = db.update_us()
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"view_gain_over_trace": out["view_gain_over_trace"], "update": out["update"]}))


if __name__ == "__main__":
    main()
