"""K16, the nearest-site field of HectorSLAM (slamhip_hs_nearest_field, slamhip_hs_nearest_pairs): wall clock per blocking call
(median of 15 after 3) on a 2048^2 x 3 pyramid from the simulator with 1080 rays, each figure beside its yardstick FROM THE SAME RUN.
 * Field build: slamhip_hs_nearest_field of a 1 x 1 rectangle -- the class map's pack, k16_rows, k16_cols, a one-cell gather and
   the wait -- on levels 0 and 2 for r = 8, 32, 255 with site_mask 2, beside slamhip_hs_distance_field of the same arguments, and
   their ratio.  Neither has a timing class, so both are the blocking call, not the launches alone.
 * Pairs: B = 1, 64, 4096 at r = 32, beside slamhip_hs_distance_score of the same poses, and their ratio.
 * Existing path: HectorSLAMProcessor.Update of the trace bench's scan, blocking, median of 35 scans; the new code is never entered on
   it.  `SLAMHIP_LIB=<a build of the parent commit> python tools/hs_nearest_bench.py --update-only` prints the same figure for that
   build; run the two alternately.
`python tools/hs_nearest_bench.py [out.json]` writes profiles/r22_hs_nearest.json by default."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import slam.net_amd.hector as hs                                           # noqa: F401 (the library is loaded before the benches import it)

import hs_dfield_bench as db
import hs_trace_bench as tb


def main():
    if "--update-only" in sys.argv:
        print(json.dumps({"update": db.update_us(), "lib": os.environ.get("SLAMHIP_LIB", "this tree")}))
        return
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r22_hs_nearest.json")
    ctx, rep, scan, truth = tb.build_map(False)
    out = {"map": tb.SIZE, "levels": tb.LEVELS, "points": int(scan.Points.shape[0]), "site_mask": 2, "field": {}, "pairs": {}}
    for level in (0, 2):
        w, h = rep.Maps[level].Dimensions
        for r in (8, 32, 255):
            us = tb.wall_us(ctx, lambda: rep.nearest_field(level, (0, 0, 1, 1), site_mask=2, radius=r))
            k9 = tb.wall_us(ctx, lambda: rep.distance_field(level, (0, 0, 1, 1), site_mask=2, radius=r))
            n = rep.nearest_field(level, (0, 0, w, h), site_mask=2, radius=r)
            out["field"]["level%d_r%d" % (level, r)] = {
                "us_per_blocking_call": round(us, 2), "distance_field_us_per_blocking_call": round(k9, 2), "ratio": round(us / k9, 3),
                "E_cells": (w + 2 * r) * (h + 2 * r), "none_fraction_in_window": float((n[..., 0] == 32767).mean())}
    for B in (1, 64, 4096):
        poses = tb.poses_of(truth, B)
        for level in (0, 2):
            us = tb.wall_us(ctx, lambda: rep.nearest_pairs(poses, level, site_mask=2, radius=32))
            k9 = tb.wall_us(ctx, lambda: rep.distance_score(poses, level, site_mask=2, radius=32))
            sums, _ = rep.nearest_pairs(poses, level, site_mask=2, radius=32)
            out["pairs"]["level%d_B%d" % (level, B)] = {"us_per_blocking_call": round(us, 2), "distance_score_us_per_blocking_call": round(k9, 2),
                                                       "ratio": round(us / k9, 3), "pose0": {k: int(sums[0][k]) for k in sums.dtype.names}}
    rep.close(); ctx.close()
    out["update"] = db.update_us()
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
