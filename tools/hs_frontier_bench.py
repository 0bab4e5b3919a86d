"""K10, the frontier clusters of HectorSLAM (slamhip_hs_frontiers): wall clock per blocking call (median of 15 after a warm-up) on the
2048^2 x 3 pyramid holding the room the K8 / K9 benches use.
 * The call on levels 0 and 2, window and world (backing on; level 2 carries the ring of 36 tiles of 64^2 cells), min_cells 1,
   max_clusters 256, without labels and with a label rectangle of the whole level -- into arrays made once, so the figure is the
   library's call alone.  It has no timing class: this is the blocking call (pack, six or seven launches, one wait, the host's
   sort), not its launches one by one.
 * Beside each figure, from the same run: K7's pack launch of that level (its timing class, device time; the window's pack) and
   slamhip_hs_distance_field at r = 8 of a 1 x 1 rectangle, blocking -- one pass over the class map, and a two-pass field over it.
 * Existing path: HectorSLAMProcessor.Update of the trace bench's drive, blocking; the new code is never entered on it.
   `SLAMHIP_LIB=<a build of the parent commit> python tools/hs_frontier_bench.py --update-only` prints the same figure for that build.
`python tools/hs_frontier_bench.py [out.json]` writes profiles/r15_hs_frontier.json by default."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import slam.net_amd.capi as capi

import hs_dfield_bench as db
import hs_trace_bench as tb


def main():
    if "--update-only" in sys.argv:
        print(json.dumps({"update": db.update_us(), "lib": os.environ.get("SLAMHIP_LIB", "this tree")}))
        return
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r15_hs_frontier.json")
    out = {"map": tb.SIZE, "levels": tb.LEVELS, "min_cells": 1, "max_clusters": 256, "frontiers": {}}
    for world in (False, True):
        ctx, rep, scan, truth = tb.build_map(world)
        for level in (0, 2):
            w, h = rep.Maps[level].Dimensions
            s = np.zeros(1, capi.FRONTIER_SUMMARY); rec = np.zeros(256, capi.FRONTIER_CLUSTER); lab = np.empty((h, w), np.int32)
            vp = lambda a: a.ctypes.data_as(C.c_void_p)                    # noqa: E731

            def call(labels):
                capi.call("slamhip_hs_frontiers", rep._h, level, 1 if world else 0, 1, 256, vp(s), vp(rec), 0, 0, w, h, vp(lab) if labels else None)
            us = tb.wall_us(ctx, lambda: call(False))
            us_l = tb.wall_us(ctx, lambda: call(True))
            df = tb.wall_us(ctx, lambda: rep.distance_field(level, (0, 0, 1, 1), site_mask=2, radius=8, world=world))
            e = {"us_per_blocking_call": round(us, 2), "us_with_full_level_labels": round(us_l, 2),
                 "distance_field_r8_us_per_blocking_call": round(df, 2), "summary": {k: int(s[0][k]) for k in s.dtype.names},
                 "largest": {k: int(rec[0][k]) for k in rec.dtype.names} if s[0]["n_returned"] else None}
            e["M_cells_per_s"] = int(s[0]["mw"]) * int(s[0]["mh"]) / (us * 1e-6)
            if not world:
                ctx.timing_enable(1 << capi.K_HS_LATTICE_PACK); ctx.timing_reset()
                for _ in range(10):
                    call(False)
                ms, n = ctx.timing_get(capi.K_HS_LATTICE_PACK)
                e["k7_pack_device_us"] = round(ms * 1e3 / max(n, 1), 2)
                ctx.timing_enable(0)
            out["frontiers"]["level%d_%s" % (level, "world" if world else "window")] = e
        rep.close(); ctx.close()
    out["update"] = db.update_us()
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
