"""K11, the cost-to-go field of HectorSLAM (slamhip_hs_nav_field): wall clock per blocking call (median of 15 after a warm-up) on the
2048^2 x 3 pyramid holding the room the K8 / K9 / K10 benches use.
 * The call on levels 0 and 2 of the window with clearance 0 and 8 (site_mask 2), one source at the robot's cell, no goals and no
   rectangle; `rounds` of each case from the call's summary.
 * On level 0, clearance 0: the bounding boxes of a K10 call's clusters (min_cells 4, at most 256) as goals with 16 paths of 4096
   cells; and the download of the whole level's cost rectangle.
 * The world: level 2 with its ring of 36 tiles of 64^2 cells.
 * The batch size: the level-0 call with SLAMHIP_NAV_BATCH = 1, 8 (the default) and 32.
 * For comparison, what a host-side planner would have to fetch first: slamhip_hs_world_cells_download of level 0, blocking.  No
   CPU Dijkstra is timed.
 * Existing path: HectorSLAMProcessor.Update of the trace bench's drive, blocking; the new code is never entered on it.
   `SLAMHIP_LIB=<a build of the parent commit> python tools/hs_nav_bench.py --update-only` prints the same figure for that build.
   `python tools/hs_nav_bench.py --merge-update-ab out.json log` stores the lines of such runs, made alternately, under "update_ab".
`python tools/hs_nav_bench.py [out.json]` writes profiles/r16_hs_nav.json by default."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import hs_dfield_bench as db
import hs_trace_bench as tb


def source_cell(rep, truth, level):
    cell = float(np.float32(rep.Maps[level].CellLength))
    return [(int(np.rint(float(truth[0]) / cell)), int(np.rint(float(truth[1]) / cell)))]


def merge_update_ab(path, log):
    d = json.load(open(path))
    d["update_ab"] = [json.loads(line) for line in open(log) if line.startswith("{")]
    with open(path, "w") as f:
        json.dump(d, f, indent=1)
        f.write("\n")


def main():
    if "--merge-update-ab" in sys.argv:
        return merge_update_ab(*sys.argv[sys.argv.index("--merge-update-ab") + 1:][:2])
    if "--update-only" in sys.argv:
        print(json.dumps({"update": db.update_us(), "lib": os.environ.get("SLAMHIP_LIB", "this tree")}))
        return
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r16_hs_nav.json")
    out = {"map": tb.SIZE, "levels": tb.LEVELS, "site_mask": 2, "nav": {}}
    ctx, rep, scan, truth = tb.build_map(False)
    for level in (0, 2):
        src = source_cell(rep, truth, level)
        for c in (0, 8):
            got = rep.nav_field(level, src, c)
            us = tb.wall_us(ctx, lambda: rep.nav_field(level, src, c))
            s = got["summary"]
            out["nav"]["level%d_clearance%d" % (level, c)] = {"us_per_blocking_call": round(us, 1), "summary": {k: int(s[k]) for k in s.dtype.names}}
    src = source_cell(rep, truth, 0)
    w, h = rep.Maps[0].Dimensions
    fr = rep.frontiers(0, 4, 256)[1]
    goals = np.stack([fr["x_min"], fr["y_min"], fr["x_max"], fr["y_max"]], 1)
    n_paths = min(16, goals.shape[0])
    got = rep.nav_field(0, src, goals=goals, n_paths=n_paths, max_path_cells=4096)
    out["nav"]["level0_goals_and_paths"] = {
        "us_per_blocking_call": round(tb.wall_us(ctx, lambda: rep.nav_field(0, src, goals=goals, n_paths=n_paths, max_path_cells=4096)), 1),
        "goals": int(goals.shape[0]), "goals_reached": int((got["goals"]["cost"] != 0xFFFFFFFF).sum()), "paths": n_paths,
        "path_cells": [int(v) for v in got["path_cells"]]}
    out["nav"]["level0_cost_rectangle"] = {
        "us_per_blocking_call": round(tb.wall_us(ctx, lambda: rep.nav_field(0, src, rect=(0, 0, w, h), want_dir=False), reps=7), 1), "cells": w * h}
    out["batch"] = {}
    for r in (1, 8, 32):
        os.environ["SLAMHIP_NAV_BATCH"] = str(r)
        out["batch"]["rounds_per_wait_%d" % r] = round(tb.wall_us(ctx, lambda: rep.nav_field(0, src)), 1)
    del os.environ["SLAMHIP_NAV_BATCH"]
    rep.close(); ctx.close()
    ctx, rep, scan, truth = tb.build_map(True)
    src = source_cell(rep, truth, 2)
    got = rep.nav_field(2, src, world=True)
    s = got["summary"]
    out["nav"]["level2_world"] = {"us_per_blocking_call": round(tb.wall_us(ctx, lambda: rep.nav_field(2, src, world=True)), 1),
                                  "summary": {k: int(s[k]) for k in s.dtype.names}}
    out["host_planner_would_first_download"] = {
        "world_cells_download_level0_us": round(tb.wall_us(ctx, lambda: rep.world_cells(0, 0, 0, w, h), reps=7), 1), "bytes": 8 * w * h}
    rep.close(); ctx.close()
    out["update"] = db.update_us()
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
