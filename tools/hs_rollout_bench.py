"""K12, command rollouts over the cost-to-go field (slamhip_hs_rollouts): wall clock per blocking call (median of 15 after a
warm-up) on the 2048^2 x 3 pyramid holding the room the K8 - K11 benches use.
 * Levels 0 and 2 of the window, clearance 0, one source 3 m from the robot, the start pose the robot's; B in {1, 4096, 65536}
   command sequences of 8 pairs held 8 steps each (T = 64), P in {0, 16} body points on a circle of 0.3 m.  For every case the whole
   call and, in the same run, slamhip_hs_nav_field alone with the same spec and source (no goals, no rectangle): the difference is
   what the rollouts add -- k12_count, k12_rollout, k12_emit, the two copies and one more wait.  The field build dominates; the
   difference of two medians of that size carries their noise, which "spread_us" (the field call's own max - min) shows.
 * pose x point tests: the sum over the rollouts of the poses tested (n_free, and the one that failed) times P + 1, over the
   difference.
 * The sub-group width: the level-2 calls (the shorter field build: less noise under the difference) with B = 256, 4096 and 65536
   and SLAMHIP_ROLLOUT_SG = 1 (a lane per rollout, the default) against 0 (a lane per item: the next power of two >= P + 1),
   alternating, 15 rounds.
 * The staged square: SLAMHIP_ROLLOUT_LDS = 1 (the traversable words of 256 x 256 cells around the start in LDS) against 0 (global
   memory throughout, the default), alternating, 15 rounds, a lane per rollout, P = 16, B = 4096 and 65536: on level 2, where every
   rollout stays inside the square (10 m to either side); on level 0, where the square is 2.5 m to either side and most rollouts
   leave it; and on level 0 from a start outside M.
 * For comparison, the first step of doing this on the host: the download of the whole level-0 cost rectangle, as
   tools/hs_nav_bench.py times it.
`python tools/hs_rollout_bench.py [out.json]` writes profiles/r17_hs_rollout.json by default."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import hs_trace_bench as tb

N_CMD, HOLD, DT = 8, 8, 0.1


def commands(B):
    g = np.random.default_rng(B)
    return np.stack([g.uniform(0.0, 1.0, (B, N_CMD)), g.uniform(-1.0, 1.0, (B, N_CMD))], 2).astype(np.float32)     # up to 1 m/s, 1 rad/s


def body(P):
    a = 2.0 * np.pi * np.arange(P) / max(P, 1)
    return np.stack([0.3 * np.cos(a), 0.3 * np.sin(a)], 1).astype(np.float32)


def spread(ctx, fn, reps=15):
    out = []
    for _ in range(reps):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(out)), float(max(out) - min(out))


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r17_hs_rollout.json")
    out = {"map": tb.SIZE, "levels": tb.LEVELS, "site_mask": 2, "clearance": 0, "n_cmd": N_CMD, "hold": HOLD, "T": N_CMD * HOLD, "dt": DT, "rollouts": {}}
    ctx, rep, scan, truth = tb.build_map(False)
    start = np.asarray(truth, np.float32)
    for level in (0, 2):
        cell = float(np.float32(rep.Maps[level].CellLength))
        src = [(int(np.rint((float(truth[0]) + 3.0) / cell)), int(np.rint(float(truth[1]) / cell)))]
        for _ in range(3):
            rep.nav_field(level, src)
        nav_us, nav_spread = spread(ctx, lambda: rep.nav_field(level, src))
        out["rollouts"]["level%d_nav_field_alone" % level] = {"us_per_blocking_call": round(nav_us, 1), "spread_us": round(nav_spread, 1)}
        for P in (0, 16):
            for B in (1, 4096, 65536):
                cmds, bd = commands(B), body(P)
                call = lambda: rep.rollouts(level, src, start, DT, cmds, HOLD, bd)
                res, sm = call()
                us = tb.wall_us(ctx, call)
                tested = int(np.minimum(res["n_free"] + 1, N_CMD * HOLD + 1).sum()) * (P + 1)
                add = us - nav_us
                out["rollouts"]["level%d_P%d_B%d" % (level, P, B)] = {
                    "us_per_blocking_call": round(us, 1), "added_by_the_rollouts_us": round(add, 1), "pose_x_point_tests": tested,
                    "tests_per_s": round(tested / (add * 1e-6)) if add > 0 else None, "n_complete": int(sm["n_complete"]),
                    "start_cost": int(sm["start_cost"]), "mean_n_free": round(float(res["n_free"].mean()), 2)}
    def ab(switch, arms, level, src, start, cmds, bd):
        """Two settings of one environment switch, alternating in this process -> {arm: {median_us, min_us}}."""
        times = {name: [] for name, _ in arms}
        for r in range(17):
            for name, value in arms:
                os.environ[switch] = value
                ctx.synchronize()
                t0 = time.perf_counter()
                rep.rollouts(level, src, start, DT, cmds, HOLD, bd)
                if r >= 2:
                    times[name].append((time.perf_counter() - t0) * 1e6)
        del os.environ[switch]
        return {k: {"median_us": round(float(np.median(v)), 1), "min_us": round(float(min(v)), 1)} for k, v in times.items()}

    src2 = src                                                             # (the last level of the loop above: 2)
    cell = float(np.float32(rep.Maps[0].CellLength))
    src = [(int(np.rint((float(truth[0]) + 3.0) / cell)), int(np.rint(float(truth[1]) / cell)))]
    out["subgroup_ab"] = {}
    for P in (1, 16):                                                      # (P = 0 is a lane per rollout either way)
        for B in (256, 4096, 65536):
            out["subgroup_ab"]["level2_P%d_B%d" % (P, B)] = ab("SLAMHIP_ROLLOUT_SG", (("lane_per_rollout", "1"), ("subgroup", "0")), 2, src2, start,
                                                               commands(B), body(P))
    out["lds_ab"] = {}
    arms = (("global_memory", "0"), ("staged_square", "1"))
    outside = np.array([-5.0, -5.0, 0.0], np.float32)
    for B in (4096, 65536):
        cmds, bd = commands(B), body(16)
        out["lds_ab"]["level2_inside_the_square_B%d" % B] = ab("SLAMHIP_ROLLOUT_LDS", arms, 2, src2, start, cmds, bd)
        out["lds_ab"]["level0_leaves_the_square_B%d" % B] = ab("SLAMHIP_ROLLOUT_LDS", arms, 0, src, start, cmds, bd)
        out["lds_ab"]["level0_start_outside_M_B%d" % B] = ab("SLAMHIP_ROLLOUT_LDS", arms, 0, src, outside, cmds, bd)
    far = rep.rollouts(0, src, start, DT, commands(4096), HOLD, body(16))[0]
    half = 128 * cell                                                      # how many of the rollouts end outside the level-0 square
    out["lds_ab"]["level0_share_ending_outside_the_square"] = round(float(((np.abs(far["x"] - start[0]) > half) | (np.abs(far["y"] - start[1]) > half)).mean()), 3)
    w, h = rep.Maps[0].Dimensions
    out["host_side_would_first_download"] = {
        "level0_cost_rectangle_us": round(tb.wall_us(ctx, lambda: rep.nav_field(0, src, rect=(0, 0, w, h), want_dir=False), reps=7), 1), "cells": w * h}
    rep.close(); ctx.close()
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
