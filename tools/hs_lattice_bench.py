"""K7, the pose-lattice search of HectorSLAM (slamhip_hs_lattice_search / slamhip_hs_relocalise): us per blocking call between two
device synchronisations after a warm-up, the device time of its two launches (pack, search) from the context's event timing in a
run of its own, node x points per second, the end-to-end Relocalise(B = 16), and in the same run MatchDataBest over hint lattices
of several sizes -- how many full matches the same time buys.  Workloads: a 2048^2 x 3 pyramid from the simulator, 1080 rays;
level 2 (512^2) with nx = ny = 64, n_theta = 180 (about 3.0 M nodes: the staged-rectangle path) and level 0 with a small lattice
(the global-memory path).  `python tools/hs_lattice_bench.py [out.json]`; writes profiles/r11_hs_lattice.json by default.

`--world [out.json]` (profiles/r12_hs_world_lattice.json): the world search (slamhip_hs_world_lattice_search) at the same size --
(a) the window search's two launches, event-timed per launch, medians; with `--parent-lib PATH` the same figures from a build of
the parent commit, measured in a child process of the same session (SLAMHIP_LIB), which is the yardstick for the search kernel;
(b) the world search with a ring of 64^2 tiles around the level-2 window: pack per cell of R beside the window pack per cell of
the window, and its search launch beside (a)'s; (c) RelocaliseWorld(B = 16) with the window 256 x 128 cells off the robot: wall
clock per call, the device time of its search and its match from the events, and a shift of the same size with its restore, wall
clock.  `--window-only` prints (a) alone (what the child process runs)."""
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


def timed(ctx, fn, warm=3, reps=20):
    for _ in range(warm):
        fn()
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) / reps * 1e6


def device_split(ctx, fn, reps=10):
    """ms of the pack and the search launches per call, from events around each launch (a run of its own: the events cost)."""
    fn()
    ctx.timing_enable((1 << capi.K_HS_LATTICE_PACK) | (1 << capi.K_HS_LATTICE))
    ctx.timing_reset()
    for _ in range(reps):
        fn()
    pack, n_pack = ctx.timing_get(capi.K_HS_LATTICE_PACK)
    search, n_search = ctx.timing_get(capi.K_HS_LATTICE)
    ctx.timing_enable(0)
    assert n_pack == n_search == reps
    return pack / reps * 1e3, search / reps * 1e3


def per_launch(ctx, fn, classes, warm=3, reps=15):
    """Median us per call of each kernel class, from events around each launch; one call per reading."""
    for _ in range(warm):
        fn()
    mask = 0
    for k in classes:
        mask |= 1 << k
    ctx.timing_enable(mask)
    rows = []
    for _ in range(reps):
        ctx.timing_reset()
        fn()
        rows.append([ctx.timing_get(k)[0] * 1e3 for k in classes])
    ctx.timing_enable(0)
    return [round(float(v), 2) for v in np.median(np.array(rows), axis=0)]


def build_map(backing):
    ctx = hs.Context(0)
    rep = hs.MapRepMultiMap(CELL, (SIZE, SIZE), LEVELS, ctx=ctx)
    if backing:
        rep.set_backing(64, 512 << 20)
    segs = sim.default_field(); rng = sim.PCG32(1234); traj = sim.trajectory(25)
    for p in traj[:-1]:
        rep.UpdateByScan(hs.ScanCloud(sim.make_scan(segs, p, RAYS, rng)[1]), p)
    truth = traj[-1]
    scan = hs.ScanCloud(sim.make_scan(segs, truth, RAYS, rng)[1])
    centre = (truth + np.array([1.0, -0.8, math.radians(40.0)], np.float32)).astype(np.float32)
    rep.set_scan(scan)
    return ctx, rep, scan, truth, centre


def window_figures(ctx, rep, lat):
    pack, search = per_launch(ctx, lambda: rep.lattice_search(None, *lat), (capi.K_HS_LATTICE_PACK, capi.K_HS_LATTICE))
    return {"device_us_pack": pack, "device_us_search": search, "us_per_blocking_call": round(timed(ctx, lambda: rep.lattice_search(None, *lat)), 2)}


def world_main(argv):
    import subprocess
    parent_lib = None
    if "--parent-lib" in argv:
        i = argv.index("--parent-lib")
        parent_lib = os.path.abspath(argv[i + 1])
        del argv[i:i + 2]
    window_only = "--window-only" in argv
    argv = [a for a in argv if not a.startswith("--")]
    out_path = argv[0] if argv else os.path.join(ROOT, "profiles", "r12_hs_world_lattice.json")
    ctx, rep, scan, truth, centre = build_map(backing=False)
    lat = (2, centre, 64, 64, 180, np.float32(math.radians(2.0)))
    nodes = 180 * 129 * 129
    win = window_figures(ctx, rep, lat)
    if window_only:
        rep.close(); ctx.close()
        print(json.dumps(win))
        return
    out = {"map": SIZE, "levels": LEVELS, "level": 2, "points": int(scan.Points.shape[0]), "nodes": nodes, "window_search": win}
    rep.close(); ctx.close()                                               # (one process on the device at a time)
    if parent_lib:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--world", "--window-only"], env=dict(os.environ, SLAMHIP_LIB=parent_lib),
                           stdout=subprocess.PIPE, check=True, timeout=300)
        out["window_search_parent"] = json.loads(r.stdout.decode().strip().splitlines()[-1])
        out["search_launch_vs_parent"] = round(win["device_us_search"] / out["window_search_parent"]["device_us_search"], 4)
    else:
        out["window_search_parent"] = "not measured (no --parent-lib)"
    ctx, rep, scan, truth, centre = build_map(backing=True)
    lat = (2, centre, 64, 64, 180, np.float32(math.radians(2.0)))
    # (b) a ring of 64^2 tiles around the 512^2 window of level 2: four strips of cells that are not Reset
    w2 = SIZE >> 2
    rng = np.random.default_rng(3)
    for x0, y0, w, h in ((-64, -64, w2 + 128, 64), (-64, w2, w2 + 128, 64), (-64, 0, 64, w2), (w2, 0, 64, w2)):
        cells = np.zeros((h, w), capi.CELL_DTYPE)
        cells["update_index"] = 1
        cells["value"] = rng.uniform(-2.0, 2.0, (h, w)).astype(np.float32)
        assert rep.world_put(2, x0, y0, cells) == 0
    tiles2 = 4 * (w2 // 64) + 4
    assert rep.backing_stats()["tiles"] == tiles2
    r_cells = (w2 + 128) ** 2
    pack_w, search_w = per_launch(ctx, lambda: rep.world_lattice_search(None, *lat), (capi.K_HS_LATTICE_PACK_WORLD, capi.K_HS_LATTICE))
    keys_w, _ = rep.world_lattice_search(None, *lat)
    keys, _ = rep.lattice_search(None, *lat)
    out["world_search"] = {
        "tiles": tiles2, "r_cells": r_cells, "device_us_pack_world": pack_w, "device_us_search": search_w,
        "note": "device_us_pack_world is the pack launch alone; the memset of R's words ahead of it is not inside the events",
        "us_per_blocking_call": round(timed(ctx, lambda: rep.world_lattice_search(None, *lat)), 2),
        "pack_ps_per_cell_of_r": round(pack_w * 1e6 / r_cells, 2), "window_pack_ps_per_cell": round(win["device_us_pack"] * 1e6 / (w2 * w2), 2),
        "search_vs_window_search": round(search_w / win["device_us_search"], 4), "same_best_node_as_window": bool(keys_w.max() == keys.max())}
    rep.close(); ctx.close()
    # (c) RelocaliseWorld(B = 16): the window 256 x 128 cells off the robot's, the lattice around the same world pose
    ctx, rep, scan, truth, centre = build_map(backing=True)
    m = hs.ScanMatcher(1)
    away = (256, -128)
    rep.shift(*away)
    off = np.array([np.float32(away[0]) * np.float32(CELL), np.float32(away[1]) * np.float32(CELL), 0.0], np.float32)
    cw = (centre - off).astype(np.float32)
    lat = (2, cw, 64, 64, 180, np.float32(math.radians(2.0)))
    classes = (capi.K_HS_LATTICE_PACK_WORLD, capi.K_HS_LATTICE, capi.K_HS_MATCH)
    rows, walls, shifts = [], [], []
    for i in range(3 + 10):
        timing = i >= 3
        ctx.timing_enable(sum(1 << k for k in classes) if timing else 0)
        ctx.timing_reset()
        pose, rpt, info = m.RelocaliseWorld(rep, scan, *lat, B=16)
        if timing:
            rows.append([ctx.timing_get(k)[0] * 1e3 for k in classes])
        ctx.timing_enable(0)
        q = (int(info["dx"]), int(info["dy"]))
        rep.shift(-q[0], -q[1])                                            # back, outside the timing; then the same move alone, with its restore
        ctx.synchronize()
        t2 = time.perf_counter()
        rep.shift(*q)
        ctx.synchronize()
        t3 = time.perf_counter()
        rep.shift(-q[0], -q[1])
        if timing:
            shifts.append((t3 - t2) * 1e6)
    # wall clock without the event timers: a run of its own
    for i in range(3 + 10):
        ctx.synchronize()
        t0 = time.perf_counter()
        pose, rpt, info = m.RelocaliseWorld(rep, scan, *lat, B=16)
        t1 = time.perf_counter()
        if i >= 3:
            walls.append((t1 - t0) * 1e6)
        rep.shift(-int(info["dx"]), -int(info["dy"]))
    med = [round(float(v), 2) for v in np.median(np.array(rows), axis=0)]
    ox, oy = rep.origin()
    world = [float(pose[0]) + (ox + int(info["dx"])) * CELL, float(pose[1]) + (oy + int(info["dy"])) * CELL, float(pose[2])]
    out["relocalise_world_B16"] = {
        "window_off_by_cells": list(away), "shift_applied": [int(info["dx"]), int(info["dy"])], "us_per_call_wall": round(float(np.median(walls)), 2),
        "device_us_pack_world": med[0], "device_us_search": med[1], "device_us_match": med[2],
        "us_shift_and_restore_wall_with_sync": round(float(np.median(shifts)), 2),
        "error_m": math.hypot(world[0] - float(truth[0]), world[1] - float(truth[1])), "residual": float(rpt["residual"]),
        "info": {n: int(info[n]) for n in info.dtype.names}}
    rep.close(); ctx.close()
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


def main():
    if "--world" in sys.argv:
        return world_main([a for a in sys.argv[1:] if a != "--world"])
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r11_hs_lattice.json")
    ctx = hs.Context(0)
    rep = hs.MapRepMultiMap(CELL, (SIZE, SIZE), LEVELS, ctx=ctx)
    segs = sim.default_field(); rng = sim.PCG32(1234); traj = sim.trajectory(25)
    for p in traj[:-1]:
        rep.UpdateByScan(hs.ScanCloud(sim.make_scan(segs, p, RAYS, rng)[1]), p)
    truth = traj[-1]
    scan = hs.ScanCloud(sim.make_scan(segs, truth, RAYS, rng)[1])
    n_pts = scan.Points.shape[0]
    centre = (truth + np.array([1.0, -0.8, math.radians(40.0)], np.float32)).astype(np.float32)
    m = hs.ScanMatcher(1)
    rep.set_scan(scan)
    out = {"map": SIZE, "levels": LEVELS, "cell_m": CELL, "points": int(n_pts), "searches": {}}
    for name, (level, nx, ny, n_theta, dth) in (("level2_129x129x180", (2, 64, 64, 180, math.radians(2.0))),
                                                ("level0_17x17x36_global_path", (0, 8, 8, 36, math.radians(10.0)))):
        lat = (level, centre, nx, ny, n_theta, np.float32(dth))
        nodes = n_theta * (2 * nx + 1) * (2 * ny + 1)
        us_call = timed(ctx, lambda: rep.lattice_search(None, *lat))
        pack_us, search_us = device_split(ctx, lambda: rep.lattice_search(None, *lat))
        keys, _ = rep.lattice_search(None, *lat)
        k = max(range(n_theta), key=lambda i: int(keys[i]))
        score, flat = hs.decode_lattice_key(keys[k])
        node = rep.lattice_node_pose(*lat, k, flat)
        out["searches"][name] = {
            "nodes": nodes, "us_per_blocking_call": round(us_call, 2), "device_us_pack": round(pack_us, 2), "device_us_search": round(search_us, 2),
            "node_points_per_s": nodes * n_pts / (search_us * 1e-6),
            "best": {"k": k, "flat": flat, "score": score, "node_pose": [float(v) for v in node],
                     "node_error_m": math.hypot(float(node[0] - truth[0]), float(node[1] - truth[1])),
                     "node_error_deg": math.degrees(abs(math.remainder(float(node[2]) - float(truth[2]), 2 * math.pi)))}}
    lat = (2, centre, 64, 64, 180, np.float32(math.radians(2.0)))
    pose, rpt, info = m.Relocalise(rep, scan, *lat, B=16)
    out["relocalise_B16"] = {
        "us_per_call": round(timed(ctx, lambda: m.Relocalise(rep, scan, *lat, B=16), reps=10), 2),
        "pose": [float(v) for v in pose], "truth": [float(v) for v in truth], "residual": float(rpt["residual"]),
        "error_m": math.hypot(float(pose[0] - truth[0]), float(pose[1] - truth[1])),
        "error_deg": math.degrees(abs(math.remainder(float(pose[2]) - float(truth[2]), 2 * math.pi))),
        "info": {n: int(info[n]) for n in info.dtype.names}}
    best = {}
    for half_xy, half_th in ((0.4, 10.0), (0.8, 20.0), (1.2, 40.0)):
        hints = hs.hint_lattice(centre, half_xy, 0.2, math.radians(half_th), math.radians(5.0))
        us = timed(ctx, lambda: m.MatchDataBest(rep, scan, hints), warm=2, reps=5)
        p, idx, r = m.MatchDataBest(rep, scan, hints)
        best[str(len(hints))] = {"us_per_call": round(us, 2), "matches_per_s": len(hints) / (us * 1e-6),
                                 "error_m": math.hypot(float(p[0] - truth[0]), float(p[1] - truth[1])), "residual": float(r["residual"])}
    out["match_best_over_hint_lattice"] = best
    rate = max(v["matches_per_s"] for v in best.values())
    out["matches_in_the_time_of_one_relocalise"] = rate * out["relocalise_B16"]["us_per_call"] * 1e-6
    out["yardstick"] = {"nodes": out["searches"]["level2_129x129x180"]["nodes"], "batched_matcher_matches_per_s": 2.0e7,
                        "ms_to_score_the_nodes_by_matching": out["searches"]["level2_129x129x180"]["nodes"] / 2.0e7 * 1e3}
    rep.close(); ctx.close()
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
