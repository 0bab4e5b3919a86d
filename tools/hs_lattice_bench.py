"""K7, the pose-lattice search of HectorSLAM (slamhip_hs_lattice_search / slamhip_hs_relocalise): us per blocking call between two
device synchronisations after a warm-up, the device time of its two launches (pack, search) from the context's event timing in a
run of its own, node x points per second, the end-to-end Relocalise(B = 16), and in the same run MatchDataBest over hint lattices
of several sizes -- how many full matches the same time buys.  Workloads: a 2048^2 x 3 pyramid from the simulator, 1080 rays;
level 2 (512^2) with nx = ny = 64, n_theta = 180 (about 3.0 M nodes: the staged-rectangle path) and level 0 with a small lattice
(the global-memory path).  `python tools/hs_lattice_bench.py [out.json]`; writes profiles/r11_hs_lattice.json by default."""
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


def main():
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
