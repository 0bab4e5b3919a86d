"""K24, the branch-and-bound pose-lattice search (slamhip_hs_lattice_search_bnb): the median wall clock per blocking call, in the
pyramid and with the scan of tools/hs_lattice_bench.py (2048^2 x 3 from the simulator, 1080 rays).
 (1) K7's configuration -- 129 x 129 x 180 on the 512^2 level, window and world -- beside slamhip_hs_lattice_search /
     slamhip_hs_world_lattice_search in the same process, for top in {3, 4, 5, 6}: time, evaluated / nodes, and that the keys agree.
 (2) Level 0 (2048^2), nx = ny = 1024, 360 headings (1.5e9 nodes: K7 refuses), per top: time, evaluated / nodes, blocks and kept
     per height.
 (3) What the change leaves alone, for the comparison with the parent commit: the K7 calls' wall clock (in (1)) and
     HectorSLAMProcessor.Update, us per call.  With `--parent-lib PATH` the same two from a build of the parent commit, in a child
     process of the same session (SLAMHIP_LIB).
`python tools/hs_bnb_bench.py [out.json]`; writes profiles/r30_hs_bnb.json by default.  `--unchanged-only` prints (3) alone."""
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np

import slam.net_amd.hector as hs
import slam.net_amd.sim as sim
import hs_lattice_bench as LB


def median_us(ctx, fn, warm=2, reps=9):
    for _ in range(warm):
        fn()
    rows = []
    for _ in range(reps):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()                                                               # (blocking: it returns with its results)
        rows.append((time.perf_counter() - t0) * 1e6)
    return round(float(np.median(rows)), 2)


def info_row(info, nodes):
    top = int(info["top"])
    return {"evaluated": int(info["evaluated"]), "evaluated_over_nodes": int(info["evaluated"]) / nodes,
            "blocks": [int(v) for v in info["blocks"][:top + 1]], "kept": [int(v) for v in info["kept"][:top + 1]]}


def unchanged_figures():
    """The K7 window search of (1) and the processor's Update: what K24 must leave as the parent commit has it."""
    ctx, rep, scan, truth, centre = LB.build_map(backing=False)
    lat = (2, centre, 64, 64, 180, np.float32(math.radians(2.0)))
    out = {"k7_window_us_per_call": median_us(ctx, lambda: rep.lattice_search(None, *lat))}
    rep.close()
    segs = sim.default_field(); rng = sim.PCG32(1234); traj = sim.trajectory(60)
    proc = hs.HectorSLAMProcessor(LB.CELL, (LB.SIZE, LB.SIZE), traj[0], LB.LEVELS, ctx=ctx)
    scans = [hs.ScanCloud(sim.make_scan(segs, p, LB.RAYS, rng)[1]) for p in traj]
    for s, p in zip(scans[:10], traj[:10]):
        proc.Update(s, p)
    ctx.synchronize()
    t0 = time.perf_counter()
    for s, p in zip(scans[10:], traj[10:]):
        proc.Update(s, p)
    ctx.synchronize()
    out["hsproc_update_us_per_call"] = round((time.perf_counter() - t0) / (len(traj) - 10) * 1e6, 2)
    proc.Dispose(); ctx.close()
    return out


def main():
    argv = sys.argv[1:]
    parent_lib = None
    if "--parent-lib" in argv:
        i = argv.index("--parent-lib")
        parent_lib = os.path.abspath(argv[i + 1])
        del argv[i:i + 2]
    if "--unchanged-only" in argv:
        print(json.dumps(unchanged_figures()))
        return
    out_path = argv[0] if argv else os.path.join(ROOT, "profiles", "r30_hs_bnb.json")
    out = {"map": LB.SIZE, "levels": LB.LEVELS, "points": LB.RAYS, "timing": "median wall clock per blocking call, us"}
    # (1) K7's configuration, window and world
    ctx, rep, scan, truth, centre = LB.build_map(backing=True)
    lat = (2, centre, 64, 64, 180, np.float32(math.radians(2.0)))
    nodes = 180 * 129 * 129
    one = {"nodes": nodes}
    for world, name, k7 in ((False, "window", rep.lattice_search), (True, "world", rep.world_lattice_search)):
        want, _ = k7(None, *lat)
        row = {"k7_us_per_call": median_us(ctx, lambda: k7(None, *lat)), "bnb": {}}
        for top in (3, 4, 5, 6):
            keys, info = rep.lattice_search_bnb(None, *lat, top, world=world)
            r = info_row(info, nodes)
            r["us_per_call"] = median_us(ctx, lambda: rep.lattice_search_bnb(None, *lat, top, world=world))
            r["keys_equal_k7"] = bool(np.array_equal(keys, want))
            row["bnb"][str(top)] = r
        one[name] = row
    out["k7_configuration_level2_129x129x180"] = one
    # (2) level 0, the whole window, the full circle
    nx = ny = 1024; n_theta = 360
    c0 = np.array([LB.SIZE * LB.CELL / 2, LB.SIZE * LB.CELL / 2, 0.0], np.float32)
    lat0 = (0, c0, nx, ny, n_theta, np.float32(math.radians(1.0)))
    nodes0 = (2 * nx + 1) * (2 * ny + 1) * n_theta
    two = {"nodes": nodes0, "bnb": {}}
    for top in (5, 6, 7, 8):
        try:
            keys, info = rep.lattice_search_bnb(None, *lat0, top)
        except hs.capi.SlamhipError as e:                                  # rule 5 at the default capacity
            two["bnb"][str(top)] = {"refused": str(e)}
            continue
        r = info_row(info, nodes0)
        r["us_per_call"] = median_us(ctx, lambda: rep.lattice_search_bnb(None, *lat0, top), warm=1, reps=5)
        k = int(np.argmax(keys))
        score, flat = hs.decode_lattice_key(keys[k])
        f32 = np.float32                                                   # (slamhip_hs_lattice_node_pose keeps K7's 2^26-node rule: the definition's node pose, by hand)
        cell = f32(rep.Maps[0].CellLength); stm = f32(1.0) / cell
        node = [f32(f32(f32(c0[0] * stm) + f32(flat % (2 * nx + 1) - nx)) * cell), f32(f32(f32(c0[1] * stm) + f32(flat // (2 * nx + 1) - ny)) * cell)]
        r["best"] = {"k": k, "score": score, "node_error_m": math.hypot(float(node[0] - truth[0]), float(node[1] - truth[1]))}
        two["bnb"][str(top)] = r
    out["level0_2049x2049x360"] = two
    rep.close(); ctx.close()                                               # (one process on the device at a time)
    # (3) what stays as it was
    out["unchanged"] = unchanged_figures()
    if parent_lib:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--unchanged-only"], env=dict(os.environ, SLAMHIP_LIB=parent_lib),
                           stdout=subprocess.PIPE, check=True, timeout=300)
        out["unchanged_parent"] = json.loads(r.stdout.decode().strip().splitlines()[-1])
    else:
        out["unchanged_parent"] = "not measured (no --parent-lib)"
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
