"""K25: the render of N stored scans into the whole world behind a scrolling window (slamhip_hs_render_world) beside K20's render of the
same scans into one pyramid large enough to hold them (slamhip_hs_render: the same work without tiles) and beside what a caller
had before -- a loop of N blocking set_scan + update_by_scan calls with the window shifted to follow the robot -> one JSON line per N.

  python tools/hs_render_world_bench.py [--n 64,1024,10000] [--reps 15] [--warmup 3] [--rays 1080] [--tile 32]
                                        [--out profiles/r31_hs_render_world.json]

World: 2048 x 2048 x 3 levels of 0.02 m, the simulator's lap; the window 512 x 512 x 3 at the world's origin, which holds a corner of the field: most lines end in tiles.  The
scans are 64 distinct simulated scans of `rays` points used in turn (hs_render_bench.py).  Wall clock per blocking call, median of
`reps` after `warmup`.  At N = 64 every scan is drawn at the pose it was cast from and every line lies inside [0, 2048)^2: the world
render's download of that square must equal K20's pyramid on level 0 or the run fails.  Beyond 64 a scan is drawn at poses it was not
cast from and some lines leave the square: K20 drops them, the world render draws them into further tiles ("tiles" says how many
exist afterwards; 5376 cover the square on the three levels), so "level0_equal" is reported and not required there.  With
slam.net_amd/build/variants/parent.so present -- a build of the parent commit -- both renders and the processor are timed in
alternating fresh interpreters, this tree then the parent, three each (--existing-only with SLAMHIP_LIB set): slamhip_hs_render
on the lap's 2048^2 pyramid and slamhip_hs_render_world in the window, N = 64 and 1024 each, and HectorSLAMProcessor.Update per scan
(hs_dfield_bench.update_us) -> "existing_alternating"; then slamhip_hs_render alone under SLAMHIP_K20_TILE=64 (--k20-only) ->
"k20_tile_64_alternating"."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import slam.net_amd.capi as capi        # noqa: E402
import slam.net_amd.hector as hs        # noqa: E402
import slam.net_amd.sim as sim          # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hs_dfield_bench as db            # noqa: E402
import hs_render_bench as rb            # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CELL, WORLD, WIN, LEVELS = 0.02, 2048, 512, 3
ORIGIN = (0, 0)                         # the window's origin: the world's, so that both renders form the SAME matrices and == is the check
                                        # (a shifted window takes poses minus (float)origin * cell: other bits, other cells at cell borders)


def median_ms(t):
    return 1e3 * float(np.median(t))


def setup(rays):
    segs = sim.default_field()
    lap, _ = sim.lap_trajectory()
    rng = sim.PCG32(7)
    base = [sim.make_scan(segs, lap[(k * len(lap)) // 64], rays, rng)[1] for k in range(64)]
    return lap, base


def timed(a, call):
    t = []
    for it in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        call()
        if it >= a.warmup:
            t.append(time.perf_counter() - t0)
    return median_ms(t)


def existing(a):
    """slamhip_hs_render and slamhip_hs_render_world on the lap, N = 64 and 1024, and the processor's Update -> ms and us (whatever
    library SLAMHIP_LIB names; --k20-only: the first alone, for the other tile side)."""
    ctx = hs.Context(0)
    lap, base = setup(a.rays)
    out = {"lib": os.path.basename(os.environ.get("SLAMHIP_LIB", "this tree")), "k20_tile": int(os.environ.get("SLAMHIP_K20_TILE", "32"))}
    for n in (64, 1024):
        poses = rb.poses_for("lap", n, lap)
        reps = [hs.MapRepMultiMap(CELL, (WORLD, WORLD), LEVELS, ctx=ctx)]
        if not a.k20_only:
            reps.append(hs.MapRepMultiMap(CELL, (WIN, WIN), LEVELS, ctx=ctx))
            reps[1].set_backing(a.tile, 1 << 30)
        for k in range(n):
            for rep in reps:
                rep.ScansAdd(hs.ScanCloud(base[k % 64]))
        out["render_lap_%d_ms" % n] = timed(a, lambda: reps[0].Render(poses))
        if not a.k20_only:
            out["render_world_%d_ms" % n] = timed(a, lambda: reps[1].RenderWorld(poses))
        for rep in reps:
            rep.close()
    ctx.close()
    if not a.k20_only:
        out["update_us"] = db.update_us()
    return out


def rows_of(a):
    ctx = hs.Context(0)
    lap, base = setup(a.rays)
    off = np.array([ORIGIN[0] * CELL, ORIGIN[1] * CELL, 0.0], np.float32)
    rows = []
    for n in [int(v) for v in a.n.split(",")]:
        poses = rb.poses_for("lap", n, lap)
        big = hs.MapRepMultiMap(CELL, (WORLD, WORLD), LEVELS, ctx=ctx)
        win = hs.MapRepMultiMap(CELL, (WIN, WIN), LEVELS, ctx=ctx)
        follow = hs.MapRepMultiMap(CELL, (WIN, WIN), LEVELS, ctx=ctx)
        for r in (win, follow):
            r.set_backing(a.tile, 1 << 30)
            r.shift(*ORIGIN)
        for k in range(n):
            big.ScansAdd(hs.ScanCloud(base[k % 64])); win.ScansAdd(hs.ScanCloud(base[k % 64]))
        pw = (poses - off).astype(np.float32)
        org = capi.f32((0.0, 0.0))
        t_world, t_k20, t_loop = [], [], []
        for it in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            win.RenderWorld(pw)
            t1 = time.perf_counter()
            big.Render(poses)
            t2 = time.perf_counter()
            if it >= a.warmup:
                t_world.append(t1 - t0); t_k20.append(t2 - t1)
        for it in range(2 + 3):                                           # the host alternative: a wait per scan, the window shifted to follow
            follow.Reset(); follow.shift(*ORIGIN)
            ctx.synchronize()
            t0 = time.perf_counter()
            for k in range(n):
                ox, oy = follow.origin()
                cx, cy = int(poses[k, 0] / CELL) - ox, int(poses[k, 1] / CELL) - oy
                dx, dy = ((cx - WIN // 2) // 128) * 128, ((cy - WIN // 2) // 128) * 128
                if dx or dy:
                    follow.shift(dx, dy)
                    ox, oy = ox + dx, oy + dy
                p = capi.f32((poses[k, 0] - np.float32(ox) * np.float32(CELL), poses[k, 1] - np.float32(oy) * np.float32(CELL), poses[k, 2]))
                s = base[k % 64]
                capi.call("slamhip_hs_set_scan", follow._h, capi.fptr(s), s.shape[0], capi.fptr(org))
                capi.call("slamhip_hs_update_by_scan", follow._h, capi.fptr(p))
            ctx.synchronize()
            if it >= 2:
                t_loop.append(time.perf_counter() - t0)
        equal = bool(np.array_equal(win.world_cells(0, 0, 0, WORLD, WORLD).reshape(-1), big.Maps[0].GetCells()))
        row = {"n_scans": n, "rays": a.rays, "tile": a.tile, "world_ms": median_ms(t_world), "k20_2048_ms": median_ms(t_k20),
               "world_over_k20": float(np.median(t_world) / np.median(t_k20)), "follow_loop_ms": median_ms(t_loop),
               "tiles": win.backing_stats()["tiles"], "level0_equal": equal}
        print(json.dumps(row), file=sys.stderr, flush=True)
        rows.append(row)
        for r in (big, win, follow):
            r.close()
        if not equal and n <= 64:
            raise SystemExit("the world render and K20's render left different maps")
    ctx.close()
    return rows


def child(args, lib=None, tile=None):
    env = dict(os.environ)
    env.pop("SLAMHIP_LIB", None); env.pop("SLAMHIP_K20_TILE", None)
    if tile:
        env["SLAMHIP_K20_TILE"] = str(tile)
    if lib:
        env["SLAMHIP_LIB"] = lib
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=env, stdout=subprocess.PIPE, timeout=900, check=True)
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="64,1024,10000")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rays", type=int, default=1080)
    ap.add_argument("--tile", type=int, default=32)
    ap.add_argument("--out", default=None)
    ap.add_argument("--existing-only", action="store_true")
    ap.add_argument("--k20-only", action="store_true")
    a = ap.parse_args()
    if a.existing_only:
        print(json.dumps(existing(a)))
        return
    out = {"tool": "tools/hs_render_world_bench.py", "device": "one MI355X", "world": "2048 x 2048 x 3 levels, 0.02 m; window 512 x 512 x 3",
           "reps": a.reps, "warmup": a.warmup, "rows": rows_of(a)}
    for row in out["rows"]:
        print(json.dumps(row), flush=True)
    parent = os.path.join(ROOT, "slam.net_amd", "build", "variants", "parent.so")
    if os.path.exists(parent):
        common = ["--existing-only", "--reps", str(a.reps), "--warmup", str(a.warmup), "--rays", str(a.rays), "--tile", str(a.tile)]
        for key, tile, more in (("existing_alternating", None, []), ("k20_tile_64_alternating", 64, ["--k20-only"])):
            out[key] = {"this_tree": [], "parent": []}
            for _ in range(3):
                out[key]["this_tree"].append(child(common + more, None, tile))
                out[key]["parent"].append(child(common + more, parent, tile))
            print(json.dumps(out[key]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
