"""What the search report costs per scan: slamhip_csproc_update in a native-caller-style loop (ctypes straight onto the C-ABI,
arrays and pointers made once; the interpreter's part of a call is ~1 us), reports off and on, at the README's headline
configuration -- 2048^2 map, 1080 rays, 16 384 candidates.

Off and on alternate in blocks inside ONE process after a warm-up (sustained clocks), so that a slow drift of the clocks hits
both alike; every block's mean is kept, and the figure is the median over blocks with the blocks' spread beside it.  The
report-off figure is the baseline; run the same script against a build of the parent commit (SLAMHIP_LIB=..., --off-only) to
confirm that it did not move.

    python tools/search_report_cost.py [--blocks 8] [--scans 300] [--json profiles/r08_search_report.json]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/search_report_cost.py --profile-run     (kernel durations, a run of its own)
"""
import argparse
import ctypes as C
import json
import math
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def clocks_state():
    """Read-only: what rocm-smi says about the clocks (no setting is changed)."""
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "--showperflevel", "-d", "0"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=20)
        keep = [l.strip() for l in r.stdout.decode(errors="replace").splitlines() if "sclk" in l or "mclk" in l or "Performance Level" in l]
        return keep[:6]
    except Exception as e:                                          # noqa: BLE001
        return ["unavailable: %r" % (e,)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--rays", type=int, default=1080)
    ap.add_argument("--cands", type=int, default=16384)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--scans", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=1500)
    ap.add_argument("--band", type=int, default=64)
    ap.add_argument("--off-only", action="store_true", help="an older build of the library: report-off blocks only")
    ap.add_argument("--profile-run", action="store_true", help="a short report-on run for rocprofv3 --kernel-trace --stats")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    import slam.net_amd.capi as capi
    import slam.net_amd.coreslam as cs
    import slam.net_amd.sim as sim
    L = capi.lib()
    ctx = cs.Context(0)
    segs = sim.default_field()
    traj = sim.trajectory(80)
    rng = sim.PCG32(5)
    scans = [np.ascontiguousarray(sim.make_scan(segs, p, a.rays, rng)[0], np.float32) for p in traj]
    nj = a.cands - 1
    threads = 64 if nj % 64 == 0 else 1
    proc = cs.CoreSLAMProcessor(40.0, a.size, a.size // 4, traj[0], 0.1, math.radians(10.0), nj // threads, threads, ctx=ctx)
    seg_pose = np.zeros((1, 3), np.float32)
    start = np.array([0, a.rays], np.int32)
    args = [(proc._h, capi.fptr(seg_pose), capi.iptr(start), 1, capi.fptr(s)) for s in scans]
    update = L.slamhip_csproc_update

    def run(n, first=0):
        t0 = time.perf_counter()
        for i in range(n):
            rc = update(*args[10 + (first + i) % 60])
            if rc != 0:
                raise RuntimeError(L.slamhip_last_error().decode())
        return (time.perf_counter() - t0) / n * 1e6

    for i in range(10):
        capi.check(update(*args[i]))
    if a.profile_run:
        proc.SetSearchReport(True, a.band)
        run(200)
        ctx.synchronize()
        proc.Dispose(); ctx.close()
        return
    run(a.warmup)
    off, on = [], []
    for b in range(a.blocks):
        if not a.off_only:
            proc.SetSearchReport(False)
        run(30)
        off.append(run(a.scans))
        if not a.off_only:
            proc.SetSearchReport(True, a.band)
            run(30)
            on.append(run(a.scans))
            assert proc.LastSearchReport is not None
    ctx.synchronize()
    out = {"config": {"map": a.size, "rays": a.rays, "candidates": a.cands, "band": a.band, "scans_per_block": a.scans, "blocks": a.blocks,
                      "warmup_scans": a.warmup, "caller": "ctypes loop over slamhip_csproc_update (native-caller style)"},
           "report_off_us_per_scan": {"median": float(np.median(off)), "min": float(min(off)), "max": float(max(off)), "blocks": [round(x, 2) for x in off]},
           "prelaunch_stats": list(proc.device.prelaunch_stats), "clocks": clocks_state()}
    if on:
        out["report_on_us_per_scan"] = {"median": float(np.median(on)), "min": float(min(on)), "max": float(max(on)), "blocks": [round(x, 2) for x in on]}
    proc.Dispose(); ctx.close()
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
