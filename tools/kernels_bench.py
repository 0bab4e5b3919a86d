"""Secondary-kernel timings (K2 HoleMap update, K3 ObstacleMap update, K4 Hector match, K5 Hector grid update,
fused search+update) on one MI355X, with the algorithmic byte counts of SURVEY.md sec.8d, and the Hector matcher in the
reference's summation order (ScanMatcher(T, referenceSummation=True), T = 1, 4, 16, beside the default order) and through
the reference's probability cache (T = 0 and 1, beside the default), and with the match report (slamhip_match_report) on and
off: single match, batches of 256 and 4096, HectorSLAMProcessor.Update, and match_best beside match_batch.  Prints one JSON
object.  --hector-only: the Hector part alone.  --shift-only: the scrolling window (slamhip_hs_shift) alone, beside a plain
device-to-device copy of the same arrays and beside the host route (download, np.roll, upload); with --backing: the shift with the backing store off, on over fresh ground
and on over ground to restore, beside a device-to-device copy of the evicted plus restored bytes.  (SLAMHIP_LIB names another build of the library for an A/B on one box; rows that
need entry points it lacks are left out.)  --world-only: loading a saved world back (slamhip_hs_world_cells_upload, slamhip_hs_world_extends) for a full level 0 of 2048 x 2048, the
window part and the tile part separately, beside a plain hipMemcpy of the same bytes."""
import ctypes as C, json, math, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import slam.net_amd.capi as capi, slam.net_amd.coreslam as cs, slam.net_amd.hector as hs, slam.net_amd.sim as sim

out = {}
ctx = cs.Context(0)
segs = sim.default_field()


def shift_rows(side, levels, cell):
    """slamhip_hs_shift on a side^2 x levels pyramid: device time per shift between two events on the operator's stream (the
    call is enqueue-only), for (g, 0), (0, g) and (side / 4, side / 4) taken down to a multiple of g.  The yardstick is not the
    code under test: hipMemcpyAsync device-to-device of the same levels' cells (8 B) and probabilities (4 B) into buffers of
    the same size, timed the same way in the same run.  And what a host had to do without the call: cells_download, np.roll,
    cells_upload per level (wall time)."""
    hip = C.CDLL("libamdhip64.so")
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]

    def ok(rc):
        if rc != 0: raise RuntimeError("HIP error %d" % rc)
    stream = C.c_void_p(ctx.stream)
    e0, e1 = C.c_void_p(), C.c_void_p()
    ok(hip.hipEventCreate(C.byref(e0))); ok(hip.hipEventCreate(C.byref(e1)))

    def device_us(fn, calls, batches=5):
        for _ in range(10): fn()                                           # warm up (the first shift also allocates)
        ctx.synchronize()
        ts = []
        for _ in range(batches):
            ok(hip.hipEventRecord(e0, stream))
            for _ in range(calls): fn()
            ok(hip.hipEventRecord(e1, stream)); ok(hip.hipEventSynchronize(e1))
            ms = C.c_float(); ok(hip.hipEventElapsedTime(C.byref(ms), e0, e1))
            ts.append(ms.value / calls * 1e3)
        return sorted(ts)[batches // 2]

    rep = hs.MapRepMultiMap(cell, (side, side), levels, ctx=ctx)
    g = 1 << (levels - 1)
    s_ = cell * side / 40.0                                                # (the 40 m field shrunk to the window: something to move)
    rng = sim.PCG32(3)
    for it in range(4):
        p = np.array([20 + 0.05 * it, 20 + 0.02 * it, 0.01 * it], np.float32)
        rep.UpdateByScan(hs.ScanCloud((sim.make_scan(segs, p, 1080, rng)[1] * np.float32(s_)).astype(np.float32)), (p * np.array([s_, s_, 1], np.float32)))
    cells = sum((side >> l) * (side >> l) for l in range(levels))
    row = {"cells": cells, "bytes_moved_once": 12 * cells}
    q = (side // 4) // g * g
    for name, (dx, dy) in (("shift_g_0", (g, 0)), ("shift_0_g", (0, g)), ("shift_quarter", (q, q))):
        sign = [1]

        def fn():                                                          # (there and back: the origin stays near 0)
            rep.shift(sign[0] * dx, sign[0] * dy); sign[0] = -sign[0]
        row[name + "_us"] = device_us(fn, 50)
    bufs = []
    for l in range(levels):
        n = (side >> l) * (side >> l)
        for b in (8 * n, 4 * n):
            a, d = C.c_void_p(), C.c_void_p()
            ok(hip.hipMalloc(C.byref(a), b)); ok(hip.hipMalloc(C.byref(d), b))
            bufs.append((a, d, b))

    def copy_all():
        for a, d, b in bufs: ok(hip.hipMemcpyAsync(d, a, b, 3, stream))    # hipMemcpyDeviceToDevice
    row["memcpy_d2d_us"] = device_us(copy_all, 50)
    for a, d, b in bufs: hip.hipFree(a); hip.hipFree(d)

    def host_route():
        for l, m in enumerate(rep.Maps):
            w, h = m.Dimensions
            c = m.GetCells().reshape(h, w)
            m.SetCells(np.roll(c, (-(g >> l), 0), axis=(1, 0)).ravel())
    host_route()
    t0 = time.perf_counter()
    for _ in range(3): host_route()
    row["host_download_roll_upload_us"] = (time.perf_counter() - t0) / 3 * 1e6
    worst = max(row[k] for k in ("shift_g_0_us", "shift_0_g_us", "shift_quarter_us"))
    row["worst_shift_over_memcpy"] = worst / row["memcpy_d2d_us"]
    rep.close()
    return row


def backing_rows(side, levels, cell, tile=64):
    """slamhip_hs_shift with the backing store (slamhip_hs_set_backing): device time per shift between two events, as in shift_rows,
    for (g, 0), (0, g) and a quarter window -- backing off (there and back, shift_rows' own figure); backing on while the window
    moves one way over fresh ground (a band to evict, nothing to restore); and on the way back over the same ground (a band to
    evict, the full band restored).  The yardstick for the added time is not the code under test: ONE hipMemcpyAsync
    device-to-device of as many bytes as the shift evicted plus restored (12 per cell, from slamhip_hs_backing_stats), a
    launch boundary of its own included, timed the same way in the same run."""
    hip = C.CDLL("libamdhip64.so")
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]

    def ok(rc):
        if rc != 0: raise RuntimeError("HIP error %d" % rc)
    stream = C.c_void_p(ctx.stream)
    e0, e1 = C.c_void_p(), C.c_void_p()
    ok(hip.hipEventCreate(C.byref(e0))); ok(hip.hipEventCreate(C.byref(e1)))

    def device_us(fn, calls, batches, warm):
        for _ in range(warm): fn()
        ctx.synchronize()
        ts = []
        for _ in range(batches):
            ok(hip.hipEventRecord(e0, stream))
            for _ in range(calls): fn()
            ok(hip.hipEventRecord(e1, stream)); ok(hip.hipEventSynchronize(e1))
            ms = C.c_float(); ok(hip.hipEventElapsedTime(C.byref(ms), e0, e1))
            ts.append(ms.value / calls * 1e3)
        return sorted(ts)[batches // 2], (max(ts) - min(ts))

    g = 1 << (levels - 1)
    s_ = cell * side / 40.0
    q = (side // 4) // g * g
    row = {"tile": tile}
    for name, (dx, dy), calls in (("g_0", (g, 0), 40), ("0_g", (0, g), 40), ("quarter", (q, q), 8)):
        rep = hs.MapRepMultiMap(cell, (side, side), levels, ctx=ctx)
        rng = sim.PCG32(3)
        for it in range(4):
            p = np.array([20 + 0.05 * it, 20 + 0.02 * it, 0.01 * it], np.float32)
            rep.UpdateByScan(hs.ScanCloud((sim.make_scan(segs, p, 1080, rng)[1] * np.float32(s_)).astype(np.float32)), (p * np.array([s_, s_, 1], np.float32)))
        sign = [1]

        def there_and_back():
            rep.shift(sign[0] * dx, sign[0] * dy); sign[0] = -sign[0]
        r = {}
        r["off_us"], r["off_spread_us"] = device_us(there_and_back, 50, 5, 10)
        rep.set_backing(tile, 3 << 30)
        batches, warm = 3, 4
        n = warm + batches * calls
        st0 = rep.backing_stats()
        r["on_fresh_us"], r["on_fresh_spread_us"] = device_us(lambda: rep.shift(dx, dy), calls, batches, warm)
        st1 = rep.backing_stats()
        r["on_return_us"], r["on_return_spread_us"] = device_us(lambda: rep.shift(-dx, -dy), calls, batches, warm)
        st2 = rep.backing_stats()
        for key, a, b in (("fresh", st0, st1), ("return", st1, st2)):
            cells = (b["evicted_cells"] - a["evicted_cells"] + b["restored_cells"] - a["restored_cells"]) / n
            r[key + "_evicted_cells_per_shift"] = (b["evicted_cells"] - a["evicted_cells"]) / n
            r[key + "_restored_cells_per_shift"] = (b["restored_cells"] - a["restored_cells"]) / n
            nbytes = max(16, int(12 * cells))
            src, dst = C.c_void_p(), C.c_void_p()
            ok(hip.hipMalloc(C.byref(src), nbytes)); ok(hip.hipMalloc(C.byref(dst), nbytes))
            r[key + "_bytes_per_shift"] = nbytes
            r[key + "_memcpy_same_bytes_us"] = device_us(lambda: ok(hip.hipMemcpyAsync(dst, src, nbytes, 3, stream)), 50, 5, 10)[0]
            r[key + "_added_us"] = r["on_%s_us" % key] - r["off_us"]
            hip.hipFree(src); hip.hipFree(dst)
        r["dropped_cells"] = st2["dropped_cells"]; r["pool_bytes"] = st2["bytes"]; r["tiles"] = st2["tiles"]
        row[name] = r
        rep.close()
    return row


def world_rows(side, levels, cell, tile=64):
    """slamhip_hs_world_cells_upload and slamhip_hs_world_extends for one full level 0 (side^2 cells, 8 B each): wall time of the
    blocking calls, median of 5 after a first call that allocates -- the rectangle that is exactly the window (backing off), and
    the same rectangle a window's width away (backing on: tiles only; the first call, which takes the slots, is reported apart).
    The yardstick is not the code under test: a blocking hipMemcpy host-to-device of the same array into a device buffer (what
    the staging alone costs), and a device-to-device hipMemcpy of the same bytes (what reading them once costs), timed the same
    way in the same run."""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipDeviceSynchronize.argtypes = []

    def ok(rc):
        if rc != 0: raise RuntimeError("HIP error %d" % rc)

    def wall(fn, n=5):
        fn(); ctx.synchronize()
        ts = []
        for _ in range(n):
            t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
        return sorted(ts)[n // 2] * 1e6

    rng = np.random.default_rng(5)
    cells = np.zeros((side, side), capi.CELL_DTYPE)
    cells["value"] = rng.standard_normal((side, side)).astype(np.float32)
    cells["update_index"] = rng.integers(0, 40, (side, side))
    cells["value"][rng.random((side, side)) < 0.5] = 0.0                   # (half of the world never seen)
    cells["update_index"][cells["value"] == 0] = -1
    nbytes = cells.nbytes
    row = {"cells": side * side, "bytes": nbytes, "tile": tile}
    rep = hs.MapRepMultiMap(cell, (side, side), levels, ctx=ctx)
    row["window_upload_us"] = wall(lambda: rep.world_put(0, 0, 0, cells))
    row["window_extends_us"] = wall(lambda: rep.world_extends(0))
    row["window_cells_upload_us"] = wall(lambda: rep.Maps[0].SetCells(cells.ravel()))        # (slamhip_hs_cells_upload: the window-only call)
    rep.set_backing(tile, 3 << 30)
    t0 = time.perf_counter(); dropped = rep.world_put(0, 2 * side, 0, cells); row["tiles_first_upload_us"] = (time.perf_counter() - t0) * 1e6
    row["tiles_upload_us"] = wall(lambda: rep.world_put(0, 2 * side, 0, cells))
    row["window_and_tiles_extends_us"] = wall(lambda: rep.world_extends(0))
    st = rep.backing_stats()
    row["tiles"] = st["tiles"]; row["pool_bytes"] = st["bytes"]; row["dropped_cells"] = dropped
    assert rep.world_extends(0) is not None
    d, d2 = C.c_void_p(), C.c_void_p()
    ok(hip.hipMalloc(C.byref(d), nbytes)); ok(hip.hipMalloc(C.byref(d2), nbytes))
    src = cells.ctypes.data_as(C.c_void_p)
    row["memcpy_h2d_same_bytes_us"] = wall(lambda: ok(hip.hipMemcpy(d, src, nbytes, 1)))     # hipMemcpyHostToDevice, pageable as the caller's array is

    def d2d():
        ok(hip.hipMemcpy(d2, d, nbytes, 3)); ok(hip.hipDeviceSynchronize())
    row["memcpy_d2d_same_bytes_us"] = wall(d2d)
    hip.hipFree(d); hip.hipFree(d2)
    row["window_upload_over_h2d"] = row["window_upload_us"] / row["memcpy_h2d_same_bytes_us"]
    row["tiles_upload_over_h2d"] = row["tiles_upload_us"] / row["memcpy_h2d_same_bytes_us"]
    rep.close()
    return row


if "--world-only" in sys.argv:
    print(json.dumps({"hs_world_3lvl_2048": world_rows(2048, 3, 40.0 / 2048)}, indent=1))
    ctx.close()
    sys.exit(0)


def shift_section():
    if "--backing" in sys.argv:
        return {"hs_backing_3lvl_2048": backing_rows(2048, 3, 40.0 / 2048), "hs_backing_4lvl_400": backing_rows(400, 4, 0.1)}

    return {"hs_shift_3lvl_2048": shift_rows(2048, 3, 40.0 / 2048), "hs_shift_4lvl_400": shift_rows(400, 4, 0.1)}


if "--shift-only" in sys.argv:
    print(json.dumps(shift_section(), indent=1))
    ctx.close()
    sys.exit(0)

for size in (() if "--hector-only" in sys.argv else (1024, 2048, 4096)):
    dev = cs.CoreSlamDevice(ctx, 40.0, size, size // 4)
    rng = sim.PCG32(1234); traj = sim.trajectory(40)
    scans = [sim.make_scan(segs, p, 1080, rng)[1] for p in traj]
    for i in range(8):
        dev.set_scan(scans[i]); dev.update_holemap(traj[i]); dev.update_obstaclemap(traj[i])
    # (per-launch event pairs; three passes over the same 32 scans, the median pass is reported: a single slow launch -- the
    # box is shared with nothing, but clocks and the host's scheduler wander -- moves a 32-launch mean by a third)
    passes = []
    for rep_ in range(3):
        ctx.timing_reset(); ctx.timing_enable(-1)
        px = 0
        for i in range(8, 40):
            dev.set_scan(scans[i]); dev.update_holemap(traj[i]); px += dev.last_holemap_pixels; dev.update_obstaclemap(traj[i])
        ms2, n2 = ctx.timing_get(capi.K_CS_HOLEMAP); ms3, n3 = ctx.timing_get(capi.K_CS_OBSTACLE)
        ctx.timing_enable(0)
        passes.append((ms2 / n2, ms3 / n3, px / n2))
    ms2n = sorted(q[0] for q in passes)[1]; ms3n = sorted(q[1] for q in passes)[1]; pxn = passes[0][2]
    out["k2_holemap_%d" % size] = {"us_per_update": ms2n * 1e3, "blended_px_per_update": pxn,
                                    "algorithmic_GBps": 4 * pxn / (ms2n * 1e-3) / 1e9, "rays_per_s": 1080 / (ms2n * 1e-3), "passes": 3}
    out["k3_obstacle_%d" % (size // 4)] = {"us_per_update": ms3n * 1e3, "passes": 3}
    if size == 2048:      # fused config C3: search (16384 candidates) + both map updates in one call
        dev.set_offsets(sim.gaussian_offsets(16383))
        base = traj[-1]
        dev.set_scan(scans[-1])
        for _ in range(30): dev.search_and_update(base)
        dts = []
        for rep_ in range(5):
            ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(200): dev.search_and_update(base)
            ctx.synchronize()        # (the call returns with the pose; the last call's map updates belong to the figure)
            dts.append((time.perf_counter() - t0) / 200)
        dt = sorted(dts)[2]
        out["c3_fused_search_update_2048"] = {"us_per_scan": dt * 1e6, "scans_per_s": 1 / dt, "batches_of_200": 5}
    dev.close()

# Hector: 3-level 2048^2 pyramid, 1080 rays (config C4)
rep = hs.MapRepMultiMap(40.0 / 2048, (2048, 2048), 3, ctx=ctx)
rng = sim.PCG32(3)
scans = []
for it in range(20):
    p = np.array([20 + 0.05 * it, 20 + 0.02 * it, 0.01 * it], np.float32)
    xy = sim.make_scan(segs, p, 1080, rng)[1]; scans.append((xy, p))
for xy, p in scans[:10]: rep.UpdateByScan(hs.ScanCloud(xy), p)
p5 = []
for rep_ in range(3):
    ctx.timing_reset(); ctx.timing_enable(-1)
    for xy, p in scans[10:]: rep.UpdateByScan(hs.ScanCloud(xy), p)
    ms5, n5 = ctx.timing_get(capi.K_HS_UPDATE)
    p5.append(ms5 / n5)
ms5, n5 = sorted(p5)[1], 1
m = hs.ScanMatcher(4)
xy, p = scans[-1]; scan = hs.ScanCloud(xy); hint = p + np.array([0.1, -0.08, 0.03], np.float32)
for _ in range(3): m.MatchData(rep, scan, hint)
ctx.timing_reset()
for _ in range(50): m.MatchData(rep, scan, hint)
ms4, n4 = ctx.timing_get(capi.K_HS_MATCH)
t0 = time.perf_counter()
for _ in range(50): m.MatchData(rep, scan, hint)
wall1 = (time.perf_counter() - t0) / 50
B = 4096
hints = np.tile(hint, (B, 1)) + np.random.default_rng(0).normal(0, 0.05, (B, 3)).astype(np.float32) * np.array([1, 1, 0.2], np.float32)
m.MatchDataBatch(rep, scan, hints); ctx.timing_reset()
for _ in range(5): m.MatchDataBatch(rep, scan, hints)
ms4b, n4b = ctx.timing_get(capi.K_HS_MATCH)
ctx.timing_enable(0)
pt_iters = 1080 * 9
out["k5_hector_update_3lvl_2048"] = {"us_per_update": ms5 / n5 * 1e3}
out["k4_hector_match_3lvl_2048"] = {"kernel_us_single": ms4 / n4 * 1e3, "blocking_call_us_single": wall1 * 1e6,
                                    "batch": B, "kernel_us_batch": ms4b / n4b * 1e3, "matches_per_s_batched": B / (ms4b / n4b * 1e-3),
                                    "point_iterations_per_s_batched": B * pt_iters / (ms4b / n4b * 1e-3),
                                    "algorithmic_GBps_batched": B * pt_iters * 24 / (ms4b / n4b * 1e-3) / 1e9}

# the reference's summation order (slamhip_hs_set_match_threads): single match, a 64-hint batch and HectorSLAMProcessor.Update
# (2048^2 x 3 levels, 1080 rays, 30 matched scans after 10 mapped ones), each beside the default order (T = 0)
hints64 = hints[:64].copy()


def match_rows(T, refcache=False):
    m = hs.ScanMatcher(max(T, 1), referenceSummation=T > 0)
    rep.set_reference_cache(1 if refcache else 0)
    ctx.timing_enable(-1)
    for _ in range(3): m.MatchData(rep, scan, hint)
    ctx.timing_reset()
    for _ in range(50): m.MatchData(rep, scan, hint)
    ms1, n1 = ctx.timing_get(capi.K_HS_MATCH)
    m.MatchDataBatch(rep, scan, hints64); ctx.timing_reset()
    for _ in range(20): m.MatchDataBatch(rep, scan, hints64)
    ms64, n64 = ctx.timing_get(capi.K_HS_MATCH)
    ctx.timing_enable(0)
    proc = hs.HectorSLAMProcessor(40.0 / 2048, (2048, 2048), scans[0][1], 3, max(T, 1), ctx=ctx, referenceSummation=T > 0,
                                  referenceCache=refcache)
    rng = sim.PCG32(77)
    pscans = [hs.ScanCloud(sim.make_scan(segs, np.array([20 + 0.03 * i, 20 + 0.01 * i, 0.004 * i], np.float32), 1080, rng)[1])
              for i in range(40)]
    for i in range(10): proc.Update(pscans[i], proc.MatchPose, True)
    ctx.synchronize()
    t0 = time.perf_counter()
    for i in range(10, 40): proc.Update(pscans[i], proc.MatchPose, False)
    ctx.synchronize()
    upd = (time.perf_counter() - t0) / 30
    proc.Dispose()
    rep.set_reference_cache(0)
    return {"kernel_us_single": ms1 / n1 * 1e3, "kernel_us_batch64": ms64 / n64 * 1e3, "processor_update_us": upd * 1e6}


out["k4_hector_match_refsum_3lvl_2048"] = {"T%d" % T: match_rows(T) for T in (0, 1, 4, 16)}
# the reference's probability cache (slamhip_hs_set_reference_cache), the same three figures beside the default at T = 0 and
# T = 1.  (The repeated single matches and batches run on one map in one epoch: after the first, their taps hit the entries
# it filled.  In the processor's flow every update starts a new epoch, so the first iteration on every level fills.)
out["k4_hector_match_refcache_3lvl_2048"] = {"T%d_%s" % (T, "refcache" if rc else "default"): match_rows(T, rc)
                                              for T in (0, 1) for rc in (False, True)}


# the match report: blocking-call wall time (what a host sees), median of 5 batches of calls, default order and cache off
def wall_us(fn, calls, batches=5):
    fn(); ctx.synchronize()
    ts = []
    for _ in range(batches):
        t0 = time.perf_counter()
        for _ in range(calls): fn()
        ts.append((time.perf_counter() - t0) / calls)
    return sorted(ts)[batches // 2] * 1e6


def proc_update_us(report):
    kw = {"matchReport": True} if report else {}
    proc = hs.HectorSLAMProcessor(40.0 / 2048, (2048, 2048), scans[0][1], 3, 1, ctx=ctx, **kw)
    rng = sim.PCG32(77)
    pscans = [hs.ScanCloud(sim.make_scan(segs, np.array([20 + 0.03 * i, 20 + 0.01 * i, 0.004 * i], np.float32), 1080, rng)[1])
              for i in range(40)]
    for i in range(10): proc.Update(pscans[i], proc.MatchPose, True)
    ctx.synchronize()
    t0 = time.perf_counter()
    for i in range(10, 40): proc.Update(pscans[i], proc.MatchPose, False)
    ctx.synchronize()
    upd = (time.perf_counter() - t0) / 30
    proc.Dispose()
    return upd * 1e6


rep.set_match_threads(0)
have_report = hasattr(capi.lib(), "slamhip_hs_match_report")
m0 = hs.ScanMatcher(1)
rows = {"single_us": {"off": wall_us(lambda: m0.MatchData(rep, scan, hint), 200)},
        "processor_update_us": {"off": sorted(proc_update_us(False) for _ in range(3))[1]}}
if have_report:
    rows["single_us"]["on"] = wall_us(lambda: m0.MatchDataReport(rep, scan, hint), 200)
    rows["processor_update_us"]["on"] = sorted(proc_update_us(True) for _ in range(3))[1]
for Bn in (256, 4096):
    hb = hints[:Bn].copy()
    r = {"off": wall_us(lambda: m0.MatchDataBatch(rep, scan, hb), 20 if Bn == 256 else 5)}
    if have_report:
        r["on"] = wall_us(lambda: m0.MatchDataBatchReport(rep, scan, hb), 20 if Bn == 256 else 5)
        r["match_best"] = wall_us(lambda: m0.MatchDataBest(rep, scan, hb), 20 if Bn == 256 else 5)
    rows["batch%d_us" % Bn] = r
out["k4_hector_match_report_3lvl_2048"] = rows
if hasattr(capi.lib(), "slamhip_hs_shift"):
    out.update(shift_section())
print(json.dumps(out, indent=1))
