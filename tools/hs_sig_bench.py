"""K18, scan signatures and the keyframe store (slamhip_hs_sig_add, _sig_add_scans, _sig_query, _sig_self): wall clock per blocking call
(median of 15 after 3), each figure beside a NumPy restatement on the host FROM THE SAME RUN, equal results asserted.
 * sig_add of a 1080-point scan; sig_add_scans of 4096 such scans in one launch (the store is emptied by slamhip_hs_reset between
   repetitions).  Host: the restatement below over the same points.
 * query of a scan against stores of N = 10^3, 10^5 and 2^20 keyframes with n_ring = 20 (seeded random words, the query's own
   signature planted at three places under three rotations), B = 16.  Host: rotate, AND and a byte-table popcount over the whole
   store in NumPy (one repetition at 2^20).
 * self search at N = 10^4 with min_gap = 50.  Host: the restatement for 64 of the 10^4 keyframes, spread evenly -- the whole search in
   NumPy takes minutes -- each equal to the device's record; the host figure is scaled from those 64.
 * Existing path: HectorSLAMProcessor.Update of the trace bench's scan, blocking, median of 35 scans; the new code is never entered on
   it.  `SLAMHIP_LIB=<a build of the parent commit> python tools/hs_sig_bench.py --update-only` prints the same figure for that
   build; run the two alternately.
None of the calls has a timing class: each figure is the blocking call, not the launches alone.
`python tools/hs_sig_bench.py [out.json]` writes profiles/r24_hs_sig.json by default."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import slam.net_amd.hector as hs                                           # noqa: E402
from slam.net_amd import capi                                              # noqa: E402

import hs_dfield_bench as db                                               # noqa: E402
import hs_trace_bench as tb                                                # noqa: E402

U64 = np.uint64
SCALE, RINGS, RC = 10.0, 20, 5                                             # cells of 0.1 m, 20 rings of 0.5 m
POP8 = np.array([bin(i).count("1") for i in range(256)], np.uint8)


def np_sig(xy):
    """Rules 2 - 5 of slamhip_hs_sig_add on the host -> the words."""
    f = np.asarray(xy, np.float32) * np.float32(SCALE)
    with np.errstate(invalid="ignore"):
        keep = (np.abs(f) < np.float32(16384.0)).all(axis=1)
    c = np.floor(f[keep].astype(np.float64)).astype(np.int64)
    u, v = 2 * c[:, 0] + 1, 2 * c[:, 1] + 1
    ring = np.searchsorted((2 * RC * np.arange(1, RINGS + 1, dtype=np.int64)) ** 2, u * u + v * v, side="right")
    C, S = [a.astype(np.int64) for a in capi.debug_sig_table()]
    cross = C[None, :] * v[:, None] - S[None, :] * u[:, None]
    sector = np.argmax((cross >= 0) & (np.roll(cross, -1, axis=1) < 0), axis=1)
    near = ring < RINGS
    sig = np.zeros(RINGS, U64)
    np.bitwise_or.at(sig, ring[near], U64(1) << sector[near].astype(U64))
    return sig


def popcount(words):
    return POP8[np.ascontiguousarray(words).view(np.uint8)].reshape(words.shape + (8,)).sum(axis=-1, dtype=np.int64)


def np_best(q, keys):
    """Rule 6 of one query against keys (N, n_ring) by rotate, AND and popcount on words -> (shift, inter)."""
    best = np.full(keys.shape[0], -1, np.int64); shift = np.zeros(keys.shape[0], np.int64)
    for s in range(64):
        rot = keys if s == 0 else (keys << U64(s)) | (keys >> U64(64 - s))
        inter = popcount(rot & q[None, :]).sum(axis=1)
        better = inter > best
        best[better] = inter[better]; shift[better] = s
    return shift, best


def np_query(q, store, n_set, first, last, B):
    shift, inter = np_best(q, store[first:last])
    nq = int(popcount(q).sum()); nk = n_set[first:last].astype(np.int64)
    uni = nq + nk - inter
    score = np.where(uni > 0, (inter << 16) // np.maximum(uni, 1), 0)
    idx = np.arange(first, last)
    o = np.lexsort((idx, -score))[:B]
    h = np.zeros(len(o), capi.SIG_HIT_DTYPE)
    h["score"] = score[o]; h["index"] = idx[o]; h["shift"] = shift[o]; h["inter"] = inter[o]; h["uni"] = uni[o]; h["n_set_key"] = nk[o]
    return h


def random_store(seed, N):
    g = np.random.Generator(np.random.Philox(seed))
    w = g.integers(0, 1 << 63, (N, RINGS), dtype=np.int64).view(U64)
    return w & g.integers(0, 1 << 63, (N, RINGS), dtype=np.int64).view(U64) & g.integers(0, 1 << 63, (N, RINGS), dtype=np.int64).view(U64)   # one bit in eight


def rotl(w, s):
    return w if s == 0 else (w << U64(s)) | (w >> U64(64 - s))


def host_us(fn, warm=1, reps=5):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(out))


def main():
    if "--update-only" in sys.argv:
        print(json.dumps({"update": db.update_us(), "lib": os.environ.get("SLAMHIP_LIB", "this tree")}))
        return
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r24_hs_sig.json")
    ctx = hs.Context(0)
    rep = hs.MapRepMultiMap(0.1, (64, 64), 1, ctx=ctx)
    rep.SigConfigure(SCALE, RINGS, RC)
    g = np.random.Generator(np.random.Philox(24))
    ang = np.arange(1080) * (2.0 * np.pi / 1080.0)
    rad = 2.0 + 7.0 * g.random(1080)
    xy = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1).astype(np.float32)
    out = {"spec": {"scale": SCALE, "n_ring": RINGS, "ring_cells": RC}, "query": {}}
    # ---- sig_add ----
    rep.set_scan(hs.ScanCloud(xy))
    _, q, _ = rep.SigAdd((0, 0, 0))
    assert np.array_equal(q, np_sig(xy))
    rec = tb.wall_us(ctx, lambda: rep.SigAdd((0, 0, 0)), spread=True)
    rec["numpy_us"] = round(host_us(lambda: np_sig(xy)), 2); rec["equal_to_device"] = True
    out["sig_add_1080_points"] = rec
    # ---- sig_add_scans ----
    B = 4096
    scans = [np.roll(xy, b, axis=0) * np.float32(1.0 + (b % 7) * 0.01) for b in range(B)]
    poses = np.zeros((B, 3), np.float32)

    def add_scans():
        rep.Reset()
        return rep.SigAddScans(scans, poses)
    rec = tb.wall_us(ctx, add_scans, warm=2, reps=7, spread=True)
    rec["note"] = "includes slamhip_hs_reset of a 64 x 64 map and the concatenation of the 4096 arrays on the host"
    got, _ = rep.SigDownload(0, B)
    t0 = time.perf_counter()
    want = np.stack([np_sig(s) for s in scans[:256]])
    rec["numpy_us"] = round((time.perf_counter() - t0) * 1e6 * B / 256, 2); rec["numpy_note"] = "256 of the 4096 scans, scaled"
    rec["equal_to_device"] = bool(np.array_equal(got[:256], want))
    assert rec["equal_to_device"]
    out["sig_add_scans_4096"] = rec
    # ---- query ----
    rep.set_scan(hs.ScanCloud(xy))
    for N in (1000, 100000, 1 << 20):
        store = random_store(N, N)
        for i, s in ((N // 3, 5), (N - 1, 63), (7, 0)):
            store[i] = rotl(q, 64 - s)
        n_set = popcount(store).sum(axis=1)
        rep.SigConfigure(SCALE, RINGS, RC)
        rep.SigUpload(store, np.zeros((N, 3), np.float32))
        rec = tb.wall_us(ctx, lambda: rep.SigQuery(16), spread=True)
        hits, _, _ = rep.SigQuery(16)
        reps = 1 if N > 200000 else 3
        rec["numpy_us"] = round(host_us(lambda: np_query(q, store, n_set, 0, N, 16), warm=0, reps=reps), 2)
        rec["equal_to_device"] = bool(hits.tobytes() == np_query(q, store, n_set, 0, N, 16).tobytes())
        assert rec["equal_to_device"], N
        rec["first_three"] = [[int(h["index"]), int(h["shift"]), int(h["score"])] for h in hits[:3]]
        out["query"]["N%d_B16" % N] = rec
    # ---- self search ----
    N, gap = 10000, 50
    store = random_store(77, N)
    for i in range(500, N, 997):
        store[i] = rotl(store[i - 400], i % 64)                            # revisits
    n_set = popcount(store).sum(axis=1)
    rep.SigConfigure(SCALE, RINGS, RC)
    rep.SigUpload(store, np.zeros((N, 3), np.float32))
    rec = tb.wall_us(ctx, lambda: rep.SigSelf(gap), warm=2, reps=7, spread=True)
    hits = rep.SigSelf(gap)
    sample = list(range(gap, N, (N - gap) // 63))[:64]
    t0 = time.perf_counter()
    ok = all(hits[i:i + 1].tobytes() == np_query(store[i], store, n_set, 0, i - gap + 1, 1).tobytes() for i in sample)
    rec["numpy_us"] = round((time.perf_counter() - t0) * 1e6 * N / len(sample), 2); rec["numpy_note"] = "64 of the 10^4 keyframes, scaled"
    rec["equal_to_device"] = bool(ok)
    assert ok
    rec["revisits_found"] = int(sum(int(hits[i]["index"]) == i - 400 and int(hits[i]["score"]) == 65536 for i in range(500, N, 997)))
    rec["revisits_planted"] = len(range(500, N, 997))
    out["self_N10000_gap50"] = rec
    rep.close(); ctx.close()
    out["update"] = db.update_us()
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
