"""The scan signatures, the keyframe store and its two searches (slamhip_hs_sig_configure, _sig_add, _sig_add_scans, _sig_query, _sig_self,
_sig_count, _sig_download, _sig_upload, _sig_clear, the slamhip_hsproc_sig_* calls and HectorSLAMProcessor.AddKeyframe / LoopCandidates)
on the device, against the host hooks and the NumPy restatement of the definition in tests/test_hs_sig_abi.py.  Everything is compared
with == on every word, count and hit; there is no tolerance anywhere.

Shapes are the smallest at which each path can go wrong: scans below, at and above k18_sig's 256-lane pass; stores below, at and above
the 64-keyframe block, k18_query's 256-key workgroup and the first allocation of 16 blocks (1024 keyframes; 4097 grows it twice);
ranges that start and end inside a block; equal scores on both sides of a workgroup boundary; ring counts on both sides of the
kernels' 8-ring register steps (3, 8, 9, 20, 32)."""
import numpy as np
import pytest

import test_hs_sig_abi as A
from test_gpu_hector_shift import hs_mod, ctx                              # noqa: F401 (fixtures)

gpu = pytest.mark.gpu
F = np.float32
U64 = np.uint64


def new_rep(hs_mod, ctx, scale, n_ring, rc):
    rep = hs_mod.MapRepMultiMap(0.1, (64, 64), 1, ctx=ctx)
    rep.SigConfigure(scale, n_ring, rc)
    return rep


def scan_of(hs_mod, pts):
    return hs_mod.ScanCloud(np.asarray(pts, F).reshape(-1, 2), (0.25, -0.5, 0.1))     # (the scan origin plays no part)


def random_scan(seed, n, reach):
    g = np.random.Generator(np.random.Philox(seed))
    return (g.standard_normal((n, 2)) * reach).astype(F)


def info_dict(info):
    return {k: int(info[k]) for k in ("n_points", "n_ignored", "n_far", "n_set")}


def same_hits(got, want):
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (got[:4], want[:4])


# ---- 1. signatures -----------------------------------------------------------------------------------------------------------------
@gpu
def test_sig_add_sizes(hs_mod, ctx):
    capi = hs_mod.capi
    scale, n_ring, rc = 10.0, 20, 5
    rep = new_rep(hs_mod, ctx, scale, n_ring, rc)
    want_store = []
    idx, sig, info = rep.SigAdd((1.0, 2.0, 3.0))                           # no scan was ever set: the empty signature
    assert idx == 0 and not sig.any() and info_dict(info) == {"n_points": 0, "n_ignored": 0, "n_far": 0, "n_set": 0}
    want_store.append(sig.copy())
    for k, n in enumerate((0, 1, 255, 256, 257, 1080)):
        pts = random_scan(40 + n, n, 6.0)
        if n >= 255:
            pts[3] = (np.nan, 1.0); pts[200] = (1.0, np.inf); pts[17] = (1700.0, 0.0); pts[250] = (-0.0, 0.0)
        rep.set_scan(scan_of(hs_mod, pts))
        idx, sig, info = rep.SigAdd((k, 0.5, -k))
        wsig, winfo = A.np_sig(pts, scale, n_ring, rc)
        assert idx == k + 1 and np.array_equal(sig, wsig) and info_dict(info) == winfo, (n, info, winfo)
        hsig, hinfo = A.hook_sig(capi, pts, scale, n_ring, rc)
        assert np.array_equal(sig, hsig) and info_dict(info) == hinfo
        want_store.append(wsig)
    assert rep.SigCount() == 7
    sig, poses = rep.SigDownload()
    assert np.array_equal(sig, np.stack(want_store)) and np.array_equal(poses[3], np.array([2, 0.5, -2], F))
    # the query of the scan that is set finds its own keyframe and appends nothing
    hits, qsig, qinfo = rep.SigQuery(B=3)
    assert np.array_equal(qsig, want_store[-1]) and info_dict(qinfo) == A.np_sig(pts, scale, n_ring, rc)[1]
    same_hits(hits, A.np_query(capi, qsig, np.stack(want_store), 0, 7, 3))
    assert hits[0]["index"] == 6 and hits[0]["score"] == 65536 and hits[0]["shift"] == 0 and rep.SigCount() == 7
    rep.close()


@gpu
@pytest.mark.parametrize("B", [1, 2, 65])
def test_sig_add_scans(hs_mod, ctx, B):
    scale, n_ring, rc = 4.0, 9, 3
    rep = new_rep(hs_mod, ctx, scale, n_ring, rc)
    sizes = [(37 * b + 300) % 613 for b in range(B)]
    if B > 2:
        sizes[B // 2] = 0                                                  # an empty scan in the middle
        sizes[1] = 256; sizes[2] = 257
    scans = [random_scan(900 + b, n, 5.0) for b, n in enumerate(sizes)]
    rep.set_scan(scan_of(hs_mod, scans[0]))
    rep.SigAdd((9, 9, 9))
    first = rep.SigAddScans(scans, np.arange(3 * B, dtype=F).reshape(B, 3))
    assert first == 1 and rep.SigCount() == B + 1
    sig, poses = rep.SigDownload(1, B)
    want = np.stack([A.np_sig(s, scale, n_ring, rc)[0] for s in scans])
    assert np.array_equal(sig, want) and np.array_equal(poses, np.arange(3 * B, dtype=F).reshape(B, 3))
    assert np.array_equal(rep.SigDownload(0, 1)[0][0], want[0])
    hits = rep.SigSelf(1)                                                  # n_set was stored with the words
    same_hits(hits, A.np_self(hs_mod.capi, np.concatenate([want[:1], want]), 0, B + 1, 1))
    capi = hs_mod.capi
    for bad in (lambda: rep.SigAddScans([], np.zeros((0, 3), F)),):
        with pytest.raises(capi.SlamhipError) as e:
            bad()
        assert e.value.code == capi.ERR_INVALID
    rep.close()


# ---- 2. stores, queries ------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("N,n_ring", [(1, 3), (63, 8), (64, 9), (65, 3), (257, 20), (4097, 3), (300, 32)])
def test_store_and_query(hs_mod, ctx, N, n_ring):
    capi = hs_mod.capi
    scale, rc = 2.0, 4
    rep = new_rep(hs_mod, ctx, scale, n_ring, rc)
    pts = random_scan(N, 400, 0.5 * n_ring * rc / scale)
    q, _ = A.np_sig(pts, scale, n_ring, rc)
    store = A.random_store(1000 + N, N, n_ring)
    # equal scores on both sides of a workgroup boundary (keys 255 | 256 from base 0; 319 | 320 from base 64), and a rotated copy
    for i, s in ((N - 1, 31), (255, 5), (256, 63), (319, 0), (320, 17), (0, 1)):
        if 0 <= i < N:
            store[i] = A.rotl(q, 64 - s)                                   # q == rotl(key, s)
    poses = np.arange(3 * N, dtype=F).reshape(N, 3)
    half = N // 2
    rep.SigUpload(store[:half], poses[:half])                              # two uploads: the second starts inside a block
    rep.SigUpload(store[half:], poses[half:])
    assert rep.SigCount() == N
    dsig, dposes = rep.SigDownload()
    assert np.array_equal(dsig, store) and np.array_equal(dposes, poses)   # download o upload is the identity
    if N > 70:
        part, pp = rep.SigDownload(61, 9)
        assert np.array_equal(part, store[61:70]) and np.array_equal(pp, poses[61:70])
    rep.set_scan(scan_of(hs_mod, pts))
    ranges = [(0, N), (0, 0), (N, N), (N - 1, N)] + ([(70, N - 3), (70, min(321, N)), (1, 64), (63, 65), (64, 128)] if N >= 257 else []) + ([(3, 60)] if N >= 63 else [])
    for first, last in ranges:
        for B in (1, 2, 16):
            hits, qsig, _ = rep.SigQuery(B, first, last)
            assert np.array_equal(qsig, q)
            same_hits(hits, A.np_query(capi, q, store, first, last, B))
            same_hits(hits, capi.debug_sig_search(q, store, first, last, 1, B))
    if N >= 257:
        hits, _, _ = rep.SigQuery(16)
        assert hits["index"][:3].tolist() == [0, 255, 256] and hits["shift"][:3].tolist() == [1, 5, 63] and (hits["score"][:3] == 65536).all()
        hits, _, _ = rep.SigQuery(2, 70, N)
        assert hits["index"].tolist() == [255, 256]
    for bad in (dict(B=0), dict(B=17), dict(first=-1), dict(first=2, last=1), dict(last=N + 1)):
        a = dict(B=1, first=0, last=N); a.update(bad)
        with pytest.raises(capi.SlamhipError) as e:
            rep.SigQuery(a["B"], a["first"], a["last"])
        assert e.value.code == capi.ERR_INVALID, bad
    rep.close()


@gpu
@pytest.mark.parametrize("N,n_ring", [(65, 9), (257, 3), (130, 32)])
def test_self_search(hs_mod, ctx, N, n_ring):
    capi = hs_mod.capi
    rep = new_rep(hs_mod, ctx, 1.0, n_ring, 2)
    store = A.random_store(2000 + N, N, n_ring, 0.3)
    store[N - 2] = A.rotl(store[1], 9); store[N // 2] = store[N // 2 - 1]; store[64] = store[0]
    rep.SigUpload(store, np.zeros((N, 3), F))
    for gap in (1, 64, 65):
        hits = rep.SigSelf(gap)
        same_hits(hits, A.np_self(capi, store, 0, N, gap))
        same_hits(hits, capi.debug_sig_search(None, store, 0, N, gap))
    hits = rep.SigSelf(1, 3, N - 1)                                        # a range inside the blocks
    same_hits(hits, A.np_self(capi, store, 3, N - 1, 1))
    assert len(rep.SigSelf(1, 5, 5)) == 0
    hits = rep.SigSelf(1)                                                  # keyframe N - 2 == rotl(keyframe 1, 9): shift 9
    assert (hits[N - 2]["index"], hits[N - 2]["shift"], hits[N - 2]["score"]) == (1, 9, 65536) and hits[64]["index"] == 0
    for bad in ((0, 0, N), (1, -1, N), (1, 0, N + 1), (1, 4, 3)):
        with pytest.raises(capi.SlamhipError) as e:
            rep.SigSelf(*bad)
        assert e.value.code == capi.ERR_INVALID
    rep.close()


# ---- 3. the store's life -----------------------------------------------------------------------------------------------------------
@gpu
def test_reset_growth_and_state(hs_mod, ctx):
    capi = hs_mod.capi
    rep = hs_mod.MapRepMultiMap(0.1, (64, 64), 1, ctx=ctx)
    for call in (lambda: rep.SigAdd((0, 0, 0)), lambda: rep.SigQuery(1, 0, 0), lambda: rep.SigSelf(1, 0, 0), rep.SigCount,
                 lambda: rep.SigUpload(np.zeros((1, 32), U64), np.zeros((1, 3), F)), lambda: rep.SigDownload(0, 0),
                 lambda: rep.SigAddScans([np.zeros((1, 2), F)], np.zeros((1, 3), F))):
        with pytest.raises(capi.SlamhipError) as e:                        # before slamhip_hs_sig_configure
            call()
        assert e.value.code == capi.ERR_STATE
    for bad in ((0.0, 4, 1), (1.0, 33, 1), (1.0, 4, 0), (1.0, 32, 513)):
        with pytest.raises(capi.SlamhipError) as e:
            rep.SigConfigure(*bad)
        assert e.value.code == capi.ERR_INVALID
    n_ring = 5
    rep.SigConfigure(3.0, n_ring, 2)
    store = A.random_store(77, 1500, n_ring)
    poses = np.arange(4500, dtype=F).reshape(1500, 3)
    rep.SigUpload(store[:1000], poses[:1000])                              # inside the first allocation of 16 blocks
    pts = random_scan(5, 300, 2.0)
    rep.set_scan(scan_of(hs_mod, pts))
    idx, sig, _ = rep.SigAdd((7, 7, 7))
    assert idx == 1000
    rep.SigUpload(store[1000:], poses[1000:])                              # the store grows: the earlier blocks bit for bit
    whole = np.concatenate([store[:1000], sig[None], store[1000:]])
    got, gp = rep.SigDownload()
    assert np.array_equal(got, whole) and np.array_equal(gp[1001:], poses[1000:]) and np.array_equal(gp[1000], np.array([7, 7, 7], F))
    same_hits(rep.SigQuery(4)[0], A.np_query(capi, sig, whole, 0, 1501, 4))
    rep.Reset()                                                            # empties the store, keeps the spec
    assert rep.SigCount() == 0 and len(rep.SigQuery(4)[0]) == 0
    idx, sig2, _ = rep.SigAdd((1, 1, 1))
    assert idx == 0 and np.array_equal(sig2, sig)
    rep.SigConfigure(3.0, 7, 2)                                            # another ring count: the store is empty and laid out anew
    assert rep.SigCount() == 0
    rep.SigUpload(A.random_store(78, 70, 7), np.zeros((70, 3), F))
    assert np.array_equal(rep.SigDownload()[0], A.random_store(78, 70, 7))
    rep.SigClear()
    with pytest.raises(capi.SlamhipError) as e:
        rep.SigCount()
    assert e.value.code == capi.ERR_STATE
    rep.SigClear()
    rep.close()


@gpu
def test_quarter_turn(hs_mod, ctx):
    scale, n_ring, rc = 4.0, 16, 2
    rep = new_rep(hs_mod, ctx, scale, n_ring, rc)
    p = A.quarter_scan()
    t = np.stack([-p[:, 1], p[:, 0]], axis=1)
    rep.set_scan(scan_of(hs_mod, p))
    _, sp, ip = rep.SigAdd((3.0, -2.0, 0.3))
    rep.set_scan(scan_of(hs_mod, t))
    hits, st, it = rep.SigQuery(1)
    assert np.array_equal(st, A.rotl(sp, 16)) and np.array_equal(sp, A.np_sig(p, scale, n_ring, rc)[0])
    h = hits[0]
    assert (h["index"], h["score"], h["shift"]) == (0, 65536, 16) and h["inter"] == h["uni"] == h["n_set_key"] == ip["n_set"] == it["n_set"]
    rep.close()


@gpu
def test_processor_twins(hs_mod, ctx):
    capi = hs_mod.capi
    scale, n_ring, rc = 2.0, 32, 1
    sim, segs, poses, scans = A.sim_lap()
    proc = hs_mod.HectorSLAMProcessor(0.1, (256, 256), (0.0, 0.0, 0.0), 2, ctx=ctx)
    with pytest.raises(capi.SlamhipError) as e:
        proc.AddKeyframe(scan_of(hs_mod, scans[0]), poses[0])
    assert e.value.code == capi.ERR_STATE
    proc.MapRep.SigConfigure(scale, n_ring, rc)
    keys = list(range(0, len(scans), 2))
    for k, i in enumerate(keys):
        idx, sig, _ = proc.AddKeyframe(scan_of(hs_mod, scans[i]), poses[i])
        assert idx == k and np.array_equal(sig, A.np_sig(scans[i], scale, n_ring, rc)[0])
    store, kp = proc.MapRep.SigDownload()
    assert np.array_equal(kp, poses[keys])
    j = len(keys) // 3
    q_xy = A.revisit(sim, segs, poses[keys[j]], A.SIM_ALPHA, A.SIM_OFFSET)
    cands = proc.LoopCandidates(scan_of(hs_mod, q_xy), B=4, exclude_recent=2)
    want = A.np_query(capi, A.np_sig(q_xy, scale, n_ring, rc)[0], store, 0, len(keys) - 2, 4)
    same_hits(np.array([c["hit"] for c in cands], capi.SIG_HIT_DTYPE), want)
    assert cands[0]["hit"]["index"] == j and cands[0]["pose"] == capi.sig_pose_guess(poses[keys[j]], want[0]["shift"])
    # the twins against the hs calls: the same scan set by hand
    proc.MapRep.set_scan(scan_of(hs_mod, q_xy))
    same_hits(proc.MapRep.SigQuery(4, 0, len(keys) - 2)[0], want)
    same_hits(proc.SelfLoopCandidates(5), proc.MapRep.SigSelf(5))
    same_hits(proc.SelfLoopCandidates(5), A.np_self(capi, store, 0, len(keys), 5))
    proc.Dispose()
