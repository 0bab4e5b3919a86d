"""The pose-graph relaxation (slamhip_hs_pg_set, _pg_relax, _pg_get, _pg_residuals, _pg_clear, slamhip_hs_sig_set_poses and
HectorSLAMProcessor.RelaxKeyframes) on the device, against the host hook slamhip_debug_pg_relax, which tests/test_hs_pg_abi.py ties to
the NumPy restatement of the definition.  Everything is compared with == on the poses, every slamhip_pg_iter field, the final chi2 and
the residuals; there is no tolerance anywhere but in the end-to-end case's "smaller".

Shapes are the smallest at which each path can go wrong: one node and no edge; two nodes; a ring of 257 (two blocks of rule 6); a chain
of 65537 with one loop edge (a second level of the tree in every workgroup; n_cg reached, and the stop word set inside a batch); a star of 1000 leaves (one lane walks 1000
edges); duplicated edges; edges in reverse order; the fixed node in the middle; two fixed nodes."""
import numpy as np
import pytest

import test_hs_pg_abi as A
from test_gpu_hector_shift import hs_mod, ctx                              # noqa: F401 (fixtures)

gpu = pytest.mark.gpu
D = np.float64
FIELDS = ("chi2", "rz0", "rz", "cg_iters", "stopped")


def new_rep(hs_mod, ctx):
    return hs_mod.MapRepMultiMap(0.1, (64, 64), 2, ctx=ctx)


def same_iters(got, want):
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (got, want)


def device_equals_hook(hs_mod, rep, poses, fixed, ij, z, w, spec):
    capi = hs_mod.capi
    hp, hit, hfin, hr, hc = capi.debug_pg_relax(poses, fixed, ij, z, w, spec)
    rep.PgSet(poses, fixed, ij, z, w)
    it, fin = rep.PgRelax(spec)
    got = rep.PgGet()
    r, c2 = rep.PgResiduals()
    assert np.array_equal(got, hp), np.abs(got - hp).max()
    same_iters(it, hit)
    assert fin == hfin and np.array_equal(r, hr) and np.array_equal(c2, hc)
    return got, it, fin


def chain(N, seed):
    """A chain of N nodes with one loop edge 0 <-> N - 1: the ring of test_hs_pg_abi cut open, formed with whole-array operations."""
    g = np.random.Generator(np.random.Philox(seed))
    R = 0.25 / (2.0 * np.sin(np.pi / N))
    phi = 2.0 * np.pi * np.arange(N) / N
    true = np.stack([R * np.cos(phi), R * np.sin(phi), phi + np.pi / 2], axis=1)
    i = np.arange(N); j = (i + 1) % N
    c, s = np.cos(true[i, 2]), np.sin(true[i, 2])
    dx, dy = true[j, 0] - true[i, 0], true[j, 1] - true[i, 1]
    z = np.stack([c * dx + s * dy, c * dy - s * dx, A.np_wrap(true[j, 2] - true[i, 2])], axis=1) + g.standard_normal((N, 3)) * A.SIGMA
    ij = np.stack([i, j], axis=1).astype(np.int32)
    ij[N - 1] = (0, N - 1)                                                 # the loop edge, node N - 1 seen from node 0
    z[N - 1] = A.rel(true[0], true[N - 1])
    poses = true + g.standard_normal((N, 3)) * np.array([0.05, 0.05, 0.01])
    poses[:, 2] = A.np_wrap(poses[:, 2])
    return poses, ij, z, np.tile(1.0 / A.SIGMA ** 2, (N, 1))


@pytest.fixture(scope="module")
def ring257():
    return A.ring(257)


# ---- 1. device against hook ----------------------------------------------------------------------------------------------------------
@gpu
def test_one_node_and_two_nodes(hs_mod, ctx):
    capi = hs_mod.capi
    rep = new_rep(hs_mod, ctx)
    none = (np.zeros((0, 2), np.int32), np.zeros((0, 3)), np.zeros((0, 3)))
    got, it, fin = device_equals_hook(hs_mod, rep, np.array([[1.0, 2.0, 3.0]]), None, *none, capi.pg_spec(2, 3))
    assert np.array_equal(got, [[1.0, 2.0, 3.0]]) and fin == 0.0 and it["cg_iters"].tolist() == [0, 0] and it["stopped"].tolist() == [0, 0]
    poses = np.array([[0.5, -1.0, 0.3], [2.0, 0.25, -0.4]])
    ij = np.array([[0, 1]], np.int32); z = np.array([[1.25, -0.5, 0.7]]); w = np.array([[4.0, 9.0, 25.0]])
    got, it, fin = device_equals_hook(hs_mod, rep, poses, None, ij, z, w, capi.pg_spec(1, 3))
    assert np.abs(got[1] - A.compose(poses[0], z[0])).max() <= 1e-12
    device_equals_hook(hs_mod, rep, poses, [0, 1], ij, z, w, capi.pg_spec(4, 3, check_every=1))
    device_equals_hook(hs_mod, rep, poses, None, ij, z, w, capi.pg_spec(2, 2, lam=0.5, tol=0.0))    # n_cg reached
    rep.close()


@gpu
def test_ring_of_257(hs_mod, ctx, ring257):
    poses, ij, z, w = ring257
    rep = new_rep(hs_mod, ctx)
    got, it, fin = device_equals_hook(hs_mod, rep, poses, None, ij, z, w, hs_mod.capi.pg_spec(6, 4 * 257, tol=1e-6))
    assert it[-1]["stopped"] == 0 and (it["cg_iters"] > 257).all() and fin < it[0]["chi2"]
    rep.close()


@gpu
def test_chain_of_65537_with_a_loop(hs_mod, ctx):
    poses, ij, z, w = chain(65537, 5)
    rep = new_rep(hs_mod, ctx)
    got, it, fin = device_equals_hook(hs_mod, rep, poses, None, ij, z, w, hs_mod.capi.pg_spec(1, 8, check_every=3))
    assert it[0]["cg_iters"] == 8 and it[0]["stopped"] == 1 and fin < it[0]["chi2"]
    # the stop word on 257 workgroups: tol = 0.1 is reached after 3 and 18 iterations, inside batches of 7 whose later launches leave
    got, it, fin = device_equals_hook(hs_mod, rep, poses, None, ij, z, w, hs_mod.capi.pg_spec(2, 64, check_every=7, tol=0.1))
    assert it["stopped"].tolist() == [0, 0] and (it["cg_iters"] > 0).all() and (it["cg_iters"] < 64).all()
    rep.close()


@gpu
def test_star_duplicates_reverse_and_fixed(hs_mod, ctx):
    capi = hs_mod.capi
    rep = new_rep(hs_mod, ctx)
    g = np.random.Generator(np.random.Philox(9))
    # a star: node 0 the centre, 1000 leaves; the centre is FREE (leaf 1 is fixed), so one lane sums 1000 edges
    L = 1000
    ang = 2.0 * np.pi * np.arange(L) / L
    true = np.concatenate([[[0.0, 0.0, 0.2]], np.stack([3.0 * np.cos(ang), 3.0 * np.sin(ang), ang], axis=1)])
    ij = np.stack([np.zeros(L, np.int32), np.arange(1, L + 1, dtype=np.int32)], axis=1)
    ij[::2] = ij[::2, ::-1]                                                # every other edge points at the centre
    z = np.stack([A.rel(true[i], true[j]) for i, j in ij]) + g.standard_normal((L, 3)) * 0.01
    w = g.uniform(1.0, 100.0, (L, 3))
    poses = true + g.standard_normal((L + 1, 3)) * 0.05
    fixed = np.zeros(L + 1, np.uint8); fixed[1] = 1
    device_equals_hook(hs_mod, rep, poses, fixed, ij, z, w, capi.pg_spec(2, 30))
    # duplicated edges, edges in reverse index order, the fixed node in the middle, two fixed nodes
    p, e, zz, ww = A.ring(40, seed=12)
    dup = np.concatenate([np.arange(40), [3, 3, 17]])
    z2 = zz[dup].copy(); z2[40:] += 0.005
    device_equals_hook(hs_mod, rep, p, None, e[dup], z2, ww[dup], capi.pg_spec(3, 160))
    rev = np.arange(40)[::-1]
    a = device_equals_hook(hs_mod, rep, p, None, e[rev], zz[rev], ww[rev], capi.pg_spec(3, 160))
    b = device_equals_hook(hs_mod, rep, p, None, e, zz, ww, capi.pg_spec(3, 160))
    assert np.abs(a[0] - b[0]).max() <= 1e-9
    mid = np.zeros(40, np.uint8); mid[20] = 1
    got, _, _ = device_equals_hook(hs_mod, rep, p, mid, e, zz, ww, capi.pg_spec(3, 160))
    assert np.array_equal(got[20], p[20]) and not np.array_equal(got[0], p[0])
    two = mid.copy(); two[5] = 1
    got, _, _ = device_equals_hook(hs_mod, rep, p, two, e, zz, ww, capi.pg_spec(3, 160, lam=1e-3))
    assert np.array_equal(got[[5, 20]], p[[5, 20]])
    rep.close()


# ---- 2. the call's life ----------------------------------------------------------------------------------------------------------------
@gpu
def test_check_every_and_two_calls(hs_mod, ctx, ring257):
    capi = hs_mod.capi
    poses, ij, z, w = ring257
    rep = new_rep(hs_mod, ctx)
    ck = [rep.Maps[l].checksum() for l in range(2)]
    n_cg = 4 * 257
    runs = []
    for every in (1, 7, n_cg):
        rep.PgSet(poses, None, ij, z, w)
        it, fin = rep.PgRelax(capi.pg_spec(2, n_cg, check_every=every))
        runs.append((rep.PgGet().tobytes(), it.tobytes(), fin))
    assert runs[0] == runs[1] == runs[2]
    rep.PgSet(poses, None, ij, z, w)
    six, fin6 = rep.PgRelax(capi.pg_spec(6, n_cg))
    p6 = rep.PgGet()
    rep.PgSet(poses, None, ij, z, w)
    a, _ = rep.PgRelax(capi.pg_spec(3, n_cg))
    b, fin33 = rep.PgRelax(capi.pg_spec(3, n_cg))                           # a second call continues from the relaxed poses
    same_iters(np.concatenate([a, b]), six)
    assert fin33 == fin6 and np.array_equal(rep.PgGet(), p6)
    assert [rep.Maps[l].checksum() for l in range(2)] == ck                # the grids are not touched
    rep.close()


@gpu
def test_set_twice_clear_reset_and_state(hs_mod, ctx, ring257):
    capi = hs_mod.capi
    rep = new_rep(hs_mod, ctx)
    spec = capi.pg_spec(1, 4)
    for call in (lambda: rep.PgRelax(spec), rep.PgGet, rep.PgResiduals):
        with pytest.raises(capi.SlamhipError) as e:                        # before slamhip_hs_pg_set
            call()
        assert e.value.code == capi.ERR_STATE
    poses, ij, z, w = ring257
    rep.PgSet(poses, None, ij, z, w)
    rep.PgRelax(spec)
    small = A.tiny_graph(3, 4, [(0, 1), (1, 2), (2, 3), (3, 0)])
    device_equals_hook(hs_mod, rep, small[0], None, small[1], small[2], small[3], capi.pg_spec(2, 12))      # the second graph is smaller
    with pytest.raises(capi.SlamhipError) as e:
        capi.call("slamhip_hs_pg_get", rep._h, np.zeros((5, 3)).ctypes.data_as(capi.C.c_void_p), 5)
    assert e.value.code == capi.ERR_INVALID
    bad = small[3].copy(); bad[1, 1] = 0.0
    with pytest.raises(capi.SlamhipError) as e:
        rep.PgSet(small[0], None, small[1], small[2], bad)
    assert e.value.code == capi.ERR_INVALID
    assert np.array_equal(rep.PgGet(), capi.debug_pg_relax(small[0], None, small[1], small[2], small[3], capi.pg_spec(2, 12))[0])   # a refused set leaves the graph
    for kw in (dict(n_outer=0), dict(n_cg=0), dict(check_every=0), dict(reserved=1), dict(tol=-1.0)):
        a = dict(n_outer=1, n_cg=4); a.update(kw)
        with pytest.raises(capi.SlamhipError) as e:
            rep.PgRelax(capi.pg_spec(**a))
        assert e.value.code == capi.ERR_INVALID, kw
    rep.PgClear()
    with pytest.raises(capi.SlamhipError) as e:
        rep.PgRelax(spec)
    assert e.value.code == capi.ERR_STATE
    rep.PgClear()
    rep.PgSet(small[0], None, small[1], small[2], small[3])
    rep.Reset()                                                            # slamhip_hs_reset drops the graph
    with pytest.raises(capi.SlamhipError) as e:
        rep.PgRelax(spec)
    assert e.value.code == capi.ERR_STATE
    rep.close()


# ---- 3. end to end ---------------------------------------------------------------------------------------------------------------
@gpu
def test_relax_keyframes_on_the_lap(hs_mod, ctx):
    """A closed lap of the simulator's field, a keyframe every metre; the stored poses drift (a heading bias that grows along the lap),
    ONE loop edge from the true relative pose of the last keyframe to the first.  Measured on an MI355X: the largest position error
    falls from 1.361 m to 0.024 m (137 PCG iterations per step).  Asserted: smaller, the store holds the relaxed poses, and device == hook."""
    import test_hs_sig_abi as S
    capi = hs_mod.capi
    sim, segs, true, scans = S.sim_lap()
    proc = hs_mod.HectorSLAMProcessor(0.1, (256, 256), (0.0, 0.0, 0.0), 2, ctx=ctx)
    proc.MapRep.SigConfigure(S.SIM_SCALE, S.SIM_RINGS, S.SIM_RC)
    N = len(scans)
    for i in range(N):
        proc.AddKeyframe(hs_mod.ScanCloud(scans[i], (0.0, 0.0, 0.0)), true[i])
    t64 = true.astype(D)
    drifted = [t64[0]]
    for k in range(N - 1):                                                 # odometry with a bias: 0.2 degrees and 2 mm per step
        zz = A.rel(t64[k], t64[k + 1]) + np.array([0.002, 0.0, np.radians(0.2)])
        drifted.append(A.compose(drifted[-1], zz))
    drifted = np.stack(drifted); drifted[:, 2] = A.np_wrap(drifted[:, 2])
    proc.MapRep.SigSetPoses(drifted.astype(np.float32))
    _, stored = proc.MapRep.SigDownload()
    assert np.array_equal(stored, drifted.astype(np.float32))
    before = np.hypot(*(stored[:, :2].astype(D) - t64[:, :2]).T).max()
    loop = (N - 1, 0, A.rel(t64[N - 1], t64[0]), (1e4, 1e4, 1e4))
    odom_w = (400.0, 400.0, 2500.0)
    spec = capi.pg_spec(5, 4 * N, tol=1e-8)
    out, iters, chi2 = proc.RelaxKeyframes([loop], odom_w, spec)
    after = np.hypot(*(out[:, :2] - t64[:, :2]).T).max()
    print("largest keyframe position error: %.3f m before, %.3f m after; PCG iterations %s" % (before, after, iters["cg_iters"].tolist()))
    assert after < before
    _, stored2 = proc.MapRep.SigDownload()
    assert np.array_equal(stored2, out.astype(np.float32)) and chi2.shape == (N,)
    # the hook over the same graph
    p0 = stored.astype(D)
    ij = [(k, k + 1) for k in range(N - 1)] + [(N - 1, 0)]
    z = [capi.pg_edge_between(p0[k], p0[k + 1]) for k in range(N - 1)] + [tuple(loop[2])]
    w = [odom_w] * (N - 1) + [loop[3]]
    hp, hit, _, _, hc = capi.debug_pg_relax(p0, None, np.array(ij, np.int32), np.array(z), np.array(w), spec)
    assert np.array_equal(out, hp) and np.array_equal(chi2, hc)
    same_iters(iters, hit)
    with pytest.raises(capi.SlamhipError) as e:
        proc.MapRep.SigSetPoses(np.zeros((2, 3), np.float32), first=N - 1)
    assert e.value.code == capi.ERR_INVALID
    proc.Dispose()
