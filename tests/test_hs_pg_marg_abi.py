"""CPU-side checks of the pose graph's marginal covariances (K27: slamhip_hs_pg_marginals, slamhip_debug_pg_marginals): the host hook --
the header text the kernels run, in plain loops, its PCG the one of slamhip_debug_pg_relax -- against the NumPy restatement of rules
M1 - M5 (tests/pg_marg_cases.py) under == on every case and every field, three wrong copies of the restatement that must each differ,
a closed form, the dense inverse, and the hook's invariances.  No device is involved; tests/test_gpu_hector_pg_marg.py ties the
kernels to the hook."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pg_marg_cases as mc
import pg_tri_cases as tc
import test_hs_pg_abi as A
from test_hs_pg_abi import capi                                            # noqa: F401 (fixture)

D = np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = mc.cases()
COL_FIELDS = ("rz0", "rz", "cg_iters", "stopped", "node", "comp")
INFO_FIELDS = ("n_cols", "n_rhs", "rhs_per_chunk", "n_chunks", "group")


def hook(capi, c, precond, **kw):
    """The hook on a catalogue case -> (blocks, cols, info)."""
    name, num = precond
    spec = capi.pg_marg_spec(kw.pop("n_cg", c["n_cg"][num]), precond=name, lam=kw.pop("lam", c["lam"]), tol=kw.pop("tol", c["tol"]), **kw)
    return capi.debug_pg_marginals(c["poses"], c["fixed"], c["ij"], c["z"], c["w"], spec, c["pairs"])


def restatement(c, precond, wrong=None, **kw):
    return mc.np_marginals(c["poses"], c["fixed"], c["ij"], c["z"], c["w"], c["pairs"], kw.pop("n_cg", c["n_cg"][precond[1]]), precond[1],
                           lam=c["lam"], tol=kw.pop("tol", c["tol"]), wrong=wrong, **kw)


def equal(got, want):
    """Every field under == (blocks by their bytes: a zero's sign counts)."""
    (gb, gc, gi), (wb, wc, wi) = got, want
    if gb.tobytes() != np.ascontiguousarray(wb).tobytes() or gc.shape[0] != len(wc):
        return False
    return all(gc[j][f] == wc[j][f] for j in range(len(wc)) for f in COL_FIELDS) and all(gi[f] == wi[f] for f in INFO_FIELDS) and not gi["reserved"].any()


@pytest.fixture(scope="module")
def hooked(capi):
    """The hook's outputs of every case and preconditioner, computed once."""
    return {(name, pc[0]): hook(capi, c, pc) for name, c in CASES.items() for pc in mc.PRECONDS}


# ---- 1. the ABI ----------------------------------------------------------------------------------------------------------------------
def test_symbols_and_struct_layout(capi):
    hdr = open(os.path.join(ROOT, "include", "slamhip.h")).read()
    for name in ("slamhip_hs_pg_marginals", "slamhip_debug_pg_marginals"):
        assert name in capi.declared_symbols() and hasattr(capi.lib(), name)
    assert capi.PG_MARG_SPEC.itemsize == 40 and capi.PG_MARG_COL.itemsize == 32 and capi.PG_MARG_INFO.itemsize == 32
    assert [capi.PG_MARG_SPEC.fields[f][1] for f in ("n_cg", "check_every", "precond", "reserved", "lambda", "tol", "max_bytes")] == [0, 4, 8, 12, 16, 24, 32]
    assert [capi.PG_MARG_COL.fields[f][1] for f in COL_FIELDS] == [0, 8, 16, 20, 24, 28]
    assert [capi.PG_MARG_INFO.fields[f][1] for f in INFO_FIELDS + ("reserved",)] == [0, 4, 8, 12, 16, 20]
    assert int(re.search(r"#define SLAMHIP_PG_MARG_MAX_COLS (\d+)", hdr).group(1)) == capi.PG_MARG_MAX_COLS == 4096
    assert re.search(r"#define SLAMHIP_PG_MARG_MAX_PAIRS \(1 << 20\)", hdr) and capi.PG_MARG_MAX_PAIRS == 1 << 20
    build = open(os.path.join(ROOT, "slam.net_amd", "build.py")).read()
    import slam.net_amd.build as b
    assert "hs_pg_marg.inc" in b.HEADERS and "hs_pg_marg.h" in b.HEADERS and "hs_pg_marg" not in " ".join(b.SOURCES), build[:0]
    native = open(os.path.join(ROOT, "bindings", "csharp", "SlamHip", "SlamHip.Native.cs")).read()
    rep = open(os.path.join(ROOT, "bindings", "csharp", "SlamHip", "HectorSLAM", "MapRepMultiMap.Hip.cs")).read()
    assert "slamhip_hs_pg_marginals" in native and "Native.slamhip_hs_pg_marginals" in rep


def test_one_pcg_on_the_host_and_one_enqueue_loop():
    """The one-definition rule of the unit: rule 7's loop stands once in the host text and the batches' enqueue loop once in the
    drivers, K27 included."""
    src = "".join(open(os.path.join(ROOT, "slam.net_amd", "csrc", f)).read() for f in ("hs_pg.hip", "hs_pg_tri.inc", "hs_pg_lm.inc", "hs_pg_marg.inc"))
    assert len(re.findall(r"const double beta = rzn / rz;", src)) == 1     # the host PCG
    assert len(re.findall(r"K19_MAX_BATCH\)", src)) == 1                   # the enqueue loop
    marg = open(os.path.join(ROOT, "slam.net_amd", "csrc", "hs_pg_marg.inc")).read()
    assert "hs_pg_pcg_loop(" in marg and "hs_pg_host_pcg(" in marg and "atomicAdd" not in marg and "asm" not in marg.replace("hs_pg_marg", "")


# ---- 2. hook == restatement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precond", mc.PRECONDS, ids=lambda p: p[0])
@pytest.mark.parametrize("name", sorted(CASES))
def test_hook_equals_restatement(hooked, name, precond):
    got = hooked[(name, precond[0])]
    want = restatement(CASES[name], precond, group=int(got[2]["group"]))
    assert equal(got, want), (got[1], want[1], got[2], want[2])
    assert np.isfinite(got[0]).all()


@pytest.mark.parametrize("wrong", ["transposed", "shared_stop", "first_appearance"])
def test_wrong_copies_differ(hooked, wrong):
    differs = [(name, pc[0]) for name, c in CASES.items() for pc in mc.PRECONDS
               if not equal(hooked[(name, pc[0])], restatement(c, pc, wrong=wrong, group=4))]
    assert differs, wrong


def test_catalogue_reaches_what_it_claims(hooked):
    """Early stop: on one call some right-hand sides stop on the count and others on the tolerance.  Stop-word independence: a column
    next to a fixed node (32, beside 33) and one far from any (18, seven nodes from 11 and 25) differ in cg_iters, and the two sit in
    different groups of 4 while 31 and 32 share one with right-hand sides that run on.  The group edges a query can reach."""
    cols = hooked[("segments", "jacobi")][1]
    assert {0, 1} <= set(cols["stopped"].tolist()), cols["stopped"]
    near = cols[(cols["node"] == 32)]["cg_iters"]; far = cols[(cols["node"] == 18)]["cg_iters"]
    assert near.max() < far.min() and (cols[cols["node"] == 32]["stopped"] == 0).all() and (cols[cols["node"] == 18]["stopped"] == 1).all(), (near, far)
    assert {int(hooked[(n, "tri")][2]["n_rhs"]) for n in CASES} >= {0, 3, 6, 9, 12}
    dead = cols[cols["node"] == 30]                                        # a free node without an edge, lambda = 0: M = 0, x = 0 at once
    assert (dead["cg_iters"] == 0).all() and (dead["rz0"] == 0).all() and (dead["stopped"] == 0).all()
    b = hooked[("segments", "jacobi")][0]
    pairs = CASES["segments"]["pairs"]
    for p, (n, m) in enumerate(pairs):
        if n in (10, 30) or m in (10, 30):
            assert b[p].tobytes() == np.zeros((3, 3)).tobytes()            # fixed or dead: +0
    assert np.array_equal(b[0], b[1]) and b[0].any()                       # duplicates
    c = CASES["duplicates"]                                                # precond = 1 with room to spare (n_cg = 30): the tolerance ends every column within 6 L' + 1
    fx = np.zeros(c["poses"].shape[0], bool); fx[0] = True
    Lp = mc.free_loops(fx, c["ij"])
    cols = hooked[("duplicates", "tri")][1]
    assert Lp == 3 and (cols["stopped"] == 0).all() and (cols["cg_iters"] <= 6 * Lp + 1).all(), cols["cg_iters"]


# ---- 3. closed form, dense inverse ------------------------------------------------------------------------------------------------------
def test_chain_closed_form(capi):
    """A chain with node 0 fixed and theta = 0: the theta-theta entry of Sigma[k][k] is k / w_theta, and with precond = 1 T = H, so every
    column ends within 2 iterations.  The bound: PCG with T = H is exact after one iteration up to rounding; the entry is a sum of k
    terms 1 / w_theta formed through the cyclic reduction, each operation within 2^-53, fewer than 64 N operations on the path:
    |error| <= 64 N 2^-53 of the value (measured: 2.71e-16 relative at worst over k = 1, 2, 18, 36)."""
    c = CASES["chain37"]
    blocks, cols, info = hook(capi, c, ("tri", 1))
    assert (cols["cg_iters"] <= 2).all() and (cols["stopped"] == 0).all(), cols
    wt = c["w"][0, 2]
    worst = 0.0
    for p, (n, m) in enumerate(c["pairs"]):
        if n == m:
            want = n / wt
            worst = max(worst, abs(blocks[p][2, 2] - want) / want)
    print("chain closed form: worst relative error %.3g" % worst)
    assert worst <= 64 * 37 * 2.0 ** -53
    bj, cj, _ = hook(capi, c, ("jacobi", 0), n_cg=200)
    assert (cj["stopped"] == 0).all() and cj["cg_iters"].max() > 2
    assert np.allclose(bj, blocks, rtol=1e-6, atol=1e-12)


def dense_sigma(c):
    """H from the restatement's Jacobians, its free block inverted by LAPACK -> (Sigma over all nodes, 0 at fixed ones)."""
    poses, fx, ij, z, w = tc.np_graph(c["poses"], c["fixed"], c["ij"], c["z"], c["w"])
    N = poses.shape[0]
    Aj, Bj, _, _ = A.np_edges(poses, ij, z, w)
    H = np.zeros((3 * N, 3 * N), D)
    for e, (i, j) in enumerate(ij):
        J = np.zeros((3, 3 * N), D)
        J[:, 3 * i:3 * i + 3] = Aj[e]; J[:, 3 * j:3 * j + 3] = Bj[e]
        H += J.T @ np.diag(w[e]) @ J
    H += c["lam"] * np.eye(3 * N)
    free = np.repeat(~fx, 3)
    S = np.zeros_like(H)
    S[np.ix_(free, free)] = np.linalg.inv(H[np.ix_(free, free)])
    return S


@pytest.mark.parametrize("name", ["ring255", "ring256", "ring257"])
def test_hook_against_the_dense_inverse(capi, name):
    """precond = 1, tol = 1e-12, n_cg = 6 L' + 1.  Measured ||X - Sigma||_F / ||Sigma||_F over the queried blocks, against NumPy's
    LAPACK inverse: ring255 5.65e-11 (7 iterations), ring256 5.21e-14 (13), ring257 3.54e-13 (19); asserted 100 times that, and never
    looser than 1e-6."""
    measured = {"ring255": 5.65e-11, "ring256": 5.21e-14, "ring257": 3.54e-13}[name]
    c = CASES[name]
    fx = np.zeros(c["poses"].shape[0], bool); fx[0] = True
    Lp = mc.free_loops(fx, c["ij"])
    assert c["n_cg"][1] >= 6 * Lp + 1 and c["tol"] == 1e-12
    blocks, cols, info = hook(capi, c, ("tri", 1))
    assert (cols["cg_iters"] <= 6 * Lp + 1).all(), cols["cg_iters"]
    S = dense_sigma(c)
    want = np.stack([S[3 * n:3 * n + 3, 3 * m:3 * m + 3] for n, m in c["pairs"]])
    err = np.linalg.norm(blocks - want) / np.linalg.norm(want)
    print("%s: ||X - Sigma||_F / ||Sigma||_F = %.3g, cg_iters %s" % (name, err, cols["cg_iters"].tolist()))
    assert err <= min(100 * measured, 1e-6)


# ---- 4. invariances and refusals -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ring257", "segments", "duplicates"])
def test_invariant_to_max_bytes_and_check_every(capi, hooked, name):
    c = CASES[name]
    N = c["poses"].shape[0]
    for pc in mc.PRECONDS:
        base = hooked[(name, pc[0])]
        R = int(base[2]["n_rhs"])
        B = mc.rhs_bytes(N, pc[1])
        assert capi.pg_marg_rhs_bytes(N, pc[0]) == B
        assert base[2]["rhs_per_chunk"] == min(R, (256 << 20) // B) == R and base[2]["n_chunks"] == 1
        for Rc in mc.CHUNKS:
            got = hook(capi, c, pc, max_bytes=Rc * B + B - 1, check_every=1 if Rc & 1 else 1000)
            assert got[0].tobytes() == base[0].tobytes() and got[1].tobytes() == base[1].tobytes()
            assert got[2]["rhs_per_chunk"] == min(R, Rc) and got[2]["n_chunks"] == -(-R // min(R, Rc)) and got[2]["n_rhs"] == R


def test_group_switch_is_read_and_changes_no_result(capi, hooked, monkeypatch):
    c = CASES["ring256"]
    monkeypatch.setenv("SLAMHIP_K27_GROUP", "4")
    got = hook(capi, c, ("tri", 1))
    base = hooked[("ring256", "tri")]
    assert got[2]["group"] == 4 and base[2]["group"] == capi.PG_MARG_GROUP == 1
    assert got[0].tobytes() == base[0].tobytes() and got[1].tobytes() == base[1].tobytes()
    monkeypatch.setenv("SLAMHIP_K27_GROUP", "3")                           # not instantiated: the default
    assert hook(capi, c, ("tri", 1))[2]["group"] == 1


def raw(capi, c, spec, pairs, P=None):
    """The hook with outputs the caller can inspect after a refusal -> (rc, blocks, cols, n, info)."""
    p, fx, e, zz, ww = capi.pg_graph(c["poses"], c["fixed"], c["ij"], c["z"], c["w"])
    pr = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
    blocks = np.full((max(pr.shape[0], 1), 3, 3), 7.0); cols = np.full(3 * 4096, 0x55, np.uint8).view(capi.PG_MARG_COL).copy()
    n = C.c_int32(-5); info = np.full(32, 0x55, np.uint8)
    rc = capi.lib().slamhip_debug_pg_marginals(capi._vp(p), capi._vp(fx), p.shape[0], capi._vp(e), capi._vp(zz), capi._vp(ww), e.shape[0],
                                               spec.ctypes.data_as(C.c_void_p), capi._vp(pr), pr.shape[0] if P is None else P, blocks.ctypes.data_as(C.c_void_p),
                                               cols.ctypes.data_as(C.c_void_p), C.byref(n), info.ctypes.data_as(C.c_void_p))
    return rc, blocks, cols, n.value, info


def test_refusals_write_nothing(capi):
    c = CASES["segments"]
    good = dict(n_cg=5, precond="tri")
    bad_specs = [dict(good, n_cg=0), dict(good, n_cg=(1 << 20) + 1), dict(good, check_every=0), dict(good, precond=2), dict(good, precond=-1),
                 dict(good, reserved=1), dict(good, lam=-1.0), dict(good, lam=float("nan")), dict(good, tol=-1e-3), dict(good, tol=float("inf")),
                 dict(good, max_bytes=-1)]
    runs = [(capi.pg_marg_spec(**s), c["pairs"], None, capi.ERR_INVALID) for s in bad_specs]
    ok = capi.pg_marg_spec(**good)
    runs += [(ok, [(0, 40)], None, capi.ERR_INVALID), (ok, [(-1, 3)], None, capi.ERR_INVALID), (ok, [(40, 3)], None, capi.ERR_INVALID),
             (ok, c["pairs"], 0, capi.ERR_INVALID), (ok, c["pairs"], (1 << 20) + 1, capi.ERR_INVALID),
             (capi.pg_marg_spec(max_bytes=mc.rhs_bytes(40, 1) - 1, **good), c["pairs"], None, capi.ERR_NOMEM)]
    for spec, pairs, P, want in runs:
        rc, blocks, cols, n, info = raw(capi, c, spec, pairs, P)
        assert rc == want, (rc, want, spec, P)
        assert (blocks == 7.0).all() and (cols.view(np.uint8) == 0x55).all() and n == -5 and (info == 0x55).all()
    rc, blocks, cols, n, info = raw(capi, c, capi.pg_marg_spec(max_bytes=mc.rhs_bytes(40, 1), **good), c["pairs"])
    assert rc == 0 and n == 21 and info.view(capi.PG_MARG_INFO)[0]["rhs_per_chunk"] == 1 and info.view(capi.PG_MARG_INFO)[0]["n_chunks"] == 21


def test_column_cap(capi):
    """C = 4096 columns are taken (n_cg = 1: the solve is not the point), 4097 refused."""
    N = 4098
    poses, ij, z, w = mc.chain(N)
    c = dict(poses=poses, fixed=None, ij=ij, z=z, w=w)
    spec = capi.pg_marg_spec(1, precond="jacobi")
    rc, _, _, n, info = raw(capi, c, spec, [(1, m) for m in range(1, 4098)])
    assert rc == capi.ERR_INVALID and n == -5
    blocks, cols, info = capi.debug_pg_marginals(poses, None, ij, z, w, spec, [(1, m) for m in range(0, 4097)])   # m = 0 is fixed: no column
    assert info["n_cols"] == 4096 and cols.shape[0] == 3 * 4096 and (cols["stopped"] == 1).all() and not blocks[0].any()
    assert np.array_equal(cols["node"], np.repeat(np.arange(1, 4097), 3)) and np.array_equal(cols["comp"], np.tile([0, 1, 2], 4096))


# ---- 5. the helpers of capi.py -----------------------------------------------------------------------------------------------------------
def test_relative_covariance_and_mahalanobis(capi):
    """pg_relative_covariance against J Sigma J^T with J = [A B] written out, pg_mahalanobis against the explicit inverse."""
    g = np.random.Generator(np.random.Philox(5))
    L = g.standard_normal((6, 6)); S = L @ L.T
    pi, pj = np.array([0.3, -0.2, 0.7]), np.array([1.1, 0.4, -0.5])
    Aj, Bj, _, _ = A.np_edges(np.stack([pi, pj]), np.array([[0, 1]]), np.zeros((1, 3)), np.ones((1, 3)))
    J = np.concatenate([Aj[0], Bj[0]], axis=1)
    got = capi.pg_relative_covariance(pi, pj, S[:3, :3], S[:3, 3:], S[3:, :3], S[3:, 3:])
    assert np.allclose(got, J @ S @ J.T, rtol=1e-12, atol=1e-12)
    r = np.array([0.1, -0.05, 0.02]); w = np.array([400.0, 400.0, 2500.0])
    assert np.isclose(capi.pg_mahalanobis(r, got, w), r @ np.linalg.inv(got + np.diag(1 / w)) @ r, rtol=1e-12)
