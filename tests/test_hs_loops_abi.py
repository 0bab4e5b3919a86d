"""CPU-side checks of the consistent set of loop edges (K23): the host hook slamhip_debug_loops_consistent -- hs_loops.h, the text the
kernels run, in plain loops -- against the NumPy restatement of tests/loops_cases.py with == on every field, the properties the
definition promises, the struct layouts, the refusals, and the end the unit is for: the ring's relaxation with the kept edges
against the relaxation with all of them.  No compute calls on a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import loops_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi():
    import slam.net_amd.build as b
    b.build()
    import slam.net_amd.capi as capi
    return capi


def hook(capi, case, **kw):
    return capi.debug_loops_consistent(case["poses"], case["ij"], case["z"], case["w"], capi.loops_spec(**case["spec"]), use=case["use"], **kw)


def same(got, want, what, d2=False):
    assert np.array_equal(got["keep"], want["keep"]), (what, "keep", np.flatnonzero(got["keep"]), np.flatnonzero(want["keep"]))
    assert np.array_equal(got["deg"], want["deg"]), (what, "deg")
    wi = want["info"] if isinstance(want["info"], dict) else {k: int(want["info"][k]) for k in want["info"].dtype.names}
    for k, v in wi.items():
        assert int(got["info"][k]) == v, (what, k, int(got["info"][k]), v)
    assert got["adj"].shape == want["adj"].shape and np.array_equal(got["adj"], want["adj"]), (what, "adj")
    if d2:
        assert np.array_equal(got["d2"], want["d2"], equal_nan=True), (what, "d2", np.argwhere(got["d2"] != want["d2"])[:4])


def all_cases(capi):
    return list(lc.CASES.items()) + [("first_non_resident", lambda: lc.big_case(capi))]


def test_symbols_struct_layout_and_build_list(capi):
    L = capi.lib()
    for n in ("slamhip_hs_loops_consistent", "slamhip_hs_loops_clear", "slamhip_debug_loops_consistent"):
        assert hasattr(L, n) and n in L._signatures
    assert [(n, capi.LOOPS_SPEC.fields[n][1]) for n in capi.LOOPS_SPEC.names] == [("gamma", 0), ("q_t", 8), ("q_theta", 16), ("n_starts", 24),
                                                                                 ("min_clique", 28), ("flags", 32), ("reserved", 36)]
    assert [(n, capi.LOOPS_INFO.fields[n][1]) for n in capi.LOOPS_INFO.names] == [("n_pairs", 0), ("n_used", 8), ("size", 12), ("start", 16),
                                                                                 ("rank", 20), ("n_starts", 24), ("reserved", 28)]
    assert capi.LOOPS_SPEC.itemsize == 40 and capi.LOOPS_INFO.itemsize == 32
    header = open(os.path.join(ROOT, "include", "slamhip.h")).read()
    assert re.search(r"\} slamhip_loops_spec;\s*/\* 40 bytes \*/", header) and re.search(r"\} slamhip_loops_info;\s*/\* 32 bytes \*/", header)
    assert "#define SLAMHIP_LOOPS_ADJ %d" % capi.LOOPS_ADJ in header and "#define SLAMHIP_LOOPS_MAX_EDGES %d" % capi.LOOPS_MAX_EDGES in header
    shared = open(os.path.join(ROOT, "slam.net_amd", "csrc", "hs_loops.h")).read()
    assert "#define HS_LP_LDS_ADJ_BYTES (144 * 1024)" in shared and capi.LOOPS_LDS_ADJ_BYTES == 144 * 1024
    import slam.net_amd.build as b
    assert "hs_loops.hip" in b.SOURCES and "hs_loops.h" in b.HEADERS
    assert lc.first_non_resident(capi) == 1085


@pytest.mark.parametrize("name", sorted(lc.CASES) + ["first_non_resident"])
def test_hook_is_the_restatement(capi, name):
    case = dict(all_cases(capi))[name]()
    want = lc.restate(case)
    got = hook(capi, case, adj=True, d2=True)
    same(got, want, name, d2=True)
    L = case["ij"].shape[0]
    Cm = lc.unpack_rows(got["adj"], L)
    assert np.array_equal(Cm, want["C"])
    assert np.array_equal(Cm, Cm.T) and not Cm.diagonal().any()            # symmetric, zero diagonal
    assert not lc.unpack_rows(got["adj"], got["adj"].shape[1] * 64)[:, L:].any()   # the bits past L
    keep = got["keep"]
    if keep.any():
        members = np.flatnonzero(keep)
        assert Cm[np.ix_(members, members)].sum() == members.size * (members.size - 1)     # a clique ...
        assert not Cm[:, members].all(axis=1).any()                                          # ... and maximal: nobody is joined to all of it
        assert members.size == int(got["info"]["size"]) >= case["spec"]["min_clique"]
        assert keep[int(got["info"]["start"])]
    use = np.ones(L, bool) if case["use"] is None else case["use"]
    assert not keep[~use].any() and not Cm[~use].any()
    assert int(got["info"]["n_used"]) == int(use.sum()) and int(got["info"]["n_pairs"]) == int(np.triu(Cm, 1).sum())


@pytest.mark.parametrize("name", lc.BRUTE)
def test_greedy_finds_a_maximum_clique(capi, name):
    """Every case with L <= 24 that claims it, the ring among them: the greedy set is a maximum clique of the consistency graph."""
    case = lc.CASES[name]()
    got = hook(capi, case, adj=True)
    L = case["ij"].shape[0]
    size, cliques = lc.brute_max_clique(lc.unpack_rows(got["adj"], L))
    assert int(got["info"]["size"]) == size
    assert tuple(np.flatnonzero(got["keep"])) in cliques


def test_ring_keeps_exactly_the_true_loops(capi):
    case = lc.CASES["ring"]()
    assert case["poses"].shape[0] == 200 and int(case["is_true"].sum()) == 12 and int((~case["is_true"]).sum()) == 9
    got = hook(capi, case)
    assert np.array_equal(got["keep"], case["is_true"])
    masked = lc.CASES["ring_masked"]()
    assert np.array_equal(hook(capi, masked)["keep"], masked["is_true"] & masked["use"])
    dup = lc.CASES["ring_duplicates"]()
    assert np.array_equal(hook(capi, dup)["keep"], dup["is_true"]) and len({tuple(e) for e in dup["ij"]}) < dup["ij"].shape[0]
    rev = lc.CASES["ring_reversed"]()
    assert (rev["ij"][:, 1] < rev["ij"][:, 0]).sum() == 5


def test_threshold_ties_and_min_clique(capi):
    z0 = hook(capi, lc.CASES["threshold_all_zero"](), d2=True)
    assert z0["keep"].all() and not z0["d2"].any() and int(z0["info"]["n_pairs"]) == 15            # d2 == 0 <= gamma == 0
    u = hook(capi, lc.CASES["threshold_one_ulp"](), d2=True)
    assert list(u["keep"]) == [True, True, True, False, True]
    assert (u["d2"][3, [0, 1, 2, 4]] > 0).all() and (u["d2"][3, [0, 1, 2, 4]] < 1e-30).all()      # one ulp of ex, squared
    for name in ("tie_two_cliques", "tie_two_cliques_one_start"):
        t = hook(capi, lc.CASES[name]())
        assert list(np.flatnonzero(t["keep"])) == [0, 2, 5] and (t["deg"] == 2).all() and int(t["info"]["start"]) == 0 and int(t["info"]["rank"]) == 0
    p = hook(capi, lc.CASES["tie_path"]())
    assert list(np.flatnonzero(p["keep"])) == [0, 1] and int(p["info"]["start"]) == 1
    m = hook(capi, lc.CASES["min_clique_above"]())
    assert not m["keep"].any() and int(m["info"]["size"]) == 12 and int(m["info"]["start"]) >= 0
    n = hook(capi, lc.CASES["nothing_used"]())
    assert not n["keep"].any() and [int(n["info"][k]) for k in ("size", "start", "rank", "n_starts", "n_used")] == [0, -1, -1, 0, 0]


@pytest.mark.parametrize("wrong", lc.WRONG)
def test_wrong_variants_fail(capi, wrong):
    """Each deliberately wrong copy of a rule differs from the hook on at least one case."""
    caught = []
    for name, make in lc.CASES.items():
        case = make()
        got, bad = hook(capi, case, adj=True), lc.restate(case, wrong)
        if not (np.array_equal(got["keep"], bad["keep"]) and np.array_equal(got["adj"], bad["adj"])):
            caught.append(name)
    assert caught, wrong


def raw(capi, name, handle, poses, N, ij, z, w, use, L, spec, adj_ptr=True, d2=False):
    """The call with sentinel-filled outputs -> (status, outputs untouched?)."""
    keep = np.full(max(L, 1) + 8, 0xA5, np.uint8); deg = np.full(max(L, 1) + 8, -77, np.int32); info = np.full(8, -77, np.int32)
    A = np.full(64 * 64, 0xA5A5A5A5A5A5A5A5, np.uint64)
    args = [capi._vp(poses), N, capi._vp(ij), capi._vp(z), capi._vp(w), capi._vp(use), L, spec.ctypes.data_as(C.c_void_p), capi._vp(keep), capi._vp(deg),
            capi._vp(info), capi._vp(A) if adj_ptr else None]
    if handle is None:
        rc = getattr(capi.lib(), name)(*args, None)
    else:
        rc = getattr(capi.lib(), name)(handle, *args)
    clean = (keep == 0xA5).all() and (deg == -77).all() and (info == -77).all() and (A == 0xA5A5A5A5A5A5A5A5).all()
    return rc, bool(clean)


def refusals(capi):
    """(what, kwargs for raw) for every refusal of rule 7."""
    c = lc.CASES["ring"]()
    L = c["ij"].shape[0]; N = c["poses"].shape[0]
    base = dict(poses=c["poses"].copy(), N=N, ij=c["ij"].copy(), z=c["z"].copy(), w=c["w"].copy(), use=None, L=L, spec=capi.loops_spec(**c["spec"]))

    def edit(what, **kw):
        d = dict(base)
        for k, v in kw.items():
            if callable(v):
                a = d[k].copy(); v(a); d[k] = a
            else:
                d[k] = v
        return what, d
    nan, inf = float("nan"), float("inf")
    out = [edit("L = 0", L=0), edit("L = 4097", L=4097), edit("N = 0", N=0), edit("N = 2^20 + 1", N=(1 << 20) + 1),
           edit("i = N", ij=lambda a: a.__setitem__((3, 0), N)), edit("j = -1", ij=lambda a: a.__setitem__((5, 1), -1)),
           edit("an end past a smaller N", N=100),
           edit("pose nan", poses=lambda a: a.__setitem__((199, 0), nan)), edit("pose inf", poses=lambda a: a.__setitem__((0, 1), inf)),
           edit("pose theta nan", poses=lambda a: a.__setitem__((7, 2), nan)), edit("pose theta 40000", poses=lambda a: a.__setitem__((7, 2), 40000.0)),
           edit("z nan", z=lambda a: a.__setitem__((2, 1), nan)), edit("z theta inf", z=lambda a: a.__setitem__((2, 2), -inf)),
           edit("w nan", w=lambda a: a.__setitem__((20, 0), nan)), edit("w inf", w=lambda a: a.__setitem__((20, 2), inf)),
           edit("w = 0", w=lambda a: a.__setitem__((0, 1), 0.0)), edit("w < 0", w=lambda a: a.__setitem__((0, 2), -1.0))]
    for what, bad in (("gamma < 0", dict(gamma=-1e-300)), ("gamma nan", dict(gamma=nan)), ("gamma inf", dict(gamma=inf)), ("q_t < 0", dict(q_t=-1.0)),
                      ("q_t nan", dict(q_t=nan)), ("q_theta inf", dict(q_theta=inf)), ("q_theta < 0", dict(q_theta=-1.0)), ("n_starts = 0", dict(n_starts=0)),
                      ("n_starts = 65", dict(n_starts=65)), ("min_clique = 0", dict(min_clique=0)), ("flags = 2", dict(flags=2)), ("reserved = 1", dict(reserved=1))):
        out.append(edit(what, spec=capi.loops_spec(**dict(c["spec"], **bad))))
    out.append(("SLAMHIP_LOOPS_ADJ without out_adj", dict(base, spec=capi.loops_spec(flags=capi.LOOPS_ADJ, **c["spec"]), adj_ptr=False)))
    return out


def test_refusals_write_nothing(capi):
    for what, kw in refusals(capi):
        rc, clean = raw(capi, "slamhip_debug_loops_consistent", None, **kw)
        assert rc == capi.ERR_INVALID and clean, (what, rc, clean)
    c = lc.CASES["ring"]()
    rc, clean = raw(capi, "slamhip_debug_loops_consistent", None, c["poses"], 200, c["ij"], c["z"], c["w"], None, 21, capi.loops_spec(**c["spec"]))
    assert rc == 0 and not clean                                           # (the same call, not refused, writes)
    i_eq_j = dict(lc.flat([1.0, 1.0]), ij=np.array([[1, 1], [0, 1]], np.int32))
    assert hook(capi, i_eq_j)["keep"].all()                                # an edge with i == j is no refusal


def relax(capi, case, loops):
    """The chain's odometry edges from the poses as they stand plus `loops`, relaxed by the existing hook, node 0 fixed."""
    p = case["poses"]; N = p.shape[0]
    ij = [(k, k + 1) for k in range(N - 1)]; z = [capi.pg_edge_between(p[k], p[k + 1]) for k in range(N - 1)]
    w = [(400.0, 400.0, 2500.0)] * (N - 1)
    for n in loops:
        ij.append(tuple(int(v) for v in case["ij"][n])); z.append(tuple(case["z"][n])); w.append(tuple(case["w"][n]))
    poses, iters, chi2, _, _ = capi.debug_pg_relax(p, None, ij, z, w, capi.pg_spec(8, 4 * N, tol=1e-10))
    return poses, chi2


def test_ring_relaxes_better_with_the_kept_edges(capi):
    """What the unit is for: the ring relaxed with the kept edges alone ends at a lower chi2, and nearer the truth, than with all 21."""
    case = lc.CASES["ring"]()
    keep = hook(capi, case)["keep"]
    p_keep, chi2_keep = relax(capi, case, np.flatnonzero(keep))
    p_all, chi2_all = relax(capi, case, range(case["ij"].shape[0]))

    def err(p):
        return float(np.hypot(p[:, 0] - case["true"][:, 0], p[:, 1] - case["true"][:, 1]).max())
    print("chi2: kept %.4g, all %.4g; largest translation error: drifted %.3f m, kept %.3f m, all %.3f m"
          % (chi2_keep, chi2_all, err(case["poses"]), err(p_keep), err(p_all)))
    assert chi2_keep < chi2_all
    assert err(p_keep) < err(p_all)
    assert err(p_keep) < err(case["poses"])
