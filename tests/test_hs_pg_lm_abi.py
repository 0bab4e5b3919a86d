"""CPU-side checks of the damped and robust relaxation's interface (K26: slamhip_hs_pg_relax_lm and the hook slamhip_debug_pg_relax_lm)
and of its definition (include/slamhip.h, rules R1 - R4): hook == the NumPy restatement of tests/pg_lm_cases.py with == on the poses,
every record field, F_final and f; every wrong copy of a rule fails its named case; NONE with lambda = 0 is slamhip_debug_pg_relax /
_relax_tri; the behaviour the unit exists for, on the issue's ring A and graph B, within the issue's bounds; the refusals.  No compute
calls on a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pg_lm_cases as lc
import test_hs_pg_abi as A
from test_hs_pg_abi import capi                                            # noqa: F401 (fixture)

ROOT = A.ROOT
D = np.float64
SYMBOLS = ("slamhip_hs_pg_relax_lm", "slamhip_debug_pg_relax_lm")
SPEC_OFFSETS = (("n_outer", 0), ("n_cg", 4), ("check_every", 8), ("precond", 12), ("kind", 16), ("reserved", 20), ("lambda0", 24), ("up", 32),
                ("down", 40), ("lambda_min", 48), ("lambda_max", 56), ("tol", 64), ("ftol", 72), ("phi", 80))
ITER_OFFSETS = (("F", 0), ("F_trial", 8), ("lambda", 16), ("rz0", 24), ("rz", 32), ("cg_iters", 40), ("stopped", 44), ("accepted", 48), ("reserved", 52))


# ---- 1. the interface ----------------------------------------------------------------------------------------------------------------
def test_symbols_and_struct_layout(capi):
    L = capi.lib()
    declared = set(capi.declared_symbols())
    for name in SYMBOLS:
        assert name in declared and hasattr(L, name) and name in L._signatures, name
    header = open(os.path.join(ROOT, "include", "slamhip.h")).read()
    for text in ("} slamhip_pg_lm_spec;                  /* 88 bytes */", "} slamhip_pg_lm_iter;                  /* 64 bytes */", " *  R1. ", " *  R2. ", " *  R3. ",
                 " *  R4. "):
        assert text in header, text
    assert capi.PG_LM_SPEC.itemsize == 88 and capi.PG_LM_ITER.itemsize == 64
    assert [(n, capi.PG_LM_SPEC.fields[n][1]) for n, _ in SPEC_OFFSETS] == list(SPEC_OFFSETS)
    assert [(n, capi.PG_LM_ITER.fields[n][1]) for n, _ in ITER_OFFSETS] == list(ITER_OFFSETS)
    for n, off in SPEC_OFFSETS:
        assert re.search(r"%s;\s*/\* offset %d:" % (n, off), header), n
    # the library's own view of the spec: a record whose tol, at offset 64, is 2 stops before iteration 0, and phi sits at offset 80
    poses, ij, z, w = lc.one_edge(0)                                        # c_e = 1
    raw = np.zeros(88, np.uint8)
    raw[0:12] = np.array([1, 3, 1], np.int32).view(np.uint8); raw[16:20] = np.array([capi.PG_LM_DCS], np.int32).view(np.uint8)
    raw[24:88] = np.array([0.0, 2.0, 0.5, 0.0, 1.0, 2.0, 0.0, 0.5], D).view(np.uint8)
    _, it, _, f = capi.debug_pg_relax_lm(poses, None, ij, z, w, raw.view(capi.PG_LM_SPEC))
    assert it[0]["cg_iters"] == 0 and it[0]["stopped"] == 0 and f[0] == (D(1.0) / D(1.5)) * (D(1.0) / D(1.5))
    raw[80:88] = np.array([2.0], D).view(np.uint8)                        # phi = 2 > c_e
    assert capi.debug_pg_relax_lm(poses, None, ij, z, w, raw.view(capi.PG_LM_SPEC))[3][0] == 1.0


def test_csharp_and_build_list():
    native = open(os.path.join(ROOT, "bindings", "csharp", "SlamHip", "SlamHip.Native.cs")).read()
    assert re.search(r"static extern int slamhip_hs_pg_relax_lm\(", native)
    rep = open(os.path.join(ROOT, "bindings", "csharp", "SlamHip", "HectorSLAM", "MapRepMultiMap.Hip.cs")).read()
    assert "Native.slamhip_hs_pg_relax_lm(" in rep
    import slam.net_amd.build as b
    assert "hs_pg.hip" in b.SOURCES and "hs_pg_lm.h" in b.HEADERS and "hs_pg_lm.inc" in b.HEADERS
    unit = open(os.path.join(b.CSRC, "hs_pg.hip")).read()
    assert '#include "hs_pg_lm.inc"' in unit                               # the unit is part of hs_pg.hip's translation unit, as K22 is


def raw_relax_lm(capi, poses, fixed, ij, z, w, spec, robust=None):
    """The hook called with sentinel-filled outputs -> (return code, whether anything was written)."""
    p = np.array(poses, D).reshape(-1, 3); before = p.copy()
    e = np.array(ij, np.int32).reshape(-1, 2); zz = np.array(z, D).reshape(-1, 3); ww = np.array(w, D).reshape(-1, 3)
    fx = None if fixed is None else np.asarray(fixed, np.uint8)
    iters = np.full(64 * 8, -7.25, D); n = np.full(1, -7, np.int32); fin = np.full(1, -7.25, D); f = np.full(max(len(e), 1), -7.25, D)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)     # noqa: E731
    rc = capi.lib().slamhip_debug_pg_relax_lm(vp(p), vp(fx), p.shape[0], vp(e), vp(zz), vp(ww), e.shape[0], vp(spec), vp(robust), vp(iters), vp(n), vp(fin), vp(f))
    written = not (np.array_equal(p, before, equal_nan=True) and (iters == -7.25).all() and n[0] == -7 and fin[0] == -7.25 and (f == -7.25).all())
    return rc, written


def test_refusals_write_nothing(capi):
    poses, ij, z, w = A.tiny_graph(2, 3, [(0, 1), (1, 2)])
    rc, written = raw_relax_lm(capi, poses, None, ij, z, w, capi.pg_lm_spec(2, 5))
    assert rc == 0 and written
    bad = [dict(n_outer=0), dict(n_outer=65), dict(n_cg=0), dict(n_cg=(1 << 20) + 1), dict(check_every=0), dict(precond=2), dict(precond=-1), dict(kind=3),
           dict(kind=-1), dict(reserved=1), dict(lambda0=-1e-3), dict(lambda0=np.nan), dict(lambda0=np.inf), dict(up=1.0), dict(up=np.inf), dict(up=np.nan),
           dict(down=0.0), dict(down=1.5), dict(down=np.nan), dict(lambda_min=-1.0), dict(lambda_min=2.0, lambda_max=1.0), dict(lambda_max=np.inf),
           dict(lambda_min=np.nan), dict(tol=-1e-3), dict(tol=np.inf), dict(ftol=-1e-3), dict(ftol=np.nan), dict(kind="dcs", phi=0.0), dict(kind="gm", phi=-1.0),
           dict(kind="dcs", phi=np.inf), dict(kind="gm", phi=np.nan)]
    for kw in bad:
        a = dict(n_outer=2, n_cg=5); a.update(kw)
        rc, written = raw_relax_lm(capi, poses, None, ij, z, w, capi.pg_lm_spec(**a))
        assert rc == capi.ERR_INVALID and not written, kw
    for kw in (dict(kind="none", phi=-1.0), dict(down=1.0), dict(lambda_min=3.0, lambda_max=3.0), dict(n_outer=64, n_cg=1 << 20, tol=0.5, check_every=1 << 30)):
        a = dict(n_outer=2, n_cg=5); a.update(kw)                          # phi is not read for NONE; the ranges' closed ends
        assert raw_relax_lm(capi, poses, None, ij, z, w, capi.pg_lm_spec(**a))[0] == 0, kw
    pp = poses.copy(); pp[1, 2] = 65537.0                                  # the graph's refusals are slamhip_debug_pg_relax's
    ww = w.copy(); ww[1, 2] = 0.0
    for gr in ((pp, None, ij, z, w), (poses, None, ij, z, ww), (poses, None, [(0, 3), (1, 2)], z, w), (poses, np.zeros(3, np.uint8), ij, z, w)):
        rc, written = raw_relax_lm(capi, *gr, capi.pg_lm_spec(2, 5))
        assert rc == capi.ERR_INVALID and not written
    # the records behind *out_n are not written: rule R3's stop after the first accepted attempt
    p = np.array(poses, D); iters = np.full(4 * 8, -7.25, D); n = C.c_int32(-7); fin = C.c_double(0.0)
    e = np.array(ij, np.int32); spec = capi.pg_lm_spec(4, 50, ftol=1.0, lambda0=0.0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)                            # noqa: E731
    capi.call("slamhip_debug_pg_relax_lm", vp(p), None, 3, vp(e), vp(z), vp(w), 2, vp(spec), None, vp(iters), C.byref(n), C.byref(fin), None)
    assert n.value == 1 and (iters[8:] == -7.25).all() and iters.view(capi.PG_LM_ITER)[0]["accepted"] == 1


# ---- 2. the definition ---------------------------------------------------------------------------------------------------------------
def restatement_cases(capi):
    """name -> (poses, fixed, ij, z, w, spec, robust)."""
    out = {}
    s64, ij64, z64, w64, _ = lc.ring_a(64, 0.03)
    out["ring_a_tri"] = (s64, None, ij64, z64, w64, capi.pg_lm_spec(8, 40, precond="tri", tol=1e-8), None)
    out["ring_a_jacobi_dcs_all"] = (s64, None, ij64, z64, w64, capi.pg_lm_spec(4, 60, kind="dcs", phi=50.0, lambda0=10.0, tol=1e-8), None)
    sb, ijb, zb, wb, _, rb = lc.graph_b()
    for kind in ("dcs", "gm"):
        out["graph_b_%s" % kind] = (sb, None, ijb, zb, wb, capi.pg_lm_spec(5, 30, precond="tri", kind=kind, tol=1e-8), rb)
    out["graph_b_none"] = (sb, None, ijb, zb, wb, capi.pg_lm_spec(3, 30, precond="tri", tol=1e-8), rb)
    out["graph_b_every_second"] = (sb, None, ijb, zb, wb, capi.pg_lm_spec(3, 30, precond="tri", kind="gm", phi=0.5, tol=1e-8), np.arange(ijb.shape[0]) % 2 == 0)
    p, ij, z, w = lc.one_edge(0, phi=0.1)
    out["c_equals_phi"] = (p, None, ij, z, w, capi.pg_lm_spec(2, 5, kind="dcs", phi=0.1), None)
    for ulps in (-1, 1):
        p, ij, z, w = lc.one_edge(ulps)
        out["c_beside_phi_%+d" % ulps] = (p, None, ij, z, w, capi.pg_lm_spec(2, 5, kind="dcs"), None)
    exact = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
    out["at_the_minimum"] = (exact, None, np.array([[0, 1]], np.int32), np.array([[1.0, 0.0, 0.0]]), np.array([[4.0, 4.0, 4.0]]), capi.pg_lm_spec(3, 5), None)
    p, ij, z, w = lc.noisy_ring(40)
    out["pinned_and_ftol"] = (p, None, ij, z, w, capi.pg_lm_spec(6, 30, precond="tri", lambda0=4.0, lambda_min=1.0, lambda_max=8.0, up=4.0, down=0.5, ftol=1e-3), None)
    fx = np.zeros(40, np.uint8); fx[[0, 17]] = 1
    out["two_fixed_no_edges"] = (p, fx, np.zeros((0, 2), np.int32), np.zeros((0, 3)), np.zeros((0, 3)), capi.pg_lm_spec(2, 5), None)
    return out


CASE_NAMES = ("ring_a_tri", "ring_a_jacobi_dcs_all", "graph_b_dcs", "graph_b_gm", "graph_b_none", "graph_b_every_second", "c_equals_phi", "c_beside_phi_-1",
              "c_beside_phi_+1", "at_the_minimum", "pinned_and_ftol", "two_fixed_no_edges")


@pytest.mark.parametrize("name", CASE_NAMES)
def test_hook_equals_restatement(capi, name):
    cases = restatement_cases(capi)
    assert sorted(cases) == sorted(CASE_NAMES)
    _, it, F, f = lc.same_as_hook(capi, *cases[name])
    if name == "at_the_minimum":                                           # F_trial == F is a rejection
        assert it["accepted"].tolist() == [0, 0, 0] and F == 0.0
    if name == "c_equals_phi":
        assert f[0] == 1.0 and it[0]["F"] == D(0.1)
    if name.startswith("c_beside_phi"):
        assert it[0]["accepted"] == 1 and abs(it[0]["F"] - 1.0) < 1e-15 and it[0]["F"] != 1.0   # one step solves it: f is the minimum's, 1


# the case each wrong copy of a rule must fail
WRONG_CASES = (("lt", "c_equals_phi"), ("accept_le", "at_the_minimum"), ("lambda_early", "ring_a_tri"), ("F_weff", "graph_b_dcs"), ("s", "graph_b_dcs"),
               ("s", "graph_b_gm"))


@pytest.mark.parametrize("wrong,name", WRONG_CASES)
def test_wrong_copies_fail(capi, wrong, name):
    assert not lc.same_as_hook(capi, *restatement_cases(capi)[name], wrong=wrong)


@pytest.mark.parametrize("precond", ["jacobi", "tri"])
def test_none_with_lambda_zero_is_gauss_newton(capi, precond):
    """The definition's consequence: kind NONE, lambda0 = lambda_min = 0, every attempt accepted."""
    for poses, ij, z, w in (lc.noisy_ring(40), lc.noisy_ring(257), A.tiny_graph(5, 6, list((k, k + 1) for k in range(5)) + [(5, 0), (2, 4)])):
        n_cg = 3 * poses.shape[0]
        old = (capi.debug_pg_relax_tri if precond == "tri" else capi.debug_pg_relax)(poses, None, ij, z, w, capi.pg_spec(3, n_cg, lam=0.0, tol=1e-8))
        p, it, F, f = capi.debug_pg_relax_lm(poses, None, ij, z, w, capi.pg_lm_spec(3, n_cg, precond=precond, lambda0=0.0, lambda_min=0.0, tol=1e-8))
        assert it["accepted"].tolist() == [1, 1, 1] and (it["lambda"] == 0.0).all()
        assert np.array_equal(p, old[0]) and F == old[2] and (f == 1.0).all()
        assert all(np.array_equal(it[n], old[1][n]) for n in ("rz0", "rz", "cg_iters", "stopped")) and np.array_equal(it["F"], old[1]["chi2"])


# ---- 3. what the unit is for -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precond", ["jacobi", "tri"])
@pytest.mark.parametrize("N,bias", lc.RING_A)
def test_ring_a_damped(capi, N, bias, precond):
    """Plain Gauss-Newton raises chi2 at its first step; the damped run never raises F and ends at the truth."""
    start, ij, z, w, true = lc.ring_a(N, bias)
    gn = (capi.debug_pg_relax_tri if precond == "tri" else capi.debug_pg_relax)(start, None, ij, z, w, capi.pg_spec(2, 4 * N, tol=1e-8))[1]
    assert gn[1]["chi2"] > gn[0]["chi2"], gn["chi2"]
    sp = capi.pg_lm_spec(40, 4 * N, precond=precond, lambda0=1e-3, up=10.0, down=0.1, tol=1e-8)
    p, it, F, _ = capi.debug_pg_relax_lm(start, None, ij, z, w, sp)
    e_xy, e_th = lc.pose_error(p, true)
    print("ring A N = %d, %s: Gauss-Newton chi2 %.6g -> %.6g; LM F %.6g -> %.3g in %d attempts (%d rejected), largest lambda %g, error %.3g m %.3g rad" %
          (N, precond, gn[0]["chi2"], gn[1]["chi2"], it[0]["F"], F, len(it), int((it["accepted"] == 0).sum()), it["lambda"].max(), e_xy, e_th))
    assert (np.diff(it["F"]) <= 0).all() and F <= it[-1]["F"]
    assert (it["accepted"] == 0).any() or (it["lambda"] > 1e-3).any()
    assert e_xy <= 1e-6 and e_th <= 1e-6


@pytest.mark.parametrize("precond", ["jacobi", "tri"])
def test_graph_b_robust(capi, precond):
    """One false loop edge: the quadratic relaxation ends more than a metre from the truth, DCS within a millimetre."""
    start, ij, z, w, true, rb = lc.graph_b()
    relax = capi.debug_pg_relax_tri if precond == "tri" else capi.debug_pg_relax
    e_gn = lc.pose_error(relax(start, None, ij, z, w, capi.pg_spec(10, 256, tol=1e-8))[0], true)[0]
    clean = lc.graph_b(false_edge=False)
    e_clean = lc.pose_error(relax(clean[0], None, clean[1], clean[2], clean[3], capi.pg_spec(10, 256, tol=1e-8))[0], true)[0]
    sp = capi.pg_lm_spec(40, 256, precond=precond, kind="dcs", phi=1.0, lambda0=1e-3, up=10.0, down=0.1, tol=1e-8)
    p, it, F, f = capi.debug_pg_relax_lm(start, None, ij, z, w, sp, rb)
    e_dcs = lc.pose_error(p, true)[0]
    print("graph B, %s: quadratic %.3f m (without the false edge %.3g m); DCS %.3g m, F %.4g, f of the loops %s" % (precond, e_gn, e_clean, e_dcs, F, f[-3:].tolist()))
    assert e_gn > 1.0 and e_clean < 1e-9
    assert e_dcs <= 1e-3
    assert f[-1] < 1e-2 and f[-2] == 1.0 and f[-3] == 1.0 and (f[:63] == 1.0).all()
    assert (np.diff(it["F"]) <= 0).all()
