"""The K2 edge cases (tests/k2_cases.py) on the CPU: every case through the C oracle and through np_oracle, pixel for pixel and
count for count after every step; the kernel's rule -- per pixel the rays that draw it by the two closed forms, found through the
slope window, the octants' ray selection and the lone-ray shortcut, blended in ray-index order, counted where no hit is inside a V --
restated in NumPy and equal to the oracles on every case; wrong copies of the rule, each failing named cases; the property each
case claims, from its own geometry; and three bounds of the kernel's comments by enumeration: the lone-ray step, the binary64
minor step and the arc margin a drawing ray needs.  Every comparison is == on the whole uint16 map."""
import numpy as np
import pytest

import k2_cases as kc

F = np.float32
SMALL = [c.name for c in kc.CASES if "big" not in c.claims]
BIGS = [c.name for c in kc.CASES if "big" in c.claims]


def blend(pix, v, alpha):
    return (((256 - alpha) * pix + alpha * v) >> 8) & 0xFFFF             # :431 (bits 8 .. 23 of the wrapped int are those of the exact one)


def pixel_octants(dx, dy):
    """kc.pixel_octant on arrays."""
    adx, ady = np.abs(dx), np.abs(dy)
    ox = np.where(dx > 0, np.where(dy < 0, 0, 1), np.where(dy > 0, 4, 5))
    oy = np.where(dy > 0, np.where(dx > 0, 2, 3), np.where(dx < 0, 6, 7))
    od = np.where(dx > 0, np.where(dy > 0, 2, 0), np.where(dy > 0, 4, 6))
    return np.where(adx > ady, ox, np.where(ady > adx, oy, od))


# ---- the kernel's rule -------------------------------------------------------------------------------------------------------------
def rule_step(size, pix, st, variant=None, stats=None):
    """One step of k2_pixels restated on the flat uint16 map `pix` (in place); returns the blended pixel count.  variant: None or the
    name of a wrong copy.  stats: a dict that collects what the rule's shortcuts left out (all zero for the right rule)."""
    xy, pxcs, hw, alpha = st
    geo = kc.geometry(size, st)
    if geo is None:
        return 0
    R = len(xy)
    t = kc.touches(size, geo, float_incv=variant == "float_incv")
    total = len(t)
    if total == 0:
        return 0
    zone, rB = kc.zone_radius(R), kc.rb_radius(R)
    keep = np.ones(total, bool)
    # the slope window: a ray is found on a pixel only if its bucket lies in the pixel's range (rs_range), in the ray's own class
    x, b = t["x"], t["b"]
    with np.errstate(all="ignore"):
        ra = (F(1.0) / np.maximum(x, 1).astype(np.float32)).astype(np.float32)
        lo = kc.rs_bucket((b.astype(np.float32) - F(0.5)) * ra - F(4.0e-6))
        hi = kc.rs_bucket((b.astype(np.float32) + F(0.5)) * ra + F(4.0e-6))
    narrow = 1 if variant == "narrow_window" else 0
    bk = kc.ray_bucket(geo)[t["ray"]]
    keep &= (x == 0) | ((bk >= lo + narrow) & (bk <= hi - narrow))
    if stats is not None:
        stats["window"] = stats.get("window", 0) + int((~keep).sum())
    order = np.lexsort((t["ray"], t["ptr"]))
    t, keep = t[order], keep[order]
    first = np.r_[True, t["ptr"][1:] != t["ptr"][:-1]]
    gid = np.cumsum(first) - 1
    starts = np.flatnonzero(first)
    # the octants' selection (arcs): a pixel from rB outwards is drawn with the rays selected for its octant -- a zone pixel's own
    # octant, a far pixel's owner ray's (the lowest index that draws it)
    if kc.arcs_on(size, st):
        M = np.stack([kc.arc_member(xy, pxcs, o, rB, 1.0 if variant == "margin_1" else 8.0) for o in range(8)], 1)
        x1, y1 = int(geo["x1"][0]), int(geo["y1"][0])
        py, px = np.divmod(t["ptr"], size)
        po = pixel_octants(px - x1, py - y1)
        owner_oct = kc.ray_octant(geo)[t["ray"][starts]][gid]
        octs = np.where(t["x"] < zone, po, owner_oct)
        sel = (t["x"] < rB) | M[t["ray"], octs]
        if stats is not None:
            stats["arcs"] = stats.get("arcs", 0) + int((keep & ~sel).sum())
        keep &= sel
    # the lone-ray shortcut: from step xalone on a far, non-diagonal step is blended without a look at the other rays
    alone = np.zeros(total, bool)
    if R <= kc.LDS_RAYS:
        xa = kc.xalone(geo, 0 if variant == "xalone_no_plus_2" else 2)[t["ray"]]
        alone = (t["x"] >= zone) & (t["x"] >= xa) & (xa < 2047)
        if variant != "xalone_on_diagonals":
            alone &= np.abs(t["b"]) != t["x"]
    t, alone = t[keep], alone[keep]
    first = np.r_[True, t["ptr"][1:] != t["ptr"][:-1]]
    starts = np.flatnonzero(first)
    ends = np.r_[starts[1:], len(t)]
    single = ends - starts == 1
    s = starts[single]
    pix[t["ptr"][s]] = blend(pix[t["ptr"][s]].astype(np.int64), t["value"][s], alpha).astype(np.uint16)
    if variant == "by_angle":
        ang = np.arctan2(np.asarray(xy, np.float64)[:, 1], np.asarray(xy, np.float64)[:, 0])
    for a, e in zip(starts[~single], ends[~single]):
        g = t[a:e]
        p = int(g["ptr"][0])
        v = int(pix[p])
        if alone[a:e].any():                                            # (never, if the bound holds: the pixel would lose hits)
            if stats is not None:
                stats["alone"] = stats.get("alone", 0) + 1
            pix[p] = blend(v, int(g["value"][np.flatnonzero(alone[a:e])[0]]), alpha)
            continue
        vals = g["value"]
        if variant == "by_angle":
            vals = vals[np.lexsort((g["ray"], ang[g["ray"]]))]
        if variant == "maxhit_3" and len(g) == kc.MAXHIT and g["x"][0] >= zone and abs(int(g["b"][0])) != int(g["x"][0]):
            vals = vals[:kc.MAXHIT - 1]
        if not g["inv"].any() or variant == "count_mixed":              # the counting shortcut: one value, as many times, to its fixed point
            for _ in range(len(vals)):
                nv = blend(v, kc.NO_OBSTACLE, alpha)
                if nv == v:
                    break
                v = nv
        else:
            for vv in vals:
                v = blend(v, int(vv), alpha)
        pix[p] = v
    return total


VARIANTS = ("by_angle", "count_mixed", "narrow_window", "xalone_no_plus_2", "xalone_on_diagonals", "margin_1", "maxhit_3", "float_incv")


def run_rule(built, variant=None, stats=None):
    pix = np.full(built.size * built.size, kc.START, np.uint16) if built.start is None else built.start.copy()
    counts = [rule_step(built.size, pix, st, variant, stats) for st in built.steps]
    return pix, counts


def run_oracle(built, mod):
    pix = np.full(built.size * built.size, kc.START, np.uint16) if built.start is None else built.start.copy()
    counts = [mod.update_holemap_pxcs(pix, built.size, 1.0, *st) for st in built.steps]
    return pix, counts


_ORACLE = {}


def oracle_of(name, oc):
    """The C oracle's result of a case, computed once."""
    if name not in _ORACLE:
        _ORACLE[name] = run_oracle(kc.by_name(name).build(), oc)
    return _ORACLE[name]


def same(got, ref, what):
    got, ref = np.asarray(got).ravel(), np.asarray(ref).ravel()
    bad = np.flatnonzero(got != ref)
    assert bad.size == 0, (what, bad.size, bad[:8], got[bad[:8]], ref[bad[:8]])


# ---- both oracles, the rule, the claims ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL)
def test_oracles_agree(oc, npo, name):
    ref, n = oracle_of(name, oc)
    got, m = run_oracle(kc.by_name(name).build(), npo)
    assert n == m
    same(got, ref, name)


@pytest.mark.parametrize("name", SMALL + BIGS)
def test_rule_equals_oracle(oc, name):
    ref, n = oracle_of(name, oc)
    stats = {}
    got, m = run_rule(kc.by_name(name).build(), None, stats)
    assert n == m
    same(got, ref, name)
    assert not any(stats.values()), stats                               # the window, the selection and the lone-ray step left no hit out
    if name in BIGS:
        _ORACLE.pop(name)                                               # (half a gigabyte)


@pytest.mark.parametrize("name", BIGS)
def test_oracles_agree_big(oc, npo, name):
    """The 16 384^2 cases through np_oracle on the touched pixels' bounding rows only would not be the whole map: both whole maps."""
    ref, n = oracle_of(name, oc)
    got, m = run_oracle(kc.by_name(name).build(), npo)
    assert n == m
    assert np.array_equal(got, ref)
    _ORACLE.pop(name)


def hits_of(size, geo, dx, dy):
    t = kc.touches(size, geo)
    p = (int(geo["y1"][0]) + dy) * size + int(geo["x1"][0]) + dx
    return t[t["ptr"] == p]


def check_claims(c):
    b = c.build()
    st = b.steps[0]
    xy = st[0]
    geo = kc.geometry(b.size, st)
    R = len(xy)
    zone, rB = kc.zone_radius(R), kc.rb_radius(R)
    ok = geo["valid"] == 1
    cl = set(c.claims)
    if "ray_count" in cl:
        assert R == int(c.name.split("_")[1]) and ok.all()
    if "rim" in cl and R >= 63:
        octs = kc.ray_octant(geo)
        for r in kc.rim_radii(R)[:6 if R >= 100 else 3]:                # (below 100 rays the scan holds the zone's rim only; rB is 1 or 2 there)
            if r >= 4:                                                  # (shorter rays have no slope inside every octant)
                assert set(octs[ok & (geo["dxc"] == r)]) == set(range(8)), (r, "every octant has a ray that ends at this radius")
            # ... on the axes and on the diagonals
            assert (ok & (geo["dxc"] == r) & (geo["dyc"] == 0)).sum() >= 4 and (ok & (geo["dxc"] == r) & (geo["dyc"] == r)).sum() >= 4, r
    if "central_marked" in cl:
        t = kc.touches(b.size, geo)
        inv = set(t["ptr"][(t["inv"] == 1) & (t["x"] < rB)])
        assert rB == 12 and (geo["lim2"][ok] < 0).all() and t["inv"].all() and len(inv) > 200     # every central pixel a ray touches is marked
    if "adjacent_octant" in cl:
        t = kc.touches(b.size, geo)
        t = t[(t["x"] > 0) & (t["x"] < rB)]
        py, px = np.divmod(t["ptr"], b.size)
        d8 = (pixel_octants(px - 32, py - 32) - kc.ray_octant(geo)[t["ray"]]) & 7
        assert set(d8) == {0, 1}                                        # its own octant or the NEXT one (axis and diagonal pixels belong to the octant that begins there): the one before never occurs
    if "mixq" in cl:
        t = kc.touches(b.size, geo)
        t = t[(t["inv"] == 1) & (t["x"] >= rB) & (t["x"] < kc.ZONE_MIN)]
        py, px = np.divmod(np.unique(t["ptr"]), b.size)
        n = np.bincount(pixel_octants(px - 128, py - 128), minlength=8)
        assert n[1] > kc.MIXQ and 0 < n[5] < kc.MIXQ, n
    if "mixed_47_48" in cl:
        assert zone > kc.ZONE_MIN
        for r in (47, 48):
            for ux, uy in kc.DIRS8:
                h = hits_of(b.size, geo, ux * r, uy * r)
                assert len(h) >= 10 and h["inv"].sum() == 1
                k = int(np.flatnonzero(h["inv"])[0])
                assert {"lo": k == 0, "mid": 0 < k < len(h) - 1, "hi": k == len(h) - 1}[c.name.rsplit("_", 1)[1]]
    if "wave_cand" in cl:
        n = int(c.name.split("_")[1])
        for dx in (29, 30, 31, 32):
            h = hits_of(b.size, geo, dx, 0)
            assert len(kc.candidates(geo, dx, 0)) == n and len(h) == n and h["inv"].sum() == 1 and rB <= dx < zone
        assert (n > kc.WAVE_CAND) == (c.name == "cand_65")
    if "far_cand" in cl:
        cc, hh = int(c.name[5]), int(c.name[8])
        h = hits_of(b.size, geo, 60, 0)
        assert zone == 48 and len(kc.candidates(geo, 60, 0)) == cc and len(h) == hh and h["inv"].sum() == 1
        k = int(np.flatnonzero(h["inv"])[0])                            # (hits_of lists the hits in ray-index order)
        assert k == {0: 0, 1: hh // 2, 2: hh - 1}[int(c.name[-1])]
    if "pair" in cl or "fan" in cl:
        xa = kc.xalone(geo)
        t = kc.touches(b.size, geo)
        t = t[(np.abs(t["b"]) != t["x"])]
        u, n = np.unique(t["ptr"], return_counts=True)
        shared = t[np.isin(t["ptr"], u[n > 1])]
        assert (shared["x"] < xa[shared["ray"]]).all()
        if "pair" in cl:
            m = int(c.name.split("_")[2][1:])
            assert len(set(kc.ray_class(geo))) == 1 and len(shared) > 0     # every pair shares pixels next to the robot at least
            assert (xa == 2047).all() == (m == 0)                       # a duplicate slope is never alone
            if 0 < m <= 2:
                assert shared["x"].max() >= zone and (shared["inv"] == 1).any() and (shared["inv"] == 0).any()
    if "diagonal" in cl:
        xa = kc.xalone(geo)
        t = kc.touches(b.size, geo)
        dg = t[(np.abs(t["b"]) == t["x"]) & (t["x"] >= xa[t["ray"]])]
        u, n = np.unique(dg["ptr"], return_counts=True)
        assert (n > 1).any() and len(set(kc.ray_class(geo)[dg["ray"]])) == 4      # (both classes of both quadrants)
    if "bucket_gap" in cl:
        k = int(c.name.split("_")[2][1:])
        bk, xa = kc.ray_bucket(geo), kc.xalone(geo)
        assert len(set(kc.ray_class(geo))) == 1 and abs(int(bk[1]) - int(bk[0])) == k
        cap = F(10.0) * (F(2.0) / F(kc.NBUCK))
        capped = kc.xalone_of_gap(cap)
        seen = kc.xalone_of_gap(min(abs(kc.ray_slope(geo)[1] - kc.ray_slope(geo)[0]), cap))     # (a partner in reach but ten buckets or more away changes nothing either)
        assert list(xa) == [seen if k <= kc.ALONE_REACH else capped] * 2 and (k <= kc.ALONE_REACH) == (k in (1, 10, 11))
        t = kc.touches(b.size, geo)
        u, n = np.unique(t["ptr"], return_counts=True)
        sh = t[np.isin(t["ptr"], u[n > 1]) & (t["x"] > 0)]
        assert len(sh) > 0 and len(set(sh["value"])) > 1                # they share pixels, with different values: the order shows
        if k == 1:
            assert sh["x"].max() >= zone                                # ... beyond the zone, where the lone-ray step matters
    if "above_inverse" in cl:
        sl = kc.ray_slope(geo)
        far = largest_shared_offset(int(geo["dxc"][0]), int(geo["dyc"][0]), int(geo["dxc"][1]), int(geo["dyc"][1]))
        assert abs(sl[1] - sl[0]) > F(1.0) / F(100) and zone <= far < 100 and (kc.xalone(geo) <= 102).all()
    if "cutoff" in cl:
        g = abs(kc.ray_slope(geo)[1] - kc.ray_slope(geo)[0])
        assert (g > F(1.0e-6)) == (c.name == "cutoff_above") and 0.99e-6 < g < 1.01e-6 and (kc.xalone(geo) == 2047).all()
    if "bucket_ends" in cl:
        bk, rc = kc.ray_bucket(geo), kc.ray_class(geo)
        ends = [set(bk[rc == k]) & {0, kc.NBUCK - 1} for k in range(4)]
        assert all(ends) and sum(len(e) == 2 for e in ends) >= 3, ends
        assert ((bk > 0) & (bk <= kc.ALONE_REACH)).any() and ((bk < kc.NBUCK - 1) & (bk >= kc.NBUCK - 1 - kc.ALONE_REACH)).any()   # neighbours inside the clamped window
    if "arc_edge" in cl:
        t = kc.touches(b.size, geo)
        py, px = np.divmod(t["ptr"], b.size)
        po = pixel_octants(px - 256, py - 256)
        u, _ = kc.arc_u(xy, st[1])
        assert rB == 12
        for k in range(8):
            M = kc.arc_member(xy, st[1], k, rB)
            for side in range(2):
                edge = M[k * 12 + side * 5:k * 12 + side * 5 + 5]
                assert edge.any() and not edge.all(), (k, side, edge)   # the five rays step across the margin's edge
            drawn = t[(po == k) & (t["x"] >= rB)]
            assert M[drawn["ray"]].all()                                # a ray that is not selected draws nothing of the octant from rB on
            at_rb = t[(po == k) & (t["x"] == rB)]
            assert (np.floor(u[at_rb["ray"]]).astype(int) % 8 != k).any()      # ... and a ray from outside the octant draws its pixel at offset exactly rB
    if "arc_need" in cl:
        for stp in b.steps:
            i = int(np.flatnonzero((stp[0] == (-31, -29)).all(1))[0])
            need = margin_needed(b.size, stp)
            r = kc.rb_radius(len(stp[0]))
            g = kc.geometry(b.size, stp)
            assert need[i] > 1.0 and kc.arcs_on(b.size, stp) and g["dxc"][i] >= r
            tt = kc.touches(b.size, g)
            tt = tt[(tt["ray"] == i) & (tt["x"] >= r)]
            py, px = np.divmod(tt["ptr"], b.size)
            outside = [not kc.arc_member(stp[0], stp[1], int(k), r, 1.0)[i] for k in pixel_octants(px - 32, py - 63)]
            assert any(outside)                                         # a margin of 1 / rB leaves the ray out of an octant it draws in
    if "plus_2" in cl:
        sl = kc.ray_slope(geo)
        far = largest_shared_offset(int(geo["dxc"][0]), int(geo["dyc"][0]), int(geo["dxc"][1]), int(geo["dyc"][1]))
        assert list(geo["dxc"]) == [510, 365] and list(geo["dyc"]) == [11, 11] and far >= zone
        assert kc.xalone_of_gap(abs(sl[1] - sl[0]), 0) <= far < kc.xalone_of_gap(abs(sl[1] - sl[0]), 2)
    if "xalone_field" in cl:
        sl = kc.ray_slope(geo)
        assert geo["dxc"][0] == 2047 and kc.xalone_of_gap(abs(sl[1] - sl[0])) == 2047 and int(F(F(1.0) / F(abs(sl[1] - sl[0]) - F(4e-7))) * F(1.0001)) + 2 > 2047
    if "own_cap" in cl:
        n = int(c.name.split("_")[1])
        assert int((ok & (kc.ray_octant(geo) == 1) & (geo["dxc"] >= zone)).sum()) == n and (n <= kc.OWN_CAP) == (c.name == "own_848")
    if "empty_octants" in cl:
        assert set(kc.ray_octant(geo)[ok]) == {1, 6}
    if "hole_width" in cl:
        assert kc.arcs_on(b.size, st) == (c.name == "arc_hole_below")
    if "sane" in cl:
        assert [kc.arcs_on(b.size, s) for s in b.steps] == [True, False, False]
        u, sane = kc.arc_u(xy, st[1])
        assert sane[0] and not sane[1] and sane[2] and not sane[3]
    if "derrorv" in cl and c.name != "v_derrorv_small":
        dv = int(c.name.split("_")[2])
        assert dv in set(geo["d"][ok]) and ok.all()                     # (towards negative coordinates the truncation makes it dv - 1)
    if c.name == "v_derrorv_small":
        g2 = kc.geometry(b.size, b.steps[1])
        assert {-1, 0, 1} <= set(geo["lim2"][ok]) | set(g2["lim2"]) and 1 in set(geo["d"][ok]) and 2 in set(g2["d"])
    if "lim1" in cl:
        e = geo["lim1"][ok] - geo["dxc"][ok]
        assert (e < 0).any() and (e == 0).any() and (e > 0).any()
    if "ties" in cl:
        e = geo["dx"][ok] - np.abs(np.where(geo["major_x"][ok] == 1, geo["y2"][ok] - geo["y1"][ok], geo["x2"][ok] - geo["x1"][ok]))
        assert {0, 1} <= set(e)
    if "arc_margin" in cl or "class_border" in cl:
        # rays the clip and the truncations moved: the float direction's octant is not the integer ray's
        u, _ = kc.arc_u(xy, st[1])
        assert (np.floor(u[ok]).astype(int) % 8 != kc.ray_octant(geo)[ok]).any()
    if "division" in cl:
        for stp in b.steps:
            g = kc.geometry(b.size, stp)
            res = kc.division_residues(g)
            assert (g["valid"] == 1).all() and set(g["dxc"]) == {kc.BIG - 1, kc.BIG - 2}
            assert all(res) and set().union(*res) == {"on", "below", "above"}      # every ray comes within 1 of a multiple of 2 dxc
            assert all(r <= {"below", "above"} for r, q in zip(res, g) if q["dxc"] % 2) and any("on" in r for r in res)
            assert set(g["major_x"]) == {0, 1}
        assert kc.arcs_on(b.size, b.steps[0]) and not kc.arcs_on(b.size, b.steps[3])   # (from the corner (0, 0) the pose is within the arcs' 16 000; the rays' end points are not: each is selected everywhere)
    if "counting" in cl:
        t = kc.touches(b.size, geo)
        assert not t["inv"][(t["x"] >= rB) & (t["x"] < 40)].any()
        for n, (px, py) in kc.COUNTS:
            assert len(hits_of(b.size, geo, px // 2, py // 2)) == n


@pytest.mark.parametrize("name", [c.name for c in kc.CASES])
def test_claims(name):
    check_claims(kc.by_name(name))


def test_every_group_and_constant_has_cases():
    tags = {t for c in kc.CASES for t in c.claims}
    assert {"ray_count", "central", "counting", "mixed", "mixq", "candidates", "wave_cand", "far_cand", "lone", "pair", "fan", "diagonal",
            "xalone_field", "arcs", "arc_margin", "arc_edge", "arc_need", "bucket_gap", "cutoff", "bucket_ends", "above_inverse", "own_cap", "hole_width", "sane", "vprofile", "division"} <= tags
    assert {kc.LDS_RAYS, kc.LDS_RAYS + 1, 1024, 1025, 90, 91, 383, 384, 1536, 1544} <= set(kc.RAY_COUNTS)
    names = {c.name for c in kc.CASES}
    for const, (one_side, other_side) in SIDES.items():
        assert one_side in names and other_side in names, const


# the constants of the issue's list: a named case on each side (each case's claim, checked in test_claims, says which side it is on)
SIDES = {
    "K2_MIXQ 192": ("mixq_overflow", "mixed_47_48_mid"),               # (one case: octant 1 above, octant 5 below) / a handful queued
    "ordered draw from radius 48": ("mixed_47_48_lo", "mixed_47_48_hi"),     # (each case: radius 47 and 48)
    "k2_arc_member margin": ("arc_edge", "arc_need"),
    "lone-ray reach, 11 buckets": ("gap_c0_b11_fwd", "gap_c0_b12_fwd"),
    "lone-ray + 2": ("pair_plus_2", "gap_above_inverse"),
    "lone-ray cut-off 1e-6": ("cutoff_below", "cutoff_above"),
    "xalone's 11 bits": ("pair_dxc_2047", "pair_c0_m1_fwd"),
    "K2_MAXHIT 4": ("far_c4_h4_o1", "far_c5_h5_o1"),
    "64 candidates": ("cand_64", "cand_65"),
    "K2_OWN_CAP 848": ("own_848", "own_849"),
    "K2_LDS_RAYS 2048": ("rays_2048", "rays_2049"),
    "binary64 minor step, maps up to 16 384": ("division_16384", "borders_300"),
    "hw_px < 8000": ("arc_hole_below", "arc_hole_at"),
    "arcs' 16 000": ("arc_sane_16384", "arc_hole_negative"),
}


def test_blend_fixed_point_both_ways():
    """The counting shortcut stops at the blend's fixed point: with the cases' counts and qualities there are pixels whose blend
    converges before the count is used up and pixels where it never does -- the literal loop (the oracles) is matched in both."""
    early, never = 0, 0
    for q in kc.QUALITIES:
        for s0 in kc.START_VALUES:
            for n, _ in kc.COUNTS:
                v, k = s0, 0
                while k < n and blend(v, kc.NO_OBSTACLE, q) != v:
                    v = blend(v, kc.NO_OBSTACLE, q); k += 1
                early += k < n
                never += k == n
    assert early > 20 and never > 20


def margin_needed(size, st):
    """Per ray the arc margin it needs, as a multiple of 1 / rB: the largest, over its steps x >= 1, of (the distance in octants from
    its float direction u to the octant of the step's pixel - 0.02) * min(x, 48) -- the pixel is drawn by that octant's workgroups
    for every rB <= x, and those select the ray if the distance is at most 1/2 + margin / rB + 0.02 from the octant's centre."""
    xy, pxcs = st[0], st[1]
    geo = kc.geometry(size, st)
    u, _ = kc.arc_u(xy, pxcs)
    out = np.full(len(xy), -1.0)
    for i in np.flatnonzero(geo["valid"] & (geo["dxc"] > 0)):
        r = geo[i]
        x = np.arange(1, int(r["dxc"]) + 1)
        a, b = r["smaj"] * x, r["smin"] * kc.minor_offset(x, int(r["dxc"]), int(r["dyc"]))
        k = pixel_octants(a, b) if r["major_x"] else pixel_octants(b, a)
        d = float(u[i]) - (k + 0.5)
        d = d - 8 * np.rint(d / 8)
        out[i] = ((np.abs(d) - 0.5 - 0.02) * np.minimum(x, kc.ZONE_MIN)).max()
    return out


def test_arc_margin_needed_by_enumeration():
    """Every integer end point within 40 pixels, from robots 0, 1, 12 and 31 pixels from the east border and 0 and 2 from the north
    one of a 64^2 map (the clip cuts the rays short and moves their slopes), hole widths 2, 9 and 3000: the margin a ray needs stays
    below the kernel's 8 / rB.  The largest found is 1.42 / rB (the case arc_need): no case in THIS enumeration separates a margin of
    4 / rB from 8 / rB, while 1 / rB is separated (the wrong copy margin_1).  A finite sample, not a proof: rotated poses (s != 0),
    larger maps and rays clipped from far away are not covered, and the kernel's own bound is 6.1 / dxc."""
    g = np.arange(-40, 41)
    P = np.array([(x, y) for x in g for y in g if (x, y) != (0, 0)], np.float32)
    worst = 0.0
    for hw in (2.0, 9.0, 3000.0):
        for bx in (0, 1, 12, 31):
            for by in (0, 2):
                worst = max(worst, margin_needed(64, (P, kc.pxcs_at(63 - bx, 63 - by), hw, 50)).max())
    assert 1.0 < worst < 4.0 < 8.0, worst


# ---- wrong copies --------------------------------------------------------------------------------------------------------------------
CATCHES = {
    "by_angle": ["central_inside_v_shuffled", "fan_c0_shuffled", "pair_c0_m1_rev"],
    "count_mixed": ["mixed_47_48_mid", "cand_64", "central_inside_v"],
    "narrow_window": ["mixq_overflow", "rays_1024", "fan_c2_fwd"],
    "xalone_no_plus_2": ["pair_plus_2"],
    "xalone_on_diagonals": ["diagonal_shared_q0", "diagonal_shared_q2", "borders_300"],
    "margin_1": ["arc_need"],
    "maxhit_3": ["far_c4_h4_o0", "far_c4_h4_o2"],
    "float_incv": ["v_derrorv_32751", "central_inside_v", "pair_c0_m1_fwd"],
}


@pytest.mark.parametrize("variant", VARIANTS)
def test_wrong_copy_is_caught(oc, variant):
    """Each wrong copy of the rule differs from the oracle on every case named for it."""
    for name in CATCHES[variant]:
        ref, _ = oracle_of(name, oc)
        got, _ = run_rule(kc.by_name(name).build(), variant)
        assert (got != ref).any(), (variant, name)


# ---- the two bounds, by enumeration ----------------------------------------------------------------------------------------------
def largest_shared_offset(dxc1, dyc1, dxc2, dyc2):
    """The largest major offset at which two rays of one class (signed minor lengths) share a non-diagonal pixel; 0: none."""
    n = min(dxc1, dxc2)
    x = np.arange(1, n + 1, dtype=np.int64)
    m1 = np.sign(dyc1) * kc.minor_offset(x, dxc1, abs(dyc1))
    m2 = np.sign(dyc2) * kc.minor_offset(x, dxc2, abs(dyc2))
    s = np.flatnonzero((m1 == m2) & (np.abs(m1) != x))
    return int(x[s[-1]]) if s.size else 0


def pair_bound_holds(dxc1, dyc1, dxc2, dyc2):
    s1, s2 = F(dyc1) / F(dxc1), F(dyc2) / F(dxc2)
    g = F(abs(F(s1 - s2)))
    if g == 0:
        return True                                                     # (the same slope: never alone)
    g = min(g, F(10.0) * (F(2.0) / F(kc.NBUCK)))
    far = largest_shared_offset(dxc1, dyc1, dxc2, dyc2)
    return all(kc.xalone_of_gap(g, 2, u) == 2047 or far < kc.xalone_of_gap(g, 2, u) for u in (-1, 0, 1))      # (2047: the field's 'never alone')


def test_lone_ray_bound_by_enumeration():
    for dxc1 in range(48, 97):
        for dxc2 in range(dxc1, 97):
            for dyc1 in range(0, dxc1 + 1, 3):
                for dyc2 in (dyc1 * dxc2 // dxc1 + e for e in (-2, -1, 0, 1, 2)):
                    if -dxc2 <= dyc2 <= dxc2:
                        assert pair_bound_holds(dxc1, dyc1, dxc2, dyc2), (dxc1, dyc1, dxc2, dyc2)
    for c in kc.CASES:
        if "fan" in c.claims:
            b = c.build()
            geo = kc.geometry(b.size, b.steps[0])
            sd = geo["smin"] * geo["dyc"]
            for i in range(len(geo)):
                for j in range(i + 1, len(geo)):
                    assert pair_bound_holds(int(geo["dxc"][i]), int(sd[i]), int(geo["dxc"][j]), int(sd[j])), (c.name, i, j)
    rng = np.random.default_rng(2)
    for _ in range(20000):
        dxc1, dxc2 = (int(v) for v in rng.integers(48, 16384, 2))
        dyc1 = int(rng.integers(-dxc1, dxc1 + 1))
        dyc2 = int(np.clip(round(dyc1 * dxc2 / dxc1) + int(rng.integers(-3, 4)), -dxc2, dxc2))
        assert pair_bound_holds(dxc1, dyc1, dxc2, dyc2), (dxc1, dyc1, dxc2, dyc2)


def test_minor_step_binary64_by_enumeration():
    """ceil(N rc - 2^-18) in binary64, rc the correctly rounded 1 / (2 dxc), is the integer ceiling of N / (2 dxc): every dxc of maps
    up to 16 384, N = 2 dyc x - dxc at the extremes of its range and within 1 of every multiple of 2 dxc it can reach."""
    for dxc in range(1, 16385):
        D = 2 * dxc
        rc = 1.0 / float(D)
        k = np.arange(0, dxc + 1, dtype=np.int64) * D                    # N < 2 dxc^2: the multiples 0 .. dxc
        N = np.concatenate([k - 1, k, k + 1, [-dxc, 2 * dxc * dxc - dxc]])
        N = N[(N >= -dxc) & (N <= 2 * dxc * dxc - dxc)]
        got = np.ceil(N.astype(np.float64) * rc - 2.0 ** -18).astype(np.int64)
        assert np.array_equal(got, -((-N) // D)), dxc
