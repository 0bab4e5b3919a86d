"""The K3 edge cases (tests/k3_cases.py) on the CPU: every case through the C oracle's literal loop and through np_oracle's, and
the property each case claims to exercise, computed from the case's own integers -- a case cannot silently stop testing what it
was built for.  At the end the closed form of the walk (what the device computes per lane, restated here in Python) against the
literal loop on every ray of every case, and two deliberately wrong copies of it that the chunk-edge and tie cases must catch."""
import numpy as np
import pytest

import k3_cases as kc

INT_MIN = kc.INT_MIN


@pytest.fixture(scope="module")
def det(oc):
    oc.set_trig_mode(oc.TRIG_DET)
    yield oc
    oc.set_trig_mode(oc.TRIG_LIBM)


def _deltas(built):
    return [(abs(ddx), abs(ddy), (ddx > 0) - (ddx < 0), (ddy > 0) - (ddy < 0)) for _, _, _, _, ddx, ddy in kc.geometry(built)
            if ddx != INT_MIN and ddy != INT_MIN]


def _per_ray(built):
    size = built[0]
    return [(g, kc.literal_cells(size, *g[:4])) for g in kc.geometry(built)]


# ---- the claims ----------------------------------------------------------------------------------------------------------------
def claim_octants(built, ref):
    d = _deltas(built)
    octs = {(sx, sy, dx > dy) for dx, dy, sx, sy in d if dx and dy and dx != dy}
    assert len(octs) == 8, octs
    assert {(sx, sy) for dx, dy, sx, sy in d if dx == 0 or dy == 0} >= {(1, 0), (-1, 0), (0, 1), (0, -1)}


def claim_tie(built, ref):
    d = _deltas(built)
    assert {(sx, sy) for dx, dy, sx, sy in d if dx == dy and dx > 0} == {(1, 1), (1, -1), (-1, 1), (-1, -1)}
    assert any(dx == dy + 1 for dx, dy, _, _ in d) and any(dy == dx + 1 for dx, dy, _, _ in d)


def claim_odd_even_major(built, ref):
    assert {max(dx, dy) % 2 for dx, dy, _, _ in _deltas(built)} == {0, 1}


def claim_n_values(built, ref):
    size = built[0]
    want = {n for n in (0, 1, 63, 64, 65, size - 1) if n <= size - 1}
    got = {max(abs(g[4]), abs(g[5])) for g, (_, end) in _per_ray(built) if end is not None}
    assert got == want, (got, want)
    if size >= 66:
        assert {63, 64, 65} <= got                       # the end point is the last lane of a chunk, the first of the next, the second


def claim_last_cell(built, ref):
    size = built[0]
    assert any(end == (size - 1, size - 1) and max(abs(g[4]), abs(g[5])) == size - 1 for g, (_, end) in _per_ray(built))
    if size == 64:
        assert (size - 1) % 64 == 63                     # ... which is then the last lane of the last chunk that reaches the map


def claim_border_outside(built, ref):
    size, start = built[0], built[1]
    rays = _per_ray(built)
    border = [end for _, (_, end) in rays if end is not None and (end[0] in (0, size - 1) or end[1] in (0, size - 1))]
    assert border, "no end point on the last cell inside"
    just, far = 0, 0
    for (x1, y1, x2, y2, _, _), (cr, end) in rays:
        if end is None:
            assert cr, "a ray that leaves the map crosses at least the robot's cell"
            out = max(-x2, x2 - (size - 1), -y2, y2 - (size - 1))
            just += out == 1
            far += out >= 300
    assert just and far
    hits, crossed, _ = kc.trace(built)
    changed = {(int(x), int(y)) for y, x in zip(*np.nonzero(ref != start))}
    assert changed <= set(hits) | crossed                # nothing but end points inside and the in-map prefixes


def claim_idle_wavefronts(built, ref):
    assert (built[2].shape[0] * kc.chunks_per_ray(built[0])) % 4 != 0


def claim_every_cell_twice(built, ref):
    size = built[0]
    hits, _, _ = kc.trace(built)
    assert len(hits) == size * size and set(hits.values()) == {2}
    assert built[1].min() == -128 and built[1].max() == 127


def claim_robot_outside(built, ref):
    assert kc.geometry(built) is None
    assert (ref == built[1]).all()


def claim_width_both_paths(built, ref):
    d = _deltas(built)
    majors = {max(dx, dy) for dx, dy, _, _ in d}
    assert {16383, 16384, 16385, 2 ** 20} <= majors and any(m > 2 ** 30 for m in majors), sorted(majors)
    assert any((dx | dy) < 16384 for dx, dy, _, _ in d) and any((dx | dy) >= 16384 for dx, dy, _, _ in d)
    minors = {min(dx, dy) for dx, dy, _, _ in d}
    assert {0, 200, 8191, 8192, 8193} <= minors


def claim_minor_step_64bit(built, ref):
    n32 = n64 = 0
    for (x1, y1, _, _, ddx, ddy), (cr, end) in _per_ray(built):
        if ddx == INT_MIN or ddy == INT_MIN:
            continue
        dx, dy = abs(ddx), abs(ddy)
        cells = cr + ([end] if end else [])
        minor = [c[1] for c in cells] if dx > dy else [c[0] for c in cells]
        stepped = len(set(minor)) > 1 and 0 < min(dx, dy) < max(dx, dy)          # (not the diagonal: a genuine slope)
        if (dx | dy) >= 16384:
            n64 += stepped
        else:
            n32 += stepped
    assert n64 >= 4 and n32 >= 1, (n32, n64)


def claim_width_32bit_only(built, ref):
    d = _deltas(built)
    assert d and all((dx | dy) < 16384 for dx, dy, _, _ in d)
    assert {max(dx, dy) for dx, dy, _, _ in d} == {16383}


def claim_int_min_delta(built, ref):
    g = kc.geometry(built)
    refused = [r for r in g if r[4] == INT_MIN or r[5] == INT_MIN]
    assert len(refused) >= 8 and len(refused) < len(g)
    hits, crossed, _ = kc.trace(built)
    assert sum(hits.values()) == len(g) - len(refused)   # the sane rays end inside
    assert (ref != built[1]).any()


def claim_int_min_wrapped_delta(built, ref):
    n = 0
    for (x1, y1, x2, y2, ddx, ddy), (cr, end) in _per_ray(built):
        if (x2 == INT_MIN and ddx > 0 and len({c[0] for c in cr}) > 1) or (y2 == INT_MIN and ddy > 0 and len({c[1] for c in cr}) > 1):
            n += 1
    assert n >= 6, n


def claim_saturation(built, ref):
    size, start, _, _, max_hits = built
    hits, crossed, _ = kc.trace(built)
    v = {c: int(start[c[1], c[0]]) for c in hits}
    assert {1, 2, 40, 300} <= set(hits.values())
    assert any(0 < max_hits - v[c] < h for c, h in hits.items()), "no cell got more hits than it had room for"
    assert any(v[c] >= max_hits for c in hits), "no hit on a cell already at or above Max"
    assert any(v[c] == max_hits - 1 for c in hits) and any(v[c] == max_hits for c in hits)
    if max_hits < 127:
        assert any(v[c] == max_hits + 1 for c in hits)
    assert {127, -128, 0, 1, -1} <= set(v.values())
    assert set(hits) & crossed, "no cell is both hit and crossed"
    cv = {int(start[y, x]) for x, y in crossed}
    assert {127, -128, 0} <= cv


def claim_beyond_first_stride(built, ref):
    size = built[0]
    stride = 64 * 16 * kc.CUS_ASSUMED
    assert size * size > stride
    hits, crossed, _ = kc.trace(built)
    assert any(y * size + x >= stride for x, y in hits) and any(y * size + x >= stride for x, y in crossed)
    assert any(y * size + x < stride for x, y in crossed)
    assert sum(ref[c[1], c[0]] != built[1][c[1], c[0]] for c in set(hits) | crossed if c[1] * size + c[0] >= stride) >= 20


CLAIMS = {"octants": claim_octants, "tie": claim_tie, "odd_even_major": claim_odd_even_major, "n_values": claim_n_values,
          "last_cell": claim_last_cell, "border_outside": claim_border_outside, "idle_wavefronts": claim_idle_wavefronts,
          "every_cell_twice": claim_every_cell_twice, "robot_outside": claim_robot_outside, "width_both_paths": claim_width_both_paths,
          "minor_step_64bit": claim_minor_step_64bit, "width_32bit_only": claim_width_32bit_only, "int_min_delta": claim_int_min_delta,
          "int_min_wrapped_delta": claim_int_min_wrapped_delta, "saturation": claim_saturation,
          "beyond_first_stride": claim_beyond_first_stride}


def test_case_names_are_unique_and_claims_known():
    names = [c.name for c in kc.CASES]
    assert len(names) == len(set(names))
    assert all(c.claims and set(c.claims) <= set(CLAIMS) for c in kc.CASES)
    assert set(CLAIMS) == {k for c in kc.CASES for k in c.claims}       # no claim without a case


@pytest.mark.parametrize("name", [c.name for c in kc.CASES])
def test_case(det, npo, name):
    oc = det
    c = kc.by_name(name)
    built = c.build()
    size, start, xy, pxcs, max_hits = built
    assert start.dtype == np.int8 and start.shape == (size, size) and xy.dtype == np.float32 and xy.shape[1] == 2
    assert pxcs[2] == 1.0 and pxcs[3] == 0.0 and pxcs[0] % 1.0 == 0.5 and pxcs[1] % 1.0 == 0.5
    fin = np.isfinite(xy)
    assert (xy[fin] == np.trunc(xy[fin])).all()                        # integer-valued points
    # where px + X is exact, the end cell is (x1 + X, y1 + Y) by construction (the (int) cast truncates towards zero: -0.5 is cell 0)
    def cell(v):
        return v if v >= 0 else v + 1
    g = kc.geometry(built)
    if g is not None:
        for (x1, y1, x2, y2, _, _), (X, Y) in zip(g, xy):
            if np.isfinite(X) and np.isfinite(Y) and abs(X) < 2 ** 22 and abs(Y) < 2 ** 22:
                assert (x2, y2) == (cell(x1 + int(X)), cell(y1 + int(Y)))
    # the riding path gets the same (px, py, c, s) from the pose (x1, y1, 0) on a map of one cell per metre
    pose = np.array([pxcs[0] - 0.5, pxcs[1] - 0.5, 0.0], np.float32)
    assert oc.normalize_angle(0.0) == 0.0 and oc.map_scale(size, float(size)) == 1.0
    assert (oc.pose_to_pxcs(pose, 1.0) == pxcs).all()
    ref = start.copy()
    oc.update_obstaclemap_pxcs(ref, size, xy, pxcs, max_hits)
    ref_np = start.copy()
    npo.update_obstaclemap_pxcs(ref_np, size, xy, pxcs, max_hits)
    assert (ref == ref_np).all()
    ref_pose = start.copy()
    oc.update_obstaclemap(ref_pose, size, 1.0, xy, pose, max_hits)
    assert (ref == ref_pose).all()
    for k in c.claims:
        CLAIMS[k](built, ref)
    # a second update in a row differs from the first on the saturation cases (what "two updates in a row" tests)
    if "saturation" in c.claims:
        ref2 = ref.copy()
        oc.update_obstaclemap_pxcs(ref2, size, xy, pxcs, max_hits)
        assert (ref2 != ref).any()


# ---- the closed form, and wrong copies of it ------------------------------------------------------------------------------
def closed_form_cells(size, x1, y1, x2, y2, form="device"):
    """Iteration i of the walk as the device computes it (k3_walk_iter): i steps along the major axis, max(0, ceil((i * minor -
    major / 2) / major)) along the minor one; the in-map iterations 0 .. size.  form: "device", or a wrong copy --
    "no_half" drops the - major / 2, "floor" rounds down."""
    ddx, ddy = kc._wrap32(x2 - x1), kc._wrap32(y2 - y1)
    if ddx == INT_MIN or ddy == INT_MIN:
        return [], None
    dx, dy = abs(ddx), abs(ddy)
    sx, sy = (ddx > 0) - (ddx < 0), (ddy > 0) - (ddy < 0)
    major, minor, n = max(dx, dy), min(dx, dy), max(dx, dy)
    crossed, end = [], None
    for i in range(0, min(n, size) + 1):
        num = i * minor - (0 if form == "no_half" else major // 2)
        if num <= 0 or major == 0:
            st = 0
        elif form == "floor":
            st = num // major
        else:
            st = (num + major - 1) // major
        ax, ay = (i, st) if dx > dy else (st, i)
        X, Y = x1 + sx * ax, y1 + sy * ay
        if not (0 <= X < size and 0 <= Y < size):
            break
        if i == n:
            end = (X, Y)
        else:
            crossed.append((X, Y))
    return crossed, end


def _mismatching_cases(form):
    bad = set()
    for c in kc.CASES:
        built = c.build()
        for g in kc.geometry(built) or []:
            if closed_form_cells(built[0], *g[:4], form=form) != kc.literal_cells(built[0], *g[:4]):
                bad.add(c.name)
                break
    return bad


def test_closed_form_equals_the_literal_loop_on_every_case():
    assert _mismatching_cases("device") == set()


@pytest.mark.parametrize("form", ["no_half", "floor"])
def test_a_wrong_closed_form_is_caught(form):
    """Negative check: a wrong copy of the closed form must fail the chunk-edge cases (end points at iterations 63, 64, 65) and
    the tie / octant cases at every size -- the cases have the resolution to see such an error."""
    bad = _mismatching_cases(form)
    for S in kc.GEOM_SIZES:
        assert "octants_%d" % S in bad, (form, S)
        assert "n_values_%d" % S in bad, (form, S)
    assert {"width_pp", "width_mm", "every_cell_16"} <= bad
    if form == "floor":
        # the exact diagonal alone catches it: floor(i - 1/2) is i - 1
        assert closed_form_cells(8, 1, 1, 5, 5, form) != kc.literal_cells(8, 1, 1, 5, 5)
