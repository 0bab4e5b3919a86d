"""K5, the Hector grid update, at its edges -- the cases of tests/k5_cases.py (each checked on the CPU for the property it claims:
tests/test_k5_cases_cpu.py) on the device through MapRepMultiMap: SetCells, UpdateByScan, GetCells.  After EVERY update of a case
the update indices and the values' bits of all cells of all levels are compared with == against the C oracle (NaN and -0.0 count);
after the last one the cached probabilities of all cells (atol 2e-7: the device's expf against libm's, as in
test_grid_update_vs_oracle; NaN for NaN), the bitmap and the map's extends.  The same cases run once more in fresh interpreters
with the tables read from memory (SLAMHIP_K5_TWO_LAUNCHES=1) and with the sectors dealt by count (SLAMHIP_K5_EQUAL_SECTORS=1).

Out of scope: the gated update inside HectorSLAMProcessor.Update (the matcher moves the pose; test_hector_processor_* guard it).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import k5_cases as kc
from test_gpu_hector import hs_mod, ctx, det                             # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in kc.CASES]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_cells(got, ref, what):
    for field in ("update_index", "value"):
        g, r = bits(got[field]), bits(ref[field])
        bad = np.flatnonzero(g != r)
        assert bad.size == 0, (what, field, bad.size, bad[:8], got[field][bad[:8]], ref[field][bad[:8]])


def oracle_prob(g):
    """The oracle's probability of every cell: its expression evaluated once per distinct value."""
    _, first, inverse = np.unique(bits(g.cells["value"]), return_index=True, return_inverse=True)
    return np.array([g.prob(int(i)) for i in first], np.float32)[inverse]


@pytest.mark.parametrize("name", NAMES)
def test_case(hs_mod, ctx, det, name):
    oc = det
    built = kc.by_name(name).build()
    levels = built.levels
    dims = kc.level_dims(built.size, levels)
    rep = hs_mod.MapRepMultiMap(built.cell_len, built.size, levels, ctx=ctx)
    ref = oc.make_pyramid(built.cell_len, built.size[0], built.size[1], levels)
    try:
        assert [m.Dimensions for m in rep.Maps] == dims
        if built.factors:
            rep.SetUpdateFactorFree(built.factors[0]); rep.SetUpdateFactorOccupied(built.factors[1])
            for g in ref:
                g.set_factors(*built.factors)

        cur = [0] * levels

        def upload(cells):
            # (SetCells moves the level's current update index past every uploaded index, kc.index_after_upload: the oracle, which
            # has no upload, follows with empty scans)
            for l in range(levels):
                rep.Maps[l].SetCells(cells[l])
                ref[l].cells[:] = cells[l]
                for _ in range((kc.index_after_upload(cells[l], cur[l]) - cur[l]) // 3):
                    ref[l].update_by_scan(np.zeros((0, 2), np.float32), (0.0, 0.0, 0.0))
                cur[l] = kc.index_after_upload(cells[l], cur[l])
        if built.start is not None:
            upload(built.start)
        for k, step in enumerate(built.steps):
            if kc.is_scan(step):
                xy, origin, pose = step
                rep.UpdateByScan(hs_mod.ScanCloud(xy, (origin[0], origin[1], 0.0)), pose)
                for g in ref:
                    g.update_by_scan(xy, pose, origin=origin)
                cur = [c + 3 for c in cur]
            elif step[0] == "reset":
                rep.Reset()
                for g in ref:
                    g.reset()
                cur = [0] * levels
            elif step[0] == "set_cells":
                upload(step[1])
            elif step[0] == "shift":
                rep.shift(step[1], step[2])
                for l, g in enumerate(ref):
                    g.cells[:] = kc.shifted(g.cells.copy(), dims[l][0], dims[l][1], step[1] >> l, step[2] >> l)
            for l in range(levels):
                same_cells(rep.Maps[l].GetCells(), ref[l].cells, (name, k, l))
        for l in range(levels):
            w, h = dims[l]
            got = rep.Maps[l].GetCachedProbability(np.arange(w * h, dtype=np.int32))
            want = oracle_prob(ref[l])
            nan = np.isnan(want)
            assert (np.isnan(got) == nan).all(), (name, l)
            assert np.allclose(got[~nan], want[~nan], rtol=0, atol=2e-7), (name, l, np.abs(got[~nan] - want[~nan]).max())
            assert (rep.Maps[l].GetBitmapData() == ref[l].bitmap()).all(), (name, l)
            assert rep.Maps[l].GetMapExtends() == ref[l].map_extends(), (name, l)
    finally:
        rep.close()
        for g in ref:
            g.close()


def test_cases_under_the_switches():
    """Every case again in a fresh interpreter with the line tables made by k5_prepare and read from memory
    (SLAMHIP_K5_TWO_LAUNCHES=1), and with phase 2's sectors dealt by count, no record read or written (SLAMHIP_K5_EQUAL_SECTORS=1)."""
    here = os.path.abspath(__file__)
    for extra in ({"SLAMHIP_K5_TWO_LAUNCHES": "1"}, {"SLAMHIP_K5_EQUAL_SECTORS": "1"}):
        r = subprocess.run(["timeout", "-k", "10", "540", sys.executable, "-m", "pytest", here, "-m", "gpu", "-x", "-q", "-k", "not under_the_switches"],
                           env=dict(os.environ, **extra), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        out = r.stdout.decode(errors="replace")
        assert r.returncode == 0 and "%d passed" % len(NAMES) in out, (extra, out[-3000:])
