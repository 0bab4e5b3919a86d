"""Loading a saved world back (slamhip_hs_world_cells_upload, slamhip_hs_world_extends, save_world / load_world) against a NumPy
model, bit for bit.

The model is the "world canvas" of test_gpu_hector_backing.py, restated: per level a dense array of world cells with an offset,
filled with LogOddsCell.Reset() (UpdateIndex -1, Value 0.0f); a put overwrites its rectangle in it.  Beside it the model keeps the
set of tiles that must exist: a tile is made by a put only where the part of the rectangle that falls into it, outside the window,
holds a cell that is not Reset.

Probabilities are never computed here: the device's own value for a cell is taken from a second pyramid that received the same
cells through slamhip_hs_cells_upload (k5_refresh_prob), and the pyramid under test must hold the same bits -- in the window after
a put, and in a tile's slot (seen once a shift brings it into the window).

Pyramids: 64 x 48 and 72 x 56 with 3 levels (g = 4) and tiles of 8 cells: level 2 has rows of 16 and 12, and of 18 and 14, and the
window origins (0, 0), (-20, 12), (36, -28) give odd and even level origins, so no 16-byte unit is safe by accident."""
import math

import numpy as np
import pytest

import test_gpu_hector_shift as S
import test_gpu_hector_backing as BK
from test_gpu_hector_shift import hs_mod, ctx, det                         # noqa: F401 (fixtures)

gpu = pytest.mark.gpu

F = np.float32
CELL, LEVELS, G = S.CELL, S.LEVELS, S.G
TILE = 8
SLOT = 12 * TILE * TILE
ENOUGH = 4 << 20
DIMS = [(64, 48), (72, 56)]
DIM_IDS = ["64x48", "72x56"]
ORIGINS = [(0, 0), (-20, 12), (36, -28)]
ORIGIN_IDS = ["o0", "oa", "ob"]
ZERO_STATS = BK.ZERO_STATS


def reset_cells(shape, dtype):
    a = np.zeros(shape, dtype)
    a["update_index"] = -1
    return a


def not_reset(c):
    return (c["update_index"] != -1) | (c["value"].view(np.uint32) != 0)


class World:
    """One level's world cells around the origin: world cell (X, Y) lies at [Y + half, X + half]."""

    def __init__(self, dtype, half, half_y=None):
        self.half = half
        self.half_y = half if half_y is None else half_y                   # (a wide, low world: fewer rows than columns)
        self.cells = reset_cells((2 * self.half_y, 2 * half), dtype)

    def sl(self, x0, y0, w, h):
        x, y = x0 + self.half, y0 + self.half_y
        assert 0 <= x and x + w <= 2 * self.half and 0 <= y and y + h <= 2 * self.half_y, (x0, y0, w, h)
        return (slice(y, y + h), slice(x, x + w))

    def put(self, x0, y0, cells):
        self.cells[self.sl(x0, y0, cells.shape[1], cells.shape[0])] = cells

    def get(self, x0, y0, w, h):
        return self.cells[self.sl(x0, y0, w, h)].copy()


def random_cells(rng, h, w, dtype, p_reset=0.3):
    """Values of both signs and update indices as scans leave them, a share of LogOddsCell.Reset() among them."""
    c = np.zeros((h, w), dtype)
    c["value"] = (rng.standard_normal((h, w)) * 2.5).astype(np.float32)
    c["update_index"] = rng.integers(0, 40, (h, w))
    r = rng.random((h, w)) < p_reset
    c["update_index"][r] = -1
    c["value"][r] = 0.0
    return c


def level_dims(dims, l):
    return dims[0] >> l, dims[1] >> l


def tiles_of_put(model_tiles, l, dims, origin, x0, y0, cells):
    """The model's directory after a put with backing on and room enough: every tile the rectangle meets outside the window is
    made if it did not exist and its piece holds a non-Reset cell."""
    w, h = level_dims(dims, l)
    OX, OY = origin[0] >> l, origin[1] >> l
    rh, rw = cells.shape
    yy, xx = np.mgrid[0:rh, 0:rw]
    X, Y = xx + x0, yy + y0
    out = ~((X >= OX) & (X < OX + w) & (Y >= OY) & (Y < OY + h)) & not_reset(cells)
    for ty, tx in set(zip(np.floor_divide(Y[out], TILE).tolist(), np.floor_divide(X[out], TILE).tolist())):
        model_tiles.add((l, ty, tx))


def pool_bytes(n_tiles, max_bytes):
    """The pool grows in chunks of 4 MiB worth of slots, never past max_bytes."""
    if n_tiles == 0:
        return 0
    per_chunk = (4 << 20) // SLOT
    bytes_, slots = 0, 0
    while slots < n_tiles:
        n = min(per_chunk, (max_bytes - bytes_) // SLOT)
        assert n > 0
        slots += n
        bytes_ += n * SLOT
    return bytes_


def reference_prob(ref_rep, l, window_cells):
    """The device's own probabilities of these cells: a second pyramid that received them through slamhip_hs_cells_upload."""
    ref_rep.Maps[l].SetCells(np.ascontiguousarray(window_cells).ravel())
    return S.device_prob(ref_rep, l)


def rect_shapes(w, h, OX, OY):
    """The shapes of the planner test (tests/test_hs_world_abi.py), relative to the level's window."""
    return [(OX + 3, OY + 2, 5, 4), (OX + w + 9, OY - 20, 11, 7), (OX - 7, OY + 1, 12, 5), (OX - 9, OY - 10, w + 19, h + 21),
            (OX + w - 1, OY - 3, 1, h + 6), (OX - 11, OY + h - 1, w + 20, 1), (OX + w - 4, OY + h - 3, 13, 9)]


def assert_window(rep, ref_rep, worlds, dims, origin, tag):
    for l in range(LEVELS):
        w, h = level_dims(dims, l)
        want = worlds[l].get(origin[0] >> l, origin[1] >> l, w, h)
        got = rep.Maps[l].GetCells().reshape(h, w)
        assert np.array_equal(S.raw(got), S.raw(want)), (tag, l)
        assert S.same_bits(S.device_prob(rep, l), reference_prob(ref_rep, l, want)), (tag, l)


# ---- 1. put, then download --------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("origin", ORIGINS, ids=ORIGIN_IDS)
@pytest.mark.parametrize("dims", DIMS, ids=DIM_IDS)
def test_put_then_download(hs_mod, ctx, dims, origin):
    capi = hs_mod.capi
    rng = np.random.default_rng(1000 * dims[0] + origin[0] % 97)
    rep = hs_mod.MapRepMultiMap(CELL, dims, LEVELS, ctx=ctx)
    ref_rep = hs_mod.MapRepMultiMap(CELL, dims, LEVELS, ctx=ctx)
    if origin != (0, 0):
        rep.shift(*origin)
    rep.set_backing(TILE, ENOUGH)                                          # (after the move: a shift with backing on makes tiles of what it evicts)
    dtype = capi.CELL_DTYPE
    worlds = [World(dtype, 160) for _ in range(LEVELS)]
    tiles = set()
    for l in range(LEVELS):
        w, h = level_dims(dims, l)
        OX, OY = origin[0] >> l, origin[1] >> l
        for k, (x0, y0, rw, rh) in enumerate(rect_shapes(w, h, OX, OY)):
            cells = random_cells(rng, rh, rw, dtype)
            assert rep.world_put(l, x0, y0, cells) == 0, (l, k)
            worlds[l].put(x0, y0, cells)
            tiles_of_put(tiles, l, dims, origin, x0, y0, cells)
            st = rep.backing_stats()
            assert st["tiles"] == len(tiles) and st["bytes"] == pool_bytes(len(tiles), ENOUGH), (l, k, st)
            n = 2 * worlds[l].half
            got = rep.world_cells(l, -worlds[l].half, -worlds[l].half, n, n)               # a surrounding rectangle
            assert np.array_equal(S.raw(got), S.raw(worlds[l].cells)), (l, k)
    assert_window(rep, ref_rep, worlds, dims, origin, "put")
    st = rep.backing_stats()
    assert st["evicted_cells"] == 0 and st["restored_cells"] == 0 and st["dropped_cells"] == 0
    # what went into tile slots, probabilities included: bring it into the window
    for dx, dy in ((-3 * G, 2 * G), (5 * G, -4 * G)):
        rep.shift(dx, dy)
        origin = (origin[0] + dx, origin[1] + dy)
        assert_window(rep, ref_rep, worlds, dims, origin, (dx, dy))
    # the update-index rule of slamhip_hs_cells_upload: a scan's marks exceed every index put (39 -> at least 42: marks 43 and 44)
    xy = np.array([[1.0, 0.3], [0.9, -0.4], [1.2, 0.0]], np.float32)
    pose = np.array([dims[0] * CELL / 2, dims[1] * CELL / 2, 0.1], np.float32)
    before = [rep.Maps[l].GetCells() for l in range(LEVELS)]
    rep.UpdateByScan(hs_mod.ScanCloud(xy), pose)
    for l in range(LEVELS):
        after = rep.Maps[l].GetCells()
        ch = S.raw(after) != S.raw(before[l])
        assert ch.any() and set(np.unique(after["update_index"][ch]).tolist()) <= {43, 44}, (l, np.unique(after["update_index"][ch]))
    rep.close()
    ref_rep.close()


@gpu
def test_put_wider_than_a_piece(hs_mod, ctx):
    """One level of 2304 x 8 cells, a put of 2310 x 12 over it: the window job is 2304 cells wide, more than the 2048 of a piece,
    so k6_world_put -- and k6_world_extends over the window -- get it one row per workgroup; 582 tile jobs behind it."""
    capi = hs_mod.capi
    dims, (x0, y0, rw, rh) = (2304, 8), (-3, -2, 2310, 12)
    jobs = capi.world_plan(*dims, 0, 0, x0, y0, rw, rh, TILE)
    assert len(jobs) == 583 and jobs[0]["kind"] == capi.WORLD_WINDOW and (jobs[0]["nx"], jobs[0]["ny"]) == dims
    rng = np.random.default_rng(2304)
    rep = hs_mod.MapRepMultiMap(CELL, dims, 1, ctx=ctx)
    ref_rep = hs_mod.MapRepMultiMap(CELL, dims, 1, ctx=ctx)
    rep.set_backing(TILE, ENOUGH)
    world = World(capi.CELL_DTYPE, 1200 + dims[0] // 2, 32)                # world cells [-2352, 2352) x [-32, 32)
    cells = random_cells(rng, rh, rw, capi.CELL_DTYPE)
    assert rep.world_put(0, x0, y0, cells) == 0
    world.put(x0, y0, cells)
    tiles = set()
    tiles_of_put(tiles, 0, dims, (0, 0), x0, y0, cells)
    st = rep.backing_stats()
    assert len(tiles) > 500 and st["tiles"] == len(tiles) and st["bytes"] == pool_bytes(len(tiles), ENOUGH) and st["dropped_cells"] == 0
    got = rep.world_cells(0, -world.half, -world.half_y, 2 * world.half, 2 * world.half_y)       # a surrounding rectangle
    assert np.array_equal(S.raw(got), S.raw(world.cells))
    want = world.get(0, 0, *dims)
    assert np.array_equal(S.raw(rep.Maps[0].GetCells().reshape(dims[1], dims[0])), S.raw(want))
    assert S.same_bits(S.device_prob(rep, 0), reference_prob(ref_rep, 0, want))
    e = rep.world_extends(0)
    assert e is not None and e == bbox(world.cells, -world.half, -world.half_y)
    assert e[2] < 0 and e[0] >= dims[0] and e[3] < 0 and e[1] >= dims[1]   # (window and tiles both count)
    rep.close()
    ref_rep.close()


@gpu
def test_arguments(hs_mod, ctx):
    capi = hs_mod.capi
    rep = hs_mod.MapRepMultiMap(CELL, (64, 48), LEVELS, ctx=ctx)
    sums = [rep.Maps[l].checksum() for l in range(LEVELS)]
    cell = np.zeros(4, capi.CELL_DTYPE)
    ptr = cell.ctypes.data_as(hs_mod.C.c_void_p)
    L = capi.lib()
    for args in ((0, 0, 0, 0, 2), (0, 0, 0, 2, -1), (0, 0, 0, 1 << 14, (1 << 12) + 1), (0, 1 << 60, 0, 2, 2), (0, 0, -(1 << 60), 2, 2),
                 (LEVELS, 0, 0, 2, 2), (-1, 0, 0, 2, 2)):
        assert L.slamhip_hs_world_cells_upload(rep._h, *args, ptr, None) == capi.ERR_INVALID, args
    assert L.slamhip_hs_world_cells_upload(rep._h, 0, 0, 0, 2, 2, None, None) == capi.ERR_INVALID
    assert [rep.Maps[l].checksum() for l in range(LEVELS)] == sums and rep.backing_stats() == ZERO_STATS
    assert L.slamhip_hs_world_cells_upload(rep._h, 0, 0, 0, 2, 2, ptr, None) == capi.OK              # out_dropped may be NULL
    rep.close()


# ---- 2. round trip and continuation -----------------------------------------------------------------------------------------------
def walk(hs_mod, ctx, sim, dims, backing=(TILE, ENOUGH)):
    """A pyramid that mapped a walk that scrolls out and back: updates in the window's frame, shifts between them."""
    w0, h0 = dims
    rep = hs_mod.MapRepMultiMap(CELL, dims, LEVELS, ctx=ctx)
    if backing:
        rep.set_backing(*backing)
    scans = S.local_scans(sim, w0, h0)
    for xy, p in scans:
        rep.UpdateByScan(hs_mod.ScanCloud(xy), p)
    n_u = 0
    for step in [(G, 0), "u", (0, -G), (4 * G, 2 * G), "u", (-3 * G, G), (0, 3 * G), "u", (6 * G, -4 * G), "u", (-9 * G, -2 * G), "u", (-G, 0)]:
        if step == "u":
            xy, p = scans[(3 * n_u + 1) % len(scans)]
            n_u += 1
            rep.UpdateByScan(hs_mod.ScanCloud(xy), p)
        else:
            rep.shift(*step)
    return rep, scans


def world_of(rep, l, reach):
    return rep.world_cells(l, -(reach >> l), -(reach >> l), 2 * (reach >> l), 2 * (reach >> l))


def bbox(cells, x0, y0):
    """(xmax, ymax, xmin, ymin) of value != 0 (a NaN counts) in a world download whose cell (0, 0) is (x0, y0), or None."""
    ys, xs = np.nonzero(cells["value"] != 0)
    if ys.size == 0:
        return None
    return (int(xs.max()) + x0, int(ys.max()) + y0, int(xs.min()) + x0, int(ys.min()) + y0)


@gpu
@pytest.mark.parametrize("dims", DIMS, ids=DIM_IDS)
def test_round_trip_and_continuation(hs_mod, ctx, sim, tmp_path, dims):
    capi = hs_mod.capi
    A, scans = walk(hs_mod, ctx, sim, dims)
    assert A.backing_stats()["tiles"] > 0 and A.backing_stats()["dropped_cells"] == 0
    path = str(tmp_path / "world.npz")
    A.save_world(path)
    B = hs_mod.MapRepMultiMap(CELL, dims, LEVELS, ctx=ctx)
    assert B.load_world(path) == 0
    assert B.origin() == A.origin() != (0, 0)
    stA, stB = A.backing_stats(), B.backing_stats()
    assert stB["on"] == 1 and stB["tile"] == TILE and stB["capacity_bytes"] == ENOUGH and 0 < stB["tiles"] <= stA["tiles"]
    reach = 512
    for l in range(LEVELS):
        assert A.Maps[l].checksum() == B.Maps[l].checksum(), l
        e = A.world_extends(l)
        assert e is not None and e == B.world_extends(l), l
        wa = A.world_cells(l, e[2], e[3], e[0] - e[2] + 1, e[1] - e[3] + 1)
        assert np.count_nonzero(wa["value"]) > 0
        assert np.array_equal(S.raw(wa), S.raw(B.world_cells(l, e[2], e[3], e[0] - e[2] + 1, e[1] - e[3] + 1))), l
        assert np.array_equal(S.raw(world_of(A, l, reach)), S.raw(world_of(B, l, reach))), l
        assert S.same_bits(S.device_prob(A, l), S.device_prob(B, l)), l
    # the same scan and hint: poses and reports equal bit for bit
    m = hs_mod.ScanMatcher(1, referenceSummation=True)
    org = A.origin()
    xy, p = scans[-1]
    p_win = np.array([p[0] - F(org[0]) * F(CELL), p[1] - F(org[1]) * F(CELL), p[2]], np.float32)
    for d in ((0, 0, 0), (0.03, -0.02, 0.02)):
        hint = p_win + np.array(d, np.float32)
        pa, ra = m.MatchDataReport(A, hs_mod.ScanCloud(xy), hint)
        pb, rb = m.MatchDataReport(B, hs_mod.ScanCloud(xy), hint)
        assert S.same_bits(pa, pb) and ra.tobytes() == rb.tobytes(), (d, pa, pb)
        assert not S.same_bits(pa, hint) and ra["n_in_map"] > 0               # (there was a map to match against)
    # six further update + shift steps on both: the worlds stay equal bit for bit, update indices included
    steps = [(G, 0), (0, 2 * G), (-3 * G, -G), (2 * G, -2 * G), (-G, G), (G, 0)]
    for k, (dx, dy) in enumerate(steps):
        xy, p = scans[(2 * k + 1) % len(scans)]
        for rep in (A, B):
            rep.UpdateByScan(hs_mod.ScanCloud(xy), p)                      # (in the window's frame, as in the walk)
            rep.shift(dx, dy)
        for l in range(LEVELS):
            wa, wb = world_of(A, l, reach), world_of(B, l, reach)
            assert np.array_equal(wa["update_index"], wb["update_index"]), (k, l)
            assert np.array_equal(S.raw(wa), S.raw(wb)), (k, l)
            assert A.Maps[l].checksum() == B.Maps[l].checksum(), (k, l)
    assert A.origin() == B.origin()
    # a pyramid of another geometry refuses the file, unchanged
    Cq = hs_mod.MapRepMultiMap(CELL, (dims[0] + 8, dims[1]), LEVELS, ctx=ctx)
    with pytest.raises(ValueError):
        Cq.load_world(path)
    assert Cq.origin() == (0, 0) and Cq.backing_stats() == ZERO_STATS and Cq.world_extends(0) is None
    for r in (A, B, Cq):
        r.close()


# ---- 3. the window wins -----------------------------------------------------------------------------------------------------------
@gpu
def test_window_wins(hs_mod, ctx):
    capi = hs_mod.capi
    dims = (64, 48)
    rng = np.random.default_rng(7)
    rep = hs_mod.MapRepMultiMap(CELL, dims, LEVELS, ctx=ctx)
    rep.shift(G, 0)                                                        # level origins 4, 2, 1: tile (0, 0) lies partly under every window
    rep.set_backing(TILE, ENOUGH)
    origin = (G, 0)
    put, win = [], []
    for l in range(LEVELS):
        w, h = level_dims(dims, l)
        OX = origin[0] >> l
        assert 0 < OX < TILE
        rep.Maps[l].SetCells(random_cells(rng, h, w, capi.CELL_DTYPE, 0.0).ravel())
        cells = random_cells(rng, TILE, TILE, capi.CELL_DTYPE, 0.0)
        assert rep.world_put(l, 0, 0, cells) == 0                          # the whole of tile (0, 0)
        put.append(cells)
        win.append(rep.Maps[l].GetCells().reshape(h, w).copy())
        assert np.array_equal(S.raw(win[l][:TILE, :TILE - OX]), S.raw(cells[:, OX:]))      # the window's part went into the window
    assert rep.backing_stats()["tiles"] == LEVELS
    far = 2 * dims[0]
    rep.shift(far, 0)                                                      # away: every level cleared, the windows' cells into their tiles
    assert all((rep.Maps[l].GetCells()["update_index"] == -1).all() for l in range(LEVELS))
    rep.shift(-far, 0)
    for l in range(LEVELS):
        w, h = level_dims(dims, l)
        OX = origin[0] >> l
        assert np.array_equal(S.raw(rep.Maps[l].GetCells().reshape(h, w)), S.raw(win[l])), l     # the window's cells survived
        got = rep.world_cells(l, 0, 0, TILE, TILE)
        assert np.array_equal(S.raw(got[:, :OX]), S.raw(put[l][:, :OX])), l                     # the tile's outside part: the put cells
        assert np.array_equal(S.raw(got[:, OX:]), S.raw(win[l][:TILE, :TILE - OX])), l
    rep.close()


# ---- 4. a sparse world loads sparse -----------------------------------------------------------------------------------------------
@gpu
def test_sparse(hs_mod, ctx):
    capi = hs_mod.capi
    rep = hs_mod.MapRepMultiMap(CELL, (64, 48), LEVELS, ctx=ctx)
    rep.set_backing(TILE, ENOUGH)
    big = reset_cells((150, 170), capi.CELL_DTYPE)
    assert rep.world_put(0, -100, -97, big) == 0                           # over the window and far around it: all Reset
    assert rep.backing_stats()["tiles"] == 0 and rep.backing_stats()["bytes"] == 0
    big["value"][100, 3] = 1.5                                             # world cell (-97, 3): tile (0, -13)
    assert rep.world_put(0, -100, -97, big) == 0
    st = rep.backing_stats()
    assert st["tiles"] == 1 and st["bytes"] == pool_bytes(1, ENOUGH)
    got = rep.world_cells(0, -100, -97, 170, 150)
    assert np.array_equal(S.raw(got), S.raw(big))
    assert rep.world_extends(0) == (-97, 3, -97, 3)
    big["value"][100, 3] = 0.0                                             # an all-Reset piece over an EXISTING tile is written
    assert rep.world_put(0, -100, -97, big) == 0
    assert rep.backing_stats()["tiles"] == 1 and rep.world_extends(0) is None
    assert np.array_equal(S.raw(rep.world_cells(0, -100, -97, 170, 150)), S.raw(big))
    rep.close()


# ---- 5. capacity ------------------------------------------------------------------------------------------------------------------
@gpu
def test_capacity(hs_mod, ctx):
    capi = hs_mod.capi
    rng = np.random.default_rng(11)
    rep = hs_mod.MapRepMultiMap(CELL, (64, 48), LEVELS, ctx=ctx)
    rep.set_backing(TILE, 2 * SLOT)
    x0, y0 = -47, -19                                                      # 3 x 2 tiles left of the window, the rectangle inside them
    cells = random_cells(rng, 2 * TILE - 5, 3 * TILE - 4, capi.CELL_DTYPE)
    jobs = capi.world_plan(64, 48, 0, 0, x0, y0, cells.shape[1], cells.shape[0], TILE)
    assert len(jobs) == 6 and (jobs["kind"] == capi.WORLD_TILE).all()
    dropped = hs_mod.C.c_int64(-1)
    capi.call("slamhip_hs_world_cells_upload", rep._h, 0, x0, y0, cells.shape[1], cells.shape[0],
              cells.ctypes.data_as(hs_mod.C.c_void_p), hs_mod.C.byref(dropped))            # SLAMHIP_OK (anything else raises)
    want = reset_cells(cells.shape, capi.CELL_DTYPE)
    lost = 0
    for k, j in enumerate(jobs):
        sl = (slice(j["sy"], j["sy"] + j["ny"]), slice(j["sx"], j["sx"] + j["nx"]))
        if k < 2:
            want[sl] = cells[sl]                                           # the first two in planner order are kept
        else:
            lost += int(not_reset(cells[sl]).sum())
    assert lost > 0 and dropped.value == lost
    st = rep.backing_stats()
    assert st["tiles"] == 2 and st["bytes"] == 2 * SLOT == st["capacity_bytes"] and st["dropped_cells"] == lost
    assert st["evicted_cells"] == 0 and st["restored_cells"] == 0
    assert np.array_equal(S.raw(rep.world_cells(0, x0, y0, cells.shape[1], cells.shape[0])), S.raw(want))
    # an existing tile is still written when the pool is full
    again = random_cells(rng, cells.shape[0], cells.shape[1], capi.CELL_DTYPE, 0.0)
    assert rep.world_put(0, x0, y0, again) == sum(int(j["nx"]) * int(j["ny"]) for j in jobs[2:])
    for j in jobs[:2]:
        sl = (slice(j["sy"], j["sy"] + j["ny"]), slice(j["sx"], j["sx"] + j["nx"]))
        want[sl] = again[sl]
    assert np.array_equal(S.raw(rep.world_cells(0, x0, y0, cells.shape[1], cells.shape[0])), S.raw(want))
    assert rep.backing_stats()["tiles"] == 2
    rep.close()


# ---- 6. backing off ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dims", DIMS, ids=DIM_IDS)
def test_backing_off(hs_mod, ctx, dims):
    capi = hs_mod.capi
    rng = np.random.default_rng(13)
    rep = hs_mod.MapRepMultiMap(CELL, dims, LEVELS, ctx=ctx)
    ref_rep = hs_mod.MapRepMultiMap(CELL, dims, LEVELS, ctx=ctx)
    origin = (-20, 12)
    rep.shift(*origin)
    for l in range(LEVELS):
        w, h = level_dims(dims, l)
        OX, OY = origin[0] >> l, origin[1] >> l
        cells = random_cells(rng, h + 21, w + 19, capi.CELL_DTYPE)
        inner = cells[10:10 + h, 9:9 + w]
        assert rep.world_put(l, OX - 9, OY - 10, cells) == int(not_reset(cells).sum()) - int(not_reset(inner).sum())
        want = reset_cells(cells.shape, capi.CELL_DTYPE)
        want[10:10 + h, 9:9 + w] = inner                                   # only the window is written
        assert np.array_equal(S.raw(rep.world_cells(l, OX - 9, OY - 10, w + 19, h + 21)), S.raw(want)), l
        assert np.array_equal(S.raw(rep.Maps[l].GetCells().reshape(h, w)), S.raw(inner)), l
        assert S.same_bits(S.device_prob(rep, l), reference_prob(ref_rep, l, inner)), l
        assert rep.world_extends(l) == bbox(want, OX - 9, OY - 10), l
        # wholly outside the window, and straddling its left edge only: nothing but the window's part is written
        far = random_cells(rng, 7, 11, capi.CELL_DTYPE)
        assert rep.world_put(l, OX + w + 9, OY - 20, far) == int(not_reset(far).sum()), l
        edge = random_cells(rng, 5, 12, capi.CELL_DTYPE)
        assert rep.world_put(l, OX - 7, OY + 1, edge) == int(not_reset(edge[:, :7]).sum()), l
        want[10:10 + h, 9:9 + w][1:6, :5] = edge[:, 7:]
        assert np.array_equal(S.raw(rep.world_cells(l, OX - 9, OY - 10, w + 19, h + 21)), S.raw(want)), l
    assert rep.backing_stats() == ZERO_STATS
    rep.close()
    ref_rep.close()


# ---- 7. the extents ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dims", DIMS, ids=DIM_IDS)
def test_extents(hs_mod, ctx, sim, dims):
    capi = hs_mod.capi
    empty = hs_mod.MapRepMultiMap(CELL, dims, LEVELS, ctx=ctx)
    assert all(empty.world_extends(l) is None for l in range(LEVELS))
    empty.set_backing(TILE, ENOUGH)
    assert all(empty.world_extends(l) is None for l in range(LEVELS))
    empty.close()
    A, _ = walk(hs_mod, ctx, sim, dims)
    reach = 512
    for l in range(LEVELS):
        e = A.world_extends(l)
        assert e is not None and e == bbox(world_of(A, l, reach), -(reach >> l), -(reach >> l)), l
        w, h = level_dims(dims, l)
        OX, OY = A.origin()[0] >> l, A.origin()[1] >> l
        assert e[2] < OX or e[0] >= OX + w or e[3] < OY or e[1] >= OY + h, l                  # (the world is wider than the window)
    # stale copies: the tiles under the window hold what was evicted earlier; clear the window, and they must not widen the extents
    stale = [A.Maps[l].GetCells() for l in range(LEVELS)]
    for l in range(LEVELS):
        w, h = level_dims(dims, l)
        assert np.count_nonzero(stale[l]["value"]) > 0
        A.Maps[l].SetCells(reset_cells(w * h, capi.CELL_DTYPE))
        nan = reset_cells((1, 1), capi.CELL_DTYPE)
        nan["value"] = np.nan                                              # a NaN counts (GridMap.cs:161)
        OX, OY = A.origin()[0] >> l, A.origin()[1] >> l
        A.world_put(l, OX + w // 2, OY + h // 2, nan)
        got = world_of(A, l, reach)
        e = A.world_extends(l)
        assert e == bbox(got, -(reach >> l), -(reach >> l)), l
        inside = got[(reach >> l) + OY:(reach >> l) + OY + h, (reach >> l) + OX:(reach >> l) + OX + w]
        assert np.count_nonzero(inside["value"] != 0) == 1, l
    # backing off: the window only
    A.set_backing(0, 0)
    for l in range(LEVELS):
        w, h = level_dims(dims, l)
        OX, OY = A.origin()[0] >> l, A.origin()[1] >> l
        assert A.world_extends(l) == (OX + w // 2, OY + h // 2, OX + w // 2, OY + h // 2), l
    A.close()


# ---- 8. the processor resumes -----------------------------------------------------------------------------------------------------
@gpu
def test_processor_resumes(hs_mod, ctx, sim, tmp_path):
    W, TRIGGER, START = S.W, S.TRIGGER, S.START
    d = BK.out_and_back(sim)
    n_a = len(d) - 4

    def make(start):
        p = hs_mod.HectorSLAMProcessor(CELL, (W, W), start, LEVELS, 1, ctx=ctx, referenceSummation=True, scrollTrigger=TRIGGER,
                                       scrollBacking=(16, 64 << 20))
        p.MinAngleDiffForMapUpdate = -200.0                                # every scan updates the map
        return p

    A = make(START)
    hint = START.copy()
    for i in range(n_a):
        if i:
            hint = (A.MatchPose + (d[i][0] - d[i - 1][0]).astype(np.float32)).astype(np.float32)
        assert A.Update(hs_mod.ScanCloud(d[i][1]), hint)
    assert A.get_origin() != (0, 0) and A.backing_stats()["tiles"] > 0 and A.backing_stats()["restored_cells"] > 0
    path = str(tmp_path / "proc.npz")
    A.SaveWorld(path)
    B = make(A.MatchPose)
    assert B.LoadWorld(path) == 0
    assert B.get_origin() == A.get_origin()
    assert np.abs(B.MatchPose - A.MatchPose).max() < 1e-4                  # (world poses: the window moved under the processor)
    reach = 1024
    for i in range(n_a, len(d)):
        hint = (A.MatchPose + (d[i][0] - d[i - 1][0]).astype(np.float32)).astype(np.float32)
        ua = A.Update(hs_mod.ScanCloud(d[i][1]), hint)
        ub = B.Update(hs_mod.ScanCloud(d[i][1]), hint)
        assert ua and ub, i
        assert S.same_bits(A.MatchPose, B.MatchPose), (i, A.MatchPose, B.MatchPose)
        assert A.get_origin() == B.get_origin(), i
        for l in range(LEVELS):
            assert np.array_equal(S.raw(world_of(A.MapRep, l, reach)), S.raw(world_of(B.MapRep, l, reach))), (i, l)
    err = A.MatchPose - d[-1][0]
    assert math.hypot(err[0], err[1]) < 0.2, err
    A.Dispose()
    B.Dispose()
