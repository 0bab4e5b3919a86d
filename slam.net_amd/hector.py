"""Host mirror of the reference's HectorSLAM public API on top of the C-ABI (include/slamhip.h).

Mirrors HectorSLAM/Main/MapRepMultiMap.cs, Map/OccGridMap.cs, Matcher/ScanMatcher.cs and
Main/HectorSLAMProcessor.cs: same names and argument meaning; all compute is in libslamhip.so.
"""
import ctypes as C
import math

import numpy as np

from . import capi
from .coreslam import Context


def hint_lattice(centre, half_xy, step_xy, half_theta, step_theta):
    """The (B, 3) float32 hint list of a relocalisation around `centre` = (x, y, theta): every combination of
    x, y in centre +- k * step_xy (k * step_xy <= half_xy) and theta in centre +- j * step_theta (j * step_theta <=
    half_theta), B = (2 * floor(half_xy / step_xy) + 1)^2 * (2 * floor(half_theta / step_theta) + 1).  The centre itself
    comes first (ties in ScanMatcher.MatchDataBest go to the lowest index); the rest follow in x-major, then y, then
    theta order.  Offsets are formed in binary64 and rounded once to binary32.  Pure host code."""
    c = np.asarray(centre, np.float64).reshape(3)
    if not (step_xy > 0 and step_theta > 0 and half_xy >= 0 and half_theta >= 0):
        raise ValueError("hint_lattice: steps must be positive and half-widths non-negative")
    nxy = int(np.floor(half_xy / step_xy + 1e-9)); nth = int(np.floor(half_theta / step_theta + 1e-9))
    out = [c]
    for i in range(-nxy, nxy + 1):
        for j in range(-nxy, nxy + 1):
            for k in range(-nth, nth + 1):
                if i or j or k:
                    out.append(c + np.array([i * step_xy, j * step_xy, k * step_theta]))
    return np.asarray(out, np.float64).astype(np.float32)


def decode_lattice_key(key):
    """A key of MapRepMultiMap.lattice_search -> (score, flat): key = ((uint32)score ^ 0x80000000) << 32 | (0xFFFFFFFF - flat)."""
    key = int(key)
    score = ((key >> 32) ^ 0x80000000) & 0xFFFFFFFF
    return (score - (1 << 32) if score >= (1 << 31) else score), 0xFFFFFFFF - (key & 0xFFFFFFFF)


def _reloc_info(info):
    return np.array([tuple(getattr(info, n) for n, _ in capi.RelocInfo._fields_)], capi.RELOC_INFO)[0]


BNB_DEFAULT_TOP = 3                                            # what top=None means: the fastest of 3 .. 6 at K7's own configuration (profiles/r30_hs_bnb.json)


def _search_kind(search):
    if search not in ("lattice", "bnb"):
        raise ValueError('search must be "lattice" or "bnb", not %r' % (search,))
    return search == "bnb"


def _world_reloc_info(info):
    return np.array([tuple(getattr(info, n) for n, _ in capi.WorldRelocInfo._fields_)], capi.WORLD_RELOC_INFO)[0]


def align_step(pose, summary, stm, base=None):
    """One closed-form 2-D alignment step from ONE capi.PAIR_SUMMARY record (slamhip_hs_nearest_pairs) -> (pose', dtheta, (tx, ty)):
    the rigid motion e' = R(dtheta) e + t, in cells, that best takes the matched end cells e onto their nearest sites q in the least
    squares sense, composed onto `pose` (the frame the summary was formed in).  Host arithmetic only: the centred sums n S_ab -
    S_a S_b are formed exactly, as integers, then everything is binary64.  n_matched >= 2: dtheta = atan2(sum(e'x q'y - e'y q'x),
    sum(e'x q'x + e'y q'y)) over the centred cells; n_matched == 1: dtheta = 0.  t = mean(q) - R(dtheta) mean(e); no matched point:
    the pose comes back as it is.  The composition follows hs_trace.h's transform, e = stm (R(theta) p + T) for a scan point p and
    the pose (T, theta): R(dtheta) e + t = stm (R(theta + dtheta) p + R(dtheta) T + t / stm), so theta' = theta + dtheta and
    T' = R(dtheta) T + t / stm.  base: the same pose in another frame of the same heading (a processor's world pose); the step's
    change T' - T is added to IT, so a zero step hands `base` back bit for bit.  The result is rounded to binary32 once."""
    s = summary
    n = int(s["n_matched"])
    x, y, th = (float(v) for v in np.asarray(pose, np.float32).reshape(3))
    bx, by, bth = (x, y, th) if base is None else (float(v) for v in np.asarray(base, np.float32).reshape(3))
    if n < 1:
        return np.array([bx, by, bth], np.float32), 0.0, (0.0, 0.0)
    S = {k: int(s["sum_" + k]) for k in ("ex", "ey", "qx", "qy", "exqx", "eyqy", "exqy", "eyqx")}
    dth = 0.0
    if n >= 2:
        cross = (n * S["exqy"] - S["ex"] * S["qy"]) - (n * S["eyqx"] - S["ey"] * S["qx"])   # n * sum(e'x q'y - e'y q'x), exact
        dot = (n * S["exqx"] - S["ex"] * S["qx"]) + (n * S["eyqy"] - S["ey"] * S["qy"])     # n * sum(e'x q'x + e'y q'y), exact
        dth = math.atan2(float(cross) / n, float(dot) / n)
    c, sn = math.cos(dth), math.sin(dth)
    tx = (S["qx"] - (c * S["ex"] - sn * S["ey"])) / n               # mean(q) - R mean(e), divided once: a pure shift comes out exact
    ty = (S["qy"] - (sn * S["ex"] + c * S["ey"])) / n
    stm = float(np.float32(stm))
    out = np.array([bx + ((c - 1.0) * x - sn * y + tx / stm), by + (sn * x + (c - 1.0) * y + ty / stm), bth + dth], np.float32)
    return out, dth, (tx, ty)


class ScanCloud:
    """BaseSLAM/ScanCloud.cs:10-21"""

    def __init__(self, points, pose=(0.0, 0.0, 0.0)):
        self.Points = capi.f32(points, (-1, 2))
        self.Pose = np.asarray(pose, np.float32)


class OccGridMap:
    """One pyramid level (HectorSLAM/Map/OccGridMap.cs + GridMap.cs), a view onto the device pyramid."""

    def __init__(self, rep, level):
        self._rep, self.level = rep, level
        w, h, c = C.c_int32(), C.c_int32(), C.c_float()
        capi.call("slamhip_hs_level_info", rep._h, level, C.byref(w), C.byref(h), C.byref(c))
        self.Dimensions = (w.value, h.value)
        self.CellLength = c.value
        self._iters = 3

    @property
    def EstimateIterations(self):
        return self._iters

    @EstimateIterations.setter
    def EstimateIterations(self, v):
        self._iters = int(v)
        self._rep._push_iterations()

    def GetCells(self):
        n = self.Dimensions[0] * self.Dimensions[1]
        out = np.empty(n, capi.CELL_DTYPE)
        capi.call("slamhip_hs_cells_download", self._rep._h, self.level, out.ctypes.data_as(C.c_void_p), n)
        return out

    def SetCells(self, cells):
        cells = np.ascontiguousarray(cells, capi.CELL_DTYPE)
        capi.call("slamhip_hs_cells_upload", self._rep._h, self.level, cells.ctypes.data_as(C.c_void_p), cells.size)

    def GetBitmapData(self):
        n = self.Dimensions[0] * self.Dimensions[1]
        out = np.empty(n, np.uint8)
        capi.call("slamhip_hs_bitmap_download", self._rep._h, self.level, out.ctypes.data_as(C.POINTER(C.c_uint8)), n)
        return out

    def GetMapExtends(self):
        """GridMap.GetMapExtends (GridMap.cs:147-207): (found, xMax, yMax, xMin, yMin), reduced on the device."""
        e = (C.c_int32 * 4)()
        f = C.c_int32()
        capi.call("slamhip_hs_map_extends", self._rep._h, self.level, e, C.byref(f))
        return (bool(f.value), e[0], e[1], e[2], e[3])

    def checksum(self):
        """(log-odds, update indices) replica-check words of this level (slamhip_hs_checksum)."""
        out = (C.c_uint64 * 2)()
        capi.call("slamhip_hs_checksum", self._rep._h, self.level, out)
        return int(out[0]), int(out[1])

    def GetCell(self, *a):
        """GridMap.GetCell(x, y) / GetCell(index) (GridMap.cs:70-96): one LogOddsCell read back from the device."""
        idx = a[1] * self.Dimensions[0] + a[0] if len(a) == 2 else int(a[0])
        return self.GetCells()[idx]

    def GetCachedProbability(self, indices):
        idx = np.ascontiguousarray(np.atleast_1d(indices), np.int32)
        out = np.empty(idx.size, np.float32)
        capi.call("slamhip_hs_probability", self._rep._h, self.level, capi.iptr(idx), idx.size, capi.fptr(out))
        return out

    def Hessian(self, pose_map):
        p = capi.f32(pose_map); H = np.empty(9, np.float32); d = np.empty(3, np.float32)
        capi.call("slamhip_hs_hessian", self._rep._h, self.level, capi.fptr(p), capi.fptr(H), capi.fptr(d))
        return H.reshape(3, 3), d


class MapRepMultiMap:
    """HectorSLAM/Main/MapRepMultiMap.cs:19-96"""

    def __init__(self, mapResolution, mapSize, numDepth, startCoords=(0.0, 0.0), ctx=None, _handle=None):
        self.ctx = ctx or Context(0)
        self._owned = _handle is None
        self._h = C.c_void_p() if _handle is None else _handle
        if _handle is None:
            capi.call("slamhip_hs_create", self.ctx._h, C.c_float(mapResolution), int(mapSize[0]), int(mapSize[1]),
                      int(numDepth), C.byref(self._h))
        self.Maps = [OccGridMap(self, l) for l in range(numDepth)]
        self._scan_set = None
        self._mcl_n = 0                                             # particles of the last mcl_set

    @property
    def NumLevels(self):
        return len(self.Maps)

    def _push_iterations(self):
        it = np.array([m._iters for m in self.Maps], np.int32)
        capi.call("slamhip_hs_set_iterations", self._h, capi.iptr(it))

    def Reset(self):
        capi.call("slamhip_hs_reset", self._h)

    def set_match_threads(self, numThreads):
        """The matcher's summation order on this pyramid (slamhip_hs_set_match_threads): 0 the device's own (default),
        1 .. 64 the reference's ScanMatcher(numThreads) chunks (ScanMatcher.cs:149-195), bit for bit."""
        capi.call("slamhip_hs_set_match_threads", self._h, int(numThreads))

    def set_reference_cache(self, on):
        """The reference's probability cache on this pyramid (slamhip_hs_set_reference_cache, deviation D5): 1 every
        probability the matcher and GetCachedProbability read goes through OccGridMap's cacheArray, stale across Reset as
        in the reference (OccGridMap.cs:97-107,248); 0 the current probability (default).  Turning it on starts from a
        new OccGridMap's cache."""
        capi.call("slamhip_hs_set_reference_cache", self._h, int(on))

    def shift(self, dx, dy):
        """Move the window by (+dx, +dy) level-0 cells on the device, in stream order (slamhip_hs_shift): on level l new
        cell (x, y) holds what old cell (x + (dx >> l), y + (dy >> l)) held, exposed cells are LogOddsCell.Reset().  dx and dy
        must be multiples of 1 << (NumLevels - 1).  Matches and updates go on working in the window's frame: a world point
        p lies at p - origin * CellLength(level 0) there."""
        capi.call("slamhip_hs_shift", self._h, int(dx), int(dy))

    def origin(self):
        """(ox, oy): the sum of all shifts since creation or the last Reset, in level-0 cells (slamhip_hs_origin)."""
        ox, oy = C.c_int64(), C.c_int64()
        capi.call("slamhip_hs_origin", self._h, C.byref(ox), C.byref(oy))
        return int(ox.value), int(oy.value)

    Origin = property(origin)

    def set_backing(self, tile, max_bytes):
        """The backing store of the scrolling window (slamhip_hs_set_backing): with max_bytes > 0, what a shift scrolls out
        of the window is kept in a device pool of at most max_bytes, in world tiles of tile x tile cells per level (a power
        of two in [8, 256]), and restored when the window returns.  max_bytes = 0 (the default state): off, the pool is freed.
        The setting survives Reset, the tiles do not."""
        capi.call("slamhip_hs_set_backing", self._h, int(tile), C.c_uint64(int(max_bytes)))

    def backing_stats(self):
        """slamhip_hs_backing_stats as a dict: tiles, bytes, capacity_bytes, evicted_cells, restored_cells, dropped_cells
        (host-side sums since backing was switched on), tile, on -- all zero while backing is off."""
        st = capi.BackingStats()
        capi.call("slamhip_hs_backing_stats", self._h, C.byref(st))
        return {name: int(getattr(st, name)) for name, _ in capi.BackingStats._fields_}

    def world_cells(self, level, x0, y0, w, h):
        """The rectangle [x0, x0 + w) x [y0, y0 + h) of `level` in WORLD cells as an (h, w) array of capi.CELL_DTYPE
        (slamhip_hs_world_cells_download): the window's cells from the window, evicted cells from their tiles, LogOddsCell.Reset()
        everywhere else.  Blocking.  Works with backing off: the window in a frame of Reset cells."""
        out = np.empty((int(h), int(w)), capi.CELL_DTYPE)
        capi.call("slamhip_hs_world_cells_download", self._h, int(level), int(x0), int(y0), int(w), int(h), out.ctypes.data_as(C.c_void_p))
        return out

    def world_put(self, level, x0, y0, cells):
        """The inverse of world_cells (slamhip_hs_world_cells_upload): `cells`, an (h, w) array of capi.CELL_DTYPE, replaces the
        rectangle [x0, x0 + w) x [y0, y0 + h) of `level` in WORLD cells -- the window's part in the window (cells and the
        probabilities formed from them), the rest in tile slots when backing is on (a tile is made only where the rectangle holds
        a cell that is not LogOddsCell.Reset()).  -> the number of non-Reset cells dropped: everything outside the window with
        backing off, what found no slot under max_bytes with backing on.  Blocking; never fails for capacity."""
        cells = np.ascontiguousarray(cells, capi.CELL_DTYPE)
        if cells.ndim != 2:
            raise ValueError("world_put: cells must be an (h, w) array")
        dropped = C.c_int64()
        capi.call("slamhip_hs_world_cells_upload", self._h, int(level), int(x0), int(y0), int(cells.shape[1]), int(cells.shape[0]),
                  cells.ctypes.data_as(C.c_void_p), C.byref(dropped))
        return int(dropped.value)

    def world_extends(self, level):
        """(xmax, ymax, xmin, ymin) in WORLD cells of `level` over the cells whose Value != 0 in the window and in every tile (a
        tile's stale copy under the window excluded), reduced on the device (slamhip_hs_world_extends); None if there is none."""
        e = (C.c_int64 * 4)()
        f = C.c_int32()
        capi.call("slamhip_hs_world_extends", self._h, int(level), e, C.byref(f))
        return (int(e[0]), int(e[1]), int(e[2]), int(e[3])) if f.value else None

    WORLD_FORMAT = 1
    _BAND_CELLS = 1 << 26                                           # the bound of one world download / upload

    def _geometry(self):
        return np.array([self.Maps[0].Dimensions[0], self.Maps[0].Dimensions[1], self.NumLevels], np.int64)

    def save_world(self, path):
        """The world as one .npz: per level the rectangle of world_extends as downloaded by world_cells (`rect_<l>` =
        (x0, y0, w, h), all zero for an empty level, and `cells_<l>`), the geometry (`cell_length` of level 0, `geometry` =
        level-0 width, height and the number of levels), the window's `origin`, the `backing` setting (tile, max_bytes; zeros:
        off) and the format `version`.  Blocking."""
        st = self.backing_stats()
        out = {"version": np.int64(self.WORLD_FORMAT), "cell_length": np.float32(self.Maps[0].CellLength), "geometry": self._geometry(),
               "origin": np.array(self.origin(), np.int64), "backing": np.array([st["tile"], st["capacity_bytes"]], np.int64)}
        for l in range(self.NumLevels):
            e = self.world_extends(l)
            if e is None:
                out["rect_%d" % l] = np.zeros(4, np.int64)
                out["cells_%d" % l] = np.zeros((0, 0), capi.CELL_DTYPE)
                continue
            x0, y0, w, h = e[2], e[3], e[0] - e[2] + 1, e[1] - e[3] + 1
            rows = max(1, self._BAND_CELLS // w)
            if w > self._BAND_CELLS:
                raise ValueError("save_world: level %d is %d cells wide, more than one download holds" % (l, w))
            out["rect_%d" % l] = np.array([x0, y0, w, h], np.int64)
            out["cells_%d" % l] = np.concatenate([self.world_cells(l, x0, y0 + r, w, min(rows, h - r)) for r in range(0, h, rows)])
        with open(path, "wb") as f:                                  # (a file object: np.savez would add ".npz" to a bare name)
            np.savez_compressed(f, **out)

    def load_world(self, path, _shift=None):
        """Resume from a world that save_world wrote: the window is shifted to the saved origin, then every level's rectangle is
        put back with world_put.  A file whose version or geometry (cell length, level-0 size, levels) differs from this
        pyramid's is refused (ValueError) before anything changes.  If backing is off here and was on when the world was saved,
        it is switched on with the saved setting once the window has moved, so that what lay outside the window is kept.  -> the cells dropped."""
        with np.load(path) as z:
            if int(z["version"]) != self.WORLD_FORMAT:
                raise ValueError("load_world: format version %d, this library reads %d" % (int(z["version"]), self.WORLD_FORMAT))
            if (np.float32(z["cell_length"]).view(np.uint32) != np.float32(self.Maps[0].CellLength).view(np.uint32)
                    or not np.array_equal(z["geometry"], self._geometry())):
                raise ValueError("load_world: the saved pyramid (cell %r, %s) is not this one (cell %r, %s)"
                                 % (float(z["cell_length"]), z["geometry"].tolist(), self.Maps[0].CellLength, self._geometry().tolist()))
            origin = tuple(int(v) for v in z["origin"])
            backing = tuple(int(v) for v in z["backing"])
            rects = [tuple(int(v) for v in z["rect_%d" % l]) for l in range(self.NumLevels)]
            cells = [np.ascontiguousarray(z["cells_%d" % l], capi.CELL_DTYPE) for l in range(self.NumLevels)]
        g = 1 << (self.NumLevels - 1)
        step = (1 << 30) // g * g                                    # (slamhip_hs_shift takes 32-bit moves)
        while self.origin() != origin:
            ox, oy = self.origin()
            (_shift or self.shift)(max(-step, min(step, origin[0] - ox)), max(-step, min(step, origin[1] - oy)))
        if backing[1] > 0 and not self.backing_stats()["on"]:        # (after the move: a fresh pyramid makes no tiles of its empty window)
            self.set_backing(*backing)
        dropped = 0
        for l, ((x0, y0, w, h), c) in enumerate(zip(rects, cells)):
            if w == 0 or h == 0:
                continue
            rows = max(1, self._BAND_CELLS // w)
            for r in range(0, h, rows):
                dropped += self.world_put(l, x0, y0 + r, c[r:r + rows])
        return dropped

    def SetUpdateFactorFree(self, factor):
        self._free = float(factor)
        capi.call("slamhip_hs_set_factors", self._h, C.c_float(factor), C.c_float(getattr(self, "_occ", 0.9)))

    def SetUpdateFactorOccupied(self, factor):
        self._occ = float(factor)
        capi.call("slamhip_hs_set_factors", self._h, C.c_float(getattr(self, "_free", 0.4)), C.c_float(factor))

    def lattice_search(self, scan, level, centre, nx, ny, n_theta, dtheta, scores=False):
        """The pose-lattice search (slamhip_hs_lattice_search; no reference counterpart): `scan` scored against the occupancy
        grid of `level` at every node of the lattice -- translations ix in [-nx, nx], iy in [-ny, ny] cells of that level around
        `centre` (a pose in the window's frame), headings centre[2] + k * dtheta, k < n_theta.  -> (keys, scores | None): keys
        (n_theta,) uint64, per heading the best node (decode_lattice_key); scores the (n_theta, 2 ny + 1, 2 nx + 1) int32 volume
        when asked for.  Blocking, behind everything already enqueued.  scan = None: the scan already set."""
        if scan is not None:
            self.set_scan(scan)
        spec = capi.lattice_spec(level, centre, nx, ny, n_theta, dtheta)
        keys = np.zeros(int(n_theta), np.uint64)
        vol = np.zeros((int(n_theta), 2 * int(ny) + 1, 2 * int(nx) + 1), np.int32) if scores else None
        capi.call("slamhip_hs_lattice_search", self._h, C.byref(spec), keys.ctypes.data_as(C.POINTER(C.c_uint64)),
                  capi.iptr(vol) if scores else None)
        return keys, vol

    def world_lattice_search(self, scan, level, centre, nx, ny, n_theta, dtheta, scores=False):
        """lattice_search over the WORLD (slamhip_hs_world_lattice_search): a node's cell outside the window is the cell of the
        tile that holds it (LogOddsCell.Reset() where none does) instead of nothing, so the lattice may reach anywhere the window
        has ever been -- `centre` stays a pose in the window's frame and may lie outside the window.  Arguments and results as
        lattice_search; with backing off, or no tile on `level`, the results are lattice_search's bit for bit."""
        if scan is not None:
            self.set_scan(scan)
        spec = capi.lattice_spec(level, centre, nx, ny, n_theta, dtheta)
        keys = np.zeros(int(n_theta), np.uint64)
        vol = np.zeros((int(n_theta), 2 * int(ny) + 1, 2 * int(nx) + 1), np.int32) if scores else None
        capi.call("slamhip_hs_world_lattice_search", self._h, C.byref(spec), keys.ctypes.data_as(C.POINTER(C.c_uint64)),
                  capi.iptr(vol) if scores else None)
        return keys, vol

    def lattice_search_bnb(self, scan, level, centre, nx, ny, n_theta, dtheta, top, world=False, max_blocks=0):
        """lattice_search's (world=True: world_lattice_search's) keys by branch and bound (slamhip_hs_lattice_search_bnb): blocks of
        2^top x 2^top translations are bounded from above through pooled maxima of the class map and only those that can still hold
        a heading's best node are split, so the lattice may have far more than lattice_search's 2^26 nodes; the keys are the
        exhaustive search's bit for bit.  max_blocks: the capacity of a level's frontier (0: 2^26).  -> (keys, info): keys
        (n_theta,) uint64, info a capi.BNB_INFO record (blocks and survivors per height, blocks evaluated).  There is no score
        volume.  Blocking, one wait per height.  scan = None: the scan already set."""
        if scan is not None:
            self.set_scan(scan)
        spec = capi.bnb_spec(level, centre, nx, ny, n_theta, dtheta, top, world, max_blocks)
        keys = np.zeros(int(n_theta), np.uint64)
        info = capi.BnbInfo()
        capi.call("slamhip_hs_lattice_search_bnb", self._h, C.byref(spec), keys.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(info))
        return keys, capi.bnb_info(info)

    def lattice_node_pose(self, level, centre, nx, ny, n_theta, dtheta, k, flat):
        """The pose of node (k, flat) of that lattice, in the window's frame (slamhip_hs_lattice_node_pose; host code)."""
        spec = capi.lattice_spec(level, centre, nx, ny, n_theta, dtheta)
        out = np.empty(3, np.float32)
        capi.call("slamhip_hs_lattice_node_pose", self._h, C.byref(spec), int(k), int(flat), capi.fptr(out))
        return out

    def set_scan(self, scan):
        org = capi.f32(scan.Pose[:2])
        capi.call("slamhip_hs_set_scan", self._h, capi.fptr(scan.Points), scan.Points.shape[0], capi.fptr(org))
        self._scan_set = (scan.Points.shape[0], org.copy())

    def trace(self, poses, level, world=False, beams=False, scan=None):
        """The beam trace (slamhip_hs_trace; no reference counterpart): what the map of `level` holds ALONG every beam of the scan
        from each of the B `poses` ((B, 3), window frame) -- the grid update's own line from the sensor cell to the beam's end cell,
        the class of every cell on it.  -> (summaries, beams | None): summaries (B,) of capi.TRACE_SUMMARY; beams the (B, n_points)
        capi.TRACE_BEAM records when asked for (B * n_points <= 2^20).  world=True: a cell outside the window is the cell of the tile
        that holds it instead of nothing.  Blocking, behind everything already enqueued; it changes nothing.  scan = None: the scan
        already set through this object."""
        if scan is not None:
            self.set_scan(scan)
        p = capi.f32(poses, (-1, 3))
        sums = np.zeros(p.shape[0], capi.TRACE_SUMMARY)
        rec = None
        if beams:
            if self._scan_set is None:
                raise ValueError("trace: beams=True needs the scan set through this object (set_scan, or scan=)")
            rec = np.zeros((p.shape[0], self._scan_set[0]), capi.TRACE_BEAM)
        capi.call("slamhip_hs_trace", self._h, int(level), capi.fptr(p), p.shape[0], 1 if world else 0, sums.ctypes.data_as(C.c_void_p),
                  rec.ctypes.data_as(C.c_void_p) if beams else None)
        return sums, rec

    def view_gain(self, poses, level, reach, commit=-1, scan=None):
        """The view gain (slamhip_hs_view_gain; no reference counterpart): the DISTINCT cells of `level` the scan's beams see from each
        of the B `poses` ((B, 3), window frame, B <= 4096), no further than `reach` cells -> (B,) capi.VIEW_SUMMARY records: n_seen
        and its split by class, n_new and n_new_unknown against the covered layer as it was before the call.  commit: -1 nothing,
        -2 every pose's cells join the layer, an index that pose's.  Blocking; it changes nothing of the map."""
        if scan is not None:
            self.set_scan(scan)
        p = capi.f32(poses, (-1, 3))
        out = np.zeros(p.shape[0], capi.VIEW_SUMMARY)
        capi.call("slamhip_hs_view_gain", self._h, int(level), int(reach), capi.fptr(p), p.shape[0], int(commit), out.ctypes.data_as(C.c_void_p))
        return out

    def view_select(self, poses, level, reach, k, mode=0, min_gain=1, scan=None):
        """The greedy choice of views (slamhip_hs_view_select): up to k <= 64 of the B `poses`, each round the pose that adds the most
        new cells (mode 0) or new unknown cells (mode 1) to the covered layer, ties to the lowest index, until the best adds fewer
        than min_gain.  -> (order, gain): the chosen pose indices in the order of choice and their gains.  The chosen views are
        committed to the layer."""
        if scan is not None:
            self.set_scan(scan)
        p = capi.f32(poses, (-1, 3))
        order = np.zeros(int(k), np.int32); gain = np.zeros(int(k), np.int32); n = C.c_int32()
        capi.call("slamhip_hs_view_select", self._h, int(level), int(reach), int(mode), int(min_gain), capi.fptr(p), p.shape[0], int(k),
                  capi.iptr(order), capi.iptr(gain), C.byref(n))
        assert (order[n.value:] == -1).all() and not gain[n.value:].any()
        return order[:n.value].copy(), gain[:n.value].copy()

    def covered(self, level, bits=None, clear=False):
        """The covered layer of `level` (slamhip_hs_view_get_covered) as an (h, capi.view_words(w)) uint32 bitmap (capi.view_unpack
        makes booleans of it).  bits: set the layer first (slamhip_hs_view_set_covered), from such a bitmap; clear=True: set it empty."""
        w, h = (int(v) for v in self.Maps[level].Dimensions)
        if bits is not None or clear:
            b = None if bits is None else np.ascontiguousarray(bits, np.uint32).reshape(h, capi.view_words(w))
            capi.call("slamhip_hs_view_set_covered", self._h, int(level), None if b is None else b.ctypes.data_as(C.c_void_p))
        out = np.empty((h, capi.view_words(w)), np.uint32)
        capi.call("slamhip_hs_view_get_covered", self._h, int(level), out.ctypes.data_as(C.c_void_p))
        return out

    def view_clear(self):
        """Free every block of the view gain, the covered layer too (slamhip_hs_view_clear)."""
        capi.call("slamhip_hs_view_clear", self._h)

    def distance_field(self, level, rect, site_mask=2, radius=32, world=False):
        """The distance field of `level` (slamhip_hs_distance_field; no reference counterpart): for every cell of rect = (x, y, w, h),
        window-frame cells of the level, the squared cell distance to the nearest site, capped at radius^2 -> (h, w) uint16.  A site
        is a cell whose class is selected by site_mask: bit 0 unknown, bit 1 occupied, bit 2 free (2: distance to obstacles, 1: to the
        unknown).  radius in [1, 255].  world=True: a cell outside the window is the cell of the tile that holds it.  rect may lie
        anywhere.  Blocking, behind everything already enqueued; it changes nothing."""
        x, y, w, h = (int(v) for v in rect)
        out = np.empty((max(h, 0), max(w, 0)), np.uint16)
        capi.call("slamhip_hs_distance_field", self._h, int(level), 1 if world else 0, int(site_mask), int(radius), x, y, w, h,
                  out.ctypes.data_as(C.c_void_p))
        return out

    def distance_score(self, poses, level, site_mask=2, radius=32, world=False, points=False, scan=None):
        """The end-point distance score (slamhip_hs_distance_score): for each of the B `poses` ((B, 3), window frame) the field's
        value at the end cell of every scan point.  -> (summaries, points | None): summaries (B,) of capi.DISTANCE_SUMMARY
        (sum_d2 / n_counted is the mean squared cell distance of the scan's end points from the sites); points the (B, n_points)
        uint16 values when asked for, capi.DISTANCE_IGNORED for an ignored point (B * n_points <= 2^22).  scan = None: the scan
        already set through this object."""
        if scan is not None:
            self.set_scan(scan)
        p = capi.f32(poses, (-1, 3))
        sums = np.zeros(p.shape[0], capi.DISTANCE_SUMMARY)
        rec = None
        if points:
            if self._scan_set is None:
                raise ValueError("distance_score: points=True needs the scan set through this object (set_scan, or scan=)")
            rec = np.zeros((p.shape[0], self._scan_set[0]), np.uint16)
        capi.call("slamhip_hs_distance_score", self._h, int(level), 1 if world else 0, int(site_mask), int(radius), capi.fptr(p), p.shape[0],
                  sums.ctypes.data_as(C.c_void_p), rec.ctypes.data_as(C.c_void_p) if points else None)
        return sums, rec

    def nearest_field(self, level, rect, site_mask=2, radius=32, world=False):
        """The nearest-site field of `level` (slamhip_hs_nearest_field; no reference counterpart): for every cell of rect = (x, y, w,
        h), window-frame cells of the level, the offset (dx, dy) to the nearest site with dx^2 + dy^2 < radius^2 -- ties to the
        smaller row, then the smaller column -- -> (h, w, 2) int16, capi.NEAREST_NONE twice where there is none.  site_mask, radius,
        world and rect as distance_field: dx^2 + dy^2 is that field wherever it is below radius^2.  Blocking, behind everything
        already enqueued; it changes nothing."""
        x, y, w, h = (int(v) for v in rect)
        out = np.empty((max(h, 0), max(w, 0), 2), np.int16)
        capi.call("slamhip_hs_nearest_field", self._h, int(level), 1 if world else 0, int(site_mask), int(radius), x, y, w, h,
                  out.ctypes.data_as(C.c_void_p))
        return out

    def nearest_pairs(self, poses, level, site_mask=2, radius=32, world=False, pairs=False, scan=None):
        """The scan-to-map pairs (slamhip_hs_nearest_pairs): for each of the B `poses` ((B, 3), window frame) the nearest site of the
        end cell of every scan point.  -> (summaries, pairs | None): summaries (B,) of capi.PAIR_SUMMARY -- counts, sum_d2 and the
        sums of e, q and their products over the matched points, what align_step needs; pairs the (B, n_points, 2) int16 offsets
        when asked for, capi.NEAREST_IGNORED twice for an ignored point, capi.NEAREST_NONE twice for a counted one without a site
        within the radius (B * n_points <= 2^22).  scan = None: the scan already set through this object."""
        if scan is not None:
            self.set_scan(scan)
        p = capi.f32(poses, (-1, 3))
        sums = np.zeros(p.shape[0], capi.PAIR_SUMMARY)
        rec = None
        if pairs:
            if self._scan_set is None:
                raise ValueError("nearest_pairs: pairs=True needs the scan set through this object (set_scan, or scan=)")
            rec = np.zeros((p.shape[0], self._scan_set[0], 2), np.int16)
        capi.call("slamhip_hs_nearest_pairs", self._h, int(level), 1 if world else 0, int(site_mask), int(radius), capi.fptr(p), p.shape[0],
                  sums.ctypes.data_as(C.c_void_p), rec.ctypes.data_as(C.c_void_p) if pairs else None)
        return sums, rec

    def align_step(self, pose, level, summary):
        """align_step of a window-frame `pose` on `level` from its nearest_pairs summary -> (pose', dtheta, (tx, ty) in cells)."""
        return align_step(pose, summary, np.float32(1.0) / np.float32(self.Maps[level].CellLength))

    def frontiers(self, level, min_cells=1, max_clusters=256, world=False, labels_rect=None):
        """The frontier clusters of `level` (slamhip_hs_frontiers; no reference counterpart): the free cells that touch the unknown,
        grouped under 8-connectivity.  -> (summary, clusters[, labels]): a capi.FRONTIER_SUMMARY record; the kept clusters (n_cells >=
        min_cells) as capi.FRONTIER_CLUSTER records, largest first, at most max_clusters, in window-frame cells of the level; with
        labels_rect = (x, y, w, h), any position, the (h, w) int32 labels of its cells (the flat index of the cluster's seed in M, -1
        where the cell is no frontier cell).  world=True: a cell outside the window is the cell of the tile that holds it.  Blocking,
        behind everything already enqueued; it changes nothing."""
        rect = (0, 0, 0, 0) if labels_rect is None else tuple(int(v) for v in labels_rect)
        shape = None if labels_rect is None else (max(rect[3], 0), max(rect[2], 0))
        return capi.frontiers_call("slamhip_hs_frontiers", [self._h, int(level), 1 if world else 0], min_cells, max_clusters, shape, rect)

    def nav_field(self, level, sources, clearance=0, site_mask=2, max_cost=0, world=False, goals=None, n_paths=0, max_path_cells=1,
                  rect=None, want_cost=True, want_dir=True):
        """The cost-to-go field of `level` (slamhip_hs_nav_field; no reference counterpart): the least 5-7 chamfer cost from the
        `sources` ((S, 2) window-frame cells) to every traversable cell -- free, and with clearance >= 1 more than `clearance` cells
        from every site (site_mask 2: obstacles, 3: obstacles or the unknown) -- over moves that cut no corner.  goals: (G, 4)
        rectangles {x_min, y_min, x_max, y_max} (a frontier cluster's box, grown as the caller sees fit); the first n_paths get
        their cell path, at most max_path_cells cells each.  rect = (x, y, w, h), any position: the costs / dirs of its cells.
        -> capi.nav_call's dict: summary, goals, paths, path_cells[, cost, dir]; an unreached cell costs capi.NAV_UNREACHED.
        Blocking, behind everything already enqueued; it changes nothing."""
        spec = capi.nav_spec(level, world, site_mask, clearance, max_cost)
        return capi.nav_call("slamhip_hs_nav_field", [self._h, spec.ctypes.data_as(C.c_void_p)], sources, goals, n_paths, max_path_cells, rect,
                             want_cost, want_dir)

    def rollouts(self, level, sources, start_pose, dt, cmds, hold=1, body=None, clearance=0, site_mask=2, max_cost=0, world=False):
        """Command rollouts over the cost-to-go field of `level` (slamhip_hs_rollouts; no reference counterpart): each of the B
        sequences cmds[b] ((B, n_cmd, 2) pairs (v, w), each held for `hold` steps of dt) is rolled forward from start_pose
        (window frame) by explicit Euler steps and cut at the first pose whose centre cell is not reached by the field of
        `sources` ((S, 2) window-frame cells, the goal) or one of whose `body` points ((P, 2) metres, robot frame) lies on an
        untraversable cell.  -> (results, summary): B capi.ROLLOUT_RESULT records (n_free, min_step, end_cost, min_cost, x, y, theta)
        and a capi.ROLLOUT_SUMMARY record (the field's summary under "nav", start_cost, n_complete, key_end, key_min;
        capi.rollout_key decodes a key).  Blocking, behind everything already enqueued; it changes nothing."""
        spec = capi.nav_spec(level, world, site_mask, clearance, max_cost)
        return capi.rollouts_call("slamhip_hs_rollouts", [self._h, spec.ctypes.data_as(C.c_void_p)], sources, start_pose, dt, body, cmds, hold)

    def mcl_set(self, poses):
        """The particle set of the localisation filter (slamhip_hs_mcl_set): (N, 3) poses in the window's frame, N <= 65536; every
        accumulated cost becomes 0.  It replaces any previous set."""
        p = capi.f32(poses, (-1, 3))
        capi.call("slamhip_hs_mcl_set", self._h, p.ctypes.data_as(C.c_void_p), p.shape[0])
        self._mcl_n = p.shape[0]

    def mcl_step(self, spec, scan=None):
        """One localisation step on the particle set (slamhip_hs_mcl_step; no reference counterpart): predict by spec's odometry
        increment with noise, weigh by the scan against the distance field, resample when the effective sample size falls below
        spec's n_eff_min -- all on the device.  spec: capi.mcl_spec's record.  -> a capi.MCL_SUMMARY record (capi.mcl_mean forms the
        weighted-mean pose and n_eff).  scan = None: the scan already set through this object.  Blocking; it changes nothing of the
        map."""
        if scan is not None:
            self.set_scan(scan)
        out = np.zeros(1, capi.MCL_SUMMARY)
        capi.call("slamhip_hs_mcl_step", self._h, spec.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
        return out[0]

    def merge_set_source(self, level, ax, ay, cells):
        """The source map of the merge (slamhip_hs_merge_set_source; no reference counterpart): `cells`, an (h, w) array of
        capi.CELL_DTYPE whose first element is source-frame cell (ax, ay) of a grid with `level`'s cell length -- what GetCells or
        world_cells of any pyramid gives.  It stays in device memory until the next merge_set_source, merge_clear_source or Reset."""
        c = np.ascontiguousarray(cells, capi.CELL_DTYPE)
        if c.ndim != 2:
            raise ValueError("merge_set_source: cells must be an (h, w) array")
        capi.call("slamhip_hs_merge_set_source", self._h, int(level), int(ax), int(ay), c.shape[1], c.shape[0], c.ctypes.data_as(C.c_void_p))

    def merge_score(self, poses):
        """Rate candidate alignments of the source with its level (slamhip_hs_merge_score): `poses` (B, 3), each the origin and heading
        of the SOURCE frame in the window's frame, B <= 4096.  -> (B,) capi.MERGE_REPORT records: joint[3 * cd + cs] counts the
        destination cells by their class and their source cell's (0 neither, 1 occupied, 2 free), n_unsourced those with no source
        cell.  Blocking; it changes nothing."""
        p = capi.f32(poses, (-1, 3))
        out = np.zeros(p.shape[0], capi.MERGE_REPORT)
        capi.call("slamhip_hs_merge_score", self._h, capi.fptr(p), p.shape[0], out.ctypes.data_as(C.c_void_p))
        return out

    def merge_apply(self, pose, rule=capi.MERGE_ADD, value_limit=50.0):
        """Fuse the source into its level at `pose` on the device (slamhip_hs_merge_apply): rule capi.MERGE_ADD (log-odds added, cut to
        +-value_limit), MERGE_FILL (unknown cells only) or MERGE_REPLACE.  -> a capi.MERGE_REPORT record.  Blocking.  The other levels,
        the tiles of the backing store and cells outside the window are not touched."""
        out = np.zeros(1, capi.MERGE_REPORT)
        capi.call("slamhip_hs_merge_apply", self._h, capi.fptr(capi.f32(pose, (3,))), int(rule), C.c_float(value_limit), out.ctypes.data_as(C.c_void_p))
        return out[0]

    def merge_clear_source(self):
        """No source from here on (slamhip_hs_merge_clear_source)."""
        capi.call("slamhip_hs_merge_clear_source", self._h)

    def _hough(self, name, handle, level, slot, world, site_mask, T, q, H):
        info, HS, Hm = capi.hough_call(name, handle, level, slot, world, site_mask, T, q, H)
        if not hasattr(self, "_hough_info"):
            self._hough_info = {}
        self._hough_info[int(slot)] = dict(info, T=int(T), q=int(q), spectrum=HS)
        return info, HS, Hm

    def hough(self, level, slot=0, world=False, site_mask=2, T=360, q=1, H=False):
        """The Hough transform of a map into a slot (slamhip_hs_hough; no reference counterpart): slot 0 the map of `level` (the
        window's, or with `world` the world rectangle's), slot 1 the merge source (level must be its level).  T angles (a multiple of
        4), bins of 2^q cells.  -> (info, HS, H): info a dict of w, h, x0, y0, D, N, n_sites; HS (T,) uint64 the spectrum; H (T, N)
        uint32 the votes if asked for, else None.  Blocking; it changes nothing of the map."""
        return self._hough("slamhip_hs_hough", self._h, level, slot, world, site_mask, T, q, H)

    def _hough_both(self):
        """What the last fills through this object reported, per slot -- only to size the result arrays: whether the slots ARE filled
        is the library's to say (SLAMHIP_ERR_STATE).  Unknown: the largest T, and no XC arrays."""
        info = getattr(self, "_hough_info", {})
        unknown = {"T": capi.HOUGH_MAX_T, "N": 0}
        return info.get(0, unknown), info.get(1, unknown)

    def hough_rotation(self):
        """The rotation scores CC (T,) uint64 of the two filled slots (slamhip_hs_hough_rotation): CC peaks where the source frame is
        turned by m pi / T (mod pi) in the destination's frame."""
        d, _ = self._hough_both()
        cc = np.zeros(d["T"], np.uint64)
        capi.call("slamhip_hs_hough_rotation", self._h, cc.ctypes.data_as(C.c_void_p))
        return cc

    def hough_shifts(self, pairs, xc=False):
        """The row correlations of pairs (P, 2) of (m, k) (slamhip_hs_hough_shifts) -> ((P,) capi.HOUGH_SHIFT records, XC (P, N_d + N_s
        - 1) uint64 if asked for, else None; entry d + N_s - 1 is the shift d)."""
        d, s = self._hough_both()
        return capi.hough_shifts_call("slamhip_hs_hough_shifts", self._h, pairs, d["N"] + s["N"] - 1 if xc and d["N"] and s["N"] else None)

    def hough_clear(self):
        """Free the blocks of the Hough transform (slamhip_hs_hough_clear); both slots are empty afterwards."""
        capi.call("slamhip_hs_hough_clear", self._h)
        self._hough_info = {}

    def SigConfigure(self, scale, n_ring, ring_cells):
        """Set the spec of the scan signatures and EMPTY the keyframe store (slamhip_hs_sig_configure; no reference counterpart):
        n_ring rings of ring_cells cells each, 64 sectors, `scale` cells per metre -- the caller's choice, unrelated to any level."""
        sp = capi.sig_spec(scale, n_ring, ring_cells)
        capi.call("slamhip_hs_sig_configure", self._h, sp.ctypes.data_as(C.c_void_p))
        self._sig_rings = int(n_ring)

    def _sig_n_ring(self):
        """n_ring of the last SigConfigure through this object -- only to size the result arrays; without one the largest."""
        return getattr(self, "_sig_rings", capi.SIG_MAX_RINGS)

    def SigAdd(self, pose):
        """The signature of the scan set_scan took, appended to the store with `pose` (opaque to the library; slamhip_hs_sig_add)
        -> (index, sig (n_ring,) uint64, a capi.SIG_INFO record)."""
        return capi.sig_add_call("slamhip_hs_sig_add", self._h, pose, self._sig_n_ring())

    def SigAddScans(self, scans, poses):
        """Many scans of a log appended in ONE launch (slamhip_hs_sig_add_scans): scans a list of (n_i, 2) point arrays, poses (B, 3)
        -> the first new index.  The scan that set_scan took is not touched."""
        pts = [capi.f32(s, (-1, 2)) for s in scans]
        off = np.zeros(len(pts) + 1, np.int32)
        off[1:] = np.cumsum([p.shape[0] for p in pts])
        xy = np.ascontiguousarray(np.concatenate(pts, axis=0)) if pts and off[-1] else np.zeros((0, 2), np.float32)
        p = capi.f32(poses, (-1, 3))
        assert p.shape[0] == len(pts)
        first = C.c_int32()
        capi.call("slamhip_hs_sig_add_scans", self._h, capi.fptr(xy) if xy.shape[0] else None, off.ctypes.data_as(C.c_void_p), len(pts), capi.fptr(p),
                  C.byref(first))
        return first.value

    def SigCount(self):
        n = C.c_int32()
        capi.call("slamhip_hs_sig_count", self._h, C.byref(n))
        return n.value

    def SigQuery(self, B=capi.SIG_MAX_HITS, first=0, last=None):
        """The scan set_scan took against the keyframes [first, last) over all 64 headings (slamhip_hs_sig_query); nothing is appended
        -> (hits, the query's sig, its info): hits capi.SIG_HIT_DTYPE records, higher score first, then lower index."""
        return capi.sig_query_call("slamhip_hs_sig_query", self._h, first, self.SigCount() if last is None else last, B, self._sig_n_ring())

    def SigSelf(self, min_gap, first=0, last=None):
        """Every keyframe i of [first, last) against the keyframes [first, i - min_gap] (slamhip_hs_sig_self) -> one hit per keyframe,
        index -1 where that range is empty."""
        return capi.sig_self_call("slamhip_hs_sig_self", self._h, first, self.SigCount() if last is None else last, min_gap)

    def SigDownload(self, first=0, n=None):
        """Keyframes [first, first + n) out of the store (slamhip_hs_sig_download) -> (sig (n, n_ring) uint64 key-major, poses (n, 3))."""
        n = self.SigCount() - int(first) if n is None else int(n)
        sig = np.zeros((max(n, 0), self._sig_n_ring()), np.uint64); poses = np.zeros((max(n, 0), 3), np.float32)
        capi.call("slamhip_hs_sig_download", self._h, int(first), n, sig.ctypes.data_as(C.c_void_p), poses.ctypes.data_as(C.c_void_p))
        return sig, poses

    def SigUpload(self, sig, poses):
        """Keyframes appended from what SigDownload gave (slamhip_hs_sig_upload); the library counts the popcounts itself."""
        s = np.ascontiguousarray(sig, np.uint64).reshape(-1, self._sig_n_ring()); p = capi.f32(poses, (-1, 3))
        assert s.shape[0] == p.shape[0]
        capi.call("slamhip_hs_sig_upload", self._h, s.shape[0], s.ctypes.data_as(C.c_void_p), capi.fptr(p))

    def SigSetPoses(self, poses, first=0):
        """Overwrite the stored poses of keyframes [first, first + len(poses)) (slamhip_hs_sig_set_poses; host-side, no launch)."""
        p = capi.f32(poses, (-1, 3))
        capi.call("slamhip_hs_sig_set_poses", self._h, int(first), p.shape[0], capi.fptr(p) if p.shape[0] else None)

    def PgSet(self, poses, fixed, ij, z, w):
        """Take a pose graph, replacing any earlier one (slamhip_hs_pg_set; no reference counterpart): poses (N, 3), fixed (N,) bools
        or None (node 0 alone), ij (E, 2), z and w (E, 3), all binary64."""
        p, fx, e, zz, ww = capi.pg_graph(poses, fixed, ij, z, w)
        assert e.shape[0] == zz.shape[0] == ww.shape[0] and (fx is None or fx.shape[0] == p.shape[0])
        capi.call("slamhip_hs_pg_set", self._h, capi._vp(p), capi._vp(fx), p.shape[0], capi._vp(e), capi._vp(zz), capi._vp(ww), e.shape[0])
        self._pg_sizes = (p.shape[0], e.shape[0])

    PG_PRECOND = {"jacobi": "slamhip_hs_pg_relax", "tri": "slamhip_hs_pg_relax_tri"}

    def PgRelax(self, spec, precond="jacobi"):
        """spec["n_outer"] Gauss-Newton steps from the poses as they stand -> (iters capi.PG_ITER records, chi2 after the last step).
        precond: "jacobi" (slamhip_hs_pg_relax, a node's own 3 x 3 block) or "tri" (slamhip_hs_pg_relax_tri, the odometry chain's
        block-tridiagonal part of H: the one for a chain of keyframes closed by a few loops)."""
        if precond not in self.PG_PRECOND:
            raise ValueError("precond = %r: one of %s" % (precond, sorted(self.PG_PRECOND)))
        iters = np.zeros(max(int(spec["n_outer"][0]), 1), capi.PG_ITER); fin = C.c_double(0.0)
        capi.call(self.PG_PRECOND[precond], self._h, spec.ctypes.data_as(C.c_void_p), iters.ctypes.data_as(C.c_void_p), C.byref(fin))
        return iters[:int(spec["n_outer"][0])].copy(), fin.value

    def PgRelaxLM(self, spec, robust=None):
        """Damped and robust relaxation from the poses as they stand (slamhip_hs_pg_relax_lm, rules R1 - R4): spec a capi.pg_lm_spec
        record, robust (E,) bools -- the edges the spec's kernel applies to -- or None for all of them
        -> (iters capi.PG_LM_ITER records, one per attempt made, F at the final poses, f (E,): every edge's factor there)."""
        E = getattr(self, "_pg_sizes", (1, 0))[1]
        return capi.pg_relax_lm_call("slamhip_hs_pg_relax_lm", (self._h,), E, spec, robust)

    def PgMarginals(self, pairs, spec, precond="tri"):
        """Marginal covariances at the poses as they stand (slamhip_hs_pg_marginals, rules M1 - M5): pairs (P, 2) node indices (n, m);
        spec a capi.pg_marg_spec record, or None for 200 iterations at tol 1e-9 with `precond` ("jacobi" / "tri"; a record has its own)
        -> (blocks (P, 3, 3) float64: Sigma[n_p][m_p], +0 where either node is fixed; cols capi.PG_MARG_COL (R,): a record per
        right-hand side; info: a capi.PG_MARG_INFO record).  Neither the poses nor a later PgRelax* change."""
        if spec is None:
            spec = capi.pg_marg_spec(200, precond=precond)
        return capi.pg_marginals_call("slamhip_hs_pg_marginals", (self._h,), spec, pairs)

    def PgTriApply(self, lam, rhs):
        """z = T^-1 rhs at the poses as they stand (slamhip_hs_pg_tri_apply): the odometry-chain preconditioner alone, lambda = lam on
        the diagonal, rhs (N, 3) -> (N, 3) float64."""
        N = getattr(self, "_pg_sizes", (1, 0))[0]
        b = np.array(rhs, np.float64).reshape(-1, 3)
        assert b.shape[0] == N
        out = np.zeros_like(b)
        capi.call("slamhip_hs_pg_tri_apply", self._h, float(lam), b.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
        return out

    def PgGet(self):
        """The graph's poses as they stand (slamhip_hs_pg_get) -> (N, 3) float64."""
        N = getattr(self, "_pg_sizes", (1, 0))[0]
        p = np.zeros((N, 3), np.float64)
        capi.call("slamhip_hs_pg_get", self._h, p.ctypes.data_as(C.c_void_p), N)
        return p

    def PgResiduals(self):
        """Rule 3 at the poses as they stand (slamhip_hs_pg_residuals) -> (r (E, 3), chi2_e (E,)) float64."""
        E = getattr(self, "_pg_sizes", (1, 0))[1]
        r = np.zeros((max(E, 1), 3), np.float64); c2 = np.zeros(max(E, 1), np.float64)
        capi.call("slamhip_hs_pg_residuals", self._h, r.ctypes.data_as(C.c_void_p), c2.ctypes.data_as(C.c_void_p))
        return r[:E].copy(), c2[:E].copy()

    def PgClear(self):
        """Free the blocks of the pose graph (slamhip_hs_pg_clear)."""
        capi.call("slamhip_hs_pg_clear", self._h)
        self.__dict__.pop("_pg_sizes", None)

    def ScansAdd(self, scan=None):
        """Append a scan to the device-resident scan store (slamhip_hs_scans_add; no reference counterpart): a ScanCloud (its points
        and Pose[:2] as the scan origin), or None for the scan that is set on this pyramid -> its index."""
        k = C.c_int32()
        if scan is None:
            capi.call("slamhip_hs_scans_add", self._h, None, 0, None, C.byref(k))
        else:
            pts = capi.f32(scan.Points, (-1, 2)); org = capi.f32(scan.Pose[:2])
            keep = np.zeros((1, 2), np.float32) if pts.shape[0] == 0 else pts          # (an empty scan still needs a non-NULL xy)
            capi.call("slamhip_hs_scans_add", self._h, capi._vp(keep), pts.shape[0], capi._vp(org), C.byref(k))
        return k.value

    def ScansCount(self):
        n = C.c_int32()
        capi.call("slamhip_hs_scans_count", self._h, C.byref(n))
        return n.value

    def ScansGet(self, k):
        """Scan k of the store (slamhip_hs_scans_info, _scans_download) -> (points (n, 2) float32, origin (2,) float32)."""
        n = C.c_int32(); org = np.zeros(2, np.float32)
        capi.call("slamhip_hs_scans_info", self._h, int(k), C.byref(n), capi._vp(org))
        pts = np.zeros((max(n.value, 1), 2), np.float32)
        capi.call("slamhip_hs_scans_download", self._h, int(k), capi._vp(pts), n.value)
        return pts[:n.value].copy(), org

    def ScansClear(self):
        """Free the scan store (slamhip_hs_scans_clear)."""
        capi.call("slamhip_hs_scans_clear", self._h)

    def Render(self, poses, first=0, last=None, keep=False):
        """Draw scans [first, last) of the scan store into the pyramid at `poses` ((last - first, 3), window frame), as that many
        set_scan + UpdateByScan calls in order would, in one call (slamhip_hs_render).  Without keep the map is cleared first."""
        last = self.ScansCount() if last is None else int(last)
        p = capi.f32(poses, (-1, 3)) if last > first else np.zeros((1, 3), np.float32)
        assert last <= first or p.shape[0] == last - first
        capi.call("slamhip_hs_render", self._h, int(first), last, capi._vp(p), capi.RENDER_KEEP if keep else 0)

    def RenderWorld(self, poses, first=0, last=None, keep=False):
        """Render, into the whole world behind the window (slamhip_hs_render_world; set_backing first): lines that leave the window
        are drawn into the backing store's tiles, which are taken as needed; without keep the window is cleared and the tiles are
        dropped first.  SlamhipError ERR_NOMEM, nothing changed, if the tiles do not fit the backing store's max_bytes."""
        last = self.ScansCount() if last is None else int(last)
        p = capi.f32(poses, (-1, 3)) if last > first else np.zeros((1, 3), np.float32)
        assert last <= first or p.shape[0] == last - first
        capi.call("slamhip_hs_render_world", self._h, int(first), last, capi._vp(p), capi.RENDER_KEEP if keep else 0)

    def scans_match(self, spec, pairs):
        """Match stored scans pairwise (slamhip_hs_scans_match; no reference counterpart): spec a capi.scanmatch_spec record, pairs
        (ref, query, guess) tuples or a capi.SCAN_PAIR array, the guess being the query's pose in the reference's frame -> a
        capi.SCANMATCH_RESULT array, one record per pair."""
        return capi.scans_match_call("slamhip_hs_scans_match", self._h, spec, pairs)

    @staticmethod
    def scans_edges(spec, pairs, results):
        """The results of scans_match as pose-graph edges (slamhip_hs_scans_edges; host only) -> (z (n, 3), w (n, 3), valid (n,))."""
        return capi.scans_edges(spec, pairs, results)

    def LoopsConsistent(self, poses, ij, z, w, spec, use=None, adj=False):
        """The largest mutually consistent set of loop edges found (slamhip_hs_loops_consistent; no reference counterpart): poses
        (N, 3) the keyframe chain in odometry order, ij (L, 2), z and w (L, 3) as PgSet takes them, spec a capi.loops_spec record, use
        (L,) bools or None (all) -> dict(keep (L,) bool, deg (L,) int32, info a capi.LOOPS_INFO record, adj the consistency matrix as
        (L, ceil(L / 64)) uint64 with adj=True, else None).  Reads and writes nothing of the map, the stores or the pose graph."""
        return capi.loops_call("slamhip_hs_loops_consistent", self._h, poses, ij, z, w, spec, use=use, adj=adj)

    def LoopsClear(self):
        """Free the buffers of LoopsConsistent (slamhip_hs_loops_clear)."""
        capi.call("slamhip_hs_loops_clear", self._h)

    def SigClear(self):
        """Free the blocks of the scan signatures and forget the spec (slamhip_hs_sig_clear)."""
        capi.call("slamhip_hs_sig_clear", self._h)
        self.__dict__.pop("_sig_rings", None)

    def mcl_get(self, poses=True, acc=True, ancestors=True):
        """The particle set as it stands (slamhip_hs_mcl_get) -> (poses (N, 3) float32, acc (N,) uint64, ancestors (N,) int32 of the
        last step); None for what was not asked for."""
        n = self._mcl_n
        if not n:
            raise ValueError("mcl_get: no particle set (mcl_set first)")
        p = np.zeros((n, 3), np.float32) if poses else None
        a = np.zeros(n, np.uint64) if acc else None
        k = np.zeros(n, np.int32) if ancestors else None
        ptr = lambda v: v.ctypes.data_as(C.c_void_p) if v is not None else None
        capi.call("slamhip_hs_mcl_get", self._h, ptr(p), ptr(a), ptr(k), n)
        return p, a, k

    def ExpectedScan(self, pose, angles, max_range, level, world=False):
        """The scan the map of `level` predicts from `pose` (window frame): per angle (rad, sensor frame) the range in metres to the
        first occupied cell on the beam of length max_range, or inf where the map holds none.  It REPLACES the scan that was set:
        far points at max_range, the scan origin at the sensor, traced with trace(beams=True); the range is
        hypot(hx - bx, hy - by) * CellLength, formed on the host in float64 from the hit cell and the sensor's cell."""
        a = np.asarray(angles, np.float64).reshape(-1)
        pts = (float(max_range) * np.stack([np.cos(a), np.sin(a)], 1)).astype(np.float32)
        _, rec = self.trace(np.asarray(pose, np.float32).reshape(1, 3), level, world=world, beams=True, scan=ScanCloud(pts))
        cell = np.float32(self.Maps[level].CellLength)
        b = capi.trace_lines(np.float32(1.0) / cell, pose, (0.0, 0.0), [[0.0, 0.0]])[0]          # (the sensor's own cell)
        r = rec[0]
        d = np.hypot(r["hx"].astype(np.float64) - float(b[0]), r["hy"].astype(np.float64) - float(b[1])) * float(cell)
        return np.where(r["first"] >= 0, d, np.inf)

    def UpdateByScan(self, scan, pose):
        self.set_scan(scan)
        p = capi.f32(pose)
        capi.call("slamhip_hs_update_by_scan", self._h, capi.fptr(p))

    def close(self):
        if self._h and self._owned:
            capi.lib().slamhip_hs_destroy(self._h)
        self._h = C.c_void_p()


class ScanMatcher:
    """HectorSLAM/Matcher/ScanMatcher.cs:18-271.  By default numThreads is accepted for source compatibility and the
    point-chunk fan-out it controlled (:149-185) is the workgroup reduction of kernel K4.  With referenceSummation=True
    the matcher sums as the reference does with numThreads threads, bit for bit: every match sets that order on its
    target pyramid first (MapRepMultiMap.set_match_threads); without it every match sets the default order (0)."""

    def __init__(self, numThreads=1, logger=None, referenceSummation=False):
        self.numThreads = numThreads
        self.referenceSummation = bool(referenceSummation)

    def _order(self, rep):
        rep.set_match_threads(self.numThreads if self.referenceSummation else 0)

    def MatchData(self, target, scan, hintPose):
        hint = capi.f32(hintPose); out = np.empty(3, np.float32)
        self._order(target if isinstance(target, MapRepMultiMap) else target._rep)
        if isinstance(target, MapRepMultiMap):                      # :41
            target.set_scan(scan)
            capi.call("slamhip_hs_match", target._h, capi.fptr(hint), capi.fptr(out))
        else:                                                       # :64 MatchData(OccGridMap, ...)
            target._rep.set_scan(scan)
            capi.call("slamhip_hs_match_level", target._rep._h, target.level, capi.fptr(hint),
                      target.EstimateIterations, capi.fptr(out))
        return out

    def MatchDataReport(self, target, scan, hintPose):
        """MatchData and the match report (slamhip_match_report, a capi.REPORT_DTYPE record): -> (pose, report)."""
        hint = capi.f32(hintPose); out = np.empty(3, np.float32); rep = np.zeros(1, capi.REPORT_DTYPE)
        self._order(target if isinstance(target, MapRepMultiMap) else target._rep)
        if isinstance(target, MapRepMultiMap):
            target.set_scan(scan)
            capi.call("slamhip_hs_match_report", target._h, capi.fptr(hint), capi.fptr(out), capi.rptr(rep))
        else:
            target._rep.set_scan(scan)
            capi.call("slamhip_hs_match_level_report", target._rep._h, target.level, capi.fptr(hint),
                      target.EstimateIterations, capi.fptr(out), capi.rptr(rep))
        return out, rep[0]

    def MatchDataBatchReport(self, rep, scan, hintPoses):
        """MatchDataBatch and every match's report: -> (poses (B, 3), reports (B,) of capi.REPORT_DTYPE)."""
        hints = capi.f32(hintPoses, (-1, 3)); out = np.empty_like(hints); reps = np.zeros(hints.shape[0], capi.REPORT_DTYPE)
        self._order(rep)
        rep.set_scan(scan)
        capi.call("slamhip_hs_match_batch_report", rep._h, capi.fptr(hints), hints.shape[0], capi.fptr(out), capi.rptr(reps))
        return out, reps

    def MatchDataBest(self, rep, scan, hintPoses):
        """The best of B hints, picked on the device by the smallest residual, ties to the lowest index
        (slamhip_hs_match_best): -> (pose, index, report).  Whether that residual is good enough is the caller's call."""
        hints = capi.f32(hintPoses, (-1, 3)); out = np.empty(3, np.float32); r = np.zeros(1, capi.REPORT_DTYPE)
        idx = C.c_int32(-1)
        self._order(rep)
        rep.set_scan(scan)
        capi.call("slamhip_hs_match_best", rep._h, capi.fptr(hints), hints.shape[0], capi.fptr(out), C.byref(idx), capi.rptr(r))
        return out, int(idx.value), r[0]

    def Relocalise(self, rep, scan, level, centre, nx, ny, n_theta, dtheta, B=16, search="lattice", top=None):
        """Lattice search, then the best of the min(B, n_theta) highest-scoring headings' nodes refined by MatchDataBest
        (slamhip_hs_relocalise): -> (pose, report, info), info a capi.RELOC_INFO record.  Poses in the window's frame.
        search="bnb": the branch-and-bound search (slamhip_hs_relocalise_bnb; top=None: 3, measured) in place of the exhaustive
        one -- the same pose, report and info, for lattices of any size -- and -> (pose, report, info, bnb), bnb a capi.BNB_INFO
        record."""
        bnb = _search_kind(search)
        spec = capi.lattice_spec(level, centre, nx, ny, n_theta, dtheta)
        out = np.empty(3, np.float32); r = np.zeros(1, capi.REPORT_DTYPE); info = capi.RelocInfo()
        self._order(rep)
        rep.set_scan(scan)
        if bnb:
            bspec = capi.bnb_spec(level, centre, nx, ny, n_theta, dtheta, BNB_DEFAULT_TOP if top is None else top, False)
            binfo = capi.BnbInfo()
            capi.call("slamhip_hs_relocalise_bnb", rep._h, C.byref(bspec), int(B), capi.fptr(out), capi.rptr(r), C.byref(info), C.byref(binfo))
            return out, r[0], _reloc_info(info), capi.bnb_info(binfo)
        capi.call("slamhip_hs_relocalise", rep._h, C.byref(spec), int(B), capi.fptr(out), capi.rptr(r), C.byref(info))
        return out, r[0], _reloc_info(info)

    def RelocaliseWorld(self, rep, scan, level, centre, nx, ny, n_theta, dtheta, B=16, search="lattice", top=None):
        """Relocalise anywhere in the world behind the window (slamhip_hs_relocalise_world; backing must be on): the world
        lattice search, the window shifted to the best node -- the backing store restores what lies there -- and the best
        headings' nodes that lie in the new window refined by MatchDataBest.  -> (pose, report, info): the pose in the NEW
        window's frame, info a capi.WORLD_RELOC_INFO record whose dx, dy say how the window moved.  search="bnb", top: as in
        Relocalise; -> (pose, report, info, bnb)."""
        bnb = _search_kind(search)
        spec = capi.lattice_spec(level, centre, nx, ny, n_theta, dtheta)
        out = np.empty(3, np.float32); r = np.zeros(1, capi.REPORT_DTYPE); info = capi.WorldRelocInfo()
        self._order(rep)
        rep.set_scan(scan)
        if bnb:
            bspec = capi.bnb_spec(level, centre, nx, ny, n_theta, dtheta, BNB_DEFAULT_TOP if top is None else top, True)
            binfo = capi.BnbInfo()
            capi.call("slamhip_hs_relocalise_bnb", rep._h, C.byref(bspec), int(B), capi.fptr(out), capi.rptr(r), C.byref(info), C.byref(binfo))
            return out, r[0], _world_reloc_info(info), capi.bnb_info(binfo)
        capi.call("slamhip_hs_relocalise_world", rep._h, C.byref(spec), int(B), capi.fptr(out), capi.rptr(r), C.byref(info))
        return out, r[0], _world_reloc_info(info)

    def MatchDataBatch(self, rep, scan, hintPoses):
        hints = capi.f32(hintPoses, (-1, 3)); out = np.empty_like(hints)
        self._order(rep)
        rep.set_scan(scan)
        capi.call("slamhip_hs_match_batch", rep._h, capi.fptr(hints), hints.shape[0], capi.fptr(out))
        return out

    def Dispose(self):
        pass


class HectorSLAMProcessor:
    """HectorSLAM/Main/HectorSLAMProcessor.cs:17-160"""

    def __init__(self, mapResolution, mapSize, startPose, numDepth, numThreads=1, logger=None, ctx=None,
                 referenceSummation=False, referenceCache=False, matchReport=False, scrollTrigger=0,
                 scrollBacking=None):
        self._own_ctx = ctx is None
        self.ctx = ctx or Context(0)
        sp = capi.f32(startPose)
        self._h = C.c_void_p()
        capi.call("slamhip_hsproc_create", self.ctx._h, C.c_float(mapResolution), int(mapSize[0]), int(mapSize[1]),
                  capi.fptr(sp), int(numDepth), C.byref(self._h))
        hsh = C.c_void_p()
        capi.call("slamhip_hsproc_hs", self._h, C.byref(hsh))
        self.MapRep = MapRepMultiMap(mapResolution, mapSize, numDepth, ctx=self.ctx, _handle=hsh)
        if referenceSummation:                                      # the processor's matcher, ScanMatcher(numThreads) (:72)
            self.MapRep.set_match_threads(numThreads)
        if referenceCache:                                          # OccGridMap's cacheArray, stale across Reset (deviation D5)
            self.MapRep.set_reference_cache(1)
        if matchReport:                                             # every Update's match leaves its report (LastMatchReport)
            capi.call("slamhip_hsproc_set_match_report", self._h, 1)
        if scrollTrigger:                                           # keep the robot in the window (slamhip_hsproc_set_scroll)
            self.set_scroll(scrollTrigger)
        if scrollBacking is not None:                               # (tile, max_bytes): keep what scrolls out (MapRep.set_backing)
            self.set_backing(*scrollBacking)
        self._min_dist, self._min_angle = 0.3, 0.13
        self._mcl_origin = None                                     # the window's origin at the last LocaliseInit / LocaliseStep

    def _get(self):
        m = np.empty(3, np.float32); l = np.empty(3, np.float32); mt, ut = C.c_float(), C.c_float()
        capi.call("slamhip_hsproc_get", self._h, capi.fptr(m), capi.fptr(l), C.byref(mt), C.byref(ut))
        return m, l, mt.value, ut.value

    def set_scroll(self, triggerCells):
        """Keep the robot in the window (slamhip_hsproc_set_scroll): 0 off (default); > 0: at the end of an Update whose match
        pose lies more than triggerCells level-0 cells from the window's middle on an axis, the pyramid is shifted on the
        device so that the pose is back within 1 << (numDepth - 1) cells of the middle.  Hints and poses stay world poses."""
        capi.call("slamhip_hsproc_set_scroll", self._h, int(triggerCells))

    def set_backing(self, tile, max_bytes):
        """The backing store of the processor's own pyramid (MapRepMultiMap.set_backing): what the scroll moves out of the
        window is kept on the device and restored when the robot returns.  max_bytes = 0: off."""
        self.MapRep.set_backing(tile, max_bytes)

    def backing_stats(self):
        return self.MapRep.backing_stats()

    def get_origin(self):
        """(ox, oy) of the processor's window in level-0 cells (slamhip_hsproc_get_origin)."""
        ox, oy = C.c_int64(), C.c_int64()
        capi.call("slamhip_hsproc_get_origin", self._h, C.byref(ox), C.byref(oy))
        return int(ox.value), int(oy.value)

    def shift(self, dx, dy):
        """MapRep.shift from outside an Update (slamhip_hsproc_shift): the window moves, MatchPose and LastMapUpdatePose stay
        the world poses they were."""
        capi.call("slamhip_hsproc_shift", self._h, int(dx), int(dy))

    def SaveWorld(self, path):
        """MapRep.save_world: the processor's world -- window and tiles -- as one .npz."""
        self.MapRep.save_world(path)

    def LoadWorld(self, path):
        """MapRep.load_world into the processor's own pyramid, the window moved through the processor so that its poses stay
        world poses: create the processor with startPose = the saved pose, LoadWorld, Update.  -> the cells dropped."""
        return self.MapRep.load_world(path, _shift=self.shift)

    def _relocalise_bnb(self, scan, centreWorld, level, nx, ny, n_theta, dtheta, B, adopt, top, world):
        spec = capi.bnb_spec(level, centreWorld, nx, ny, n_theta, dtheta, BNB_DEFAULT_TOP if top is None else top, world)
        org = capi.f32(scan.Pose[:2])
        out = np.empty(3, np.float32); r = np.zeros(1, capi.REPORT_DTYPE); binfo = capi.BnbInfo()
        info = capi.WorldRelocInfo() if world else capi.RelocInfo()
        capi.call("slamhip_hsproc_relocalise_bnb", self._h, capi.fptr(scan.Points), scan.Points.shape[0], capi.fptr(org), C.byref(spec),
                  int(B), 1 if adopt else 0, capi.fptr(out), capi.rptr(r), C.byref(info), C.byref(binfo))
        self.MapRep._scan_set = (scan.Points.shape[0], org.copy())
        return out, r[0], (_world_reloc_info if world else _reloc_info)(info), capi.bnb_info(binfo)

    def Relocalise(self, scan, centreWorld, level, nx, ny, n_theta, dtheta, B=16, adopt=True, search="lattice", top=None):
        """Find the robot in the map the window holds (slamhip_hsproc_relocalise): lattice search around centreWorld (a world
        pose) on `level`, the best nodes refined by the matcher.  -> (poseWorld, report, info).  adopt=True: the pose becomes
        MatchPose and LastMapUpdatePose, so the next Update matches from it and writes the map only once the robot has moved;
        adopt=False: the processor is untouched.  The resume flow: LoadWorld, Relocalise, Update.  search="bnb": the
        branch-and-bound search (slamhip_hsproc_relocalise_bnb; top=None: 3, measured), for lattices of any size;
        -> (poseWorld, report, info, bnb), bnb a capi.BNB_INFO record."""
        if _search_kind(search):
            return self._relocalise_bnb(scan, centreWorld, level, nx, ny, n_theta, dtheta, B, adopt, top, False)
        spec = capi.lattice_spec(level, centreWorld, nx, ny, n_theta, dtheta)
        org = capi.f32(scan.Pose[:2])
        out = np.empty(3, np.float32); r = np.zeros(1, capi.REPORT_DTYPE); info = capi.RelocInfo()
        capi.call("slamhip_hsproc_relocalise", self._h, capi.fptr(scan.Points), scan.Points.shape[0], capi.fptr(org), C.byref(spec),
                  int(B), 1 if adopt else 0, capi.fptr(out), capi.rptr(r), C.byref(info))
        self.MapRep._scan_set = (scan.Points.shape[0], org.copy())
        return out, r[0], _reloc_info(info)

    def RelocaliseWorldBnb(self, scan, centreWorld, level, nx, ny, n_theta, dtheta, B=16, adopt=True, top=None):
        """RelocaliseWorld with the branch-and-bound search (slamhip_hsproc_relocalise_bnb, world = 1; top=None: 3, measured) in place
        of the exhaustive one, for lattices of any size: -> (poseWorld, report, info, bnb), the first three RelocaliseWorld's bit for
        bit wherever that call accepts the lattice, bnb a capi.BNB_INFO record.  (A method of its own: RelocaliseWorld's parameter
        list is pinned.)"""
        return self._relocalise_bnb(scan, centreWorld, level, nx, ny, n_theta, dtheta, B, adopt, top, True)

    def RelocaliseWorld(self, scan, centreWorld, level, nx, ny, n_theta, dtheta, B=16, adopt=True):
        """Find the robot anywhere in the saved world (slamhip_hsproc_relocalise_world; backing must be on): as Relocalise, but
        the lattice is scored against the window AND the tiles behind it, and the window then moves to the best node.
        -> (poseWorld, report, info), info a capi.WORLD_RELOC_INFO record (dx, dy: the shift).  MatchPose and LastMapUpdatePose
        stay the world poses they were (adopt=False) or become the result (adopt=True).  The resume flow: LoadWorld,
        RelocaliseWorld, Update.  RelocaliseWorldBnb: the same by branch and bound."""
        spec = capi.lattice_spec(level, centreWorld, nx, ny, n_theta, dtheta)
        org = capi.f32(scan.Pose[:2])
        out = np.empty(3, np.float32); r = np.zeros(1, capi.REPORT_DTYPE); info = capi.WorldRelocInfo()
        capi.call("slamhip_hsproc_relocalise_world", self._h, capi.fptr(scan.Points), scan.Points.shape[0], capi.fptr(org), C.byref(spec),
                  int(B), 1 if adopt else 0, capi.fptr(out), capi.rptr(r), C.byref(info))
        self.MapRep._scan_set = (scan.Points.shape[0], org.copy())
        return out, r[0], _world_reloc_info(info)

    def Trace(self, scan, posesWorld, level, world=False, beams=False):
        """MapRep.trace of `scan` at WORLD poses (slamhip_hsproc_trace): the poses are taken to the window's frame as Relocalise takes
        its centre.  -> (summaries, beams | None); hx, hy of a beam record stay window-frame cells of `level` (get_origin converts:
        world cell = (origin >> level) + cell).  MatchPose, LastMapUpdatePose and the update gate are untouched."""
        p = capi.f32(posesWorld, (-1, 3)); org = capi.f32(scan.Pose[:2])
        sums = np.zeros(p.shape[0], capi.TRACE_SUMMARY)
        rec = np.zeros((p.shape[0], scan.Points.shape[0]), capi.TRACE_BEAM) if beams else None
        capi.call("slamhip_hsproc_trace", self._h, capi.fptr(scan.Points), scan.Points.shape[0], capi.fptr(org), capi.fptr(p), p.shape[0],
                  int(level), 1 if world else 0, sums.ctypes.data_as(C.c_void_p), rec.ctypes.data_as(C.c_void_p) if beams else None)
        self.MapRep._scan_set = (scan.Points.shape[0], org.copy())
        return sums, rec

    def ViewGain(self, scan, posesWorld, level, reach, commit=-1):
        """MapRep.view_gain of `scan` at WORLD poses (slamhip_hsproc_view_gain), taken to the window's frame as Trace takes them.
        MatchPose, LastMapUpdatePose and the update gate are untouched."""
        p = capi.f32(posesWorld, (-1, 3)); org = capi.f32(scan.Pose[:2])
        out = np.zeros(p.shape[0], capi.VIEW_SUMMARY)
        capi.call("slamhip_hsproc_view_gain", self._h, capi.fptr(scan.Points), scan.Points.shape[0], capi.fptr(org), capi.fptr(p), p.shape[0],
                  int(level), int(reach), int(commit), out.ctypes.data_as(C.c_void_p))
        self.MapRep._scan_set = (scan.Points.shape[0], org.copy())
        return out

    def ViewSelect(self, scan, posesWorld, level, reach, k, mode=0, min_gain=1):
        """MapRep.view_select of `scan` at WORLD poses (slamhip_hsproc_view_select) -> (order, gain)."""
        p = capi.f32(posesWorld, (-1, 3)); org = capi.f32(scan.Pose[:2])
        order = np.zeros(int(k), np.int32); gain = np.zeros(int(k), np.int32); n = C.c_int32()
        capi.call("slamhip_hsproc_view_select", self._h, capi.fptr(scan.Points), scan.Points.shape[0], capi.fptr(org), capi.fptr(p), p.shape[0],
                  int(level), int(reach), int(mode), int(min_gain), int(k), capi.iptr(order), capi.iptr(gain), C.byref(n))
        self.MapRep._scan_set = (scan.Points.shape[0], org.copy())
        return order[:n.value].copy(), gain[:n.value].copy()

    def DistanceScore(self, scan, posesWorld, level, site_mask=2, radius=32, world=False, points=False):
        """MapRep.distance_score of `scan` at WORLD poses (slamhip_hsproc_distance_score): the poses are taken to the window's frame
        as Trace takes them.  -> (summaries, points | None).  MatchPose, LastMapUpdatePose and the update gate are untouched."""
        p = capi.f32(posesWorld, (-1, 3)); org = capi.f32(scan.Pose[:2])
        sums = np.zeros(p.shape[0], capi.DISTANCE_SUMMARY)
        rec = np.zeros((p.shape[0], scan.Points.shape[0]), np.uint16) if points else None
        capi.call("slamhip_hsproc_distance_score", self._h, capi.fptr(scan.Points), scan.Points.shape[0], capi.fptr(org), capi.fptr(p), p.shape[0],
                  int(level), 1 if world else 0, int(site_mask), int(radius), sums.ctypes.data_as(C.c_void_p),
                  rec.ctypes.data_as(C.c_void_p) if points else None)
        self.MapRep._scan_set = (scan.Points.shape[0], org.copy())
        return sums, rec

    def NearestPairs(self, scan, posesWorld, level, site_mask=2, radius=32, world=False, pairs=False):
        """MapRep.nearest_pairs of `scan` at WORLD poses (slamhip_hsproc_nearest_pairs): the poses are taken to the window's frame as
        Trace takes them.  -> (summaries, pairs | None); the summaries' cell sums stay window-frame cells of `level`.  MatchPose,
        LastMapUpdatePose and the update gate are untouched."""
        p = capi.f32(posesWorld, (-1, 3)); org = capi.f32(scan.Pose[:2])
        sums = np.zeros(p.shape[0], capi.PAIR_SUMMARY)
        rec = np.zeros((p.shape[0], scan.Points.shape[0], 2), np.int16) if pairs else None
        capi.call("slamhip_hsproc_nearest_pairs", self._h, capi.fptr(scan.Points), scan.Points.shape[0], capi.fptr(org), capi.fptr(p), p.shape[0],
                  int(level), 1 if world else 0, int(site_mask), int(radius), sums.ctypes.data_as(C.c_void_p),
                  rec.ctypes.data_as(C.c_void_p) if pairs else None)
        self.MapRep._scan_set = (scan.Points.shape[0], org.copy())
        return sums, rec

    def AlignStep(self, scan, poseWorld, level, site_mask=2, radius=32, world=False):
        """One point-to-map alignment step of `scan` at the WORLD pose poseWorld: NearestPairs at that pose, then align_step -- host
        arithmetic only -- on the pose in the window's frame (minus (float)origin * cell0 per axis, rounded as the library rounds
        it), taken back by the same offset.  -> (poseWorld', summary).  Iteration is the caller's loop: call again with the result
        until summary["n_zero"] == summary["n_matched"] or the step is small enough.  Nothing of the processor changes."""
        pw = capi.f32(poseWorld, (3,))
        sums, _ = self.NearestPairs(scan, pw[None, :], level, site_mask=site_mask, radius=radius, world=world)
        ox, oy = self.get_origin()
        if not (ox or oy):                                          # (the window has never moved: the two frames are one)
            return align_step(pw, sums[0], self._stm(level))[0], sums[0]
        off = self._window_offset()
        win = np.array([pw[0] - off[0], pw[1] - off[1], pw[2]], np.float32)
        return align_step(win, sums[0], self._stm(level), base=pw)[0], sums[0]

    def _stm(self, level):
        return np.float32(1.0) / np.float32(self.MapRep.Maps[level].CellLength)   # ScaleToMap, as the library forms it

    def Frontiers(self, level, min_cells=1, max_clusters=256, world=False, labels_rect=None):
        """MapRep.frontiers in WORLD cells of `level` (slamhip_hsproc_frontiers): seeds, boxes, sums, mx0 / my0 and labels_rect are world
        cells.  -> (summary, clusters, centroids[, labels]); centroids the (n, 2) float64 centres of the clusters in metres, world
        frame: the sums taken to the window's frame of the level (- n_cells * (origin >> level), exact), the mean cell through the
        level's cell-to-world transform (cell * CellLength, as ExpectedScan forms ranges) and back by (float)origin * cell0 as every
        world pose is.  No scan is
        needed; MatchPose, LastMapUpdatePose and the update gate are untouched."""
        rect = (0, 0, 0, 0) if labels_rect is None else tuple(int(v) for v in labels_rect)
        shape = None if labels_rect is None else (max(rect[3], 0), max(rect[2], 0))
        out = capi.frontiers_call("slamhip_hsproc_frontiers", [self._h, int(level), 1 if world else 0], min_cells, max_clusters, shape, rect)
        rec = out[1]
        ox, oy = self.get_origin()
        cell = float(np.float32(self.MapRep.Maps[level].CellLength)); cell0 = np.float32(self.MapRep.Maps[0].CellLength)
        n = rec["n_cells"].astype(np.int64)                         # (the sums back in the window's frame: integers, exact)
        cx = (rec["sum_x"] - n * (ox >> level)) / n * cell + float(np.float32(ox) * cell0)
        cy = (rec["sum_y"] - n * (oy >> level)) / n * cell + float(np.float32(oy) * cell0)
        return out[:2] + (np.stack([cx, cy], 1),) + out[2:]

    def NavField(self, level, sources, clearance=0, site_mask=2, max_cost=0, world=False, goals=None, n_paths=0, max_path_cells=1,
                 rect=None, want_cost=True, want_dir=True):
        """MapRep.nav_field in WORLD cells of `level` (slamhip_hsproc_nav_field): sources, goals and rect are world cells, and so are
        the goals' cells, the paths and mx0 / my0 of the summary.  No scan is needed; MatchPose, LastMapUpdatePose and the update gate
        are untouched."""
        spec = capi.nav_spec(level, world, site_mask, clearance, max_cost)
        return capi.nav_call("slamhip_hsproc_nav_field", [self._h, spec.ctypes.data_as(C.c_void_p)], sources, goals, n_paths, max_path_cells, rect,
                             want_cost, want_dir)

    def ExploreGoals(self, level, clearance, site_mask=2, min_cells=1, max_clusters=256, grow=0, n_paths=0, max_path_cells=1, world=False):
        """Which frontier to drive to: Frontiers, then NavField from the cell of MatchPose with each returned cluster's bounding box,
        grown by `grow` cells on every side, as a goal (the box, not the cluster's own cells).  -> (clusters, results, nav): the
        clusters and their capi.NAV_GOAL_RESULT records, reachable ones first by cost ascending (equal costs in Frontiers' order), the
        unreachable ones behind them in Frontiers' order; nav is NavField's dict with `order`, the row of Frontiers' list each entry
        came from -- nav["paths"][k] belongs to Frontiers' cluster k, for k < n_paths.  Composition only: no device work of its
        own."""
        rec = self.Frontiers(level, min_cells=min_cells, max_clusters=max_clusters, world=world)[1]
        if rec.shape[0] == 0:
            return rec, np.zeros(0, capi.NAV_GOAL_RESULT), None
        goals = np.stack([rec["x_min"] - grow, rec["y_min"] - grow, rec["x_max"] + grow, rec["y_max"] + grow], 1)
        nav = self.NavField(level, [self.PoseCell(level)], clearance, site_mask, world=world, goals=goals,
                            n_paths=min(int(n_paths), goals.shape[0]), max_path_cells=max_path_cells)
        order = np.argsort(nav["goals"]["cost"], kind="stable")          # (an unreachable goal's cost is the largest uint32)
        nav["order"] = order
        return rec[order], nav["goals"][order], nav

    def Rollouts(self, level, sources, dt, cmds, hold=1, body=None, start_pose=None, clearance=0, site_mask=2, max_cost=0, world=False):
        """MapRep.rollouts in WORLD cells and the WORLD pose (slamhip_hsproc_rollouts): sources are world cells of `level`,
        start_pose a world pose (None: MatchPose), and the results' poses and nav.mx0 / nav.my0 are world values.  No scan is needed;
        MatchPose, LastMapUpdatePose and the update gate are untouched."""
        spec = capi.nav_spec(level, world, site_mask, clearance, max_cost)
        return capi.rollouts_call("slamhip_hsproc_rollouts", [self._h, spec.ctypes.data_as(C.c_void_p)], sources, start_pose, dt, body, cmds, hold)

    def DriveCommand(self, level, goal_cells, clearance, v_values, w_values, dt, steps, body=None, start_pose=None, site_mask=2, max_cost=0,
                     world=False):
        """Which constant command to drive: Rollouts of the outer product of v_values and w_values (B = len(v) * len(w) commands,
        command b = (v[b // len(w)], w[b % len(w)]), n_cmd = 1, hold = steps) towards goal_cells ((S, 2) world cells).  -> (v, w,
        which, result, summary): the command decoded from key_end -- the complete rollout that ends cheapest, which = "end" -- or,
        if nothing completes, from key_min -- the rollout that comes closest before it is cut, which = "min"; its
        capi.ROLLOUT_RESULT record and the call's summary.  (None, None, None, None, summary) when no rollout has a free pose.
        Composition only: no device work of its own."""
        v = np.asarray(v_values, np.float32).reshape(-1); w = np.asarray(w_values, np.float32).reshape(-1)
        cmds = np.stack([np.repeat(v, w.shape[0]), np.tile(w, v.shape[0])], 1).reshape(-1, 1, 2)
        res, summary = self.Rollouts(level, goal_cells, dt, cmds, int(steps), body, start_pose, clearance, site_mask, max_cost, world)
        for which in ("end", "min"):
            key = capi.rollout_key(summary["key_" + which])
            if key is not None:
                b = key[1]
                return float(cmds[b, 0, 0]), float(cmds[b, 0, 1]), which, res[b], summary
        return None, None, None, None, summary

    def _window_offset(self):
        """(float)origin * cell0 per axis, as the library forms it: what a world pose loses on its way into the window's frame."""
        ox, oy = self.get_origin()
        cell0 = np.float32(self.MapRep.Maps[0].CellLength)
        return np.float32(ox) * cell0, np.float32(oy) * cell0

    def merge_set_source(self, level, ax, ay, cells):
        """MapRep.merge_set_source through the processor (slamhip_hsproc_merge_set_source): the source's frame is its own."""
        c = np.ascontiguousarray(cells, capi.CELL_DTYPE)
        if c.ndim != 2:
            raise ValueError("merge_set_source: cells must be an (h, w) array")
        capi.call("slamhip_hsproc_merge_set_source", self._h, int(level), int(ax), int(ay), c.shape[1], c.shape[0], c.ctypes.data_as(C.c_void_p))

    def merge_score(self, posesWorld):
        """MapRep.merge_score at WORLD poses of the source frame's origin (slamhip_hsproc_merge_score), taken to the window's frame as
        Trace takes its poses."""
        p = capi.f32(posesWorld, (-1, 3))
        out = np.zeros(p.shape[0], capi.MERGE_REPORT)
        capi.call("slamhip_hsproc_merge_score", self._h, capi.fptr(p), p.shape[0], out.ctypes.data_as(C.c_void_p))
        return out

    def merge_apply(self, poseWorld, rule=capi.MERGE_ADD, value_limit=50.0):
        """MapRep.merge_apply at a WORLD pose (slamhip_hsproc_merge_apply).  MatchPose, LastMapUpdatePose and the update gate are
        untouched."""
        out = np.zeros(1, capi.MERGE_REPORT)
        capi.call("slamhip_hsproc_merge_apply", self._h, capi.fptr(capi.f32(poseWorld, (3,))), int(rule), C.c_float(value_limit),
                  out.ctypes.data_as(C.c_void_p))
        return out[0]

    def merge_clear_source(self):
        self.MapRep.merge_clear_source()

    def hough(self, level, slot=0, world=False, site_mask=2, T=360, q=1, H=False):
        """MapRep.hough through the processor (slamhip_hsproc_hough): cells and bins, no pose to convert."""
        return self.MapRep._hough("slamhip_hsproc_hough", self._h, level, slot, world, site_mask, T, q, H)

    def hough_rotation(self):
        """MapRep.hough_rotation through the processor (slamhip_hsproc_hough_rotation)."""
        d, _ = self.MapRep._hough_both()
        cc = np.zeros(d["T"], np.uint64)
        capi.call("slamhip_hsproc_hough_rotation", self._h, cc.ctypes.data_as(C.c_void_p))
        return cc

    def hough_shifts(self, pairs, xc=False):
        """MapRep.hough_shifts through the processor (slamhip_hsproc_hough_shifts)."""
        d, s = self.MapRep._hough_both()
        return capi.hough_shifts_call("slamhip_hsproc_hough_shifts", self._h, pairs, d["N"] + s["N"] - 1 if xc and d["N"] and s["N"] else None)

    def AlignMaps(self, level, T=360, q=1, n_rot=4, site_mask=2):
        """Align the merge source (merge_set_source first) with the window's map of its level WITHOUT a scan, by the Hough spectrum:
        both slots filled (hough), the rotation scores' best n_rot peaks, each at m and m + T (the pi ambiguity), two row correlations
        per hypothesis in ONE hough_shifts call (rows ka = arg-max HS_d and ka + T/2), the translation from the two shifts
        (capi.hough_pose), and every hypothesis rated by merge_score.  -> a list of dicts (m, pose, shifts, report), poses in the
        WORLD frame, ordered by report.joint[4] (occupied on occupied) descending, then by index.  Host composition
        (capi.align_maps); the library forms no threshold and picks no peak."""
        info_d, hs_d, _ = self.hough(level, 0, False, site_mask, T, q)
        info_s, hs_s, _ = self.hough(level, 1, False, site_mask, T, q)
        stm = float(np.float32(1.0) / np.float32(self.MapRep.Maps[level].CellLength))
        off = self._window_offset() if self.get_origin() != (0, 0) else (np.float32(0.0), np.float32(0.0))

        def score(poses):                                                  # (window-frame poses -> world poses, as merge_score takes them)
            p = poses.copy()
            p[:, 0] += off[0]; p[:, 1] += off[1]
            return self.merge_score(p)
        out = capi.align_maps(int(T), int(q), n_rot, hs_d, hs_s, info_d, info_s, stm, self.hough_rotation, lambda pairs: self.hough_shifts(pairs)[0], score)
        for h in out:
            h["pose"][0] += off[0]; h["pose"][1] += off[1]
        return out

    def AddKeyframe(self, scan, poseWorld, keep_scan=False):
        """The signature of `scan` appended to the keyframe store with its WORLD pose (slamhip_hsproc_sig_add; MapRep.SigConfigure
        first) -> (index, sig, info).  With keep_scan the scan itself is appended to the scan store too (slamhip_hsproc_scans_add),
        under the same index: what RenderKeyframes draws from.  MatchPose, LastMapUpdatePose and the update gate are untouched."""
        org = capi.f32(scan.Pose[:2])
        out = capi.sig_add_call("slamhip_hsproc_sig_add", self._h, poseWorld, self.MapRep._sig_n_ring(), (scan.Points, org))
        self.MapRep._scan_set = (scan.Points.shape[0], org.copy())
        if keep_scan:
            k = C.c_int32()
            capi.call("slamhip_hsproc_scans_add", self._h, C.byref(k))
            assert k.value == out[0], (k.value, out[0])             # (the two stores' indices agree)
        return out

    def RenderKeyframes(self, poses=None, first=0, last=None, keep=False):
        """Draw the stored keyframe scans [first, last) into the map at WORLD poses (slamhip_hsproc_render) -- by default the poses
        of the signature store, which RelaxKeyframes has just corrected.  Without keep the map is cleared first."""
        last = self.MapRep.ScansCount() if last is None else int(last)
        if poses is None:
            _, kp = self.MapRep.SigDownload()
            poses = kp[first:last]
        p = capi.f32(poses, (-1, 3)) if last > first else np.zeros((1, 3), np.float32)
        assert last <= first or p.shape[0] == last - first
        capi.call("slamhip_hsproc_render", self._h, int(first), last, capi._vp(p), capi.RENDER_KEEP if keep else 0)

    def RenderKeyframesWorld(self, poses=None, first=0, last=None, keep=False):
        """RenderKeyframes into the whole world behind the window (slamhip_hsproc_render_world; set_backing first): what a loop
        closure needs when the map is larger than the window.  poses as RenderKeyframes takes them."""
        last = self.MapRep.ScansCount() if last is None else int(last)
        if poses is None:
            _, kp = self.MapRep.SigDownload()
            poses = kp[first:last]
        p = capi.f32(poses, (-1, 3)) if last > first else np.zeros((1, 3), np.float32)
        assert last <= first or p.shape[0] == last - first
        capi.call("slamhip_hsproc_render_world", self._h, int(first), last, capi._vp(p), capi.RENDER_KEEP if keep else 0)

    def LoopCandidates(self, scan, B=capi.SIG_MAX_HITS, exclude_recent=0):
        """The keyframes `scan` resembles most, over all 64 headings (slamhip_hsproc_sig_query over [0, count - exclude_recent))
        -> a list of dicts (hit: the capi.SIG_HIT_DTYPE record, pose: the guess (x_k, y_k, theta_k - shift 2 pi / 64) from the
        keyframe's stored pose), higher score first.  Candidates only: VerifyLoop checks one against the map."""
        org = capi.f32(scan.Pose[:2])
        last = max(self.MapRep.SigCount() - int(exclude_recent), 0)
        hits, _, _ = capi.sig_query_call("slamhip_hsproc_sig_query", self._h, 0, last, B, self.MapRep._sig_n_ring(), (scan.Points, org))
        self.MapRep._scan_set = (scan.Points.shape[0], org.copy())
        out = []
        for h in hits:
            _, pose = self.MapRep.SigDownload(int(h["index"]), 1)
            out.append({"hit": h.copy(), "pose": capi.sig_pose_guess(pose[0], h["shift"])})
        return out

    def SelfLoopCandidates(self, min_gap, first=0, last=None):
        """MapRep.SigSelf through the processor (slamhip_hsproc_sig_self)."""
        return capi.sig_self_call("slamhip_hsproc_sig_self", self._h, first, self.MapRep.SigCount() if last is None else last, min_gap)

    def VerifyLoop(self, scan, hit, level, nx, ny, n_theta, dtheta, B=16, search="lattice", top=None):
        """Check one loop candidate (an entry of LoopCandidates) against the map: Relocalise centred on the candidate's pose guess,
        adopt=False.  -> (poseWorld, report, info) as Relocalise (search="bnb": with the bnb record behind them).  Host composition
        only; the caller judges the report."""
        return self.Relocalise(scan, hit["pose"], level, nx, ny, n_theta, dtheta, B=B, adopt=False, search=search, top=top)

    def _keyframe_graph(self, loops, odom_w, fixed):
        """The keyframe store's pose graph, handed to MapRep.PgSet: the store's poses as nodes, an odometry edge per pair of consecutive
        keyframes (z from their stored poses, weights odom_w), then one edge per entry (i, j, z, w) of `loops` -> (poses, ij, z, w)."""
        _, kp = self.MapRep.SigDownload()
        N = kp.shape[0]
        poses = kp.astype(np.float64)
        ij = [(k, k + 1) for k in range(N - 1)]; z = [capi.pg_edge_between(poses[k], poses[k + 1]) for k in range(N - 1)]
        w = [tuple(float(v) for v in odom_w)] * (N - 1)
        for (i, j, zl, wl) in loops:
            ij.append((int(i), int(j))); z.append(tuple(float(v) for v in zl)); w.append(tuple(float(v) for v in wl))
        ij = np.array(ij, np.int32).reshape(-1, 2); z = np.array(z, np.float64).reshape(-1, 3); w = np.array(w, np.float64).reshape(-1, 3)
        self.MapRep.PgSet(poses, fixed, ij, z, w)
        return poses, ij, z, w

    def KeyframeCovariances(self, pairs, odom_w, loops=(), spec=None, fixed=None):
        """How well the keyframes are known relative to one another (host composition of slamhip_hs_pg_set and _pg_marginals; no
        reference counterpart): the graph RelaxKeyframes builds, at the store's poses as they stand -- nothing is relaxed or written
        back.  pairs (Q, 2) keyframe indices (i, j); the four marginal blocks of every pair are asked for in one query; spec a
        capi.pg_marg_spec record (None: MapRep.PgMarginals' default, the odometry-chain preconditioner)
        -> dict(blocks (Q, 2, 2, 3, 3): [[S_ii, S_ij], [S_ji, S_jj]], rel (Q, 3, 3): capi.pg_relative_covariance of them at the two
        poses, cols, info)."""
        poses = self._keyframe_graph(loops, odom_w, fixed)[0]
        pr = np.asarray(pairs, np.int32).reshape(-1, 2)
        ask = np.stack([pr[:, [0, 0]], pr[:, [0, 1]], pr[:, [1, 0]], pr[:, [1, 1]]], axis=1).reshape(-1, 2)
        b, cols, info = self.MapRep.PgMarginals(ask, spec)
        blocks = b.reshape(-1, 2, 2, 3, 3)
        rel = np.stack([capi.pg_relative_covariance(poses[i], poses[j], q[0, 0], q[0, 1], q[1, 0], q[1, 1]) for (i, j), q in zip(pr, blocks)]) \
            if pr.shape[0] else np.zeros((0, 3, 3))
        return dict(blocks=blocks, rel=rel, cols=cols, info=info)

    def LoopMahalanobis(self, loops, odom_w, accepted=(), spec=None, fixed=None):
        """The squared Mahalanobis distance of every candidate loop edge (i, j, z, w) of `loops` against the graph WITHOUT that edge --
        the odometry chain and the `accepted` loops --: rule 3's residual r of the candidate at the store's poses, and
        capi.pg_mahalanobis(r, S_rel, w) with S_rel the pair's relative covariance (KeyframeCovariances) -> (d2 (len(loops),), the
        KeyframeCovariances dict).  A candidate that lies within what the trajectory's uncertainty allows has d2 of the order of 3."""
        loops = list(loops)
        cov = self.KeyframeCovariances([(int(l[0]), int(l[1])) for l in loops], odom_w, loops=accepted, spec=spec, fixed=fixed)
        _, kp = self.MapRep.SigDownload()
        poses = kp.astype(np.float64)
        d2 = np.zeros(len(loops))
        for k, (i, j, zl, wl) in enumerate(loops):
            ux, uy, dt = capi.pg_edge_between(poses[int(i)], poses[int(j)])
            r = np.array([ux - zl[0], uy - zl[1], math.remainder(dt - zl[2], 2.0 * math.pi)])
            d2[k] = capi.pg_mahalanobis(r, cov["rel"][k], wl)
        return d2, cov

    def RelaxKeyframes(self, loops, odom_w, spec, fixed=None, precond="jacobi", lm=None):
        """Spread verified loops over the keyframe store's poses (host composition of slamhip_hs_pg_set, _pg_relax, _pg_get,
        _pg_residuals and slamhip_hs_sig_set_poses; no reference counterpart).  Nodes: the store's poses; an odometry edge joins every
        pair of consecutive keyframes, its z formed from their stored poses (capi.pg_edge_between), its weights odom_w = (wx, wy,
        wtheta); one more edge per entry (i, j, z, w) of `loops`, as the caller derives it from VerifyLoop; node 0 is fixed unless
        `fixed` says otherwise; precond as MapRepMultiMap.PgRelax takes it ("tri" fits this graph).  The relaxed poses are written back to the store (rounded to binary32, as it keeps them)
        -> (poses (N, 3) float64, iters, per-edge chi2 at the relaxed poses: the N - 1 odometry edges, then the loops).
        lm: a capi.pg_lm_spec record -- the graph is then relaxed by MapRepMultiMap.PgRelaxLM instead, `robust` set on exactly the loop
        edges (spec and precond are not read: the record has its own), iters are capi.PG_LM_ITER records, and a fourth value follows:
        f, every edge's factor at the relaxed poses in chi2's order."""
        rep = self.MapRep
        poses, ij, _, _ = self._keyframe_graph(loops, odom_w, fixed)
        N = poses.shape[0]
        f = None
        if lm is None:
            iters, _ = rep.PgRelax(spec, precond=precond)
        else:
            iters, _, f = rep.PgRelaxLM(lm, robust=np.arange(len(ij)) >= N - 1)
        out = rep.PgGet()
        _, chi2 = rep.PgResiduals()
        rep.SigSetPoses(out.astype(np.float32))
        return (out, iters, chi2) if lm is None else (out, iters, chi2, f)

    def ConsistentLoops(self, loops, spec):
        """MapRep.LoopsConsistent over the keyframe store's poses as they stand: loops as RelaxKeyframes takes them, entries
        (i, j, z, w); spec a capi.loops_spec record -> LoopsConsistent's dict.  keep says which entries to hand to RelaxKeyframes."""
        _, kp = self.MapRep.SigDownload()
        ij = np.array([(int(l[0]), int(l[1])) for l in loops], np.int32).reshape(-1, 2)
        z = np.array([l[2] for l in loops], np.float64).reshape(-1, 3); w = np.array([l[3] for l in loops], np.float64).reshape(-1, 3)
        return self.MapRep.LoopsConsistent(kp.astype(np.float64), ij, z, w, spec)

    def scans_match(self, spec, pairs):
        """MapRep.scans_match through the processor (slamhip_hsproc_scans_match): relative poses, no frame to convert."""
        return capi.scans_match_call("slamhip_hsproc_scans_match", self._h, spec, pairs)

    def close_loops(self, min_gap, spec, accept, odom_w=(400.0, 400.0, 2500.0), pg=None, render=False, guess_from_poses=False, precond="jacobi", consistency=None, lm=None):
        """Close the loops of the keyframe store (host composition; AddKeyframe with keep_scan first): SelfLoopCandidates(min_gap) names
        one candidate per keyframe; its guess is (0, 0, -shift 2 pi / 64) by K18's sign rule -- or, with guess_from_poses, the
        translation between the two stored poses in the candidate's frame; scans_match turns the candidates into edges (keyframe
        hit.index -> keyframe i) and `accept`, the caller's predicate over a capi.SCANMATCH_RESULT record (score, n_query, cnt), filters
        them: the library sets no threshold.  RelaxKeyframes then adds the odometry edges of consecutive stored poses (weights odom_w),
        relaxes (pg: a capi.pg_spec record; default 5 steps of 4 N iterations; precond: RelaxKeyframes') and writes the poses back; render=True draws the
        stored scans again at them (RenderKeyframes), render="world" into the window and the backing tiles (RenderKeyframesWorld).  -> dict(pairs, results, z, w, accepted (bool array), poses, iters, chi2);
        without an accepted edge nothing is relaxed and poses is None.  consistency: a capi.loops_spec record -- the accepted edges are
        then cut down to their largest mutually consistent set (ConsistentLoops) before they are relaxed, and the dict gains
        consistent (bool array over the pairs: accepted and kept) and loops_info (the capi.LOOPS_INFO record); None: no such step.
        lm: a capi.pg_lm_spec record, handed to RelaxKeyframes (pg and precond are then not read); the dict gains f."""
        hits = self.SelfLoopCandidates(min_gap)
        _, kp = self.MapRep.SigDownload()
        pairs = []
        for i, h in enumerate(hits):
            j = int(h["index"])
            if j < 0:
                continue
            th = -int(h["shift"]) * 2.0 * math.pi / capi.SIG_SECTORS
            g = (0.0, 0.0, math.remainder(th, 2.0 * math.pi))
            if guess_from_poses:
                zz = capi.pg_edge_between(kp[j], kp[i])
                g = (zz[0], zz[1], g[2])
            pairs.append((j, i, g))
        out = dict(pairs=pairs, results=None, z=None, w=None, accepted=np.zeros(0, bool), poses=None, iters=None, chi2=None)
        if not pairs:
            return out
        res = self.scans_match(spec, pairs)
        z, w, valid = capi.scans_edges(spec, pairs, res)
        ok = np.array([bool(valid[n]) and bool(accept(res[n])) for n in range(len(pairs))], bool)
        out.update(results=res, z=z, w=w, accepted=ok)
        loops = [(pairs[n][0], pairs[n][1], z[n], w[n]) for n in range(len(pairs)) if ok[n]]
        if consistency is not None:
            out.update(consistent=np.zeros(len(pairs), bool), loops_info=None)
            if loops:
                cl = self.ConsistentLoops(loops, consistency)
                out["consistent"][np.flatnonzero(ok)[cl["keep"]]] = True
                out["loops_info"] = cl["info"]
                loops = [l for l, k in zip(loops, cl["keep"]) if k]
        if not loops:
            return out
        N = kp.shape[0]
        relaxed = self.RelaxKeyframes(loops, odom_w, capi.pg_spec(5, 4 * N, tol=1e-8) if pg is None else pg, precond=precond, lm=lm)
        out.update(poses=relaxed[0], iters=relaxed[1], chi2=relaxed[2])
        if lm is not None:
            out.update(f=relaxed[3])
        if isinstance(render, str):
            if render != "world":
                raise ValueError("close_loops: render = %r must be False, True or \"world\"" % (render,))
            self.RenderKeyframesWorld()
        elif render:
            self.RenderKeyframes()
        return out

    def LocaliseInit(self, poses_world):
        """Start Monte-Carlo localisation: the particle set of the processor's own pyramid (MapRep.mcl_set) from WORLD poses, taken to
        the window's frame as Relocalise takes its centre (- (float)origin * cell0 per axis)."""
        p = capi.f32(poses_world, (-1, 3)).copy()
        off = self._window_offset()
        if self.get_origin() != (0, 0):
            p[:, 0] = p[:, 0] - off[0]; p[:, 1] = p[:, 1] - off[1]
        self.MapRep.mcl_set(p)
        self._mcl_origin = self.get_origin()

    def LocaliseStep(self, scan, odometry_delta, sigma, level, beta, n_eff_min, seed=0, stream=0, site_mask=2, radius=32, world=False):
        """One localisation step (slamhip_hsproc_mcl_step): odometry_delta = (dx, dy, dth) in the robot's frame since the last step,
        sigma the noise scales.  If the window has scrolled since the last step, the particles -- window-frame poses -- are re-based by
        frame_offset = -(the window's movement in metres).  -> (poseWorld, n_eff, n_distinct, summary): the weighted-mean pose in
        the world frame (float64), A^2 / Q, the distinct ancestors, the capi.MCL_SUMMARY record.  MatchPose, LastMapUpdatePose, the
        update gate and the map are untouched; the caller advances `stream` per step."""
        if self._mcl_origin is None:
            raise ValueError("LocaliseStep: no particle set (LocaliseInit first)")
        org_now = self.get_origin()
        was = self._mcl_origin
        cell0 = np.float32(self.MapRep.Maps[0].CellLength)
        fo = (-(np.float32(org_now[0] - was[0]) * cell0), -(np.float32(org_now[1] - was[1]) * cell0))
        spec = capi.mcl_spec(level, radius, odometry_delta, sigma, beta, n_eff_min, seed, stream, site_mask, world, fo)
        org = capi.f32(scan.Pose[:2])
        out = np.zeros(1, capi.MCL_SUMMARY)
        capi.call("slamhip_hsproc_mcl_step", self._h, capi.fptr(scan.Points), scan.Points.shape[0], capi.fptr(org), spec.ctypes.data_as(C.c_void_p),
                  out.ctypes.data_as(C.c_void_p))
        self.MapRep._scan_set = (scan.Points.shape[0], org.copy())
        self._mcl_origin = org_now
        off = self._window_offset()
        pose, n_eff = capi.mcl_mean(out[0], (float(off[0]), float(off[1])) if org_now != (0, 0) else (0.0, 0.0))
        return pose, n_eff, int(out[0]["n_distinct"]), out[0]

    def PoseCell(self, level):
        """The WORLD cell of `level` that MatchPose lies in: the pose over the level's CellLength, rounded as the grid update rounds
        an end point (to nearest, ties to even)."""
        cell = float(np.float32(self.MapRep.Maps[level].CellLength))
        m = self.MatchPose
        return int(np.rint(float(m[0]) / cell)), int(np.rint(float(m[1]) / cell))

    MatchPose = property(lambda self: self._get()[0])
    LastMapUpdatePose = property(lambda self: self._get()[1])
    MatchTiming = property(lambda self: self._get()[2])
    UpdateTiming = property(lambda self: self._get()[3])

    @property
    def LastMatchReport(self):
        """The report of the last Update's match (a capi.REPORT_DTYPE record), or None: before the first match, after
        Reset, after an Update with mapWithoutMatching, and when the processor was made without matchReport."""
        r = np.zeros(1, capi.REPORT_DTYPE); valid = C.c_int32()
        capi.call("slamhip_hsproc_get_report", self._h, capi.rptr(r), C.byref(valid))
        return r[0] if valid.value else None

    @property
    def MinDistanceDiffForMapUpdate(self):
        return self._min_dist

    @MinDistanceDiffForMapUpdate.setter
    def MinDistanceDiffForMapUpdate(self, v):
        self._min_dist = float(v)
        capi.call("slamhip_hsproc_set_thresholds", self._h, C.c_float(self._min_dist), C.c_float(self._min_angle))

    @property
    def MinAngleDiffForMapUpdate(self):
        return self._min_angle

    @MinAngleDiffForMapUpdate.setter
    def MinAngleDiffForMapUpdate(self, v):
        self._min_angle = float(v)
        capi.call("slamhip_hsproc_set_thresholds", self._h, C.c_float(self._min_dist), C.c_float(self._min_angle))

    def Update(self, scan, poseHintWorld, mapWithoutMatching=False):
        hint = capi.f32(poseHintWorld); org = capi.f32(scan.Pose[:2]); upd = C.c_int32()
        capi.call("slamhip_hsproc_update", self._h, capi.fptr(scan.Points), scan.Points.shape[0], capi.fptr(org),
                  capi.fptr(hint), 1 if mapWithoutMatching else 0, C.byref(upd))
        self.MapRep._scan_set = (scan.Points.shape[0], org.copy())      # (what MapRep.trace sizes its beam records by)
        return bool(upd.value)

    def Reset(self):
        capi.call("slamhip_hsproc_reset", self._h)

    def Dispose(self):
        if self._h:
            capi.lib().slamhip_hsproc_destroy(self._h)
            self._h = C.c_void_p()
        if self._own_ctx:
            self.ctx.close()
