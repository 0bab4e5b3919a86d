"""ctypes binding of include/slamhip.h -- one Python function per C-ABI entry point, nothing else.

Loading fails loudly when libslamhip.so is missing (run ``python -m slam.net_amd.build`` or
``__graft_entry__.build()``); there is no CPU fallback in this package.
"""
import ctypes as C
import math
import os
import re

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(_HERE, "libslamhip.so")
HEADER = os.path.join(os.path.dirname(_HERE), "include", "slamhip.h")

OK = 0
ERR_INVALID, ERR_HIP, ERR_NOMEM, ERR_STATE, ERR_RCCL, ERR_TIMEOUT = -1, -2, -3, -4, -5, -6
K_CS_PREP, K_CS_DISTANCE, K_CS_REDUCE, K_CS_HOLEMAP, K_CS_OBSTACLE, K_HS_MATCH, K_HS_UPDATE, K_HS_LATTICE_PACK, K_HS_LATTICE = range(9)
K_HS_LATTICE_PACK_WORLD = 9

CELL_DTYPE = np.dtype([("update_index", np.int32), ("value", np.float32)])


class MatchReport(C.Structure):
    """slamhip_match_report (include/slamhip.h): 19 four-byte fields, 76 bytes, no padding."""
    _fields_ = [("pose_map", C.c_float * 3), ("H", C.c_float * 9), ("dTr", C.c_float * 3), ("residual", C.c_float),
                ("n_in_map", C.c_int32), ("n_points", C.c_int32), ("level", C.c_int32)]


# ... the same layout for arrays of reports (slamhip_hs_match_batch_report)
REPORT_DTYPE = np.dtype([("pose_map", np.float32, 3), ("H", np.float32, (3, 3)), ("dTr", np.float32, 3),
                         ("residual", np.float32), ("n_in_map", np.int32), ("n_points", np.int32), ("level", np.int32)])
assert C.sizeof(MatchReport) == REPORT_DTYPE.itemsize == 76


class SearchReport(C.Structure):
    """slamhip_search_report (include/slamhip.h): 9 doubles + 12 int32, 120 bytes, no padding."""
    _fields_ = [("sum_off", C.c_double * 3), ("sum_off2", C.c_double * 6), ("best_dist", C.c_int32), ("best_index", C.c_int32),
                ("runner_dist", C.c_int32), ("runner_index", C.c_int32), ("dist0", C.c_int32), ("n_candidates", C.c_int32),
                ("n_unscored", C.c_int32), ("n_ties", C.c_int32), ("band", C.c_int32), ("n_band", C.c_int32),
                ("n_in_map", C.c_int32), ("n_points", C.c_int32)]


SEARCH_REPORT_DTYPE = np.dtype([("sum_off", np.float64, 3), ("sum_off2", np.float64, 6), ("best_dist", np.int32), ("best_index", np.int32),
                                ("runner_dist", np.int32), ("runner_index", np.int32), ("dist0", np.int32), ("n_candidates", np.int32),
                                ("n_unscored", np.int32), ("n_ties", np.int32), ("band", np.int32), ("n_band", np.int32),
                                ("n_in_map", np.int32), ("n_points", np.int32)])
assert C.sizeof(SearchReport) == SEARCH_REPORT_DTYPE.itemsize == 120


class BackingStats(C.Structure):
    """slamhip_backing_stats (include/slamhip.h): 6 int64 + 2 int32, 56 bytes."""
    _fields_ = [("tiles", C.c_int64), ("bytes", C.c_int64), ("capacity_bytes", C.c_int64), ("evicted_cells", C.c_int64),
                ("restored_cells", C.c_int64), ("dropped_cells", C.c_int64), ("tile", C.c_int32), ("on", C.c_int32)]


class BackingJob(C.Structure):
    """slamhip_backing_job (include/slamhip.h): one job of the backing store's planner, 48 bytes."""
    _fields_ = [("level", C.c_int32), ("kind", C.c_int32), ("wx", C.c_int32), ("wy", C.c_int32), ("nx", C.c_int32), ("ny", C.c_int32),
                ("tx", C.c_int64), ("ty", C.c_int64), ("lx", C.c_int32), ("ly", C.c_int32)]


BACKING_EVICT, BACKING_RESTORE = 0, 1
BACKING_JOB_DTYPE = np.dtype([("level", np.int32), ("kind", np.int32), ("wx", np.int32), ("wy", np.int32), ("nx", np.int32), ("ny", np.int32),
                              ("tx", np.int64), ("ty", np.int64), ("lx", np.int32), ("ly", np.int32)])
assert C.sizeof(BackingStats) == 56 and C.sizeof(BackingJob) == BACKING_JOB_DTYPE.itemsize == 48


class WorldJob(C.Structure):
    """slamhip_world_job (include/slamhip.h): one job of the world upload's planner, 48 bytes."""
    _fields_ = [("kind", C.c_int32), ("sx", C.c_int32), ("sy", C.c_int32), ("nx", C.c_int32), ("ny", C.c_int32), ("lx", C.c_int32),
                ("ly", C.c_int32), ("pad", C.c_int32), ("tx", C.c_int64), ("ty", C.c_int64)]


WORLD_WINDOW, WORLD_TILE = 0, 1
WORLD_JOB_DTYPE = np.dtype([("kind", np.int32), ("sx", np.int32), ("sy", np.int32), ("nx", np.int32), ("ny", np.int32), ("lx", np.int32),
                            ("ly", np.int32), ("pad", np.int32), ("tx", np.int64), ("ty", np.int64)])
assert C.sizeof(WorldJob) == WORLD_JOB_DTYPE.itemsize == 48


class LATTICE_SPEC(C.Structure):
    """slamhip_lattice_spec (include/slamhip.h): the pose lattice of slamhip_hs_lattice_search, 8 four-byte fields, 32 bytes."""
    _fields_ = [("level", C.c_int32), ("nx", C.c_int32), ("ny", C.c_int32), ("n_theta", C.c_int32), ("centre", C.c_float * 3),
                ("dtheta", C.c_float)]


class RelocInfo(C.Structure):
    """slamhip_reloc_info (include/slamhip.h): 7 int32, 28 bytes."""
    _fields_ = [("n_hints", C.c_int32), ("best_hint", C.c_int32), ("k", C.c_int32), ("ix", C.c_int32), ("iy", C.c_int32),
                ("score", C.c_int32), ("top_score", C.c_int32)]


RELOC_INFO = np.dtype([("n_hints", np.int32), ("best_hint", np.int32), ("k", np.int32), ("ix", np.int32), ("iy", np.int32),
                       ("score", np.int32), ("top_score", np.int32)])
assert C.sizeof(LATTICE_SPEC) == 32 and C.sizeof(RelocInfo) == RELOC_INFO.itemsize == 28


class WorldRelocInfo(C.Structure):
    """slamhip_world_reloc_info (include/slamhip.h): the fields of slamhip_reloc_info, then dx, dy, n_far; 10 int32, 40 bytes."""
    _fields_ = RelocInfo._fields_ + [("dx", C.c_int32), ("dy", C.c_int32), ("n_far", C.c_int32)]


WORLD_RELOC_INFO = np.dtype([(n, np.int32) for n, _ in WorldRelocInfo._fields_])
assert C.sizeof(WorldRelocInfo) == WORLD_RELOC_INFO.itemsize == 40


BNB_MAX_TOP = 8                                                # the limit of slamhip_bnb_spec.top


class BNB_SPEC(C.Structure):
    """slamhip_bnb_spec (include/slamhip.h): the lattice, then top, world, max_blocks, reserved; 48 bytes."""
    _fields_ = [("lattice", LATTICE_SPEC), ("top", C.c_int32), ("world", C.c_int32), ("max_blocks", C.c_int32), ("reserved", C.c_int32)]


class BnbInfo(C.Structure):
    """slamhip_bnb_info (include/slamhip.h): 88 bytes."""
    _fields_ = [("top", C.c_int32), ("n_levels", C.c_int32), ("evaluated", C.c_int64), ("blocks", C.c_int32 * 9), ("kept", C.c_int32 * 9)]


BNB_INFO = np.dtype([("top", np.int32), ("n_levels", np.int32), ("evaluated", np.int64), ("blocks", np.int32, (9,)), ("kept", np.int32, (9,))])
assert C.sizeof(BNB_SPEC) == 48 and C.sizeof(BnbInfo) == BNB_INFO.itemsize == 88


TRACE_MAX_DA = 32768
TRACE_BEAM = np.dtype([("da", np.int32), ("first", np.int32), ("n_unknown", np.int32), ("end_class", np.int32), ("hx", np.int32),
                       ("hy", np.int32)])                  # slamhip_trace_beam (include/slamhip.h): 6 int32, 24 bytes
TRACE_SUMMARY = np.dtype([("n_walked", np.int32), ("n_same", np.int32), ("n_ignored", np.int32), ("n_end_hit", np.int32),
                          ("n_blocked", np.int32), ("n_end_free", np.int32), ("unknown_cells", np.int64)])   # slamhip_trace_summary: 32 bytes
assert TRACE_BEAM.itemsize == 24 and TRACE_SUMMARY.itemsize == 32
DISTANCE_SUMMARY = np.dtype([("n_counted", np.int32), ("n_ignored", np.int32), ("n_zero", np.int32), ("n_capped", np.int32),
                             ("sum_d2", np.int64)])            # slamhip_distance_summary (include/slamhip.h): 4 int32 + 1 int64, 24 bytes
assert DISTANCE_SUMMARY.itemsize == 24
DISTANCE_IGNORED = 0xFFFF                                      # the per-point record of an ignored point
PAIR_SUMMARY = np.dtype([(n, np.int32) for n in ("n_counted", "n_ignored", "n_matched", "n_zero")] +
                        [(n, np.int64) for n in ("sum_d2", "sum_ex", "sum_ey", "sum_qx", "sum_qy", "sum_exqx", "sum_eyqy", "sum_exqy",
                                                 "sum_eyqx")])     # slamhip_pair_summary (include/slamhip.h): 4 int32 + 9 int64, 88 bytes
assert PAIR_SUMMARY.itemsize == 88
NEAREST_NONE, NEAREST_IGNORED = 32767, -32768                  # SLAMHIP_NEAREST_NONE / _IGNORED: both components of the pair
FRONTIER_MAX_CLUSTERS = 65536
FRONTIER_CLUSTER = np.dtype([("seed_x", np.int32), ("seed_y", np.int32), ("n_cells", np.int32), ("n_runs", np.int32), ("x_min", np.int32),
                             ("y_min", np.int32), ("x_max", np.int32), ("y_max", np.int32), ("sum_x", np.int64),
                             ("sum_y", np.int64)])             # slamhip_frontier_cluster (include/slamhip.h): 8 int32 + 2 int64, 48 bytes
FRONTIER_SUMMARY = np.dtype([(n, np.int32) for n in ("mx0", "my0", "mw", "mh", "n_frontier_cells", "n_runs", "n_clusters", "n_kept",
                                                     "n_returned", "kept_cells")])   # slamhip_frontier_summary: 10 int32, 40 bytes
assert FRONTIER_CLUSTER.itemsize == 48 and FRONTIER_SUMMARY.itemsize == 40
NAV_UNREACHED = 0xFFFFFFFF                                     # SLAMHIP_NAV_UNREACHED: the cost of an unreached cell
NAV_DIR_SOURCE, NAV_DIR_NONE = 8, 255
NAV_DX = (1, 1, 0, -1, -1, -1, 0, 1)                           # the direction table of slamhip_hs_nav_field, step 3
NAV_DY = (0, 1, 1, 1, 0, -1, -1, -1)
NAV_MAX_SOURCES, NAV_MAX_GOALS, NAV_MAX_PATHS, NAV_MAX_PATH_CELLS = 4096, 4096, 64, 65536
NAV_SPEC = np.dtype([("level", np.int32), ("world", np.int32), ("site_mask", np.int32), ("clearance", np.int32),
                     ("max_cost", np.uint32)])                 # slamhip_nav_spec (include/slamhip.h): 5 words, 20 bytes
NAV_GOAL_RESULT = np.dtype([("cost", np.uint32), ("bx", np.int32), ("by", np.int32), ("n_reached", np.int32)])   # slamhip_nav_goal_result: 16 bytes
NAV_PATH = np.dtype([("n_cells", np.int32), ("n_written", np.int32)])                                            # slamhip_nav_path: 8 bytes
NAV_SUMMARY = np.dtype([(n, np.int32) for n in ("mx0", "my0", "mw", "mh", "n_traversable", "n_reached", "n_sources_used",
                                                "n_sources_blocked")] + [("max_cost_reached", np.uint32), ("rounds", np.int32)])   # slamhip_nav_summary: 40 bytes
assert NAV_SPEC.itemsize == 20 and NAV_GOAL_RESULT.itemsize == 16 and NAV_PATH.itemsize == 8 and NAV_SUMMARY.itemsize == 40
ROLLOUT_MAX_B, ROLLOUT_MAX_CMD, ROLLOUT_MAX_T, ROLLOUT_MAX_POINTS = 65536, 256, 1024, 32   # the limits of slamhip_hs_rollouts
ROLLOUT_RESULT = np.dtype([("n_free", np.int32), ("min_step", np.int32), ("end_cost", np.uint32), ("min_cost", np.uint32),
                           ("x", np.float32), ("y", np.float32), ("theta", np.float32)])   # slamhip_rollout_result: 7 words, 28 bytes
ROLLOUT_SUMMARY = np.dtype([("nav", NAV_SUMMARY), ("start_cost", np.uint32), ("n_complete", np.int32), ("key_end", np.uint64),
                            ("key_min", np.uint64)])           # slamhip_rollout_summary: 64 bytes, no padding
ROLLOUT_NO_KEY = 0xFFFFFFFFFFFFFFFF                            # key_end / key_min when no rollout qualifies
assert ROLLOUT_RESULT.itemsize == 28 and ROLLOUT_SUMMARY.itemsize == 64
MCL_MAX_N, MCL_MAX_POINTS = 65536, 7680                        # the limits of slamhip_hs_mcl_set / slamhip_hs_mcl_step
MCL_SPEC = np.dtype([("level", np.int32), ("world", np.int32), ("site_mask", np.int32), ("radius", np.int32), ("delta", np.float32, (3,)),
                     ("sigma", np.float32, (3,)), ("frame_offset", np.float32, (2,)), ("beta", np.uint32), ("n_eff_min", np.int32),
                     ("seed", np.uint64), ("stream", np.uint64)])          # slamhip_mcl_spec (include/slamhip.h): 72 bytes, no padding
MCL_SUMMARY = np.dtype([("W", np.uint64), ("A", np.uint64), ("Q", np.uint64), ("key_best", np.uint64), ("sum_hx", np.int64), ("sum_hy", np.int64),
                        ("sum_hc", np.int64), ("sum_hs", np.int64), ("cost_min", np.uint64), ("cost_max", np.uint64), ("resampled", np.int32),
                        ("n_distinct", np.int32), ("n_unplaced", np.int32), ("n_particles", np.int32)])   # slamhip_mcl_summary: 96 bytes
assert MCL_SPEC.itemsize == 72 and MCL_SUMMARY.itemsize == 96
MERGE_MAX_CELLS, MERGE_MAX_POSES = 1 << 26, 4096                # the limits of slamhip_hs_merge_set_source / slamhip_hs_merge_score
MERGE_ADD, MERGE_FILL, MERGE_REPLACE = 0, 1, 2                  # the rules of slamhip_hs_merge_apply
MERGE_REPORT = np.dtype([("joint", np.int64, (9,)), ("n_unsourced", np.int64), ("n_changed", np.int64), ("n_clamped", np.int64)])   # slamhip_merge_report
assert MERGE_REPORT.itemsize == 96
HOUGH_MAX_T, HOUGH_MAX_Q, HOUGH_MAX_DIM, HOUGH_MAX_BINS, HOUGH_MAX_PAIRS, HOUGH_MAX_XC = 1024, 3, 16384, 1 << 24, 256, 1 << 22   # the limits of slamhip_hs_hough / _hough_shifts
HOUGH_SHIFT = np.dtype([("best_shift", np.int32), ("n_ties", np.int32), ("best_value", np.uint64), ("sum", np.uint64)])   # slamhip_hough_shift
assert HOUGH_SHIFT.itemsize == 24
SIG_SECTORS, SIG_MAX_RINGS, SIG_MAX_HITS, SIG_MAX_KEYS, SIG_MAX_SCANS = 64, 32, 16, 1 << 20, 4096   # the limits of slamhip_hs_sig_*
SIG_SPEC = np.dtype([("scale", np.float32), ("n_ring", np.int32), ("ring_cells", np.int32)])            # slamhip_sig_spec: 12 bytes
SIG_INFO = np.dtype([(n, np.int32) for n in ("n_points", "n_ignored", "n_far", "n_set")])              # slamhip_sig_info: 16 bytes
SIG_HIT_DTYPE = np.dtype([("score", np.uint32), ("index", np.int32), ("shift", np.int16), ("inter", np.int16), ("uni", np.int16),
                          ("n_set_key", np.int16)])                                                     # slamhip_sig_hit: 16 bytes
assert SIG_SPEC.itemsize == 12 and SIG_INFO.itemsize == 16 and SIG_HIT_DTYPE.itemsize == 16
RENDER_KEEP = 1                                                # SLAMHIP_RENDER_KEEP: slamhip_hs_render starts from what the pyramid holds
RENDER_MAX_SCANS = 1 << 20                                     # the scan store's limit
PG_MAX_NODES, PG_MAX_EDGES, PG_MAX_OUTER, PG_MAX_CG = 1 << 20, 1 << 22, 64, 1 << 20   # the limits of slamhip_hs_pg_*
PG_SPEC = np.dtype([("n_outer", np.int32), ("n_cg", np.int32), ("check_every", np.int32), ("reserved", np.int32), ("lambda", np.float64),
                    ("tol", np.float64)])                                                           # slamhip_pg_spec: 32 bytes
PG_ITER = np.dtype([("chi2", np.float64), ("rz0", np.float64), ("rz", np.float64), ("cg_iters", np.int32), ("stopped", np.int32)])   # slamhip_pg_iter: 32 bytes
assert PG_SPEC.itemsize == 32 and PG_ITER.itemsize == 32
PG_LM_NONE, PG_LM_DCS, PG_LM_GM = 0, 1, 2                                                          # slamhip_pg_lm_spec.kind
PG_LM_SPEC = np.dtype([("n_outer", np.int32), ("n_cg", np.int32), ("check_every", np.int32), ("precond", np.int32), ("kind", np.int32),
                       ("reserved", np.int32), ("lambda0", np.float64), ("up", np.float64), ("down", np.float64), ("lambda_min", np.float64),
                       ("lambda_max", np.float64), ("tol", np.float64), ("ftol", np.float64), ("phi", np.float64)])   # slamhip_pg_lm_spec: 88 bytes
PG_LM_ITER = np.dtype([("F", np.float64), ("F_trial", np.float64), ("lambda", np.float64), ("rz0", np.float64), ("rz", np.float64),
                       ("cg_iters", np.int32), ("stopped", np.int32), ("accepted", np.int32), ("reserved", np.int32, (3,))])   # slamhip_pg_lm_iter: 64 bytes
assert PG_LM_SPEC.itemsize == 88 and PG_LM_ITER.itemsize == 64
PG_MARG_MAX_PAIRS, PG_MARG_MAX_COLS, PG_MARG_GROUP = 1 << 20, 4096, 1                              # the limits of slamhip_hs_pg_marginals; k27's default G
PG_MARG_SPEC = np.dtype([("n_cg", np.int32), ("check_every", np.int32), ("precond", np.int32), ("reserved", np.int32), ("lambda", np.float64),
                         ("tol", np.float64), ("max_bytes", np.int64)])                            # slamhip_pg_marg_spec: 40 bytes
PG_MARG_COL = np.dtype([("rz0", np.float64), ("rz", np.float64), ("cg_iters", np.int32), ("stopped", np.int32), ("node", np.int32),
                        ("comp", np.int32)])                                                        # slamhip_pg_marg_col: 32 bytes
PG_MARG_INFO = np.dtype([("n_cols", np.int32), ("n_rhs", np.int32), ("rhs_per_chunk", np.int32), ("n_chunks", np.int32), ("group", np.int32),
                         ("reserved", np.int32, (3,))])                                             # slamhip_pg_marg_info: 32 bytes
assert PG_MARG_SPEC.itemsize == 40 and PG_MARG_COL.itemsize == 32 and PG_MARG_INFO.itemsize == 32
SCANMATCH_MAX_HALF, SCANMATCH_MAX_N, SCANMATCH_MAX_PAIRS, SCANMATCH_MAX_NODES, SCANMATCH_MAX_CALL_NODES = 192, 64, 4096, 1 << 20, 1 << 26   # the limits of slamhip_hs_scans_match
SCANMATCH_SPEC = np.dtype([("scale", np.float32), ("half", np.int32), ("nx", np.int32), ("ny", np.int32), ("nt", np.int32), ("dtheta", np.float32),
                           ("margin", np.int32), ("reserved", np.int32)])                                # slamhip_scanmatch_spec: 32 bytes
SCAN_PAIR = np.dtype([("ref", np.int32), ("query", np.int32), ("guess", np.float32, (3,))])             # slamhip_scan_pair: 20 bytes
SCANMATCH_RESULT = np.dtype([(n, np.int32) for n in ("k", "ix", "iy", "score", "n_ref", "n_query", "cnt", "reserved")] +
                            [(n, np.int64) for n in ("sum_x", "sum_y", "sum_k", "sum_xx", "sum_yy", "sum_kk", "sum_xy", "sum_xk", "sum_yk")])   # slamhip_scanmatch_result: 104 bytes
assert SCANMATCH_SPEC.itemsize == 32 and SCAN_PAIR.itemsize == 20 and SCANMATCH_RESULT.itemsize == 104
LOOPS_MAX_EDGES, LOOPS_MAX_NODES, LOOPS_MAX_STARTS, LOOPS_ADJ = 4096, 1 << 20, 64, 1          # the limits of slamhip_hs_loops_consistent; SLAMHIP_LOOPS_ADJ
LOOPS_LDS_ADJ_BYTES = 144 * 1024                               # HS_LP_LDS_ADJ_BYTES: k23_clique keeps the matrix in LDS while L * (ceil(L / 64) | 1) * 8 is at most this
LOOPS_SPEC = np.dtype([("gamma", np.float64), ("q_t", np.float64), ("q_theta", np.float64), ("n_starts", np.int32), ("min_clique", np.int32),
                       ("flags", np.int32), ("reserved", np.int32)])                                    # slamhip_loops_spec: 40 bytes
LOOPS_INFO = np.dtype([("n_pairs", np.int64), ("n_used", np.int32), ("size", np.int32), ("start", np.int32), ("rank", np.int32),
                       ("n_starts", np.int32), ("reserved", np.int32)])                                 # slamhip_loops_info: 32 bytes
assert LOOPS_SPEC.itemsize == 40 and LOOPS_INFO.itemsize == 32
VIEW_MAX_REACH, VIEW_MAX_POSES, VIEW_MAX_K, VIEW_LDS_WORDS = 4096, 4096, 64, 8704   # the limits of slamhip_hs_view_gain / _view_select; K15_LDS_WORDS
VIEW_SUMMARY = np.dtype([(n, np.int32) for n in ("n_walked", "n_same", "n_ignored", "n_cut", "n_seen", "n_unknown", "n_free", "n_occupied", "n_new",
                                                 "n_new_unknown")])   # slamhip_view_summary: ten int32, 40 bytes
assert VIEW_SUMMARY.itemsize == 40


def lattice_spec(level, centre, nx, ny, n_theta, dtheta):
    """A LATTICE_SPEC from Python values (centre rounded to binary32 as f32 rounds it)."""
    c = f32(centre, (3,))
    return LATTICE_SPEC(int(level), int(nx), int(ny), int(n_theta), (C.c_float * 3)(*[float(v) for v in c]), float(np.float32(dtheta)))


def bnb_spec(level, centre, nx, ny, n_theta, dtheta, top, world=False, max_blocks=0, reserved=0):
    """A BNB_SPEC from Python values: lattice_spec's lattice, then the fields of the branch-and-bound search."""
    return BNB_SPEC(lattice_spec(level, centre, nx, ny, n_theta, dtheta), int(top), int(world), int(max_blocks), int(reserved))


def bnb_info(info):
    """A BnbInfo as a BNB_INFO record."""
    return np.frombuffer(bytes(info), BNB_INFO)[0].copy()


class SlamhipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("slamhip error %d: %s" % (code, msg))
        self.code = code


_lib = None


def declared_symbols():
    """Every function name declared in include/slamhip.h."""
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(slamhip_[a-z0-9_]+)\s*\(", txt)))


def lib():
    global _lib
    if _lib is None:
        so = os.environ.get("SLAMHIP_LIB") or SO_PATH            # (developer aid: an alternative build of the same ABI, for A/B timing on one box)
        if not os.path.exists(so):
            raise ImportError("libslamhip.so not built at %s -- build it with hipcc (python -m slam.net_amd.build); "
                              "slam.net_amd has no CPU fallback" % so)
        L = C.CDLL(so)
        _declare(L)
        _lib = L
    return _lib


def _declare(L):
    i32, u64, i64, f, vp, sz = C.c_int32, C.c_uint64, C.c_int64, C.c_float, C.c_void_p, C.c_size_t
    P = C.POINTER
    fp, ip, u16p, i8p, u8p, u64p, vpp = P(f), P(i32), P(C.c_uint16), P(C.c_int8), P(C.c_uint8), P(u64), P(vp)
    rp = P(MatchReport)
    srp = P(SearchReport)
    lsp, rip, wrip = P(LATTICE_SPEC), P(RelocInfo), P(WorldRelocInfo)
    bsp, bip = P(BNB_SPEC), P(BnbInfo)
    sig = {
        "slamhip_version": (C.c_char_p, []),
        "slamhip_last_error": (C.c_char_p, []),
        "slamhip_device_count": (i32, [ip]),
        "slamhip_ctx_create": (i32, [i32, vpp]),
        "slamhip_ctx_destroy": (i32, [vp]),
        "slamhip_ctx_synchronize": (i32, [vp]),
        "slamhip_ctx_device": (i32, [vp, ip]),
        "slamhip_ctx_stream": (vp, [vp]),
        "slamhip_ctx_set_wait_timeout": (i32, [vp, i64]),
        "slamhip_ctx_poisoned": (i32, [vp, ip]),
        "slamhip_ctx_philox4x32_10": (i32, [vp, P(C.c_uint32), P(C.c_uint32), P(C.c_uint32)]),
        "slamhip_debug_flag_wait": (i32, [P(C.c_uint32), C.c_uint32, i64]),
        "slamhip_debug_live_blocks": (i32, [P(i64), P(i64)]),
        "slamhip_debug_backing_plan": (i32, [i32, i32, i32, i64, i64, i32, i32, i32, P(BackingJob), i32, ip]),
        "slamhip_debug_world_plan": (i32, [i32, i32, i64, i64, i64, i64, i32, i32, i32, P(WorldJob), i32, ip]),
        "slamhip_debug_lattice_cells": (i32, [f, fp, f, fp, i32, ip]),
        "slamhip_debug_lattice_bnb": (i32, [fp, i32, i32, f, bsp, fp, i32, u64p, bip]),
        "slamhip_debug_world_pack_plan": (i32, [i32, i32, i64, i64, i32, P(i64), i32, P(i64), P(WorldJob), i32, ip]),
        "slamhip_debug_trace_lines": (i32, [f, fp, fp, fp, i32, ip]),
        "slamhip_debug_trace_cells": (i32, [i32, i32, i32, i32, ip, i32, ip]),
        "slamhip_debug_distance_field": (i32, [vp, i32, i32, i32, i32, i32, i32, i32, i32, vp]),
        "slamhip_debug_nearest_field": (i32, [vp, i32, i32, i32, i32, i32, i32, i32, i32, vp]),
        "slamhip_debug_hough_table": (i32, [i32, vp]),
        "slamhip_debug_hough": (i32, [vp, i32, i32, i32, i32, i32, vp, vp]),
        "slamhip_debug_hough_rotation": (i32, [vp, vp, i32, vp]),
        "slamhip_debug_hough_xcorr": (i32, [vp, i32, vp, i32, i32, vp, vp]),
        "slamhip_debug_sig_table": (i32, [vp]),
        "slamhip_debug_sig": (i32, [vp, i32, vp, vp, vp]),
        "slamhip_debug_sig_ring": (i32, [vp, i32, i32, i32, vp]),
        "slamhip_debug_sig_sector": (i32, [vp, i32, vp]),
        "slamhip_debug_sig_search": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp]),
        "slamhip_debug_pg_relax": (i32, [vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp]),
        "slamhip_debug_pg_sum": (i32, [vp, i32, vp]),
        "slamhip_debug_pg_relax_tri": (i32, [vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp]),
        "slamhip_debug_pg_tri_apply": (i32, [vp, vp, i32, vp, vp, vp, i32, C.c_double, vp, vp]),
        "slamhip_debug_pg_relax_lm": (i32, [vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp]),
        "slamhip_debug_pg_marginals": (i32, [vp, vp, i32, vp, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp]),
        "slamhip_debug_scans_match": (i32, [vp, vp, i32, vp, vp, i32, vp]),
        "slamhip_debug_loops_consistent": (i32, [vp, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp]),
        "slamhip_debug_render": (i32, [i32, vp, f, vp, vp, vp, f, f, vp, vp, vp, vp, i32, i32]),
        "slamhip_debug_render_clip": (i32, [i32, i32, i32, i32, vp, vp, vp, vp]),
        "slamhip_debug_render_world": (i32, [i32, vp, f, vp, vp, vp, f, f, vp, vp, vp, vp, i32, i32]),
        "slamhip_debug_sincos": (i32, [vp, i32, vp, vp]),
        "slamhip_debug_frontiers": (i32, [vp, i32, i32, i32, i32, vp, vp, vp]),
        "slamhip_debug_nav_field": (i32, [vp, i32, i32, i32, i32, C.c_uint32, vp, i32, vp, i32, vp, i32, i32, vp, vp, i32, i32, i32, i32, vp, vp, vp]),
        "slamhip_debug_rollouts": (i32, [vp, i32, i32, i32, i32, C.c_uint32, vp, i32, C.c_float, vp, C.c_float, vp, i32, vp, i32, i32, i32, vp, vp]),
        "slamhip_debug_mcl_step": (i32, [vp, i32, i32, C.c_float, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp]),
        "slamhip_debug_mcl_table": (i32, [vp]),
        "slamhip_debug_merge": (i32, [vp, i32, i32, vp, i32, i32, i32, i32, fp, C.c_float, i32, C.c_float, vp, vp]),
        "slamhip_debug_merge_box": (i32, [fp, C.c_float, i32, i32, i32, i32, i32, i32, i32, i32, ip, ip]),
        "slamhip_debug_view": (i32, [fp, i32, i32, C.c_float, fp, fp, fp, i32, i32, vp, vp, vp]),
        "slamhip_ctx_timing_enable": (i32, [vp, i32]),
        "slamhip_ctx_timing_reset": (i32, [vp]),
        "slamhip_ctx_timing_get": (i32, [vp, i32, P(C.c_double), P(i64)]),
        "slamhip_cs_create": (i32, [vp, f, i32, i32, vpp]),
        "slamhip_cs_destroy": (i32, [vp]),
        "slamhip_cs_info": (i32, [vp, ip, fp, ip, fp]),
        "slamhip_cs_reset": (i32, [vp, i32]),
        "slamhip_cs_holemap_upload": (i32, [vp, u16p, sz]),
        "slamhip_cs_holemap_download": (i32, [vp, u16p, sz]),
        "slamhip_cs_holemap_download_packed": (i32, [vp, u8p, sz]),
        "slamhip_cs_holemap_mirror": (i32, [vp, u16p, sz, ip]),
        "slamhip_cs_holemap_mirror_async": (i32, [vp, u16p, sz]),
        "slamhip_cs_holemap_mirror_wait": (i32, [vp, ip, P(i64)]),
        "slamhip_cs_holemap_mirror_release": (i32, [vp]),
        "slamhip_cs_obstaclemap_upload": (i32, [vp, i8p, sz]),
        "slamhip_cs_obstaclemap_download": (i32, [vp, i8p, sz]),
        "slamhip_cs_set_scan": (i32, [vp, fp, i32]),
        "slamhip_cs_distance_pxcs": (i32, [vp, fp, i32, ip, ip, ip]),
        "slamhip_cs_distance_poses": (i32, [vp, fp, i32, ip, ip, ip]),
        "slamhip_cs_set_offsets": (i32, [vp, fp, i32]),
        "slamhip_cs_generate_offsets": (i32, [vp, i32, f, f, u64, u64]),
        "slamhip_cs_generate_offsets_lattice": (i32, [vp, i32, f, f, u64, u64]),
        "slamhip_cs_offsets_download": (i32, [vp, fp, i32]),
        "slamhip_cs_search": (i32, [vp, fp, fp, ip, ip]),
        "slamhip_cs_search_shard": (i32, [vp, fp, i32, i32, u64p]),
        "slamhip_cs_search_shard_async": (i32, [vp, fp, i32, i32, vp]),
        "slamhip_cs_search_shard_enqueue": (i32, [vp, fp, i32, i32, C.POINTER(C.c_void_p)]),
        "slamhip_cs_key_read": (i32, [vp, vp, u64p]),
        "slamhip_cs_pose_from_key": (i32, [vp, fp, u64, fp, ip, ip]),
        "slamhip_cs_update_holemap": (i32, [vp, fp, f, i32]),
        "slamhip_cs_update_holemap_pxcs": (i32, [vp, fp, f, i32]),
        "slamhip_cs_update_obstaclemap": (i32, [vp, fp, i32]),
        "slamhip_cs_update_obstaclemap_pxcs": (i32, [vp, fp, i32]),
        "slamhip_cs_last_holemap_pixels": (i32, [vp, P(i64)]),
        "slamhip_cs_maps_checksum": (i32, [vp, P(u64)]),
        "slamhip_cs_search_and_update": (i32, [vp, fp, f, i32, i32, fp, ip, ip]),
        "slamhip_cs_scan_search_and_update": (i32, [vp, fp, i32, fp, f, i32, i32, fp, ip, ip]),
        "slamhip_cs_search_and_update_pxcs": (i32, [vp, fp, fp, fp, i32, f, i32, i32, ip, ip]),
        "slamhip_cs_update_maps_pxcs": (i32, [vp, fp, fp, f, i32, i32]),
        "slamhip_cs_search_report": (i32, [vp, fp, i32, fp, srp]),
        "slamhip_cs_search_distances": (i32, [vp, ip, i32]),
        "slamhip_cs_search_and_update_report": (i32, [vp, fp, i32, f, i32, i32, fp, srp]),
        "slamhip_cs_scan_search_and_update_report": (i32, [vp, fp, i32, fp, i32, f, i32, i32, fp, srp]),
        "slamhip_cs_selfcheck_failures": (i32, [vp, P(C.c_uint32)]),
        "slamhip_cs_selfcheck_counts": (i32, [vp, P(C.c_uint32)]),
        "slamhip_cs_prelaunch_stats": (i32, [vp, P(C.c_uint64)]),
        "slamhip_cs_plan_stats": (i32, [vp, P(C.c_uint64)]),
        "slamhip_cs_prepared_lists": (i32, [vp, P(C.c_uint64), P(C.c_uint64)]),
        "slamhip_csproc_create": (i32, [vp, f, i32, i32, fp, f, f, i32, i32, vpp]),
        "slamhip_csproc_destroy": (i32, [vp]),
        "slamhip_csproc_reset": (i32, [vp]),
        "slamhip_csproc_update": (i32, [vp, fp, ip, i32, fp]),
        "slamhip_csproc_get_pose": (i32, [vp, fp]),
        "slamhip_csproc_set_params": (i32, [vp, i32, f, i32, i32, i32]),
        "slamhip_csproc_set_seed": (i32, [vp, u64]),
        "slamhip_csproc_set_lattice": (i32, [vp, i32]),
        "slamhip_csproc_set_offsets": (i32, [vp, fp, i32]),
        "slamhip_csproc_set_search_report": (i32, [vp, i32, i32]),
        "slamhip_csproc_get_report": (i32, [vp, srp, ip]),
        "slamhip_csproc_cs": (i32, [vp, vpp]),
        "slamhip_scan_segments_to_cloud": (i32, [fp, ip, i32, fp, fp]),
        "slamhip_hs_create": (i32, [vp, f, i32, i32, i32, vpp]),
        "slamhip_hs_destroy": (i32, [vp]),
        "slamhip_hs_reset": (i32, [vp]),
        "slamhip_hs_level_info": (i32, [vp, i32, ip, ip, fp]),
        "slamhip_hs_set_factors": (i32, [vp, f, f]),
        "slamhip_hs_set_iterations": (i32, [vp, ip]),
        "slamhip_hs_cells_upload": (i32, [vp, i32, vp, sz]),
        "slamhip_hs_cells_download": (i32, [vp, i32, vp, sz]),
        "slamhip_hs_bitmap_download": (i32, [vp, i32, u8p, sz]),
        "slamhip_hs_map_extends": (i32, [vp, i32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
        "slamhip_hs_checksum": (i32, [vp, i32, P(u64)]),
        "slamhip_hs_probability": (i32, [vp, i32, ip, i32, fp]),
        "slamhip_hs_set_scan": (i32, [vp, fp, i32, fp]),
        "slamhip_hs_match": (i32, [vp, fp, fp]),
        "slamhip_hs_match_level": (i32, [vp, i32, fp, i32, fp]),
        "slamhip_hs_match_batch": (i32, [vp, fp, i32, fp]),
        "slamhip_hs_hessian": (i32, [vp, i32, fp, fp, fp]),
        "slamhip_hs_match_report": (i32, [vp, fp, fp, rp]),
        "slamhip_hs_match_level_report": (i32, [vp, i32, fp, i32, fp, rp]),
        "slamhip_hs_match_batch_report": (i32, [vp, fp, i32, fp, rp]),
        "slamhip_hs_match_best": (i32, [vp, fp, i32, fp, ip, rp]),
        "slamhip_hs_lattice_search": (i32, [vp, lsp, u64p, ip]),
        "slamhip_hs_lattice_node_pose": (i32, [vp, lsp, i32, i32, fp]),
        "slamhip_hs_relocalise": (i32, [vp, lsp, i32, fp, rp, rip]),
        "slamhip_hs_world_lattice_search": (i32, [vp, lsp, u64p, ip]),
        "slamhip_hs_relocalise_world": (i32, [vp, lsp, i32, fp, rp, wrip]),
        "slamhip_hs_lattice_search_bnb": (i32, [vp, bsp, u64p, bip]),
        "slamhip_hs_relocalise_bnb": (i32, [vp, bsp, i32, fp, rp, vp, bip]),
        "slamhip_hs_trace": (i32, [vp, i32, fp, i32, i32, vp, vp]),
        "slamhip_hs_distance_field": (i32, [vp, i32, i32, i32, i32, i32, i32, i32, i32, vp]),
        "slamhip_hs_distance_score": (i32, [vp, i32, i32, i32, i32, fp, i32, vp, vp]),
        "slamhip_hs_nearest_field": (i32, [vp, i32, i32, i32, i32, i32, i32, i32, i32, vp]),
        "slamhip_hs_nearest_pairs": (i32, [vp, i32, i32, i32, i32, fp, i32, vp, vp]),
        "slamhip_hs_hough": (i32, [vp, i32, i32, i32, i32, i32, i32, vp, vp, vp]),
        "slamhip_hs_hough_rotation": (i32, [vp, vp]),
        "slamhip_hs_hough_shifts": (i32, [vp, vp, i32, vp, vp]),
        "slamhip_hs_hough_clear": (i32, [vp]),
        "slamhip_hs_sig_configure": (i32, [vp, vp]),
        "slamhip_hs_sig_add": (i32, [vp, fp, ip, vp, vp]),
        "slamhip_hs_sig_add_scans": (i32, [vp, fp, vp, i32, fp, ip]),
        "slamhip_hs_sig_query": (i32, [vp, i32, i32, i32, vp, ip, vp, vp]),
        "slamhip_hs_sig_self": (i32, [vp, i32, i32, i32, vp]),
        "slamhip_hs_sig_count": (i32, [vp, ip]),
        "slamhip_hs_sig_download": (i32, [vp, i32, i32, vp, vp]),
        "slamhip_hs_sig_upload": (i32, [vp, i32, vp, vp]),
        "slamhip_hs_sig_clear": (i32, [vp]),
        "slamhip_hs_sig_set_poses": (i32, [vp, i32, i32, fp]),
        "slamhip_hs_pg_set": (i32, [vp, vp, vp, i32, vp, vp, vp, i32]),
        "slamhip_hs_pg_relax": (i32, [vp, vp, vp, vp]),
        "slamhip_hs_pg_relax_tri": (i32, [vp, vp, vp, vp]),
        "slamhip_hs_pg_tri_apply": (i32, [vp, C.c_double, vp, vp]),
        "slamhip_hs_pg_relax_lm": (i32, [vp, vp, vp, vp, vp, vp, vp]),
        "slamhip_hs_pg_marginals": (i32, [vp, vp, vp, i32, vp, vp, vp, vp]),
        "slamhip_hs_pg_get": (i32, [vp, vp, i32]),
        "slamhip_hs_pg_residuals": (i32, [vp, vp, vp]),
        "slamhip_hs_pg_clear": (i32, [vp]),
        "slamhip_hs_scans_add": (i32, [vp, vp, i32, vp, ip]),
        "slamhip_hs_scans_count": (i32, [vp, ip]),
        "slamhip_hs_scans_info": (i32, [vp, i32, ip, vp]),
        "slamhip_hs_scans_download": (i32, [vp, i32, vp, i32]),
        "slamhip_hs_scans_clear": (i32, [vp]),
        "slamhip_hs_render": (i32, [vp, i32, i32, vp, i32]),
        "slamhip_hs_render_world": (i32, [vp, i32, i32, vp, i32]),
        "slamhip_hs_scans_match": (i32, [vp, vp, vp, i32, vp]),
        "slamhip_hs_scans_edges": (i32, [vp, vp, vp, i32, vp, vp, vp]),
        "slamhip_hs_loops_consistent": (i32, [vp, vp, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp]),
        "slamhip_hs_loops_clear": (i32, [vp]),
        "slamhip_hs_frontiers": (i32, [vp, i32, i32, i32, i32, vp, vp, i32, i32, i32, i32, vp]),
        "slamhip_hs_nav_field": (i32, [vp, vp, vp, i32, vp, i32, vp, i32, i32, vp, vp, i32, i32, i32, i32, vp, vp, vp]),
        "slamhip_hs_rollouts": (i32, [vp, vp, vp, i32, vp, C.c_float, vp, i32, vp, i32, i32, i32, vp, vp]),
        "slamhip_hs_mcl_set": (i32, [vp, vp, i32]),
        "slamhip_hs_mcl_step": (i32, [vp, vp, vp]),
        "slamhip_hs_mcl_get": (i32, [vp, vp, vp, vp, i32]),
        "slamhip_hs_merge_set_source": (i32, [vp, i32, i32, i32, i32, i32, vp]),
        "slamhip_hs_merge_score": (i32, [vp, fp, i32, vp]),
        "slamhip_hs_merge_apply": (i32, [vp, fp, i32, C.c_float, vp]),
        "slamhip_hs_merge_clear_source": (i32, [vp]),
        "slamhip_hs_view_set_covered": (i32, [vp, i32, vp]),
        "slamhip_hs_view_get_covered": (i32, [vp, i32, vp]),
        "slamhip_hs_view_clear": (i32, [vp]),
        "slamhip_hs_view_gain": (i32, [vp, i32, i32, fp, i32, i32, vp]),
        "slamhip_hs_view_select": (i32, [vp, i32, i32, i32, i32, fp, i32, i32, ip, ip, ip]),
        "slamhip_hs_set_match_threads": (i32, [vp, i32]),
        "slamhip_hs_set_reference_cache": (i32, [vp, i32]),
        "slamhip_hs_update_by_scan": (i32, [vp, fp]),
        "slamhip_hs_shift": (i32, [vp, i32, i32]),
        "slamhip_hs_origin": (i32, [vp, P(i64), P(i64)]),
        "slamhip_hs_set_backing": (i32, [vp, i32, u64]),
        "slamhip_hs_backing_stats": (i32, [vp, P(BackingStats)]),
        "slamhip_hs_world_cells_download": (i32, [vp, i32, i64, i64, i32, i32, vp]),
        "slamhip_hs_world_cells_upload": (i32, [vp, i32, i64, i64, i32, i32, vp, P(i64)]),
        "slamhip_hs_world_extends": (i32, [vp, i32, P(i64), ip]),
        "slamhip_hsproc_create": (i32, [vp, f, i32, i32, fp, i32, vpp]),
        "slamhip_hsproc_destroy": (i32, [vp]),
        "slamhip_hsproc_reset": (i32, [vp]),
        "slamhip_hsproc_update": (i32, [vp, fp, i32, fp, fp, i32, ip]),
        "slamhip_hsproc_get": (i32, [vp, fp, fp, fp, fp]),
        "slamhip_hsproc_set_match_report": (i32, [vp, i32]),
        "slamhip_hsproc_get_report": (i32, [vp, rp, ip]),
        "slamhip_hsproc_set_thresholds": (i32, [vp, f, f]),
        "slamhip_hsproc_hs": (i32, [vp, vpp]),
        "slamhip_hsproc_set_scroll": (i32, [vp, i32]),
        "slamhip_hsproc_get_origin": (i32, [vp, P(i64), P(i64)]),
        "slamhip_hsproc_shift": (i32, [vp, i32, i32]),
        "slamhip_hsproc_relocalise": (i32, [vp, fp, i32, fp, lsp, i32, i32, fp, rp, rip]),
        "slamhip_hsproc_relocalise_world": (i32, [vp, fp, i32, fp, lsp, i32, i32, fp, rp, wrip]),
        "slamhip_hsproc_relocalise_bnb": (i32, [vp, fp, i32, fp, bsp, i32, i32, fp, rp, vp, bip]),
        "slamhip_hsproc_trace": (i32, [vp, fp, i32, fp, fp, i32, i32, i32, vp, vp]),
        "slamhip_hsproc_distance_score": (i32, [vp, fp, i32, fp, fp, i32, i32, i32, i32, i32, vp, vp]),
        "slamhip_hsproc_nearest_pairs": (i32, [vp, fp, i32, fp, fp, i32, i32, i32, i32, i32, vp, vp]),
        "slamhip_hsproc_hough": (i32, [vp, i32, i32, i32, i32, i32, i32, vp, vp, vp]),
        "slamhip_hsproc_hough_rotation": (i32, [vp, vp]),
        "slamhip_hsproc_hough_shifts": (i32, [vp, vp, i32, vp, vp]),
        "slamhip_hsproc_sig_add": (i32, [vp, fp, i32, fp, fp, ip, vp, vp]),
        "slamhip_hsproc_sig_query": (i32, [vp, fp, i32, fp, i32, i32, i32, vp, ip, vp, vp]),
        "slamhip_hsproc_sig_self": (i32, [vp, i32, i32, i32, vp]),
        "slamhip_hsproc_scans_add": (i32, [vp, ip]),
        "slamhip_hsproc_render": (i32, [vp, i32, i32, vp, i32]),
        "slamhip_hsproc_render_world": (i32, [vp, i32, i32, vp, i32]),
        "slamhip_hsproc_scans_match": (i32, [vp, vp, vp, i32, vp]),
        "slamhip_hsproc_frontiers": (i32, [vp, i32, i32, i32, i32, vp, vp, i32, i32, i32, i32, vp]),
        "slamhip_hsproc_nav_field": (i32, [vp, vp, vp, i32, vp, i32, vp, i32, i32, vp, vp, i32, i32, i32, i32, vp, vp, vp]),
        "slamhip_hsproc_rollouts": (i32, [vp, vp, vp, i32, vp, C.c_float, vp, i32, vp, i32, i32, i32, vp, vp]),
        "slamhip_hsproc_mcl_step": (i32, [vp, fp, i32, fp, vp, vp]),
        "slamhip_hsproc_merge_set_source": (i32, [vp, i32, i32, i32, i32, i32, vp]),
        "slamhip_hsproc_merge_score": (i32, [vp, fp, i32, vp]),
        "slamhip_hsproc_merge_apply": (i32, [vp, fp, i32, C.c_float, vp]),
        "slamhip_hsproc_view_gain": (i32, [vp, fp, i32, fp, fp, i32, i32, i32, i32, vp]),
        "slamhip_hsproc_view_select": (i32, [vp, fp, i32, fp, fp, i32, i32, i32, i32, i32, i32, ip, ip, ip]),
        "slamhip_group_create": (i32, [ip, i32, f, i32, i32, vpp]),
        "slamhip_group_destroy": (i32, [vp]),
        "slamhip_group_size": (i32, [vp, ip]),
        "slamhip_group_cs": (i32, [vp, i32, vpp]),
        "slamhip_group_reset": (i32, [vp, i32]),
        "slamhip_group_holemap_upload": (i32, [vp, u16p, sz]),
        "slamhip_group_set_scan": (i32, [vp, fp, i32]),
        "slamhip_group_set_offsets": (i32, [vp, fp, i32]),
        "slamhip_group_generate_offsets": (i32, [vp, i32, f, f, u64, u64]),
        "slamhip_group_search": (i32, [vp, fp, fp, ip, ip]),
        "slamhip_group_update_maps": (i32, [vp, fp, f, i32, i32]),
        "slamhip_group_search_and_update": (i32, [vp, fp, f, i32, i32, fp, ip, ip]),
        "slamhip_group_replicas_equal": (i32, [vp, P(i32)]),
        "slamhip_comm_probe": (i32, []),
        "slamhip_comm_unique_id": (i32, [u8p]),
        "slamhip_comm_create": (i32, [vp, u8p, i32, i32, vpp]),
        "slamhip_comm_destroy": (i32, [vp]),
        "slamhip_comm_info": (i32, [vp, ip, ip]),
        "slamhip_cs_search_allreduce_async": (i32, [vp, vp, fp, i32, i32, C.POINTER(C.c_void_p)]),
        "slamhip_comm_wait": (i32, [vp, C.POINTER(C.c_uint64)]),
        "slamhip_comm_set_batch": (i32, [vp, i32]),
        "slamhip_cs_search_allreduce": (i32, [vp, vp, fp, i32, i32, u64p]),
        "slamhip_cs_search_allreduce_and_update": (i32, [vp, vp, fp, i32, i32, f, i32, i32, fp, ip, ip]),
        "slamhip_comm_allreduce_probe": (i32, [vp, i32, fp]),
        "slamhip_comm_replicas_equal": (i32, [vp, vp, P(i32)]),
    }
    for name, (res, args) in sig.items():
        if os.environ.get("SLAMHIP_LIB") and not hasattr(L, name):
            continue                                               # (developer aid: an OLDER build of the library timed beside the current one)
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    L._signatures = sig


def live_blocks():
    """(blocks, bytes) that the Hector units of every hs of the process hold right now (slamhip_debug_live_blocks; no device involved)."""
    n, b = C.c_int64(), C.c_int64()
    call("slamhip_debug_live_blocks", C.byref(n), C.byref(b))
    return n.value, b.value


def backing_plan(levels, w0, h0, ox, oy, dx, dy, tile):
    """The job list of the backing store's planner for one shift (slamhip_debug_backing_plan; no device involved): a
    BACKING_JOB_DTYPE array in the order the shift uses."""
    n = C.c_int32()
    rc = lib().slamhip_debug_backing_plan(levels, w0, h0, ox, oy, dx, dy, tile, None, 0, C.byref(n))
    if rc == OK:
        return np.zeros(0, BACKING_JOB_DTYPE)
    if n.value <= 0:
        check(rc)
    jobs = np.zeros(n.value, BACKING_JOB_DTYPE)
    call("slamhip_debug_backing_plan", levels, w0, h0, ox, oy, dx, dy, tile, jobs.ctypes.data_as(C.POINTER(BackingJob)), n.value, C.byref(n))
    return jobs


def world_plan(w, h, OX, OY, x0, y0, rw, rh, tile):
    """The job list of the world upload's planner for one rectangle (slamhip_debug_world_plan; no device involved): a
    WORLD_JOB_DTYPE array in the order the upload uses."""
    n = C.c_int32()
    rc = lib().slamhip_debug_world_plan(w, h, OX, OY, x0, y0, rw, rh, tile, None, 0, C.byref(n))
    if rc == OK:
        return np.zeros(0, WORLD_JOB_DTYPE)
    if n.value <= 0:
        check(rc)
    jobs = np.zeros(n.value, WORLD_JOB_DTYPE)
    call("slamhip_debug_world_plan", w, h, OX, OY, x0, y0, rw, rh, tile, jobs.ctypes.data_as(C.POINTER(WorldJob)), n.value, C.byref(n))
    return jobs


def world_pack_plan(w, h, OX, OY, tile, tiles):
    """The plan of the world search's class map for one level (slamhip_debug_world_pack_plan; no device involved): `tiles` the
    (ty, tx) pairs of the tiles that exist, row-major.  -> ((x0, y0, rw, rh), jobs): the rectangle R in window-frame cells and a
    WORLD_JOB_DTYPE array in the order the pack launch uses.  An R of more than 2^28 cells raises SlamhipError (ERR_INVALID)."""
    t = np.ascontiguousarray(tiles, np.int64).reshape(-1, 2)
    tp = t.ctypes.data_as(C.POINTER(C.c_int64)) if t.shape[0] else None
    rect = (C.c_int64 * 4)()
    n = C.c_int32()
    rc = lib().slamhip_debug_world_pack_plan(w, h, OX, OY, tile, tp, t.shape[0], rect, None, 0, C.byref(n))
    if n.value <= 0:
        check(rc)
    jobs = np.zeros(n.value, WORLD_JOB_DTYPE)
    call("slamhip_debug_world_pack_plan", w, h, OX, OY, tile, tp, t.shape[0], rect, jobs.ctypes.data_as(C.POINTER(WorldJob)), n.value, C.byref(n))
    return tuple(int(v) for v in rect), jobs


def lattice_cells(cell_length, centre, theta, xy):
    """(gx, gy) of every point of `xy` for one heading of the pose-lattice search (slamhip_debug_lattice_cells; no device involved):
    an (n, 2) int32 array, INT32_MIN twice for a point the search ignores."""
    xy = f32(xy, (-1, 2)); c = f32(centre, (3,))
    out = np.empty((xy.shape[0], 2), np.int32)
    call("slamhip_debug_lattice_cells", C.c_float(cell_length), fptr(c), C.c_float(theta), fptr(xy), xy.shape[0], iptr(out))
    return out


def bnb_call(values, w, h, cell_length, spec, xy):
    """The branch-and-bound lattice search of the definition (slamhip_bnb_spec, rules 1 - 6) on the host (slamhip_debug_lattice_bnb; no
    device involved): `values` the w x h cell values of one level, `spec` a BNB_SPEC (bnb_spec), `xy` the scan's points.
    -> (keys (n_theta,) uint64, a BNB_INFO record).  A refused spec raises SlamhipError."""
    v = f32(values, (-1,)); xy = f32(xy, (-1, 2))
    assert v.size == int(w) * int(h)
    keys = np.zeros(max(int(spec.lattice.n_theta), 1), np.uint64)
    info = BnbInfo()
    call("slamhip_debug_lattice_bnb", fptr(v), int(w), int(h), C.c_float(cell_length), C.byref(spec), fptr(xy), xy.shape[0],
         keys.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(info))
    return keys, bnb_info(info)


def trace_lines(stm, pose, origin, xy):
    """{bx, by, ex, ey, da} of every beam of `xy` for one pose of the beam trace (slamhip_debug_trace_lines; no device involved): an
    (n, 5) int32 array; an ignored beam is (0, 0, 0, 0, -1)."""
    xy = f32(xy, (-1, 2)); p = f32(pose, (3,)); o = f32(origin, (2,))
    out = np.empty((xy.shape[0], 5), np.int32)
    call("slamhip_debug_trace_lines", C.c_float(stm), fptr(p), fptr(o), fptr(xy), xy.shape[0], iptr(out))
    return out


def trace_cells(bx, by, ex, ey):
    """The cells the beam trace walks from cell (bx, by) to cell (ex, ey), in order (slamhip_debug_trace_cells; no device involved):
    a (da + 1, 2) int32 array.  A line no walked beam has raises SlamhipError (ERR_INVALID)."""
    cap = min(max(abs(int(ex) - int(bx)), abs(int(ey) - int(by))), TRACE_MAX_DA) + 1
    out = np.empty((max(cap, 1), 2), np.int32)
    n = C.c_int32()
    call("slamhip_debug_trace_cells", int(bx), int(by), int(ex), int(ey), iptr(out), out.shape[0], C.byref(n))
    return out[:n.value]


def debug_distance_field(cls, site_mask, radius, rect):
    """The distance field of the definition (slamhip_hs_distance_field) over the (h, w) uint8 array `cls` of class bits, class 0
    outside it, for rect = (x, y, w, h) in the array's cells (slamhip_debug_distance_field; no device involved): an (h, w) uint16
    array of squared cell distances capped at radius^2."""
    c = np.ascontiguousarray(cls, np.uint8)
    x, y, w, h = (int(v) for v in rect)
    out = np.empty((max(h, 0), max(w, 0)), np.uint16)
    call("slamhip_debug_distance_field", c.ctypes.data_as(C.c_void_p), c.shape[1], c.shape[0], int(site_mask), int(radius), x, y, w, h,
         out.ctypes.data_as(C.c_void_p))
    return out


def debug_nearest_field(cls, site_mask, radius, rect):
    """The nearest-site field of the definition (slamhip_hs_nearest_field) over the (h, w) uint8 array `cls` of class bits, class 0
    outside it, for rect = (x, y, w, h) in the array's cells (slamhip_debug_nearest_field; no device involved): an (h, w, 2) int16
    array of offsets (dx, dy), NEAREST_NONE twice where no site lies within the radius."""
    c = np.ascontiguousarray(cls, np.uint8)
    x, y, w, h = (int(v) for v in rect)
    out = np.empty((max(h, 0), max(w, 0), 2), np.int16)
    call("slamhip_debug_nearest_field", c.ctypes.data_as(C.c_void_p), c.shape[1], c.shape[0], int(site_mask), int(radius), x, y, w, h,
         out.ctypes.data_as(C.c_void_p))
    return out


def frontiers_call(name, head, min_cells, max_clusters, labels_shape, rect=None):
    """One of the three frontier entry points: `head` its leading arguments, rect = (lx, ly, lw, lh) for the two device calls.
    -> (summary, clusters[, labels]): a FRONTIER_SUMMARY record, the n_returned FRONTIER_CLUSTER records, the int32 label array."""
    summary = np.zeros(1, FRONTIER_SUMMARY)
    rec = np.zeros(max(int(max_clusters), 0), FRONTIER_CLUSTER)
    labels = np.empty(labels_shape, np.int32) if labels_shape is not None else None
    tail = [labels.ctypes.data_as(C.c_void_p) if labels is not None else None]
    if rect is not None:
        tail = [int(v) for v in rect] + tail
    call(name, *head, int(min_cells), int(max_clusters), summary.ctypes.data_as(C.c_void_p),
         rec.ctypes.data_as(C.c_void_p) if rec.shape[0] else None, *tail)
    out = (summary[0], rec[:int(summary[0]["n_returned"])].copy())
    return out + (labels,) if labels is not None else out


def debug_frontiers(cls, min_cells=1, max_clusters=256, labels=True):
    """The frontier clusters of the definition (slamhip_hs_frontiers) over the (h, w) uint8 array `cls` of class bits, M = (0, 0, w, h)
    (slamhip_debug_frontiers; no device involved) -> (summary, clusters[, labels]), labels the whole (h, w) int32 array."""
    c = np.ascontiguousarray(cls, np.uint8)
    return frontiers_call("slamhip_debug_frontiers", [c.ctypes.data_as(C.c_void_p), c.shape[1], c.shape[0]], min_cells, max_clusters,
                          c.shape if labels else None)


def nav_call(name, head, sources, goals=None, n_paths=0, max_path_cells=1, rect=None, want_cost=True, want_dir=True):
    """One of the three cost-to-go entry points: `head` its leading arguments (the hs or processor and a NAV_SPEC record's pointer, or
    the hook's class array and scalars).  sources: (S, 2) cells; goals: (G, 4) rectangles {x_min, y_min, x_max, y_max}; rect = (rx, ry,
    rw, rh): the rectangle whose costs (want_cost) and dirs (want_dir) are returned.  -> a dict: summary (a NAV_SUMMARY record), goals
    (G NAV_GOAL_RESULT records), paths (a list of n_paths (n_written, 2) int32 arrays), path_cells (the n_paths true lengths), and with
    rect, cost ((rh, rw) uint32) and dir ((rh, rw) uint8)."""
    vp = C.c_void_p
    src = np.ascontiguousarray(sources, np.int32).reshape(-1, 2)
    gl = np.ascontiguousarray(goals if goals is not None else np.zeros((0, 4)), np.int32).reshape(-1, 4)
    res = np.zeros(gl.shape[0], NAV_GOAL_RESULT)
    heads = np.zeros(max(int(n_paths), 0), NAV_PATH)
    cells = np.zeros((max(int(n_paths), 0), max(int(max_path_cells), 0), 2), np.int32)
    summary = np.zeros(1, NAV_SUMMARY)
    rx, ry, rw, rh = (int(v) for v in rect) if rect is not None else (0, 0, 0, 0)
    cost = np.empty((max(rh, 0), max(rw, 0)), np.uint32) if rect is not None and want_cost else None
    dirs = np.empty((max(rh, 0), max(rw, 0)), np.uint8) if rect is not None and want_dir else None
    ptr = lambda a: a.ctypes.data_as(vp) if a is not None and a.size else None
    call(name, *head, ptr(src), src.shape[0], ptr(gl), gl.shape[0], ptr(res), int(n_paths), int(max_path_cells), ptr(heads), ptr(cells),
         rx, ry, rw, rh, cost.ctypes.data_as(vp) if cost is not None else None, dirs.ctypes.data_as(vp) if dirs is not None else None,
         summary.ctypes.data_as(vp))
    out = {"summary": summary[0], "goals": res, "path_cells": heads["n_cells"].copy(),
           "paths": [cells[i, :int(heads[i]["n_written"])].copy() for i in range(heads.shape[0])]}
    if cost is not None:
        out["cost"] = cost
    if dirs is not None:
        out["dir"] = dirs
    return out


def nav_spec(level, world, site_mask, clearance, max_cost):
    """A NAV_SPEC record (one-element array) from Python values."""
    s = np.zeros(1, NAV_SPEC)
    s[0] = (int(level), 1 if world else 0, int(site_mask), int(clearance), int(max_cost))
    return s


def debug_nav_field(cls, sources, site_mask=2, clearance=0, max_cost=0, goals=None, n_paths=0, max_path_cells=1, rect="all", **kw):
    """The cost-to-go field of the definition (slamhip_hs_nav_field) over the (h, w) uint8 array `cls` of class bits, M = (0, 0, w, h)
    (slamhip_debug_nav_field; no device involved; the costs by a sequential Dijkstra) -> nav_call's dict; rect "all": the array's own
    rectangle."""
    c = np.ascontiguousarray(cls, np.uint8)
    if isinstance(rect, str):
        rect = (0, 0, c.shape[1], c.shape[0])
    return nav_call("slamhip_debug_nav_field", [c.ctypes.data_as(C.c_void_p), c.shape[1], c.shape[0], int(site_mask), int(clearance), int(max_cost)],
                    sources, goals, n_paths, max_path_cells, rect, **kw)


def rollouts_call(name, head, sources, start_pose, dt, body, cmds, hold=1, stm=None):
    """One of the three rollout entry points: `head` its leading arguments (the hs or processor and a NAV_SPEC record's pointer, or
    the hook's class array and scalars; stm: the hook's ScaleToMap, which it takes behind the sources).  sources: (S, 2) cells; start_pose: 3 floats or None (the processor's MatchPose); body: (P, 2) metres in the
    robot's frame or None; cmds: (B, n_cmd, 2) pairs (v, w).  -> (results, summary): B ROLLOUT_RESULT records and a ROLLOUT_SUMMARY
    record."""
    vp = C.c_void_p
    mid = [C.c_float(stm)] if stm is not None else []
    src = np.ascontiguousarray(sources, np.int32).reshape(-1, 2)
    pose = f32(start_pose, (3,)) if start_pose is not None else None
    bd = f32(body if body is not None else np.zeros((0, 2)), (-1, 2))
    cm = f32(cmds)
    if cm.ndim != 3 or cm.shape[2] != 2:
        raise ValueError("rollouts: cmds must be (B, n_cmd, 2)")
    res = np.zeros(cm.shape[0], ROLLOUT_RESULT)
    summary = np.zeros(1, ROLLOUT_SUMMARY)
    ptr = lambda a: a.ctypes.data_as(vp) if a is not None and a.size else None
    call(name, *head, ptr(src), src.shape[0], *mid, ptr(pose), C.c_float(dt), ptr(bd), bd.shape[0], ptr(cm), cm.shape[0], cm.shape[1], int(hold),
         ptr(res), summary.ctypes.data_as(vp))
    return res, summary[0]


def debug_rollouts(cls, sources, stm, start_pose, dt, body, cmds, hold=1, site_mask=2, clearance=0, max_cost=0):
    """The command rollouts of the definition (slamhip_hs_rollouts) over the (h, w) uint8 array `cls` of class bits, M = (0, 0, w, h),
    stm = 1 / cell length (slamhip_debug_rollouts; no device involved) -> rollouts_call's pair."""
    c = np.ascontiguousarray(cls, np.uint8)
    return rollouts_call("slamhip_debug_rollouts", [c.ctypes.data_as(C.c_void_p), c.shape[1], c.shape[0], int(site_mask), int(clearance), int(max_cost)],
                         sources, start_pose, dt, body, cmds, hold, stm)


def rollout_key(key):
    """(cost, b) of a key_end / key_min, or None for ROLLOUT_NO_KEY."""
    key = int(key)
    return None if key == ROLLOUT_NO_KEY else (key >> 32, key & 0xFFFFFFFF)


def mcl_spec(level, radius, delta, sigma, beta, n_eff_min, seed=0, stream=0, site_mask=2, world=False, frame_offset=(0.0, 0.0)):
    """A MCL_SPEC record (one-element array) from Python values (the floats rounded to binary32)."""
    s = np.zeros(1, MCL_SPEC)
    s["level"] = int(level); s["world"] = 1 if world else 0; s["site_mask"] = int(site_mask); s["radius"] = int(radius)
    s["delta"][0] = f32(delta, (3,)); s["sigma"][0] = f32(sigma, (3,)); s["frame_offset"][0] = f32(frame_offset, (2,))
    s["beta"] = int(beta); s["n_eff_min"] = int(n_eff_min)
    s["seed"] = int(seed) & 0xFFFFFFFFFFFFFFFF; s["stream"] = int(stream) & 0xFFFFFFFFFFFFFFFF
    return s


def mcl_beta(sigma_cells, temper=1.0):
    """beta of a MCL_SPEC for a Gaussian end-point model: the weight exp(-cost / (2 sigma_cells^2 temper)) halves every
    2 sigma_cells^2 temper ln 2 units of cost, so beta = round(65536 * 64 * log2(e) / (2 sigma_cells^2 temper)), at least 1."""
    return max(1, min(0xFFFFFFFF, int(round(65536.0 * 64.0 * math.log2(math.e) / (2.0 * float(sigma_cells) ** 2 * float(temper))))))


def mcl_mean(summary, frame_offset=(0.0, 0.0)):
    """(pose, n_eff) of a MCL_SUMMARY: the weighted-mean pose of the placed particles -- (sum_hx / A' / 1024, sum_hy / A' / 1024,
    atan2(sum_hs, sum_hc)) in float64, A' = A when nothing is unplaced -- plus frame_offset on x and y, and A^2 / Q."""
    A, Q = int(summary["A"]), int(summary["Q"])
    pose = np.array([int(summary["sum_hx"]) / A / 1024.0 + float(frame_offset[0]), int(summary["sum_hy"]) / A / 1024.0 + float(frame_offset[1]),
                     math.atan2(int(summary["sum_hs"]), int(summary["sum_hc"]))])
    return pose, A * A / Q


def debug_mcl_step(cls, stm, points, particles, spec, acc=None):
    """One localisation step of the definition (slamhip_hs_mcl_step) over the (h, w) uint8 array `cls` of class bits, M = (0, 0, w, h),
    stm = 1 / cell length (slamhip_debug_mcl_step; no device involved).  points: (n, 2); particles: (N, 3); spec: mcl_spec's record;
    acc: (N,) uint64 or None for zeros.  -> (particles, acc, ancestors, summary)."""
    vp = C.c_void_p
    c = np.ascontiguousarray(cls, np.uint8)
    pts = f32(points, (-1, 2)); part = f32(particles, (-1, 3))
    N = part.shape[0]
    a_in = np.ascontiguousarray(acc, np.uint64).reshape(N) if acc is not None else None
    out_p = np.zeros((N, 3), np.float32); out_a = np.zeros(N, np.uint64); out_anc = np.zeros(N, np.int32); summary = np.zeros(1, MCL_SUMMARY)
    call("slamhip_debug_mcl_step", c.ctypes.data_as(vp), c.shape[1], c.shape[0], C.c_float(stm), pts.ctypes.data_as(vp), pts.shape[0],
         part.ctypes.data_as(vp), a_in.ctypes.data_as(vp) if a_in is not None else None, N, spec.ctypes.data_as(vp), out_p.ctypes.data_as(vp),
         out_a.ctypes.data_as(vp), out_anc.ctypes.data_as(vp), summary.ctypes.data_as(vp))
    return out_p, out_a, out_anc, summary[0]


def debug_mcl_table():
    """The weight table T of slamhip_hs_mcl_step's step 5 (slamhip_debug_mcl_table): 64 uint32."""
    t = np.zeros(64, np.uint32)
    call("slamhip_debug_mcl_table", t.ctypes.data_as(C.c_void_p))
    return t


def check(rc):
    if rc != OK:
        raise SlamhipError(rc, lib().slamhip_last_error().decode(errors="replace"))


def call(name, *args):
    check(getattr(lib(), name)(*args))


def fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def iptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def rptr(a):
    """A REPORT_DTYPE array as the slamhip_match_report pointer of the C-ABI."""
    return a.ctypes.data_as(C.POINTER(MatchReport))


def srptr(a):
    """A SEARCH_REPORT_DTYPE array as the slamhip_search_report pointer of the C-ABI."""
    return a.ctypes.data_as(C.POINTER(SearchReport))


def f32(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a if shape is None else a.reshape(shape)


def debug_merge(dst, src, ax, ay, pose, stm, rule, value_limit):
    """The merge of the definition (slamhip_hs_merge_apply, steps 1 - 4) on the host (slamhip_debug_merge; no device involved): dst an
    (dh, dw) and src an (sh, sw) array of CELL_DTYPE, src's first cell source-frame cell (ax, ay); stm = 1 / cell length.
    -> (merged cells (dh, dw), a MERGE_REPORT record)."""
    vp = C.c_void_p
    d = np.ascontiguousarray(dst, CELL_DTYPE); s = np.ascontiguousarray(src, CELL_DTYPE)
    assert d.ndim == 2 and s.ndim == 2
    out = np.empty_like(d); rep = np.zeros(1, MERGE_REPORT)
    call("slamhip_debug_merge", d.ctypes.data_as(vp), d.shape[1], d.shape[0], s.ctypes.data_as(vp), int(ax), int(ay), s.shape[1], s.shape[0],
         fptr(f32(pose, (3,))), C.c_float(stm), int(rule), C.c_float(value_limit), out.ctypes.data_as(vp), rep.ctypes.data_as(vp))
    return out, rep[0]


def hough_bins(w, h, q):
    """D and N of step 2 of slamhip_hs_hough for a w x h map."""
    D = int(w) + int(h)
    return D, ((2 * D) >> int(q)) + 1


def debug_hough_table(T):
    """Step 1 of slamhip_hs_hough (slamhip_debug_hough_table) -> (C, S), two (T,) int32 arrays."""
    cs = np.zeros(2 * int(T), np.int32)
    call("slamhip_debug_hough_table", int(T), cs.ctypes.data_as(C.c_void_p))
    return cs[:int(T)].copy(), cs[int(T):].copy()


def debug_hough(cls, site_mask, T, q):
    """Steps 1 - 3 of slamhip_hs_hough over the (h, w) uint8 array `cls` of class bits (slamhip_debug_hough; no device involved)
    -> (H (T, N) uint32, HS (T,) uint64)."""
    c = np.ascontiguousarray(cls, np.uint8)
    _, N = hough_bins(c.shape[1], c.shape[0], q)
    H = np.zeros((int(T), N), np.uint32); HS = np.zeros(int(T), np.uint64)
    call("slamhip_debug_hough", c.ctypes.data_as(C.c_void_p), c.shape[1], c.shape[0], int(site_mask), int(T), int(q), H.ctypes.data_as(C.c_void_p),
         HS.ctypes.data_as(C.c_void_p))
    return H, HS


def debug_hough_rotation(spectrum_d, spectrum_s):
    """Step 4 of slamhip_hs_hough over two spectra (slamhip_debug_hough_rotation) -> CC (T,) uint64."""
    a = np.ascontiguousarray(spectrum_d, np.uint64); b = np.ascontiguousarray(spectrum_s, np.uint64)
    assert a.shape == b.shape and a.ndim == 1
    cc = np.zeros(a.shape[0], np.uint64)
    call("slamhip_debug_hough_rotation", a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), a.shape[0], cc.ctypes.data_as(C.c_void_p))
    return cc


def debug_hough_xcorr(A, B, flip):
    """Step 5 of slamhip_hs_hough over a destination row A and a source ROW B, flipped inside when `flip` (slamhip_debug_hough_xcorr)
    -> (XC (Nd + Ns - 1,) uint64, a HOUGH_SHIFT record)."""
    a = np.ascontiguousarray(A, np.uint32); b = np.ascontiguousarray(B, np.uint32)
    xc = np.zeros(a.shape[0] + b.shape[0] - 1, np.uint64); rec = np.zeros(1, HOUGH_SHIFT)
    call("slamhip_debug_hough_xcorr", a.ctypes.data_as(C.c_void_p), a.shape[0], b.ctypes.data_as(C.c_void_p), b.shape[0], int(bool(flip)),
         xc.ctypes.data_as(C.c_void_p), rec.ctypes.data_as(C.c_void_p))
    return xc, rec[0]


def hough_call(name, handle, level, slot, world, site_mask, T, q, want_H):
    """slamhip_hs_hough / slamhip_hsproc_hough -> (info dict, HS (T,) uint64, H (T, N) uint32 or None).  N is known only from the
    call's own info, so H is asked for in a second call's worth of room: the buffer is sized by the largest N the limits allow for T."""
    info = np.zeros(7, np.int32); HS = np.zeros(int(T), np.uint64)
    H = np.zeros(HOUGH_MAX_BINS, np.uint32) if want_H else None
    call(name, handle, int(level), int(slot), int(bool(world)) if world in (True, False) else int(world), int(site_mask), int(T), int(q),
         info.ctypes.data_as(C.c_void_p), HS.ctypes.data_as(C.c_void_p), H.ctypes.data_as(C.c_void_p) if want_H else None)
    d = dict(zip(("w", "h", "x0", "y0", "D", "N", "n_sites"), (int(v) for v in info)))
    if want_H:
        H = H[:int(T) * d["N"]].reshape(int(T), d["N"]).copy()
    return d, HS, H


def hough_shifts_call(name, handle, pairs, n_xc):
    """slamhip_hs_hough_shifts / slamhip_hsproc_hough_shifts: pairs (P, 2) of (m, k); n_xc: None, or N_d + N_s - 1 to get the XC arrays
    -> ((P,) HOUGH_SHIFT records, XC (P, n_xc) uint64 or None)."""
    p = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    rec = np.zeros(p.shape[0], HOUGH_SHIFT)
    xc = np.zeros((p.shape[0], int(n_xc)), np.uint64) if n_xc else None
    call(name, handle, p.ctypes.data_as(C.c_void_p), p.shape[0], rec.ctypes.data_as(C.c_void_p), xc.ctypes.data_as(C.c_void_p) if n_xc else None)
    return rec, xc


def hough_peaks(cc, n_rot):
    """The rotation hypotheses of AlignMaps from CC: the m with CC[m] > CC[m - 1] and CC[m] >= CC[m + 1], circularly, ranked by CC
    descending then m ascending; the best n_rot, or [0] if there is none."""
    c = [int(v) for v in cc]
    T = len(c)
    peaks = [m for m in range(T) if c[m] > c[m - 1] and c[m] >= c[(m + 1) % T]]
    peaks.sort(key=lambda m: (-c[m], m))
    return peaks[:int(n_rot)] or [0]


def hough_pose(m, T, q, recs, ks, info_d, info_s, stm):
    """The pose (tx, ty, theta) of the source frame in the destination's from the two shift records `recs` of pairs (m, ks[0]) and
    (m, ks[1]), by the formula of include/slamhip.h (slamhip_hs_hough): float64 on the host, theta = m pi / T taken to (-pi, pi]."""
    b = 1 << int(q)
    theta = m * math.pi / T
    rows, rhs = [], []
    for rec, k in zip(recs, ks):
        psi = k * math.pi / T
        kk, f = k - m, 0
        while kk < 0:
            kk += T; f ^= 1
        n_d = (math.cos(psi), math.sin(psi)); n_s = (math.cos(psi - theta), math.sin(psi - theta))
        r = (b * int(rec["best_shift"]) + info_d["x0"] * n_d[0] + info_d["y0"] * n_d[1] - info_s["x0"] * n_s[0] - info_s["y0"] * n_s[1]
             - info_d["D"] + info_s["D"] + ((b - 1 - (2 * info_s["D"]) % b) if f else 0))
        rows.append(n_d); rhs.append(r)
    det = rows[0][0] * rows[1][1] - rows[0][1] * rows[1][0]
    tx = (rhs[0] * rows[1][1] - rhs[1] * rows[0][1]) / det
    ty = (rows[0][0] * rhs[1] - rows[1][0] * rhs[0]) / det
    th = math.remainder(theta, 2.0 * math.pi)
    if th <= -math.pi:
        th += 2.0 * math.pi
    return tx / stm, ty / stm, th


def align_maps(T, q, n_rot, hs_d, hs_s, info_d, info_s, stm, rotation, shifts, score):
    """The host composition of HectorSLAMProcessor.AlignMaps over three callables -- rotation() -> CC, shifts(pairs) -> HOUGH_SHIFT
    records, score(poses) -> MERGE_REPORT records -- so that the device calls and the host hooks run the same text.
    -> a list of dicts (m, pose, shifts, report), ordered by report.joint[4] descending, then by index."""
    peaks = hough_peaks(rotation(), n_rot)
    ms = [m + e for m in peaks for e in (0, T)]                            # the pi ambiguity
    ka = int(np.argmax(np.asarray(hs_d, np.uint64)))                       # (lowest index on ties)
    kb = (ka + T // 2) % T
    pairs = np.array([[m, k] for m in ms for k in (ka, kb)], np.int32)
    recs = shifts(pairs)
    poses = np.array([hough_pose(m, T, q, (recs[2 * i], recs[2 * i + 1]), (ka, kb), info_d, info_s, stm) for i, m in enumerate(ms)], np.float32)
    reps = score(poses)
    out = [{"m": m, "pose": poses[i].copy(), "shifts": (recs[2 * i].copy(), recs[2 * i + 1].copy()), "report": reps[i].copy()} for i, m in enumerate(ms)]
    out.sort(key=lambda h: -int(h["report"]["joint"][4]))                  # (stable: ties keep the index order)
    return out


def sig_spec(scale, n_ring, ring_cells):
    """A slamhip_sig_spec record (a (1,) SIG_SPEC array; scale rounded to binary32)."""
    sp = np.zeros(1, SIG_SPEC)
    sp["scale"] = np.float32(scale); sp["n_ring"] = int(n_ring); sp["ring_cells"] = int(ring_cells)
    return sp


def debug_sig_table():
    """Rule 1 of slamhip_hs_sig_add (slamhip_debug_sig_table) -> (C, S), two (64,) int32 arrays."""
    cs = np.zeros(2 * SIG_SECTORS, np.int32)
    call("slamhip_debug_sig_table", cs.ctypes.data_as(C.c_void_p))
    return cs[:SIG_SECTORS].copy(), cs[SIG_SECTORS:].copy()


def debug_sig(xy, spec):
    """Rules 2 - 5 of slamhip_hs_sig_add over the (n, 2) float32 points (slamhip_debug_sig; no device involved)
    -> (sig (n_ring,) uint64, a SIG_INFO record)."""
    p = f32(xy, (-1, 2))
    sig = np.zeros(SIG_MAX_RINGS, np.uint64); info = np.zeros(1, SIG_INFO)   # (room for the most a spec the library accepts can ask for)
    call("slamhip_debug_sig", p.ctypes.data_as(C.c_void_p) if p.shape[0] else None, p.shape[0], spec.ctypes.data_as(C.c_void_p),
         sig.ctypes.data_as(C.c_void_p), info.ctypes.data_as(C.c_void_p))
    return sig[:int(spec["n_ring"][0])].copy(), info[0]


def debug_sig_ring(d2, n_ring, ring_cells):
    """Rule 3 as the kernel forms it (slamhip_debug_sig_ring) for an int32 array of d2 -> rings, int32."""
    d = np.ascontiguousarray(d2, np.int32).ravel()
    out = np.zeros(d.shape[0], np.int32)
    call("slamhip_debug_sig_ring", d.ctypes.data_as(C.c_void_p), d.shape[0], int(n_ring), int(ring_cells), out.ctypes.data_as(C.c_void_p))
    return out


def debug_sig_sector(uv):
    """Rule 4 as the kernel forms it (slamhip_debug_sig_sector) for an (n, 2) int32 array of odd (u, v) -> sectors, int32."""
    a = np.ascontiguousarray(uv, np.int32).reshape(-1, 2)
    out = np.zeros(a.shape[0], np.int32)
    call("slamhip_debug_sig_sector", a.ctypes.data_as(C.c_void_p), a.shape[0], out.ctypes.data_as(C.c_void_p))
    return out


def sig_popcounts(store):
    """n_set of every keyframe of a key-major (N, n_ring) uint64 store -> (N,) uint16."""
    s = np.ascontiguousarray(store, np.uint64)
    return np.unpackbits(s.view(np.uint8).reshape(s.shape[0], 8 * s.shape[1]), axis=1).sum(axis=1).astype(np.uint16)


def debug_sig_search(query, store, first, last, min_gap=1, B=1, n_set=None):
    """Rule 7 (query a (n_ring,) uint64 array) or rule 8 (query None) of slamhip_hs_sig_add over a key-major (N, n_ring) uint64 store
    (slamhip_debug_sig_search; no device involved) -> the SIG_HIT_DTYPE records."""
    s = np.ascontiguousarray(store, np.uint64)
    assert s.ndim == 2
    ns = sig_popcounts(s) if n_set is None else np.ascontiguousarray(n_set, np.uint16)
    q = None if query is None else np.ascontiguousarray(query, np.uint64)
    room = max(int(B), 1) if q is not None else max(int(last) - int(first), 1)
    hits = np.zeros(room, SIG_HIT_DTYPE); n = C.c_int32()
    call("slamhip_debug_sig_search", None if q is None else q.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p) if s.shape[0] else None,
         ns.ctypes.data_as(C.c_void_p) if s.shape[0] else None, s.shape[0], s.shape[1], int(first), int(last), int(min_gap), int(B),
         hits.ctypes.data_as(C.c_void_p), C.byref(n))
    return hits[:n.value].copy()


def sig_add_call(name, handle, pose, n_ring, scan=None):
    """slamhip_hs_sig_add (scan None) / slamhip_hsproc_sig_add (scan = (xy, origin)) -> (index, sig (n_ring,) uint64, SIG_INFO record)."""
    idx = C.c_int32(); sig = np.zeros(int(n_ring), np.uint64); info = np.zeros(1, SIG_INFO)
    tail = (fptr(f32(pose, (3,))), C.byref(idx), sig.ctypes.data_as(C.c_void_p), info.ctypes.data_as(C.c_void_p))
    if scan is None:
        call(name, handle, *tail)
    else:
        xy = f32(scan[0], (-1, 2))
        call(name, handle, fptr(xy) if xy.shape[0] else None, xy.shape[0], fptr(f32(scan[1], (2,))), *tail)
    return idx.value, sig, info[0]


def sig_query_call(name, handle, first, last, B, n_ring, scan=None):
    """slamhip_hs_sig_query (scan None) / slamhip_hsproc_sig_query (scan = (xy, origin))
    -> (hits SIG_HIT_DTYPE, the query's sig (n_ring,) uint64, its SIG_INFO record)."""
    hits = np.zeros(SIG_MAX_HITS, SIG_HIT_DTYPE); n = C.c_int32(); sig = np.zeros(int(n_ring), np.uint64); info = np.zeros(1, SIG_INFO)
    tail = (int(first), int(last), int(B), hits.ctypes.data_as(C.c_void_p), C.byref(n), sig.ctypes.data_as(C.c_void_p), info.ctypes.data_as(C.c_void_p))
    if scan is None:
        call(name, handle, *tail)
    else:
        xy = f32(scan[0], (-1, 2))
        call(name, handle, fptr(xy) if xy.shape[0] else None, xy.shape[0], fptr(f32(scan[1], (2,))), *tail)
    return hits[:n.value].copy(), sig, info[0]


def sig_self_call(name, handle, first, last, min_gap):
    """slamhip_hs_sig_self / slamhip_hsproc_sig_self -> (last - first,) SIG_HIT_DTYPE records."""
    hits = np.zeros(max(int(last) - int(first), 1), SIG_HIT_DTYPE)
    call(name, handle, int(first), int(last), int(min_gap), hits.ctypes.data_as(C.c_void_p))
    return hits[:max(int(last) - int(first), 0)].copy()


def sig_pose_guess(key_pose, shift):
    """The pose guess of a hit: the keyframe's position and theta_k - shift * 2 pi / 64 (rule 6's sign), theta taken to (-pi, pi]."""
    th = math.remainder(float(key_pose[2]) - int(shift) * 2.0 * math.pi / SIG_SECTORS, 2.0 * math.pi)
    if th <= -math.pi:
        th += 2.0 * math.pi
    return float(key_pose[0]), float(key_pose[1]), th


def pg_spec(n_outer, n_cg, check_every=None, lam=0.0, tol=1e-6, reserved=0):
    """A slamhip_pg_spec record (a (1,) PG_SPEC array); check_every defaults to min(n_cg, 64)."""
    sp = np.zeros(1, PG_SPEC)
    sp["n_outer"] = int(n_outer); sp["n_cg"] = int(n_cg); sp["check_every"] = min(int(n_cg), 64) if check_every is None else int(check_every)
    sp["reserved"] = int(reserved); sp["lambda"] = float(lam); sp["tol"] = float(tol)
    return sp


def pg_graph(poses, fixed, ij, z, w):
    """The arrays of a pose graph as the library takes them -> (poses (N, 3) float64, fixed (N,) uint8 or None, ij (E, 2) int32,
    z (E, 3) float64, w (E, 3) float64), each contiguous and a copy."""
    p = np.array(poses, np.float64).reshape(-1, 3)
    fx = None if fixed is None else np.ascontiguousarray(np.asarray(fixed).astype(bool).astype(np.uint8))
    e = np.array(ij, np.int32).reshape(-1, 2)
    return p, fx, e, np.array(z, np.float64).reshape(-1, 3), np.array(w, np.float64).reshape(-1, 3)


def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None


def debug_pg_relax(poses, fixed, ij, z, w, spec, entry="slamhip_debug_pg_relax"):
    """The whole definition of slamhip_hs_pg_relax on the host (slamhip_debug_pg_relax; no device involved)
    -> (poses (N, 3), iters PG_ITER (n_outer,), chi2_final, r (E, 3), chi2_e (E,)).  The caller's arrays are not written."""
    p, fx, e, zz, ww = pg_graph(poses, fixed, ij, z, w)
    assert e.shape[0] == zz.shape[0] == ww.shape[0] and (fx is None or fx.shape[0] == p.shape[0])
    iters = np.zeros(max(int(spec["n_outer"][0]), 1), PG_ITER); fin = C.c_double(0.0)
    r = np.zeros((e.shape[0], 3), np.float64); c2 = np.zeros(e.shape[0], np.float64)
    call(entry, _vp(p), _vp(fx), p.shape[0], _vp(e), _vp(zz), _vp(ww), e.shape[0], spec.ctypes.data_as(C.c_void_p),
         iters.ctypes.data_as(C.c_void_p), C.byref(fin), _vp(r), _vp(c2))
    return p, iters[:int(spec["n_outer"][0])].copy(), fin.value, r, c2


def debug_pg_relax_tri(poses, fixed, ij, z, w, spec):
    """The whole definition of slamhip_hs_pg_relax_tri on the host (slamhip_debug_pg_relax_tri; no device involved): what
    debug_pg_relax returns, with the odometry-chain preconditioner (rules T1 - T5)."""
    return debug_pg_relax(poses, fixed, ij, z, w, spec, entry="slamhip_debug_pg_relax_tri")


PG_LM_PRECOND = {"jacobi": 0, "tri": 1}
PG_LM_KIND = {"none": PG_LM_NONE, "dcs": PG_LM_DCS, "gm": PG_LM_GM}


def pg_lm_spec(n_outer, n_cg, check_every=None, precond="jacobi", kind="none", lambda0=1e-3, up=10.0, down=0.1, lambda_min=0.0, lambda_max=1e12,
               tol=1e-6, ftol=0.0, phi=1.0, reserved=0):
    """A slamhip_pg_lm_spec record (a (1,) PG_LM_SPEC array); check_every defaults to min(n_cg, 64); precond "jacobi" / "tri" and kind
    "none" / "dcs" / "gm" by name, or the header's numbers."""
    sp = np.zeros(1, PG_LM_SPEC)
    sp["n_outer"] = int(n_outer); sp["n_cg"] = int(n_cg); sp["check_every"] = min(int(n_cg), 64) if check_every is None else int(check_every)
    sp["precond"] = PG_LM_PRECOND.get(precond, precond); sp["kind"] = PG_LM_KIND.get(kind, kind); sp["reserved"] = int(reserved)
    for name, v in (("lambda0", lambda0), ("up", up), ("down", down), ("lambda_min", lambda_min), ("lambda_max", lambda_max), ("tol", tol),
                    ("ftol", ftol), ("phi", phi)):
        sp[name] = float(v)
    return sp


def pg_robust(robust, E):
    """The robust bytes of slamhip_hs_pg_relax_lm: None, or (E,) uint8, contiguous."""
    if robust is None:
        return None
    rb = np.ascontiguousarray(np.asarray(robust).astype(bool).astype(np.uint8))
    assert rb.shape == (E,), (rb.shape, E)
    return rb


def pg_relax_lm_call(entry, head, E, spec, robust):
    """The tail of slamhip_hs_pg_relax_lm / slamhip_debug_pg_relax_lm behind the arguments `head`
    -> (iters PG_LM_ITER (*out_n,), F_final, f (E,))."""
    rb = pg_robust(robust, E)
    iters = np.zeros(max(int(spec["n_outer"][0]), 1), PG_LM_ITER); n = C.c_int32(0); fin = C.c_double(0.0); f = np.zeros(E, np.float64)
    call(entry, *head, spec.ctypes.data_as(C.c_void_p), _vp(rb), iters.ctypes.data_as(C.c_void_p), C.byref(n), C.byref(fin), _vp(f))
    return iters[:n.value].copy(), fin.value, f


def debug_pg_relax_lm(poses, fixed, ij, z, w, spec, robust=None):
    """The whole definition of slamhip_hs_pg_relax_lm on the host (slamhip_debug_pg_relax_lm; no device involved)
    -> (poses (N, 3), iters PG_LM_ITER (*out_n,), F_final, f (E,)).  The caller's arrays are not written."""
    p, fx, e, zz, ww = pg_graph(poses, fixed, ij, z, w)
    assert e.shape[0] == zz.shape[0] == ww.shape[0] and (fx is None or fx.shape[0] == p.shape[0])
    it, fin, f = pg_relax_lm_call("slamhip_debug_pg_relax_lm", (_vp(p), _vp(fx), p.shape[0], _vp(e), _vp(zz), _vp(ww), e.shape[0]), e.shape[0], spec, robust)
    return p, it, fin, f


def pg_marg_spec(n_cg, check_every=None, precond="tri", lam=0.0, tol=1e-9, max_bytes=0, reserved=0):
    """A slamhip_pg_marg_spec record (a (1,) PG_MARG_SPEC array); check_every defaults to min(n_cg, 64); precond "jacobi" / "tri" by
    name, or the header's numbers; max_bytes 0: the library's 256 MiB."""
    sp = np.zeros(1, PG_MARG_SPEC)
    sp["n_cg"] = int(n_cg); sp["check_every"] = min(int(n_cg), 64) if check_every is None else int(check_every)
    sp["precond"] = PG_LM_PRECOND.get(precond, precond); sp["reserved"] = int(reserved)
    sp["lambda"] = float(lam); sp["tol"] = float(tol); sp["max_bytes"] = int(max_bytes)
    return sp


def pg_marg_rhs_bytes(N, precond):
    """Rule M5's B of slamhip_hs_pg_marginals: the bytes of one right-hand side in the work block."""
    N = int(N); tot = 0; n = N
    while True:
        tot += n
        if n == 1:
            break
        n = (n + 1) // 2
    return 120 * N + 16 * ((N + 255) // 256) + 40 + (24 * (tot - N) + 24 if PG_LM_PRECOND.get(precond, precond) else 0)


def pg_marginals_call(entry, head, spec, pairs):
    """The tail of slamhip_hs_pg_marginals / slamhip_debug_pg_marginals behind the arguments `head`
    -> (blocks (P, 3, 3) float64, cols PG_MARG_COL (R,), info: a PG_MARG_INFO record)."""
    pr = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
    P = pr.shape[0]
    blocks = np.zeros((max(P, 1), 3, 3), np.float64); cols = np.zeros(3 * max(min(P, PG_MARG_MAX_COLS), 1), PG_MARG_COL)
    n = C.c_int32(0); info = np.zeros(1, PG_MARG_INFO)
    call(entry, *head, spec.ctypes.data_as(C.c_void_p), _vp(pr), P, blocks.ctypes.data_as(C.c_void_p), cols.ctypes.data_as(C.c_void_p), C.byref(n),
         info.ctypes.data_as(C.c_void_p))
    return blocks[:P], cols[:n.value].copy(), info[0]


def debug_pg_marginals(poses, fixed, ij, z, w, spec, pairs):
    """The whole definition of slamhip_hs_pg_marginals on the host (slamhip_debug_pg_marginals; no device involved)
    -> (blocks (P, 3, 3), cols PG_MARG_COL (R,), info).  The caller's arrays are not written."""
    p, fx, e, zz, ww = pg_graph(poses, fixed, ij, z, w)
    assert e.shape[0] == zz.shape[0] == ww.shape[0] and (fx is None or fx.shape[0] == p.shape[0])
    return pg_marginals_call("slamhip_debug_pg_marginals", (_vp(p), _vp(fx), p.shape[0], _vp(e), _vp(zz), _vp(ww), e.shape[0]), spec, pairs)


def pg_relative_covariance(pose_i, pose_j, S_ii, S_ij, S_ji, S_jj):
    """The 3 x 3 covariance of rule 3's predicted measurement of an edge (i, j) -- node j seen in node i's frame -- from the four
    marginal blocks of the two nodes: A S_ii A^T + A S_ij B^T + B S_ji A^T + B S_jj B^T, A and B rule 3's Jacobians at the two poses.
    Host NumPy in binary64."""
    xi, yi, ti = (float(v) for v in pose_i); xj, yj, _ = (float(v) for v in pose_j)
    c, s = math.cos(ti), math.sin(ti)
    dx, dy = xj - xi, yj - yi
    ux, uy = c * dx + s * dy, c * dy - s * dx
    A = np.array([[-c, -s, uy], [s, -c, -ux], [0.0, 0.0, -1.0]], np.float64)
    B = np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]], np.float64)
    S_ii, S_ij, S_ji, S_jj = (np.asarray(S, np.float64).reshape(3, 3) for S in (S_ii, S_ij, S_ji, S_jj))
    return A @ S_ii @ A.T + A @ S_ij @ B.T + B @ S_ji @ A.T + B @ S_jj @ B.T


def pg_mahalanobis(r, S_rel, w):
    """r^T (S_rel + diag(1 / w))^-1 r: the squared Mahalanobis distance of an edge's residual r under the graph's relative covariance
    S_rel (pg_relative_covariance) and the edge's own weights w.  Host NumPy in binary64."""
    r = np.asarray(r, np.float64).reshape(3)
    S = np.asarray(S_rel, np.float64).reshape(3, 3) + np.diag(1.0 / np.asarray(w, np.float64).reshape(3))
    return float(r @ np.linalg.solve(S, r))


def debug_pg_tri_apply(poses, fixed, ij, z, w, lam, rhs):
    """Rules T1 - T4 on the host (slamhip_debug_pg_tri_apply; no device involved): z = T^-1 rhs at the given poses -> (N, 3) float64."""
    p, fx, e, zz, ww = pg_graph(poses, fixed, ij, z, w)
    assert e.shape[0] == zz.shape[0] == ww.shape[0] and (fx is None or fx.shape[0] == p.shape[0])
    b = np.array(rhs, np.float64).reshape(-1, 3)
    assert b.shape[0] == p.shape[0]
    out = np.zeros_like(b)
    call("slamhip_debug_pg_tri_apply", _vp(p), _vp(fx), p.shape[0], _vp(e), _vp(zz), _vp(ww), e.shape[0], float(lam), _vp(b), _vp(out))
    return out


def debug_pg_sum(v):
    """Rule 6 of slamhip_hs_pg_relax over a float64 array (slamhip_debug_pg_sum)."""
    a = np.ascontiguousarray(v, np.float64).ravel(); out = C.c_double(0.0)
    call("slamhip_debug_pg_sum", _vp(a), a.shape[0], C.byref(out))
    return out.value


def debug_sincos(a):
    """Rule 2 of slamhip_hs_pg_relax, sh_det_sincos, for a float64 array (slamhip_debug_sincos) -> (sin, cos)."""
    x = np.ascontiguousarray(a, np.float64).ravel(); s = np.zeros_like(x); c = np.zeros_like(x)
    call("slamhip_debug_sincos", _vp(x), x.shape[0], _vp(s), _vp(c))
    return s, c


def pg_edge_between(pose_i, pose_j):
    """The measurement z of an edge (i, j) that the two poses satisfy exactly up to rounding: node j in node i's frame, libm trig in
    binary64 (host composition: HectorSLAMProcessor.RelaxKeyframes forms its odometry edges with it)."""
    xi, yi, ti = (float(v) for v in pose_i); xj, yj, tj = (float(v) for v in pose_j)
    c, s = math.cos(ti), math.sin(ti)
    dx, dy = xj - xi, yj - yi
    return c * dx + s * dy, c * dy - s * dx, math.remainder(tj - ti, 2.0 * math.pi)


def debug_merge_box(pose, stm, ax, ay, sw, sh, x0, y0, x1, y1):
    """The kernels' tile box (slamhip_debug_merge_box) of destination tile [x0, x1] x [y0, y1] -> (u0, v0, u1, v1) in cells of the
    source array, inclusive, or None: no cell of the tile is sourced."""
    box = (C.c_int32 * 4)(); any_ = C.c_int32()
    call("slamhip_debug_merge_box", fptr(f32(pose, (3,))), C.c_float(stm), int(ax), int(ay), int(sw), int(sh), int(x0), int(y0), int(x1), int(y1),
         box, C.byref(any_))
    return tuple(int(v) for v in box) if any_.value else None


def view_words(w):
    """uint32 words per row of a covered or seen bitmap of w cells (slamhip_view_summary, step 4)."""
    return (int(w) + 31) // 32


def view_pack(mask):
    """An (h, w) boolean array -> the (h, view_words(w)) uint32 bitmap of step 4: cell x is bit x & 31 of word x >> 5."""
    m = np.asarray(mask, bool)
    h, w = m.shape
    pad = np.zeros((h, view_words(w) * 32), np.uint8)
    pad[:, :w] = m
    return np.ascontiguousarray(np.packbits(pad, axis=1, bitorder="little")).view(np.uint32).reshape(h, view_words(w))


def view_unpack(bits, w):
    """The (h, view_words(w)) uint32 bitmap of step 4 -> an (h, w) boolean array (the padding bits dropped)."""
    b = np.ascontiguousarray(bits, np.uint32)
    return np.unpackbits(b.view(np.uint8).reshape(b.shape[0], -1), axis=1, bitorder="little")[:, :w].astype(bool)


def debug_view(values, stm, pose, origin, xy, reach, covered=None):
    """V and the summary of one pose of the view gain (slamhip_debug_view; no device involved): values an (h, w) float32 array of cell
    Values, covered an (h, view_words(w)) uint32 bitmap or None.  -> (V as such a bitmap, a VIEW_SUMMARY record)."""
    v = f32(values)
    assert v.ndim == 2
    h, w = v.shape
    xy = f32(xy, (-1, 2))
    cov = None if covered is None else np.ascontiguousarray(covered, np.uint32).reshape(h, view_words(w))
    out = np.empty((h, view_words(w)), np.uint32); s = np.zeros(1, VIEW_SUMMARY)
    call("slamhip_debug_view", fptr(v), w, h, C.c_float(stm), fptr(f32(pose, (3,))), fptr(f32(origin, (2,))), fptr(xy), xy.shape[0], int(reach),
         None if cov is None else cov.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p))
    return out, s[0]


def debug_render(dims, cell_length, cells, update_index, cache_index, scans, origins, poses, keep=False, factors=(0.4, 0.9), flags=None):
    """The definition of slamhip_hs_render on the host (slamhip_debug_render; no device involved): dims a list of (w, h) per level,
    cells a list of CELL_DTYPE arrays per level (copied), update_index / cache_index per level, scans a list of (n_i, 2) point
    arrays, origins (N, 2), poses (N, 3) -> (cells per level, update_index list, cache_index list)."""
    d = np.ascontiguousarray(dims, np.int32).reshape(-1, 2)
    allc = np.ascontiguousarray(np.concatenate([np.ascontiguousarray(c, CELL_DTYPE).reshape(-1) for c in cells]))
    assert allc.size == int((d[:, 0].astype(np.int64) * d[:, 1]).sum())
    ui = np.array(update_index, np.int32).reshape(-1).copy(); ci = np.array(cache_index, np.int32).reshape(-1).copy()
    assert ui.size == ci.size == d.shape[0]
    pts = [f32(s, (-1, 2)) for s in scans]
    off = np.zeros(len(pts) + 1, np.int32)
    off[1:] = np.cumsum([p.shape[0] for p in pts])
    xy = np.ascontiguousarray(np.concatenate(pts, axis=0)) if pts and off[-1] else np.zeros((1, 2), np.float32)
    og = f32(origins, (-1, 2)) if len(pts) else np.zeros((1, 2), np.float32)
    ps = f32(poses, (-1, 3)) if len(pts) else np.zeros((1, 3), np.float32)
    assert len(pts) == 0 or (og.shape[0] == ps.shape[0] == len(pts))
    fl = (RENDER_KEEP if keep else 0) if flags is None else int(flags)
    call("slamhip_debug_render", d.shape[0], _vp(d), C.c_float(cell_length), _vp(allc), _vp(ui), _vp(ci), C.c_float(factors[0]), C.c_float(factors[1]),
         _vp(xy), _vp(off), _vp(og), _vp(ps), len(pts), fl)
    out, at = [], 0
    for w, h in d:
        out.append(allc[at:at + int(w) * int(h)].copy()); at += int(w) * int(h)
    return out, [int(v) for v in ui], [int(v) for v in ci]


def debug_render_world(rects, cell_length, cells, update_index, cache_index, scans, origins, poses, keep=False, factors=(0.4, 0.9), flags=None):
    """The definition of slamhip_hs_render_world on the host (slamhip_debug_render_world; no device involved): rects a list of
    (x0, y0, w, h) per level in window-frame cells, cells a list of CELL_DTYPE arrays per level (copied), the rest as debug_render
    -> (cells per level, update_index list, cache_index list)."""
    r = np.ascontiguousarray(rects, np.int32).reshape(-1, 4)
    allc = np.ascontiguousarray(np.concatenate([np.ascontiguousarray(c, CELL_DTYPE).reshape(-1) for c in cells]))
    assert allc.size == int((r[:, 2].astype(np.int64) * r[:, 3]).sum())
    ui = np.array(update_index, np.int32).reshape(-1).copy(); ci = np.array(cache_index, np.int32).reshape(-1).copy()
    assert ui.size == ci.size == r.shape[0]
    pts = [f32(s, (-1, 2)) for s in scans]
    off = np.zeros(len(pts) + 1, np.int32)
    off[1:] = np.cumsum([p.shape[0] for p in pts])
    xy = np.ascontiguousarray(np.concatenate(pts, axis=0)) if pts and off[-1] else np.zeros((1, 2), np.float32)
    og = f32(origins, (-1, 2)) if len(pts) else np.zeros((1, 2), np.float32)
    ps = f32(poses, (-1, 3)) if len(pts) else np.zeros((1, 3), np.float32)
    assert len(pts) == 0 or (og.shape[0] == ps.shape[0] == len(pts))
    fl = (RENDER_KEEP if keep else 0) if flags is None else int(flags)
    call("slamhip_debug_render_world", r.shape[0], _vp(r), C.c_float(cell_length), _vp(allc), _vp(ui), _vp(ci), C.c_float(factors[0]), C.c_float(factors[1]),
         _vp(xy), _vp(off), _vp(og), _vp(ps), len(pts), fl)
    out, at = [], 0
    for _, _, w, h in r:
        out.append(allc[at:at + int(w) * int(h)].copy()); at += int(w) * int(h)
    return out, [int(v) for v in ui], [int(v) for v in ci]


def debug_render_clip(da, db, T, a0, b0):
    """The steps of a (da, db) line inside windows of T x T offsets whose first are (a0[k], b0[k]) (slamhip_debug_render_clip)
    -> (i0, i1) int32 arrays; empty where i0 > i1."""
    a = np.ascontiguousarray(a0, np.int32).reshape(-1); b = np.ascontiguousarray(b0, np.int32).reshape(-1)
    assert a.size == b.size
    i0 = np.zeros(max(a.size, 1), np.int32); i1 = np.zeros(max(a.size, 1), np.int32)
    call("slamhip_debug_render_clip", int(da), int(db), int(T), a.size, _vp(a) if a.size else _vp(i0), _vp(b) if b.size else _vp(i0), _vp(i0), _vp(i1))
    return i0[:a.size], i1[:a.size]


def scanmatch_spec(scale, half, nx, ny, nt, dtheta, margin=0, reserved=0):
    """A slamhip_scanmatch_spec record (a (1,) SCANMATCH_SPEC array)."""
    sp = np.zeros(1, SCANMATCH_SPEC)
    sp["scale"] = np.float32(scale); sp["half"] = int(half); sp["nx"] = int(nx); sp["ny"] = int(ny); sp["nt"] = int(nt)
    sp["dtheta"] = np.float32(dtheta); sp["margin"] = int(margin); sp["reserved"] = int(reserved)
    return sp


def scan_pairs(pairs):
    """(ref, query, (gx, gy, gtheta)) tuples, or a SCAN_PAIR array -> a contiguous SCAN_PAIR array (a copy)."""
    if isinstance(pairs, np.ndarray) and pairs.dtype == SCAN_PAIR:
        return np.ascontiguousarray(pairs).reshape(-1).copy()
    out = np.zeros(len(pairs), SCAN_PAIR)
    for i, (r, q, g) in enumerate(pairs):
        out[i]["ref"] = int(r); out[i]["query"] = int(q); out[i]["guess"] = f32(g, (3,))
    return out


def scans_match_call(name, handle, spec, pairs):
    """slamhip_hs_scans_match / slamhip_hsproc_scans_match -> a SCANMATCH_RESULT array, one record per pair."""
    pr = scan_pairs(pairs)
    out = np.zeros(max(pr.shape[0], 1), SCANMATCH_RESULT)
    call(name, handle, spec.ctypes.data_as(C.c_void_p), pr.ctypes.data_as(C.c_void_p), pr.shape[0], out.ctypes.data_as(C.c_void_p))
    return out[:pr.shape[0]].copy()


def scans_edges(spec, pairs, results):
    """Rule 6 of slamhip_hs_scans_match (slamhip_hs_scans_edges; no device involved) -> (z (n, 3), w (n, 3) float64, valid (n,) bool)."""
    pr = scan_pairs(pairs); rs = np.ascontiguousarray(results, SCANMATCH_RESULT).reshape(-1)
    assert pr.shape[0] == rs.shape[0]
    n = pr.shape[0]
    z = np.zeros((max(n, 1), 3), np.float64); w = np.zeros((max(n, 1), 3), np.float64); v = np.zeros(max(n, 1), np.int32)
    call("slamhip_hs_scans_edges", spec.ctypes.data_as(C.c_void_p), pr.ctypes.data_as(C.c_void_p), rs.ctypes.data_as(C.c_void_p), n,
         z.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p))
    return z[:n].copy(), w[:n].copy(), v[:n].astype(bool)


def debug_scans_match(scans, spec, pairs):
    """Rules 1 - 5 of slamhip_hs_scans_match on the host (slamhip_debug_scans_match; no device involved): scans a list of (n_i, 2)
    point arrays standing for the scan store -> a SCANMATCH_RESULT array, one record per pair."""
    pts = [f32(s, (-1, 2)) for s in scans]
    off = np.zeros(len(pts) + 1, np.int32)
    off[1:] = np.cumsum([p.shape[0] for p in pts])
    xy = np.ascontiguousarray(np.concatenate(pts, axis=0)) if pts and off[-1] else np.zeros((1, 2), np.float32)
    pr = scan_pairs(pairs)
    out = np.zeros(max(pr.shape[0], 1), SCANMATCH_RESULT)
    call("slamhip_debug_scans_match", _vp(xy), _vp(off), len(pts), spec.ctypes.data_as(C.c_void_p), pr.ctypes.data_as(C.c_void_p), pr.shape[0],
         out.ctypes.data_as(C.c_void_p))
    return out[:pr.shape[0]].copy()


def loops_spec(gamma, q_t, q_theta, n_starts=8, min_clique=1, flags=0, reserved=0):
    """A slamhip_loops_spec record (a (1,) LOOPS_SPEC array)."""
    sp = np.zeros(1, LOOPS_SPEC)
    sp["gamma"] = float(gamma); sp["q_t"] = float(q_t); sp["q_theta"] = float(q_theta); sp["n_starts"] = int(n_starts)
    sp["min_clique"] = int(min_clique); sp["flags"] = int(flags); sp["reserved"] = int(reserved)
    return sp


def loops_words(L):
    """Words of a row of the consistency matrix: ceil(L / 64)."""
    return (int(L) + 63) // 64


def loops_call(name, handle, poses, ij, z, w, spec, use=None, adj=False, d2=False):
    """slamhip_hs_loops_consistent (handle: the hs) or slamhip_debug_loops_consistent (handle None; no device involved) ->
    dict(keep (L,) bool, deg (L,) int32, info a LOOPS_INFO record, adj (L, ceil(L / 64)) uint64 or None[, d2 (L, L) float64: the hook's]).
    adj=True sets SLAMHIP_LOOPS_ADJ in a copy of the spec."""
    p = np.array(poses, np.float64).reshape(-1, 3)
    e = np.array(ij, np.int32).reshape(-1, 2); zz = np.array(z, np.float64).reshape(-1, 3); ww = np.array(w, np.float64).reshape(-1, 3)
    L = e.shape[0]
    assert zz.shape[0] == L and ww.shape[0] == L
    u = None if use is None else np.ascontiguousarray(np.asarray(use).astype(bool).astype(np.uint8))
    assert u is None or u.shape == (L,)
    sp = spec.copy()
    if adj:
        sp["flags"] |= LOOPS_ADJ
    keep = np.zeros(max(L, 1), np.uint8); deg = np.zeros(max(L, 1), np.int32); info = np.zeros(1, LOOPS_INFO)
    A = np.zeros((max(L, 1), max(loops_words(L), 1)), np.uint64) if adj else None
    args = [_vp(p), p.shape[0], _vp(e), _vp(zz), _vp(ww), _vp(u), L, sp.ctypes.data_as(C.c_void_p), _vp(keep), _vp(deg),
            info.ctypes.data_as(C.c_void_p), _vp(A)]
    out = dict(adj=None)
    if handle is None:
        D = np.zeros((max(L, 1), max(L, 1)), np.float64) if d2 else None
        call(name, *args, _vp(D))
        if d2:
            out["d2"] = D[:L, :L]
    else:
        call(name, handle, *args)
    out.update(keep=keep[:L].astype(bool), deg=deg[:L].copy(), info=info[0].copy())
    if adj:
        out["adj"] = A[:L]
    return out


def debug_loops_consistent(poses, ij, z, w, spec, use=None, adj=True, d2=False):
    """Rules 1 - 6 of slamhip_hs_loops_consistent on the host (slamhip_debug_loops_consistent; no device involved): loops_call's dict."""
    return loops_call("slamhip_debug_loops_consistent", None, poses, ij, z, w, spec, use=use, adj=adj, d2=d2)
