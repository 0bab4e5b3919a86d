// hs_internal.h -- device state of the HectorSLAM operator object (slamhip_hs) and what its units share.  slamhip_hs is a calloc'ed
// C struct that frees its own blocks by hand (slamhip_hs_destroy); a unit's struct owns its blocks (hs_block, hs_blocks.h) and
// needs no free function here: it is dropped through the unit table at the struct's end.
#pragma once
#include "common.h"
#include "m3x2.h"
#include <stdlib.h>

#define HS_MAX_LEVELS 8
#define HS_NONE 0xFFFFFFFFu
#define HS_MAX_UNITS 24                    // slots of slamhip_hs's unit table: one per unit pointer of the struct (18), and room
// sizes of K4's (hs_match.hip) and K5's (hs_update.hip) LDS tables that host entry points of other units test
#define HS_LDS_PTS 2048                    // scan points kept in LDS (16 KB); longer scans are read from global memory
#define HS_REF_MAX_T 64                    // ParallelWorker.Work waits with WaitHandle.WaitAll: at most 64 handles (BaseSLAM/ParallelWorker.cs:113-115)
#define K5_LDS_LINES 3072

struct hs_level {
    int w, h; float cell, stm;             // MapProperties: Dimensions, CellLength, ScaleToMap (MapProperties.cs:22-32)
    sh_m3x2 map_t_world, world_t_map;      // GridMap.cs:46-47
    slamhip_cell *d_cells;                 // mapArray (GridMap.cs:13) in the reference's own layout, LogOddsCell {UpdateIndex, Value} (LogOddsCell.cs:16-21): the grid
                                           // update reads and writes a cell with ONE 8-byte access (two arrays: 30.8 -> 26.9 us per update with the second one left out)
    float *d_prob;                         // GetCachedProbability of every cell (OccGridMap.cs:97-107), kept current by every writer of d_cells
    slamhip_cell *d_cells_alt; float *d_prob_alt;   // the second set slamhip_hs_shift moves the window into (allocated by the first shift); the
                                           // launch reads d_cells / d_prob, writes these, and the host then swaps the names
    unsigned long long *d_cache;           // cacheArray (OccGridMap.cs:16), one CachedMapElement {Value, Index} per cell as ONE 8-byte word
                                           // (Value's bits low, Index high); allocated when the reference's cache is first turned on
    int curr_update_index;                 // OccGridMap.cs:20
    int curr_cache_index;                  // OccGridMap.cs:19, kept in every mode: UpdateByScan +1 (:147), Reset 0 (:248)
    int iterations;                        // EstimateIterations (OccGridMap.cs:53)
};

struct hs_level_dev {                      // what the kernels need, by value
    int w, h; float cell, stm;
    sh_m3x2 map_t_world, world_t_map;
    const float *prob;                     // what the matcher's taps read: exp and divide happen when a cell changes, not per tap
    const slamhip_cell *cells;             // (HS_PROB_MODE 1 / 2, developer experiment: the taps read the cells and form the probabilities themselves)
    int iterations;
};
#ifndef HS_PROB_MODE
#define HS_PROB_MODE 0                     // 0: the probability grid, kept by every writer of the cells | 1: from the cells, exact expf and division per tap | 2: ... hardware exp and reciprocal
#endif

struct hs_backing;                         // hs_tiles.h
struct hs_world;                           // hs_world.hip
struct hs_lattice;                         // hs_lattice.hip
struct hs_pose_batch;                      // hs_blocks.h
struct hs_field_unit;                      // hs_field.h
struct hs_frontier;                        // hs_frontier.hip
struct hs_nav;                             // hs_nav.hip
struct hs_rollout;                         // hs_rollout.hip
struct hs_mcl;                             // hs_mcl.hip
struct hs_merge;                           // hs_merge.hip
struct hs_view;                            // hs_view.hip
struct hs_hough;                           // hs_hough.hip
struct hs_sig;                             // hs_sig.hip
struct hs_pg;                              // hs_pg.hip
struct hs_scans;                           // hs_scans.h
struct hs_scanmatch;                       // hs_scanmatch.hip
struct hs_loops;                           // hs_loops.hip
struct hs_bnb;                             // hs_bnb.hip
template <typename T> struct hs_field_of;  // hs_dfield.h
typedef hs_field_of<uint16_t> hs_field;
struct slamhip_hs {
    slamhip_ctx *ctx;
    int n_levels;
    hs_level lv[HS_MAX_LEVELS];
    float odds_free, odds_occ, lo_free, lo_occ;          // OccGridMap.cs:24-27
    int n_points, cap_points;
    float2 *d_pts; float origin[2];
    float2 *d_pts_base; int pts_buf; uint64_t launch_count, launch_done, pts_use[2], match_launch_no;   // two device blocks used in turn; which launches read which (see slamhip_cs_set_scan)
    float *h_pts; hipEvent_t ev_pts; bool pts_in_flight;   // pinned staging of the scan: one async copy (or upload launch), no wait in set_scan
    bool upload_pending; size_t upload_bytes;              // set_scan filled the staging block; the first launch that reads the points issues the upload (hs_flush_scan) -- a single match pulls the block itself
    uint32_t upload_seq;                                   // upload launches issued; the launch stores it behind the staged points (h_pts + 2 * cap) when it has read them
    float *d_io; float *h_io; int cap_io;                // hints in / poses out (floats)
    // K5 line tables, per level: lines by index, lines sorted by (direction class, slope bucket), bucket starts, header
    void *d_k5_byidx, *d_k5_cand; int *d_k5_start, *d_k5_hdr; int cap_lines;
    int *d_k5_sec; int k5_sec_parity; bool k5_toggle_pending;                        // [2][HS_MAX_LEVELS][K5_SEC] sector records of the cell kernel: an update reads the set the last one wrote
    int match_threads;                                     // slamhip_hs_set_match_threads: 0 the device's summation order, 1 .. HS_REF_MAX_T the reference's
    int ref_cache;                                         // slamhip_hs_set_reference_cache: 1 every probability reader goes through d_cache
    // the match reports (slamhip_match_report): the batch's reports and the best-of-batch key word in device memory, and a pinned,
    // device-visible block the host reads them from -- a single blocking match stores its report there itself, in front of the
    // mailbox's sequence word (the mailbox is 64 B, the report 76)
    slamhip_match_report *d_rep, *h_rep; int cap_rep; unsigned long long *d_best_key;
    int64_t win_ox, win_oy;                                // slamhip_hs_shift: where cell (0, 0) of level 0 lies in the world, in level-0 cells (host-side books only)
    hipEvent_t ev_call;                                    // what the blocking calls of K7 .. K14 record and wait on before they return (hs_call_finish, hs_blocks.h)
    struct hs_backing *bk;                                 // slamhip_hs_set_backing: the tile pool and its host directory; nullptr while backing is off
    struct hs_world *wp;                                   // slamhip_hs_world_cells_upload / _world_extends: their staging buffer, made by the first call, kept
    struct hs_lattice *lat;                                // slamhip_hs_lattice_search: the class map and the result blocks, made by the first search, kept
    struct hs_pose_batch *trc;                                  // slamhip_hs_trace: the poses' and the results' blocks, made by the first trace, kept
    struct hs_field_unit *dfd;                                 // slamhip_hs_distance_field / _score: the field of E and the results' blocks, made by the first call, kept
    struct hs_frontier *frl;                               // slamhip_hs_frontiers: the frontier words, the union-find's arrays and the results' blocks, made by the first call, kept
    struct hs_nav *nav;                                    // slamhip_hs_nav_field: the traversable words, costs, dirs, tile flags and the results' blocks, made by the first call, kept
    struct hs_rollout *rol;                                // slamhip_hs_rollouts: the commands', body points' and results' blocks, made by the first call, kept
    struct hs_mcl *mcl;                                    // slamhip_hs_mcl_set / _step / _get: the particle set and the step's blocks, made by the first set, kept
    struct hs_merge *mrg;                                  // slamhip_hs_merge_set_source / _score / _apply: the source map and the reports' blocks, made by the first set_source, kept
    struct hs_view *vw;                                    // slamhip_hs_view_gain / _select / _set_covered: the covered layer, the slots and the results' blocks, made by the first call, kept
    struct hs_field_unit *nrs;                                // slamhip_hs_nearest_field / _pairs: the row offsets and the pairs of E and the results' blocks, made by the first call, kept
    struct hs_hough *hgh;                                  // slamhip_hs_hough / _hough_rotation / _hough_shifts: the two slots' votes, spectra and row extents and the results' blocks, made by the first call, kept
    struct hs_sig *sig;                                    // slamhip_hs_sig_configure / _sig_add / _sig_query / _sig_self: the spec, the store of keyframe signatures, the poses and the results' blocks, made by configure, kept
    struct hs_scans *scn;                                  // slamhip_hs_scans_add / slamhip_hs_render: the store of keyframe scans -- the records on the host, the points in one device pool -- and the blocks of a render, made by the first call, kept
    struct hs_pg *pg;                                      // slamhip_hs_pg_set / _pg_relax / _pg_get / _pg_residuals: the pose graph's one device block and its pinned staging, made by the first set, kept
    struct hs_scanmatch *smt;                              // slamhip_hs_scans_match: the pairs' and the results' device blocks and their pinned staging, made by the first call, kept
    struct hs_loops *lps;                                  // slamhip_hs_loops_consistent: the edges', the matrix's and the results' device block and its pinned staging, made by the first call, kept
    struct hs_bnb *bnb;                                    // slamhip_hs_lattice_search_bnb: the pooled maps, the frontiers and the results' blocks, made by the first call, kept
    // how to drop each unit above that has been made (hs_unit records it, a slot once; hs_blocks.h): what slamhip_hs_destroy walks
    void (*unit_drop[HS_MAX_UNITS])(slamhip_hs *); int n_units;
};

struct hs_levels_arg { hs_level_dev lv[HS_MAX_LEVELS]; int n; };
struct hs_cache_arg { unsigned long long *c[HS_MAX_LEVELS]; int epoch[HS_MAX_LEVELS]; };
// what a match is to report (hs_run_match): out_reports -- B reports, or the winner's alone with best_index set (slamhip_hs_match_best:
// `out` is then the winner's pose)
struct hs_report_req { slamhip_match_report *out_reports; int32_t *best_index; };

// The update gated on the device (HectorSLAMProcessor's per-scan flow, slamhip_hsproc_update): the launch is enqueued right
// behind the match, before the host has the pose -- the kernel reads the matched pose the match left in device memory, applies
// the processor's own test (HectorSLAMProcessor.cs:107-109: moved more than min_dist or turned more than min_angle since the
// last update) with the very float operations the host applies to the pose it receives, and either returns at once or forms
// the level transforms (OccGridMap.cs:120-123) itself.  Without it the update waited for host round trip + launch: 11.5 us of
// idle device between the two kernels of a scan.
struct k5_gate { const float *d_pose; float last[3]; float min_dist, min_angle; float stm[HS_MAX_LEVELS]; int on; };
__host__ __device__ static inline float hs_deg_diff(float a, float b)      // MathEx.DegDiff (BaseSLAM/MathEx.cs:69-73)
{
    float d = ((a - b) + 180.0f) / 360.0f;
    return ((d - floorf(d)) * 360.0f) - 180.0f;
}
__host__ __device__ static inline bool hs_moved_enough(const float pose[3], const float last[3], float min_dist, float min_angle)
{
    const float ddx = pose[0] - last[0], ddy = pose[1] - last[1];
    const float dist2 = ddx * ddx + ddy * ddy;                            // Vector2.DistanceSquared :107
    return dist2 > min_dist * min_dist || hs_deg_diff(pose[2], last[2]) > min_angle;   // :108 (radians through DegDiff, as the reference does)
}

// OccGridMap.GetCachedProbability (:97-107)
__device__ static inline float hs_prob_v(float v)
{
    const float odds = expf(v);                                            // :101
    return odds / (odds + 1.0f);                                           // :102
}
// a CachedMapElement {Value, Index} as one word (hs_cache_taps, hs_match.hip)
__device__ static __forceinline__ float hs_cache_entry_value(unsigned long long e) { return __uint_as_float((unsigned)e); }
__device__ static __forceinline__ bool hs_cache_entry_hit(unsigned long long e, int epoch) { return (int)(e >> 32) == epoch; }   // :99
__device__ static __forceinline__ unsigned long long hs_cache_entry(float v, int epoch)
{
    return ((unsigned long long)(unsigned)epoch << 32) | (unsigned long long)__float_as_uint(v);
}
// LogOddsCell.Reset (LogOddsCell.cs:38-42), and the probability every writer of the cells keeps beside it: hs_prob_v(0.0f) =
// exp(0) / (exp(0) + 1), exactly 0.5f
__host__ __device__ static inline slamhip_cell hs_reset_cell() { slamhip_cell c; c.update_index = -1; c.value = 0.0f; return c; }
#define HS_RESET_PROB 0.5f
// OccGridMap.ProbToLogOdds (OccGridMap.cs:86-90), on the host: what slamhip_hs_create and slamhip_hs_set_factors form lo_free and lo_occ by
static inline float hs_prob_to_logodds(float prob) { const float odds = prob / (1.0f - prob); return logf(odds); }

// hector.hip
// launches the scan upload that slamhip_hs_set_scan left pending (every launch that reads the points calls it first)
int32_t hs_flush_scan(slamhip_hs *hs);
// a level's cacheArray := new CachedMapElement[] (enqueued on the operator's stream; slamhip_hs_set_reference_cache)
void    hs_cache_clear_enqueue(slamhip_hs *hs, int level);
// hs_match.hip
int32_t hs_run_match(slamhip_hs *hs, const float *hints, int B, float *out, int only_level, int iters, uint32_t *defer_seq = nullptr,
                     const hs_report_req *rq = nullptr);
int32_t hs_match_collect(slamhip_hs *hs, uint32_t seq, float *out, slamhip_match_report *out_report = nullptr);
// hs_update.hip
// the launches of UpdateByScan on the operator's stream; gate_in: the device-gated form, committed by hs_update_commit once the
// host knows that the update took place
int32_t hs_update_enqueue(slamhip_hs *hs, const float pose[3], const k5_gate *gate_in = nullptr);
void    hs_update_commit(slamhip_hs *hs);
bool    hs_update_gateable(slamhip_hs *hs);
// hs_window.hip
void    hs_bk_reset(slamhip_hs *hs);        // slamhip_hs_reset with backing on: the directory goes, the pool stays -- every slot Reset again
void    hs_bk_free(slamhip_hs *hs);         // (the caller has drained the stream)
// hs_lattice.hip
// K7's class map of one level -- 2 bits per cell, rows of wpr words -- for another launch on the operator's stream: w x h cells
// whose first is cell (x0, y0) of the window's frame (the window itself, or the world's rectangle R).  _prepare plans and
// allocates and launches nothing; _enqueue packs.
struct hs_class_map { const uint32_t *cls; int w, h, wpr, x0, y0; };
int32_t hs_lat_pack_prepare(slamhip_hs *hs, int level, bool world, hs_class_map *M);
int32_t hs_lat_pack_enqueue(slamhip_hs *hs, int level, bool world, const hs_class_map *M);
// what K7 refuses for a spec alone; cap_nodes false: without the 2^26-node rule (K24)
int32_t hs_lat_check_spec(const slamhip_hs *hs, const slamhip_lattice_spec *S, bool cap_nodes);
// what follows the search in slamhip_hs_relocalise and in slamhip_hs_relocalise_world (its pre-checks: _world_check), from n_theta keys
int32_t hs_lat_reloc_finish(slamhip_hs *hs, const slamhip_lattice_spec *spec, const uint64_t *keys, int32_t B, float out_pose[3],
                            slamhip_match_report *out_report, slamhip_reloc_info *out_info);
int32_t hs_lat_reloc_world_check(const slamhip_hs *hs);
int32_t hs_lat_reloc_world_finish(slamhip_hs *hs, const slamhip_lattice_spec *spec, const uint64_t *keys, int32_t B, float out_pose[3],
                                  slamhip_match_report *out_report, slamhip_world_reloc_info *out_info);
// hs_trace.hip
// what slamhip_hs_trace refuses for its arguments alone, for a scan of n_points (scan_is_set false: the caller is about to set one,
// so its absence is no error)
int32_t hs_trc_check(int n_levels, int32_t level, int32_t B, int32_t world, bool want_beams, int n_points, bool scan_is_set);
// hs_dfield.hip
// what slamhip_hs_distance_field and _score refuse for level, world, site_mask and radius (K13 refuses the same); who: the message's prefix
int32_t hs_df_check(const char *who, int n_levels, int32_t level, int32_t world, int32_t site_mask, int32_t radius);
// ... and what slamhip_hs_distance_score refuses for its arguments alone (n_points, scan_is_set: as hs_trc_check)
int32_t hs_df_check_score(const char *who, int n_levels, int32_t level, int32_t world, int32_t site_mask, int32_t radius, int32_t B, bool want_points,
                          int n_points, bool scan_is_set);
// K9's field of one level (hs_field, hs_dfield.h) for another launch on the operator's stream.  _prepare plans (the class map too),
// allocates and launches nothing; _enqueue packs the class map and launches the field's two kernels.  slamhip_hs_distance_field and
// _score run these two themselves.
int32_t hs_df_field_prepare(slamhip_hs *hs, int level, bool world, int site_mask, int radius, hs_class_map *M, hs_field *E);
int32_t hs_df_field_enqueue(slamhip_hs *hs, int level, bool world, const hs_class_map *M, const hs_field *E, int site_mask);
// hs_nav.hip
// K11's counter block (k11_peek and k11_emit store it to pinned memory)
#define K11_C_TRAV 0
#define K11_C_REACHED 1
#define K11_C_USED 2
#define K11_C_BLOCKED 3
#define K11_C_MAXCOST 4
#define K11_C_FLAG 5
#define K11_CTRS 8
// K11's field of one level for another launch on the operator's stream (slamhip_hs_rollouts): what slamhip_hs_nav_field runs up to
// the end of its relaxation, by the same function.  _check refuses what that call refuses for spec and sources, nothing launched;
// _for_rollouts returns with the costs of M final in device memory and the stream drained (the batch waits are the field's own).
// K11_C_REACHED and K11_C_MAXCOST of ctr are still 0: k11_dirs, which counts them, is not run.
struct hs_nav_view { const uint32_t *tw; const uint32_t *cost; uint32_t *ctr; int twpr; hs_class_map M; int rounds; };
int32_t hs_nav_check_field(int n_levels, const slamhip_nav_spec *spec, const int32_t *sources, int32_t S);
int32_t hs_nav_field_for_rollouts(slamhip_hs *hs, const slamhip_nav_spec *spec, const int32_t *sources, int32_t S, hs_nav_view *out);
// hs_mcl.hip
// what slamhip_hs_mcl_step refuses before it launches anything, for a scan of n_points (scan_is_set false: the caller is about to set
// one, so its absence is no error)
int32_t hs_mcl_check_step(const slamhip_hs *hs, const slamhip_mcl_spec *spec, int n_points, bool scan_is_set);
// hs_merge.hip
void    hs_merge_drop_source(slamhip_hs *hs);   // slamhip_hs_reset, slamhip_hs_merge_clear_source: no source from here on; the blocks stay
// what slamhip_hs_merge_score and _apply refuse before they launch anything
int32_t hs_merge_check_score(const slamhip_hs *hs, int32_t B);
int32_t hs_merge_check_apply(const slamhip_hs *hs, int32_t rule, float value_limit);
// the merge source's packed classes as a class map whose first cell is source-frame cell (ax, ay), and its level, for another launch
// on the operator's stream (K17's slot 1); SLAMHIP_ERR_STATE without a source
int32_t hs_merge_source_map(const slamhip_hs *hs, hs_class_map *M, int *level);
// hs_view.hip
// what slamhip_hs_view_gain and _view_select refuse for their arguments alone, for a scan of n_points (scan_is_set false: the caller
// is about to set one, so its absence is no error)
int32_t hs_view_check_gain(const slamhip_hs *hs, int32_t level, int32_t reach, int32_t B, int32_t commit, int n_points, bool scan_is_set);
int32_t hs_view_check_select(const slamhip_hs *hs, int32_t level, int32_t reach, int32_t mode, int32_t min_gain, int32_t B, int32_t k, int n_points,
                             bool scan_is_set);
// hs_nearest.hip
// what slamhip_hs_nearest_pairs refuses for its arguments alone (n_points, scan_is_set: as hs_trc_check)
int32_t hs_nr_check_pairs(int n_levels, int32_t level, int32_t world, int32_t site_mask, int32_t radius, int32_t B, bool want_pairs, int n_points,
                          bool scan_is_set);
// hs_hough.hip
void    hs_hg_drop_slot(slamhip_hs *hs, int slot);   // slamhip_hs_reset (both), slamhip_hs_merge_set_source / _clear_source (slot 1): the slot is empty from here on; the blocks stay
// hs_sig.hip
void    hs_sg_reset(slamhip_hs *hs);        // slamhip_hs_reset: the store is empty from here on; the blocks and the spec stay
// what slamhip_hs_sig_add and _sig_query refuse before they launch anything
int32_t hs_sg_check_add(const slamhip_hs *hs);
int32_t hs_sg_check_query(const slamhip_hs *hs, int32_t first, int32_t last, int32_t B);
// hs_pg.hip
void    hs_pg_reset(slamhip_hs *hs);        // slamhip_hs_reset: no graph from here on; the blocks stay
// hs_render.hip
void    hs_scn_reset(slamhip_hs *hs);       // slamhip_hs_reset: the store is empty from here on; the pool and the blocks stay
