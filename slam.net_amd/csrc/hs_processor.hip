// hs_processor.hip -- HectorSLAMProcessor (slamhip_hsproc_*): the per-scan flow over the operator object.  Host code only.
#include "hs_internal.h"
#include <algorithm>
#include <chrono>
#include <stddef.h>
#include <vector>

// ---- HectorSLAMProcessor (Main/HectorSLAMProcessor.cs) ---------------------------------------------------------------
struct slamhip_hsproc {
    slamhip_hs *hs;
    float start_pose[3], match_pose[3], last_update_pose[3];
    float match_timing, update_timing;
    float min_dist, min_angle;
    unsigned upd_hist;                                     // the last scans' update decisions, newest in bit 0
    int want_report, report_valid;                         // slamhip_hsproc_set_match_report; the last Update's match left `report`
    slamhip_match_report report;
    int scroll_trigger;                                    // slamhip_hsproc_set_scroll: 0 off.  match_pose and last_update_pose are kept in the WINDOW's frame
};

static const float F_MIN = -3.40282347e+38f;       // float.MinValue

extern "C" int32_t slamhip_hsproc_create(slamhip_ctx *ctx, float res, int32_t w, int32_t h, const float start[3], int32_t depth,
                                         slamhip_hsproc **out)
{
    SH_CHECK_ARG(ctx && start && out);
    slamhip_hs *hs = nullptr;
    SH_TRY(slamhip_hs_create(ctx, res, w, h, depth, &hs));                // :71
    slamhip_hsproc *p = (slamhip_hsproc *)calloc(1, sizeof(*p));
    if (!p) { slamhip_hs_destroy(hs); SH_FAIL(SLAMHIP_ERR_NOMEM, "out of host memory"); }
    p->hs = hs;
    memcpy(p->start_pose, start, sizeof(float) * 3);
    memcpy(p->match_pose, start, sizeof(float) * 3);                      // :75
    p->last_update_pose[0] = p->last_update_pose[1] = p->last_update_pose[2] = F_MIN;   // :76
    p->min_dist = 0.3f; p->min_angle = 0.13f;                             // :51,:56
    *out = p;
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hsproc_destroy(slamhip_hsproc *p)
{
    if (!p) return SLAMHIP_OK;
    slamhip_hs_destroy(p->hs);
    free(p);
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hsproc_reset(slamhip_hsproc *p)
{
    SH_CHECK_ARG(p);
    SH_TRY(slamhip_hs_reset(p->hs));                                      // :133
    memcpy(p->match_pose, p->start_pose, sizeof(float) * 3);              // :136
    p->last_update_pose[0] = p->last_update_pose[1] = p->last_update_pose[2] = F_MIN;   // :137
    p->upd_hist = 0;
    p->report_valid = 0;
    return SLAMHIP_OK;
}

// (float)origin * cell0 per axis: what takes a world coordinate to the window's frame and back (slamhip_hs_shift's contract)
static inline void hsproc_window_offset(const slamhip_hsproc *p, float off[2])
{
    off[0] = (float)p->hs->win_ox * p->hs->lv[0].cell;
    off[1] = (float)p->hs->win_oy * p->hs->lv[0].cell;
}

// The two frames.  Poses and cells cross the C-ABI in the world's frame; the hs works in the window's.  While the window has never
// moved the two are one and every bit passes through, -0.0f included; after that a position costs one rounded subtraction on the
// way in and one rounded addition on the way out, per axis.  The heading is the same in both.
static inline bool hsproc_moved(const slamhip_hsproc *p) { return p->hs->win_ox != 0 || p->hs->win_oy != 0; }
static inline void hsproc_pose_to_window(const slamhip_hsproc *p, const float world[3], float out[3])
{
    float off[2];
    hsproc_window_offset(p, off);
    if (hsproc_moved(p)) { out[0] = world[0] - off[0]; out[1] = world[1] - off[1]; out[2] = world[2]; }
    else memmove(out, world, sizeof(float) * 3);
}
static inline void hsproc_pose_to_world(const slamhip_hsproc *p, const float window[3], float out[3])
{
    float off[2];
    hsproc_window_offset(p, off);
    if (hsproc_moved(p)) { out[0] = window[0] + off[0]; out[1] = window[1] + off[1]; out[2] = window[2]; }
    else memmove(out, window, sizeof(float) * 3);
}
// B poses: the caller's own array while the window has never moved, else `buf`
static const float *hsproc_poses_to_window(const slamhip_hsproc *p, const float *world, int32_t B, std::vector<float> &buf)
{
    if (!hsproc_moved(p)) return world;
    buf.resize(3 * (size_t)B);
    for (int i = 0; i < B; i++) hsproc_pose_to_window(p, world + 3 * i, buf.data() + 3 * i);
    return buf.data();
}
// a cell coordinate of one level, o = origin >> level on its axis: clamped where it lies too far out to be a cell of M wherever M is
static inline int32_t hsproc_cell_to_window(int64_t v, int64_t o)
{
    const int64_t far = (int64_t)1 << 30;
    return (int32_t)std::min(std::max(v - o, -far), far);
}

// HectorSLAMProcessor.Update (:83-125) in the window's frame: hint, match_pose and last_update_pose all are window-frame poses
static int32_t hsproc_update_window(slamhip_hsproc *p, const float *xy, int32_t n, const float origin[2],
                                    const float hint[3], int32_t map_without_matching, int32_t *out_updated)
{
    p->report_valid = 0;
    const hs_report_req rq = { &p->report, nullptr };
    SH_TRY(slamhip_hs_set_scan(p->hs, xy, n, origin));
    static const bool wait_update = sh_env_set("SLAMHIP_HS_WAIT_UPDATE");
    // (worth it when the update does take place: a gated launch that returns at once still costs the stream ~15 us -- 512 workgroups
    // of 1024 lanes are dispatched to find that out -- so the flow is taken while the last two scans both updated the map: measured,
    // every scan updating 70 -> 66 us per scan; one scan in five, where it is never taken, 55 either way, 71 if it always were)
    if (!map_without_matching && !wait_update && (p->upd_hist & 3u) == 3u && hs_update_gateable(p->hs)) {
        // The per-scan flow on the device: match, then the grid update gated by the processor's own test (k5_gate) -- both enqueued
        // before the host has the pose, which it then takes from the mailbox and puts to the same test for its own books.
        slamhip_hs *hs = p->hs;
        sh_mail_guard lock(hs->ctx);
        auto t0 = std::chrono::steady_clock::now();
        float m[3];
        uint32_t seq = 0;
        SH_TRY(hs_run_match(hs, hint, 1, m, -1, 0, &seq, p->want_report ? &rq : nullptr));   // :93
        k5_gate g;
        memset(&g, 0, sizeof(g));
        g.d_pose = hs->d_io + 3;                                          // (the single match's result in device memory: hs_run_match)
        memcpy(g.last, p->last_update_pose, sizeof(g.last));
        g.min_dist = p->min_dist; g.min_angle = p->min_angle;
        const int32_t rc_u = hs_update_enqueue(hs, hint, &g);
        auto t1 = std::chrono::steady_clock::now();
        SH_TRY(hs_match_collect(hs, seq, m, p->want_report ? &p->report : nullptr));
        SH_TRY(rc_u);
        p->report_valid = p->want_report;
        memcpy(p->match_pose, m, sizeof(m));
        auto t2 = std::chrono::steady_clock::now();
        const float ms_u = std::chrono::duration<float, std::milli>(t1 - t0).count();      // (launches of match + update; the match's share is a few us)
        const float ms_m = std::chrono::duration<float, std::milli>(t2 - t0).count();
        p->match_timing = (3.0f * p->match_timing + ms_m) / 4.0f;         // :96
        int updated = 0;
        if (hs_moved_enough(p->match_pose, p->last_update_pose, p->min_dist, p->min_angle)) {   // :107-108, as the kernel decided
            hs_update_commit(hs);
            p->update_timing = (3.0f * p->update_timing + ms_u) / 4.0f;   // :115 (the time of the enqueue)
            memcpy(p->last_update_pose, p->match_pose, sizeof(float) * 3);    // :118
            updated = 1;                                                  // :122
        } else hs->k5_toggle_pending = false;
        p->upd_hist = (p->upd_hist << 1) | (unsigned)updated;
        if (out_updated) *out_updated = updated;
        return SLAMHIP_OK;
    }
    if (!map_without_matching) {                                          // :89
        auto t0 = std::chrono::steady_clock::now();
        float m[3];
        SH_TRY(hs_run_match(p->hs, hint, 1, m, -1, 0, nullptr, p->want_report ? &rq : nullptr));   // :93
        p->report_valid = p->want_report;
        memcpy(p->match_pose, m, sizeof(m));
        const float ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        p->match_timing = (3.0f * p->match_timing + ms) / 4.0f;           // :96
    } else {
        memcpy(p->match_pose, hint, sizeof(float) * 3);                   // :100
    }
    int updated = 0;
    if (hs_moved_enough(p->match_pose, p->last_update_pose, p->min_dist, p->min_angle) ||   // :107-108
        map_without_matching) {                                           // :109
        // The grid update returns nothing to the host: it is enqueued and runs on while the caller prepares its next scan --
        // the next match, a download or an export is ordered behind it on the operator's stream (UpdateTiming :115 is then
        // the time of the enqueue; SLAMHIP_HS_WAIT_UPDATE=1 waits for the update as before).
        auto t0 = std::chrono::steady_clock::now();
        if (wait_update) { SH_TRY(slamhip_hs_update_by_scan(p->hs, p->match_pose)); }   // :112
        else { SH_TRY(hs_update_enqueue(p->hs, p->match_pose)); }
        const float ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        p->update_timing = (3.0f * p->update_timing + ms) / 4.0f;         // :115
        memcpy(p->last_update_pose, p->match_pose, sizeof(float) * 3);    // :118
        updated = 1;                                                      // :122
    }
    p->upd_hist = (p->upd_hist << 1) | (unsigned)updated;
    if (out_updated) *out_updated = updated;
    return SLAMHIP_OK;
}

// slamhip_hs_shift of the processor's own hs with the stored poses, kept in the window's frame, re-based: the one place where the
// scroll and slamhip_hsproc_shift move the window.  All in binary32, one rounding per operation.
static void hsproc_rebase(slamhip_hsproc *p, int32_t dx, int32_t dy)
{
    const int32_t q[2] = { dx, dy };
    for (int a = 0; a < 2; a++) {
        const float m = (float)q[a] * p->hs->lv[0].cell;                   // (the product is rounded, then the difference)
        p->match_pose[a] = p->match_pose[a] - m;
        p->last_update_pose[a] = p->last_update_pose[a] - m;               // (float.MinValue absorbs it: "never updated" survives)
    }
}
static int32_t hsproc_shift_rebase(slamhip_hsproc *p, int32_t dx, int32_t dy)
{
    SH_TRY(slamhip_hs_shift(p->hs, dx, dy));
    hsproc_rebase(p, dx, dy);
    return SLAMHIP_OK;
}

// The scrolling window (slamhip_hsproc_set_scroll), at the end of an Update: the match pose is on the host and this scan's grid
// update -- gated or not -- is enqueued, with the pose it reads in device memory in THIS scan's window frame; the shift goes
// behind it on the same stream.  Nothing is enqueued ahead for the next scan: its match and update take the cell pointers and
// the hint when they are enqueued, after the swap and the re-base below.  All in binary32, one rounding per operation.
static int32_t hsproc_scroll(slamhip_hsproc *p)
{
    slamhip_hs *hs = p->hs;
    const hs_level &L0 = hs->lv[0];
    const int g = 1 << (hs->n_levels - 1);
    const float cf[2] = { floorf(p->match_pose[0] * L0.stm), floorf(p->match_pose[1] * L0.stm) };
    if (!(fabsf(cf[0]) < 1.0e9f && fabsf(cf[1]) < 1.0e9f)) return SLAMHIP_OK;    // (a pose that is no number or nowhere near any map moves nothing)
    const int c[2] = { (int)cf[0], (int)cf[1] };
    const int half[2] = { L0.w / 2, L0.h / 2 };
    int q[2];
    for (int a = 0; a < 2; a++) {
        const int d = c[a] - half[a];
        q[a] = (d > p->scroll_trigger || -d > p->scroll_trigger) ? (d / g) * g : 0;   // (C division: toward zero)
    }
    if (q[0] == 0 && q[1] == 0) return SLAMHIP_OK;
    return hsproc_shift_rebase(p, q[0], q[1]);
}

extern "C" int32_t slamhip_hsproc_update(slamhip_hsproc *p, const float *xy, int32_t n, const float origin[2],
                                         const float hint[3], int32_t map_without_matching, int32_t *out_updated)
{
    SH_CHECK_ARG(p && hint);
    if (p->hs->win_ox == 0 && p->hs->win_oy == 0 && p->scroll_trigger == 0)
        return hsproc_update_window(p, xy, n, origin, hint, map_without_matching, out_updated);
    float off[2];
    hsproc_window_offset(p, off);
    const float hint_w[3] = { hint[0] - off[0], hint[1] - off[1], hint[2] };       // poses cross the C-ABI in the world frame
    SH_TRY(hsproc_update_window(p, xy, n, origin, hint_w, map_without_matching, out_updated));
    return p->scroll_trigger > 0 ? hsproc_scroll(p) : SLAMHIP_OK;
}

extern "C" int32_t slamhip_hsproc_set_scroll(slamhip_hsproc *p, int32_t trigger_cells)
{
    SH_CHECK_ARG(p);
    const hs_level &L0 = p->hs->lv[0];
    const int g = 1 << (p->hs->n_levels - 1);
    const int lim = (L0.w < L0.h ? L0.w : L0.h) / 2 - g;
    if (trigger_cells < 0 || trigger_cells >= lim)
        SH_FAIL(SLAMHIP_ERR_INVALID, "slamhip_hsproc_set_scroll: trigger_cells = %d is outside [0, min(w0, h0) / 2 - g) = [0, %d)", trigger_cells, lim > 0 ? lim : 0);
    p->scroll_trigger = trigger_cells;                                    // (read at the end of the next slamhip_hsproc_update)
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hsproc_get_origin(slamhip_hsproc *p, int64_t *ox, int64_t *oy)
{
    SH_CHECK_ARG(p);
    return slamhip_hs_origin(p->hs, ox, oy);
}

// slamhip_hs_shift from outside an Update, the poses re-based as the scroll re-bases them
extern "C" int32_t slamhip_hsproc_shift(slamhip_hsproc *p, int32_t dx, int32_t dy)
{
    SH_CHECK_ARG(p);
    return hsproc_shift_rebase(p, dx, dy);
}

// Relocalise in the window: the scan set, the lattice's centre taken to the window's frame as slamhip_hsproc_update takes its hint,
// the result brought back as slamhip_hsproc_get brings the stored poses back.  No scroll, no grid update.
extern "C" int32_t slamhip_hsproc_relocalise(slamhip_hsproc *p, const float *xy, int32_t n, const float origin[2], const slamhip_lattice_spec *spec_world,
                                             int32_t B, int32_t adopt, float out_pose_world[3], slamhip_match_report *out_report, slamhip_reloc_info *out_info)
{
    SH_CHECK_ARG(p && spec_world && out_pose_world && out_report && out_info && (adopt == 0 || adopt == 1));
    SH_TRY(slamhip_hs_set_scan(p->hs, xy, n, origin));
    slamhip_lattice_spec S = *spec_world;
    hsproc_pose_to_window(p, spec_world->centre, S.centre);
    float m[3];
    SH_TRY(slamhip_hs_relocalise(p->hs, &S, B, m, out_report, out_info));
    if (adopt) {
        memcpy(p->match_pose, m, sizeof(m));
        memcpy(p->last_update_pose, m, sizeof(m));
    }
    hsproc_pose_to_world(p, m, out_pose_world);
    return SLAMHIP_OK;
}

// Relocalise in the world: as above, but the window moves to the winner (slamhip_hs_relocalise_world) and the stored poses with it.
extern "C" int32_t slamhip_hsproc_relocalise_world(slamhip_hsproc *p, const float *xy, int32_t n, const float origin[2], const slamhip_lattice_spec *spec_world,
                                                   int32_t B, int32_t adopt, float out_pose_world[3], slamhip_match_report *out_report,
                                                   slamhip_world_reloc_info *out_info)
{
    SH_CHECK_ARG(p && spec_world && out_pose_world && out_report && out_info && (adopt == 0 || adopt == 1));
    SH_TRY(slamhip_hs_set_scan(p->hs, xy, n, origin));
    slamhip_lattice_spec S = *spec_world;
    hsproc_pose_to_window(p, spec_world->centre, S.centre);
    float m[3];
    memset(out_info, 0, sizeof(*out_info));
    const int32_t rc = slamhip_hs_relocalise_world(p->hs, &S, B, m, out_report, out_info);
    hsproc_rebase(p, out_info->dx, out_info->dy);                          // (the stored poses follow the window, also if the match behind the shift failed)
    SH_TRY(rc);
    if (adopt) {
        memcpy(p->match_pose, m, sizeof(m));
        memcpy(p->last_update_pose, m, sizeof(m));
    }
    hsproc_pose_to_world(p, m, out_pose_world);                            // (the window's new frame)
    return SLAMHIP_OK;
}

// The two calls above with the branch-and-bound search (K24) in place of the exhaustive one: world = 0 follows the first, world = 1 the second.
extern "C" int32_t slamhip_hsproc_relocalise_bnb(slamhip_hsproc *p, const float *xy, int32_t n, const float origin[2], const slamhip_bnb_spec *spec_world,
                                                 int32_t B, int32_t adopt, float out_pose_world[3], slamhip_match_report *out_report, void *out_info,
                                                 slamhip_bnb_info *out_bnb)
{
    SH_CHECK_ARG(p && spec_world && out_pose_world && out_report && out_info && out_bnb && (adopt == 0 || adopt == 1));
    SH_CHECK_ARG(spec_world->world == 0 || spec_world->world == 1);
    SH_TRY(slamhip_hs_set_scan(p->hs, xy, n, origin));
    slamhip_bnb_spec S = *spec_world;
    hsproc_pose_to_window(p, spec_world->lattice.centre, S.lattice.centre);
    float m[3];
    if (S.world) {
        slamhip_world_reloc_info *info = (slamhip_world_reloc_info *)out_info;
        memset(info, 0, sizeof(*info));
        const int32_t rc = slamhip_hs_relocalise_bnb(p->hs, &S, B, m, out_report, info, out_bnb);
        hsproc_rebase(p, info->dx, info->dy);                              // (the stored poses follow the window, also if the match behind the shift failed)
        SH_TRY(rc);
    } else SH_TRY(slamhip_hs_relocalise_bnb(p->hs, &S, B, m, out_report, out_info, out_bnb));
    if (adopt) {
        memcpy(p->match_pose, m, sizeof(m));
        memcpy(p->last_update_pose, m, sizeof(m));
    }
    hsproc_pose_to_world(p, m, out_pose_world);
    return SLAMHIP_OK;
}

// The beam trace at world poses: the scan set, every pose taken to the window's frame as slamhip_hsproc_relocalise takes its centre.
// Nothing of the processor's own state is read or written beyond the window's origin.
extern "C" int32_t slamhip_hsproc_trace(slamhip_hsproc *p, const float *xy, int32_t n, const float origin[2], const float *poses_world, int32_t B,
                                        int32_t level, int32_t world, slamhip_trace_summary *out_summaries, slamhip_trace_beam *out_beams)
{
    SH_CHECK_ARG(p && poses_world && out_summaries);
    // (what slamhip_hs_trace refuses for its arguments alone, ahead of the scan: a refused call leaves the scan that was set)
    SH_TRY(hs_trc_check(p->hs->n_levels, level, B, world, out_beams != nullptr, n, false));
    SH_TRY(slamhip_hs_set_scan(p->hs, xy, n, origin));
    std::vector<float> buf;
    return slamhip_hs_trace(p->hs, level, hsproc_poses_to_window(p, poses_world, B, buf), B, world, out_summaries, out_beams);
}

// The end-point distance score at world poses: slamhip_hsproc_trace's shape -- the arguments checked ahead of the scan, the scan
// set, every pose taken to the window's frame.
extern "C" int32_t slamhip_hsproc_distance_score(slamhip_hsproc *p, const float *xy, int32_t n, const float origin[2], const float *poses_world, int32_t B,
                                                 int32_t level, int32_t world, int32_t site_mask, int32_t radius,
                                                 slamhip_distance_summary *out_summaries, uint16_t *out_points)
{
    SH_CHECK_ARG(p && poses_world && out_summaries);
    // (what slamhip_hs_distance_score refuses for its arguments alone, ahead of the scan: a refused call leaves the scan that was set)
    SH_TRY(hs_df_check_score("distance score", p->hs->n_levels, level, world, site_mask, radius, B, out_points != nullptr, n, false));
    SH_TRY(slamhip_hs_set_scan(p->hs, xy, n, origin));
    std::vector<float> buf;
    return slamhip_hs_distance_score(p->hs, level, world, site_mask, radius, hsproc_poses_to_window(p, poses_world, B, buf), B, out_summaries, out_points);
}

// The scan-to-map pairs at world poses: slamhip_hsproc_distance_score's shape.  The summaries' cell sums stay in the window's frame.
extern "C" int32_t slamhip_hsproc_nearest_pairs(slamhip_hsproc *p, const float *xy, int32_t n, const float origin[2], const float *poses_world, int32_t B,
                                                int32_t level, int32_t world, int32_t site_mask, int32_t radius,
                                                slamhip_pair_summary *out_summaries, int16_t *out_pairs)
{
    SH_CHECK_ARG(p && poses_world && out_summaries);
    // (what slamhip_hs_nearest_pairs refuses for its arguments alone, ahead of the scan: a refused call leaves the scan that was set)
    SH_TRY(hs_nr_check_pairs(p->hs->n_levels, level, world, site_mask, radius, B, out_pairs != nullptr, n, false));
    SH_TRY(slamhip_hs_set_scan(p->hs, xy, n, origin));
    std::vector<float> buf;
    return slamhip_hs_nearest_pairs(p->hs, level, world, site_mask, radius, hsproc_poses_to_window(p, poses_world, B, buf), B, out_summaries, out_pairs);
}

// The frontier clusters in WORLD cells of the level: slamhip_hs_frontiers, the label rectangle taken to the window's frame and every
// cell field of the results taken back ((origin >> level) per axis; the window's origin is a multiple of 1 << (n_levels - 1)).
extern "C" int32_t slamhip_hsproc_frontiers(slamhip_hsproc *p, int32_t level, int32_t world, int32_t min_cells, int32_t max_clusters,
                                            slamhip_frontier_summary *out_summary, slamhip_frontier_cluster *out_clusters,
                                            int32_t lx, int32_t ly, int32_t lw, int32_t lh, int32_t *out_labels)
{
    SH_CHECK_ARG(p && out_summary);
    if (level < 0 || level >= p->hs->n_levels) SH_FAIL(SLAMHIP_ERR_INVALID, "frontiers: level %d of %d", level, p->hs->n_levels);
    const int64_t ox = p->hs->win_ox >> level, oy = p->hs->win_oy >> level;
    slamhip_frontier_summary S;
    memset(&S, 0, sizeof(S));
    const int32_t rc = slamhip_hs_frontiers(p->hs, level, world, min_cells, max_clusters, &S, out_clusters, hsproc_cell_to_window(lx, ox),
                                            hsproc_cell_to_window(ly, oy), lw, lh, out_labels);
    if (S.mw > 0) { S.mx0 += (int32_t)ox; S.my0 += (int32_t)oy; *out_summary = S; }   // (filled also when too many clusters are kept; a refused call writes nothing)
    SH_TRY(rc);
    for (int i = 0; i < S.n_returned; i++) {
        slamhip_frontier_cluster *c = out_clusters + i;
        c->seed_x += (int32_t)ox; c->x_min += (int32_t)ox; c->x_max += (int32_t)ox; c->sum_x += (int64_t)c->n_cells * ox;
        c->seed_y += (int32_t)oy; c->y_min += (int32_t)oy; c->y_max += (int32_t)oy; c->sum_y += (int64_t)c->n_cells * oy;
    }
    return SLAMHIP_OK;
}

// The cost-to-go field in WORLD cells of the level: slamhip_hs_nav_field with sources, goals and the rectangle taken to the window's
// frame ((origin >> level) per axis, clamped where a cell lies too far out to be a cell of M anyway) and the results taken back.
extern "C" int32_t slamhip_hsproc_nav_field(slamhip_hsproc *p, const slamhip_nav_spec *spec, const int32_t *sources, int32_t S, const int32_t *goals,
                                            int32_t G, slamhip_nav_goal_result *out_goal_results, int32_t n_paths, int32_t max_path_cells,
                                            slamhip_nav_path *out_paths, int32_t *out_path_cells, int32_t rx, int32_t ry, int32_t rw, int32_t rh,
                                            uint32_t *out_cost, uint8_t *out_dir, slamhip_nav_summary *out_summary)
{
    SH_CHECK_ARG(p && spec && out_summary);
    if (spec->level < 0 || spec->level >= p->hs->n_levels) SH_FAIL(SLAMHIP_ERR_INVALID, "navigation field: level %d of %d", spec->level, p->hs->n_levels);
    const int64_t ox = p->hs->win_ox >> spec->level, oy = p->hs->win_oy >> spec->level;
    if (ox == 0 && oy == 0)
        return slamhip_hs_nav_field(p->hs, spec, sources, S, goals, G, out_goal_results, n_paths, max_path_cells, out_paths, out_path_cells, rx, ry, rw,
                                    rh, out_cost, out_dir, out_summary);
    // (the counts are checked by slamhip_hs_nav_field; here they only bound the copies)
    const size_t ns = (sources && S >= 1 && S <= 4096) ? (size_t)S : 0, ng = (goals && G >= 1 && G <= 4096) ? (size_t)G : 0;
    std::vector<int32_t> w(2 * ns + 4 * ng);
    for (size_t i = 0; i < ns; i++) { w[2 * i] = hsproc_cell_to_window(sources[2 * i], ox); w[2 * i + 1] = hsproc_cell_to_window(sources[2 * i + 1], oy); }
    int32_t *wg = w.data() + 2 * ns;
    for (size_t i = 0; i < 4 * ng; i++) wg[i] = hsproc_cell_to_window(goals[i], (i & 1) ? oy : ox);   // (monotonic: an inverted rectangle stays inverted or becomes empty outside M)
    for (size_t i = 0; i < ng; i++)
        if (goals[4 * i] > goals[4 * i + 2] || goals[4 * i + 1] > goals[4 * i + 3]) { wg[4 * i] = 1; wg[4 * i + 2] = 0; }   // (refused below, as given)
    slamhip_nav_summary Sm;
    SH_TRY(slamhip_hs_nav_field(p->hs, spec, ns ? w.data() : sources, S, ng ? wg : goals, G, out_goal_results, n_paths, max_path_cells, out_paths,
                                out_path_cells, hsproc_cell_to_window(rx, ox), hsproc_cell_to_window(ry, oy), rw, rh, out_cost, out_dir, &Sm));
    Sm.mx0 += (int32_t)ox; Sm.my0 += (int32_t)oy;
    *out_summary = Sm;
    for (int i = 0; i < G; i++)
        if (out_goal_results[i].cost != SLAMHIP_NAV_UNREACHED) { out_goal_results[i].bx += (int32_t)ox; out_goal_results[i].by += (int32_t)oy; }
    for (int i = 0; i < n_paths; i++)
        for (int k = 0; k < out_paths[i].n_written; k++) {
            out_path_cells[2 * ((size_t)i * max_path_cells + k)] += (int32_t)ox;
            out_path_cells[2 * ((size_t)i * max_path_cells + k) + 1] += (int32_t)oy;
        }
    return SLAMHIP_OK;
}

// The command rollouts in WORLD cells and the WORLD pose: slamhip_hs_rollouts with the sources taken to the window's frame as
// slamhip_hsproc_nav_field takes them, the start pose as slamhip_hsproc_trace takes its poses (NULL: MatchPose, which is kept in the
// window's frame), and M and the results' poses taken back.  With the origin at (0, 0) every bit passes through.
extern "C" int32_t slamhip_hsproc_rollouts(slamhip_hsproc *p, const slamhip_nav_spec *spec, const int32_t *sources, int32_t S,
                                           const float *start_pose_world, float dt, const float *body, int32_t P, const float *cmds, int32_t B,
                                           int32_t n_cmd, int32_t hold, slamhip_rollout_result *out_results, slamhip_rollout_summary *out_summary)
{
    SH_CHECK_ARG(p && spec && out_summary);
    if (spec->level < 0 || spec->level >= p->hs->n_levels) SH_FAIL(SLAMHIP_ERR_INVALID, "navigation field: level %d of %d", spec->level, p->hs->n_levels);
    const int64_t ox = p->hs->win_ox >> spec->level, oy = p->hs->win_oy >> spec->level;
    float start[3];
    if (!start_pose_world) memcpy(start, p->match_pose, sizeof(start));
    else hsproc_pose_to_window(p, start_pose_world, start);
    if (!hsproc_moved(p)) return slamhip_hs_rollouts(p->hs, spec, sources, S, start, dt, body, P, cmds, B, n_cmd, hold, out_results, out_summary);
    const size_t ns = (sources && S >= 1 && S <= 4096) ? (size_t)S : 0;    // (the count is checked by slamhip_hs_rollouts; here it only bounds the copy)
    std::vector<int32_t> w(2 * ns);
    for (size_t i = 0; i < ns; i++) { w[2 * i] = hsproc_cell_to_window(sources[2 * i], ox); w[2 * i + 1] = hsproc_cell_to_window(sources[2 * i + 1], oy); }
    slamhip_rollout_summary Sm;
    SH_TRY(slamhip_hs_rollouts(p->hs, spec, ns ? w.data() : sources, S, start, dt, body, P, cmds, B, n_cmd, hold, out_results, &Sm));
    Sm.nav.mx0 += (int32_t)ox; Sm.nav.my0 += (int32_t)oy;
    *out_summary = Sm;
    static_assert(offsetof(slamhip_rollout_result, theta) == offsetof(slamhip_rollout_result, x) + 2 * sizeof(float), "x, y, theta: a pose");
    for (int i = 0; i < B; i++) hsproc_pose_to_world(p, &out_results[i].x, &out_results[i].x);
    return SLAMHIP_OK;
}

// The localisation step through the processor: the scan set as slamhip_hsproc_relocalise sets it, then slamhip_hs_mcl_step.  What
// that call refuses for its spec, the particle set or the scan's size is refused ahead of the scan: such a call leaves the scan that
// was set.
extern "C" int32_t slamhip_hsproc_mcl_step(slamhip_hsproc *p, const float *xy, int32_t n, const float origin[2], const slamhip_mcl_spec *spec,
                                           slamhip_mcl_summary *out)
{
    SH_CHECK_ARG(p && spec && out);
    SH_TRY(hs_mcl_check_step(p->hs, spec, n, false));
    SH_TRY(slamhip_hs_set_scan(p->hs, xy, n, origin));
    return slamhip_hs_mcl_step(p->hs, spec, out);
}

// The merge through the processor: the source as given, the poses taken to the window's frame as slamhip_hsproc_trace takes its poses.
// What the hs calls refuse for their arguments is refused ahead of the conversion.
extern "C" int32_t slamhip_hsproc_merge_set_source(slamhip_hsproc *p, int32_t level, int32_t ax, int32_t ay, int32_t w, int32_t h, const slamhip_cell *cells)
{
    SH_CHECK_ARG(p);
    return slamhip_hs_merge_set_source(p->hs, level, ax, ay, w, h, cells);
}

extern "C" int32_t slamhip_hsproc_merge_score(slamhip_hsproc *p, const float *poses_world, int32_t B, slamhip_merge_report *out_reports)
{
    SH_CHECK_ARG(p && poses_world && out_reports);
    SH_TRY(hs_merge_check_score(p->hs, B));
    std::vector<float> buf;
    return slamhip_hs_merge_score(p->hs, hsproc_poses_to_window(p, poses_world, B, buf), B, out_reports);
}

extern "C" int32_t slamhip_hsproc_merge_apply(slamhip_hsproc *p, const float pose_world[3], int32_t rule, float value_limit, slamhip_merge_report *out_report)
{
    SH_CHECK_ARG(p && pose_world && out_report);
    float pose[3];
    hsproc_pose_to_window(p, pose_world, pose);
    return slamhip_hs_merge_apply(p->hs, pose, rule, value_limit, out_report);
}

// The Hough transform through the processor: cells and bins, no pose to convert -- the calls of the processor's own hs as they are
extern "C" int32_t slamhip_hsproc_hough(slamhip_hsproc *p, int32_t level, int32_t slot, int32_t world, int32_t site_mask, int32_t T, int32_t q,
                                        int32_t out_info[7], uint64_t *out_spectrum, uint32_t *out_H)
{
    SH_CHECK_ARG(p);
    return slamhip_hs_hough(p->hs, level, slot, world, site_mask, T, q, out_info, out_spectrum, out_H);
}

extern "C" int32_t slamhip_hsproc_hough_rotation(slamhip_hsproc *p, uint64_t *out_cc)
{
    SH_CHECK_ARG(p);
    return slamhip_hs_hough_rotation(p->hs, out_cc);
}

extern "C" int32_t slamhip_hsproc_hough_shifts(slamhip_hsproc *p, const int32_t *pairs, int32_t P, slamhip_hough_shift *out_shifts, uint64_t *out_xc)
{
    SH_CHECK_ARG(p);
    return slamhip_hs_hough_shifts(p->hs, pairs, P, out_shifts, out_xc);
}

// The scan signatures through the processor: the scan set as slamhip_hsproc_relocalise sets it -- what the hs call refuses for its
// arguments or the store's state ahead of it: a refused call leaves the scan that was set -- then the call of the processor's own hs.
// The pose is the caller's WORLD pose, stored as given.
extern "C" int32_t slamhip_hsproc_sig_add(slamhip_hsproc *p, const float *xy, int32_t n, const float origin[2], const float pose_world[3], int32_t *out_index,
                                          uint64_t *out_sig, slamhip_sig_info *out_info)
{
    SH_CHECK_ARG(p && pose_world);
    SH_TRY(hs_sg_check_add(p->hs));
    SH_TRY(slamhip_hs_set_scan(p->hs, xy, n, origin));
    return slamhip_hs_sig_add(p->hs, pose_world, out_index, out_sig, out_info);
}

extern "C" int32_t slamhip_hsproc_sig_query(slamhip_hsproc *p, const float *xy, int32_t n, const float origin[2], int32_t first, int32_t last, int32_t B,
                                            slamhip_sig_hit *out_hits, int32_t *out_n, uint64_t *out_sig, slamhip_sig_info *out_info)
{
    SH_CHECK_ARG(p && out_hits && out_n);
    SH_TRY(hs_sg_check_query(p->hs, first, last, B));
    SH_TRY(slamhip_hs_set_scan(p->hs, xy, n, origin));
    return slamhip_hs_sig_query(p->hs, first, last, B, out_hits, out_n, out_sig, out_info);
}

extern "C" int32_t slamhip_hsproc_sig_self(slamhip_hsproc *p, int32_t first, int32_t last, int32_t min_gap, slamhip_sig_hit *out_hits)
{
    SH_CHECK_ARG(p);
    return slamhip_hs_sig_self(p->hs, first, last, min_gap, out_hits);
}

// The scan store and the render through the processor: the scan that is set on the processor's own hs appended; the render's WORLD
// poses taken to the window's frame.  Nothing of the processor's own state is read or written beyond the window's origin.
extern "C" int32_t slamhip_hsproc_scans_add(slamhip_hsproc *p, int32_t *out_index)
{
    SH_CHECK_ARG(p);
    return slamhip_hs_scans_add(p->hs, nullptr, 0, nullptr, out_index);
}

extern "C" int32_t slamhip_hsproc_scans_match(slamhip_hsproc *p, const slamhip_scanmatch_spec *spec, const slamhip_scan_pair *pairs, int32_t n_pairs,
                                              slamhip_scanmatch_result *out_results)
{
    SH_CHECK_ARG(p);
    return slamhip_hs_scans_match(p->hs, spec, pairs, n_pairs, out_results);   // (relative poses: no frame to convert)
}

extern "C" int32_t slamhip_hsproc_render(slamhip_hsproc *p, int32_t first, int32_t last, const float *poses_world, int32_t flags)
{
    SH_CHECK_ARG(p);
    std::vector<float> buf;
    int32_t count = 0;
    SH_TRY(slamhip_hs_scans_count(p->hs, &count));
    // (a range outside the store reads no pose here: slamhip_hs_render refuses it without touching the caller's array)
    const bool have = poses_world && first >= 0 && last > first && last <= count;
    return slamhip_hs_render(p->hs, first, last, have ? hsproc_poses_to_window(p, poses_world, last - first, buf) : poses_world, flags);
}

extern "C" int32_t slamhip_hsproc_render_world(slamhip_hsproc *p, int32_t first, int32_t last, const float *poses_world, int32_t flags)
{
    SH_CHECK_ARG(p);
    std::vector<float> buf;
    int32_t count = 0;
    SH_TRY(slamhip_hs_scans_count(p->hs, &count));
    const bool have = poses_world && first >= 0 && last > first && last <= count;      // (as slamhip_hsproc_render)
    return slamhip_hs_render_world(p->hs, first, last, have ? hsproc_poses_to_window(p, poses_world, last - first, buf) : poses_world, flags);
}

// The view gain through the processor: slamhip_hsproc_trace's shape -- the arguments checked ahead of the scan, the scan set, every
// pose taken to the window's frame.
extern "C" int32_t slamhip_hsproc_view_gain(slamhip_hsproc *p, const float *xy, int32_t n, const float origin[2], const float *poses_world, int32_t B,
                                            int32_t level, int32_t reach, int32_t commit, slamhip_view_summary *out_summaries)
{
    SH_CHECK_ARG(p && poses_world && out_summaries);
    SH_TRY(hs_view_check_gain(p->hs, level, reach, B, commit, n, false));
    SH_TRY(slamhip_hs_set_scan(p->hs, xy, n, origin));
    std::vector<float> buf;
    return slamhip_hs_view_gain(p->hs, level, reach, hsproc_poses_to_window(p, poses_world, B, buf), B, commit, out_summaries);
}

extern "C" int32_t slamhip_hsproc_view_select(slamhip_hsproc *p, const float *xy, int32_t n, const float origin[2], const float *poses_world, int32_t B,
                                              int32_t level, int32_t reach, int32_t mode, int32_t min_gain, int32_t k, int32_t *out_order,
                                              int32_t *out_gain, int32_t *out_n)
{
    SH_CHECK_ARG(p && poses_world && out_order && out_gain && out_n);
    SH_TRY(hs_view_check_select(p->hs, level, reach, mode, min_gain, B, k, n, false));
    SH_TRY(slamhip_hs_set_scan(p->hs, xy, n, origin));
    std::vector<float> buf;
    return slamhip_hs_view_select(p->hs, level, reach, mode, min_gain, hsproc_poses_to_window(p, poses_world, B, buf), B, k, out_order, out_gain, out_n);
}

extern "C" int32_t slamhip_hsproc_get(slamhip_hsproc *p, float match_pose[3], float last[3], float *mt, float *ut)
{
    SH_CHECK_ARG(p);
    if (match_pose) hsproc_pose_to_world(p, p->match_pose, match_pose);
    if (last) hsproc_pose_to_world(p, p->last_update_pose, last);
    if (mt) *mt = p->match_timing;
    if (ut) *ut = p->update_timing;
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hsproc_set_match_report(slamhip_hsproc *p, int32_t on)
{
    SH_CHECK_ARG(p && (on == 0 || on == 1));
    p->want_report = on;                                                  // (read by the next slamhip_hsproc_update)
    if (!on) p->report_valid = 0;
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hsproc_get_report(slamhip_hsproc *p, slamhip_match_report *out, int32_t *out_valid)
{
    SH_CHECK_ARG(p && out && out_valid);
    *out_valid = p->report_valid;
    if (p->report_valid) *out = p->report;
    else memset(out, 0, sizeof(*out));
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hsproc_set_thresholds(slamhip_hsproc *p, float min_dist, float min_angle)
{
    SH_CHECK_ARG(p);
    p->min_dist = min_dist; p->min_angle = min_angle;
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hsproc_hs(slamhip_hsproc *p, slamhip_hs **out)
{
    SH_CHECK_ARG(p && out);
    *out = p->hs;
    return SLAMHIP_OK;
}
