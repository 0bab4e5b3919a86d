// hs_render_world.hip -- K25, the stored scans drawn again into the WHOLE world behind the scrolling window: the window's arrays and the
// backing store's tiles (slamhip_hs_render_world, slamhip_debug_render_world).  Definition: include/slamhip.h.  The render is
// hs_render.h's, which K20 (hs_render.hip) shares -- the line, the boxes kernel, the body of the block kernel, the chunk frame, the
// hook's walk -- under the world bound instead of a level's w x h.  K25's own:
//  * the boxes are read back by the host BEFORE anything is changed: they say what is refused (a cell beyond the world bound, a line of
//    more than HS_LINE_MAX_DA cells) and which tiles the render needs.
//  * k25_render<B>: a workgroup per block of B x B world cells of one level, all levels in one grid, the work from a job table the
//    host writes.  B = min(T, 32): a block never leaves its tile, so a job names ONE slot, and the host's check of the table is a
//    division and a directory look-up per job (DESIGN.md section 4 "K25" weighs this against 32-cell blocks over several small
//    tiles).  The window is aligned to the shift granularity, not to tiles: a block may straddle its edge, so every cell's address is
//    chosen per cell -- inside the window's rectangle the window's arrays (the window wins, as in the world download), outside it the
//    tile's slot, cells then probabilities; the part of a tile under the window is neither read nor written.
#include "hs_render.h"
#include "hs_tiles.h"
#include <vector>

#define K25_BLOCK_MAX 32

// a block of B x B cells whose first is window-frame cell (x0, y0) of `level`, cell (lx0, ly0) of the tile whose slot is `slot`
// (nullptr: no cell of the block outside the window is drawn)
struct k25_job { unsigned char *slot; int32_t x0, y0; int32_t level; uint16_t lx0, ly0; uint64_t pad; };
static_assert(sizeof(k25_job) == 32, "a job is two 16-byte words");
struct k25_arg {
    hs_render_args<hs_box> P; hs_render_level lv[HS_MAX_LEVELS]; int T; const k25_job *jobs;       // lv: the window, cells (0, 0) .. (w - 1, h - 1)
    __device__ hs_bound_world bound(int) const { return {}; }              // (a level's w, h do not bound the world)
};

// where cell c of the job's block lives: the window's arrays inside the window's rectangle, else the tile's slot; false: nowhere
// (outside the window without a slot -- no line reaches such a cell, the host took a slot for every tile a box meets)
template <int B>
struct k25_cells {
    const hs_render_level &L; const k25_job &J; int T;
    __device__ __forceinline__ bool operator()(int c, slamhip_cell **cell, float **prob) const
    {
        const int cx = c & (B - 1), cy = c / B;
        const int X = J.x0 + cx, Y = J.y0 + cy;
        if ((unsigned)X < (unsigned)L.w && (unsigned)Y < (unsigned)L.h) {
            const size_t g = (size_t)Y * L.w + X;
            *cell = L.cells + g; *prob = L.prob + g;
            return true;
        }
        if (!J.slot) return false;
        const size_t g = (size_t)(J.ly0 + cy) * T + (J.lx0 + cx);          // (< T * T: the host checks lx0 + B <= T and ly0 + B <= T)
        *cell = (slamhip_cell *)J.slot + g;
        *prob = (float *)(J.slot + k6p_slot_prob_offset((size_t)T * T)) + g;
        return true;
    }
};

template <int B>
__global__ void __launch_bounds__(HS_RENDER_LANES) k25_render(const k25_arg A)
{
    const k25_job J = A.jobs[blockIdx.x];
    const hs_render_level &L = A.lv[J.level];
    hs_render_block<B>(A.P, J.level, L.base, A.bound(J.level), k25_cells<B>{ L, J, A.T }, J.x0, J.y0, J.x0 + B - 1, J.y0 + B - 1);
}

// ---- host side ---------------------------------------------------------------------------------------------------
// Tiles a render needs, as runs of one tile row: collected per box, then sorted and merged -- no table over the world, whose tile
// grid has up to 2^18 x 2^18 entries a level.
struct k25_run { int level; int64_t ty, tx0, tx1; };

static void k25_merge(std::vector<k25_run> &runs)
{
    std::sort(runs.begin(), runs.end(), [](const k25_run &a, const k25_run &b) {
        return a.level != b.level ? a.level < b.level : a.ty != b.ty ? a.ty < b.ty : a.tx0 < b.tx0;
    });
    size_t n = 0;
    for (const k25_run &r : runs) {
        if (n && runs[n - 1].level == r.level && runs[n - 1].ty == r.ty && r.tx0 <= runs[n - 1].tx1 + 1) runs[n - 1].tx1 = std::max(runs[n - 1].tx1, r.tx1);
        else runs[n++] = r;
    }
    runs.resize(n);
}

// the tile rows of the window-frame rectangle [x0, x1] x [y0, y1] of one level whose window cell (0, 0) is world cell (OX, OY)
static void k25_add_rect(std::vector<k25_run> &runs, int level, int64_t OX, int64_t OY, int x0, int y0, int x1, int y1, int T)
{
    const int64_t tx0 = bp_floor_div(OX + x0, T), tx1 = bp_floor_div(OX + x1, T);
    for (int64_t ty = bp_floor_div(OY + y0, T); ty <= bp_floor_div(OY + y1, T); ty++) runs.push_back({ level, ty, tx0, tx1 });
}

// What keeps the launch inside its arrays, checked against the handle and the directory, not against the code that wrote the table:
// a job's block lies in ONE tile, on the block grid; its slot is that tile's slot in the directory, or none.
static int32_t k25_check_jobs(const slamhip_hs *hs, const std::vector<k25_job> &jobs, int B)
{
    const hs_backing *bk = hs->bk;
    const int T = bk->T;
    for (const k25_job &j : jobs) {
        bool ok = j.level >= 0 && j.level < hs->n_levels && j.lx0 % B == 0 && j.ly0 % B == 0 && j.lx0 + B <= T && j.ly0 + B <= T &&
                  j.x0 >= -HS_WORLD_BOUND - 2 * T && j.x0 <= HS_WORLD_BOUND + 2 * T && j.y0 >= -HS_WORLD_BOUND - 2 * T && j.y0 <= HS_WORLD_BOUND + 2 * T;
        if (ok) {
            const int64_t X = (hs->win_ox >> j.level) + j.x0 - j.lx0, Y = (hs->win_oy >> j.level) + j.y0 - j.ly0;   // the tile's first world cell
            ok = bp_floor_div(X, T) * T == X && bp_floor_div(Y, T) * T == Y;
            if (ok && j.slot) ok = j.slot == bk->find(j.level, bp_floor_div(Y, T), bp_floor_div(X, T));
        }
        if (!ok) SH_FAIL(SLAMHIP_ERR_STATE, "slamhip_hs_render_world: the job table names a block outside its tile or a slot the directory does not hold (level %d)", j.level);
    }
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_render_world(slamhip_hs *hs, int32_t first, int32_t last, const float *poses, int32_t flags)
{
    SH_CHECK_ARG(hs);
    SH_TRY(hs_render_check("slamhip_hs_render_world", hs, first, last, poses, flags));
    if (!hs->bk)
        SH_FAIL(SLAMHIP_ERR_INVALID, "slamhip_hs_render_world: backing is off (slamhip_hs_set_backing) -- there is no world behind the window; "
                "slamhip_hs_render draws the window alone");
    SH_TRY(hs_render_check_cache("slamhip_hs_render_world", hs));
    if (last == first && (flags & SLAMHIP_RENDER_KEEP)) return SLAMHIP_OK;
    slamhip_ctx *ctx = hs->ctx;
    hs_backing *bk = hs->bk;
    hs_render_frame F;
    k25_arg A;
    SH_TRY(hs_render_begin(F, A, "slamhip_hs_render_world", hs, first, last, poses, flags));
    hs_scans *g = F.g;
    const bool keep = F.keep;
    const int N = F.N, NL = F.NL, chunk = F.chunk, T = bk->T, B = std::min(T, K25_BLOCK_MAX), per = T / B;
    A.T = T;

    // ---- pass 1: the boxes of the whole range, read back; nothing is changed ------------------------------------------------------
    SH_TRY(hs_render_lay(F, A.P, 0, true));                                // (the pinned block mirrors the device's: the boxes there are the ones read back)
    std::vector<k25_run> need;
    for (int c0 = 0; c0 < N; c0 += chunk) {
        const int nc = std::min(chunk, N - c0);
        SH_TRY(hs_render_stage(F, A, c0, nc));
        const hs_box *hb = (const hs_box *)(g->h_io + F.in_bytes);
        SH_HIP(hipMemcpyAsync((void *)hb, A.P.boxes, sizeof(hs_box) * (size_t)nc * NL, hipMemcpyDeviceToHost, ctx->stream));
        SH_TRY(hs_call_finish(hs));
        for (int k = 0; k < nc; k++)
            for (int l = 0; l < NL; l++) {
                const hs_box &b = hb[(size_t)k * NL + l];
                if (b.nv < 0)
                    SH_FAIL(SLAMHIP_ERR_INVALID, "slamhip_hs_render_world: scan %d has a begin or end cell beyond +-2^20 cells of the window's cell (0, 0) on level %d",
                            first + c0 + k, l);
                if (b.nv > 0 && b.da > HS_LINE_MAX_DA)
                    SH_FAIL(SLAMHIP_ERR_INVALID, "slamhip_hs_render_world: scan %d has a line of %d cells on level %d, more than %d", first + c0 + k, b.da, l, HS_LINE_MAX_DA);
                if (b.nv > 0) k25_add_rect(need, l, hs->win_ox >> l, hs->win_oy >> l, b.x0, b.y0, b.x1, b.y1, T);
            }
    }
    k25_merge(need);

    // ---- the plan: the tiles to take, the jobs; still nothing is changed ------------------------------------------------------------
    // the tiles wholly under the window on a level: [wtx0, wtx1] x [wty0, wty1], empty where the window holds no whole tile
    int64_t wtx0[HS_MAX_LEVELS], wtx1[HS_MAX_LEVELS], wty0[HS_MAX_LEVELS], wty1[HS_MAX_LEVELS];
    for (int l = 0; l < NL; l++) {
        const int64_t OX = hs->win_ox >> l, OY = hs->win_oy >> l;
        wtx0[l] = bp_floor_div(OX + T - 1, T); wtx1[l] = bp_floor_div(OX + hs->lv[l].w, T) - 1;
        wty0[l] = bp_floor_div(OY + T - 1, T); wty1[l] = bp_floor_div(OY + hs->lv[l].h, T) - 1;
    }
    auto under_window = [&](int l, int64_t ty, int64_t tx) { return tx >= wtx0[l] && tx <= wtx1[l] && ty >= wty0[l] && ty <= wty1[l]; };
    uint64_t need_tiles = 0, win_tiles = 0;
    for (const k25_run &r : need) need_tiles += (uint64_t)(r.tx1 - r.tx0 + 1);
    for (int l = 0; l < NL; l++) win_tiles += (uint64_t)(sh_div_up(hs->lv[l].w, T) + 1) * (uint64_t)(sh_div_up(hs->lv[l].h, T) + 1);
    if (need_tiles > win_tiles + bk->max_bytes / bk->slot_bytes)          // (the tiles outside the window alone pass the pool's capacity: no need to name them)
        SH_FAIL(SLAMHIP_ERR_NOMEM, "slamhip_hs_render_world: the render needs about %llu tiles of %zu bytes, more than max_bytes = %llu holds",
                (unsigned long long)need_tiles, bk->slot_bytes, (unsigned long long)bk->max_bytes);
    std::vector<hs_tile_key> take;                                         // the tiles to take, (level, ty, tx) ascending: the runs' own order
    for (const k25_run &r : need)
        for (int64_t tx = r.tx0; tx <= r.tx1; tx++)
            if (!under_window(r.level, r.ty, tx) && !(keep && bk->find(r.level, r.ty, tx))) take.push_back(hs_tile_key(r.level, r.ty, tx));
    size_t at_hand = bk->free_slots.size();
    if (!keep) { at_hand = 0; for (const hs_bk_chunk &c : bk->chunks) at_hand += c.slots; }     // (the directory goes: every slot of the pool is free again)
    std::vector<k25_run> runs = need;                                      // the tiles whose blocks run: the needed ones, and without KEEP the window's (the clear)
    if (!keep) {
        for (int l = 0; l < NL; l++) k25_add_rect(runs, l, hs->win_ox >> l, hs->win_oy >> l, 0, 0, hs->lv[l].w - 1, hs->lv[l].h - 1, T);
        k25_merge(runs);
    }
    uint64_t max_jobs = 0;
    for (const k25_run &r : runs) max_jobs += (uint64_t)(r.tx1 - r.tx0 + 1) * (uint64_t)(per * per);
    if (max_jobs > (uint64_t)INT32_MAX) SH_FAIL(SLAMHIP_ERR_INVALID, "slamhip_hs_render_world: %llu blocks in one render", (unsigned long long)max_jobs);
    SH_TRY(hs_render_lay(F, A.P, sizeof(k25_job) * (size_t)max_jobs, true));          // the jobs behind the boxes (the blocks' contents are gone: pass 2 stages every chunk again)
    A.jobs = (const k25_job *)((const unsigned char *)A.P.boxes + F.box_bytes);
    if (take.size() > at_hand) SH_TRY(hs_bk_reserve(hs, take.size() - at_hand));      // SLAMHIP_ERR_NOMEM: max_bytes, or a chunk's allocation -- the pool as it was

    // ---- from here on the world changes --------------------------------------------------------------------------------------------
    if (!keep) hs_bk_reset(hs);                                            // rule 1: the directory goes (in stream order, ahead of the launches)
    for (const hs_tile_key &t : take)
        if (!bk->find_or_take(hs, std::get<0>(t), std::get<1>(t), std::get<2>(t)))
            SH_FAIL(SLAMHIP_ERR_STATE, "slamhip_hs_render_world: the pool gave no slot behind its own reserve");
    std::vector<k25_job> jobs;
    jobs.reserve((size_t)max_jobs);
    for (const k25_run &r : runs) {
        const hs_level &L = hs->lv[r.level];
        const int64_t OX = hs->win_ox >> r.level, OY = hs->win_oy >> r.level;
        for (int64_t tx = r.tx0; tx <= r.tx1; tx++) {
            unsigned char *slot = under_window(r.level, r.ty, tx) ? nullptr : bk->find(r.level, r.ty, tx);
            for (int by = 0; by < per; by++)
                for (int bx = 0; bx < per; bx++) {
                    k25_job j;
                    memset(&j, 0, sizeof(j));
                    j.slot = slot; j.level = r.level; j.lx0 = (uint16_t)(bx * B); j.ly0 = (uint16_t)(by * B);
                    j.x0 = (int32_t)(tx * T - OX + bx * B); j.y0 = (int32_t)(r.ty * T - OY + by * B);
                    const bool meets_window = j.x0 < L.w && j.x0 + B > 0 && j.y0 < L.h && j.y0 + B > 0;
                    if (slot || meets_window) jobs.push_back(j);            // (neither: a block of a window tile outside the window, nothing to draw or clear)
                }
        }
    }
    SH_TRY(k25_check_jobs(hs, jobs, B));
    if (!jobs.empty()) {
        unsigned char *hj = g->h_io + F.in_bytes + F.box_bytes;
        memcpy(hj, jobs.data(), sizeof(k25_job) * jobs.size());
        SH_HIP(hipMemcpyAsync((void *)A.jobs, hj, sizeof(k25_job) * jobs.size(), hipMemcpyHostToDevice, ctx->stream));
    }
    return hs_render_chunks(F, A, [&](int) -> int32_t {
        if (jobs.empty()) return SLAMHIP_OK;
        const dim3 grid((unsigned)jobs.size()), lanes(HS_RENDER_LANES);
        if (B == 8) hipLaunchKernelGGL(k25_render<8>, grid, lanes, 0, ctx->stream, A);
        else if (B == 16) hipLaunchKernelGGL(k25_render<16>, grid, lanes, 0, ctx->stream, A);
        else hipLaunchKernelGGL(k25_render<32>, grid, lanes, 0, ctx->stream, A);
        SH_HIP(hipGetLastError());
        return SLAMHIP_OK;
    });
}

// ---- CPU-side test hook: the definition over caller arrays, as slamhip_debug_render (hs_line_walk over each level's rectangle), under
// the world bound; the first walk only looks (what is refused leaves the arrays as they were), the second draws. -------------------------
extern "C" int32_t slamhip_debug_render_world(int32_t n_levels, const int32_t *rects, float cell_length, slamhip_cell *cells, int32_t *update_index,
                                              int32_t *cache_index, float free_factor, float occ_factor, const float *xy, const int32_t *offsets,
                                              const float *origins, const float *poses, int32_t N, int32_t flags)
{
    SH_CHECK_ARG(rects && cells && update_index && cache_index && n_levels >= 1 && n_levels <= HS_MAX_LEVELS && cell_length > 0.0f && N >= 0 && N <= K20_MAX_SCANS);
    SH_CHECK_ARG(N == 0 || (offsets && origins && poses));
    for (int l = 0; l < n_levels; l++) {
        const int32_t *R = rects + 4 * l;
        SH_CHECK_ARG(R[2] >= 1 && R[3] >= 1 && (int64_t)R[2] * R[3] <= ((int64_t)1 << 26) && hs_world_cell_ok(R[0], R[1]) && hs_world_cell_ok(R[0] + R[2] - 1, R[1] + R[3] - 1));
    }
    SH_TRY(hs_render_check_offsets("render world", xy, offsets, N));
    SH_TRY(k20_check("render world", 0, N, N, poses, flags, update_index, n_levels));
    const float lo_free = hs_prob_to_logodds(free_factor), lo_occ = hs_prob_to_logodds(occ_factor);
    for (int draw = 0; draw < 2; draw++) {
        float res = cell_length;
        slamhip_cell *C = cells;
        for (int l = 0; l < n_levels; l++) {
            const int X0 = rects[4 * l], Y0 = rects[4 * l + 1], w = rects[4 * l + 2], h = rects[4 * l + 3];
            const float stm = 1.0f / res;                                  // MapProperties.cs:32, as slamhip_hs_create forms it
            int ui = update_index[l];
            if (draw && !(flags & SLAMHIP_RENDER_KEEP)) {
                for (size_t i = 0; i < (size_t)w * h; i++) C[i] = hs_reset_cell();
                ui = 0; cache_index[l] = 0;
            }
            for (int k = 0; k < N; k++) {
                const int mark_free = ui + 1, mark_occ = ui + 2;           // :116-117
                const sh_m3x2 M = k20_matrix(poses + 3 * (size_t)k, stm);
                int bx, by;
                hs_line_begin(origins[2 * k], origins[2 * k + 1], M, &bx, &by);
                if (!draw && offsets[k + 1] > offsets[k] && !hs_world_cell_ok(bx, by))
                    SH_FAIL(SLAMHIP_ERR_INVALID, "render world: scan %d's begin cell lies beyond +-2^20 cells on level %d", k, l);
                for (int i = offsets[k]; i < offsets[k + 1]; i++) {        // :130
                    int ex, ey;
                    const hs_line ln = hs_line_make(xy[2 * (size_t)i], xy[2 * (size_t)i + 1], M, bx, by, hs_bound_world{}, &ex, &ey);
                    if (!draw) {
                        if (!hs_world_cell_ok(ex, ey)) SH_FAIL(SLAMHIP_ERR_INVALID, "render world: point %d of scan %d ends beyond +-2^20 cells on level %d", i - offsets[k], k, l);
                        if (!(ln.flags & 1)) continue;
                        if (ln.da > HS_LINE_MAX_DA) SH_FAIL(SLAMHIP_ERR_INVALID, "render world: a line of %d cells in scan %d on level %d, more than %d", ln.da, k, l, HS_LINE_MAX_DA);
                        if (bx < X0 || by < Y0 || bx >= X0 + w || by >= Y0 + h || ex < X0 || ey < Y0 || ex >= X0 + w || ey >= Y0 + h)
                            SH_FAIL(SLAMHIP_ERR_INVALID, "render world: scan %d's box leaves the rectangle of level %d", k, l);
                        continue;
                    }
                    if (ln.flags & 1) hs_line_walk(C, w, X0, Y0, ln, bx, by, ex, ey, mark_free, mark_occ, lo_free, lo_occ);
                }
                ui += 3;                                                   // :144
                if (draw) cache_index[l]++;                                // :147
            }
            if (draw) update_index[l] = ui;
            C += (size_t)w * h;
            res *= 2.0f;                                                   // MapRepMultiMap.cs:56
        }
    }
    return SLAMHIP_OK;
}
