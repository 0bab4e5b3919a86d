// hs_merge.hip -- K14, the merge of a second map into the window of HectorSLAM under a rigid transform: a source map kept in
// device memory, candidate alignments rated without touching either map, and the source's evidence fused into one level at the
// chosen alignment (slamhip_hs_merge_set_source, _score, _apply, _clear_source, slamhip_debug_merge, slamhip_debug_merge_box).  No
// reference counterpart.  Definition: include/slamhip.h (slamhip_hs_merge_apply); the arithmetic host and device share: hs_merge.h.
//
//  * k14_pack_source, one launch per set_source: a lane per 16 cells of a source row reads the staged cells and stores their
//    Values as float[w * h] and their classes (hs_lat_class_bits) as one word of K7's layout -- 2 bits per cell, rows padded to
//    whole words, the padding zero.
//  * k14_score: the grid is (destination tiles, pose chunks).  A workgroup of four wavefronts owns a tile of 64 x 16 destination
//    cells -- a wavefront takes whole 64-cell row segments, rows wave, wave + 4, ... -- reads their classes once from K7's class map
//    of the level into registers and loops over K14_POSES poses.  Per pose: the tile box (hs_merge_box_of, the same bits in every
//    lane); a tile the box shows to be unsourced adds its cell count to n_unsourced and does nothing else; otherwise every lane forms
//    its cells' source cells and reads their class bits from the packed source (1 MB for a 2048^2 map: it stays in the L2), forms
//    3 * cd + cs, and the ten counts come from ballots and popcounts.  The wavefronts' counts meet in LDS; at the end of the chunk
//    ONE 64-bit agent-scope atomic add per workgroup, pose and counter that is not zero goes to the pose's report, which a memset
//    zeroed in-stream ahead of the launch.  Integers throughout: every order of the adds gives the same bits.
//  * k14_apply<TW, TH>: ONE launch over the window, a workgroup per tile of TW x TH destination cells, consecutive lanes consecutive
//    x, so the 8-byte cell reads and the cell and probability writes of a wavefront are whole row segments.  The tile box first: a
//    tile with no sourced cell leaves with one atomic add.  DIRECT, what runs by default: the gathers read the source in global
//    memory, bounds-checked by hs_merge_source_cell.  STAGED (the developer switch SLAMHIP_K14_STAGED): the box's source Values are
//    copied into LDS row by row (coalesced) and the gathers read LDS; a box that does not fit the LDS block takes the direct path.
//    Both paths run the same loop.  Measured (tools/hs_merge_bench.py, docs/EXPERIMENTS.md): staging does not win at any angle, so
//    it is not the default.  A cell is written -- Value and index as one 8-byte store, hs_prob_v(Value) beside it -- only where
//    its Value's bits change.  The twelve counts: ballots, the wavefronts' sums through LDS, one atomic add per workgroup and
//    counter that is not zero.
//    The tile is 64 x 32 (SLAMHIP_K14_TILE32: 32 x 32, measured slower at 2048^2).
#include "hs_blocks.h"
#include "hs_merge.h"
#include <stddef.h>
#include <vector>

#define K14_LANES 256
#define K14_SW 64                          // k14_score's tile
#define K14_SH 16
#define K14_POSES 16                       // poses a workgroup of k14_score loops over
#define K14_SCORE_CTRS 10                  // joint[9] and n_unsourced

static_assert(sizeof(slamhip_merge_report) == 96 && sizeof(slamhip_merge_report) == HS_MERGE_CTRS * sizeof(int64_t), "the record of include/slamhip.h");
static_assert(offsetof(slamhip_merge_report, n_unsourced) == HS_MERGE_C_UNSOURCED * 8 && offsetof(slamhip_merge_report, n_changed) == HS_MERGE_C_CHANGED * 8 &&
              offsetof(slamhip_merge_report, n_clamped) == HS_MERGE_C_CLAMPED * 8, "the counters' order");

typedef unsigned long long k14_u64;

__global__ void __launch_bounds__(256) k14_pack_source(const slamhip_cell *__restrict__ cells, int w, int h, int wpr, float *__restrict__ val,
                                                       uint32_t *__restrict__ cls)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= wpr * h) return;                                              // (w * h <= 2^26: wpr * h < 2^27)
    const int y = i / wpr, x0 = (i - y * wpr) * 16;
    const size_t row = (size_t)y * w;
    uint32_t word = 0;
#pragma unroll
    for (int b = 0; b < 16; b++)
        if (x0 + b < w) {
            const float v = cells[row + x0 + b].value;
            val[row + x0 + b] = v;
            word |= hs_lat_class_bits(v) << (2 * b);
        }
    cls[i] = word;
}

// the class bits of cell (x, y) of a packed map of rows of wpr words; the caller has checked the cell to lie in the map
__device__ static __forceinline__ uint32_t k14_class(const uint32_t *__restrict__ cls, int wpr, int x, int y)
{
    return (cls[(size_t)y * wpr + (x >> 4)] >> ((x & 15) * 2)) & 3u;
}

struct k14_score_arg {
    const uint32_t *dcls; int w, h, dwpr;  // K7's class map of the destination level (the window)
    const uint32_t *scls; int swpr;        // the packed source
    hs_merge_src S;
    const hs_merge_xf *xf; int B;          // the poses' constants (hs_merge_xf_of, formed on the host: the same text)
    int tiles_x;
    k14_u64 *rep;                          // B x HS_MERGE_CTRS
};

__global__ void __launch_bounds__(K14_LANES) k14_score(const k14_score_arg A)
{
    __shared__ int red_s[K14_LANES / 64][K14_POSES][K14_SCORE_CTRS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile_y = blockIdx.x / A.tiles_x, tile_x = blockIdx.x - tile_y * A.tiles_x;
    const int x0 = tile_x * K14_SW, y0 = tile_y * K14_SH;
    const int x1 = min(x0 + K14_SW - 1, A.w - 1), y1 = min(y0 + K14_SH - 1, A.h - 1);
    const int p0 = blockIdx.y * K14_POSES, np = min(K14_POSES, A.B - p0);
    constexpr int ROWS = K14_SH / (K14_LANES / 64);                        // rows of a wavefront
    const int x = x0 + lane;
    uint32_t cd[ROWS]; bool valid[ROWS];
    int n_valid = 0;                                                       // (of the wavefront)
#pragma unroll
    for (int k = 0; k < ROWS; k++) {
        const int y = y0 + wave + k * (K14_LANES / 64);
        valid[k] = x <= x1 && y <= y1;
        cd[k] = valid[k] ? k14_class(A.dcls, A.dwpr, x, y) : 0u;
        n_valid += (int)__popcll(__ballot(valid[k]));
    }
    for (int p = 0; p < np; p++) {
        const hs_merge_xf t = A.xf[p0 + p];                                // (uniform)
        int cnt[K14_SCORE_CTRS];
#pragma unroll
        for (int c = 0; c < K14_SCORE_CTRS; c++) cnt[c] = 0;
        hs_merge_box bx;
        if (!hs_merge_box_of(t, A.S, x0, y0, x1, y1, &bx)) cnt[HS_MERGE_C_UNSOURCED] = n_valid;
        else {
#pragma unroll
            for (int k = 0; k < ROWS; k++) {
                const int y = y0 + wave + k * (K14_LANES / 64);
                int su, sv, idx = -1;
                if (valid[k]) {
                    idx = HS_MERGE_C_UNSOURCED;
                    if (hs_merge_source_cell(t, A.S, x, y, &su, &sv)) idx = 3 * (int)cd[k] + (int)k14_class(A.scls, A.swpr, su, sv);
                }
#pragma unroll
                for (int c = 0; c < K14_SCORE_CTRS; c++) cnt[c] += (int)__popcll(__ballot(idx == c));
            }
        }
        if (lane == 0) {
#pragma unroll
            for (int c = 0; c < K14_SCORE_CTRS; c++) red_s[wave][p][c] = cnt[c];
        }
    }
    __syncthreads();
    for (int i = tid; i < np * K14_SCORE_CTRS; i += K14_LANES) {
        const int p = i / K14_SCORE_CTRS, c = i - p * K14_SCORE_CTRS;
        int v = 0;
        for (int wv = 0; wv < K14_LANES / 64; wv++) v += red_s[wv][p][c];
        if (v) __hip_atomic_fetch_add(A.rep + (size_t)(p0 + p) * HS_MERGE_CTRS + c, (k14_u64)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

struct k14_apply_arg {
    slamhip_cell *cells; float *prob; int w, h;   // the destination level
    const float *sval;                     // the source's Values
    hs_merge_src S;
    hs_merge_xf t;
    int rule; float limit;
    int direct;                            // 1: no staging; 0: SLAMHIP_K14_STAGED
    int tiles_x;
    k14_u64 *rep;                          // HS_MERGE_CTRS
};

// floats of the LDS block: the box of a TW x TH tile has at most ((TW - 1 + TH - 1) / sqrt 2 + 3)^2 cells -- 47^2 = 2209 for 32 x 32,
// 70^2 = 4900 for 64 x 32; a larger one (none is known) takes the direct path
template <int TW, int TH> struct k14_cap { static constexpr int floats = TW * TH <= 1024 ? 2560 : 5120; };

template <int TW, int TH>
__global__ void __launch_bounds__(K14_LANES) k14_apply(const k14_apply_arg A)
{
    constexpr int CAP = k14_cap<TW, TH>::floats;
    __shared__ float box_s[CAP];
    __shared__ int red_s[K14_LANES / 64][HS_MERGE_CTRS];
    const int tid = threadIdx.x;
    const int tile_y = blockIdx.x / A.tiles_x, tile_x = blockIdx.x - tile_y * A.tiles_x;
    const int x0 = tile_x * TW, y0 = tile_y * TH;
    const int x1 = min(x0 + TW - 1, A.w - 1), y1 = min(y0 + TH - 1, A.h - 1);
    hs_merge_box bx;
    if (!hs_merge_box_of(A.t, A.S, x0, y0, x1, y1, &bx)) {                 // (uniform over the workgroup)
        if (tid == 0)
            __hip_atomic_fetch_add(A.rep + HS_MERGE_C_UNSOURCED, (k14_u64)((x1 - x0 + 1) * (y1 - y0 + 1)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    const int bw = bx.u1 - bx.u0 + 1, bh = bx.v1 - bx.v0 + 1;              // (bw * bh <= w * h <= 2^26)
    const bool staged = !A.direct && bw * bh <= CAP;
    if (staged) {
        const float *src = A.sval + ((size_t)bx.v0 * A.S.w + bx.u0);
        for (int j = tid; j < bw * bh; j += K14_LANES) {
            const int r = j / bw;
            box_s[j] = src[(size_t)r * A.S.w + (j - r * bw)];
        }
        __syncthreads();
    }
    int cnt[HS_MERGE_CTRS];
#pragma unroll
    for (int c = 0; c < HS_MERGE_CTRS; c++) cnt[c] = 0;
#pragma unroll 1                                                           // (unrolled, the ballots' words and the twelve sums spill scalar registers)
    for (int k = 0; k < TW * TH / K14_LANES; k++) {
        const int j = tid + k * K14_LANES;
        const int x = x0 + (j % TW), y = y0 + (j / TW);
        const bool valid = x <= x1 && y <= y1;
        int idx = -1;
        bool changed = false, clamped = false;
        if (valid) {
            const size_t i = (size_t)y * A.w + x;
            slamhip_cell cell = A.cells[i];
            int su, sv;
            idx = HS_MERGE_C_UNSOURCED;
            if (hs_merge_source_cell(A.t, A.S, x, y, &su, &sv)) {
                // (staged: a sourced cell's source cell lies in the box -- hs_merge_box_of; tests/test_hs_merge_abi.py samples it)
                const float s = staged ? box_s[(sv - bx.v0) * bw + (su - bx.u0)] : A.sval[(size_t)sv * A.S.w + su];
                const uint32_t cd = hs_lat_class_bits(cell.value), cs = hs_lat_class_bits(s);
                idx = 3 * (int)cd + (int)cs;
                float t;
                if (hs_merge_rule(A.rule, A.limit, cell.value, s, cd, cs, &t, &clamped) && hs_merge_bits(t) != hs_merge_bits(cell.value)) {
                    changed = true;
                    cell.value = t;
                    A.cells[i] = cell;                                     // (the index as it was)
                    A.prob[i] = hs_prob_v(t);
                }
            }
        }
#pragma unroll
        for (int c = 0; c <= HS_MERGE_C_UNSOURCED; c++) cnt[c] += (int)__popcll(__ballot(idx == c));
        cnt[HS_MERGE_C_CHANGED] += (int)__popcll(__ballot(changed));
        cnt[HS_MERGE_C_CLAMPED] += (int)__popcll(__ballot(clamped));
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int c = 0; c < HS_MERGE_CTRS; c++) red_s[tid >> 6][c] = cnt[c];
    }
    __syncthreads();
    if (tid < HS_MERGE_CTRS) {
        int v = 0;
        for (int wv = 0; wv < K14_LANES / 64; wv++) v += red_s[wv][tid];
        if (v) __hip_atomic_fetch_add(A.rep + tid, (k14_u64)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------
// What the merge keeps, made by the first slamhip_hs_merge_set_source: the pinned and the device block a source's cells pass
// through, the source's Values and class words, and the blocks of the poses' constants and the reports of a score or an apply.
struct hs_merge {
    hs_block<slamhip_cell, HS_MEM_PINNED> h_stage;
    hs_block<slamhip_cell, HS_MEM_DEVICE> d_stage;
    hs_block<float, HS_MEM_DEVICE> d_val;
    hs_block<uint32_t, HS_MEM_DEVICE> d_cls;
    hs_block<hs_merge_xf, HS_MEM_DEVICE> d_xf;
    hs_block<k14_u64, HS_MEM_DEVICE> d_rep;
    hs_block<unsigned char, HS_MEM_PINNED> h_io;     // the reports; behind them the poses' constants
    bool have; int level, wpr;
    hs_merge_src S;
};

void hs_merge_drop_source(slamhip_hs *hs)
{
    if (hs->mrg) hs->mrg->have = false;
    hs_hg_drop_slot(hs, 1);                                                // (K17's slot 1 is the Hough transform of THIS source)
}

int32_t hs_merge_source_map(const slamhip_hs *hs, hs_class_map *M, int *level)
{
    const hs_merge *m = hs->mrg;
    if (!m || !m->have) SH_FAIL(SLAMHIP_ERR_STATE, "merge: no source (slamhip_hs_merge_set_source first)");
    M->cls = m->d_cls; M->w = m->S.w; M->h = m->S.h; M->wpr = m->wpr;
    M->x0 = m->S.ax; M->y0 = m->S.ay;
    *level = m->level;
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_merge_set_source(slamhip_hs *hs, int32_t level, int32_t ax, int32_t ay, int32_t w, int32_t h, const slamhip_cell *cells)
{
    SH_CHECK_ARG(hs && cells);
    if (level < 0 || level >= hs->n_levels) SH_FAIL(SLAMHIP_ERR_INVALID, "merge: level %d of %d", level, hs->n_levels);
    if (w < 1 || h < 1 || (int64_t)w * h > (int64_t)HS_MERGE_MAX_CELLS)
        SH_FAIL(SLAMHIP_ERR_INVALID, "merge: a source of %d x %d cells; both at least 1, at most 2^26 cells in all", w, h);
    if (ax < -HS_MERGE_MAX_ORIGIN || ax > HS_MERGE_MAX_ORIGIN || ay < -HS_MERGE_MAX_ORIGIN || ay > HS_MERGE_MAX_ORIGIN)
        SH_FAIL(SLAMHIP_ERR_INVALID, "merge: the source's first cell (%d, %d) lies more than 2^30 cells from its frame's origin", ax, ay);
    SH_TRY(hs_call_begin(hs));
    SH_TRY(hs_unit<&slamhip_hs::mrg>(hs));
    hs_merge *m = hs->mrg;
    m->have = false;                                                       // (no source until this one has landed)
    hs_hg_drop_slot(hs, 1);
    const size_t n = (size_t)w * h;
    const int wpr = (w + 15) / 16;
    // (the blocks are idle: every call waits for its own launches, and a call that timed out has poisoned the context)
    SH_TRY(m->h_stage.grow(sizeof(slamhip_cell) * n, "merge"));
    SH_TRY(m->d_stage.grow(sizeof(slamhip_cell) * n, "merge"));
    SH_TRY(m->d_val.grow(sizeof(float) * n, "merge"));
    SH_TRY(m->d_cls.grow(sizeof(uint32_t) * (size_t)wpr * h, "merge"));
    memcpy(m->h_stage, cells, sizeof(slamhip_cell) * n);
    hipStream_t st = hs->ctx->stream;
    SH_HIP(hipMemcpyAsync(m->d_stage, m->h_stage, sizeof(slamhip_cell) * n, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k14_pack_source, dim3((unsigned)sh_div_up(wpr * h, 256)), dim3(256), 0, st, (const slamhip_cell *)m->d_stage, w, h, wpr, m->d_val, m->d_cls);
    SH_HIP(hipGetLastError());
    SH_TRY(hs_call_finish(hs));
    m->level = level; m->wpr = wpr;
    m->S.ax = ax; m->S.ay = ay; m->S.w = w; m->S.h = h;
    m->have = true;
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_merge_clear_source(slamhip_hs *hs)
{
    SH_CHECK_ARG(hs);
    hs_merge_drop_source(hs);
    return SLAMHIP_OK;
}

int32_t hs_merge_check_score(const slamhip_hs *hs, int32_t B)
{
    if (B < 1 || B > HS_MERGE_MAX_POSES) SH_FAIL(SLAMHIP_ERR_INVALID, "merge: B = %d must lie in [1, %d]", B, HS_MERGE_MAX_POSES);
    if (!hs->mrg || !hs->mrg->have) SH_FAIL(SLAMHIP_ERR_STATE, "merge: no source (slamhip_hs_merge_set_source first)");
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_merge_score(slamhip_hs *hs, const float *poses, int32_t B, slamhip_merge_report *out_reports)
{
    SH_CHECK_ARG(hs && poses && out_reports);
    SH_TRY(hs_merge_check_score(hs, B));
    SH_TRY(hs_call_begin(hs));
    hs_merge *m = hs->mrg;
    const hs_level &L = hs->lv[m->level];
    hs_class_map M;
    SH_TRY(hs_lat_pack_prepare(hs, m->level, false, &M));
    const size_t rep_bytes = sizeof(slamhip_merge_report) * (size_t)B, xf_bytes = sizeof(hs_merge_xf) * (size_t)B;
    SH_TRY(m->d_xf.grow(xf_bytes, "merge"));
    SH_TRY(m->d_rep.grow(rep_bytes, "merge"));
    SH_TRY(m->h_io.grow(rep_bytes + xf_bytes, "merge"));
    hs_merge_xf *h_xf = (hs_merge_xf *)(m->h_io + rep_bytes);
    for (int i = 0; i < B; i++) h_xf[i] = hs_merge_xf_of(L.stm, poses[3 * i], poses[3 * i + 1], poses[3 * i + 2]);
    hipStream_t st = hs->ctx->stream;
    SH_HIP(hipMemcpyAsync(m->d_xf, h_xf, xf_bytes, hipMemcpyHostToDevice, st));
    SH_TRY(hs_lat_pack_enqueue(hs, m->level, false, &M));
    SH_HIP(hipMemsetAsync(m->d_rep, 0, rep_bytes, st));
    k14_score_arg A;
    A.dcls = M.cls; A.w = M.w; A.h = M.h; A.dwpr = M.wpr;
    A.scls = m->d_cls; A.swpr = m->wpr;
    A.S = m->S;
    A.xf = m->d_xf; A.B = B;
    A.tiles_x = sh_div_up(M.w, K14_SW);
    A.rep = m->d_rep;
    hipLaunchKernelGGL(k14_score, dim3((unsigned)(A.tiles_x * sh_div_up(M.h, K14_SH)), (unsigned)sh_div_up(B, K14_POSES)), dim3(K14_LANES), 0, st, A);
    SH_HIP(hipGetLastError());
    SH_HIP(hipMemcpyAsync(m->h_io, m->d_rep, rep_bytes, hipMemcpyDeviceToHost, st));
    SH_TRY(hs_call_finish(hs));
    memcpy(out_reports, m->h_io, rep_bytes);
    return SLAMHIP_OK;
}

int32_t hs_merge_check_apply(const slamhip_hs *hs, int32_t rule, float value_limit)
{
    if (rule < 0 || rule > 2) SH_FAIL(SLAMHIP_ERR_INVALID, "merge: rule = %d must be 0 (add), 1 (fill) or 2 (replace)", rule);
    if (!(isfinite(value_limit) && value_limit > 0.0f)) SH_FAIL(SLAMHIP_ERR_INVALID, "merge: value_limit = %g must be finite and above 0", value_limit);
    if (hs->ref_cache)
        SH_FAIL(SLAMHIP_ERR_INVALID, "slamhip_hs_merge_apply: the reference's cache is on (slamhip_hs_set_reference_cache) -- its literal stale entries have "
                "no meaning under an operation the reference lacks; turn it off first");
    if (!hs->mrg || !hs->mrg->have) SH_FAIL(SLAMHIP_ERR_STATE, "merge: no source (slamhip_hs_merge_set_source first)");
    return SLAMHIP_OK;
}

// the developer switches (tests, tools/hs_merge_bench.py): the tile box staged in LDS; the 32 x 32 tile.  Measured slower than the
// 64 x 32 tile with gathers from global memory (profiles/r20_hs_merge.json), which is what runs without them.
static bool k14_staged() { static const bool v = sh_env_set("SLAMHIP_K14_STAGED"); return v; }
static bool k14_tile32() { static const bool v = sh_env_set("SLAMHIP_K14_TILE32"); return v; }

extern "C" int32_t slamhip_hs_merge_apply(slamhip_hs *hs, const float pose[3], int32_t rule, float value_limit, slamhip_merge_report *out_report)
{
    SH_CHECK_ARG(hs && pose && out_report);
    SH_TRY(hs_merge_check_apply(hs, rule, value_limit));
    SH_TRY(hs_call_begin(hs));
    hs_merge *m = hs->mrg;
    hs_level &L = hs->lv[m->level];
    const size_t rep_bytes = sizeof(slamhip_merge_report);
    SH_TRY(m->d_rep.grow(rep_bytes, "merge"));
    SH_TRY(m->h_io.grow(rep_bytes, "merge"));
    hipStream_t st = hs->ctx->stream;
    SH_HIP(hipMemsetAsync(m->d_rep, 0, rep_bytes, st));
    k14_apply_arg A;
    A.rep = m->d_rep;
    A.cells = L.d_cells; A.prob = L.d_prob; A.w = L.w; A.h = L.h;
    A.sval = m->d_val;
    A.S = m->S;
    A.t = hs_merge_xf_of(L.stm, pose[0], pose[1], pose[2]);
    A.rule = rule; A.limit = value_limit;
    A.direct = k14_staged() ? 0 : 1;
    if (!k14_tile32()) {
        A.tiles_x = sh_div_up(L.w, 64);
        hipLaunchKernelGGL((k14_apply<64, 32>), dim3((unsigned)(A.tiles_x * sh_div_up(L.h, 32))), dim3(K14_LANES), 0, st, A);
    } else {
        A.tiles_x = sh_div_up(L.w, 32);
        hipLaunchKernelGGL((k14_apply<32, 32>), dim3((unsigned)(A.tiles_x * sh_div_up(L.h, 32))), dim3(K14_LANES), 0, st, A);
    }
    SH_HIP(hipGetLastError());
    SH_HIP(hipMemcpyAsync(m->h_io, m->d_rep, rep_bytes, hipMemcpyDeviceToHost, st));
    SH_TRY(hs_call_finish(hs));
    memcpy(out_report, m->h_io, rep_bytes);
    return SLAMHIP_OK;
}

// CPU-side test hooks: hs_merge.h -- the text the kernels run -- in plain loops
extern "C" int32_t slamhip_debug_merge(const slamhip_cell *dst, int32_t dw, int32_t dh, const slamhip_cell *src, int32_t ax, int32_t ay, int32_t sw, int32_t sh,
                                       const float pose[3], float stm, int32_t rule, float value_limit, slamhip_cell *out_cells,
                                       slamhip_merge_report *out_report)
{
    SH_CHECK_ARG(dst && src && pose && out_cells && out_report && dw >= 1 && dh >= 1 && sw >= 1 && sh >= 1);
    SH_CHECK_ARG((int64_t)dw * dh <= (int64_t)HS_MERGE_MAX_CELLS && (int64_t)sw * sh <= (int64_t)HS_MERGE_MAX_CELLS);
    SH_CHECK_ARG(ax >= -HS_MERGE_MAX_ORIGIN && ax <= HS_MERGE_MAX_ORIGIN && ay >= -HS_MERGE_MAX_ORIGIN && ay <= HS_MERGE_MAX_ORIGIN);
    SH_CHECK_ARG(rule >= 0 && rule <= 2 && isfinite(value_limit) && value_limit > 0.0f);
    const hs_merge_xf t = hs_merge_xf_of(stm, pose[0], pose[1], pose[2]);
    const hs_merge_src S = { ax, ay, sw, sh };
    int64_t ctr[HS_MERGE_CTRS] = { 0 };
    for (int y = 0; y < dh; y++)
        for (int x = 0; x < dw; x++) {
            const size_t i = (size_t)y * dw + x;
            slamhip_cell cell = dst[i];
            int su, sv;
            if (!hs_merge_source_cell(t, S, x, y, &su, &sv)) ctr[HS_MERGE_C_UNSOURCED]++;
            else {
                const float s = src[(size_t)sv * sw + su].value;
                const uint32_t cd = hs_lat_class_bits(cell.value), cs = hs_lat_class_bits(s);
                ctr[3 * cd + cs]++;
                float v; bool clamped;
                if (hs_merge_rule(rule, value_limit, cell.value, s, cd, cs, &v, &clamped) && hs_merge_bits(v) != hs_merge_bits(cell.value)) {
                    ctr[HS_MERGE_C_CHANGED]++;
                    cell.value = v;
                }
                if (clamped) ctr[HS_MERGE_C_CLAMPED]++;
            }
            out_cells[i] = cell;
        }
    memcpy(out_report, ctr, sizeof(ctr));
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_debug_merge_box(const float pose[3], float stm, int32_t ax, int32_t ay, int32_t sw, int32_t sh, int32_t x0, int32_t y0,
                                           int32_t x1, int32_t y1, int32_t out_box[4], int32_t *out_any)
{
    SH_CHECK_ARG(pose && out_box && out_any && sw >= 1 && sh >= 1 && x0 >= 0 && y0 >= 0 && x1 >= x0 && y1 >= y0 && x1 < 32768 && y1 < 32768);
    SH_CHECK_ARG(ax >= -HS_MERGE_MAX_ORIGIN && ax <= HS_MERGE_MAX_ORIGIN && ay >= -HS_MERGE_MAX_ORIGIN && ay <= HS_MERGE_MAX_ORIGIN);
    const hs_merge_src S = { ax, ay, sw, sh };
    hs_merge_box B = { 0, 0, -1, -1 };
    *out_any = hs_merge_box_of(hs_merge_xf_of(stm, pose[0], pose[1], pose[2]), S, x0, y0, x1, y1, &B) ? 1 : 0;
    out_box[0] = B.u0; out_box[1] = B.v0; out_box[2] = B.u1; out_box[3] = B.v1;
    return SLAMHIP_OK;
}
