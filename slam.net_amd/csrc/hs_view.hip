// hs_view.hip -- K15, the view gain of HectorSLAM: the DISTINCT cells of one level of the window that the scan's beams see from
// many poses, counted by class and against a covered layer the hs keeps, and the greedy choice of the few poses that together
// reveal the most (slamhip_hs_view_gain, _view_select, _view_set_covered, _view_get_covered, _view_clear, slamhip_debug_view).  No
// reference counterpart.  Definition: include/slamhip.h (slamhip_view_summary); the arithmetic host and device share: hs_view.h.
//
// The class map is K7's (hs_lattice.hip), re-packed on every call (k7_pack, the window only).  A pose owns a SLOT of seen words:
// the words of its box (hs_view_box_of), rows of the box's own width, at most slot_words = hs_view_slot_rows x hs_view_slot_wpr.
//  * k15_view<LDSV>, one workgroup of 256 lanes per pose, beams strided over the lanes.  Lane 0 forms t and the box.  LDSV: the
//    slot lives in LDS (the host takes this path when slot_words <= K15_LDS_WORDS, 34 KB: four workgroups per compute unit);
//    otherwise in the pose's slot of the scratch block, which a memset zeroed in-stream.  A lane walks its beam with K8's
//    recurrence, K8_AHEAD steps at a time with their class look-ups (the packed map in global memory) issued together, and ORs
//    its seen bits in with vector atomics: in global scratch the bits of the current seen word are kept in a register and ONE
//    atomic is issued when the word changes or the beam ends -- an x-major line costs an atomic per 32 cells; in LDS one atomic
//    per cell, which measured no slower there (K15_ACC_LDS, K15_ACC_GLOBAL: side builds of the other forms).  After a barrier
//    the lanes take the slot's words, count them by popcount against the class words and the covered word (hs_view_word_counts),
//    reduce through shuffles and LDS, and ten lanes store the pose's summary: one workgroup owns the pose, nothing is zeroed
//    ahead.  With `slots` given the LDS path also stores the words to the pose's slot (coalesced) and the box to its header.
//  * k15_commit: ORs the slots of poses [first, first + count) into the covered layer with vector atomics (slots overlap).
//  * k15_gain, a workgroup per pose not yet chosen: popc(V & ~C [& unknown]) over its slot.  k15_pick, ONE workgroup: the maximum
//    of hs_view_key, the threshold, the record, and the winner's slot ORed into C.  The pair is enqueued k times back to back; the
//    winner's index stays on the device, a choice that has stopped leaves the later launches with nothing to do, and the call
//    waits ONCE, at its end.
// Every loop is bounded by reach, n_points, B or the slot's size.
#include "hs_blocks.h"
#include "hs_view.h"
#include <vector>

#define K15_LANES 256
#define K15_AHEAD 8                        // steps of a walk whose look-ups are issued together (K8_AHEAD)
// whether a lane keeps the bits of the current seen word in a register and issues one atomic per word, or one atomic per cell:
// measured (profiles/r21_hs_view.json), a register-kept word is no faster in LDS (equal at reach 64, 0 - 21 % slower at reach 255) and
// 4 - 9 % faster in global scratch, so each path runs its faster form; side builds set the other (tools/hs_view_bench.py)
#ifndef K15_ACC_LDS
#define K15_ACC_LDS 0
#endif
#ifndef K15_ACC_GLOBAL
#define K15_ACC_GLOBAL 1
#endif

static_assert(sizeof(slamhip_view_summary) == 40 && sizeof(slamhip_view_summary) == HS_VIEW_CTRS * sizeof(int32_t), "the record of include/slamhip.h");
static_assert(sizeof(hs_view_box) == 16, "a header of the scratch block");

struct k15_arg {
    const float2 *pts; int n; float ox, oy;   // the scan and its origin
    const float *poses;                    // B x 3, window frame
    const uint32_t *cls; int w, h, wpr16;  // K7's class map of the level
    float stm; int reach;
    const uint32_t *cov; int cwpr;         // the covered layer as it was before the call; nullptr: empty
    uint32_t *slots; int slot_words;       // the scratch block (nullptr on the LDS path: the slots are not kept)
    hs_view_box *hdr;                      // the poses' boxes, with `slots`
    int32_t *sums;                         // B x HS_VIEW_CTRS
};

__device__ static __forceinline__ uint32_t k15_class(const uint32_t *__restrict__ cls, int w, int h, int wpr16, int x, int y)
{
    const bool in = (unsigned)x < (unsigned)w && (unsigned)y < (unsigned)h;
    const uint32_t word = cls[in ? y * wpr16 + (x >> 4) : 0];               // (h * wpr16 < 2^27)
    return in ? (word >> ((x & 15) * 2)) & 3u : 0u;
}

// one walked beam (l.da >= 1): its seen bits ORed into `bits`, the box's slot; true: the beam is cut.  ACC: the bits of the current
// word are kept in a register and ORed in when the word changes; otherwise one atomic per seen cell.
template <bool ACC>
__device__ static __forceinline__ bool k15_beam(const hs_trace_line l, const k15_arg &A, const hs_view_box bx, uint32_t *bits)
{
    hs_trace_walk w = hs_trace_walk_begin(l);
    const int last = hs_view_last(l.da, A.reach);
    int cur = -1;                                                          // the word whose bits `acc` holds
    uint32_t acc = 0;
    bool hit = false;
    for (bool done = false; !done;) {                                      // (w.a goes up by K15_AHEAD per turn and ends at last <= reach)
        int xs[K15_AHEAD], ys[K15_AHEAD];
        uint32_t cs[K15_AHEAD];
        const int a0 = w.a;
#pragma unroll
        for (int u = 0; u < K15_AHEAD; u++) {
            xs[u] = w.x; ys[u] = w.y;
            if (w.a < w.da) hs_trace_walk_next(w);
        }
#pragma unroll
        for (int u = 0; u < K15_AHEAD; u++) cs[u] = a0 + u <= last ? k15_class(A.cls, A.w, A.h, A.wpr16, xs[u], ys[u]) : 0u;
#pragma unroll
        for (int u = 0; u < K15_AHEAD; u++) {
            if (done || a0 + u > last) continue;
            const int j = hs_view_slot_word(bx, A.w, A.h, xs[u], ys[u]);
            if (j >= 0) {
                if constexpr (ACC) {
                    if (j != cur) {
                        if (acc) atomicOr(bits + cur, acc);
                        cur = j; acc = 0;
                    }
                    acc |= 1u << (xs[u] & 31);
                } else atomicOr(bits + j, 1u << (xs[u] & 31));
            }
            if (cs[u] == 1u) { hit = true; done = true; }
        }
        if (a0 + K15_AHEAD > last) done = true;
    }
    if (acc) atomicOr(bits + cur, acc);
    return hs_view_cut(l.da, hit, A.reach);
}

template <bool LDSV>
__global__ void __launch_bounds__(K15_LANES) k15_view(const k15_arg A)
{
    __shared__ uint32_t seen_s[LDSV ? K15_LDS_WORDS : 1];
    __shared__ sh_m3x2 t_s;
    __shared__ hs_view_box box_s;
    __shared__ int red_s[K15_LANES / 64][HS_VIEW_CTRS];
    const int tid = threadIdx.x, pose = blockIdx.x;
    if (tid == 0) {
        t_s = hs_trace_transform(A.stm, A.poses[3 * pose], A.poses[3 * pose + 1], A.poses[3 * pose + 2]);
        hs_view_box b = hs_view_box_of(t_s, A.ox, A.oy, A.reach, A.w, A.h);
        if (b.nwpr * b.rows > A.slot_words) b.nwpr = b.rows = 0;           // (never: the slot is what any box fits -- hs_view_slot_rows, _wpr)
        box_s = b;
    }
    __syncthreads();
    const hs_view_box bx = box_s;
    const int nwords = bx.nwpr * bx.rows;
    uint32_t *gslot = A.slots ? A.slots + (size_t)pose * (size_t)A.slot_words : (uint32_t *)nullptr;
    if constexpr (LDSV) {
        for (int j = tid; j < nwords; j += K15_LANES) seen_s[j] = 0u;
        __syncthreads();
    }
    int cnt[HS_VIEW_CTRS];
#pragma unroll
    for (int c = 0; c < HS_VIEW_CTRS; c++) cnt[c] = 0;
    for (int i = tid; i < A.n; i += K15_LANES) {
        const float2 p = A.pts[i];
        const hs_trace_line l = hs_trace_line_of(t_s, A.ox, A.oy, p.x, p.y);
        if (l.da < 0) cnt[HS_VIEW_C_IGNORED]++;
        else if (l.da == 0) {
            cnt[HS_VIEW_C_SAME]++;
            const int j = hs_view_slot_word(bx, A.w, A.h, l.bx, l.by);
            if (j >= 0) {
                if constexpr (LDSV) atomicOr(seen_s + j, 1u << (l.bx & 31));
                else atomicOr(gslot + j, 1u << (l.bx & 31));
            }
        } else {
            cnt[HS_VIEW_C_WALKED]++;
            bool cut;
            if constexpr (LDSV) cut = k15_beam<K15_ACC_LDS != 0>(l, A, bx, seen_s);
            else cut = k15_beam<K15_ACC_GLOBAL != 0>(l, A, bx, gslot);
            cnt[HS_VIEW_C_CUT] += cut ? 1 : 0;
        }
    }
    if constexpr (!LDSV) __threadfence();                                  // (the atomics of every wavefront, ahead of the loads below)
    __syncthreads();
    for (int j = tid; j < nwords; j += K15_LANES) {
        uint32_t seen;
        if constexpr (LDSV) {
            seen = seen_s[j];
            if (gslot) gslot[j] = seen;
        } else seen = __hip_atomic_load(gslot + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (!seen) continue;
        const int r = j / bx.nwpr, c = j - r * bx.nwpr;
        const int y = bx.y0 + r, xw = bx.xw0 + c;
        uint32_t unk, fre, occ;
        hs_view_class_words(A.cls, A.wpr16, A.w, y, xw * 32, &unk, &fre, &occ);
        const uint32_t cov = A.cov ? A.cov[(size_t)y * A.cwpr + xw] : 0u;
        hs_view_word_counts(seen, unk, fre, occ, cov, cnt);
    }
#pragma unroll
    for (int c = 0; c < HS_VIEW_CTRS; c++)
        for (int off = 32; off > 0; off >>= 1) cnt[c] += __shfl_down(cnt[c], off, 64);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int c = 0; c < HS_VIEW_CTRS; c++) red_s[tid >> 6][c] = cnt[c];
    }
    __syncthreads();
    if (tid < HS_VIEW_CTRS) {
        int v = 0;
        for (int wv = 0; wv < K15_LANES / 64; wv++) v += red_s[wv][tid];
        A.sums[(size_t)pose * HS_VIEW_CTRS + tid] = v;
    }
    if (tid == 0 && A.hdr) A.hdr[pose] = bx;
}

// the slots of poses [first, first + gridDim.y) ORed into the covered layer
__global__ void __launch_bounds__(K15_LANES) k15_commit(const uint32_t *__restrict__ slots, int slot_words, const hs_view_box *__restrict__ hdr, int first,
                                                        uint32_t *cov, int cwpr, int h)
{
    const int pose = first + blockIdx.y;
    const hs_view_box bx = hdr[pose];
    const int j = blockIdx.x * K15_LANES + threadIdx.x;
    if (j >= bx.nwpr * bx.rows) return;
    const uint32_t v = slots[(size_t)pose * (size_t)slot_words + j];
    const int r = j / bx.nwpr, c = j - r * bx.nwpr;
    const int y = bx.y0 + r, xw = bx.xw0 + c;
    if (v && y < h && xw < cwpr) atomicOr(cov + (size_t)y * cwpr + xw, v);
}

struct k15_sel_arg {
    const uint32_t *slots; int slot_words; const hs_view_box *hdr;
    uint32_t *cov; int cwpr;
    const uint32_t *cls; int w, h, wpr16;
    int mode, min_gain, B;
    int32_t *chosen, *gain;                // B each
    int32_t *order, *gains, *state;        // k, k; state: {chosen so far, 1 once the choice has stopped}
};

__global__ void __launch_bounds__(K15_LANES) k15_gain(const k15_sel_arg A)
{
    __shared__ int red_s[K15_LANES / 64];
    const int tid = threadIdx.x, pose = blockIdx.x;
    if (A.state[1]) return;                                                // (uniform: the choice has stopped)
    if (A.chosen[pose]) { if (tid == 0) A.gain[pose] = -1; return; }
    const hs_view_box bx = A.hdr[pose];
    const int nwords = bx.nwpr * bx.rows;
    const uint32_t *slot = A.slots + (size_t)pose * (size_t)A.slot_words;
    int g = 0;
    for (int j = tid; j < nwords; j += K15_LANES) {
        const uint32_t seen = slot[j];
        if (!seen) continue;
        const int r = j / bx.nwpr, c = j - r * bx.nwpr;
        const int y = bx.y0 + r, xw = bx.xw0 + c;
        const uint32_t unk = A.mode ? hs_df_site_word(A.cls + (size_t)y * A.wpr16, A.w, xw * 32, 1) : 0u;
        g += hs_view_word_gain(seen, unk, A.cov[(size_t)y * A.cwpr + xw], A.mode);
    }
    for (int off = 32; off > 0; off >>= 1) g += __shfl_down(g, off, 64);
    if ((tid & 63) == 0) red_s[tid >> 6] = g;
    __syncthreads();
    if (tid == 0) {
        int v = 0;
        for (int wv = 0; wv < K15_LANES / 64; wv++) v += red_s[wv];
        A.gain[pose] = v;
    }
}

__global__ void __launch_bounds__(K15_LANES) k15_pick(const k15_sel_arg A)
{
    __shared__ unsigned long long key_s[K15_LANES / 64];
    const int tid = threadIdx.x;
    if (A.state[1]) return;                                                // (uniform)
    unsigned long long key = 0ull;                                         // (below every pose's: a key's low word is never 0 for an index < 2^32 - 1)
    for (int p = tid; p < A.B; p += K15_LANES) {
        const unsigned long long k = hs_view_key(A.gain[p], p);
        key = k > key ? k : key;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_down(key, off, 64);
        key = o > key ? o : key;
    }
    if ((tid & 63) == 0) key_s[tid >> 6] = key;
    __syncthreads();
    key = key_s[0];
    for (int wv = 1; wv < K15_LANES / 64; wv++) key = key_s[wv] > key ? key_s[wv] : key;
    const int best = hs_view_key_index(key), g = hs_view_key_gain(key);
    if (hs_view_stops(g, A.min_gain) || (unsigned)best >= (unsigned)A.B) {
        if (tid == 0) A.state[1] = 1;
        return;
    }
    if (tid == 0) {
        const int n = A.state[0];
        A.order[n] = best; A.gains[n] = g;
        A.state[0] = n + 1;
        A.chosen[best] = 1;
    }
    // all of V(best) joins C, in either mode; this workgroup is the only writer of C while it runs
    const hs_view_box bx = A.hdr[best];
    const int nwords = bx.nwpr * bx.rows;
    const uint32_t *slot = A.slots + (size_t)best * (size_t)A.slot_words;
    for (int j = tid; j < nwords; j += K15_LANES) {
        const uint32_t seen = slot[j];
        if (!seen) continue;
        const int r = j / bx.nwpr, c = j - r * bx.nwpr;
        A.cov[(size_t)(bx.y0 + r) * A.cwpr + (bx.xw0 + c)] |= seen;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------
// What the view gain keeps, made by the first call that needs it: the covered layer of ONE level with the window origin it was
// made under, the poses, summaries, slot headers, the scratch block of the slots, the choice's block, and the pinned block the
// poses leave and the results reach the host through.
struct hs_view {
    hs_block<uint32_t, HS_MEM_DEVICE> d_cov;
    bool have; int level, cwpr, ch; int64_t ox, oy;
    hs_block<float, HS_MEM_DEVICE> d_poses;
    hs_block<int32_t, HS_MEM_DEVICE> d_sums;
    hs_block<hs_view_box, HS_MEM_DEVICE> d_hdr;
    hs_block<uint32_t, HS_MEM_DEVICE> d_slots;
    hs_block<int32_t, HS_MEM_DEVICE> d_sel;        // chosen[B], gain[B], then order[64], gains[64], state[2]
    hs_block<unsigned char, HS_MEM_PINNED> h_io;
};
#define K15_RES_INTS (2 * HS_VIEW_MAX_K + 2)

// the developer switch (tests, tools/hs_view_bench.py): the slots in global scratch at any size
static bool k15_global() { static const bool v = sh_env_set("SLAMHIP_K15_GLOBAL"); return v; }

// the plan of one call: the slot, where it lives, whether the scratch block is needed
struct k15_plan { int slot_words; bool lds, slots; };

static k15_plan k15_plan_of(const slamhip_hs *hs, int level, int reach, bool keep)
{
    k15_plan P;
    P.slot_words = hs_view_slot_rows(reach, hs->lv[level].h) * hs_view_slot_wpr(reach, hs->lv[level].w);   // (at most 8193 x 258)
    P.lds = !k15_global() && P.slot_words <= K15_LDS_WORDS;
    P.slots = keep || !P.lds;
    return P;
}

int32_t hs_view_check(const slamhip_hs *hs, const char *who, int32_t level, int32_t reach, int32_t B, bool keep, int n_points, bool scan_is_set)
{
    if (level < 0 || level >= hs->n_levels) SH_FAIL(SLAMHIP_ERR_INVALID, "%s: level %d of %d", who, level, hs->n_levels);
    if (reach < 1 || reach > HS_VIEW_MAX_REACH) SH_FAIL(SLAMHIP_ERR_INVALID, "%s: reach = %d must lie in [1, %d]", who, reach, HS_VIEW_MAX_REACH);
    if (B < 1 || B > HS_VIEW_MAX_POSES) SH_FAIL(SLAMHIP_ERR_INVALID, "%s: B = %d must lie in [1, %d]", who, B, HS_VIEW_MAX_POSES);
    const k15_plan P = k15_plan_of(hs, level, reach, keep);
    if (P.slots && (int64_t)B * P.slot_words > HS_VIEW_MAX_SCRATCH)
        SH_FAIL(SLAMHIP_ERR_INVALID, "%s: %d poses x %d scratch words each, more than 2^25", who, B, P.slot_words);
    if (scan_is_set && n_points <= 0) SH_FAIL(SLAMHIP_ERR_STATE, "%s: no scan (slamhip_hs_set_scan first)", who);
    return SLAMHIP_OK;
}

int32_t hs_view_check_gain(const slamhip_hs *hs, int32_t level, int32_t reach, int32_t B, int32_t commit, int n_points, bool scan_is_set)
{
    if (commit < -2 || (B >= 1 && commit >= B)) SH_FAIL(SLAMHIP_ERR_INVALID, "view gain: commit = %d must be -1 (none), -2 (all) or a pose index below %d", commit, B);
    return hs_view_check(hs, "view gain", level, reach, B, commit != -1, n_points, scan_is_set);
}

int32_t hs_view_check_select(const slamhip_hs *hs, int32_t level, int32_t reach, int32_t mode, int32_t min_gain, int32_t B, int32_t k, int n_points,
                             bool scan_is_set)
{
    if (mode != 0 && mode != 1) SH_FAIL(SLAMHIP_ERR_INVALID, "view select: mode = %d must be 0 (new cells) or 1 (new unknown cells)", mode);
    if (min_gain < 1) SH_FAIL(SLAMHIP_ERR_INVALID, "view select: min_gain = %d must be at least 1", min_gain);
    if (k < 1 || k > HS_VIEW_MAX_K) SH_FAIL(SLAMHIP_ERR_INVALID, "view select: k = %d must lie in [1, %d]", k, HS_VIEW_MAX_K);
    return hs_view_check(hs, "view select", level, reach, B, true, n_points, scan_is_set);
}

// the layer a call on `level` meets: none, or one of that level made under the window origin of now
static int32_t k15_layer_check(const slamhip_hs *hs, const char *who, int level)
{
    const hs_view *v = hs->vw;
    if (!v || !v->have) return SLAMHIP_OK;
    if (v->level != level) SH_FAIL(SLAMHIP_ERR_STATE, "%s: the covered layer belongs to level %d, not %d (slamhip_hs_view_set_covered or _view_clear first)", who, v->level, level);
    if (v->ox != hs->win_ox || v->oy != hs->win_oy)
        SH_FAIL(SLAMHIP_ERR_STATE, "%s: the window has moved since the covered layer was made; set the layer again (slamhip_hs_view_set_covered)", who);
    return SLAMHIP_OK;
}

// the layer of `level`, made empty (a memset on the operator's stream) if there is none
static int32_t k15_layer_make(slamhip_hs *hs, int level, bool zero)
{
    hs_view *v = hs->vw;
    const hs_level &L = hs->lv[level];
    const int cwpr = (L.w + 31) / 32;
    const size_t bytes = sizeof(uint32_t) * (size_t)cwpr * L.h;
    v->have = false;
    SH_TRY(v->d_cov.grow(bytes, "view"));
    if (zero) SH_HIP(hipMemsetAsync(v->d_cov, 0, bytes, hs->ctx->stream));
    v->level = level; v->cwpr = cwpr; v->ch = L.h;
    v->ox = hs->win_ox; v->oy = hs->win_oy;
    v->have = true;
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_view_set_covered(slamhip_hs *hs, int32_t level, const uint32_t *bits)
{
    SH_CHECK_ARG(hs);
    if (level < 0 || level >= hs->n_levels) SH_FAIL(SLAMHIP_ERR_INVALID, "view: level %d of %d", level, hs->n_levels);
    SH_TRY(hs_call_begin(hs));
    SH_TRY(hs_unit<&slamhip_hs::vw>(hs));
    hs_view *v = hs->vw;
    const hs_level &L = hs->lv[level];
    const int cwpr = (L.w + 31) / 32;
    const size_t bytes = sizeof(uint32_t) * (size_t)cwpr * L.h;
    if (bits) SH_TRY(v->h_io.grow(bytes, "view"));
    SH_TRY(k15_layer_make(hs, level, bits == nullptr));
    if (bits) {
        uint32_t *st = (uint32_t *)v->h_io.p;
        memcpy(st, bits, bytes);
        if (L.w & 31)                                                      // the padding bits are ignored
            for (int y = 0; y < L.h; y++) st[(size_t)y * cwpr + cwpr - 1] &= (1u << (L.w & 31)) - 1u;
        SH_HIP(hipMemcpyAsync(v->d_cov, st, bytes, hipMemcpyHostToDevice, hs->ctx->stream));
    }
    const int32_t rc = hs_call_finish(hs);
    if (rc != SLAMHIP_OK) v->have = false;
    return rc;
}

extern "C" int32_t slamhip_hs_view_get_covered(slamhip_hs *hs, int32_t level, uint32_t *bits)
{
    SH_CHECK_ARG(hs && bits);
    if (level < 0 || level >= hs->n_levels) SH_FAIL(SLAMHIP_ERR_INVALID, "view: level %d of %d", level, hs->n_levels);
    SH_TRY(k15_layer_check(hs, "view", level));
    const hs_level &L = hs->lv[level];
    const size_t bytes = sizeof(uint32_t) * (size_t)((L.w + 31) / 32) * L.h;
    hs_view *v = hs->vw;
    if (!v || !v->have) { memset(bits, 0, bytes); return SLAMHIP_OK; }     // (empty until set or committed to)
    SH_TRY(hs_call_begin(hs));
    SH_TRY(v->h_io.grow(bytes, "view"));
    SH_HIP(hipMemcpyAsync(v->h_io, v->d_cov, bytes, hipMemcpyDeviceToHost, hs->ctx->stream));
    SH_TRY(hs_call_finish(hs));
    memcpy(bits, v->h_io, bytes);
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_view_clear(slamhip_hs *hs)
{
    SH_CHECK_ARG(hs);
    if (!hs->vw) return SLAMHIP_OK;
    SH_TRY(hs_call_begin(hs));
    SH_HIP(hipStreamSynchronize(hs->ctx->stream));                         // (the blocks are idle after every call of this unit; other units' launches may be in flight)
    hs_unit_drop<&slamhip_hs::vw>(hs);
    return SLAMHIP_OK;
}

// What gain and select share: the blocks, the poses' upload, the class map, the layer, and the launch of k15_view.  h_off: the
// bytes of the pinned block in front of the poses' staging.  On return A is the launch's argument (the later launches read it).
static int32_t k15_enqueue_view(slamhip_hs *hs, int level, int reach, const float *poses, int B, const k15_plan &P, bool need_layer, size_t h_off, k15_arg *out)
{
    hs_class_map M;
    SH_TRY(hs_lat_pack_prepare(hs, level, false, &M));
    SH_TRY(hs_unit<&slamhip_hs::vw>(hs));
    hs_view *v = hs->vw;
    const size_t pose_bytes = sizeof(float) * 3 * (size_t)B;
    SH_TRY(v->d_poses.grow(pose_bytes, "view"));
    SH_TRY(v->d_sums.grow(sizeof(slamhip_view_summary) * (size_t)B, "view"));
    SH_TRY(v->h_io.grow(h_off + pose_bytes, "view"));
    if (P.slots) {
        SH_TRY(v->d_hdr.grow(sizeof(hs_view_box) * (size_t)B, "view"));
        SH_TRY(v->d_slots.grow(sizeof(uint32_t) * (size_t)B * (size_t)P.slot_words, "view"));
    }
    hipStream_t st = hs->ctx->stream;
    if (need_layer && !v->have) SH_TRY(k15_layer_make(hs, level, true));
    float *h_poses = (float *)(v->h_io + h_off);
    memcpy(h_poses, poses, pose_bytes);
    SH_TRY(hs_flush_scan(hs));
    SH_HIP(hipMemcpyAsync(v->d_poses, h_poses, pose_bytes, hipMemcpyHostToDevice, st));
    if (!P.lds) SH_HIP(hipMemsetAsync(v->d_slots, 0, sizeof(uint32_t) * (size_t)B * (size_t)P.slot_words, st));
    SH_TRY(hs_lat_pack_enqueue(hs, level, false, &M));
    k15_arg A;
    A.pts = hs->d_pts; A.n = hs->n_points; A.ox = hs->origin[0]; A.oy = hs->origin[1];
    A.poses = v->d_poses;
    A.cls = M.cls; A.w = M.w; A.h = M.h; A.wpr16 = M.wpr;
    A.stm = hs->lv[level].stm; A.reach = reach;
    A.cov = v->have ? v->d_cov : (const uint32_t *)nullptr; A.cwpr = (M.w + 31) / 32;
    A.slots = P.slots ? v->d_slots : (uint32_t *)nullptr; A.slot_words = P.slot_words;
    A.hdr = P.slots ? v->d_hdr : (hs_view_box *)nullptr;
    A.sums = v->d_sums;
    if (P.lds) hipLaunchKernelGGL(k15_view<true>, dim3((unsigned)B), dim3(K15_LANES), 0, st, A);    // (no timing class of its own)
    else hipLaunchKernelGGL(k15_view<false>, dim3((unsigned)B), dim3(K15_LANES), 0, st, A);
    SH_HIP(hipGetLastError());
    *out = A;
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_view_gain(slamhip_hs *hs, int32_t level, int32_t reach, const float *poses, int32_t B, int32_t commit,
                                        slamhip_view_summary *out_summaries)
{
    SH_CHECK_ARG(hs && poses && out_summaries);
    SH_TRY(hs_view_check_gain(hs, level, reach, B, commit, hs->n_points, true));
    SH_TRY(k15_layer_check(hs, "view gain", level));
    SH_TRY(hs_call_begin(hs));
    const k15_plan P = k15_plan_of(hs, level, reach, commit != -1);
    const size_t sum_bytes = sizeof(slamhip_view_summary) * (size_t)B;
    k15_arg A;
    SH_TRY(k15_enqueue_view(hs, level, reach, poses, B, P, commit != -1, sum_bytes, &A));
    hs_view *v = hs->vw;
    hipStream_t st = hs->ctx->stream;
    if (commit != -1) {
        const int first = commit == -2 ? 0 : commit, count = commit == -2 ? B : 1;
        hipLaunchKernelGGL(k15_commit, dim3((unsigned)sh_div_up(P.slot_words, K15_LANES), (unsigned)count), dim3(K15_LANES), 0, st,
                           (const uint32_t *)v->d_slots, P.slot_words, (const hs_view_box *)v->d_hdr, first, v->d_cov, v->cwpr, v->ch);
        SH_HIP(hipGetLastError());
    }
    SH_HIP(hipMemcpyAsync(v->h_io, v->d_sums, sum_bytes, hipMemcpyDeviceToHost, st));
    SH_TRY(hs_call_finish(hs));
    memcpy(out_summaries, v->h_io, sum_bytes);
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_view_select(slamhip_hs *hs, int32_t level, int32_t reach, int32_t mode, int32_t min_gain, const float *poses, int32_t B,
                                          int32_t k, int32_t *out_order, int32_t *out_gain, int32_t *out_n)
{
    SH_CHECK_ARG(hs && poses && out_order && out_gain && out_n);
    SH_TRY(hs_view_check_select(hs, level, reach, mode, min_gain, B, k, hs->n_points, true));
    SH_TRY(k15_layer_check(hs, "view select", level));
    SH_TRY(hs_call_begin(hs));
    const k15_plan P = k15_plan_of(hs, level, reach, true);
    const size_t res_bytes = sizeof(int32_t) * K15_RES_INTS;
    SH_TRY(hs_unit<&slamhip_hs::vw>(hs));
    hs_view *v = hs->vw;
    SH_TRY(v->d_sel.grow(sizeof(int32_t) * (2 * (size_t)B + K15_RES_INTS), "view"));
    k15_arg A;
    SH_TRY(k15_enqueue_view(hs, level, reach, poses, B, P, true, 2 * res_bytes, &A));   // (pinned: the results, their initial values, the poses)
    hipStream_t st = hs->ctx->stream;
    int32_t *h_res = (int32_t *)v->h_io.p, *h_init = h_res + K15_RES_INTS;
    for (int i = 0; i < HS_VIEW_MAX_K; i++) { h_init[i] = -1; h_init[HS_VIEW_MAX_K + i] = 0; }
    h_init[2 * HS_VIEW_MAX_K] = 0; h_init[2 * HS_VIEW_MAX_K + 1] = 0;
    k15_sel_arg S;
    S.slots = v->d_slots; S.slot_words = P.slot_words; S.hdr = v->d_hdr;
    S.cov = v->d_cov; S.cwpr = v->cwpr;
    S.cls = A.cls; S.w = A.w; S.h = A.h; S.wpr16 = A.wpr16;
    S.mode = mode; S.min_gain = min_gain; S.B = B;
    S.chosen = v->d_sel; S.gain = v->d_sel + B;
    S.order = v->d_sel + 2 * (size_t)B; S.gains = S.order + HS_VIEW_MAX_K; S.state = S.gains + HS_VIEW_MAX_K;
    SH_HIP(hipMemsetAsync(v->d_sel, 0, sizeof(int32_t) * 2 * (size_t)B, st));
    SH_HIP(hipMemcpyAsync(S.order, h_init, res_bytes, hipMemcpyHostToDevice, st));
    for (int j = 0; j < k; j++) {                                          // (the rounds back to back: no wait between them)
        hipLaunchKernelGGL(k15_gain, dim3((unsigned)B), dim3(K15_LANES), 0, st, S);
        hipLaunchKernelGGL(k15_pick, dim3(1), dim3(K15_LANES), 0, st, S);
    }
    SH_HIP(hipGetLastError());
    SH_HIP(hipMemcpyAsync(h_res, S.order, res_bytes, hipMemcpyDeviceToHost, st));
    SH_TRY(hs_call_finish(hs));
    memcpy(out_order, h_res, sizeof(int32_t) * (size_t)k);
    memcpy(out_gain, h_res + HS_VIEW_MAX_K, sizeof(int32_t) * (size_t)k);
    *out_n = h_res[2 * HS_VIEW_MAX_K];
    return SLAMHIP_OK;
}

// CPU-side test hook: hs_view.h -- the text the kernels run -- in plain loops
extern "C" int32_t slamhip_debug_view(const float *values, int32_t w, int32_t h, float stm, const float pose[3], const float origin[2], const float *xy,
                                      int32_t n, int32_t reach, const uint32_t *covered, uint32_t *out_bits, slamhip_view_summary *out_summary)
{
    SH_CHECK_ARG(values && pose && origin && out_bits && out_summary && n >= 0 && (xy || n == 0));
    SH_CHECK_ARG(w >= 1 && h >= 1 && (int64_t)w * h <= ((int64_t)1 << 26) && reach >= 1 && reach <= HS_VIEW_MAX_REACH);
    const int wpr16 = (w + 15) / 16, cwpr = (w + 31) / 32;
    std::vector<uint32_t> cls((size_t)wpr16 * h, 0u);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) cls[(size_t)y * wpr16 + (x >> 4)] |= hs_lat_class_bits(values[(size_t)y * w + x]) << ((x & 15) * 2);
    const sh_m3x2 t = hs_trace_transform(stm, pose[0], pose[1], pose[2]);
    const hs_view_box bx = hs_view_box_of(t, origin[0], origin[1], reach, w, h);
    std::vector<uint32_t> slot((size_t)bx.nwpr * bx.rows + 1, 0u);
    int cnt[HS_VIEW_CTRS] = { 0 };
    for (int i = 0; i < n; i++) {
        const hs_trace_line l = hs_trace_line_of(t, origin[0], origin[1], xy[2 * i], xy[2 * i + 1]);
        if (l.da < 0) { cnt[HS_VIEW_C_IGNORED]++; continue; }
        if (l.da == 0) {
            cnt[HS_VIEW_C_SAME]++;
            const int j = hs_view_slot_word(bx, w, h, l.bx, l.by);
            if (j >= 0) slot[j] |= 1u << (l.bx & 31);
            continue;
        }
        cnt[HS_VIEW_C_WALKED]++;
        hs_trace_walk wk = hs_trace_walk_begin(l);
        const int last = hs_view_last(l.da, reach);
        bool hit = false;
        for (;;) {
            const int j = hs_view_slot_word(bx, w, h, wk.x, wk.y);
            if (j >= 0) {
                slot[j] |= 1u << (wk.x & 31);
                if (((cls[(size_t)wk.y * wpr16 + (wk.x >> 4)] >> ((wk.x & 15) * 2)) & 3u) == 1u) { hit = true; break; }
            }
            if (wk.a >= last) break;
            hs_trace_walk_next(wk);
        }
        if (hs_view_cut(l.da, hit, reach)) cnt[HS_VIEW_C_CUT]++;
    }
    memset(out_bits, 0, sizeof(uint32_t) * (size_t)cwpr * h);
    for (int j = 0; j < bx.nwpr * bx.rows; j++) {
        const uint32_t seen = slot[j];
        if (!seen) continue;
        const int r = j / bx.nwpr, c = j - r * bx.nwpr;
        const int y = bx.y0 + r, xw = bx.xw0 + c;
        uint32_t unk, fre, occ;
        hs_view_class_words(cls.data(), wpr16, w, y, xw * 32, &unk, &fre, &occ);
        uint32_t cov = covered ? covered[(size_t)y * cwpr + xw] : 0u;
        if (xw == cwpr - 1 && (w & 31)) cov &= (1u << (w & 31)) - 1u;     // (the padding bits are ignored)
        hs_view_word_counts(seen, unk, fre, occ, cov, cnt);
        out_bits[(size_t)y * cwpr + xw] = seen;
    }
    memcpy(out_summary, cnt, sizeof(cnt));
    return SLAMHIP_OK;
}
