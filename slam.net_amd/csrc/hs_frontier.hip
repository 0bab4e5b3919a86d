// hs_frontier.hip -- K10, the frontier cells of HectorSLAM's map and their connected clusters: the free cells of one level that touch
// the unknown, grouped under 8-connectivity, each cluster with its seed, size, runs, bounding box and coordinate sums
// (slamhip_hs_frontiers, slamhip_debug_frontiers).  No reference counterpart.  Definition: include/slamhip.h (slamhip_hs_frontiers);
// the arithmetic host and device share: hs_frontier.h.
//
// The class map is K7's (hs_lattice.hip), re-packed on every call: M = (x0, y0, w, h) in the window's frame, the window or the
// world's rectangle R.  Everything below works in M's own cells; the host moves the results to the window's frame.  A cell's flat
// index is y * w + x; a RUN is named by the flat index of its first cell, and two int32 arrays over M -- parent and count -- are
// touched at run starts only.  Every launch but the last two has the same shape: a lane per frontier word (32 cells), a workgroup
// of K10_WG_WORDS words x K10_WG_ROWS rows, and a lane walks the runs that BEGIN in its word (hs_fr_starts), however far they reach.
//  * k10_mark: class words -> frontier words (hs_fr_word), parent[start] = start and count[start] = 0 at every run start; frontier
//    cells and runs counted by popcount, one pair of agent-scope adds per workgroup.
//  * k10_merge: each run unites itself with every run of the row above that overlaps [start - 1, end + 1] (8-connectivity).
//    Lock-free union-find: find both roots, atomicMin the larger root's parent to the smaller; if the value that comes back shows
//    the root had already moved, carry on from that value.  parent[i] <= i always, so there are no cycles, and a component's final
//    root is its minimum -- its seed.  Parents are read with relaxed agent-scope atomic loads within this launch: the XCDs' L2s are
//    not coherent with each other and a CU's L1 is never refreshed by another CU's stores.  A stale parent is still an ancestor, so
//    staleness costs iterations, not correctness; whether a root is still a root is decided by the atomicMin's return value alone.
//  * k10_count: per run, the root found, parent[start] := root, count[root] += the run's length.
//  * k10_slots: a root with count >= min_cells draws a slot from an atomic counter and its parent becomes -2 - slot; the slot's
//    record is initialised from the root (seed, n_cells).  A smaller root, or a draw beyond the block, becomes HS_FR_DROPPED; the
//    counter keeps counting, which is how the host learns n_kept.
//  * k10_stats: per run of a kept cluster, one set of atomics into its slot: n_runs, sum_x, sum_y, x_min, x_max, y_max (y_min is the
//    seed's row).
//  * k10_emit: the counters and the drawn slots into the pinned block the host reads -- only what was drawn, not the 3 MB block.
//  * k10_gather (labels asked for): per cell of the rectangle the frontier bit, the run start by word, the root, the label.
// Every loop that follows parent links or retries an atomic carries the cap G.cap = cells of M + 2: a path is never longer than the
// number of run starts, and a retry happens only when a root has changed, which it does at most once per run.  Word scans end at
// the row's ends.  On overrun the lane sets the flag word and leaves the loop; the host then reports SLAMHIP_ERR_STATE.
#include "hs_blocks.h"
#include "hs_frontier.h"
#include <algorithm>
#include <vector>

#define K10_WG_WORDS 16                    // frontier words of one row a workgroup owns: 512 cells
#define K10_WG_ROWS 16
#define K10_LANES (K10_WG_WORDS * K10_WG_ROWS)
// the counter block
#define K10_C_CELLS 0
#define K10_C_RUNS 1
#define K10_C_CLUSTERS 2
#define K10_C_KEPT 3                       // the slot counter: every kept root draws, also beyond the block
#define K10_C_KEPT_CELLS 4
#define K10_C_FLAG 5
#define K10_CTRS 8

static_assert(sizeof(slamhip_frontier_cluster) == 48 && sizeof(slamhip_frontier_summary) == 40, "the records of include/slamhip.h");
static_assert(HS_FR_MAX_CLUSTERS == SLAMHIP_FRONTIER_MAX_CLUSTERS && K10_LANES == 256, "one block of slots; four wavefronts");

struct k10_geo {
    const uint32_t *cls; int w, h, wpr;    // the class map
    uint32_t *fw; int fwpr, wgx;           // frontier words: rows of fwpr words; workgroups per row of words
    int *parent, *count;                   // per cell of M, run starts only
    int *ctr;
    slamhip_frontier_cluster *rec;
    int cap, min_cells;
};

__device__ static __forceinline__ bool k10_where(const k10_geo &G, int *y, int *j)
{
    const int wy = blockIdx.x / G.wgx, wx = blockIdx.x - wy * G.wgx;
    *j = wx * K10_WG_WORDS + (threadIdx.x & (K10_WG_WORDS - 1));
    *y = wy * K10_WG_ROWS + (int)(threadIdx.x / K10_WG_WORDS);
    return *j < G.fwpr && *y < G.h;
}
// the run starts of word j of row y
__device__ static __forceinline__ uint32_t k10_starts(const k10_geo &G, int y, int j)
{
    const uint32_t *row = G.fw + (size_t)y * G.fwpr;
    return hs_fr_starts(row[j], j > 0 ? row[j - 1] : 0u);
}
__device__ static __forceinline__ void k10_overrun(const k10_geo &G) { __hip_atomic_fetch_or(G.ctr + K10_C_FLAG, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// workgroup sums of up to two per-lane counts into the counter block
__device__ static __forceinline__ void k10_add2(const k10_geo &G, int a, int ia, int b, int ib)
{
    __shared__ int red_s[K10_LANES / 64][2];
    for (int off = 32; off > 0; off >>= 1) { a += __shfl_down(a, off, 64); b += __shfl_down(b, off, 64); }
    if ((threadIdx.x & 63) == 0) { red_s[threadIdx.x >> 6][0] = a; red_s[threadIdx.x >> 6][1] = b; }
    __syncthreads();
    if (threadIdx.x < 2) {
        int v = 0;
        for (int wv = 0; wv < K10_LANES / 64; wv++) v += red_s[wv][threadIdx.x];
        if (v) __hip_atomic_fetch_add(G.ctr + (threadIdx.x ? ib : ia), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ void __launch_bounds__(K10_LANES) k10_mark(const k10_geo G)
{
    int y, j;
    uint32_t f = 0, st = 0;
    if (k10_where(G, &y, &j)) {
        const uint32_t *self = G.cls + (size_t)y * G.wpr;
        const uint32_t *up = y > 0 ? self - G.wpr : (const uint32_t *)nullptr, *down = y + 1 < G.h ? self + G.wpr : (const uint32_t *)nullptr;
        f = hs_fr_word(up, self, down, G.w, 32 * j);
        st = hs_fr_starts(f, j > 0 ? hs_fr_word(up, self, down, G.w, 32 * (j - 1)) : 0u);
        G.fw[(size_t)y * G.fwpr + j] = f;
        for (uint32_t s = st; s; s &= s - 1) {                             // (at most 16 run starts in a word)
            const int idx = y * G.w + 32 * j + hs_df_ctz(s);               // (a set bit is a cell of M: below w)
            G.parent[idx] = idx; G.count[idx] = 0;
        }
    }
    k10_add2(G, __popc(f), K10_C_CELLS, __popc(st), K10_C_RUNS);
}

// ---- the union-find over run starts ----
__device__ static __forceinline__ int k10_find_atomic(const k10_geo &G, int a)
{
    for (int it = 0; it < G.cap; it++) {
        const int p = __hip_atomic_load(G.parent + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p == a) return a;
        a = p;
    }
    k10_overrun(G);
    return -1;
}
__device__ static __forceinline__ void k10_unite(const k10_geo &G, int a, int b)
{
    for (int it = 0; it < G.cap; it++) {
        const int ra = k10_find_atomic(G, a), rb = k10_find_atomic(G, b);
        if (ra < 0 || rb < 0 || ra == rb) return;
        const int hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
        const int old = __hip_atomic_fetch_min(G.parent + hi, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == hi) return;                                             // hi was a root and now hangs under lo
        a = old; b = lo;                                                   // hi had moved under `old` already: unite that with lo
    }
    k10_overrun(G);
}

__global__ void __launch_bounds__(K10_LANES) k10_merge(const k10_geo G)
{
    int y, j;
    if (!k10_where(G, &y, &j) || y == 0) return;
    const uint32_t *row = G.fw + (size_t)y * G.fwpr, *above = row - G.fwpr;
    for (uint32_t st = k10_starts(G, y, j); st; st &= st - 1) {
        const int s = 32 * j + hs_df_ctz(st), e = hs_fr_run_end(row, G.fwpr, s);
        const int lo = s > 0 ? s - 1 : 0, hi = e + 1 < G.w ? e + 1 : G.w - 1;
        int p = lo, it = 0;
        for (; it <= G.w; it++) {                                          // (every turn moves p at least two cells on)
            const int q = hs_fr_next_set(above, G.fwpr, p);
            if (q > hi) break;
            k10_unite(G, y * G.w + s, (y - 1) * G.w + hs_fr_run_start(above, q));
            p = hs_fr_run_end(above, G.fwpr, q) + 2;
        }
        if (it > G.w) k10_overrun(G);
    }
}

// the root of run start a once k10_merge has ended: plain loads (the launch boundary has made every parent visible; k10_count's
// own stores only replace an ancestor by the root)
__device__ static __forceinline__ int k10_find(const k10_geo &G, int a)
{
    for (int it = 0; it < G.cap; it++) {
        const int p = G.parent[a];
        if (p == a) return a;
        a = p;
    }
    k10_overrun(G);
    return -1;
}

__global__ void __launch_bounds__(K10_LANES) k10_count(const k10_geo G)
{
    int y, j;
    if (!k10_where(G, &y, &j)) return;
    const uint32_t *row = G.fw + (size_t)y * G.fwpr;
    for (uint32_t st = k10_starts(G, y, j); st; st &= st - 1) {
        const int s = 32 * j + hs_df_ctz(st), e = hs_fr_run_end(row, G.fwpr, s);
        const int idx = y * G.w + s, root = k10_find(G, idx);
        if (root < 0) continue;
        if (root != idx) G.parent[idx] = root;
        __hip_atomic_fetch_add(G.count + root, e - s + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ void __launch_bounds__(K10_LANES) k10_slots(const k10_geo G)
{
    int y, j;
    int roots = 0, kept_cells = 0;
    if (k10_where(G, &y, &j))
        for (uint32_t st = k10_starts(G, y, j); st; st &= st - 1) {
            const int s = 32 * j + hs_df_ctz(st), idx = y * G.w + s;
            if (G.parent[idx] != idx) continue;                            // (every other run start points at its root since k10_count)
            roots++;
            const int n = G.count[idx];
            int enc = HS_FR_DROPPED;
            if (n >= G.min_cells) {
                kept_cells += n;
                const int slot = __hip_atomic_fetch_add(G.ctr + K10_C_KEPT, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (slot < HS_FR_MAX_CLUSTERS) {
                    slamhip_frontier_cluster c;
                    c.seed_x = s; c.seed_y = y; c.n_cells = n; c.n_runs = 0;
                    c.x_min = INT32_MAX; c.y_min = y; c.x_max = INT32_MIN; c.y_max = y;
                    c.sum_x = 0; c.sum_y = 0;
                    G.rec[slot] = c;
                    enc = -2 - slot;
                }
            }
            G.parent[idx] = enc;
        }
    k10_add2(G, roots, K10_C_CLUSTERS, kept_cells, K10_C_KEPT_CELLS);
}

// parent[] after k10_slots: a root holds its code (< 0), every other run start its root
__device__ static __forceinline__ int k10_root_of(const k10_geo &G, int idx, int *enc)
{
    const int p = G.parent[idx];
    if (p < 0) { *enc = p; return idx; }
    *enc = G.parent[p];
    return p;
}

__global__ void __launch_bounds__(K10_LANES) k10_stats(const k10_geo G)
{
    int y, j;
    if (!k10_where(G, &y, &j)) return;
    const uint32_t *row = G.fw + (size_t)y * G.fwpr;
    for (uint32_t st = k10_starts(G, y, j); st; st &= st - 1) {
        const int s = 32 * j + hs_df_ctz(st), e = hs_fr_run_end(row, G.fwpr, s);
        int enc;
        (void)k10_root_of(G, y * G.w + s, &enc);
        if (enc > -2) continue;                                            // dropped (or, after an overrun, not a code at all)
        slamhip_frontier_cluster *c = G.rec + (-2 - enc);
        __hip_atomic_fetch_add(&c->n_runs, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add((unsigned long long *)&c->sum_x, (unsigned long long)hs_fr_run_sum(s, e), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add((unsigned long long *)&c->sum_y, (unsigned long long)((long long)(e - s + 1) * y), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_min(&c->x_min, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_max(&c->x_max, e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_max(&c->y_max, y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// the counters, then the drawn slots, word by word, into the pinned block: out[0 .. K10_CTRS) the counters, the records behind
__global__ void __launch_bounds__(256) k10_emit(const int *__restrict__ ctr, const int *__restrict__ rec, int *__restrict__ out)
{
    const int kept = ctr[K10_C_KEPT];
    const int words = (kept < HS_FR_MAX_CLUSTERS ? kept : HS_FR_MAX_CLUSTERS) * (int)(sizeof(slamhip_frontier_cluster) / sizeof(int));
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < K10_CTRS) out[t] = ctr[t];
    if (t < words) out[K10_CTRS + t] = rec[t];
}

__global__ void __launch_bounds__(256) k10_gather(const k10_geo G, int gx, int gy, int gw, int n, int *__restrict__ out)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const int ry = t / gw, rx = t - ry * gw;
    const long long x = (long long)gx + rx, y = (long long)gy + ry;        // M's cells
    int label = -1;
    if (x >= 0 && x < G.w && y >= 0 && y < G.h) {
        const uint32_t *row = G.fw + (size_t)y * G.fwpr;
        if ((row[x >> 5] >> (x & 31)) & 1u) {
            int enc;
            label = k10_root_of(G, (int)y * G.w + hs_fr_run_start(row, (int)x), &enc);
        }
    }
    out[t] = label;
}

// ---- host side ---------------------------------------------------------------------------------------------------
// What the labelling needs, made by the first call and kept: the frontier words, parent and count over M, the counters and the
// record block, the labels' device block, and the two pinned, device-visible blocks the results reach the host through (counters and
// records, stored by k10_emit; the labels, copied).
struct hs_frontier {
    hs_block<uint32_t, HS_MEM_DEVICE> d_fw;
    hs_block<int, HS_MEM_DEVICE> d_parent;
    hs_block<int, HS_MEM_DEVICE> d_count;
    hs_block<int, HS_MEM_DEVICE> d_ctr;
    hs_block<slamhip_frontier_cluster, HS_MEM_DEVICE> d_rec;
    hs_block<int, HS_MEM_DEVICE> d_labels;
    hs_block<unsigned char, HS_MEM_PINNED_VISIBLE> h_head;   // device-visible: k10_emit stores into it
    hs_block<unsigned char, HS_MEM_PINNED_VISIBLE> h_labels;
};
#define HS_FR_HEAD_BYTES (sizeof(int) * K10_CTRS + sizeof(slamhip_frontier_cluster) * (size_t)HS_FR_MAX_CLUSTERS)

// what both entry points refuse for their arguments alone
static int32_t hs_fr_check(int32_t min_cells, int32_t max_clusters, const void *out_clusters)
{
    if (min_cells < 1) SH_FAIL(SLAMHIP_ERR_INVALID, "frontiers: min_cells = %d must be at least 1", min_cells);
    if (max_clusters < 0 || max_clusters > HS_FR_MAX_CLUSTERS)
        SH_FAIL(SLAMHIP_ERR_INVALID, "frontiers: max_clusters = %d must lie in [0, %d]", max_clusters, HS_FR_MAX_CLUSTERS);
    if (max_clusters > 0 && !out_clusters) SH_FAIL(SLAMHIP_ERR_INVALID, "frontiers: out_clusters is NULL with max_clusters = %d", max_clusters);
    return SLAMHIP_OK;
}

// The host's part of the result, shared with the test hook.  ctr: the counter block; rec: the drawn slots in M's cells, any order
// (sorted here by step 6: n_cells descending, equal sizes by label ascending); (x0, y0): M's first cell in the window's frame.
static int32_t hs_fr_finish(const int *ctr, slamhip_frontier_cluster *rec, int x0, int y0, int w, int h, int32_t max_clusters,
                            slamhip_frontier_summary *S, slamhip_frontier_cluster *out)
{
    S->mx0 = x0; S->my0 = y0; S->mw = w; S->mh = h;
    S->n_frontier_cells = ctr[K10_C_CELLS]; S->n_runs = ctr[K10_C_RUNS]; S->n_clusters = ctr[K10_C_CLUSTERS];
    S->n_kept = ctr[K10_C_KEPT]; S->n_returned = 0; S->kept_cells = ctr[K10_C_KEPT_CELLS];
    if (S->n_kept > HS_FR_MAX_CLUSTERS)
        SH_FAIL(SLAMHIP_ERR_INVALID, "frontiers: %d clusters are kept, more than the %d the record block holds; raise min_cells", S->n_kept,
                HS_FR_MAX_CLUSTERS);
    std::sort(rec, rec + S->n_kept, [w](const slamhip_frontier_cluster &a, const slamhip_frontier_cluster &b) {
        if (a.n_cells != b.n_cells) return a.n_cells > b.n_cells;
        return (int64_t)a.seed_y * w + a.seed_x < (int64_t)b.seed_y * w + b.seed_x;
    });
    S->n_returned = std::min(S->n_kept, max_clusters);
    for (int i = 0; i < S->n_returned; i++) {
        slamhip_frontier_cluster c = rec[i];
        c.seed_x += x0; c.x_min += x0; c.x_max += x0; c.sum_x += (int64_t)c.n_cells * x0;
        c.seed_y += y0; c.y_min += y0; c.y_max += y0; c.sum_y += (int64_t)c.n_cells * y0;
        out[i] = c;
    }
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_frontiers(slamhip_hs *hs, int32_t level, int32_t world, int32_t min_cells, int32_t max_clusters,
                                        slamhip_frontier_summary *out_summary, slamhip_frontier_cluster *out_clusters,
                                        int32_t lx, int32_t ly, int32_t lw, int32_t lh, int32_t *out_labels)
{
    SH_CHECK_ARG(hs && out_summary);
    if (level < 0 || level >= hs->n_levels) SH_FAIL(SLAMHIP_ERR_INVALID, "frontiers: level %d of %d", level, hs->n_levels);
    if (world != 0 && world != 1) SH_FAIL(SLAMHIP_ERR_INVALID, "frontiers: world = %d must be 0 (the window) or 1 (the world)", world);
    SH_TRY(hs_fr_check(min_cells, max_clusters, out_clusters));
    if (out_labels && (lw < 1 || lh < 1 || (int64_t)lw * lh > HS_FR_MAX_RECT))
        SH_FAIL(SLAMHIP_ERR_INVALID, "frontiers: a label rectangle of %d x %d cells; lw, lh >= 1 and lw * lh <= 2^24", lw, lh);
    slamhip_ctx *ctx = hs->ctx;
    SH_TRY(hs_call_begin(hs));
    hs_class_map M;
    SH_TRY(hs_lat_pack_prepare(hs, level, world != 0, &M));
    const int64_t cells = (int64_t)M.w * M.h;
    if (cells > HS_FR_MAX_M)
        SH_FAIL(SLAMHIP_ERR_INVALID, "frontiers: M, the class map of level %d, is %d x %d cells, more than 2^25", level, M.w, M.h);
    SH_TRY(hs_unit<&slamhip_hs::frl>(hs));
    hs_frontier *fr = hs->frl;
    k10_geo G;
    G.cls = M.cls; G.w = M.w; G.h = M.h; G.wpr = M.wpr;
    G.fwpr = (M.w + 31) / 32; G.wgx = sh_div_up(G.fwpr, K10_WG_WORDS);
    G.cap = (int)cells + 2; G.min_cells = min_cells;
    const int n_labels = out_labels ? lw * lh : 0;
    const size_t label_bytes = sizeof(int) * (size_t)n_labels;
    SH_TRY(fr->d_fw.grow(sizeof(uint32_t) * (size_t)G.fwpr * G.h, "frontiers"));
    SH_TRY(fr->d_parent.grow(sizeof(int) * (size_t)cells, "frontiers"));
    SH_TRY(fr->d_count.grow(sizeof(int) * (size_t)cells, "frontiers"));
    SH_TRY(fr->d_ctr.grow(sizeof(int) * K10_CTRS, "frontiers"));
    SH_TRY(fr->d_rec.grow(sizeof(slamhip_frontier_cluster) * (size_t)HS_FR_MAX_CLUSTERS, "frontiers"));
    if (n_labels) SH_TRY(fr->d_labels.grow(label_bytes, "frontiers"));
    SH_TRY(fr->h_head.grow(HS_FR_HEAD_BYTES, "frontiers"));
    if (n_labels) SH_TRY(fr->h_labels.grow(label_bytes, "frontiers"));
    G.fw = fr->d_fw; G.parent = fr->d_parent; G.count = fr->d_count; G.ctr = fr->d_ctr; G.rec = fr->d_rec;
    // (at most 2^25 cells in M: no grid reaches 2^31 workgroups)
    const dim3 grid((unsigned)G.wgx * (unsigned)sh_div_up(G.h, K10_WG_ROWS)), lanes(K10_LANES);
    SH_HIP(hipMemsetAsync(fr->d_ctr, 0, sizeof(int) * K10_CTRS, ctx->stream));
    SH_TRY(hs_lat_pack_enqueue(hs, level, world != 0, &M));
    hipLaunchKernelGGL(k10_mark, grid, lanes, 0, ctx->stream, G);
    SH_HIP(hipGetLastError());
    hipLaunchKernelGGL(k10_merge, grid, lanes, 0, ctx->stream, G);
    SH_HIP(hipGetLastError());
    hipLaunchKernelGGL(k10_count, grid, lanes, 0, ctx->stream, G);
    SH_HIP(hipGetLastError());
    hipLaunchKernelGGL(k10_slots, grid, lanes, 0, ctx->stream, G);
    SH_HIP(hipGetLastError());
    hipLaunchKernelGGL(k10_stats, grid, lanes, 0, ctx->stream, G);
    SH_HIP(hipGetLastError());
    const int rec_words = HS_FR_MAX_CLUSTERS * (int)(sizeof(slamhip_frontier_cluster) / sizeof(int));
    hipLaunchKernelGGL(k10_emit, dim3((unsigned)sh_div_up(rec_words, 256)), dim3(256), 0, ctx->stream, (const int *)fr->d_ctr, (const int *)fr->d_rec.p,
                       (int *)fr->h_head.p);
    SH_HIP(hipGetLastError());
    if (n_labels) {
        hipLaunchKernelGGL(k10_gather, dim3((unsigned)sh_div_up(n_labels, 256)), dim3(256), 0, ctx->stream, G, lx - M.x0, ly - M.y0, lw, n_labels,
                           fr->d_labels);                                  // (-2^28 < x0 <= 0 and the kernel widens: a far rectangle is simply outside M)
        SH_HIP(hipGetLastError());
        SH_HIP(hipMemcpyAsync(fr->h_labels, fr->d_labels, label_bytes, hipMemcpyDeviceToHost, ctx->stream));
    }
    SH_TRY(hs_call_finish(hs));
    const int *ctr = (const int *)fr->h_head.p;
    if (ctr[K10_C_FLAG]) SH_FAIL(SLAMHIP_ERR_STATE, "frontier labelling did not converge (level %d, M of %d x %d cells)", level, M.w, M.h);
    SH_TRY(hs_fr_finish(ctr, (slamhip_frontier_cluster *)(fr->h_head + sizeof(int) * K10_CTRS), M.x0, M.y0, M.w, M.h, max_clusters, out_summary,
                        out_clusters));
    if (n_labels) memcpy(out_labels, fr->h_labels, label_bytes);
    return SLAMHIP_OK;
}

// CPU-side test hook: the clusters of the definition over a caller's class array.  The classes are packed as K7 packs them; the
// frontier words by hs_fr_word and the runs by hs_fr_starts / hs_fr_run_end / hs_fr_next_set / hs_fr_run_start -- the text the
// kernels run -- and the components by a plain sequential union-find over run starts (the smaller root wins, as on the device).
extern "C" int32_t slamhip_debug_frontiers(const uint8_t *cls, int32_t cw, int32_t ch, int32_t min_cells, int32_t max_clusters,
                                           slamhip_frontier_summary *out_summary, slamhip_frontier_cluster *out_clusters, int32_t *out_labels)
{
    SH_CHECK_ARG(cls && out_summary);
    if (cw < 1 || ch < 1 || (int64_t)cw * ch > HS_FR_MAX_M)
        SH_FAIL(SLAMHIP_ERR_INVALID, "frontiers: a class array of %d x %d cells; cw, ch >= 1 and cw * ch <= 2^25", cw, ch);
    SH_TRY(hs_fr_check(min_cells, max_clusters, out_clusters));
    const int wpr = (cw + 15) / 16, fwpr = (cw + 31) / 32;
    std::vector<uint32_t> packed((size_t)wpr * ch, 0u), fw((size_t)fwpr * ch);
    for (int cy = 0; cy < ch; cy++)
        for (int cx = 0; cx < cw; cx++) packed[(size_t)cy * wpr + (cx >> 4)] |= (uint32_t)(cls[(size_t)cy * cw + cx] & 3u) << (2 * (cx & 15));
    int ctr[K10_CTRS] = { 0 };
    for (int y = 0; y < ch; y++) {
        const uint32_t *self = packed.data() + (size_t)y * wpr;
        const uint32_t *up = y > 0 ? self - wpr : (const uint32_t *)nullptr, *down = y + 1 < ch ? self + wpr : (const uint32_t *)nullptr;
        for (int j = 0; j < fwpr; j++) {
            const uint32_t f = hs_fr_word(up, self, down, cw, 32 * j);
            fw[(size_t)y * fwpr + j] = f;
            ctr[K10_C_CELLS] += __builtin_popcount(f);
        }
    }
    std::vector<int> parent((size_t)cw * ch, -1), count((size_t)cw * ch, 0);
    auto find = [&parent](int a) { while (parent[(size_t)a] != a) a = parent[(size_t)a]; return a; };
    // every run start of row y, by word: fn(s, e)
    auto runs = [&](int y, auto fn) {
        const uint32_t *row = fw.data() + (size_t)y * fwpr;
        for (int j = 0; j < fwpr; j++)
            for (uint32_t st = hs_fr_starts(row[j], j > 0 ? row[j - 1] : 0u); st; st &= st - 1) {
                const int s = 32 * j + hs_df_ctz(st);
                fn(s, hs_fr_run_end(row, fwpr, s));
            }
    };
    for (int y = 0; y < ch; y++) {
        const uint32_t *above = y > 0 ? fw.data() + (size_t)(y - 1) * fwpr : (const uint32_t *)nullptr;
        runs(y, [&](int s, int e) {
            const int idx = y * cw + s;
            parent[(size_t)idx] = idx;
            ctr[K10_C_RUNS]++;
            if (!above) return;
            const int hi = e + 1 < cw ? e + 1 : cw - 1;
            for (int p = s > 0 ? s - 1 : 0;;) {
                const int q = hs_fr_next_set(above, fwpr, p);
                if (q > hi) break;
                const int ra = find(idx), rb = find((y - 1) * cw + hs_fr_run_start(above, q));
                if (ra != rb) parent[(size_t)std::max(ra, rb)] = std::min(ra, rb);
                p = hs_fr_run_end(above, fwpr, q) + 2;
            }
        });
    }
    for (int y = 0; y < ch; y++)
        runs(y, [&](int s, int e) {
            const int idx = y * cw + s, root = find(idx);
            parent[(size_t)idx] = root;
            count[(size_t)root] += e - s + 1;
        });
    std::vector<slamhip_frontier_cluster> rec;
    std::vector<int> slot_of((size_t)cw * ch, HS_FR_DROPPED);                // per root
    for (int y = 0; y < ch; y++)
        runs(y, [&](int s, int) {
            const int idx = y * cw + s;
            if (parent[(size_t)idx] != idx) return;
            ctr[K10_C_CLUSTERS]++;
            const int n = count[(size_t)idx];
            if (n < min_cells) return;
            ctr[K10_C_KEPT_CELLS] += n;
            if (ctr[K10_C_KEPT]++ >= HS_FR_MAX_CLUSTERS) return;
            slamhip_frontier_cluster c;
            c.seed_x = s; c.seed_y = y; c.n_cells = n; c.n_runs = 0;
            c.x_min = INT32_MAX; c.y_min = y; c.x_max = INT32_MIN; c.y_max = y;
            c.sum_x = 0; c.sum_y = 0;
            slot_of[(size_t)idx] = (int)rec.size();
            rec.push_back(c);
        });
    for (int y = 0; y < ch; y++)
        runs(y, [&](int s, int e) {
            const int slot = slot_of[(size_t)parent[(size_t)(y * cw + s)]];
            if (slot < 0) return;
            slamhip_frontier_cluster &c = rec[(size_t)slot];
            c.n_runs++;
            c.sum_x += hs_fr_run_sum(s, e); c.sum_y += (int64_t)(e - s + 1) * y;
            c.x_min = std::min(c.x_min, s); c.x_max = std::max(c.x_max, e); c.y_max = std::max(c.y_max, y);
        });
    SH_TRY(hs_fr_finish(ctr, rec.data(), 0, 0, cw, ch, max_clusters, out_summary, out_clusters));
    if (out_labels)
        for (int y = 0; y < ch; y++) {
            const uint32_t *row = fw.data() + (size_t)y * fwpr;
            for (int x = 0; x < cw; x++)
                out_labels[(size_t)y * cw + x] = ((row[x >> 5] >> (x & 31)) & 1u) ? parent[(size_t)(y * cw + hs_fr_run_start(row, x))] : -1;
        }
    return SLAMHIP_OK;
}
