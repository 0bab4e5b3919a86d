// hs_nav.hip -- K11, the cost-to-go field of HectorSLAM's map: for every traversable cell of one level the least 5-7 chamfer cost
// of a path from a set of source cells that keeps a clearance from the walls and cuts no corner, the step towards the source, the
// cheapest reachable cell of each of a list of goal rectangles and the cell paths to the first few of them (slamhip_hs_nav_field,
// slamhip_debug_nav_field).  No reference counterpart.  Definition: include/slamhip.h (slamhip_hs_nav_field); the arithmetic host
// and device share: hs_nav.h.
//
// The class map is K7's (hs_lattice.hip), re-packed on every call: M = (x0, y0, w, h) in the window's frame, the window or the
// world's rectangle R; for a clearance c >= 1 K9's field with radius c + 1 is built behind it (hs_df_field_*).  Everything below
// works in M's own cells; a cell's flat index is y * w + x.
//  * k11_trav: class words (and the field) -> traversable words (hs_nav_trav_word), 1 bit per cell; n_traversable by popcount.
//  * k11_seed: cost 0 at every used source, the counts of used and blocked sources, the active flag of each source's tile.
//  * k11_relax, one launch per ROUND, a workgroup per tile of K11_TILE x K11_TILE cells.  Two flag arrays of a byte per tile: in
//    round k a workgroup whose flag in act[k & 1] is clear returns at once.  An active one clears its flag, loads its tile and a
//    one-cell halo of costs and traversable bits into LDS, relaxes there until a whole pass changes nothing, stores the cells that
//    got lower and, where a cell of its outer ring got lower, sets act[(k + 1) & 1] of every neighbouring tile that touches that cell
//    and adds to the round's counter.  In LDS a lane owns one column of 16 rows of the tile (a wavefront reads 64 consecutive words:
//    no bank conflict) and sweeps it downwards and upwards in turn; a cell is written by its owner only, its neighbours are read
//    while their owners may be writing them (32-bit LDS accesses are whole), and every value ever held is the cost of a real path,
//    so the order is free: the pass that changes nothing has read the fixed point.  The passes are capped by the tile's cells + 1.
//    A workgroup writes only its own tile's costs in global memory and reads the halo with plain loads: a halo cell that a neighbour
//    lowers in the same round is read old or new, either is the cost of a real path, and the neighbour's change re-activates this
//    tile for the next round.  The launch boundary makes every store of a round visible to the next.  So the costs need no
//    atomics; the flags are idempotent agent-scope byte stores and the counter an atomic add.  When a round sets no flag every tile
//    is converged against a halo that did not move: the global fixed point, which is unique.
//  * k11_peek: the round counters of a batch and the counter block into pinned memory -- the host enqueues a BATCH of rounds, this
//    launch, and waits once per batch (bounded wait); it stops when the last round of the batch set no flag.  No launch waits for
//    another workgroup, so a relaxation bug cannot hang the device: rounds are capped by n_traversable + 1 on the host.
//  * k11_dirs: a lane per cell of M, the dir byte by hs_nav_dir; n_reached and max_cost_reached.
//  * k11_goals: a workgroup per goal rectangle, the minimum of (cost << 32 | flat index) over its clip to M and the reached cells.
//  * k11_paths: a lane per path follows the dir bytes, capped by n_traversable.
//  * k11_gather: the caller's rectangle of costs and / or dirs, the outside values outside M.
//  * k11_emit: the counters, the goal results and the path heads into pinned memory.
#include "hs_blocks.h"
#include "hs_nav.h"
#include "hs_nav_host.h"
#include <algorithm>
#include <functional>
#include <queue>
#include <vector>

#define K11_TILE 64                        // cells per side of a relaxation tile: (64 + 2)^2 costs = 17 KB of LDS, three workgroups per CU and more
#define K11_BATCH 8                        // rounds the host enqueues per wait (SLAMHIP_NAV_BATCH overrides: 1 .. K11_MAX_BATCH)
#define K11_MAX_BATCH 64
#define K11_LANES 256
#define K11_ROWS (K11_TILE * K11_TILE / K11_LANES)   // rows of its column a lane owns
#define K11_PITCH (K11_TILE + 2)
#define K11_TW ((K11_PITCH + 31) / 32)     // traversable words of a tile row with its halo
// (the counter block, K11_C_* and K11_CTRS: hs_internal.h)

static_assert(sizeof(slamhip_nav_spec) == 20 && sizeof(slamhip_nav_goal_result) == 16 && sizeof(slamhip_nav_path) == 8 &&
              sizeof(slamhip_nav_summary) == 40, "the records of include/slamhip.h");
static_assert(K11_TILE == 64 && K11_LANES == 256 && K11_ROWS == 16 && K11_TW == 3, "a wavefront per tile row; the halo's bits from two words of a row");
static_assert(HS_NAV_UNREACHED == SLAMHIP_NAV_UNREACHED, "one value for the unreached");

struct k11_geo {
    const uint32_t *cls; int w, h, wpr;    // the class map
    const uint16_t *f; int fpitch, fr;     // K9's field at M's cell (-fr, -fr), or nullptr (clearance 0)
    uint32_t c2;
    uint32_t *tw; int twpr;                // traversable words: rows of twpr words
    uint32_t *cost; uint8_t *dir;          // per cell of M
    uint8_t *act; int tiles_x, tiles_y;    // 2 x tiles_x * tiles_y flags
    uint32_t *ctr;
    uint32_t max_cost;
    int x0, y0;                            // M's first cell in the window's frame
};

__device__ static __forceinline__ void k11_overrun(const k11_geo &G) { __hip_atomic_fetch_or(G.ctr + K11_C_FLAG, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ static __forceinline__ int k11_wave_sum(int v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

__global__ void __launch_bounds__(256) k11_trav(const k11_geo G)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    uint32_t word = 0;
    if (t < G.twpr * G.h) {
        const int y = t / G.twpr, j = t - y * G.twpr;
        const uint16_t *f = G.f ? G.f + (size_t)(y + G.fr) * G.fpitch + (size_t)(32 * j + G.fr) : (const uint16_t *)nullptr;
        word = hs_nav_trav_word(G.cls + (size_t)y * G.wpr, G.w, 32 * j, f, G.c2);
        G.tw[t] = word;
    }
    const int n = k11_wave_sum(__popc(word));
    if ((threadIdx.x & 63) == 0 && n) __hip_atomic_fetch_add(G.ctr + K11_C_TRAV, (uint32_t)n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// src: S pairs in window-frame cells
__global__ void __launch_bounds__(256) k11_seed(const k11_geo G, const int *__restrict__ src, int S)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= S) return;
    const long long x = (long long)src[2 * i] - G.x0, y = (long long)src[2 * i + 1] - G.y0;
    const bool used = x >= 0 && x < G.w && y >= 0 && y < G.h && hs_nav_bit(G.tw + (size_t)y * G.twpr, G.twpr, (int)x);
    if (used) {
        G.cost[(size_t)y * G.w + (size_t)x] = 0u;                          // (a source given twice stores twice)
        __hip_atomic_store(G.act + ((int)y / K11_TILE) * G.tiles_x + (int)x / K11_TILE, (uint8_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __hip_atomic_fetch_add(G.ctr + (used ? K11_C_USED : K11_C_BLOCKED), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(K11_LANES) k11_relax(const k11_geo G, int round, uint32_t *__restrict__ n_set)
{
    __shared__ uint32_t cost_s[K11_PITCH * K11_PITCH];
    __shared__ uint32_t trav_s[K11_PITCH * K11_TW];
    __shared__ uint32_t nb_s;
    const int tid = threadIdx.x, tile = blockIdx.x, nt = G.tiles_x * G.tiles_y;
    uint8_t *cur = G.act + (round & 1) * nt, *nxt = G.act + ((round + 1) & 1) * nt;
    if (!cur[tile]) return;                                                // (nobody stores into cur in this round but lane 0 below, behind the barrier)
    const int ty = tile / G.tiles_x, tx = tile - ty * G.tiles_x;
    const int gx0 = tx * K11_TILE - 1, gy0 = ty * K11_TILE - 1;            // the halo's first cell
    for (int j = tid; j < K11_PITCH * K11_TW; j += K11_LANES) {
        const int ly = j / K11_TW, k = j - ly * K11_TW, gy = gy0 + ly;
        uint32_t v = 0;
        if (gy >= 0 && gy < G.h) {                                         // local bit lx is cell gx0 + lx, and gx0 is 31 modulo 32
            const uint32_t *row = G.tw + (size_t)gy * G.twpr;
            const int wi = ((gx0 + 1) >> 5) + k - 1;
            const uint32_t lo = (wi >= 0 && wi < G.twpr) ? row[wi] : 0u, hi = (wi + 1 < G.twpr) ? row[wi + 1] : 0u;
            v = (lo >> 31) | (hi << 1);
            if (k == K11_TW - 1) v &= (1u << (K11_PITCH - 32 * (K11_TW - 1))) - 1u;
        }
        trav_s[j] = v;
    }
    for (int j = tid; j < K11_PITCH * K11_PITCH; j += K11_LANES) {
        const int ly = j / K11_PITCH, lx = j - ly * K11_PITCH, gx = gx0 + lx, gy = gy0 + ly;
        cost_s[j] = (gx >= 0 && gx < G.w && gy >= 0 && gy < G.h) ? G.cost[(size_t)gy * G.w + gx] : HS_NAV_UNREACHED;
    }
    if (tid == 0) nb_s = 0u;
    __syncthreads();
    if (tid == 0) cur[tile] = 0;
    // this lane's cells: column lx, rows ly0 .. ly0 + K11_ROWS - 1 of the LDS tile; the moves of each, 8 bits a cell
    const int lx = 1 + (tid & (K11_TILE - 1)), ly0 = 1 + (tid / K11_TILE) * K11_ROWS;
    unsigned long long mv_lo = 0ull, mv_hi = 0ull;                         // (two words, not an array: the sweep indexes them by a run-time row)
    bool any = false;
#pragma unroll
    for (int i = 0; i < K11_ROWS; i++) {
        const uint32_t *r = trav_s + (ly0 + i) * K11_TW;
        const uint32_t m = hs_nav_moves(hs_nav_bits3(r - K11_TW, K11_TW, lx), hs_nav_bits3(r, K11_TW, lx), hs_nav_bits3(r + K11_TW, K11_TW, lx));
        if (i < 8) mv_lo |= (unsigned long long)m << (8 * i); else mv_hi |= (unsigned long long)m << (8 * (i - 8));
        any |= m != 0u;
    }
    volatile uint32_t *col = cost_s + ly0 * K11_PITCH + lx;
    uint32_t lowered = 0u;                                                 // bit i: cell i got lower
    for (int pass = 0;; pass++) {
        bool changed = false;
        if (any) {
#pragma unroll
            for (int s = 0; s < K11_ROWS; s++) {
                const int i = (pass & 1) ? K11_ROWS - 1 - s : s;
                const uint32_t m = (uint32_t)((i < 8 ? mv_lo : mv_hi) >> (8 * (i & 7))) & 0xFFu;
                if (!m) continue;
                volatile uint32_t *p = col + i * K11_PITCH;
                const uint32_t c = *p;
                uint32_t best = c;
#pragma unroll
                for (int d = 0; d < 8; d++)
                    if ((m >> d) & 1u) {
                        const uint32_t v = hs_nav_via(p[hs_nav_dy(d) * K11_PITCH + hs_nav_dx(d)], d, G.max_cost);
                        best = v < best ? v : best;
                    }
                if (best < c) { *p = best; changed = true; lowered |= 1u << i; }
            }
        }
        if (!__syncthreads_or(changed)) break;
        if (pass >= K11_TILE * K11_TILE) { if (tid == 0) k11_overrun(G); break; }   // (uniform)
    }
    uint32_t nb = 0u;                                                      // the neighbouring tiles this lane's lowered cells touch
    const int cx = lx - 1, gx = gx0 + lx;
    for (uint32_t s = lowered; s; s &= s - 1) {
        const int i = hs_df_ctz(s), cy = ly0 + i - 1, gy = gy0 + ly0 + i;
        G.cost[(size_t)gy * G.w + gx] = col[i * K11_PITCH];                // (a lowered cell is traversable: a cell of M)
        const uint32_t l = cx == 0, r = cx == K11_TILE - 1, u = cy == 0, d = cy == K11_TILE - 1;
        nb |= l | (r << 1) | (u << 2) | (d << 3) | ((l & u) << 4) | ((r & u) << 5) | ((l & d) << 6) | ((r & d) << 7);
    }
    if (nb) atomicOr(&nb_s, nb);
    __syncthreads();
    if (tid < 8 && ((nb_s >> tid) & 1u)) {
        const int ddx = (tid == 0 || tid == 4 || tid == 6) ? -1 : (tid == 1 || tid == 5 || tid == 7) ? 1 : 0;
        const int ddy = (tid == 2 || tid == 4 || tid == 5) ? -1 : (tid == 3 || tid == 6 || tid == 7) ? 1 : 0;
        const int ntx = tx + ddx, nty = ty + ddy;
        if (ntx >= 0 && ntx < G.tiles_x && nty >= 0 && nty < G.tiles_y) {
            __hip_atomic_store(nxt + nty * G.tiles_x + ntx, (uint8_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(n_set, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// out[0 .. K11_MAX_BATCH): the flags each round of the batch set; out[K11_MAX_BATCH .. + K11_CTRS): the counter block
__global__ void __launch_bounds__(128) k11_peek(const uint32_t *__restrict__ batch, const uint32_t *__restrict__ ctr, uint32_t *__restrict__ out)
{
    const int t = threadIdx.x;
    if (t < K11_MAX_BATCH) out[t] = batch[t];
    else if (t < K11_MAX_BATCH + K11_CTRS) out[t] = ctr[t - K11_MAX_BATCH];
}

__global__ void __launch_bounds__(256) k11_dirs(const k11_geo G, int n)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    uint32_t c = HS_NAV_UNREACHED;
    if (t < n) {
        c = G.cost[t];
        uint32_t dir = c == 0u ? HS_NAV_DIR_SOURCE : HS_NAV_DIR_NONE;
        if (c != HS_NAV_UNREACHED && c != 0u) {
            const int y = t / G.w, x = t - y * G.w;
            const uint32_t *self = G.tw + (size_t)y * G.twpr;
            const uint32_t *up = y > 0 ? self - G.twpr : (const uint32_t *)nullptr, *down = y + 1 < G.h ? self + G.twpr : (const uint32_t *)nullptr;
            const uint32_t m = hs_nav_moves(hs_nav_bits3(up, G.twpr, x), hs_nav_bits3(self, G.twpr, x), hs_nav_bits3(down, G.twpr, x));
            uint32_t cn[8];
#pragma unroll
            for (int d = 0; d < 8; d++) cn[d] = ((m >> d) & 1u) ? G.cost[t + hs_nav_dy(d) * G.w + hs_nav_dx(d)] : HS_NAV_UNREACHED;   // (an allowed move ends in M)
            dir = hs_nav_dir(c, m, cn);
            if (dir == HS_NAV_DIR_NONE) k11_overrun(G);                    // the costs are no fixed point
        }
        G.dir[t] = (uint8_t)dir;
    }
    const bool reached = c != HS_NAV_UNREACHED;
    const int n_r = (int)__popcll(__ballot(reached));
    uint32_t mx = reached ? c : 0u;
    for (int off = 32; off > 0; off >>= 1) { const uint32_t o = __shfl_down(mx, off, 64); mx = o > mx ? o : mx; }
    if ((threadIdx.x & 63) == 0 && n_r) {
        __hip_atomic_fetch_add(G.ctr + K11_C_REACHED, (uint32_t)n_r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_max(G.ctr + K11_C_MAXCOST, mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// goals: rectangles {x_min, y_min, x_max, y_max} in window-frame cells
__global__ void __launch_bounds__(256) k11_goals(const k11_geo G, const int *__restrict__ goals, slamhip_nav_goal_result *__restrict__ out)
{
    __shared__ unsigned long long key_s[4];
    __shared__ int cnt_s[4];
    const int tid = threadIdx.x;
    const int *q = goals + 4 * blockIdx.x;
    long long ax0 = (long long)q[0] - G.x0, ay0 = (long long)q[1] - G.y0, ax1 = (long long)q[2] - G.x0, ay1 = (long long)q[3] - G.y0;   // the clip to M
    ax0 = ax0 < 0 ? 0 : ax0; ay0 = ay0 < 0 ? 0 : ay0;
    ax1 = ax1 > G.w - 1 ? G.w - 1 : ax1; ay1 = ay1 > G.h - 1 ? G.h - 1 : ay1;
    unsigned long long best = ~0ull;
    int cnt = 0;
    if (ax0 <= ax1 && ay0 <= ay1) {
        const int nx = (int)(ax1 - ax0 + 1), n = nx * (int)(ay1 - ay0 + 1);   // (at most 2^25)
        for (int j = tid; j < n; j += 256) {
            const int ry = j / nx, flat = ((int)ay0 + ry) * G.w + (int)ax0 + (j - ry * nx);
            const uint32_t c = G.cost[flat];
            if (c == HS_NAV_UNREACHED) continue;
            cnt++;
            const unsigned long long key = ((unsigned long long)c << 32) | (unsigned long long)(uint32_t)flat;
            best = key < best ? key : best;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_down(best, off, 64);
        best = o < best ? o : best;
        cnt += __shfl_down(cnt, off, 64);
    }
    if ((tid & 63) == 0) { key_s[tid >> 6] = best; cnt_s[tid >> 6] = cnt; }
    __syncthreads();
    if (tid == 0) {
        for (int wv = 1; wv < 4; wv++) { best = key_s[wv] < best ? key_s[wv] : best; cnt += cnt_s[wv]; }
        slamhip_nav_goal_result r;
        r.cost = HS_NAV_UNREACHED; r.bx = 0; r.by = 0; r.n_reached = cnt;
        if (cnt) {
            const int flat = (int)(uint32_t)best;
            r.cost = (uint32_t)(best >> 32); r.bx = flat % G.w + G.x0; r.by = flat / G.w + G.y0;
        }
        out[blockIdx.x] = r;
    }
}

__global__ void __launch_bounds__(64) k11_paths(const k11_geo G, const slamhip_nav_goal_result *__restrict__ res, int n_paths, int max_cells,
                                                slamhip_nav_path *__restrict__ heads, int *__restrict__ cells)
{
    const int i = threadIdx.x;
    if (i >= n_paths) return;
    slamhip_nav_path hd;
    hd.n_cells = 0; hd.n_written = 0;
    if (res[i].cost != HS_NAV_UNREACHED) {
        int x = res[i].bx - G.x0, y = res[i].by - G.y0, n = 0;
        const int cap = (int)G.ctr[K11_C_TRAV];                            // a path visits a traversable cell once
        int *out = cells + 2 * (size_t)i * (size_t)max_cells;
        for (;;) {
            if (x < 0 || x >= G.w || y < 0 || y >= G.h || n >= cap) { k11_overrun(G); break; }
            if (n < max_cells) { out[2 * n] = x + G.x0; out[2 * n + 1] = y + G.y0; }
            n++;
            const int d = G.dir[(size_t)y * G.w + x];
            if (d == HS_NAV_DIR_SOURCE) break;
            if (d > 7) { k11_overrun(G); break; }
            x += hs_nav_dx(d); y += hs_nav_dy(d);
        }
        hd.n_cells = n; hd.n_written = n < max_cells ? n : max_cells;
    }
    heads[i] = hd;
}

// (gx, gy): the rectangle's first cell in M's cells
__global__ void __launch_bounds__(256) k11_gather(const k11_geo G, int gx, int gy, int gw, int n, uint32_t *__restrict__ out_cost, uint8_t *__restrict__ out_dir)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const int ry = t / gw, rx = t - ry * gw;
    const long long x = (long long)gx + rx, y = (long long)gy + ry;
    const bool in = x >= 0 && x < G.w && y >= 0 && y < G.h;
    const size_t flat = in ? (size_t)y * G.w + (size_t)x : 0;
    if (out_cost) out_cost[t] = in ? G.cost[flat] : HS_NAV_UNREACHED;
    if (out_dir) out_dir[t] = in ? G.dir[flat] : (uint8_t)HS_NAV_DIR_NONE;
}

// the counters, the goal results and the path heads, word by word, into the pinned block
__global__ void __launch_bounds__(256) k11_emit(const uint32_t *__restrict__ ctr, const uint32_t *__restrict__ res, int res_words,
                                                const uint32_t *__restrict__ heads, int head_words, uint32_t *__restrict__ out)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < K11_CTRS) out[t] = ctr[t];
    else if (t < K11_CTRS + res_words) out[t] = res[t - K11_CTRS];
    else if (t < K11_CTRS + res_words + head_words) out[t] = heads[t - K11_CTRS - res_words];
}

// ---- host side ---------------------------------------------------------------------------------------------------
// What the field needs, made by the first call and kept: the traversable words, the cost and dir of every cell of M, the tiles'
// flags, the counters, the sources, goals, goal results, path heads and path cells in device memory, the rectangle's device block,
// a pinned, device-visible block for what the kernels store (k11_peek, k11_emit), and a second one for what is copied.
struct hs_nav {
    hs_block<uint32_t, HS_MEM_DEVICE> d_tw;
    hs_block<uint32_t, HS_MEM_DEVICE> d_cost;
    hs_block<uint8_t, HS_MEM_DEVICE> d_dir;
    hs_block<uint8_t, HS_MEM_DEVICE> d_act;
    hs_block<uint32_t, HS_MEM_DEVICE> d_ctr;
    hs_block<uint32_t, HS_MEM_DEVICE> d_batch;
    hs_block<int, HS_MEM_DEVICE> d_in;              // sources, then goals
    hs_block<unsigned char, HS_MEM_DEVICE> d_res;  // goal results, then path heads
    hs_block<int, HS_MEM_DEVICE> d_pcells;
    hs_block<unsigned char, HS_MEM_DEVICE> d_rect;   // the rectangle's costs, then its dirs
    hs_block<uint32_t, HS_MEM_PINNED_VISIBLE> h_head;     // device-visible: the peek block, then k11_emit's
    hs_block<unsigned char, HS_MEM_PINNED_VISIBLE> h_io;    // sources and goals going in; path cells and the rectangle coming out
};
#define HS_NAV_PEEK_WORDS (K11_MAX_BATCH + K11_CTRS)
#define HS_NAV_HEAD_BYTES (sizeof(uint32_t) * (HS_NAV_PEEK_WORDS + K11_CTRS + 4 * (size_t)HS_NAV_MAX_GOALS + 2 * (size_t)HS_NAV_MAX_PATHS))

// what both entry points refuse for their arguments alone
static int32_t hs_nav_check(int32_t site_mask, int32_t clearance, const int32_t *sources, int32_t S, const int32_t *goals, int32_t G,
                            const void *out_goal_results, int32_t n_paths, int32_t max_path_cells, const void *out_paths, const void *out_path_cells,
                            int32_t rw, int32_t rh, const void *out_cost, const void *out_dir)
{
    if (site_mask != 2 && site_mask != 3) SH_FAIL(SLAMHIP_ERR_INVALID, "navigation field: site_mask = %d must be 2 (obstacles) or 3 (obstacles or the unknown)", site_mask);
    if (clearance < 0 || clearance > HS_NAV_MAX_CLEARANCE) SH_FAIL(SLAMHIP_ERR_INVALID, "navigation field: clearance = %d must lie in [0, %d]", clearance, HS_NAV_MAX_CLEARANCE);
    if (S < 1 || S > HS_NAV_MAX_SOURCES) SH_FAIL(SLAMHIP_ERR_INVALID, "navigation field: S = %d sources must lie in [1, %d]", S, HS_NAV_MAX_SOURCES);
    if (!sources) SH_FAIL(SLAMHIP_ERR_INVALID, "navigation field: sources is NULL");
    if (G < 0 || G > HS_NAV_MAX_GOALS) SH_FAIL(SLAMHIP_ERR_INVALID, "navigation field: G = %d goals must lie in [0, %d]", G, HS_NAV_MAX_GOALS);
    if (G > 0 && (!goals || !out_goal_results)) SH_FAIL(SLAMHIP_ERR_INVALID, "navigation field: goals or out_goal_results is NULL with G = %d", G);
    if (n_paths < 0 || n_paths > std::min(G, HS_NAV_MAX_PATHS)) SH_FAIL(SLAMHIP_ERR_INVALID, "navigation field: n_paths = %d must lie in [0, min(G, %d)]", n_paths, HS_NAV_MAX_PATHS);
    if (max_path_cells < 1 || max_path_cells > HS_NAV_MAX_PATH_CELLS)
        SH_FAIL(SLAMHIP_ERR_INVALID, "navigation field: max_path_cells = %d must lie in [1, %d]", max_path_cells, HS_NAV_MAX_PATH_CELLS);
    if ((int64_t)n_paths * max_path_cells > HS_NAV_MAX_PATH_TOTAL) SH_FAIL(SLAMHIP_ERR_INVALID, "navigation field: n_paths * max_path_cells = %d * %d exceeds 2^20", n_paths, max_path_cells);
    if (n_paths > 0 && (!out_paths || !out_path_cells)) SH_FAIL(SLAMHIP_ERR_INVALID, "navigation field: out_paths or out_path_cells is NULL with n_paths = %d", n_paths);
    for (int i = 0; i < G; i++)
        if (goals[4 * i] > goals[4 * i + 2] || goals[4 * i + 1] > goals[4 * i + 3])
            SH_FAIL(SLAMHIP_ERR_INVALID, "navigation field: goal %d is the inverted rectangle (%d, %d) .. (%d, %d)", i, goals[4 * i], goals[4 * i + 1], goals[4 * i + 2], goals[4 * i + 3]);
    if ((out_cost || out_dir) && (rw < 1 || rh < 1 || (int64_t)rw * rh > HS_NAV_MAX_RECT))
        SH_FAIL(SLAMHIP_ERR_INVALID, "navigation field: a rectangle of %d x %d cells; rw, rh >= 1 and rw * rh <= 2^24", rw, rh);
    return SLAMHIP_OK;
}

static void hs_nav_summary_of(const uint32_t *ctr, int x0, int y0, int w, int h, int rounds, slamhip_nav_summary *S)
{
    S->mx0 = x0; S->my0 = y0; S->mw = w; S->mh = h;
    S->n_traversable = (int32_t)ctr[K11_C_TRAV]; S->n_reached = (int32_t)ctr[K11_C_REACHED];
    S->n_sources_used = (int32_t)ctr[K11_C_USED]; S->n_sources_blocked = (int32_t)ctr[K11_C_BLOCKED];
    S->max_cost_reached = ctr[K11_C_MAXCOST]; S->rounds = rounds;
}

// What slamhip_hs_nav_field refuses for its spec and sources alone (slamhip_hs_rollouts refuses the same).
int32_t hs_nav_check_field(int n_levels, const slamhip_nav_spec *spec, const int32_t *sources, int32_t S)
{
    if (spec->level < 0 || spec->level >= n_levels) SH_FAIL(SLAMHIP_ERR_INVALID, "navigation field: level %d of %d", spec->level, n_levels);
    if (spec->world != 0 && spec->world != 1) SH_FAIL(SLAMHIP_ERR_INVALID, "navigation field: world = %d must be 0 (the window) or 1 (the world)", spec->world);
    return hs_nav_check(spec->site_mask, spec->clearance, sources, S, nullptr, 0, nullptr, 0, 1, nullptr, nullptr, 0, 0, nullptr, nullptr);
}

// what the field's build leaves for the launches behind it
struct hs_nav_built { k11_geo A; hs_class_map M; int64_t cells; int rounds; const int *d_goals; size_t src_bytes, goal_bytes; };

// Steps 1 to 4 of the definition on the operator's stream -- the class map, the field for a clearance, k11_trav, k11_seed and the
// relaxation rounds with their batch waits -- for slamhip_hs_nav_field and slamhip_hs_rollouts alike: when it returns the costs of
// every cell of M are final in device memory and the stream has drained.  The arguments are checked by the caller.  goals: G
// rectangles copied behind the sources; pc_bytes, rc_bytes, rd_bytes: the path cells and the rectangle the caller will ask for.
static int32_t hs_nav_build(slamhip_hs *hs, const slamhip_nav_spec *spec, const int32_t *sources, int32_t S, const int32_t *goals, int32_t G,
                            size_t pc_bytes, size_t rc_bytes, size_t rd_bytes, hs_nav_built *out)
{
    const int level = spec->level, c = spec->clearance;
    const bool world = spec->world != 0;
    slamhip_ctx *ctx = hs->ctx;
    SH_TRY(hs_call_begin(hs));
    hs_class_map M;
    hs_field E = { nullptr, 0, 0, 0, 0, 0, 0u };                           // (no clearance: no field)
    if (c >= 1) SH_TRY(hs_df_field_prepare(hs, level, world, spec->site_mask, c + 1, &M, &E));
    else SH_TRY(hs_lat_pack_prepare(hs, level, world, &M));
    const int64_t cells = (int64_t)M.w * M.h;
    if (cells > HS_NAV_MAX_M) SH_FAIL(SLAMHIP_ERR_INVALID, "navigation field: M, the class map of level %d, is %d x %d cells, more than 2^25", level, M.w, M.h);
    SH_TRY(hs_unit<&slamhip_hs::nav>(hs));
    hs_nav *nv = hs->nav;
    k11_geo A;
    A.cls = M.cls; A.w = M.w; A.h = M.h; A.wpr = M.wpr;
    A.f = E.f; A.fpitch = E.pitch; A.fr = c >= 1 ? c + 1 : 0; A.c2 = (uint32_t)(c * c);
    A.twpr = (M.w + 31) / 32;
    A.tiles_x = sh_div_up(M.w, K11_TILE); A.tiles_y = sh_div_up(M.h, K11_TILE);
    A.max_cost = spec->max_cost; A.x0 = M.x0; A.y0 = M.y0;
    const int nt = A.tiles_x * A.tiles_y;
    const size_t src_bytes = sizeof(int) * 2 * (size_t)S, goal_bytes = sizeof(int) * 4 * (size_t)G;
    const size_t act_bytes = ((size_t)2 * nt + 15) & ~(size_t)15;
    SH_TRY(nv->d_tw.grow(sizeof(uint32_t) * (size_t)A.twpr * M.h, "navigation field"));
    SH_TRY(nv->d_cost.grow(sizeof(uint32_t) * (size_t)cells, "navigation field"));
    SH_TRY(nv->d_dir.grow((size_t)cells, "navigation field"));
    SH_TRY(nv->d_act.grow(act_bytes, "navigation field"));
    SH_TRY(nv->d_ctr.grow(sizeof(uint32_t) * K11_CTRS, "navigation field"));
    SH_TRY(nv->d_batch.grow(sizeof(uint32_t) * K11_MAX_BATCH, "navigation field"));
    SH_TRY(nv->d_in.grow(src_bytes + goal_bytes, "navigation field"));
    SH_TRY(nv->d_res.grow(sizeof(slamhip_nav_goal_result) * (size_t)HS_NAV_MAX_GOALS + sizeof(slamhip_nav_path) * HS_NAV_MAX_PATHS, "navigation field"));
    if (pc_bytes) SH_TRY(nv->d_pcells.grow(pc_bytes, "navigation field"));
    if (rc_bytes + rd_bytes) SH_TRY(nv->d_rect.grow(rc_bytes + rd_bytes, "navigation field"));
    SH_TRY(nv->h_head.grow(HS_NAV_HEAD_BYTES, "navigation field"));
    SH_TRY(nv->h_io.grow(std::max(src_bytes + goal_bytes, pc_bytes + rc_bytes + rd_bytes), "navigation field"));
    A.tw = nv->d_tw; A.cost = nv->d_cost; A.dir = nv->d_dir; A.act = nv->d_act; A.ctr = nv->d_ctr;
    int *d_src = nv->d_in;
    const int batch = (int)std::min<long long>(std::max<long long>(sh_env_int("SLAMHIP_NAV_BATCH", K11_BATCH), 1), K11_MAX_BATCH);
    hipStream_t st = ctx->stream;
    memcpy(nv->h_io, sources, src_bytes);
    if (G) memcpy(nv->h_io + src_bytes, goals, goal_bytes);
    SH_HIP(hipMemcpyAsync(nv->d_in, nv->h_io, src_bytes + goal_bytes, hipMemcpyHostToDevice, st));
    SH_HIP(hipMemsetAsync(nv->d_ctr, 0, sizeof(uint32_t) * K11_CTRS, st));
    SH_HIP(hipMemsetAsync(nv->d_act, 0, act_bytes, st));
    SH_HIP(hipMemsetAsync(nv->d_cost, 0xFF, sizeof(uint32_t) * (size_t)cells, st));
    if (c >= 1) SH_TRY(hs_df_field_enqueue(hs, level, world, &M, &E, spec->site_mask));
    else SH_TRY(hs_lat_pack_enqueue(hs, level, world, &M));
    // (at most 2^25 cells in M: no grid reaches 2^31 workgroups)
    hipLaunchKernelGGL(k11_trav, dim3((unsigned)sh_div_up(A.twpr * M.h, 256)), dim3(256), 0, st, A);
    SH_HIP(hipGetLastError());
    hipLaunchKernelGGL(k11_seed, dim3((unsigned)sh_div_up(S, 256)), dim3(256), 0, st, A, (const int *)d_src, S);
    SH_HIP(hipGetLastError());
    const uint32_t *peek = nv->h_head;
    int rounds = 0;
    for (int64_t issued = 0;;) {
        SH_HIP(hipMemsetAsync(nv->d_batch, 0, sizeof(uint32_t) * K11_MAX_BATCH, st));
        for (int j = 0; j < batch; j++) {
            hipLaunchKernelGGL(k11_relax, dim3((unsigned)nt), dim3(K11_LANES), 0, st, A, (int)((issued + j) & 1), nv->d_batch + j);
            SH_HIP(hipGetLastError());
        }
        hipLaunchKernelGGL(k11_peek, dim3(1), dim3(128), 0, st, (const uint32_t *)nv->d_batch, (const uint32_t *)nv->d_ctr, nv->h_head);
        SH_HIP(hipGetLastError());
        SH_TRY(hs_call_finish(hs));
        if (peek[K11_MAX_BATCH + K11_C_FLAG]) SH_FAIL(SLAMHIP_ERR_STATE, "navigation field did not converge: a tile's relaxation overran (level %d, M of %d x %d cells)", level, M.w, M.h);
        int j = 0;
        while (j < batch && peek[j]) j++;
        if (j < batch) { rounds = (int)(issued + j + 1); break; }          // round j set no flag: nothing is active any more
        issued += batch;
        if (issued > (int64_t)peek[K11_MAX_BATCH + K11_C_TRAV] + 1)        // (a shortest path is simple: it crosses tile borders fewer times than it has cells)
            SH_FAIL(SLAMHIP_ERR_STATE, "navigation field did not converge in %lld rounds (level %d, M of %d x %d cells)", (long long)issued, level, M.w, M.h);
    }
    out->A = A; out->M = M; out->cells = cells; out->rounds = rounds;
    out->d_goals = nv->d_in + 2 * (size_t)S; out->src_bytes = src_bytes; out->goal_bytes = goal_bytes;
    return SLAMHIP_OK;
}

// The field for slamhip_hs_rollouts (hs_rollout.hip): hs_nav_build with no goals, no paths and no rectangle.
int32_t hs_nav_field_for_rollouts(slamhip_hs *hs, const slamhip_nav_spec *spec, const int32_t *sources, int32_t S, hs_nav_view *out)
{
    hs_nav_built Bt;
    SH_TRY(hs_nav_build(hs, spec, sources, S, nullptr, 0, 0, 0, 0, &Bt));
    out->tw = Bt.A.tw; out->cost = Bt.A.cost; out->ctr = Bt.A.ctr; out->twpr = Bt.A.twpr; out->M = Bt.M; out->rounds = Bt.rounds;
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_nav_field(slamhip_hs *hs, const slamhip_nav_spec *spec, const int32_t *sources, int32_t S, const int32_t *goals,
                                        int32_t G, slamhip_nav_goal_result *out_goal_results, int32_t n_paths, int32_t max_path_cells,
                                        slamhip_nav_path *out_paths, int32_t *out_path_cells, int32_t rx, int32_t ry, int32_t rw, int32_t rh,
                                        uint32_t *out_cost, uint8_t *out_dir, slamhip_nav_summary *out_summary)
{
    SH_CHECK_ARG(hs && spec && out_summary);
    const int level = spec->level;
    if (level < 0 || level >= hs->n_levels) SH_FAIL(SLAMHIP_ERR_INVALID, "navigation field: level %d of %d", level, hs->n_levels);
    if (spec->world != 0 && spec->world != 1) SH_FAIL(SLAMHIP_ERR_INVALID, "navigation field: world = %d must be 0 (the window) or 1 (the world)", spec->world);
    SH_TRY(hs_nav_check(spec->site_mask, spec->clearance, sources, S, goals, G, out_goal_results, n_paths, max_path_cells, out_paths, out_path_cells, rw, rh, out_cost, out_dir));
    const bool rect = out_cost || out_dir;
    const int n_rect = rect ? rw * rh : 0;
    const size_t pc_bytes = sizeof(int) * 2 * (size_t)n_paths * (size_t)max_path_cells;
    const size_t rc_bytes = out_cost ? sizeof(uint32_t) * (size_t)n_rect : 0, rd_bytes = out_dir ? ((size_t)n_rect + 3) & ~(size_t)3 : 0;
    hs_nav_built Bt;
    SH_TRY(hs_nav_build(hs, spec, sources, S, goals, G, pc_bytes, rc_bytes, rd_bytes, &Bt));
    slamhip_ctx *ctx = hs->ctx;
    hs_nav *nv = hs->nav;
    const k11_geo &A = Bt.A;
    const hs_class_map &M = Bt.M;
    const int64_t cells = Bt.cells;
    const int rounds = Bt.rounds;
    const int *d_goals = Bt.d_goals;
    slamhip_nav_goal_result *d_res = (slamhip_nav_goal_result *)nv->d_res.p;
    slamhip_nav_path *d_heads = (slamhip_nav_path *)(nv->d_res + sizeof(slamhip_nav_goal_result) * (size_t)HS_NAV_MAX_GOALS);
    hipStream_t st = ctx->stream;
    const uint32_t *head = nv->h_head + HS_NAV_PEEK_WORDS;
    hipLaunchKernelGGL(k11_dirs, dim3((unsigned)sh_div_up((int)cells, 256)), dim3(256), 0, st, A, (int)cells);
    SH_HIP(hipGetLastError());
    if (G) {
        hipLaunchKernelGGL(k11_goals, dim3((unsigned)G), dim3(256), 0, st, A, (const int *)d_goals, d_res);
        SH_HIP(hipGetLastError());
    }
    if (n_paths) {
        hipLaunchKernelGGL(k11_paths, dim3(1), dim3(64), 0, st, A, (const slamhip_nav_goal_result *)d_res, n_paths, max_path_cells, d_heads, nv->d_pcells);
        SH_HIP(hipGetLastError());
        SH_HIP(hipMemcpyAsync(nv->h_io, nv->d_pcells, pc_bytes, hipMemcpyDeviceToHost, st));
    }
    if (rect) {
        const int64_t far = (int64_t)1 << 30;                              // (a rectangle that far from M lies outside it; -2^28 < x0 <= 0)
        const int gx = (int)std::min(std::max((int64_t)rx - M.x0, -far), far), gy = (int)std::min(std::max((int64_t)ry - M.y0, -far), far);
        hipLaunchKernelGGL(k11_gather, dim3((unsigned)sh_div_up(n_rect, 256)), dim3(256), 0, st, A, gx, gy, rw, n_rect,
                           out_cost ? (uint32_t *)nv->d_rect.p : (uint32_t *)nullptr, out_dir ? (uint8_t *)(nv->d_rect + rc_bytes) : (uint8_t *)nullptr);
        SH_HIP(hipGetLastError());
        SH_HIP(hipMemcpyAsync(nv->h_io + pc_bytes, nv->d_rect, rc_bytes + rd_bytes, hipMemcpyDeviceToHost, st));
    }
    hipLaunchKernelGGL(k11_emit, dim3((unsigned)sh_div_up(K11_CTRS + 4 * G + 2 * n_paths, 256)), dim3(256), 0, st, (const uint32_t *)nv->d_ctr,
                       (const uint32_t *)d_res, 4 * G, (const uint32_t *)d_heads, 2 * n_paths, nv->h_head + HS_NAV_PEEK_WORDS);
    SH_HIP(hipGetLastError());
    SH_TRY(hs_call_finish(hs));
    if (head[K11_C_FLAG]) SH_FAIL(SLAMHIP_ERR_STATE, "navigation field did not converge: the costs are no fixed point (level %d, M of %d x %d cells)", level, M.w, M.h);
    hs_nav_summary_of(head, M.x0, M.y0, M.w, M.h, rounds, out_summary);
    if (G) memcpy(out_goal_results, head + K11_CTRS, sizeof(slamhip_nav_goal_result) * (size_t)G);
    if (n_paths) {
        const slamhip_nav_path *hd = (const slamhip_nav_path *)(head + K11_CTRS + 4 * (size_t)G);
        memcpy(out_paths, hd, sizeof(slamhip_nav_path) * (size_t)n_paths);
        for (int i = 0; i < n_paths; i++)
            memcpy(out_path_cells + 2 * (size_t)i * max_path_cells, nv->h_io + sizeof(int) * 2 * (size_t)i * max_path_cells, sizeof(int) * 2 * (size_t)hd[i].n_written);
    }
    if (out_cost) memcpy(out_cost, nv->h_io + pc_bytes, rc_bytes);
    if (out_dir) memcpy(out_dir, nv->h_io + pc_bytes + rc_bytes, (size_t)n_rect);
    return SLAMHIP_OK;
}

// Steps 1 to 4 over a caller's class array for the two hooks (hs_nav_host.h): the traversable words, the costs by Dijkstra and three
// of the counters.
int32_t hs_nav_debug_costs(const uint8_t *cls, int32_t cw, int32_t ch, int32_t site_mask, int32_t clearance, uint32_t max_cost, const int32_t *sources,
                           int32_t S, std::vector<uint32_t> &tw, std::vector<uint32_t> &cost, uint32_t ctr[K11_CTRS])
{
    const int wpr = (cw + 15) / 16, twpr = (cw + 31) / 32;
    const size_t cells = (size_t)cw * ch;
    std::vector<uint32_t> packed((size_t)wpr * ch, 0u);
    tw.assign((size_t)twpr * ch, 0u);
    for (int cy = 0; cy < ch; cy++)
        for (int cx = 0; cx < cw; cx++) packed[(size_t)cy * wpr + (cx >> 4)] |= (uint32_t)(cls[(size_t)cy * cw + cx] & 3u) << (2 * (cx & 15));
    std::vector<uint16_t> F;
    if (clearance >= 1) {
        F.resize(cells);
        SH_TRY(slamhip_debug_distance_field(cls, cw, ch, site_mask, clearance + 1, 0, 0, cw, ch, F.data()));
    }
    for (int y = 0; y < ch; y++)
        for (int j = 0; j < twpr; j++) {
            const uint32_t t = hs_nav_trav_word(packed.data() + (size_t)y * wpr, cw, 32 * j, clearance >= 1 ? F.data() + (size_t)y * cw + 32 * j : (const uint16_t *)nullptr,
                                                (uint32_t)(clearance * clearance));
            tw[(size_t)y * twpr + j] = t;
            ctr[K11_C_TRAV] += (uint32_t)__builtin_popcount(t);
        }
    auto moves = [&](int x, int y) {
        const uint32_t *self = tw.data() + (size_t)y * twpr;
        const uint32_t *up = y > 0 ? self - twpr : (const uint32_t *)nullptr, *down = y + 1 < ch ? self + twpr : (const uint32_t *)nullptr;
        return hs_nav_moves(hs_nav_bits3(up, twpr, x), hs_nav_bits3(self, twpr, x), hs_nav_bits3(down, twpr, x));
    };
    cost.assign(cells, HS_NAV_UNREACHED);
    typedef std::pair<uint32_t, int> item;
    std::priority_queue<item, std::vector<item>, std::greater<item>> heap;
    for (int i = 0; i < S; i++) {
        const int x = sources[2 * i], y = sources[2 * i + 1];
        if (x < 0 || x >= cw || y < 0 || y >= ch || !hs_nav_bit(tw.data() + (size_t)y * twpr, twpr, x)) { ctr[K11_C_BLOCKED]++; continue; }
        ctr[K11_C_USED]++;
        if (cost[(size_t)y * cw + x] != 0u) { cost[(size_t)y * cw + x] = 0u; heap.push(item(0u, y * cw + x)); }
    }
    while (!heap.empty()) {
        const item it = heap.top();
        heap.pop();
        if (it.first != cost[(size_t)it.second]) continue;                 // a stale entry
        const int y = it.second / cw, x = it.second - y * cw;
        const uint32_t m = moves(x, y);
        for (int d = 0; d < 8; d++) {
            if (!((m >> d) & 1u)) continue;
            const int n = it.second + hs_nav_dy(d) * cw + hs_nav_dx(d);
            const uint32_t v = hs_nav_via(it.first, d, max_cost);
            if (v < cost[(size_t)n]) { cost[(size_t)n] = v; heap.push(item(v, n)); }
        }
    }
    return SLAMHIP_OK;
}

// CPU-side test hook: the field of the definition over a caller's class array, M = (0, 0, cw, ch).  The classes are packed as K7
// packs them and the field for a clearance comes from slamhip_debug_distance_field; the traversable words, the moves and the dirs
// are hs_nav.h's -- the text the kernels run -- but the costs come from a plain sequential Dijkstra with a binary heap, not from
// the tiled relaxation.
extern "C" int32_t slamhip_debug_nav_field(const uint8_t *cls, int32_t cw, int32_t ch, int32_t site_mask, int32_t clearance, uint32_t max_cost,
                                           const int32_t *sources, int32_t S, const int32_t *goals, int32_t G,
                                           slamhip_nav_goal_result *out_goal_results, int32_t n_paths, int32_t max_path_cells,
                                           slamhip_nav_path *out_paths, int32_t *out_path_cells, int32_t rx, int32_t ry, int32_t rw, int32_t rh,
                                           uint32_t *out_cost, uint8_t *out_dir, slamhip_nav_summary *out_summary)
{
    SH_CHECK_ARG(cls && out_summary);
    if (cw < 1 || ch < 1 || (int64_t)cw * ch > HS_NAV_MAX_M)
        SH_FAIL(SLAMHIP_ERR_INVALID, "navigation field: a class array of %d x %d cells; cw, ch >= 1 and cw * ch <= 2^25", cw, ch);
    SH_TRY(hs_nav_check(site_mask, clearance, sources, S, goals, G, out_goal_results, n_paths, max_path_cells, out_paths, out_path_cells, rw, rh, out_cost, out_dir));
    const int twpr = (cw + 31) / 32;
    const size_t cells = (size_t)cw * ch;
    std::vector<uint32_t> tw, cost;
    uint32_t ctr[K11_CTRS] = { 0 };
    SH_TRY(hs_nav_debug_costs(cls, cw, ch, site_mask, clearance, max_cost, sources, S, tw, cost, ctr));
    auto moves = [&](int x, int y) {
        const uint32_t *self = tw.data() + (size_t)y * twpr;
        const uint32_t *up = y > 0 ? self - twpr : (const uint32_t *)nullptr, *down = y + 1 < ch ? self + twpr : (const uint32_t *)nullptr;
        return hs_nav_moves(hs_nav_bits3(up, twpr, x), hs_nav_bits3(self, twpr, x), hs_nav_bits3(down, twpr, x));
    };
    std::vector<uint8_t> dir(cells);
    for (int y = 0; y < ch; y++)
        for (int x = 0; x < cw; x++) {
            const size_t t = (size_t)y * cw + x;
            const uint32_t c = cost[t], m = (c != HS_NAV_UNREACHED && c != 0u) ? moves(x, y) : 0u;
            uint32_t cn[8];
            for (int d = 0; d < 8; d++) cn[d] = ((m >> d) & 1u) ? cost[t + hs_nav_dy(d) * cw + hs_nav_dx(d)] : HS_NAV_UNREACHED;
            dir[t] = (uint8_t)hs_nav_dir(c, m, cn);
            if (c != HS_NAV_UNREACHED) { ctr[K11_C_REACHED]++; ctr[K11_C_MAXCOST] = std::max(ctr[K11_C_MAXCOST], c); }
        }
    hs_nav_summary_of(ctr, 0, 0, cw, ch, 0, out_summary);
    for (int g = 0; g < G; g++) {
        const int *q = goals + 4 * g;
        slamhip_nav_goal_result r;
        r.cost = HS_NAV_UNREACHED; r.bx = 0; r.by = 0; r.n_reached = 0;
        for (int y = std::max(q[1], 0); y <= std::min(q[3], ch - 1); y++)
            for (int x = std::max(q[0], 0); x <= std::min(q[2], cw - 1); x++) {
                const uint32_t c = cost[(size_t)y * cw + x];
                if (c == HS_NAV_UNREACHED) continue;
                r.n_reached++;
                if (c < r.cost) { r.cost = c; r.bx = x; r.by = y; }       // (row-major order: the first of equal costs stays)
            }
        out_goal_results[g] = r;
    }
    for (int i = 0; i < n_paths; i++) {
        const slamhip_nav_goal_result &r = out_goal_results[i];
        int n = 0;
        if (r.cost != HS_NAV_UNREACHED)
            for (int x = r.bx, y = r.by;;) {
                if (n < max_path_cells) { out_path_cells[2 * ((size_t)i * max_path_cells + n)] = x; out_path_cells[2 * ((size_t)i * max_path_cells + n) + 1] = y; }
                n++;
                const int d = dir[(size_t)y * cw + x];
                if (d == HS_NAV_DIR_SOURCE) break;
                if (d > 7 || n > (int)ctr[K11_C_TRAV]) SH_FAIL(SLAMHIP_ERR_STATE, "navigation field: the path of goal %d does not end at a source", i);
                x += hs_nav_dx(d); y += hs_nav_dy(d);
            }
        out_paths[i].n_cells = n; out_paths[i].n_written = std::min(n, max_path_cells);
    }
    if (out_cost || out_dir)
        for (int j = 0; j < rh; j++)
            for (int i = 0; i < rw; i++) {
                const int64_t x = (int64_t)rx + i, y = (int64_t)ry + j;
                const bool in = x >= 0 && x < cw && y >= 0 && y < ch;
                if (out_cost) out_cost[(size_t)j * rw + i] = in ? cost[(size_t)y * cw + (size_t)x] : HS_NAV_UNREACHED;
                if (out_dir) out_dir[(size_t)j * rw + i] = in ? dir[(size_t)y * cw + (size_t)x] : (uint8_t)HS_NAV_DIR_NONE;
            }
    return SLAMHIP_OK;
}
