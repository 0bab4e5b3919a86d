// hs_bnb.hip -- K24, the branch-and-bound pose-lattice search of HectorSLAM: K7's keys without scoring every node
// (slamhip_hs_lattice_search_bnb, slamhip_hs_relocalise_bnb, slamhip_debug_lattice_bnb).  No reference counterpart.  Definition:
// include/slamhip.h (slamhip_bnb_spec, rules 1 - 7); the arithmetic host and device share: hs_bnb.h; the class map, its world
// variant and the point cells are K7's (hs_lattice.hip, hs_lattice.h), used and not copied.
//
// The launches of one call, on the operator's stream:
//  * K7's pack (k7_pack or k7_pack_world) into K7's class map.
//  * k24_pool, once per height 0 .. top.  Height 0 copies the class map into the unit's FRAME (hs_bnb_frame): the map behind a zero
//    margin of whole words in x and 2^top - 1 rows in y, because a window that starts off the map can still reach into it, and zero is
//    "neither", which is what rule 2 says of the outside.  Height h doubles the window: P_h = the maximum of P_(h-1) at the four
//    offsets {0, 2^(h-1)}^2.  On the packed 2-bit codes (1 occupied, 0 neither, 2 free) the maximum BY VALUE is word logic -- the low
//    bit is the OR of the low bits, the high bit the AND of the high bits -- so a lane handles a whole 16-cell word with a funnel
//    shift across the neighbouring word for the x offset; nothing is unpacked.
//  * per level h = top .. 0, k24_score: a lane per block, a workgroup of 256 lanes serves ONE heading -- the top level is a regular
//    grid (blockIdx.y the heading), a lower level reads a frontier grouped by heading through a job table that maps a workgroup to
//    (heading, slice of its segment).  The heading's point cells are formed once per workgroup, chunk by chunk (K24_CHUNK points)
//    into LDS, and read as broadcasts; per point a lane gathers one word of P_h and one of P_0 from global memory, where the pooled
//    maps of a level stay in L2 / MALL (2048^2 packed is 1 MB per height).  U goes to the level's array, the key of (E, origin's
//    flat) through a wave maximum and the wavefronts' maxima in LDS into ONE 64-bit maximum at agent scope on key[k], as in K7.
//  * for h > 0, k24_filter: behind the WHOLE level's score launch -- rule 4's "after the whole level" is the launch boundary -- the
//    survivors and their children are counted per heading (a workgroup scan, one 32-bit add per workgroup); the counts go to the
//    host, which waits (the level's one wait), forms the segments' offsets and the next job table and checks rule 5; then k24_emit
//    writes the children into their heading's segment: a workgroup scan and one add on the heading's cursor per workgroup.  The order
//    inside a segment depends on the adds' arrival; no output depends on it.
// Left out: staging a rectangle of the pooled maps in LDS as K7 does, and a wavefront-per-block form for thin frontiers.
#include "hs_blocks.h"
#include "hs_bnb.h"
#include <math.h>
#include <vector>

#define K24_LANES 256
#define K24_CHUNK 1024                     // points per LDS chunk (8 KB)
// (gx, gy) of an ignored point in LDS.  The walk adds a - nx + mx (|.| <= 4096 + 8192 + 256) to it: the sum stays negative -- outside
// every frame -- and far from overflow.  A point that counts has |gx| < 2^24 and -2^28 < x0 <= 0 (K7's bound on R), so gx - x0 plus
// that offset does not overflow either.
#define K24_IGNORED (-(1 << 30))

struct k24_job { int32_t k, first, n, pad; };   // a workgroup of a lower level: heading, its first block in the frontier, how many (<= K24_LANES)

struct k24_arg {
    const float2 *pts; int n;
    const uint32_t *maps; hs_bnb_frame F;  // P_0 .. P_top, F.words each
    int x0, y0;                            // the class map's first cell in the window's frame: (0, 0), or R's origin
    float stm;
    slamhip_lattice_spec S;
    int h;                                 // the level's height
    int gx, gcount;                        // the top level (front == nullptr): blocks per grid row and per heading; block idx = k * gcount + i
    const uint32_t *front; const k24_job *jobs;   // a lower level: the packed blocks grouped by heading, and the job table
    int32_t *u;                            // U of every block of the level, by the block's index
    unsigned long long *keys;
    int32_t *counts;                       // k24_filter: {survivors, children} per heading
    const int32_t *off; int32_t *cursor;   // k24_emit: a heading's segment starts at off[k]; cursor[k] children have been placed
    uint32_t *next; int next_cap;
};

__global__ void __launch_bounds__(256) k24_pool(const uint32_t *__restrict__ cls, int cw, uint32_t *__restrict__ maps, const hs_bnb_frame F, int h)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= F.words) return;
    const int y = (int)(i / (size_t)F.wpr), wx = (int)(i - (size_t)y * F.wpr);
    uint32_t *out = maps + (size_t)h * F.words;
    if (h == 0) {                                                          // the class map behind its margin (F.wpr = cw + mx / 16, F.rows = the map's + my)
        const int sy = y - F.my, sx = wx - F.mx / 16;
        out[i] = sy >= 0 && sx >= 0 ? cls[(size_t)sy * cw + sx] : 0u;
    } else out[i] = hs_bnb_pool_word(maps + (size_t)(h - 1) * F.words, F.wpr, F.rows, y, wx, 1 << (h - 1));
}

// which heading this workgroup serves, the index of its first block and how many blocks it has (uniform)
__device__ static __forceinline__ void k24_locate(const k24_arg &A, int *k, int *first, int *cnt)
{
    if (A.front) {
        const k24_job J = A.jobs[blockIdx.x];
        *k = J.k; *first = J.first; *cnt = J.n;
    } else {
        const int i0 = blockIdx.x * K24_LANES;
        *k = blockIdx.y; *first = blockIdx.y * A.gcount + i0; *cnt = min(K24_LANES, A.gcount - i0);
    }
}
__device__ static __forceinline__ void k24_block(const k24_arg &A, int k, int idx, int *a, int *b)
{
    if (A.front) { const uint32_t p = A.front[idx]; *a = hs_bnb_a(p); *b = hs_bnb_b(p); }
    else { const int i = idx - k * A.gcount, r = i / A.gx; *a = (i - r * A.gx) << A.h; *b = r << A.h; }
}

// The walk of one lane over m points: E, the sum in P_0, and with BOTH also U, the sum in P_h, of the frame cells (g.x + ox, g.y + oy).
template <bool BOTH>
__device__ static __forceinline__ void k24_walk(const uint32_t *__restrict__ p0, const uint32_t *__restrict__ ph, const hs_bnb_frame &F, const int2 *pts, int m,
                                                int ox, int oy, int *E, int *U)
{
    int e = 0, u = 0;
    const int wc = F.wpr * 16;
#pragma unroll 4
    for (int j = 0; j < m; j++) {
        const int2 g = pts[j];
        const int x = g.x + ox, y = g.y + oy;
        const bool in = (unsigned)x < (unsigned)wc && (unsigned)y < (unsigned)F.rows;
        const size_t o = in ? (size_t)y * F.wpr + (size_t)(x >> 4) : (size_t)0;
        const int sh = (x & 15) * 2;
        e += hs_lat_class_value(in ? (p0[o] >> sh) & 3u : 0u);
        if constexpr (BOTH) u += hs_lat_class_value(in ? (ph[o] >> sh) & 3u : 0u);
    }
    *E += e; *U += u;
}

__global__ void __launch_bounds__(K24_LANES) k24_score(const k24_arg A)
{
    __shared__ int2 pts_s[K24_CHUNK];
    __shared__ unsigned long long wmax_s[K24_LANES / 64];
    const int tid = threadIdx.x;
    int k, first, cnt;
    k24_locate(A, &k, &first, &cnt);
    const bool active = tid < cnt;
    const int idx = first + tid;
    int a = 0, b = 0;
    if (active) k24_block(A, k, idx, &a, &b);
    const hs_lat_heading H = hs_lat_heading_of(A.stm, A.S.centre[0], A.S.centre[1], hs_lat_theta(A.S, k));
    const int ox = a - A.S.nx + A.F.mx, oy = b - A.S.ny + A.F.my;
    const uint32_t *p0 = A.maps, *ph = A.maps + (size_t)A.h * A.F.words;
    int E = 0, U = 0;
    for (int base = 0; base < A.n; base += K24_CHUNK) {
        const int m = min(K24_CHUNK, A.n - base);
        if (base > 0) __syncthreads();                                     // (the previous chunk has been walked)
        for (int i = tid; i < m; i += K24_LANES) {
            const float2 p = A.pts[base + i];
            int gx, gy;
            if (!hs_lat_point_cell(H, p.x, p.y, &gx, &gy)) { gx = K24_IGNORED; gy = K24_IGNORED; }
            else { gx -= A.x0; gy -= A.y0; }                               // (integers: exact)
            pts_s[i] = make_int2(gx, gy);
        }
        __syncthreads();
        if (active) {
            if (A.h > 0) k24_walk<true>(p0, ph, A.F, pts_s, m, ox, oy, &E, &U);
            else k24_walk<false>(p0, ph, A.F, pts_s, m, ox, oy, &E, &U);
        }
    }
    if (active && A.h > 0) A.u[idx] = U;
    const uint32_t flat = (uint32_t)(b * (2 * A.S.nx + 1) + a);           // the origin node: ix + nx = a, iy + ny = b
    unsigned long long key = active ? hs_lat_key(E, flat) : 0ull;          // (a node's key is never 0: its high word is at least 1)
    for (int msk = 1; msk < 64; msk <<= 1) {
        const unsigned long long o = __shfl_xor(key, msk);
        key = o > key ? o : key;
    }
    if ((tid & 63) == 0) wmax_s[tid >> 6] = key;
    __syncthreads();
    if (tid == 0) {
        for (int v = 1; v < K24_LANES / 64; v++) key = wmax_s[v] > key ? wmax_s[v] : key;
        __hip_atomic_fetch_max(A.keys + k, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// the exclusive prefix of v over the workgroup's lanes and the workgroup's total (ws: one word per wavefront; a barrier inside)
__device__ static __forceinline__ int k24_wg_scan(int v, int *ws, int *total)
{
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(inc, d);
        if (lane >= d) inc += o;
    }
    if (lane == 63) ws[wv] = inc;
    __syncthreads();
    int base = 0, tot = 0;
    for (int i = 0; i < K24_LANES / 64; i++) { const int s = ws[i]; if (i < wv) base += s; tot += s; }
    *total = tot;
    return base + inc - v;
}

// rule 4 for this lane's block, by the keys as the level's score launch left them: how many children it has (0: it does not survive)
__device__ static __forceinline__ int k24_children_of(const k24_arg &A, int k, int idx, bool active, int *a, int *b)
{
    *a = 0; *b = 0;
    if (!active) return 0;
    k24_block(A, k, idx, a, b);
    const int best = hs_bnb_key_score(A.keys[k]);
    return hs_bnb_survives(A.h, A.u[idx], best) ? hs_bnb_children(*a, *b, A.h, A.S.nx, A.S.ny) : 0;
}

__global__ void __launch_bounds__(K24_LANES) k24_filter(const k24_arg A)
{
    __shared__ int ws_s[2][K24_LANES / 64];
    int k, first, cnt, a, b, kept, children;
    k24_locate(A, &k, &first, &cnt);
    const int c = k24_children_of(A, k, first + (int)threadIdx.x, (int)threadIdx.x < cnt, &a, &b);
    (void)k24_wg_scan(c > 0 ? 1 : 0, ws_s[0], &kept);
    (void)k24_wg_scan(c, ws_s[1], &children);
    if (threadIdx.x == 0 && kept) { atomicAdd(A.counts + 2 * k, kept); atomicAdd(A.counts + 2 * k + 1, children); }
}

__global__ void __launch_bounds__(K24_LANES) k24_emit(const k24_arg A)
{
    __shared__ int ws_s[K24_LANES / 64];
    __shared__ int base_s;
    int k, first, cnt, a, b, total;
    k24_locate(A, &k, &first, &cnt);
    const int c = k24_children_of(A, k, first + (int)threadIdx.x, (int)threadIdx.x < cnt, &a, &b);
    const int mine = k24_wg_scan(c, ws_s, &total);
    if (total == 0) return;                                                // (uniform)
    if (threadIdx.x == 0) base_s = atomicAdd(A.cursor + k, total);
    __syncthreads();
    if (c == 0) return;
    const int d = 1 << (A.h - 1);
    int pos = A.off[k] + base_s + mine;
    for (int v = 0; v < 2; v++)
        for (int q = 0; q < 2; q++) {
            const int ca = a + q * d, cb = b + v * d;
            if (ca > 2 * A.S.nx || cb > 2 * A.S.ny) continue;              // the child's origin lies outside the lattice
            if (pos >= 0 && pos < A.next_cap) A.next[pos] = hs_bnb_pack(ca, cb);   // (the counts k24_filter gave size the block: always true)
            pos++;
        }
}

// ---- host side ---------------------------------------------------------------------------------------------------
// What the unit keeps, made by the first call: the pooled maps; a level's frontier, its U and its job table, each twice -- level h
// uses set h & 1, so that the set of level h - 1 can grow (which gives up what it held) while level h's is still read -- the job
// table's pinned staging; and the control block -- keys | counts | offsets | cursors -- with its pinned twin the results come back
// through.
struct hs_bnb {
    hs_block<uint32_t, HS_MEM_DEVICE> d_maps;
    hs_block<uint32_t, HS_MEM_DEVICE> d_front[2];
    hs_block<int32_t, HS_MEM_DEVICE> d_u[2];
    hs_block<unsigned char, HS_MEM_DEVICE> d_jobs[2];
    hs_block<unsigned char, HS_MEM_PINNED> h_jobs;
    hs_block<unsigned char, HS_MEM_DEVICE> d_ctl;
    hs_block<unsigned char, HS_MEM_PINNED> h_ctl;
};

// rule 1, what needs no hs: the fields of the bnb record and the top grid against max_blocks (the lattice's own fields have been checked)
static int32_t k24_check_fields(const char *who, const slamhip_bnb_spec *sp)
{
    if (sp->top < 0 || sp->top > HS_BNB_MAX_TOP) SH_FAIL(SLAMHIP_ERR_INVALID, "%s: top = %d must lie in [0, %d]", who, sp->top, HS_BNB_MAX_TOP);
    if (sp->world != 0 && sp->world != 1) SH_FAIL(SLAMHIP_ERR_INVALID, "%s: world = %d must be 0 (the window) or 1 (the world)", who, sp->world);
    if (sp->reserved != 0) SH_FAIL(SLAMHIP_ERR_INVALID, "%s: reserved = %d must be 0", who, sp->reserved);
    if (sp->max_blocks < 0) SH_FAIL(SLAMHIP_ERR_INVALID, "%s: max_blocks = %d must be >= 0 (0: 2^26)", who, sp->max_blocks);
    const slamhip_lattice_spec &S = sp->lattice;
    const int64_t blocks = (int64_t)hs_bnb_grid(S.nx, sp->top) * hs_bnb_grid(S.ny, sp->top) * S.n_theta;
    const int cap = sp->max_blocks ? sp->max_blocks : HS_BNB_DEFAULT_BLOCKS;
    if (blocks > (int64_t)cap)
        SH_FAIL(SLAMHIP_ERR_INVALID, "%s: %lld blocks at top = %d, more than max_blocks = %d: raise max_blocks or top", who, (long long)blocks, sp->top, cap);
    return SLAMHIP_OK;
}

// rule 5
static int32_t k24_overflow(const char *who, int h, long long count, int cap)
{
    SH_FAIL(SLAMHIP_ERR_INVALID, "%s: the frontier of height %d holds %lld blocks, more than max_blocks = %d: raise max_blocks or top", who, h, count, cap);
}

// From the per-heading {survivors, children} of one level: the survivors' total, the segments' offsets and the next level's job
// table.  -> the children's total
static long long k24_plan_level(const int32_t *counts, int n_theta, int32_t *off, std::vector<k24_job> *jobs, int *kept)
{
    long long total = 0;
    *kept = 0;
    for (int k = 0; k < n_theta; k++) { *kept += counts[2 * k]; total += counts[2 * k + 1]; }
    if (!off || total > (long long)INT32_MAX) return total;
    jobs->clear();
    int32_t at = 0;
    for (int k = 0; k < n_theta; k++) {
        off[k] = at;
        const int c = counts[2 * k + 1];
        for (int j = 0; j < c; j += K24_LANES) jobs->push_back(k24_job{ k, at + j, c - j < K24_LANES ? c - j : K24_LANES, 0 });
        at += c;
    }
    return total;
}

// The search into the unit's pinned block: *keys (n_theta of them) points into it and stays valid until the next search of this hs.
static int32_t k24_run(slamhip_hs *hs, const slamhip_bnb_spec *sp, const uint64_t **keys, slamhip_bnb_info *info)
{
    static const char *who = "slamhip_hs_lattice_search_bnb";
    SH_CHECK_ARG(hs && sp);
    const slamhip_lattice_spec *S = &sp->lattice;
    SH_TRY(hs_lat_check_spec(hs, S, false));
    SH_TRY(k24_check_fields(who, sp));
    if (hs->n_points <= 0) SH_FAIL(SLAMHIP_ERR_STATE, "%s: no scan (slamhip_hs_set_scan first)", who);
    slamhip_ctx *ctx = hs->ctx;
    hipStream_t st = ctx->stream;
    SH_TRY(hs_call_begin(hs));
    const bool world = sp->world != 0;
    const int top = sp->top, n_theta = S->n_theta, cap = sp->max_blocks ? sp->max_blocks : HS_BNB_DEFAULT_BLOCKS;
    hs_class_map M;
    SH_TRY(hs_lat_pack_prepare(hs, S->level, world, &M));                  // (the world's R of more than 2^28 cells is refused here, nothing launched)
    const hs_bnb_frame F = hs_bnb_frame_of(M.w, M.h, top);
    if (F.words * (size_t)(top + 1) > ((size_t)1 << 31))
        SH_FAIL(SLAMHIP_ERR_NOMEM, "%s: the %d pooled maps of %d x %d cells would take more than 8 GB", who, top + 1, M.w, M.h);
    SH_TRY(hs_unit<&slamhip_hs::bnb>(hs));
    hs_bnb *u = hs->bnb;
    // the control block: keys | counts | offsets | cursors
    const size_t key_bytes = sizeof(uint64_t) * (size_t)n_theta, cnt_bytes = sizeof(int32_t) * 2 * (size_t)n_theta, idx_bytes = sizeof(int32_t) * (size_t)n_theta;
    const size_t o_cnt = key_bytes, o_off = o_cnt + cnt_bytes, o_cur = o_off + idx_bytes;
    SH_TRY(u->d_maps.grow(sizeof(uint32_t) * F.words * (size_t)(top + 1), who));
    SH_TRY(u->d_ctl.grow(o_cur + idx_bytes, who));
    SH_TRY(u->h_ctl.grow(o_cur, who));
    k24_arg A;
    memset(&A, 0, sizeof(A));
    A.pts = hs->d_pts; A.n = hs->n_points;
    A.maps = u->d_maps; A.F = F;
    A.x0 = M.x0; A.y0 = M.y0;
    A.stm = hs->lv[S->level].stm;
    A.S = *S;
    A.gx = hs_bnb_grid(S->nx, top); A.gcount = A.gx * hs_bnb_grid(S->ny, top);
    A.keys = (unsigned long long *)u->d_ctl.p;
    A.counts = (int32_t *)(u->d_ctl + o_cnt); A.off = (const int32_t *)(u->d_ctl + o_off); A.cursor = (int32_t *)(u->d_ctl + o_cur);
    SH_TRY(hs_flush_scan(hs));
    SH_HIP(hipMemsetAsync(u->d_ctl, 0, key_bytes, st));
    SH_TRY(hs_lat_pack_enqueue(hs, S->level, world, &M));
    for (int h = 0; h <= top; h++) {
        hipLaunchKernelGGL(k24_pool, dim3((unsigned)((F.words + 255) / 256)), dim3(256), 0, st, M.cls, M.wpr, u->d_maps, F, h);
        SH_HIP(hipGetLastError());
    }
    slamhip_bnb_info I;
    memset(&I, 0, sizeof(I));
    I.top = top; I.n_levels = top + 1;
    int count = A.gcount * n_theta;                                        // |F_h| (rule 1: at most max_blocks <= 2^26 at the top)
    dim3 grid((unsigned)sh_div_up(A.gcount, K24_LANES), (unsigned)n_theta);
    std::vector<k24_job> jobs;
    if (top > 0) SH_TRY(u->d_u[top & 1].grow(sizeof(int32_t) * (size_t)count, who));
    for (int h = top; h >= 0; h--) {
        A.h = h;
        A.u = u->d_u[h & 1];
        hipLaunchKernelGGL(k24_score, grid, dim3(K24_LANES), 0, st, A);
        SH_HIP(hipGetLastError());
        I.blocks[h] = count; I.evaluated += count;
        if (h == 0) break;
        SH_HIP(hipMemsetAsync(A.counts, 0, cnt_bytes, st));
        hipLaunchKernelGGL(k24_filter, grid, dim3(K24_LANES), 0, st, A);
        SH_HIP(hipGetLastError());
        SH_HIP(hipMemcpyAsync(u->h_ctl + o_cnt, A.counts, cnt_bytes, hipMemcpyDeviceToHost, st));
        SH_TRY(hs_call_finish(hs));                                        // the level's wait
        int32_t *h_off = (int32_t *)(u->h_ctl + o_off);
        const long long total = k24_plan_level((const int32_t *)(u->h_ctl + o_cnt), n_theta, h_off, &jobs, &I.kept[h]);
        if (total > (long long)cap) return k24_overflow(who, h - 1, total, cap);
        if (total == 0) break;                                             // (cannot happen: the block that holds a heading's best origin survives)
        // the set of level h - 1: whatever read it last (level h + 1) ended before this level's wait
        const int dst = (h - 1) & 1;
        const size_t job_bytes = sizeof(k24_job) * jobs.size();
        SH_TRY(u->d_front[dst].grow(sizeof(uint32_t) * (size_t)total, who));
        if (h > 1) SH_TRY(u->d_u[dst].grow(sizeof(int32_t) * (size_t)total, who));
        SH_TRY(u->d_jobs[dst].grow(job_bytes, who));
        SH_TRY(u->h_jobs.grow(job_bytes, who));
        unsigned char *d_next_jobs = u->d_jobs[dst];
        memcpy(u->h_jobs, jobs.data(), job_bytes);
        SH_HIP(hipMemcpyAsync((void *)A.off, h_off, idx_bytes, hipMemcpyHostToDevice, st));
        SH_HIP(hipMemcpyAsync(d_next_jobs, u->h_jobs, job_bytes, hipMemcpyHostToDevice, st));
        SH_HIP(hipMemsetAsync(A.cursor, 0, idx_bytes, st));
        A.next = u->d_front[dst]; A.next_cap = (int)total;
        hipLaunchKernelGGL(k24_emit, grid, dim3(K24_LANES), 0, st, A);
        SH_HIP(hipGetLastError());
        A.front = u->d_front[dst]; A.jobs = (const k24_job *)d_next_jobs;
        count = (int)total;
        grid = dim3((unsigned)jobs.size());
    }
    SH_HIP(hipMemcpyAsync(u->h_ctl, u->d_ctl, key_bytes, hipMemcpyDeviceToHost, st));
    SH_TRY(hs_call_finish(hs));
    *keys = (const uint64_t *)u->h_ctl.p;
    *info = I;
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_lattice_search_bnb(slamhip_hs *hs, const slamhip_bnb_spec *spec, uint64_t *out_keys, slamhip_bnb_info *out_info)
{
    SH_CHECK_ARG(hs && spec && out_keys && out_info);
    const uint64_t *keys = nullptr;
    slamhip_bnb_info I;
    SH_TRY(k24_run(hs, spec, &keys, &I));
    memcpy(out_keys, keys, sizeof(uint64_t) * (size_t)spec->lattice.n_theta);
    *out_info = I;
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_relocalise_bnb(slamhip_hs *hs, const slamhip_bnb_spec *spec, int32_t B, float out_pose[3],
                                             slamhip_match_report *out_report, void *out_info, slamhip_bnb_info *out_bnb)
{
    SH_CHECK_ARG(hs && spec && out_pose && out_report && out_info && out_bnb && B >= 1 && B <= 64);
    if (spec->world == 1) SH_TRY(hs_lat_reloc_world_check(hs));            // (slamhip_hs_relocalise_world's pre-checks, ahead of the search's as there)
    const uint64_t *keys = nullptr;
    slamhip_bnb_info I;
    SH_TRY(k24_run(hs, spec, &keys, &I));
    *out_bnb = I;
    if (spec->world) return hs_lat_reloc_world_finish(hs, &spec->lattice, keys, B, out_pose, out_report, (slamhip_world_reloc_info *)out_info);
    return hs_lat_reloc_finish(hs, &spec->lattice, keys, B, out_pose, out_report, (slamhip_reloc_info *)out_info);
}

// CPU-side test hook: rules 1 - 6 in plain loops over hs_bnb.h, the text the kernels run
extern "C" int32_t slamhip_debug_lattice_bnb(const float *values, int32_t w, int32_t h, float cell_length, const slamhip_bnb_spec *spec,
                                             const float *xy, int32_t n, uint64_t *out_keys, slamhip_bnb_info *out_info)
{
    static const char *who = "lattice bnb";
    SH_CHECK_ARG(values && spec && out_keys && out_info && w >= 1 && h >= 1 && (int64_t)w * h <= ((int64_t)1 << 28) && cell_length > 0.0f && n >= 0 && (xy || n == 0));
    const slamhip_lattice_spec &S = spec->lattice;
    if (S.nx < 0 || S.nx > HS_LAT_MAX_HALF || S.ny < 0 || S.ny > HS_LAT_MAX_HALF)
        SH_FAIL(SLAMHIP_ERR_INVALID, "%s: nx = %d, ny = %d must lie in [0, %d]", who, S.nx, S.ny, HS_LAT_MAX_HALF);
    if (S.n_theta < 1 || S.n_theta > HS_LAT_MAX_THETA) SH_FAIL(SLAMHIP_ERR_INVALID, "%s: n_theta = %d must lie in [1, %d]", who, S.n_theta, HS_LAT_MAX_THETA);
    if (!(isfinite(S.centre[0]) && isfinite(S.centre[1]) && isfinite(S.centre[2]) && isfinite(S.dtheta)))
        SH_FAIL(SLAMHIP_ERR_INVALID, "%s: centre and dtheta must be finite", who);
    SH_TRY(k24_check_fields(who, spec));
    if (spec->world != 0) SH_FAIL(SLAMHIP_ERR_INVALID, "%s: the hook runs the window case, world = %d", who, spec->world);
    const int top = spec->top, n_theta = S.n_theta, cap = spec->max_blocks ? spec->max_blocks : HS_BNB_DEFAULT_BLOCKS;
    const int NX = 2 * S.nx + 1;
    const float stm = 1.0f / cell_length;
    // rule 2: the class map in its frame, then the doublings
    const hs_bnb_frame F = hs_bnb_frame_of(w, h, top);
    std::vector<uint32_t> maps(F.words * (size_t)(top + 1), 0u);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++)
            maps[(size_t)(y + F.my) * F.wpr + (size_t)((x + F.mx) >> 4)] |= hs_lat_class_bits(values[(size_t)y * w + x]) << (((x + F.mx) & 15) * 2);
    for (int l = 1; l <= top; l++)
        for (int y = 0; y < F.rows; y++)
            for (int wx = 0; wx < F.wpr; wx++)
                maps[(size_t)l * F.words + (size_t)y * F.wpr + wx] = hs_bnb_pool_word(maps.data() + (size_t)(l - 1) * F.words, F.wpr, F.rows, y, wx, 1 << (l - 1));
    // the point cells of every heading, the ignored ones left out
    std::vector<std::vector<int>> cells((size_t)n_theta);
    for (int k = 0; k < n_theta; k++) {
        const hs_lat_heading H = hs_lat_heading_of(stm, S.centre[0], S.centre[1], hs_lat_theta(S, k));
        for (int i = 0; i < n; i++) {
            int gx, gy;
            if (hs_lat_point_cell(H, xy[2 * i], xy[2 * i + 1], &gx, &gy)) { cells[(size_t)k].push_back(gx); cells[(size_t)k].push_back(gy); }
        }
    }
    // rules 3, 4: the frontier as (k, packed block) pairs, heading-major
    std::vector<uint64_t> keys((size_t)n_theta, 0ull);
    std::vector<uint32_t> fk, fb, nk, nb;
    std::vector<int32_t> U;
    const int gx_n = hs_bnb_grid(S.nx, top), gy_n = hs_bnb_grid(S.ny, top);
    for (int k = 0; k < n_theta; k++)
        for (int j = 0; j < gy_n; j++)
            for (int i = 0; i < gx_n; i++) { fk.push_back((uint32_t)k); fb.push_back(hs_bnb_pack(i << top, j << top)); }
    slamhip_bnb_info I;
    memset(&I, 0, sizeof(I));
    I.top = top; I.n_levels = top + 1;
    for (int l = top; l >= 0 && !fk.empty(); l--) {
        const uint32_t *p0 = maps.data(), *pl = maps.data() + (size_t)l * F.words;
        U.resize(fk.size());
        for (size_t f = 0; f < fk.size(); f++) {
            const int k = (int)fk[f], a = hs_bnb_a(fb[f]), b = hs_bnb_b(fb[f]);
            const std::vector<int> &c = cells[(size_t)k];
            const int ox = a - S.nx + F.mx, oy = b - S.ny + F.my;
            int E = 0, Ul = 0;
            for (size_t j = 0; j < c.size(); j += 2) {
                E += hs_bnb_cell(p0, F.wpr, F.rows, c[j] + ox, c[j + 1] + oy);
                if (l > 0) Ul += hs_bnb_cell(pl, F.wpr, F.rows, c[j] + ox, c[j + 1] + oy);
            }
            U[f] = l > 0 ? Ul : E;
            const uint64_t key = hs_lat_key(E, (uint32_t)(b * NX + a));
            keys[(size_t)k] = key > keys[(size_t)k] ? key : keys[(size_t)k];
        }
        I.blocks[l] = (int32_t)fk.size(); I.evaluated += (int64_t)fk.size();
        if (l == 0) break;
        nk.clear(); nb.clear();
        long long total = 0;
        const int d = 1 << (l - 1);
        for (size_t f = 0; f < fk.size(); f++) {
            const int k = (int)fk[f], a = hs_bnb_a(fb[f]), b = hs_bnb_b(fb[f]);
            if (!hs_bnb_survives(l, U[f], hs_bnb_key_score(keys[(size_t)k]))) continue;
            I.kept[l]++;
            total += hs_bnb_children(a, b, l, S.nx, S.ny);
            if (total > (long long)cap) continue;                          // (rule 5: counted on, not stored)
            for (int v = 0; v < 2; v++)
                for (int q = 0; q < 2; q++)
                    if (a + q * d <= 2 * S.nx && b + v * d <= 2 * S.ny) { nk.push_back((uint32_t)k); nb.push_back(hs_bnb_pack(a + q * d, b + v * d)); }
        }
        if (total > (long long)cap) return k24_overflow(who, l - 1, total, cap);
        fk.swap(nk); fb.swap(nb);
    }
    memcpy(out_keys, keys.data(), sizeof(uint64_t) * (size_t)n_theta);
    *out_info = I;
    return SLAMHIP_OK;
}
