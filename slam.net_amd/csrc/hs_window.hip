// hs_window.hip -- K6, the scrolling map window of HectorSLAM (slamhip_hs_shift) and its backing store (slamhip_hs_set_backing):
// the enqueue-only path.  The blocking calls on the world behind both (download, upload, extents): hs_world.hip.
#include "hs_tiles.h"

// ---- K6: the scrolling window (slamhip_hs_shift) -------------------------------------------------------------------------------
// Something the reference lacks (its `offset`, GridMap.cs:45, is ignored by UpdateByScan and by the matcher): the CONTENTS of every
// level move by a whole number of cells, so that K4 and K5 go on working in the window's frame with the transforms they have.  On
// level l new cell (x, y) holds what old cell (x + sx, y + sy) held, sx = dx >> l; a cell whose source lies outside the level
// becomes LogOddsCell.Reset() (LogOddsCell.cs:38-42) with probability 0.5f -- exp(0) / (exp(0) + 1), what k5_fill_cells and
// k5_refresh_prob give for Value 0.  Not in place (a workgroup would read what another has overwritten): the launch reads one set
// of arrays and writes the other, and the host swaps the pointers behind it -- every launch takes its pointers from hs->lv when it
// is enqueued (levels_arg, hs_update_enqueue's k5_arg, the downloads and reports), none is kept past a call, and the stream orders
// the launches.  ONE launch for all levels, cells and probabilities, exposed bands included.
// Lane mapping: a workgroup owns K6_BLOCK consecutive cells of a level's flat array; a lane moves 16-byte units of the DESTINATION,
// which are always aligned (two cells, four probabilities): one store each, consecutive lanes consecutive units.  A unit that lies
// in one row with all its sources inside the map is one load as wide as the source's alignment allows -- the source index differs
// from the destination's by sy * w + sx, a multiple of 4 on level 0 of a pyramid of three levels or more, of 2 on level 1, of
// anything on the coarsest (which is small); every other unit (a row's end where w is no multiple of the unit, the exposed band,
// the array's tail) goes element by element with the bounds test per element.
#define K6_BLOCK 1024
struct k6_level { int w, h, sx, sy, blk0; const slamhip_cell *src_c; slamhip_cell *dst_c; const float *src_p; float *dst_p; };
struct k6_arg { k6_level lv[HS_MAX_LEVELS]; int n; };

template <typename T, int N>                   // N elements of T are 16 bytes; i: the unit's first element, a multiple of N
__device__ static __forceinline__ void k6_unit(const T *__restrict__ src, T *__restrict__ dst, int w, int h, int sx, int sy, int i, int n, const T fill)
{
    static_assert(sizeof(T) * N == 16, "a unit is 16 bytes");
    if (i >= n) return;
    struct alignas(16) unit { T e[N]; };
    struct alignas(8) half { T e[N / 2]; };
    const int y = i / w, x = i - y * w;
    const int ys = y + sy, xs = x + sx;
    if (i + N <= n && x + N <= w && ys >= 0 && ys < h && xs >= 0 && xs + N <= w) {
        const T *s = src + ((size_t)ys * w + xs);                         // (inside the array: 0 <= ys < h, 0 <= xs, xs + N <= w)
        const unsigned mis = (unsigned)(xs + ys * w) & (N - 1);
        unit v;
        if (mis == 0) v = *(const unit *)s;
        else if (N == 4 && mis == 2) {
            const half a = *(const half *)s, b = *(const half *)(s + N / 2);
#pragma unroll
            for (int k = 0; k < N / 2; k++) { v.e[k] = a.e[k]; v.e[N / 2 + k] = b.e[k]; }
        } else {
#pragma unroll
            for (int k = 0; k < N; k++) v.e[k] = s[k];
        }
        *(unit *)(dst + i) = v;
        return;
    }
#pragma unroll
    for (int k = 0; k < N; k++) {
        const int ik = i + k;
        if (ik >= n) break;
        const int yk = ik / w, xk = ik - yk * w;
        const int yy = yk + sy, xx = xk + sx;
        const bool in = yy >= 0 && yy < h && xx >= 0 && xx < w;
        dst[ik] = in ? src[(size_t)yy * w + xx] : fill;
    }
}

__global__ void __launch_bounds__(256) k6_shift(const k6_arg A)
{
    int lvl = 0;
    for (int l = 1; l < A.n; l++) if ((int)blockIdx.x >= A.lv[l].blk0) lvl = l;
    const k6_level &L = A.lv[lvl];
    const int n = L.w * L.h;                                               // (<= 2^30: slamhip_hs_create bounds w and h by 32768)
    const int base = ((int)blockIdx.x - L.blk0) * K6_BLOCK, t = threadIdx.x;
    const slamhip_cell reset = hs_reset_cell();
    k6_unit<slamhip_cell, 2>(L.src_c, L.dst_c, L.w, L.h, L.sx, L.sy, base + 2 * t, n, reset);
    k6_unit<slamhip_cell, 2>(L.src_c, L.dst_c, L.w, L.h, L.sx, L.sy, base + K6_BLOCK / 2 + 2 * t, n, reset);
    k6_unit<float, 4>(L.src_p, L.dst_p, L.w, L.h, L.sx, L.sy, base + 4 * t, n, HS_RESET_PROB);
}

// ---- K6 page: the backing store of the scrolling window (slamhip_hs_set_backing) -------------------------------------------------
// ONE launch behind k6_shift.  Evict jobs copy pieces of the OLD set of arrays (the `_alt` names after the swap: K6 is not in
// place, so they are intact until the next shift, and the stream orders that) into tile slots; restore jobs copy pieces of tile
// slots into the exposed bands of the NEW set, over the Reset that k6_shift wrote.  The departing and the arriving cells are
// disjoint in world cells but may share a tile, and on the coarse levels dx >> l may be odd: a 16-byte unit (two cells, four
// probabilities) is used only where it lies wholly inside one job's row and is aligned on both sides; everything else goes element
// by element (probabilities also in 8-byte halves where the tile's side is aligned to 8 only) -- no lane touches an element of
// another job, so evict and restore jobs of one tile may run side by side.
// Lane mapping: jobs are thin (g cells by T for the common small shift), so a WORKGROUP owns a job piece -- at most K6P_CELLS cells
// in whole rows of one job, cut on the host -- and its lanes take the piece's 16-byte groups, laid out by the WINDOW side's
// alignment (the wide side: rows of w cells), consecutive lanes consecutive groups of a row, the next row behind the last group.
// The job table is read from a pinned host block (32 bytes per workgroup, the same for all lanes).  A slot: T * T cells, then
// T * T probabilities.
struct k6p_job { unsigned char *slot; int32_t wx, wy; uint16_t nx, ny, lx, ly; uint32_t level_kind, pad; };   // level_kind: level * 2 + kind
static_assert(sizeof(k6p_job) == 32, "a job piece is two 16-byte words");
struct k6p_level { int w; const slamhip_cell *old_c; const float *old_p; slamhip_cell *new_c; float *new_p; };
struct k6p_arg { k6p_level lv[HS_MAX_LEVELS]; const k6p_job *jobs; int T; };

template <typename E, int N>                   // N elements of E are 16 bytes
__device__ static __forceinline__ void k6p_rows(E *__restrict__ win, E *__restrict__ tile, const bool evict, const int w, const int T,
                                                const int wx, const int wy, const int nx, const int ny, const int lx, const int ly)
{
    static_assert(sizeof(E) * N == 16, "a unit is 16 bytes");
    struct alignas(16) unit { E e[N]; };
    struct alignas(8) half { E e[N / 2]; };
    const int gpr = (nx + N - 1) / N + 1;                                  // groups per row, a row's misaligned head included
    const int items = gpr * ny;
    for (int i = threadIdx.x; i < items; i += 256) {
        const int r = i / gpr, g = i - r * gpr;
        const size_t a = (size_t)(wy + r) * w + wx;                        // the row's first element in the window's array
        const int b = (ly + r) * T + lx;                                   // ... and in the tile's
        const int e0 = g * N - (int)(a & (N - 1));                        // the group's first element in the row: a + e0 is a multiple of N
        if (e0 >= nx) continue;
        if (e0 >= 0 && e0 + N <= nx && ((b + e0) & (N / 2 - 1 + (N == 2))) == 0) {   // whole, and the tile's side aligned to 8 at least
            E *pw = win + (a + e0), *pt = tile + (b + e0);
            if (((b + e0) & (N - 1)) == 0) {
                if (evict) *(unit *)pt = *(const unit *)pw; else *(unit *)pw = *(const unit *)pt;
            } else {                                                       // (N == 4 only: the tile's side in two halves)
                if (evict) {
                    const unit v = *(const unit *)pw;
                    half lo, hi;
#pragma unroll
                    for (int k = 0; k < N / 2; k++) { lo.e[k] = v.e[k]; hi.e[k] = v.e[N / 2 + k]; }
                    *(half *)pt = lo; *(half *)(pt + N / 2) = hi;
                } else {
                    const half lo = *(const half *)pt, hi = *(const half *)(pt + N / 2);
                    unit v;
#pragma unroll
                    for (int k = 0; k < N / 2; k++) { v.e[k] = lo.e[k]; v.e[N / 2 + k] = hi.e[k]; }
                    *(unit *)pw = v;
                }
            }
            continue;
        }
#pragma unroll
        for (int k = 0; k < N; k++) {
            const int e = e0 + k;
            if (e < 0 || e >= nx) continue;
            if (evict) tile[b + e] = win[a + e]; else win[a + e] = tile[b + e];
        }
    }
}

__global__ void __launch_bounds__(256) k6_page(const k6p_arg A)
{
    const k6p_job J = A.jobs[blockIdx.x];
    const int lvl = (int)(J.level_kind >> 1);
    const bool evict = (J.level_kind & 1u) == SLAMHIP_BACKING_EVICT;
    const k6p_level &L = A.lv[lvl];
    const int T = A.T;
    slamhip_cell *tc = (slamhip_cell *)J.slot;
    float *tp = (float *)(J.slot + k6p_slot_prob_offset((size_t)T * T));
    slamhip_cell *wc = evict ? const_cast<slamhip_cell *>(L.old_c) : L.new_c;
    float *wp = evict ? const_cast<float *>(L.old_p) : L.new_p;
    k6p_rows<slamhip_cell, 2>(wc, tc, evict, L.w, T, J.wx, J.wy, J.nx, J.ny, J.lx, J.ly);
    k6p_rows<float, 4>(wp, tp, evict, L.w, T, J.wx, J.wy, J.nx, J.ny, J.lx, J.ly);
}

// a chunk of new slots: Reset cells and 0.5f (what k5_fill_cells writes), slot by slot in the slot layout
__global__ void __launch_bounds__(256) k6_fill_slots(unsigned char *base, int t2, size_t n)    // n = slots * t2
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const size_t s = i / t2, e = i - s * t2;
        unsigned char *slot = base + s * k6p_slot_bytes(t2);
        ((slamhip_cell *)slot)[e] = hs_reset_cell();
        ((float *)(slot + k6p_slot_prob_offset(t2)))[e] = HS_RESET_PROB;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------
// (the books -- pool, directory, ring: hs_tiles.h)
#define HS_BK_CHUNK_BYTES ((size_t)4 << 20)

static void hs_bk_fill_chunk(slamhip_hs *hs, const hs_bk_chunk &c)
{
    const int t2 = hs->bk->T * hs->bk->T;
    const size_t n = c.slots * (size_t)t2, want = (n + 2047) / 2048;
    hipLaunchKernelGGL(k6_fill_slots, dim3((unsigned)(want < 1 ? 1 : want > 2048 ? 2048 : want)), dim3(256), 0, hs->ctx->stream, c.base, t2, n);
}
static void hs_bk_push_free(hs_backing *bk, const hs_bk_chunk &c)
{
    for (size_t k = c.slots; k-- > 0;) bk->free_slots.push_back(c.base + k * bk->slot_bytes);
}

unsigned char *hs_bk_slot(slamhip_hs *hs)
{
    hs_backing *bk = hs->bk;
    if (bk->free_slots.empty()) {
        const uint64_t room = bk->max_bytes > (uint64_t)bk->bytes ? bk->max_bytes - (uint64_t)bk->bytes : 0;
        size_t n = HS_BK_CHUNK_BYTES / bk->slot_bytes;
        if (n < 1) n = 1;
        if ((uint64_t)n > room / bk->slot_bytes) n = (size_t)(room / bk->slot_bytes);
        if (n == 0) return nullptr;
        hs_bk_chunk c = { nullptr, n };
        if (hipMalloc(&c.base, n * bk->slot_bytes) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        bk->chunks.push_back(c);
        bk->bytes += (int64_t)(n * bk->slot_bytes);
        hs_bk_fill_chunk(hs, c);
        hs_bk_push_free(bk, c);
    }
    unsigned char *s = bk->free_slots.back();
    bk->free_slots.pop_back();
    return s;
}

// n more slots in the pool, ALL of them or none (slamhip_hs_render_world plans before it changes anything): chunks sized as
// hs_bk_slot sizes them, allocated first and entered into the books only when the last one is there
int32_t hs_bk_reserve(slamhip_hs *hs, size_t n)
{
    hs_backing *bk = hs->bk;
    std::vector<hs_bk_chunk> got;
    uint64_t bytes = (uint64_t)bk->bytes;
    bool ok = true;
    while (ok && n > 0) {
        const uint64_t room = bk->max_bytes > bytes ? bk->max_bytes - bytes : 0;
        size_t k = HS_BK_CHUNK_BYTES / bk->slot_bytes;
        if (k < 1) k = 1;
        if ((uint64_t)k > room / bk->slot_bytes) k = (size_t)(room / bk->slot_bytes);
        hs_bk_chunk c = { nullptr, k };
        if (k == 0 || hipMalloc(&c.base, k * bk->slot_bytes) != hipSuccess) { (void)hipGetLastError(); ok = false; break; }
        got.push_back(c);
        bytes += (uint64_t)(k * bk->slot_bytes);
        n -= std::min(n, k);
    }
    if (!ok) {
        for (const hs_bk_chunk &c : got) (void)hipFree(c.base);
        SH_FAIL(SLAMHIP_ERR_NOMEM, "the backing store cannot take %zu more tiles of %zu bytes: max_bytes = %llu with %lld in use, or a chunk's allocation failed",
                n, bk->slot_bytes, (unsigned long long)bk->max_bytes, (long long)bk->bytes);
    }
    for (const hs_bk_chunk &c : got) {
        bk->chunks.push_back(c);
        bk->bytes += (int64_t)(c.slots * bk->slot_bytes);
        hs_bk_fill_chunk(hs, c);
        hs_bk_push_free(bk, c);
    }
    return SLAMHIP_OK;
}

// (the caller has drained the stream)
void hs_bk_free(slamhip_hs *hs)
{
    hs_backing *bk = hs->bk;
    if (!bk) return;
    for (const hs_bk_chunk &c : bk->chunks) (void)hipFree(c.base);
    for (int i = 0; i < HS_BK_RING; i++) {
        if (bk->ring[i].h) (void)hipHostFree(bk->ring[i].h);
        if (bk->ring[i].ev) (void)hipEventDestroy(bk->ring[i].ev);
    }
    delete bk;
    hs->bk = nullptr;
}

// The second launch of a shift with backing on: plan (backing_plan.h), deal slots in job order, cut the jobs into pieces of whole
// rows, put the table into the next block of the pinned ring and enqueue k6_page behind k6_shift.  (ox, oy): the origin BEFORE
// the shift; hs->lv already carries the swapped names.
static int32_t hs_bk_page(slamhip_hs *hs, int64_t ox, int64_t oy, int32_t dx, int32_t dy)
{
    hs_backing *bk = hs->bk;
    const int T = bk->T;
    bp_plan(hs->n_levels, hs->lv[0].w, hs->lv[0].h, ox, oy, dx, dy, T, bk->plan);
    bk->pieces.clear();
    for (const slamhip_backing_job &j : bk->plan) {
        const hs_level &L = hs->lv[j.level];
        // (what keeps the launch inside its arrays: a piece of the window, a piece of one tile)
        if (j.level < 0 || j.level >= hs->n_levels || j.nx < 1 || j.ny < 1 || j.wx < 0 || j.wy < 0 || j.wx + j.nx > L.w || j.wy + j.ny > L.h ||
            j.lx < 0 || j.ly < 0 || j.lx + j.nx > T || j.ly + j.ny > T)
            SH_FAIL(SLAMHIP_ERR_STATE, "slamhip_hs_shift: the backing store's planner produced a job outside its window or tile (level %d)", j.level);
        const int64_t area = (int64_t)j.nx * j.ny;
        const bool evict = j.kind == SLAMHIP_BACKING_EVICT;
        unsigned char *slot = evict ? bk->find_or_take(hs, j.level, j.ty, j.tx) : bk->find(j.level, j.ty, j.tx);
        // no slot: an evict job's cells are dropped; a restore job has nothing to bring -- nothing was ever evicted there, k6_shift's Reset stands
        if (!slot) { if (evict) bk->dropped += area; continue; }
        (evict ? bk->evicted : bk->restored) += area;
        hs_cut_rows(j.nx, j.ny, [&](int r0, int rows) {
            k6p_job p;
            p.slot = slot; p.wx = j.wx; p.wy = j.wy + r0;
            p.nx = (uint16_t)j.nx; p.ny = (uint16_t)rows; p.lx = (uint16_t)j.lx; p.ly = (uint16_t)(j.ly + r0);
            p.level_kind = (uint32_t)(j.level * 2 + j.kind); p.pad = 0;
            bk->pieces.push_back(p);
        });
    }
    if (bk->pieces.empty()) return SLAMHIP_OK;
    if (bk->pieces.size() > (size_t)INT32_MAX) SH_FAIL(SLAMHIP_ERR_INVALID, "slamhip_hs_shift: %zu job pieces in one shift", bk->pieces.size());
    hs_bk_block &B = bk->ring[bk->ring_next++ % HS_BK_RING];
    if (!B.ev) SH_HIP(hipEventCreateWithFlags(&B.ev, hipEventDisableTiming));
    if (B.in_flight) { SH_TRY(sh_event_wait(hs->ctx, B.ev)); B.in_flight = false; }
    if (B.cap < bk->pieces.size()) {
        if (B.h) { (void)hipHostFree(B.h); B.h = nullptr; B.cap = 0; }
        const size_t cap = bk->pieces.size() + bk->pieces.size() / 2 + 256;
        SH_HIP(hipHostMalloc((void **)&B.h, sizeof(k6p_job) * cap, hipHostMallocMapped | hipHostMallocCoherent));
        B.cap = cap;
    }
    memcpy(B.h, bk->pieces.data(), sizeof(k6p_job) * bk->pieces.size());
    k6p_arg A;
    memset(&A, 0, sizeof(A));
    for (int l = 0; l < hs->n_levels; l++) {
        const hs_level &L = hs->lv[l];
        A.lv[l].w = L.w;
        A.lv[l].old_c = L.d_cells_alt; A.lv[l].old_p = L.d_prob_alt;       // (after the swap: what the window was)
        A.lv[l].new_c = L.d_cells; A.lv[l].new_p = L.d_prob;
    }
    A.jobs = B.h; A.T = T;
    hipLaunchKernelGGL(k6_page, dim3((unsigned)bk->pieces.size()), dim3(256), 0, hs->ctx->stream, A);
    SH_HIP(hipGetLastError());
    SH_HIP(hipEventRecord(B.ev, hs->ctx->stream));
    B.in_flight = true;
    return SLAMHIP_OK;
}

// slamhip_hs_reset: the directory goes, the pool stays -- every slot Reset again
void hs_bk_reset(slamhip_hs *hs)
{
    hs->bk->dir.clear();
    hs->bk->free_slots.clear();
    for (const hs_bk_chunk &c : hs->bk->chunks) { hs_bk_fill_chunk(hs, c); hs_bk_push_free(hs->bk, c); }
}

// The window moves by (+dx, +dy) level-0 cells (K6 above).  Enqueue-only: behind every update and match already on the operator's
// stream, ahead of whatever is enqueued later; no host wait.
extern "C" int32_t slamhip_hs_shift(slamhip_hs *hs, int32_t dx, int32_t dy)
{
    SH_CHECK_ARG(hs);
    if (hs->ctx->poisoned) SH_FAIL(SLAMHIP_ERR_TIMEOUT, "the context was poisoned by a blocking wait that timed out; destroy it");
    const int32_t g = 1 << (hs->n_levels - 1);
    if ((dx & (g - 1)) != 0 || (dy & (g - 1)) != 0)
        SH_FAIL(SLAMHIP_ERR_INVALID, "slamhip_hs_shift: dx = %d and dy = %d must be multiples of %d = 1 << (levels - 1), so that every level moves by whole cells",
                dx, dy, g);
    if (hs->ref_cache)
        SH_FAIL(SLAMHIP_ERR_INVALID, "slamhip_hs_shift: the reference's cache is on (slamhip_hs_set_reference_cache) -- its literal stale entries have "
                "no meaning under an operation the reference lacks; turn it off first");
    if (dx == 0 && dy == 0) return SLAMHIP_OK;
    SH_HIP(hipSetDevice(hs->ctx->device));
    if (!hs->lv[0].d_cells_alt) {                                          // the first shift: the second set, all levels or none
        for (int l = 0; l < hs->n_levels; l++) {
            hs_level &L = hs->lv[l];
            const size_t n = (size_t)L.w * L.h;
            if (hipMalloc(&L.d_cells_alt, sizeof(slamhip_cell) * n) != hipSuccess || hipMalloc(&L.d_prob_alt, sizeof(float) * n) != hipSuccess) {
                (void)hipGetLastError();
                for (int k = 0; k < hs->n_levels; k++) {
                    (void)hipFree(hs->lv[k].d_cells_alt); (void)hipFree(hs->lv[k].d_prob_alt);
                    hs->lv[k].d_cells_alt = nullptr; hs->lv[k].d_prob_alt = nullptr;
                }
                SH_FAIL(SLAMHIP_ERR_NOMEM, "device allocation of the window's second set of arrays failed (level %d)", l);
            }
        }
    }
    k6_arg A;
    memset(&A, 0, sizeof(A));
    A.n = hs->n_levels;
    int blocks = 0;
    for (int l = 0; l < hs->n_levels; l++) {
        const hs_level &L = hs->lv[l];
        k6_level &K = A.lv[l];
        K.w = L.w; K.h = L.h;
        const int sx = dx >> l, sy = dy >> l;                              // (exact: dx and dy are multiples of 1 << (levels - 1); arithmetic shift)
        // a move by the level's size or more clears the level: every source is then outside it whatever the other axis says, and
        // the clamp keeps sy * w + sx inside 32 bits
        K.sx = sx >= L.w ? L.w : sx <= -L.w ? -L.w : sx;
        K.sy = sy >= L.h ? L.h : sy <= -L.h ? -L.h : sy;
        K.blk0 = blocks;
        K.src_c = L.d_cells; K.dst_c = L.d_cells_alt; K.src_p = L.d_prob; K.dst_p = L.d_prob_alt;
        blocks += (int)(((size_t)L.w * L.h + K6_BLOCK - 1) / K6_BLOCK);
    }
    hipLaunchKernelGGL(k6_shift, dim3(blocks), dim3(256), 0, hs->ctx->stream, A);
    SH_HIP(hipGetLastError());
    for (int l = 0; l < hs->n_levels; l++) {
        hs_level &L = hs->lv[l];
        slamhip_cell *c = L.d_cells; L.d_cells = L.d_cells_alt; L.d_cells_alt = c;
        float *p = L.d_prob; L.d_prob = L.d_prob_alt; L.d_prob_alt = p;
    }
    // K5's sector records (d_k5_sec) stay: they split the NEXT scan's lines, by line index, into eight ranges of equal expected
    // work -- a balance hint only ("any partition is correct", k5_cells) that says nothing about where cells lie in memory.
    hs->win_ox += dx; hs->win_oy += dy;
    if (hs->bk) return hs_bk_page(hs, hs->win_ox - dx, hs->win_oy - dy, dx, dy);   // slamhip_hs_set_backing: ONE more launch
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_set_backing(slamhip_hs *hs, int32_t tile_cells, uint64_t max_bytes)
{
    SH_CHECK_ARG(hs);
    if (max_bytes == 0) {                                                  // off: every tile dropped, the pool freed
        if (!hs->bk) return SLAMHIP_OK;
        SH_HIP(hipSetDevice(hs->ctx->device));
        if (!hs->ctx->poisoned) SH_HIP(hipStreamSynchronize(hs->ctx->stream));   // (launches that read the pool or the ring may be in flight)
        hs_bk_free(hs);
        return SLAMHIP_OK;
    }
    if (tile_cells < 8 || tile_cells > 256 || (tile_cells & (tile_cells - 1)) != 0)
        SH_FAIL(SLAMHIP_ERR_INVALID, "slamhip_hs_set_backing: tile_cells = %d must be a power of two in [8, 256]", tile_cells);
    const size_t slot_bytes = k6p_slot_bytes((size_t)tile_cells * tile_cells);
    if (max_bytes < slot_bytes)
        SH_FAIL(SLAMHIP_ERR_INVALID, "slamhip_hs_set_backing: max_bytes = %llu is less than one slot of %zu bytes", (unsigned long long)max_bytes, slot_bytes);
    if (hs->bk) {
        hs_backing *bk = hs->bk;
        if (bk->T == tile_cells && max_bytes >= (uint64_t)bk->bytes) { bk->max_bytes = max_bytes; return SLAMHIP_OK; }
        if (!bk->dir.empty())
            SH_FAIL(SLAMHIP_ERR_INVALID, "slamhip_hs_set_backing: tiles exist -- tile_cells (%d -> %d) cannot change and max_bytes cannot fall below the pool's "
                    "%lld bytes; switch backing off first", bk->T, tile_cells, (long long)bk->bytes);
        SH_TRY(slamhip_hs_set_backing(hs, 0, 0));                          // (no tiles: a new pool under the new setting)
    }
    hs_backing *bk = new (std::nothrow) hs_backing();
    if (!bk) SH_FAIL(SLAMHIP_ERR_NOMEM, "out of host memory");
    bk->T = tile_cells; bk->max_bytes = max_bytes; bk->slot_bytes = slot_bytes;
    bk->bytes = bk->evicted = bk->restored = bk->dropped = 0;
    memset(bk->ring, 0, sizeof(bk->ring)); bk->ring_next = 0;
    hs->bk = bk;
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_backing_stats(slamhip_hs *hs, slamhip_backing_stats *out)
{
    SH_CHECK_ARG(hs && out);
    memset(out, 0, sizeof(*out));
    if (!hs->bk) return SLAMHIP_OK;
    const hs_backing *bk = hs->bk;
    out->tiles = (int64_t)bk->dir.size(); out->bytes = bk->bytes; out->capacity_bytes = (int64_t)bk->max_bytes;
    out->evicted_cells = bk->evicted; out->restored_cells = bk->restored; out->dropped_cells = bk->dropped;
    out->tile = bk->T; out->on = 1;
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_origin(slamhip_hs *hs, int64_t *ox, int64_t *oy)
{
    SH_CHECK_ARG(hs && ox && oy);
    *ox = hs->win_ox; *oy = hs->win_oy;
    return SLAMHIP_OK;
}
