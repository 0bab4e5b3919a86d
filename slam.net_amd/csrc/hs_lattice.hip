// hs_lattice.hip -- K7, the pose-lattice (correlative) search of HectorSLAM: relocalisation in a loaded map (slamhip_hs_lattice_search,
// slamhip_hs_lattice_node_pose, slamhip_hs_relocalise, slamhip_debug_lattice_cells).  No reference counterpart: the reference's
// HectorSLAMProcessor can only Reset.  Definition of the score: include/slamhip.h (slamhip_lattice_spec); the arithmetic host and
// device share: hs_lattice.h.
//
// Two launches per search on the operator's stream.
//  * k7_pack turns the level's cell values into a CLASS MAP of 2 bits per cell (hs_lat_class_bits: 1 occupied, 2 free, 0 neither),
//    16 cells per 32-bit word, rows padded to whole words, the padding zero.  A 512^2 level is 64 KB instead of 2 MB of cells, and the
//    score needs nothing else of a cell.  Re-packed on every search: one pass over one level, cheaper than tracking every writer.
//  * k7_search: the grid is (translation tiles, headings).  A workgroup of 256 lanes owns a tile of 64 x 4 (or 16 x 16, for a
//    narrow lattice) translations of one heading, one translation per lane, consecutive lanes consecutive ix.  It forms the
//    heading's (gx, gy) of every point once, cooperatively -- first for their bounding box, then chunk by chunk (K7_CHUNK points)
//    into LDS -- and stages the sub-rectangle of the class map its tile can touch: the bounding box grown by the tile's ix / iy
//    range, clipped to the map, in whole words.  Each lane then walks the points: one broadcast read of the point, one read of the
//    word its cell lies in (a wavefront reads the same or neighbouring words).  A cell outside the staged rectangle lies outside
//    the map by construction (and the padding bits are zero), so the out-of-map test is the rectangle test and is exact.
//    When the rectangle does not fit K7_RECT_WORDS the SAME loop (k7_walk<false>) reads the packed map from global memory, where a
//    coarse level stays in the L2, with the map's own extent as its rectangle: decided per workgroup from the rectangle it found,
//    a template argument of the loop and no option of the library.
//    LDS: 48 KB rectangle + 8 KB points + 64 B = 56 KB per workgroup: two workgroups per compute unit (160 KB), under the 64 KB a
//    static allocation may have.  48 KB of class map is 196608 cells: the whole of a 384 x 512 level, so a coarse level's room fits.
//    The workgroup's best key: a wave maximum, the wavefronts' maxima through LDS, then ONE 64-bit maximum at agent scope on key[k]
//    (K1's packed-key idiom, mirrored: highest score, ties to the lowest flat index); the keys are zeroed in-stream ahead of it.
#include "hs_internal.h"
#include "hs_lattice.h"
#include <algorithm>
#include <math.h>
#include <new>

#define K7_LANES 256
#define K7_RECT_WORDS 12288                // 48 KB of class map
#define K7_CHUNK 1024                      // points per LDS chunk (8 KB)
#define K7_IGNORED (-(1 << 30))            // (gx, gy) of an ignored point in LDS: outside every rectangle, and far from overflow under +-4096

__global__ void __launch_bounds__(256) k7_pack(const slamhip_cell *__restrict__ cells, int w, int h, int wpr, uint32_t *__restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= wpr * h) return;
    const int y = i / wpr, x0 = (i - y * wpr) * 16;
    const slamhip_cell *row = cells + (size_t)y * w;
    uint32_t word = 0;
#pragma unroll
    for (int b = 0; b < 16; b++)
        if (x0 + b < w) word |= hs_lat_class_bits(row[x0 + b].value) << (2 * b);
    out[i] = word;
}

struct k7_arg {
    const float2 *pts; int n;
    const uint32_t *cls; int w, h, wpr;    // the packed class map of the level
    float stm;
    slamhip_lattice_spec S;
    int txl, tiles_x;                      // a tile is (1 << txl) x (K7_LANES >> txl) translations; tiles per lattice row
    unsigned long long *keys; int32_t *scores;
};

// The walk of one lane over m points: the sum of the classes of the cells (g.x + dx, g.y + dy), coordinates relative to the
// rectangle's first cell, which is rwc x rh cells in rows of rwpr words.  LDSR: the rectangle is `rect` in LDS; otherwise the whole
// packed map in global memory.  A cell outside the rectangle reads word 0 and counts nothing.
template <bool LDSR>
__device__ static __forceinline__ int k7_walk(const uint32_t *__restrict__ gmap, const uint32_t *rect, const int2 *pts, int m,
                                              int dx, int dy, int rwc, int rh, int rwpr)
{
    int score = 0;
#pragma unroll 4
    for (int j = 0; j < m; j++) {
        const int2 g = pts[j];
        const int x = g.x + dx, y = g.y + dy;
        const bool in = (unsigned)x < (unsigned)rwc && (unsigned)y < (unsigned)rh;
        const int o = in ? y * rwpr + (x >> 4) : 0;
        uint32_t word;
        if constexpr (LDSR) word = rect[o];
        else word = gmap[o];
        score += hs_lat_class_value(in ? (word >> ((x & 15) * 2)) & 3u : 0u);
    }
    return score;
}

__global__ void __launch_bounds__(K7_LANES) k7_search(const k7_arg A)
{
    __shared__ uint32_t rect_s[K7_RECT_WORDS];
    __shared__ int2 pts_s[K7_CHUNK];
    __shared__ int bb_s[4];
    __shared__ unsigned long long wmax_s[K7_LANES / 64];
    const int tid = threadIdx.x;
    const int k = blockIdx.y;
    const int nx = A.S.nx, ny = A.S.ny, NX = 2 * nx + 1;
    const int TX = 1 << A.txl, TY = K7_LANES >> A.txl;
    const int tile_y = blockIdx.x / A.tiles_x, tile_x = blockIdx.x - tile_y * A.tiles_x;
    const int ix0 = -nx + tile_x * TX, iy0 = -ny + tile_y * TY;            // the tile's first translation
    const int ix1 = min(ix0 + TX - 1, nx), iy1 = min(iy0 + TY - 1, ny);    // ... and its last one inside the lattice
    const int ix = ix0 + (tid & (TX - 1)), iy = iy0 + (tid >> A.txl);
    const bool active = ix <= nx && iy <= ny;
    const hs_lat_heading H = hs_lat_heading_of(A.stm, A.S.centre[0], A.S.centre[1], hs_lat_theta(A.S, k));

    // the bounding box of the heading's point cells
    if (tid < 4) bb_s[tid] = (tid & 1) ? INT_MIN : INT_MAX;                // {min x, max x, min y, max y}
    __syncthreads();
    {
        int x_lo = INT_MAX, x_hi = INT_MIN, y_lo = INT_MAX, y_hi = INT_MIN;
        for (int i = tid; i < A.n; i += K7_LANES) {
            const float2 p = A.pts[i];
            int gx, gy;
            if (hs_lat_point_cell(H, p.x, p.y, &gx, &gy)) { x_lo = min(x_lo, gx); x_hi = max(x_hi, gx); y_lo = min(y_lo, gy); y_hi = max(y_hi, gy); }
        }
        if (x_lo <= x_hi) { atomicMin(&bb_s[0], x_lo); atomicMax(&bb_s[1], x_hi); atomicMin(&bb_s[2], y_lo); atomicMax(&bb_s[3], y_hi); }
    }
    __syncthreads();
    // the rectangle of the class map this tile can touch, clipped to the map, in whole words; none: every score of the tile is 0
    int rx0 = 0, ry0 = 0, rwpr = 0, rh = 0;
    bool in_lds = true;
    if (bb_s[0] <= bb_s[1]) {
        const int x_lo = max(bb_s[0] + ix0, 0), x_hi = min(bb_s[1] + ix1, A.w - 1);
        const int y_lo = max(bb_s[2] + iy0, 0), y_hi = min(bb_s[3] + iy1, A.h - 1);
        if (x_lo <= x_hi && y_lo <= y_hi) {
            const int w0 = x_lo >> 4;
            rwpr = (x_hi >> 4) - w0 + 1; rh = y_hi - y_lo + 1;
            rx0 = w0 * 16; ry0 = y_lo;
            in_lds = rwpr * rh <= K7_RECT_WORDS;                           // (at most 2048 words x 32768 rows: no overflow)
            if (in_lds) {
                const uint32_t *src = A.cls + (size_t)y_lo * A.wpr + w0;
                for (int i = tid; i < rwpr * rh; i += K7_LANES) {
                    const int r = i / rwpr;
                    rect_s[i] = src[(size_t)r * A.wpr + (i - r * rwpr)];
                }
            } else { rx0 = 0; ry0 = 0; rwpr = A.wpr; rh = A.h; }           // the whole packed map, from global memory
        }
    }
    const int rwc = rwpr * 16;                                             // (cells past the level's width in the last word: zero bits)
    const int dx = ix - rx0, dy = iy - ry0;
    int score = 0;
    for (int base = 0; base < A.n; base += K7_CHUNK) {
        const int m = min(K7_CHUNK, A.n - base);
        if (base > 0) __syncthreads();                                     // (the previous chunk has been walked)
        for (int i = tid; i < m; i += K7_LANES) {
            const float2 p = A.pts[base + i];
            int gx, gy;
            if (!hs_lat_point_cell(H, p.x, p.y, &gx, &gy)) { gx = K7_IGNORED; gy = K7_IGNORED; }
            pts_s[i] = make_int2(gx, gy);
        }
        __syncthreads();                                                   // (the points, and with the first chunk the rectangle)
        if (active) {
            if (in_lds) score += k7_walk<true>(A.cls, rect_s, pts_s, m, dx, dy, rwc, rh, rwpr);
            else score += k7_walk<false>(A.cls, rect_s, pts_s, m, dx, dy, rwc, rh, rwpr);
        }
    }
    const uint32_t flat = (uint32_t)((iy + ny) * NX + (ix + nx));
    if (active && A.scores) A.scores[((size_t)k * (2 * ny + 1) + (size_t)(iy + ny)) * NX + (size_t)(ix + nx)] = score;
    unsigned long long key = active ? hs_lat_key(score, flat) : 0ull;      // (a node's key is never 0: its high word is at least 1)
    for (int msk = 1; msk < 64; msk <<= 1) {
        const unsigned long long o = __shfl_xor(key, msk);
        key = o > key ? o : key;
    }
    if ((tid & 63) == 0) wmax_s[tid >> 6] = key;
    __syncthreads();
    if (tid == 0) {
        for (int v = 1; v < K7_LANES / 64; v++) key = wmax_s[v] > key ? wmax_s[v] : key;
        __hip_atomic_fetch_max(A.keys + k, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------
// What a search needs, made by the first one and kept: the class map (grown to the largest level searched), the device block of
// keys and scores, its pinned twin the results reach the host through, and the event the bounded wait polls.
struct hs_lattice {
    uint32_t *d_cls; size_t cap_cls;                                       // words
    unsigned char *d_out; size_t cap_out;                                  // n_theta keys, then the score volume
    unsigned char *h_out; size_t cap_h;
    hipEvent_t ev;
};

void hs_lat_free(slamhip_hs *hs)
{
    hs_lattice *lt = hs->lat;
    if (!lt) return;
    (void)hipFree(lt->d_cls); (void)hipFree(lt->d_out);
    if (lt->h_out) (void)hipHostFree(lt->h_out);
    if (lt->ev) (void)hipEventDestroy(lt->ev);
    delete lt;
    hs->lat = nullptr;
}

static int32_t hs_lat_check_spec(const slamhip_hs *hs, const slamhip_lattice_spec *S)
{
    SH_CHECK_ARG(hs && S);
    if (S->level < 0 || S->level >= hs->n_levels) SH_FAIL(SLAMHIP_ERR_INVALID, "lattice: level %d of %d", S->level, hs->n_levels);
    if (S->nx < 0 || S->nx > HS_LAT_MAX_HALF || S->ny < 0 || S->ny > HS_LAT_MAX_HALF)
        SH_FAIL(SLAMHIP_ERR_INVALID, "lattice: nx = %d, ny = %d must lie in [0, %d]", S->nx, S->ny, HS_LAT_MAX_HALF);
    if (S->n_theta < 1 || S->n_theta > HS_LAT_MAX_THETA) SH_FAIL(SLAMHIP_ERR_INVALID, "lattice: n_theta = %d must lie in [1, %d]", S->n_theta, HS_LAT_MAX_THETA);
    if ((int64_t)S->n_theta * (2 * S->nx + 1) * (2 * S->ny + 1) > (int64_t)HS_LAT_MAX_NODES)
        SH_FAIL(SLAMHIP_ERR_INVALID, "lattice: %lld nodes, more than 2^26", (long long)S->n_theta * (2 * S->nx + 1) * (2 * S->ny + 1));
    if (!(isfinite(S->centre[0]) && isfinite(S->centre[1]) && isfinite(S->centre[2]) && isfinite(S->dtheta)))
        SH_FAIL(SLAMHIP_ERR_INVALID, "lattice: centre and dtheta must be finite");
    return SLAMHIP_OK;
}

static int32_t hs_lat_grow(void **p, size_t *cap, size_t want, bool pinned)
{
    if (*cap >= want) return SLAMHIP_OK;
    if (*p) { if (pinned) (void)hipHostFree(*p); else (void)hipFree(*p); *p = nullptr; *cap = 0; }
    if ((pinned ? hipHostMalloc(p, want, hipHostMallocDefault) : hipMalloc(p, want)) != hipSuccess) {
        (void)hipGetLastError();
        *p = nullptr;
        SH_FAIL(SLAMHIP_ERR_NOMEM, "lattice: allocation of %zu bytes of %s memory failed", want, pinned ? "pinned host" : "device");
    }
    *cap = want;
    return SLAMHIP_OK;
}

// The search into the library's pinned block: *keys (n_theta) and, if asked for, *scores point into it and stay valid until the
// next search of this hs.
static int32_t hs_lat_run(slamhip_hs *hs, const slamhip_lattice_spec *S, bool want_scores, const uint64_t **keys, const int32_t **scores)
{
    SH_TRY(hs_lat_check_spec(hs, S));
    if (hs->n_points <= 0) SH_FAIL(SLAMHIP_ERR_STATE, "lattice: no scan (slamhip_hs_set_scan first)");
    slamhip_ctx *ctx = hs->ctx;
    if (ctx->poisoned) SH_FAIL(SLAMHIP_ERR_TIMEOUT, "the context was poisoned by a blocking wait that timed out; destroy it");
    SH_HIP(hipSetDevice(ctx->device));
    if (!hs->lat) {
        hs->lat = new (std::nothrow) hs_lattice();                        // (value-initialised: nothing allocated yet)
        if (!hs->lat) SH_FAIL(SLAMHIP_ERR_NOMEM, "out of host memory");
    }
    hs_lattice *lt = hs->lat;
    if (!lt->ev) SH_HIP(hipEventCreateWithFlags(&lt->ev, hipEventDisableTiming));
    const hs_level &L = hs->lv[S->level];
    const int wpr = (L.w + 15) / 16;
    const int NX = 2 * S->nx + 1, NY = 2 * S->ny + 1;
    const size_t key_bytes = sizeof(uint64_t) * (size_t)S->n_theta;
    const size_t out_bytes = key_bytes + (want_scores ? sizeof(int32_t) * (size_t)S->n_theta * NX * NY : 0);
    // (the blocks are idle: every search waits for its own launches, and a search that timed out has poisoned the context)
    SH_TRY(hs_lat_grow((void **)&lt->d_cls, &lt->cap_cls, sizeof(uint32_t) * (size_t)wpr * L.h, false));
    SH_TRY(hs_lat_grow((void **)&lt->d_out, &lt->cap_out, out_bytes, false));
    SH_TRY(hs_lat_grow((void **)&lt->h_out, &lt->cap_h, out_bytes, true));
    SH_TRY(hs_flush_scan(hs));
    SH_HIP(hipMemsetAsync(lt->d_out, 0, key_bytes, ctx->stream));
    {
        sh_timer t(ctx, SLAMHIP_K_HS_LATTICE_PACK);
        hipLaunchKernelGGL(k7_pack, dim3((unsigned)sh_div_up(wpr * L.h, 256)), dim3(256), 0, ctx->stream, (const slamhip_cell *)L.d_cells, L.w, L.h, wpr, lt->d_cls);
    }
    SH_HIP(hipGetLastError());
    k7_arg A;
    A.pts = hs->d_pts; A.n = hs->n_points;
    A.cls = lt->d_cls; A.w = L.w; A.h = L.h; A.wpr = wpr;
    A.stm = L.stm;
    A.S = *S;
    A.txl = NX > 32 ? 6 : 4;                                               // 64 x 4 translations per workgroup; a narrow lattice 16 x 16
    const int TX = 1 << A.txl, TY = K7_LANES >> A.txl;
    A.tiles_x = sh_div_up(NX, TX);
    A.keys = (unsigned long long *)lt->d_out;
    A.scores = want_scores ? (int32_t *)(lt->d_out + key_bytes) : (int32_t *)nullptr;
    {
        sh_timer t(ctx, SLAMHIP_K_HS_LATTICE);
        hipLaunchKernelGGL(k7_search, dim3((unsigned)(A.tiles_x * sh_div_up(NY, TY)), (unsigned)S->n_theta), dim3(K7_LANES), 0, ctx->stream, A);
    }
    SH_HIP(hipGetLastError());
    SH_HIP(hipMemcpyAsync(lt->h_out, lt->d_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    SH_HIP(hipEventRecord(lt->ev, ctx->stream));
    SH_TRY(sh_event_wait(ctx, lt->ev));
    hs->launch_done = hs->launch_count;                                    // (the stream has drained up to here)
    *keys = (const uint64_t *)lt->h_out;
    if (scores) *scores = want_scores ? (const int32_t *)(lt->h_out + key_bytes) : (const int32_t *)nullptr;
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_lattice_search(slamhip_hs *hs, const slamhip_lattice_spec *spec, uint64_t *out_keys, int32_t *out_scores)
{
    SH_CHECK_ARG(hs && spec && out_keys);
    const uint64_t *keys = nullptr; const int32_t *scores = nullptr;
    SH_TRY(hs_lat_run(hs, spec, out_scores != nullptr, &keys, &scores));
    memcpy(out_keys, keys, sizeof(uint64_t) * (size_t)spec->n_theta);
    if (out_scores) memcpy(out_scores, scores, sizeof(int32_t) * (size_t)spec->n_theta * (2 * spec->nx + 1) * (2 * spec->ny + 1));
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_lattice_node_pose(slamhip_hs *hs, const slamhip_lattice_spec *spec, int32_t k, int32_t flat, float out_pose[3])
{
    SH_CHECK_ARG(out_pose);
    SH_TRY(hs_lat_check_spec(hs, spec));
    const int NX = 2 * spec->nx + 1, NY = 2 * spec->ny + 1;
    SH_CHECK_ARG(k >= 0 && k < spec->n_theta && flat >= 0 && flat < NX * NY);
    const hs_level &L = hs->lv[spec->level];
    hs_lat_node_pose(*spec, L.cell, L.stm, k, flat % NX - spec->nx, flat / NX - spec->ny, out_pose);
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_relocalise(slamhip_hs *hs, const slamhip_lattice_spec *spec, int32_t B, float out_pose[3],
                                         slamhip_match_report *out_report, slamhip_reloc_info *out_info)
{
    SH_CHECK_ARG(hs && spec && out_pose && out_report && out_info && B >= 1 && B <= 64);
    const uint64_t *keys = nullptr;
    SH_TRY(hs_lat_run(hs, spec, false, &keys, nullptr));
    const int nh = B < spec->n_theta ? B : spec->n_theta;
    int order[HS_LAT_MAX_THETA];
    for (int k = 0; k < spec->n_theta; k++) order[k] = k;
    std::stable_sort(order, order + spec->n_theta, [keys](int a, int b) { return keys[a] > keys[b]; });   // (descending; equal keys: the lower k first)
    const hs_level &L = hs->lv[spec->level];
    const int NX = 2 * spec->nx + 1;
    float hints[3 * 64];
    int node[64][4];                                                       // k, ix, iy, score
    for (int i = 0; i < nh; i++) {
        const int k = order[i], flat = (int)hs_lat_key_flat(keys[k]);
        node[i][0] = k; node[i][1] = flat % NX - spec->nx; node[i][2] = flat / NX - spec->ny; node[i][3] = hs_lat_key_score(keys[k]);
        hs_lat_node_pose(*spec, L.cell, L.stm, k, node[i][1], node[i][2], hints + 3 * i);
    }
    int32_t best = -1;
    const hs_report_req rq = { out_report, &best };
    SH_TRY(hs_run_match(hs, hints, nh, out_pose, -1, 0, nullptr, &rq));    // slamhip_hs_match_best
    if (best < 0 || best >= nh) SH_FAIL(SLAMHIP_ERR_STATE, "relocalise: the matcher's winner %d is none of the %d hints", best, nh);
    out_info->n_hints = nh; out_info->best_hint = best;
    out_info->k = node[best][0]; out_info->ix = node[best][1]; out_info->iy = node[best][2]; out_info->score = node[best][3];
    out_info->top_score = node[0][3];
    return SLAMHIP_OK;
}

// CPU-side test hook: hs_lat_point_cell, the text the kernel runs
extern "C" int32_t slamhip_debug_lattice_cells(float cell_length, const float centre[3], float theta, const float *xy, int32_t n, int32_t *out_gxgy)
{
    SH_CHECK_ARG(centre && n >= 0 && ((xy && out_gxgy) || n == 0) && cell_length > 0.0f);
    const hs_lat_heading H = hs_lat_heading_of(1.0f / cell_length, centre[0], centre[1], theta);
    for (int i = 0; i < n; i++) {
        int gx, gy;
        if (!hs_lat_point_cell(H, xy[2 * i], xy[2 * i + 1], &gx, &gy)) { gx = HS_LAT_IGNORED; gy = HS_LAT_IGNORED; }
        out_gxgy[2 * i] = gx; out_gxgy[2 * i + 1] = gy;
    }
    return SLAMHIP_OK;
}
