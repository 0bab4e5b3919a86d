// hector.hip -- the HectorSLAM operator object (slamhip_hs): create / destroy / reset, the scan, uploads, downloads and the small
// kernels over a level's cells.  K4 (scan matcher): hs_match.hip; K5 (grid update): hs_update.hip; K6 (scrolling window and its
// backing store): hs_window.hip, the world behind them: hs_world.hip; K7 (pose-lattice search): hs_lattice.hip; HectorSLAMProcessor: hs_processor.hip; shared state and
// helpers: hs_internal.h.
#include "hs_blocks.h"

__global__ void k5_fill_cells(slamhip_cell *cells, float *prob, size_t n)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) { cells[i] = hs_reset_cell(); prob[i] = HS_RESET_PROB; }
}

// the cached probabilities of an uploaded mapArray
__global__ void k5_refresh_prob(const slamhip_cell *cells, float *prob, size_t n)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) prob[i] = hs_prob_v(cells[i].value);
}
// GridMap.GetBitmapData (GridMap.cs:104-115)
__global__ void k5_bitmap(const slamhip_cell *cells, uint8_t *out, size_t n)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = cells[i].value;
    const int sgn = (v > 0.0f) - (v < 0.0f);
    out[i] = (uint8_t)(127 - sgn * 127);                                   // :111
}
// GridMap.GetMapExtends (GridMap.cs:147-207): bounding rectangle of the cells whose Value != 0.  ext = {xMax, yMax, xMin, yMin},
// preset to {-1, -1, 10000, 10000} (:149-150 -- the reference's minima start at 10000 whatever the map size).
__global__ void k5_extends_init(int32_t *ext)
{
    if (threadIdx.x < 4) ext[threadIdx.x] = threadIdx.x < 2 ? -1 : 10000;
}
__global__ __launch_bounds__(256) void k5_extends(const slamhip_cell *cells, int w, int h, int32_t *ext)
{
    int xmax = -1, ymax = -1, xmin = 10000, ymin = 10000;
    for (int y = blockIdx.x; y < h; y += gridDim.x) {                      // one row per workgroup pass: coalesced reads
        const slamhip_cell *row = cells + (size_t)y * w;
        for (int x = threadIdx.x; x < w; x += 256)
            if (row[x].value != 0.0f) {                                          // :161 (a NaN cell counts, as in the reference)
                xmax = max(xmax, x); xmin = min(xmin, x);
                ymax = max(ymax, y); ymin = min(ymin, y);
            }
    }
    for (int m = 1; m < 64; m <<= 1) {
        xmax = max(xmax, __shfl_xor(xmax, m)); ymax = max(ymax, __shfl_xor(ymax, m));
        xmin = min(xmin, __shfl_xor(xmin, m)); ymin = min(ymin, __shfl_xor(ymin, m));
    }
    if ((threadIdx.x & 63) == 0 && xmax >= 0) {
        atomicMax(ext + 0, xmax); atomicMax(ext + 1, ymax);
        atomicMin(ext + 2, xmin); atomicMin(ext + 3, ymin);
    }
}
__global__ void k5_probability(const slamhip_cell *cells, const int32_t *idx, int n, float *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = hs_prob_v(cells[idx[i]].value);                   // OccGridMap.GetCachedProbability (:97-107)
}
// ... through the reference's cache (slamhip_hs_set_reference_cache): :99-106 with the fills the matcher's taps make
// (hs_cache_taps) -- repeated indices in one list give what the reference's sequential calls give, in any order
__global__ void k5_probability_cached(const float *prob, unsigned long long *cache, int epoch, const int32_t *idx, int n, float *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int c = idx[i];
    const unsigned long long e = __hip_atomic_load(cache + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    float v = hs_cache_entry_value(e);                                     // :106
    if (!hs_cache_entry_hit(e, epoch)) {                                   // :99
        v = prob[c];                                                       // :101-102
        __hip_atomic_store(cache + c, hs_cache_entry(v, epoch), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);   // :103
    }
    out[i] = v;
}
// new CachedMapElement[] with every Index = -1 (OccGridMap.cs:38-42): {Value 0, Index -1}
__global__ void k5_cache_clear(unsigned long long *cache, size_t n)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) cache[i] = hs_cache_entry(0.0f, -1);
}

void hs_cache_clear_enqueue(slamhip_hs *hs, int level)
{
    hs_level &L = hs->lv[level];
    const size_t n = (size_t)L.w * L.h;
    hipLaunchKernelGGL(k5_cache_clear, dim3((unsigned)(n / 256 < 1024 ? (n + 255) / 256 : 1024)), dim3(256), 0, hs->ctx->stream, L.d_cache, n);
}

// the two words of slamhip_hs_checksum (common.h: k_checksum's definition, per member of the cell): out[0] over the values' bit
// patterns, out[1] over the update indices
__global__ void __launch_bounds__(256) k5_checksum_cells(const slamhip_cell *__restrict__ cells, size_t n, unsigned long long *__restrict__ out)
{
    unsigned long long av = 0, au = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const slamhip_cell c = cells[i];
        av += sh_mix64(((unsigned long long)i << 32) | (unsigned long long)__float_as_uint(c.value));
        au += sh_mix64(((unsigned long long)i << 32) | (unsigned long long)(uint32_t)c.update_index);
    }
    for (int off = 32; off > 0; off >>= 1) { av += __shfl_down(av, off, 64); au += __shfl_down(au, off, 64); }
    if ((threadIdx.x & 63) == 0) { atomicAdd(out, av); atomicAdd(out + 1, au); }
}

// ---- host side ---------------------------------------------------------------------------------------------------
static float prob_to_logodds(float prob) { return hs_prob_to_logodds(prob); }   // OccGridMap.cs:86-90 (hs_internal.h: slamhip_debug_render forms them by the same text)

// the units' live blocks (hs_block, hs_blocks.h)
std::atomic<int64_t> hs_live_blocks{0}, hs_live_bytes{0};
extern "C" int32_t slamhip_debug_live_blocks(int64_t *out_blocks, int64_t *out_bytes)
{
    if (out_blocks) *out_blocks = hs_live_blocks.load(std::memory_order_relaxed);
    if (out_bytes) *out_bytes = hs_live_bytes.load(std::memory_order_relaxed);
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_destroy(slamhip_hs *hs)
{
    if (!hs) return SLAMHIP_OK;
    (void)hipSetDevice(hs->ctx->device);
    (void)hipStreamSynchronize(hs->ctx->stream);
    for (int l = 0; l < hs->n_levels; l++) {
        (void)hipFree(hs->lv[l].d_cells); (void)hipFree(hs->lv[l].d_prob); (void)hipFree(hs->lv[l].d_cache);
        (void)hipFree(hs->lv[l].d_cells_alt); (void)hipFree(hs->lv[l].d_prob_alt);
    }
    hs_bk_free(hs);
    hs_units_drop_all(hs);
    (void)hipFree(hs->d_pts_base); (void)hipFree(hs->d_io);
    if (hs->h_pts) (void)hipHostFree(hs->h_pts);
    if (hs->ev_pts) (void)hipEventDestroy(hs->ev_pts);
    if (hs->ev_call) (void)hipEventDestroy(hs->ev_call);
    (void)hipFree(hs->d_k5_sec);
    (void)hipFree(hs->d_k5_byidx); (void)hipFree(hs->d_k5_cand); (void)hipFree(hs->d_k5_start); (void)hipFree(hs->d_k5_hdr);
    if (hs->h_io) (void)hipHostFree(hs->h_io);
    (void)hipFree(hs->d_rep); (void)hipFree(hs->d_best_key);
    if (hs->h_rep) (void)hipHostFree(hs->h_rep);
    free(hs);
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_reset(slamhip_hs *hs)
{
    SH_CHECK_ARG(hs);
    SH_HIP(hipSetDevice(hs->ctx->device));
    for (int l = 0; l < hs->n_levels; l++) {
        hs_level &L = hs->lv[l];
        hipLaunchKernelGGL(k5_fill_cells, dim3(1024), dim3(256), 0, hs->ctx->stream, L.d_cells, L.d_prob, (size_t)L.w * L.h);                   // GridMap.Reset :56-62
        L.curr_update_index = 0;                                           // OccGridMap.Reset :244-252
        L.curr_cache_index = 0;                                            // :248 (the cache entries are left as they are)
    }
    if (hs->bk) hs_bk_reset(hs);
    SH_HIP(hipStreamSynchronize(hs->ctx->stream));
    hs->win_ox = hs->win_oy = 0;                                           // (slamhip_hs_shift: an empty map has no frame to keep)
    hs_merge_drop_source(hs);                                              // (slamhip_hs_merge_set_source: a source belongs to the map it was to be merged into)
    hs_hg_drop_slot(hs, 0);                                                // (slamhip_hs_hough: slot 0 held the map that is gone; the source's drop emptied slot 1)
    hs_sg_reset(hs);                                                       // (slamhip_hs_sig_add: the keyframes belonged to the map that is gone)
    hs_pg_reset(hs);                                                       // (slamhip_hs_pg_set: so did the graph of their poses)
    hs_scn_reset(hs);                                                      // (slamhip_hs_scans_add: and their scans -- the two stores' indices stay aligned)
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_create(slamhip_ctx *ctx, float cell_length, int32_t w, int32_t h, int32_t levels, slamhip_hs **out)
{
    SH_CHECK_ARG(ctx && out && levels >= 1 && levels <= HS_MAX_LEVELS && cell_length > 0.0f);
    SH_CHECK_ARG(w >= 2 && h >= 2 && w <= 32768 && h <= 32768 && (w >> (levels - 1)) >= 2 && (h >> (levels - 1)) >= 2);
    SH_HIP(hipSetDevice(ctx->device));
    slamhip_hs *hs = (slamhip_hs *)calloc(1, sizeof(slamhip_hs));
    if (!hs) SH_FAIL(SLAMHIP_ERR_NOMEM, "out of host memory");
    hs->ctx = ctx;
    hs->n_levels = levels;
    hs->odds_occ = 0.9f; hs->odds_free = 0.4f;                            // OccGridMap.cs:24-25
    hs->lo_free = prob_to_logodds(hs->odds_free);                         // :46
    hs->lo_occ = prob_to_logodds(hs->odds_occ);                           // :47
    float res = cell_length;
    int32_t rc = SLAMHIP_OK;
    for (int l = 0; l < levels && rc == SLAMHIP_OK; l++) {                // MapRepMultiMap.cs:49-57
        hs_level &L = hs->lv[l];
        L.w = w; L.h = h; L.cell = res; L.stm = 1.0f / res;               // MapProperties.cs:32
        L.iterations = 3;                                                 // OccGridMap.cs:53
        L.map_t_world = sh_m3x2_mul(sh_m3x2_scale(L.stm), sh_m3x2_translation(0.0f, 0.0f));   // GridMap.cs:46 (offset = 0)
        if (!sh_m3x2_invert(L.map_t_world, &L.world_t_map)) { slamhip_set_error("Map to world matrix is not invertible"); rc = SLAMHIP_ERR_INVALID; break; }  // :47-50
        const size_t n = (size_t)w * h;
        if (hipMalloc(&L.d_cells, sizeof(slamhip_cell) * n) != hipSuccess || hipMalloc(&L.d_prob, sizeof(float) * n) != hipSuccess) {
            slamhip_set_error("device allocation failed (level %d)", l); rc = SLAMHIP_ERR_NOMEM; break;
        }
        w /= 2; h /= 2;                                                   // :55
        res *= 2.0f;                                                      // :56
    }
    if (rc == SLAMHIP_OK) {
        hs->cap_io = 4096;
        if (hipMalloc(&hs->d_io, sizeof(float) * hs->cap_io) != hipSuccess || hipHostMalloc(&hs->h_io, sizeof(float) * hs->cap_io) != hipSuccess) {
            slamhip_set_error("device allocation failed"); rc = SLAMHIP_ERR_NOMEM;
        }
    }
    if (rc == SLAMHIP_OK && hipEventCreateWithFlags(&hs->ev_call, hipEventDisableTiming) != hipSuccess) {
        slamhip_set_error("event creation failed"); rc = SLAMHIP_ERR_HIP;
    }
    if (rc == SLAMHIP_OK) rc = slamhip_hs_reset(hs);
    if (rc != SLAMHIP_OK) { slamhip_hs_destroy(hs); return rc; }
    *out = hs;
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_level_info(slamhip_hs *hs, int32_t level, int32_t *w, int32_t *h, float *cell)
{
    SH_CHECK_ARG(hs && level >= 0 && level < hs->n_levels);
    if (w) *w = hs->lv[level].w;
    if (h) *h = hs->lv[level].h;
    if (cell) *cell = hs->lv[level].cell;
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_set_factors(slamhip_hs *hs, float free_f, float occ_f)
{
    SH_CHECK_ARG(hs);
    hs->odds_free = free_f; hs->lo_free = prob_to_logodds(free_f);        // OccGridMap.cs:58-66
    hs->odds_occ = occ_f;   hs->lo_occ = prob_to_logodds(occ_f);          // :71-79
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_set_iterations(slamhip_hs *hs, const int32_t *it)
{
    SH_CHECK_ARG(hs && it);
    for (int l = 0; l < hs->n_levels; l++) { SH_CHECK_ARG(it[l] >= 0 && it[l] <= 1000); hs->lv[l].iterations = it[l]; }
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_cells_upload(slamhip_hs *hs, int32_t level, const slamhip_cell *cells, size_t n)
{
    SH_CHECK_ARG(hs && cells && level >= 0 && level < hs->n_levels);
    hs_level &L = hs->lv[level];
    SH_CHECK_ARG(n == (size_t)L.w * L.h);
    SH_HIP(hipSetDevice(hs->ctx->device));
    // (the device holds the reference's own layout: a plain copy, then the cached probabilities.  The reference's cache and its
    // epoch -- slamhip_hs_set_reference_cache -- are left as they are: the reference has no upload, and only its own events move them)
    SH_HIP(hipMemcpyAsync(L.d_cells, cells, sizeof(slamhip_cell) * n, hipMemcpyHostToDevice, hs->ctx->stream));
    hipLaunchKernelGGL(k5_refresh_prob, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, hs->ctx->stream, (const slamhip_cell *)L.d_cells, L.d_prob, n);
    SH_HIP(hipStreamSynchronize(hs->ctx->stream));
    // keep the once-per-scan guards meaningful: the next scan's marks must exceed every stored index
    int mx = -1;
    for (size_t i = 0; i < n; i++) if (cells[i].update_index > mx) mx = cells[i].update_index;
    if (mx >= 0) {                      // marks of scan k are 3k+1 / 3k+2 (OccGridMap.cs:116-117,:144)
        const long long need = ((long long)mx / 3 + 1) * 3;                // (64-bit: an index near INT_MAX has no marks above it and moves nothing)
        if (need <= 0x7fffffffLL - 2 && need > L.curr_update_index) L.curr_update_index = (int)need;
    }
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_cells_download(slamhip_hs *hs, int32_t level, slamhip_cell *cells, size_t n)
{
    SH_CHECK_ARG(hs && cells && level >= 0 && level < hs->n_levels);
    hs_level &L = hs->lv[level];
    SH_CHECK_ARG(n == (size_t)L.w * L.h);
    SH_HIP(hipSetDevice(hs->ctx->device));
    SH_HIP(hipMemcpyAsync(cells, L.d_cells, sizeof(slamhip_cell) * n, hipMemcpyDeviceToHost, hs->ctx->stream));
    SH_HIP(hipStreamSynchronize(hs->ctx->stream));
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_bitmap_download(slamhip_hs *hs, int32_t level, uint8_t *out, size_t n)
{
    SH_CHECK_ARG(hs && out && level >= 0 && level < hs->n_levels);
    hs_level &L = hs->lv[level];
    SH_CHECK_ARG(n == (size_t)L.w * L.h);
    SH_HIP(hipSetDevice(hs->ctx->device));
    uint8_t *d = nullptr;
    SH_HIP(hipMalloc(&d, n));
    hipLaunchKernelGGL(k5_bitmap, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, hs->ctx->stream, (const slamhip_cell *)L.d_cells, d, n);
    hipError_t e = hipMemcpyAsync(out, d, n, hipMemcpyDeviceToHost, hs->ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(hs->ctx->stream);
    (void)hipFree(d);
    SH_HIP(e);
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_map_extends(slamhip_hs *hs, int32_t level, int32_t extends[4], int32_t *found)
{
    SH_CHECK_ARG(hs && extends && found && level >= 0 && level < hs->n_levels);
    hs_level &L = hs->lv[level];
    SH_HIP(hipSetDevice(hs->ctx->device));
    int32_t *d = nullptr;
    SH_HIP(hipMalloc(&d, 4 * sizeof(int32_t)));
    hipLaunchKernelGGL(k5_extends_init, dim3(1), dim3(64), 0, hs->ctx->stream, d);
    hipLaunchKernelGGL(k5_extends, dim3(L.h < 2048 ? L.h : 2048), dim3(256), 0, hs->ctx->stream, (const slamhip_cell *)L.d_cells, L.w, L.h, d);
    int32_t e4[4] = {0, 0, 0, 0};
    hipError_t e = hipMemcpyAsync(e4, d, sizeof(e4), hipMemcpyDeviceToHost, hs->ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(hs->ctx->stream);
    (void)hipFree(d);
    SH_HIP(e);
    // :186-205 -- all four must have moved off their start values, otherwise (false, 0, 0, 0, 0)
    const bool ok = e4[0] != -1 && e4[1] != -1 && e4[2] != 10000 && e4[3] != 10000;
    for (int i = 0; i < 4; i++) extends[i] = ok ? e4[i] : 0;
    *found = ok ? 1 : 0;
    return SLAMHIP_OK;
}

// Replica check (one match is too small to shard, the grids are replicas): checksums of a level's log-odds
// (bit patterns) and update indices behind everything enqueued so far; definition in common.h (sh_mix64 / k_checksum).
extern "C" int32_t slamhip_hs_checksum(slamhip_hs *hs, int32_t level, uint64_t out[2])
{
    SH_CHECK_ARG(hs && out && level >= 0 && level < hs->n_levels);
    hs_level &L = hs->lv[level];
    slamhip_ctx *ctx = hs->ctx;
    SH_HIP(hipSetDevice(ctx->device));
    unsigned long long *d = nullptr;
    SH_HIP(hipMalloc(&d, 2 * sizeof(unsigned long long)));
    hipError_t e = hipMemsetAsync(d, 0, 2 * sizeof(unsigned long long), ctx->stream);
    if (e == hipSuccess) {
        const size_t n = (size_t)L.w * L.h, want = (n + 2047) / 2048;
        hipLaunchKernelGGL(k5_checksum_cells, dim3((unsigned)(want < 1 ? 1 : want > 2048 ? 2048 : want)), dim3(256), 0, ctx->stream, (const slamhip_cell *)L.d_cells, n, d);
        e = hipMemcpyAsync(out, d, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    (void)hipFree(d);
    SH_HIP(e);
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_probability(slamhip_hs *hs, int32_t level, const int32_t *indices, int32_t n, float *out)
{
    SH_CHECK_ARG(hs && indices && out && n > 0 && level >= 0 && level < hs->n_levels);
    hs_level &L = hs->lv[level];
    for (int i = 0; i < n; i++) SH_CHECK_ARG(indices[i] >= 0 && (size_t)indices[i] < (size_t)L.w * L.h);
    SH_HIP(hipSetDevice(hs->ctx->device));
    int32_t *di = nullptr; float *dout = nullptr;
    SH_HIP(hipMalloc(&di, sizeof(int32_t) * n));
    hipError_t e = hipMalloc(&dout, sizeof(float) * n);
    if (e == hipSuccess) e = hipMemcpyAsync(di, indices, sizeof(int32_t) * n, hipMemcpyHostToDevice, hs->ctx->stream);
    if (e == hipSuccess) {
        if (hs->ref_cache)
            hipLaunchKernelGGL(k5_probability_cached, dim3(sh_div_up(n, 256)), dim3(256), 0, hs->ctx->stream, (const float *)L.d_prob, L.d_cache,
                               L.curr_cache_index, (const int32_t *)di, n, dout);
        else
            hipLaunchKernelGGL(k5_probability, dim3(sh_div_up(n, 256)), dim3(256), 0, hs->ctx->stream, (const slamhip_cell *)L.d_cells, di, n, dout);
        e = hipMemcpyAsync(out, dout, sizeof(float) * n, hipMemcpyDeviceToHost, hs->ctx->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(hs->ctx->stream);
    (void)hipFree(di); (void)hipFree(dout);
    SH_HIP(e);
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_set_scan(slamhip_hs *hs, const float *xy, int32_t n, const float origin[2])
{
    SH_CHECK_ARG(hs && n >= 0 && (xy || n == 0));
    SH_HIP(hipSetDevice(hs->ctx->device));
    hs->origin[0] = origin ? origin[0] : 0.0f;
    hs->origin[1] = origin ? origin[1] : 0.0f;
    hs->n_points = 0;                                  // (stays "no scan" if anything below fails)
    if (n == 0) return SLAMHIP_OK;
    if (n > hs->cap_points) {
        SH_HIP(hipStreamSynchronize(hs->ctx->stream));
        (void)hipFree(hs->d_pts_base); hs->d_pts_base = nullptr; hs->d_pts = nullptr; hs->cap_points = 0;
        if (hs->h_pts) { (void)hipHostFree(hs->h_pts); hs->h_pts = nullptr; }
        const int cap = (n + n / 4 + 64 + 1) & ~1;                         // (even: the upload launch moves 16-byte units)
        SH_HIP(hipMalloc(&hs->d_pts_base, sizeof(float2) * (size_t)cap * 2));
        hs->pts_use[0] = hs->pts_use[1] = 0;
        SH_HIP(hipHostMalloc(&hs->h_pts, sizeof(float2) * (size_t)cap + 64, hipHostMallocMapped | hipHostMallocCoherent));   // (+ the upload's completion word)
        memset(hs->h_pts + 2 * (size_t)cap, 0, 64);
        hs->upload_seq = 0;
        if (!hs->ev_pts) SH_HIP(hipEventCreateWithFlags(&hs->ev_pts, hipEventDisableTiming));
        hs->cap_points = cap;
        hs->pts_in_flight = false;
    }
    uint32_t *up_flag = (uint32_t *)(hs->h_pts + 2 * (size_t)hs->cap_points);
    if (hs->upload_pending) hs->upload_pending = false; // (the staged scan was never consumed: nothing was launched, the block is ours)
    else if (hs->pts_in_flight) {                       // the previous copy has left the staging block
        if (!hs->ctx->mail_off) SH_TRY(sh_upload_wait(hs->ctx, up_flag, hs->upload_seq));
        else SH_HIP(hipEventSynchronize(hs->ev_pts));
        hs->pts_in_flight = false;
    }
    memcpy(hs->h_pts, xy, sizeof(float) * 2 * (size_t)n);
    hs->pts_buf ^= 1;
    hs->d_pts = hs->d_pts_base + (size_t)hs->pts_buf * (size_t)hs->cap_points;
    if (hs->ctx->large_bar && hs->pts_use[hs->pts_buf] <= hs->launch_done) {
        // (the block is idle and the host can store into device memory: the upload is a copy by the CPU through the PCIe aperture,
        // see slamhip_cs_set_scan -- the match then reads its points from device memory instead of pulling them over PCIe)
        memcpy(hs->d_pts, xy, sizeof(float) * 2 * (size_t)n);
        __builtin_ia32_sfence();
        hs->upload_pending = false;
    } else if (!hs->ctx->mail_off) {                    // (see slamhip_cs_set_scan: the per-scan path is launches only, and the upload is left pending)
        hs->upload_pending = true;
        hs->upload_bytes = (sizeof(float) * 2 * (size_t)n + 15) & ~(size_t)15;
    } else {
        SH_HIP(hipMemcpyAsync(hs->d_pts, hs->h_pts, sizeof(float) * 2 * (size_t)n, hipMemcpyHostToDevice, hs->ctx->stream));
        SH_HIP(hipEventRecord(hs->ev_pts, hs->ctx->stream));
        hs->pts_in_flight = true;
    }
    hs->n_points = n;
    return SLAMHIP_OK;
}

// launches the scan upload that slamhip_hs_set_scan left pending (every launch that reads the points calls it first)
int32_t hs_flush_scan(slamhip_hs *hs)
{
    hs->pts_use[hs->pts_buf] = ++hs->launch_count;
    if (!hs->upload_pending) return SLAMHIP_OK;
    // (the upload state is committed once the launch that carries it is in the stream: on an error the scan stays pending)
    SH_TRY(sh_upload(hs->ctx, hs->h_pts, hs->d_pts, hs->upload_bytes, (uint32_t *)(hs->h_pts + 2 * (size_t)hs->cap_points), hs->upload_seq + 1));
    hs->upload_pending = false;
    hs->upload_seq++;
    hs->pts_in_flight = true;
    return SLAMHIP_OK;
}
