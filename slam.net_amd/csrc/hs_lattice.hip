// hs_lattice.hip -- K7, the pose-lattice (correlative) search of HectorSLAM: relocalisation in a loaded map (slamhip_hs_lattice_search,
// slamhip_hs_lattice_node_pose, slamhip_hs_relocalise, slamhip_debug_lattice_cells), in the window or anywhere in the world behind
// it (slamhip_hs_world_lattice_search, slamhip_hs_relocalise_world).  No reference counterpart: the reference's
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
// The WORLD search (window over tiles, Reset elsewhere) differs in the class map alone: it covers a rectangle R of the level -- the
// bounding box of the window and of every tile of the level (world_pack_plan.h), cell (x0, y0) of the window's frame its first --
// and k7_search subtracts (x0, y0) from every point cell; the window search is the case R = the window, (x0, y0) = (0, 0).
//  * k7_pack_world, ONE launch behind a memset of R's words to zero (holes between tiles, and what no tile holds, are class 0).
//    A WORKGROUP owns a job piece, as in k6_world_put -- whole rows of the window or of one tile's part outside the window, cut on
//    the host by hs_cut_rows; the 32-byte records reach the device in a block the library owns.  Pieces are disjoint in cells but
//    their edges fall anywhere in a 16-cell word (a tile's edge, (ox >> level) odd): a lane forms the bits of the up to 16 cells
//    that one piece row has in one word, stores the word plainly if the row covers all of it, and merges it with a 32-bit atomic
//    OR otherwise.  No word is both stored and merged: a word that one row covers wholly holds no cell of another piece.
#include "hs_blocks.h"
#include "hs_tiles.h"
#include "hs_lattice.h"
#include "world_pack_plan.h"
#include <algorithm>
#include <math.h>

#define K7_LANES 256
#define K7_CHUNK 1024                      // points per LDS chunk (8 KB)
// (gx, gy) of an ignored point in LDS, taken as it is (the origin is not subtracted).  The walk adds dx = ix - rx0 to it with
// |ix| <= 4096 and 0 <= rx0 < 2^28 (a rectangle starts inside R, and R has at most 2^28 cells): the sum lies in
// (-2^30 - 2^28 - 4096, -2^30 + 4096], negative -- outside every rectangle -- and far from overflow.  A point that counts has
// |gx| < 2^24 and -2^28 < x0 <= 0 (R contains the window's cell (0, 0)), so gx - x0 lies in (-2^24, 2^24 + 2^28) and neither the
// bounding box nor gx - x0 + dx overflows.
#define K7_IGNORED (-(1 << 30))

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

// ---- the world class map ---------------------------------------------------------------------------------------------------------
// a job piece: nx x ny cells from `src` (rows of `pitch` cells: the window's array or a tile slot's cells) go to R from cell (rx, ry)
#define K7W_LANES 128
struct k7w_piece { const slamhip_cell *src; int32_t pitch, rx, ry; uint16_t nx, ny; uint32_t pad[2]; };
static_assert(sizeof(k7w_piece) == 32, "a job piece is two 16-byte words");

__global__ void __launch_bounds__(K7W_LANES) k7_pack_world(const k7w_piece *__restrict__ pieces, int wpr, uint32_t *__restrict__ out)
{
    const k7w_piece J = pieces[blockIdx.x];
    const int nx = J.nx;
    const int w0 = J.rx >> 4;                                              // the first word a row of the piece touches (rx >= 0)
    const int nw = ((J.rx + nx - 1) >> 4) - w0 + 1;                        // ... and how many
    const int items = nw * (int)J.ny;                                      // (at most K6P_CELLS cells: a few hundred)
    for (int i = threadIdx.x; i < items; i += K7W_LANES) {
        const int r = i / nw, wi = i - r * nw;
        const int e0 = (w0 + wi) * 16 - J.rx;                              // the word's first cell, counted in the piece's row: may be negative
        const slamhip_cell *row = J.src + (size_t)r * J.pitch;
        uint32_t word = 0;
#pragma unroll
        for (int b = 0; b < 16; b++)
            if (e0 + b >= 0 && e0 + b < nx) word |= hs_lat_class_bits(row[e0 + b].value) << (2 * b);
        uint32_t *dst = out + ((size_t)(J.ry + r) * wpr + (size_t)(w0 + wi));
        if (e0 >= 0 && e0 + 16 <= nx) *dst = word;                         // the row covers the whole word
        else if (word) atomicOr(dst, word);                                // an edge: another piece (or nobody) has the other cells
    }
}

struct k7_arg {
    const float2 *pts; int n;
    const uint32_t *cls; int w, h, wpr;    // the packed class map: the level's, or R's
    int x0, y0;                            // the map's first cell in the window's frame: (0, 0), or R's origin
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
            if (hs_lat_point_cell(H, p.x, p.y, &gx, &gy)) {
                gx -= A.x0; gy -= A.y0;
                x_lo = min(x_lo, gx); x_hi = max(x_hi, gx); y_lo = min(y_lo, gy); y_hi = max(y_hi, gy);
            }
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
            in_lds = rwpr * rh <= K7_RECT_WORDS;                           // (at most 2^28 cells in rows of whole words: no overflow)
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
            else { gx -= A.x0; gy -= A.y0; }                               // (integers: exact)
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
// keys and scores, and its pinned twin the results reach the host through.
struct hs_lattice {
    hs_block<uint32_t, HS_MEM_DEVICE> d_cls;                                       // words
    hs_block<unsigned char, HS_MEM_DEVICE> d_out;                                  // n_theta keys, then the score volume
    hs_block<unsigned char, HS_MEM_PINNED> h_out;
    // the world search: the job pieces in device memory, and the host vectors they are planned in
    hs_block<unsigned char, HS_MEM_DEVICE> d_pieces;
    std::vector<int64_t> tiles;                                            // (ty, tx) of every tile of the level
    std::vector<slamhip_world_job> plan;
    std::vector<k7w_piece> pieces;
};

int32_t hs_lat_check_spec(const slamhip_hs *hs, const slamhip_lattice_spec *S, bool cap_nodes)
{
    SH_CHECK_ARG(hs && S);
    if (S->level < 0 || S->level >= hs->n_levels) SH_FAIL(SLAMHIP_ERR_INVALID, "lattice: level %d of %d", S->level, hs->n_levels);
    if (S->nx < 0 || S->nx > HS_LAT_MAX_HALF || S->ny < 0 || S->ny > HS_LAT_MAX_HALF)
        SH_FAIL(SLAMHIP_ERR_INVALID, "lattice: nx = %d, ny = %d must lie in [0, %d]", S->nx, S->ny, HS_LAT_MAX_HALF);
    if (S->n_theta < 1 || S->n_theta > HS_LAT_MAX_THETA) SH_FAIL(SLAMHIP_ERR_INVALID, "lattice: n_theta = %d must lie in [1, %d]", S->n_theta, HS_LAT_MAX_THETA);
    if (cap_nodes && (int64_t)S->n_theta * (2 * S->nx + 1) * (2 * S->ny + 1) > (int64_t)HS_LAT_MAX_NODES)
        SH_FAIL(SLAMHIP_ERR_INVALID, "lattice: %lld nodes, more than 2^26", (long long)S->n_theta * (2 * S->nx + 1) * (2 * S->ny + 1));
    if (!(isfinite(S->centre[0]) && isfinite(S->centre[1]) && isfinite(S->centre[2]) && isfinite(S->dtheta)))
        SH_FAIL(SLAMHIP_ERR_INVALID, "lattice: centre and dtheta must be finite");
    return SLAMHIP_OK;
}

// The plan of the world class map of one level: R, and lt->pieces -- the window, then every tile's part outside it (the tile
// directory's order), each cut into rows.  Nothing is launched or allocated on the device here.
static int32_t hs_lat_plan_world(slamhip_hs *hs, hs_lattice *lt, int level, wpp_rect *R)
{
    const hs_level &L = hs->lv[level];
    const hs_backing *bk = hs->bk;
    const int T = bk ? bk->T : 0;
    lt->tiles.clear();
    if (bk) bk->for_each_tile(level, [&](int64_t ty, int64_t tx, const unsigned char *) { lt->tiles.push_back(ty); lt->tiles.push_back(tx); });
    const int64_t OX = hs->win_ox >> level, OY = hs->win_oy >> level;
    *R = wpp_bounds(L.w, L.h, OX, OY, T, lt->tiles.data(), lt->tiles.size() / 2);
    if (!wpp_fits(*R))
        SH_FAIL(SLAMHIP_ERR_INVALID, "world lattice: the rectangle of the window and the tiles of level %d is %lld x %lld cells, more than 2^28 "
                "(rows padded to 16 cells)", level, (long long)R->w, (long long)R->h);
    wpp_plan(L.w, L.h, OX, OY, T, lt->tiles.data(), lt->tiles.size() / 2, *R, lt->plan);
    lt->pieces.clear();
    for (const slamhip_world_job &j : lt->plan) {
        const bool win = j.kind == SLAMHIP_WORLD_WINDOW;
        const int sw = win ? L.w : T, sh = win ? L.h : T;
        // (what keeps the launch inside its arrays: a piece of the window or of one tile into a piece of R)
        if ((!win && j.kind != SLAMHIP_WORLD_TILE) || j.nx < 1 || j.ny < 1 || j.sx < 0 || j.sy < 0 || j.sx + j.nx > R->w || j.sy + j.ny > R->h ||
            j.lx < 0 || j.ly < 0 || j.lx + j.nx > sw || j.ly + j.ny > sh)
            SH_FAIL(SLAMHIP_ERR_STATE, "world lattice: the planner produced a job outside its rectangle, window or tile (level %d)", level);
        const slamhip_cell *src = win ? L.d_cells : (const slamhip_cell *)bk->find(level, j.ty, j.tx);
        if (!src) SH_FAIL(SLAMHIP_ERR_STATE, "world lattice: tile (%lld, %lld) of level %d has left the directory", (long long)j.ty, (long long)j.tx, level);
        hs_cut_rows(j.nx, j.ny, [&](int r0, int rows) {
            k7w_piece p;
            p.src = src + ((size_t)(j.ly + r0) * sw + j.lx); p.pitch = sw;
            p.rx = j.sx; p.ry = j.sy + r0; p.nx = (uint16_t)j.nx; p.ny = (uint16_t)rows; p.pad[0] = p.pad[1] = 0;
            lt->pieces.push_back(p);
        });
    }
    if (lt->pieces.size() > (size_t)INT32_MAX) SH_FAIL(SLAMHIP_ERR_INVALID, "world lattice: %zu job pieces", lt->pieces.size());
    return SLAMHIP_OK;
}

// The class map of one level for a launch on the operator's stream, in two steps.  hs_lat_pack_prepare: the hs's lattice state made
// if this is its first use, the world's plan (which refuses before anything is allocated or launched), the map's and the pieces'
// device blocks grown.  hs_lat_pack_enqueue: the pack launch -- k7_pack for the window, the memset and k7_pack_world for the world.
int32_t hs_lat_pack_prepare(slamhip_hs *hs, int level, bool world, hs_class_map *M)
{
    SH_TRY(hs_unit<&slamhip_hs::lat>(hs));
    hs_lattice *lt = hs->lat;
    const hs_level &L = hs->lv[level];
    wpp_rect R = { 0, 0, L.w, L.h };                                       // what the class map covers, in the window's frame
    if (world) SH_TRY(hs_lat_plan_world(hs, lt, level, &R));               // (refuses before anything is allocated or launched)
    M->w = (int)R.w; M->h = (int)R.h; M->wpr = (M->w + 15) / 16;
    M->x0 = (int)R.x0; M->y0 = (int)R.y0;
    SH_TRY(lt->d_cls.grow(sizeof(uint32_t) * (size_t)M->wpr * M->h, "lattice"));
    if (world) SH_TRY(lt->d_pieces.grow(sizeof(k7w_piece) * lt->pieces.size(), "lattice"));
    M->cls = lt->d_cls;
    return SLAMHIP_OK;
}

int32_t hs_lat_pack_enqueue(slamhip_hs *hs, int level, bool world, const hs_class_map *M)
{
    slamhip_ctx *ctx = hs->ctx;
    hs_lattice *lt = hs->lat;
    const hs_level &L = hs->lv[level];
    if (!world) {
        sh_timer t(ctx, SLAMHIP_K_HS_LATTICE_PACK);
        hipLaunchKernelGGL(k7_pack, dim3((unsigned)sh_div_up(M->wpr * L.h, 256)), dim3(256), 0, ctx->stream, (const slamhip_cell *)L.d_cells, L.w, L.h, M->wpr, lt->d_cls);
    } else {
        SH_HIP(hipMemsetAsync(lt->d_cls, 0, sizeof(uint32_t) * (size_t)M->wpr * M->h, ctx->stream));
        SH_HIP(hipMemcpyAsync(lt->d_pieces, lt->pieces.data(), sizeof(k7w_piece) * lt->pieces.size(), hipMemcpyHostToDevice, ctx->stream));
        sh_timer t(ctx, SLAMHIP_K_HS_LATTICE_PACK_WORLD);
        hipLaunchKernelGGL(k7_pack_world, dim3((unsigned)lt->pieces.size()), dim3(K7W_LANES), 0, ctx->stream, (const k7w_piece *)lt->d_pieces.p, M->wpr, lt->d_cls);
    }
    SH_HIP(hipGetLastError());
    return SLAMHIP_OK;
}

// The search into the library's pinned block: *keys (n_theta) and, if asked for, *scores point into it and stay valid until the
// next search of this hs.  world: the class map covers the window and the level's tiles (k7_pack_world) instead of the window.
static int32_t hs_lat_run(slamhip_hs *hs, const slamhip_lattice_spec *S, bool want_scores, bool world, const uint64_t **keys, const int32_t **scores)
{
    SH_TRY(hs_lat_check_spec(hs, S, true));
    if (hs->n_points <= 0) SH_FAIL(SLAMHIP_ERR_STATE, "lattice: no scan (slamhip_hs_set_scan first)");
    slamhip_ctx *ctx = hs->ctx;
    SH_TRY(hs_call_begin(hs));
    hs_class_map M;
    SH_TRY(hs_lat_pack_prepare(hs, S->level, world, &M));
    hs_lattice *lt = hs->lat;
    const hs_level &L = hs->lv[S->level];
    const int NX = 2 * S->nx + 1, NY = 2 * S->ny + 1;
    const size_t key_bytes = sizeof(uint64_t) * (size_t)S->n_theta;
    const size_t out_bytes = key_bytes + (want_scores ? sizeof(int32_t) * (size_t)S->n_theta * NX * NY : 0);
    SH_TRY(lt->d_out.grow(out_bytes, "lattice"));
    SH_TRY(lt->h_out.grow(out_bytes, "lattice"));
    SH_TRY(hs_flush_scan(hs));
    SH_HIP(hipMemsetAsync(lt->d_out, 0, key_bytes, ctx->stream));
    SH_TRY(hs_lat_pack_enqueue(hs, S->level, world, &M));
    k7_arg A;
    A.pts = hs->d_pts; A.n = hs->n_points;
    A.cls = M.cls; A.w = M.w; A.h = M.h; A.wpr = M.wpr;
    A.x0 = M.x0; A.y0 = M.y0;
    A.stm = L.stm;
    A.S = *S;
    A.txl = NX > 32 ? 6 : 4;                                               // 64 x 4 translations per workgroup; a narrow lattice 16 x 16
    const int TX = 1 << A.txl, TY = K7_LANES >> A.txl;
    A.tiles_x = sh_div_up(NX, TX);
    A.keys = (unsigned long long *)lt->d_out.p;
    A.scores = want_scores ? (int32_t *)(lt->d_out + key_bytes) : (int32_t *)nullptr;
    {
        sh_timer t(ctx, SLAMHIP_K_HS_LATTICE);
        hipLaunchKernelGGL(k7_search, dim3((unsigned)(A.tiles_x * sh_div_up(NY, TY)), (unsigned)S->n_theta), dim3(K7_LANES), 0, ctx->stream, A);
    }
    SH_HIP(hipGetLastError());
    SH_HIP(hipMemcpyAsync(lt->h_out, lt->d_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    SH_TRY(hs_call_finish(hs));
    *keys = (const uint64_t *)lt->h_out.p;
    if (scores) *scores = want_scores ? (const int32_t *)(lt->h_out + key_bytes) : (const int32_t *)nullptr;
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_lattice_search(slamhip_hs *hs, const slamhip_lattice_spec *spec, uint64_t *out_keys, int32_t *out_scores)
{
    SH_CHECK_ARG(hs && spec && out_keys);
    const uint64_t *keys = nullptr; const int32_t *scores = nullptr;
    SH_TRY(hs_lat_run(hs, spec, out_scores != nullptr, false, &keys, &scores));
    memcpy(out_keys, keys, sizeof(uint64_t) * (size_t)spec->n_theta);
    if (out_scores) memcpy(out_scores, scores, sizeof(int32_t) * (size_t)spec->n_theta * (2 * spec->nx + 1) * (2 * spec->ny + 1));
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_world_lattice_search(slamhip_hs *hs, const slamhip_lattice_spec *spec, uint64_t *out_keys, int32_t *out_scores)
{
    SH_CHECK_ARG(hs && spec && out_keys);
    const uint64_t *keys = nullptr; const int32_t *scores = nullptr;
    SH_TRY(hs_lat_run(hs, spec, out_scores != nullptr, true, &keys, &scores));
    memcpy(out_keys, keys, sizeof(uint64_t) * (size_t)spec->n_theta);
    if (out_scores) memcpy(out_scores, scores, sizeof(int32_t) * (size_t)spec->n_theta * (2 * spec->nx + 1) * (2 * spec->ny + 1));
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_lattice_node_pose(slamhip_hs *hs, const slamhip_lattice_spec *spec, int32_t k, int32_t flat, float out_pose[3])
{
    SH_CHECK_ARG(out_pose);
    SH_TRY(hs_lat_check_spec(hs, spec, true));
    const int NX = 2 * spec->nx + 1, NY = 2 * spec->ny + 1;
    SH_CHECK_ARG(k >= 0 && k < spec->n_theta && flat >= 0 && flat < NX * NY);
    const hs_level &L = hs->lv[spec->level];
    hs_lat_node_pose(*spec, L.cell, L.stm, k, flat % NX - spec->nx, flat / NX - spec->ny, out_pose);
    return SLAMHIP_OK;
}

// The hints of a relocalisation: the n_theta keys sorted descending (equal keys: the lower k first), the first min(B, n_theta) as
// node poses; node[i] = {k, ix, iy, score} of hint i.  -> how many
static int hs_lat_hints(const slamhip_hs *hs, const slamhip_lattice_spec *spec, const uint64_t *keys, int B, float hints[3 * 64], int node[64][4])
{
    const int nh = B < spec->n_theta ? B : spec->n_theta;
    int order[HS_LAT_MAX_THETA];
    for (int k = 0; k < spec->n_theta; k++) order[k] = k;
    std::stable_sort(order, order + spec->n_theta, [keys](int a, int b) { return keys[a] > keys[b]; });
    const hs_level &L = hs->lv[spec->level];
    const int NX = 2 * spec->nx + 1;
    for (int i = 0; i < nh; i++) {
        const int k = order[i], flat = (int)hs_lat_key_flat(keys[k]);
        node[i][0] = k; node[i][1] = flat % NX - spec->nx; node[i][2] = flat / NX - spec->ny; node[i][3] = hs_lat_key_score(keys[k]);
        hs_lat_node_pose(*spec, L.cell, L.stm, k, node[i][1], node[i][2], hints + 3 * i);
    }
    return nh;
}

// What follows the search in slamhip_hs_relocalise: sort, hints, slamhip_hs_match_best (K24's slamhip_hs_relocalise_bnb runs the same
// text on its own keys)
int32_t hs_lat_reloc_finish(slamhip_hs *hs, const slamhip_lattice_spec *spec, const uint64_t *keys, int32_t B, float out_pose[3],
                            slamhip_match_report *out_report, slamhip_reloc_info *out_info)
{
    float hints[3 * 64];
    int node[64][4];
    const int nh = hs_lat_hints(hs, spec, keys, B, hints, node);
    int32_t best = -1;
    const hs_report_req rq = { out_report, &best };
    SH_TRY(hs_run_match(hs, hints, nh, out_pose, -1, 0, nullptr, &rq));    // slamhip_hs_match_best
    if (best < 0 || best >= nh) SH_FAIL(SLAMHIP_ERR_STATE, "relocalise: the matcher's winner %d is none of the %d hints", best, nh);
    out_info->n_hints = nh; out_info->best_hint = best;
    out_info->k = node[best][0]; out_info->ix = node[best][1]; out_info->iy = node[best][2]; out_info->score = node[best][3];
    out_info->top_score = node[0][3];
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_relocalise(slamhip_hs *hs, const slamhip_lattice_spec *spec, int32_t B, float out_pose[3],
                                         slamhip_match_report *out_report, slamhip_reloc_info *out_info)
{
    SH_CHECK_ARG(hs && spec && out_pose && out_report && out_info && B >= 1 && B <= 64);
    const uint64_t *keys = nullptr;
    SH_TRY(hs_lat_run(hs, spec, false, false, &keys, nullptr));
    return hs_lat_reloc_finish(hs, spec, keys, B, out_pose, out_report, out_info);
}

// what slamhip_hs_relocalise_world refuses before anything is launched or moved, beyond the search's own refusals
int32_t hs_lat_reloc_world_check(const slamhip_hs *hs)
{
    if (!hs->bk) SH_FAIL(SLAMHIP_ERR_STATE, "slamhip_hs_relocalise_world: backing is off (slamhip_hs_set_backing) -- moving the window would destroy the map");
    if (hs->ref_cache)
        SH_FAIL(SLAMHIP_ERR_INVALID, "slamhip_hs_relocalise_world: the reference's cache is on (slamhip_hs_set_reference_cache) -- slamhip_hs_shift "
                "refuses; turn it off first");
    return SLAMHIP_OK;
}

// Relocalise anywhere in the world, behind the world search: the window brought to the best node (slamhip_hs_shift: the backing
// store restores what lies there), the hints re-based into the new frame, and the match_best path over those that lie in the new
// window.  All in binary32, one rounding per operation.
int32_t hs_lat_reloc_world_finish(slamhip_hs *hs, const slamhip_lattice_spec *spec, const uint64_t *keys, int32_t B, float out_pose[3],
                                  slamhip_match_report *out_report, slamhip_world_reloc_info *out_info)
{
    float hints[3 * 64];
    int node[64][4];
    const int nh = hs_lat_hints(hs, spec, keys, B, hints, node);
    // the shift: slamhip_hsproc_set_scroll's rule with trigger 0, applied to the top node
    const hs_level &L0 = hs->lv[0];
    const int g = 1 << (hs->n_levels - 1);
    const float cf[2] = { floorf(hints[0] * L0.stm), floorf(hints[1] * L0.stm) };
    int q[2] = { 0, 0 };
    if (fabsf(cf[0]) < 1.0e9f && fabsf(cf[1]) < 1.0e9f) {                  // (a node nowhere near any map moves nothing)
        const int half[2] = { L0.w / 2, L0.h / 2 };
        for (int a = 0; a < 2; a++) q[a] = (((int)cf[a] - half[a]) / g) * g;   // (C division: toward zero)
    }
    SH_TRY(slamhip_hs_shift(hs, q[0], q[1]));
    out_info->dx = q[0]; out_info->dy = q[1];                              // (from here on the window has moved, whatever follows)
    const float m[2] = { (float)q[0] * L0.cell, (float)q[1] * L0.cell };    // (the product is rounded, then the difference)
    const float lim[2] = { (float)L0.w, (float)L0.h };
    int kept[64], n_kept = 0;
    for (int i = 0; i < nh; i++) {
        float *h = hints + 3 * i;
        h[0] = h[0] - m[0]; h[1] = h[1] - m[1];
        const float fx = h[0] * L0.stm, fy = h[1] * L0.stm;
        if (i > 0 && !(fx >= 0.0f && fx < lim[0] && fy >= 0.0f && fy < lim[1])) continue;    // outside the new window (hint 0 is always kept)
        if (n_kept != i) memcpy(hints + 3 * n_kept, h, sizeof(float) * 3);
        kept[n_kept++] = i;
    }
    int32_t best = -1;
    const hs_report_req rq = { out_report, &best };
    SH_TRY(hs_run_match(hs, hints, n_kept, out_pose, -1, 0, nullptr, &rq));    // slamhip_hs_match_best
    if (best < 0 || best >= n_kept) SH_FAIL(SLAMHIP_ERR_STATE, "relocalise: the matcher's winner %d is none of the %d hints", best, n_kept);
    const int *N = node[kept[best]];
    out_info->n_hints = n_kept; out_info->best_hint = best;
    out_info->k = N[0]; out_info->ix = N[1]; out_info->iy = N[2]; out_info->score = N[3];
    out_info->top_score = node[0][3];
    out_info->n_far = nh - n_kept;
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_relocalise_world(slamhip_hs *hs, const slamhip_lattice_spec *spec, int32_t B, float out_pose[3],
                                               slamhip_match_report *out_report, slamhip_world_reloc_info *out_info)
{
    SH_CHECK_ARG(hs && spec && out_pose && out_report && out_info && B >= 1 && B <= 64);
    SH_TRY(hs_lat_reloc_world_check(hs));
    const uint64_t *keys = nullptr;
    SH_TRY(hs_lat_run(hs, spec, false, true, &keys, nullptr));
    return hs_lat_reloc_world_finish(hs, spec, keys, B, out_pose, out_report, out_info);
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
