// hs_field.h -- what a separable field over E is, for the two units that build one: K9's distance field (hs_dfield.hip) and K16's
// nearest-site field (hs_nearest.hip).  The class map is K7's (hs_lattice.hip), re-packed on every call: M = (x0, y0, w, h) in the
// window's frame, the window or the world's rectangle R.  The field is kept for E, M grown by r cells on every side; outside E it is
// a constant.  E's cell (ex, ey) is cell (ex - r, ey - r) of M.  The pass is two launches:
//  * rows: a workgroup of HS_FIELD_ROW_LANES lanes owns HS_FIELD_SEG consecutive cells of one row of E.  It turns the packed 2-bit
//    words the segment can see -- its cells and r more on both sides -- into a 1-bit site mask in LDS (hs_field_row_bits: at most
//    HS_FIELD_BITW words), then every lane takes four consecutive cells by the unit's own row primitive and stores them at once.
//    Padding cells of a row's last packed word and every cell outside M are class 0 by hs_df_site_word's own test, not by what the
//    padding holds.  Rows of E above and below M are rows of class 0 like any other.
//  * columns: a workgroup of HS_FIELD_COL_LANES lanes owns a tile of HS_FIELD_TX columns x HS_FIELD_TY rows and stages its rows and
//    r more above and below in LDS, HS_FIELD_SROWS at r = 255; what it stages and how it walks is the unit's own.
// Here: the tile constants and caps, the geometry both launches take, the head of a row kernel, the gather of a field call, and
// the host plan -- the unit's blocks, prepare, enqueue, the field call and the skeleton of the CPU-side test hook.  The field as a
// launch reads it (hs_field_of, hs_field_lookup) is hs_dfield.h's.
#pragma once
#include "hs_blocks.h"
#include "hs_dfield.h"
#include <algorithm>
#include <vector>

#define HS_FIELD_ROW_LANES 128
#define HS_FIELD_ROW_CELLS 4               // consecutive cells per lane: one store
#define HS_FIELD_SEG (HS_FIELD_ROW_LANES * HS_FIELD_ROW_CELLS)
#define HS_FIELD_BITW (((HS_FIELD_SEG + 2 * HS_DF_MAX_RADIUS + 31 + 31) >> 5) + 1)   // site words a segment can see: its first word starts up to 31 cells early
#define HS_FIELD_TX 64
#define HS_FIELD_TY 128
#define HS_FIELD_COL_LANES 256
#define HS_FIELD_SROWS (HS_FIELD_TY + 2 * HS_DF_MAX_RADIUS)                // staged rows of a tile at r = 255
#define HS_FIELD_MAX_E ((int64_t)1 << 26)  // cells of E: 1 + 2 bytes each for K9 (192 MB), 2 + 4 for K16 (384 MB)
#define HS_FIELD_MAX_RECT ((int64_t)1 << 24)   // cells of a field call's rectangle: 32 MB of staging for K9, 64 MB for K16
#define HS_FIELD_MAX_POSES 65536
#define HS_FIELD_LOG2_MAX_POINTS 22        // B * n_points with per-point records

// the class map M, and E = M grown by r; the rows' values and the field are rows of `pitch` cells (a multiple of 4)
struct hs_field_geo {
    const uint32_t *cls; int w, h, wpr;
    int r, mask;
    int ew, eh, pitch;
};

template <typename T>
static inline hs_field_geo hs_field_geo_of(const hs_class_map &M, const hs_field_of<T> &E, int site_mask)
{
    hs_field_geo G;
    G.cls = M.cls; G.w = M.w; G.h = M.h; G.wpr = M.wpr;
    G.r = M.x0 - E.e_x0; G.mask = site_mask;
    G.ew = E.ew; G.eh = E.eh; G.pitch = E.pitch;
    return G;
}

// The site words that cells [first, last] of a row of M can see, r cells further on both sides: the mask's first cell bmx0, down
// to a multiple of 32, and the count of words.  Cell mx is bit mx - bmx0 of the mask.
__host__ __device__ static inline void hs_field_bits_span(int first, int last, int r, int *bmx0, int *nw)
{
    *bmx0 = (first - r) & ~31;
    *nw = ((last + r - *bmx0) >> 5) + 1;
}

// The head of a row kernel: the site mask of segment `seg` of row ey of E into bits_s (HS_FIELD_BITW words), and a barrier.
__device__ static __forceinline__ void hs_field_row_bits(const hs_field_geo &A, int ey, int seg, uint32_t *bits_s, int *bmx0, int *nw)
{
    const int my = ey - A.r;
    const uint32_t *row = (my >= 0 && my < A.h) ? A.cls + (size_t)my * A.wpr : (const uint32_t *)nullptr;
    const int mx0 = seg * HS_FIELD_SEG - A.r;                              // the segment's first cell, in M's cells
    hs_field_bits_span(mx0, mx0 + HS_FIELD_SEG - 1, A.r, bmx0, nw);        // (at most HS_FIELD_BITW words)
    for (int j = threadIdx.x; j < *nw; j += HS_FIELD_ROW_LANES) bits_s[j] = hs_df_site_word(row, A.w, *bmx0 + 32 * j, A.mask);
    __syncthreads();
}

// the field call: the asked rectangle out of E, the constant outside, into the block the result leaves through; E is never downloaded
template <typename T>
__global__ void __launch_bounds__(256) hs_field_gather(const hs_field_of<T> E, int x, int y, int w, int n, T *__restrict__ out)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const int ry = j / w, rx = j - ry * w;
    out[j] = (T)hs_field_lookup(E, (long long)x + rx, (long long)y + ry);
}

// ---- host side ---------------------------------------------------------------------------------------------------
// What a unit needs, made by its first call and kept: the rows' values and the field of E, and the blocks of a pose batch, through
// which a field call's rectangle leaves too.
struct hs_field_unit {
    hs_block<void, HS_MEM_DEVICE> d_g;
    hs_block<void, HS_MEM_DEVICE> d_f;
    hs_pose_batch pb;
};

// The plan of one field: the class map prepared (the world's plan refuses before anything is launched), E sized and refused if too
// large, the unit's struct made if this is its first use, the rows' values (g_size bytes a cell) and the field grown.  Nothing is
// launched.
template <auto SLOT, typename T>
static inline int32_t hs_field_prepare(slamhip_hs *hs, const char *who, size_t g_size, int level, bool world, int radius,
                                       uint32_t outside, hs_class_map *M, hs_field_of<T> *E)
{
    SH_TRY(hs_lat_pack_prepare(hs, level, world, M));
    const int64_t ew = (int64_t)M->w + 2 * radius, eh = (int64_t)M->h + 2 * radius;
    if (ew * eh > HS_FIELD_MAX_E)
        SH_FAIL(SLAMHIP_ERR_INVALID, "%s: E, the map of level %d grown by the radius, is %lld x %lld cells, more than 2^26", who, level,
                (long long)ew, (long long)eh);
    SH_TRY(hs_unit<SLOT>(hs));
    hs_field_unit *u = hs->*SLOT;
    E->ew = (int)ew; E->eh = (int)eh; E->pitch = ((int)ew + 3) & ~3;
    E->e_x0 = M->x0 - radius; E->e_y0 = M->y0 - radius;                    // (-2^28 < x0 <= 0: no overflow)
    E->outside = outside;
    const size_t cells = (size_t)E->pitch * (size_t)E->eh;
    SH_TRY(u->d_g.grow(cells * g_size, who));
    SH_TRY(u->d_f.grow(cells * sizeof(T), who));
    E->f = (const T *)u->d_f.p;
    return SLAMHIP_OK;
}

// the class map's pack and the two launches of the planned field, on the operator's stream (no timing class of their own)
template <typename G, typename T>
static inline int32_t hs_field_enqueue(slamhip_hs *hs, hs_field_unit *u, void (*rows)(hs_field_geo, int, G *), void (*cols)(hs_field_geo, int, const G *, T *),
                                       int level, bool world, const hs_class_map *M, const hs_field_of<T> *E, int site_mask)
{
    SH_TRY(hs_lat_pack_enqueue(hs, level, world, M));
    const hs_field_geo A = hs_field_geo_of(*M, *E, site_mask);
    const int segs = sh_div_up(A.pitch, HS_FIELD_SEG), tiles_x = sh_div_up(A.ew, HS_FIELD_TX), tiles_y = sh_div_up(A.eh, HS_FIELD_TY);
    // (at most 2^26 cells in E: neither grid reaches 2^31 workgroups)
    hipLaunchKernelGGL(rows, dim3((unsigned)segs * (unsigned)A.eh), dim3(HS_FIELD_ROW_LANES), 0, hs->ctx->stream, A, segs, (G *)u->d_g.p);
    SH_HIP(hipGetLastError());
    hipLaunchKernelGGL(cols, dim3((unsigned)tiles_x * (unsigned)tiles_y), dim3(HS_FIELD_COL_LANES), 0, hs->ctx->stream, A, tiles_x, (const G *)u->d_g.p, (T *)u->d_f.p);
    SH_HIP(hipGetLastError());
    return SLAMHIP_OK;
}

// The field call, behind the caller's refusals for level, world, site_mask and radius: the rectangle refused, the frame of a
// blocking call around the plan, the field, the gather of the rectangle and its way to `out`.
template <auto SLOT, typename G, typename T>
static inline int32_t hs_field_call(slamhip_hs *hs, const char *who, void (*rows)(hs_field_geo, int, G *),
                                    void (*cols)(hs_field_geo, int, const G *, T *), int level, bool world, int site_mask, int radius, uint32_t outside,
                                    int x, int y, int w, int h, void *out)
{
    if (w < 1 || h < 1 || (int64_t)w * h > HS_FIELD_MAX_RECT)
        SH_FAIL(SLAMHIP_ERR_INVALID, "%s: a rectangle of %d x %d cells; w, h >= 1 and w * h <= 2^24", who, w, h);
    SH_TRY(hs_call_begin(hs));
    hs_class_map M; hs_field_of<T> E;
    SH_TRY(hs_field_prepare<SLOT>(hs, who, sizeof(G), level, world, radius, outside, &M, &E));
    hs_pose_batch *pb = &(hs->*SLOT)->pb;
    const int n = w * h;
    const size_t out_bytes = sizeof(T) * (size_t)n;
    SH_TRY(pb->d_out.grow(out_bytes, who));
    SH_TRY(pb->h_io.grow(out_bytes, who));
    SH_TRY(hs_field_enqueue(hs, hs->*SLOT, rows, cols, level, world, &M, &E, site_mask));
    hipLaunchKernelGGL(hs_field_gather<T>, dim3((unsigned)sh_div_up(n, 256)), dim3(256), 0, hs->ctx->stream, E, x, y, w, n, (T *)pb->d_out.p);
    SH_HIP(hipGetLastError());
    SH_HIP(hipMemcpyAsync(pb->h_io, pb->d_out, out_bytes, hipMemcpyDeviceToHost, hs->ctx->stream));
    SH_TRY(hs_call_finish(hs));
    memcpy(out, pb->h_io, out_bytes);
    return SLAMHIP_OK;
}

// The skeleton of a CPU-side test hook: the field of the definition over a caller's class array, by the text the kernels run.  The
// rectangle is filled with the outside constant and clipped to E; the classes are packed as K7 packs them; then, for the nx columns
// of E the rectangle touches,
//  * row(nx, srows, sy, bits, nw, p0) stages row sy of the srows = ny + 2 r rows the rectangle's ny rows can see: cell i of it is
//    bit p0 + i of the nw site words `bits` (hs_df_site_word), and bits is nullptr for a row outside E, the constant of a class-0 row;
//  * col(nx, sy, i) is the field at column i of staged row sy, from the rows r above and below it.
// What is staged, and as what, is the caller's business.  out: w x h values of T, at any alignment; outside_of(): the constant.
template <typename T, typename Outside, typename Row, typename Col>
static inline int32_t hs_field_debug(const char *who, const uint8_t *cls, int cw, int ch, int site_mask, int r, int x, int y, int w, int h, void *out,
                                     Outside outside_of, Row row, Col col)
{
    if (site_mask < 1 || site_mask > 7) SH_FAIL(SLAMHIP_ERR_INVALID, "%s: site_mask = %d must lie in [1, 7]", who, site_mask);
    if (r < 1 || r > HS_DF_MAX_RADIUS) SH_FAIL(SLAMHIP_ERR_INVALID, "%s: radius = %d must lie in [1, %d]", who, r, HS_DF_MAX_RADIUS);
    if (w < 1 || h < 1 || (int64_t)w * h > HS_FIELD_MAX_RECT)
        SH_FAIL(SLAMHIP_ERR_INVALID, "%s: a rectangle of %d x %d cells; w, h >= 1 and w * h <= 2^24", who, w, h);
    unsigned char *o = (unsigned char *)out;
    const T outside = outside_of();                                        // (behind the refusals: r * r does not overflow)
    for (int64_t j = 0; j < (int64_t)w * h; j++) memcpy(o + sizeof(T) * (size_t)j, &outside, sizeof(T));
    // the part of the rectangle inside E, in the map's cells: [ax0, ax1) x [ay0, ay1)
    const int64_t ax0 = std::max<int64_t>(x, -r), ax1 = std::min<int64_t>((int64_t)x + w, (int64_t)cw + r);
    const int64_t ay0 = std::max<int64_t>(y, -r), ay1 = std::min<int64_t>((int64_t)y + h, (int64_t)ch + r);
    if (ax0 >= ax1 || ay0 >= ay1) return SLAMHIP_OK;
    const int wpr = (cw + 15) / 16;
    std::vector<uint32_t> packed((size_t)wpr * ch, 0u);
    for (int cy = 0; cy < ch; cy++)
        for (int cx = 0; cx < cw; cx++) packed[(size_t)cy * wpr + (cx >> 4)] |= (uint32_t)(cls[(size_t)cy * cw + cx] & 3u) << (2 * (cx & 15));
    const int nx = (int)(ax1 - ax0), ny = (int)(ay1 - ay0);
    int bmx0, nw;
    hs_field_bits_span((int)ax0, (int)ax1 - 1, r, &bmx0, &nw);
    std::vector<uint32_t> bits((size_t)nw);
    for (int sy = 0; sy < ny + 2 * r; sy++) {                              // rows ay0 - r .. ay1 - 1 + r
        const int64_t my = ay0 - r + sy;
        const bool in_e = my >= -r && my < (int64_t)ch + r;
        const uint32_t *mrow = (my >= 0 && my < ch) ? packed.data() + (size_t)my * wpr : (const uint32_t *)nullptr;
        if (in_e)
            for (int j = 0; j < nw; j++) bits[(size_t)j] = hs_df_site_word(mrow, cw, bmx0 + 32 * j, site_mask);
        row(nx, ny + 2 * r, sy, in_e ? bits.data() : (const uint32_t *)nullptr, nw, (int)ax0 - bmx0);
    }
    for (int iy = 0; iy < ny; iy++)
        for (int i = 0; i < nx; i++) {
            const T v = col(nx, iy + r, i);
            memcpy(o + sizeof(T) * ((size_t)(ay0 + iy - y) * (size_t)w + (size_t)(ax0 + i - x)), &v, sizeof(T));
        }
    return SLAMHIP_OK;
}
