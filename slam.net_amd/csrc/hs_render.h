// hs_render.h -- what K20's kernels (hs_render.hip) and K20's host hook (slamhip_debug_render) share, ONE text for host and device: the
// line OccGridMap.UpdateByScan draws for one scan point, the steps of that line that fall into a rectangle of cells, and the two state
// transitions of a cell.  Definition: include/slamhip.h (slamhip_hs_render).  K5 (hs_update.hip) keeps its own copy of the line-making
// and of the transitions: DESIGN.md section 4 "K20" says why; the GPU tests hold the two to == on every cell.
#pragma once
#include "common.h"
#include "m3x2.h"
#include <algorithm>
#include <cmath>

// One line of OccGridMap.UpdateByScan (OccGridMap.cs:130-140, :155-190) on one level: da the major length, sdb the minor length with
// its sign, flags = valid | major_x << 1 | (smaj + 1) << 2 (smaj: the sign of the major step).  Not valid: the end cell is the begin
// cell (:137), or either lies outside the level (:158-161); da = sdb = flags = 0 then.
struct hs_line { int da, sdb, flags; };

// the begin cell of a scan: the scan's origin through the level's matrix, ToRoundPoint (:126-127; banker's, VectorEx.cs:183-186)
__host__ __device__ static inline void hs_line_begin(float ox, float oy, const sh_m3x2 &t, int *bx, int *by)
{
    float bxf, byf;
    sh_v2_transform(ox, oy, t, &bxf, &byf);                                // :126
    *bx = sh_f2i(rintf(bxf)); *by = sh_f2i(rintf(byf));                    // :127
}

// the line to the end point (px, py); *ex, *ey: its end cell, whether the line is valid or not
__host__ __device__ static inline hs_line hs_line_make(float px, float py, const sh_m3x2 &t, int bx, int by, int w, int h, int *ex_out, int *ey_out)
{
    float exf, eyf;
    sh_v2_transform(px, py, t, &exf, &eyf);                                // :133
    const int ex = sh_f2i(rintf(exf)), ey = sh_f2i(rintf(eyf));            // :134
    const bool same = (bx == ex) & (by == ey);                             // :137
    const bool inside = (bx >= 0) & (by >= 0) & (bx < w) & (by < h) & (ex >= 0) & (ey >= 0) & (ex < w) & (ey < h);   // :158-161
    hs_line e; e.da = 0; e.sdb = 0; e.flags = 0;
    if (!same && inside) {
        const int dx = ex - bx, dy = ey - by;
        const int adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy;
        const bool major_x = adx >= ady;                                   // :175
        e.da = major_x ? adx : ady;
        e.sdb = major_x ? dy : dx;                                         // minor extent with its sign (:169-170)
        const int smaj = sh_sign(major_x ? dx : dy);
        e.flags = 1 | (major_x ? 2 : 0) | ((smaj + 1) << 2);
    }
    *ex_out = ex; *ey_out = ey;
    return e;
}

// K25 (hs_render_world.hip): the same line on the unbounded grid of the world.  The inside test against w, h is replaced by the world
// bound -- begin and end cell within +-HS_WORLD_BOUND cells of window cell (0, 0) -- and nothing else changes; rintf is already right
// for negative coordinates.  A cell beyond the bound makes the line not valid HERE, and the callers refuse the whole render for it
// (hs_world_cell_ok on the cells this returns).  A copy, not a parameter of hs_line_make: K20's kernels stay the text they were.
#define HS_WORLD_BOUND (1 << 20)
__host__ __device__ static inline bool hs_world_cell_ok(int x, int y)
{
    return (x >= -HS_WORLD_BOUND) & (x <= HS_WORLD_BOUND) & (y >= -HS_WORLD_BOUND) & (y <= HS_WORLD_BOUND);
}
__host__ __device__ static inline hs_line hs_line_make_world(float px, float py, const sh_m3x2 &t, int bx, int by, int *ex_out, int *ey_out)
{
    float exf, eyf;
    sh_v2_transform(px, py, t, &exf, &eyf);                                // :133
    const int ex = sh_f2i(rintf(exf)), ey = sh_f2i(rintf(eyf));            // :134
    const bool same = (bx == ex) & (by == ey);                             // :137
    const bool inside = hs_world_cell_ok(bx, by) & hs_world_cell_ok(ex, ey);
    hs_line e; e.da = 0; e.sdb = 0; e.flags = 0;
    if (!same && inside) {                                                 // (|dx|, |dy| <= 2^21)
        const int dx = ex - bx, dy = ey - by;
        const int adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy;
        const bool major_x = adx >= ady;                                   // :175
        e.da = major_x ? adx : ady;
        e.sdb = major_x ? dy : dx;
        const int smaj = sh_sign(major_x ? dx : dy);
        e.flags = 1 | (major_x ? 2 : 0) | ((smaj + 1) << 2);
    }
    *ex_out = ex; *ey_out = ey;
    return e;
}
#define HS_LINE_MAX_DA 32767               // what hs_line_clip's 32-bit proof asks of a line; K20's levels give it, K25 refuses a longer line

// Bresenham2D (:220-239) is monotone: step i = 0 .. da of a line lies at major offset i and minor offset (da / 2 + i * db) / da
// (tests/test_closed_forms.py; the end cell, step da, at minor offset db: da / 2 < da).  The steps whose cell lies at major offsets
// [A0, A1] and minor offsets [B0, B1] -- both measured from the begin cell along the line's own directions -- are therefore ONE
// interval [*i0, *i1], empty when *i0 > *i1:
//   minor(i) >= B0  <=>  da / 2 + i * db >= B0 * da        <=>  i >= ceil((B0 * da - da / 2) / db)
//   minor(i) <= B1  <=>  da / 2 + i * db <  (B1 + 1) * da  <=>  i <= floor(((B1 + 1) * da - da / 2 - 1) / db)
// Integers only.  0 <= db <= da <= 32767 (a level is at most 32768 cells a side), and a bound takes part in a product only while
// 0 < B0 <= db or 0 <= B1 < db: every product is at most 32767 * 32767 < 2^30 and every sum below 2^31 -- 32 bits hold them all.
__host__ __device__ static inline void hs_line_clip(int da, int db, int A0, int A1, int B0, int B1, int *i0, int *i1)
{
    int lo = A0 > 0 ? A0 : 0, hi = A1 < da ? A1 : da;
    const int e0 = da / 2;
    if (B1 < 0 || B0 > db) { lo = 1; hi = 0; }                             // (the minor offsets of a line are 0 .. db)
    else {
        if (B0 > 0) { const int k = (B0 * da - e0 + db - 1) / db; lo = k > lo ? k : lo; }       // (db >= B0 > 0; the numerator is positive)
        if (B1 < db) { const int k = ((B1 + 1) * da - e0 - 1) / db; hi = k < hi ? k : hi; }     // (db > B1 >= 0; the numerator is >= 0)
    }
    *i0 = lo; *i1 = hi;
}

// The state transitions of one cell in one scan: BresenhamCellFree (:192-199) by the first line that crosses it, then
// BresenhamCellOcc (:201-218) by the first line that ends in it (first_free, first_occ: the smallest such line indices, 0x7fffffff
// for none); a cell first touched by an end point is not marked free any more (mark_occ is above mark_free).  The tests on the
// update index are the reference's own, literally: they also hold for indices above the marks.
__host__ __device__ static inline void hs_cell_transition(float &v, int &u, int mark_free, int mark_occ, int first_free, int first_occ, float lo_free, float lo_occ)
{
    if (first_free < first_occ && u < mark_free) { v += lo_free; u = mark_free; }     // :192-199
    if (first_occ != 0x7fffffff && u < mark_occ) {                         // :201-218
        if (u == mark_free) v -= lo_free;                                  // :206-209
        if (v < 50.0f) v += lo_occ;                                        // :211-214
        u = mark_occ;                                                      // :216
    }
}

// ---- host side, shared by K20 (hs_render.hip) and K25 (hs_render_world.hip) ----------------------------------------------------------
#define K20_MAX_SCANS (1 << 20)

// the matrix of one pose on one level, formed as hs_update_enqueue forms it (OccGridMap.cs:120-123)
static inline sh_m3x2 k20_matrix(const float pose[3], float stm)
{
    return sh_m3x2_mul(sh_m3x2_mul(sh_m3x2_rotation(pose[2]), sh_m3x2_translation(pose[0], pose[1])), sh_m3x2_scale(stm));
}

// what the renders and their hooks refuse for the range, the poses and the indices; base: the levels' update indices in front of the
// first scan
static inline int32_t k20_check(const char *who, int32_t first, int32_t last, int count, const float *poses, int32_t flags, const int *base, int n_levels)
{
    if (flags & ~SLAMHIP_RENDER_KEEP) SH_FAIL(SLAMHIP_ERR_INVALID, "%s: flags = %d holds bits other than SLAMHIP_RENDER_KEEP", who, flags);
    if (first < 0 || last < first || last > count) SH_FAIL(SLAMHIP_ERR_INVALID, "%s: the range [%d, %d) of %d scans", who, first, last, count);
    if (last > first && !poses) SH_FAIL(SLAMHIP_ERR_INVALID, "%s: no poses", who);
    for (size_t i = 0; i < 3 * (size_t)(last - first); i++)
        if (!std::isfinite(poses[i])) SH_FAIL(SLAMHIP_ERR_INVALID, "%s: component %d of pose %d is not finite", who, (int)(i % 3), (int)(i / 3));
    for (int l = 0; l < n_levels; l++) {
        const long long b = (flags & SLAMHIP_RENDER_KEEP) ? base[l] : 0;
        if (b + 3ll * (last - first) > 0x7fffffffll)
            SH_FAIL(SLAMHIP_ERR_INVALID, "%s: level %d's update index %lld + 3 x %d scans passes INT_MAX", who, l, b, last - first);
    }
    return SLAMHIP_OK;
}

static inline int k20_chunk()      // scans per launch: what bounds the blocks of a render (SLAMHIP_K20_CHUNK: tests put a boundary inside six scans)
{
    static const long long v = std::min(std::max(1ll, sh_env_int("SLAMHIP_K20_CHUNK", 16384)), (long long)K20_MAX_SCANS);
    return (int)v;
}
