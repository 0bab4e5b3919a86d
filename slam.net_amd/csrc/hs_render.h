// hs_render.h -- what K20's kernels (hs_render.hip) and K20's host hook (slamhip_debug_render) share, ONE text for host and device: the
// line OccGridMap.UpdateByScan draws for one scan point, the steps of that line that fall into a rectangle of cells, and the two state
// transitions of a cell.  Definition: include/slamhip.h (slamhip_hs_render).  K5 (hs_update.hip) keeps its own copy of the line-making
// and of the transitions: DESIGN.md section 4 "K20" says why; the GPU tests hold the two to == on every cell.
#pragma once
#include "common.h"
#include "m3x2.h"

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
