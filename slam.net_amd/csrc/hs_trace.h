// hs_trace.h -- the arithmetic of the beam trace (K8, hs_trace.hip) that host and device share: the kernel and the test hooks
// slamhip_debug_trace_lines / slamhip_debug_trace_cells run this text.  Definition: include/slamhip.h, slamhip_trace_beam.
// Every binary32 operation is rounded on its own: the build's -ffp-contract=off keeps multiply and add separate on both sides.
#pragma once
#include "common.h"
#include "m3x2.h"

// one beam on one level: begin and end cell in window-frame cells, and da -- -1 ignored (the cells are then 0), 0 same, else the
// major length
struct hs_trace_line { int32_t bx, by, ex, ey, da; };

// the transform K5 runs for a pose in the window's frame (OccGridMap.cs:120-123)
__host__ __device__ static inline sh_m3x2 hs_trace_transform(float stm, float x, float y, float theta)
{
    return sh_m3x2_mul(sh_m3x2_mul(sh_m3x2_rotation(theta), sh_m3x2_translation(x, y)), sh_m3x2_scale(stm));
}

__host__ __device__ static inline bool hs_trace_counts(float f) { return fabsf(f) < 16777216.0f; }    // (a NaN fails)

// The end cell of scan point (px, py) under t, for the units that look a field up there (k9_score, k16_pairs, hs_mcl_point); false:
// the point is ignored, as hs_trace_line_of ignores its beam, and the cell is not written.
__host__ __device__ static inline bool hs_trace_end_cell(const sh_m3x2 &t, float px, float py, int *ex, int *ey)
{
    float exf, eyf;
    sh_v2_transform(px, py, t, &exf, &eyf);
    if (!(hs_trace_counts(exf) && hs_trace_counts(eyf))) return false;
    *ex = sh_f2i(rintf(exf)); *ey = sh_f2i(rintf(eyf));                    // ToRoundPoint (banker's)
    return true;
}

// the beam from scan origin (ox, oy) to scan point (px, py) under t
__host__ __device__ static inline hs_trace_line hs_trace_line_of(const sh_m3x2 &t, float ox, float oy, float px, float py)
{
    hs_trace_line l = { 0, 0, 0, 0, -1 };
    float bxf, byf, exf, eyf;
    sh_v2_transform(ox, oy, t, &bxf, &byf);                                // :126
    sh_v2_transform(px, py, t, &exf, &eyf);                                // :133
    if (!(hs_trace_counts(bxf) && hs_trace_counts(byf) && hs_trace_counts(exf) && hs_trace_counts(eyf))) return l;
    const int bx = sh_f2i(rintf(bxf)), by = sh_f2i(rintf(byf));            // :127 ToRoundPoint (banker's)
    const int ex = sh_f2i(rintf(exf)), ey = sh_f2i(rintf(eyf));            // :134
    const int adx = ex < bx ? bx - ex : ex - bx, ady = ey < by ? by - ey : ey - by;    // (|cells| <= 2^24: no overflow)
    const int da = adx >= ady ? adx : ady;
    if (da > SLAMHIP_TRACE_MAX_DA) return l;
    l.bx = bx; l.by = by; l.ex = ex; l.ey = ey; l.da = da;                 // (da == 0: b == e, :137)
    return l;
}

// The walk of a line with da >= 1, one cell per call: Bresenham2D's own recurrence (:226-238), whose cell at step a is the one of
// the closed form -- major offset a, minor offset (da / 2 + a * db) / da (tests/test_closed_forms.py) -- and the end cell at
// a == da (:187).  (x, y) is the cell of step `a`; hs_trace_walk_next moves to step a + 1 <= da.
struct hs_trace_walk { int32_t x, y, a, da, db, err, sax, say, sbx, sby, ex, ey; };

__host__ __device__ static inline hs_trace_walk hs_trace_walk_begin(const hs_trace_line &l)
{
    hs_trace_walk w;
    const int dx = l.ex - l.bx, dy = l.ey - l.by;
    const int adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy;
    const bool major_x = adx >= ady;                                       // :175
    w.x = l.bx; w.y = l.by; w.a = 0;
    w.da = major_x ? adx : ady; w.db = major_x ? ady : adx;
    w.err = w.da / 2;                                                      // :177, :183
    w.sax = major_x ? sh_sign(dx) : 0; w.say = major_x ? 0 : sh_sign(dy);  // the major step
    w.sbx = major_x ? 0 : sh_sign(dx); w.sby = major_x ? sh_sign(dy) : 0;  // the minor step
    w.ex = l.ex; w.ey = l.ey;
    return w;
}

__host__ __device__ static inline void hs_trace_walk_next(hs_trace_walk &w)
{
    w.a++;
    if (w.a >= w.da) { w.x = w.ex; w.y = w.ey; return; }                   // the end cell (:187)
    w.x += w.sax; w.y += w.say;                                            // :228
    w.err += w.db;                                                         // :229 (err < da, db <= da <= 32768)
    if (w.err >= w.da) { w.x += w.sbx; w.y += w.sby; w.err -= w.da; }      // :231-235
}
