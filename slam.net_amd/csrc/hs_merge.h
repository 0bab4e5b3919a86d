// hs_merge.h -- the arithmetic of the map merge (K14, hs_merge.hip) that host and device share: the kernels k14_score and k14_apply
// and the test hooks slamhip_debug_merge / slamhip_debug_merge_box run this text.  Definition: include/slamhip.h,
// slamhip_hs_merge_apply.  Every binary32 operation is rounded on its own (the build uses -ffp-contract=off: no fused
// multiply-add); everything else is integer arithmetic.
#pragma once
#include "common.h"
#include "hs_lattice.h"
#include "m3x2.h"

#define HS_MERGE_MAX_CELLS (1 << 26)       // w * h of a source
#define HS_MERGE_MAX_ORIGIN (1 << 30)      // |ax|, |ay|
#define HS_MERGE_MAX_POSES 4096            // B of a score
#define HS_MERGE_LIMIT 16777216.0f         // |u|, |v| of a sourced cell lie below it (hs_trace_counts' bound)
// the counters of a slamhip_merge_report, as int64_t[12]
#define HS_MERGE_C_UNSOURCED 9
#define HS_MERGE_C_CHANGED 10
#define HS_MERGE_C_CLAMPED 11
#define HS_MERGE_CTRS 12

// step 1: the transform's constants of a pose (tx, ty, theta) on a level with ScaleToMap stm; (c, s): what the beam trace's
// Rotation(theta) holds (sh_m3x2_rotation: IEEERemainder, the four snapped angles, the deterministic sine and cosine)
struct hs_merge_xf { float txc, tyc, c, s; };
__host__ __device__ static inline hs_merge_xf hs_merge_xf_of(float stm, float tx, float ty, float theta)
{
    const sh_m3x2 r = sh_m3x2_rotation(theta);
    hs_merge_xf t;
    t.txc = tx * stm; t.tyc = ty * stm;
    t.c = r.m11; t.s = r.m12;
    return t;
}

// the source array: w x h cells whose first is source-frame cell (ax, ay)
struct hs_merge_src { int ax, ay, w, h; };

// step 2: (u, v) of destination cell (x, y)
__host__ __device__ static inline void hs_merge_uv(const hs_merge_xf &t, int x, int y, float *u, float *v)
{
    const float dxf = (float)x - t.txc, dyf = (float)y - t.tyc;
    const float cx = t.c * dxf, sy = t.s * dyf, cy = t.c * dyf, sx = t.s * dxf;
    *u = cx + sy;
    *v = cy - sx;
}
// step 2: the cell of the source ARRAY that destination cell (x, y) reads; false: the cell is not sourced
__host__ __device__ static inline bool hs_merge_source_cell(const hs_merge_xf &t, const hs_merge_src &S, int x, int y, int *su, int *sv)
{
    float u, v;
    hs_merge_uv(t, x, y, &u, &v);
    if (!(fabsf(u) < HS_MERGE_LIMIT && fabsf(v) < HS_MERGE_LIMIT)) return false;   // (a NaN fails)
    const int iu = (int)rintf(u) - S.ax, iv = (int)rintf(v) - S.ay;        // (|rint| <= 2^24, |ax| <= 2^30: no overflow)
    if (iu < 0 || iu >= S.w || iv < 0 || iv >= S.h) return false;
    *su = iu; *sv = iv;
    return true;
}

// step 4 for a sourced cell: true when the rule gives the cell a value t (which may equal d's bits: the caller writes only where
// they differ).  A sum that is NaN -- an infinity met its opposite; d is not NaN here and sv has a class -- is stored as the quiet
// NaN 0x7FC00000: binary32 leaves that NaN's sign to the platform.
__host__ __device__ static inline bool hs_merge_rule(int rule, float limit, float d, float sv, uint32_t cd, uint32_t cs, float *t, bool *clamped)
{
    *clamped = false;
    if (cs == 0u) return false;
    if (rule == 0) {                                                       // ADD
        if (d != d) return false;                                          // a NaN d stays as it is
        float a = d + sv;
        if (a != a) {
#ifdef __HIP_DEVICE_COMPILE__
            a = __uint_as_float(0x7FC00000u);
#else
            const uint32_t q = 0x7FC00000u; memcpy(&a, &q, sizeof(a));
#endif
        }
        if (a > limit) { a = limit; *clamped = true; }
        if (a < -limit) { a = -limit; *clamped = true; }
        *t = a;
        return true;
    }
    if (rule == 1 && cd != 0u) return false;                               // FILL
    *t = sv;                                                               // FILL into an unknown cell, REPLACE
    return true;
}

__host__ __device__ static inline uint32_t hs_merge_bits(float f)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __float_as_uint(f);
#else
    uint32_t b; memcpy(&b, &f, sizeof(b)); return b;
#endif
}

// The tile box: the rectangle of the source ARRAY that holds the source cell of every sourced cell of the destination tile
// [x0, x1] x [y0, y1], by interval arithmetic on step 2's own operations.  Each of them is monotone in its operand -- (float)x - txc
// in x, c * dxf in dxf (rising or falling with c's sign), a rounded sum in both terms, rintf in its argument -- so the image of an
// interval lies between the images of its ends, rounding included.  An end that is NaN (c or s NaN, or txc, tyc not finite: every
// cell's u or v is then NaN or infinite) or a box that misses the array: nothing of the tile is sourced, false.
struct hs_merge_box { int u0, v0, u1, v1; };                               // inclusive, in cells of the array
__host__ __device__ static inline bool hs_merge_box_of(const hs_merge_xf &t, const hs_merge_src &S, int x0, int y0, int x1, int y1, hs_merge_box *B)
{
    const float dx0 = (float)x0 - t.txc, dx1 = (float)x1 - t.txc, dy0 = (float)y0 - t.tyc, dy1 = (float)y1 - t.tyc;
    const float cxa = t.c * dx0, cxb = t.c * dx1, sya = t.s * dy0, syb = t.s * dy1;
    const float cya = t.c * dy0, cyb = t.c * dy1, sxa = t.s * dx0, sxb = t.s * dx1;
    const float ulo = fminf(cxa, cxb) + fminf(sya, syb), uhi = fmaxf(cxa, cxb) + fmaxf(sya, syb);
    const float vlo = fminf(cya, cyb) - fmaxf(sxa, sxb), vhi = fmaxf(cya, cyb) - fminf(sxa, sxb);
    // (fminf / fmaxf drop a NaN operand, so the products are tested themselves)
    if (cxa != cxa || cxb != cxb || sya != sya || syb != syb || cya != cya || cyb != cyb || sxa != sxa || sxb != sxb) return false;
    if (!(ulo <= uhi && vlo <= vhi)) return false;                         // (a NaN sum: +inf met -inf)
    const float ul = fmaxf(ulo, -HS_MERGE_LIMIT), uh = fminf(uhi, HS_MERGE_LIMIT);
    const float vl = fmaxf(vlo, -HS_MERGE_LIMIT), vh = fminf(vhi, HS_MERGE_LIMIT);
    if (!(ul <= uh && vl <= vh)) return false;
    int u0 = (int)rintf(ul) - S.ax, u1 = (int)rintf(uh) - S.ax, v0 = (int)rintf(vl) - S.ay, v1 = (int)rintf(vh) - S.ay;
    u0 = u0 < 0 ? 0 : u0; v0 = v0 < 0 ? 0 : v0;
    u1 = u1 > S.w - 1 ? S.w - 1 : u1; v1 = v1 > S.h - 1 ? S.h - 1 : v1;
    if (u0 > u1 || v0 > v1) return false;
    B->u0 = u0; B->v0 = v0; B->u1 = u1; B->v1 = v1;
    return true;
}
