// hs_rollout.h -- the arithmetic of the command rollouts (K12, hs_rollout.hip) that host and device share: the kernel k12_rollout
// and the test hook slamhip_debug_rollouts run this text.  Definition: include/slamhip.h, slamhip_hs_rollouts.
// Every binary32 operation is rounded on its own (the build uses -ffp-contract=off: no fused multiply-add); the cells are
// hs_trace.h's end-point rule (rintf: to nearest, ties to even; |f| < 2^24), the field is hs_nav.h's.
#pragma once
#include "det_trig.h"
#include "hs_nav.h"

#define HS_RO_MAX_B 65536                  // rollouts per call
#define HS_RO_MAX_CMD 256                  // n_cmd, and hold
#define HS_RO_MAX_T 1024                   // n_cmd * hold: the bound of the device loop
#define HS_RO_MAX_PAIRS ((int64_t)1 << 22) // B * n_cmd: 32 MB of staging
#define HS_RO_MAX_POINTS 32                // body points: with the centre, at most a wavefront's lanes per rollout

struct hs_ro_pose { float x, y, th; };
// the field as the rollouts read it: the traversable words and costs of M, M's first cell in the window's frame
struct hs_ro_field { const uint32_t *tw; const uint32_t *cost; int twpr, w, h, x0, y0; float stm; };
// slamhip_rollout_result, field by field
struct hs_ro_result { int32_t n_free, min_step; uint32_t end_cost, min_cost; float x, y, theta; };

// step 2: pose i + 1 from pose i, (s, c) = sh_det_sincosf(theta_i)
__host__ __device__ static inline hs_ro_pose hs_ro_step(const hs_ro_pose &p, float s, float c, float v, float w, float dt)
{
    const float d = v * dt;
    const float dx = d * c, dy = d * s, dth = w * dt;
    hs_ro_pose q;
    q.x = p.x + dx; q.y = p.y + dy; q.th = p.th + dth;
    return q;
}

// step 3: the cell of one metric coordinate, in the window's frame; false: the coordinate has no cell (a NaN fails)
__host__ __device__ static inline bool hs_ro_cell(float m, float stm, int *cell)
{
    const float f = m * stm;
    if (!(fabsf(f) < 16777216.0f)) return false;
    *cell = (int)rintf(f);
    return true;
}

// step 3: body point (bx, by) of the robot's frame at pose p
__host__ __device__ static inline void hs_ro_body(const hs_ro_pose &p, float s, float c, float bx, float by, float *wx, float *wy)
{
    const float cx = c * bx, sy = s * by, sx = s * bx, cy = c * by;
    *wx = (cx - sy) + p.x;
    *wy = (sx + cy) + p.y;
}

// the cell of (mx, my) [metres] in M's own cells -- which may lie outside M; false: a coordinate has no cell
__host__ __device__ static inline bool hs_ro_cell_of(const hs_ro_field &F, float mx, float my, long long *x, long long *y)
{
    int cx, cy;
    if (!hs_ro_cell(mx, F.stm, &cx) || !hs_ro_cell(my, F.stm, &cy)) return false;
    *x = (long long)cx - F.x0; *y = (long long)cy - F.y0;
    return true;
}

// the traversable bit of cell (x, y) of M's frame.  Cells outside M never are traversable.
__host__ __device__ static inline bool hs_ro_trav_at(const hs_ro_field &F, long long x, long long y)
{
    if (x < 0 || x >= F.w || y < 0 || y >= F.h) return false;
    return hs_nav_bit(F.tw + (size_t)y * F.twpr, F.twpr, (int)x) != 0u;
}

// is the cell of (mx, my) [metres] traversable?
__host__ __device__ static inline bool hs_ro_traversable(const hs_ro_field &F, float mx, float my)
{
    long long x, y;
    return hs_ro_cell_of(F, mx, my, &x, &y) && hs_ro_trav_at(F, x, y);
}

// C at the cell of (mx, my), HS_NAV_UNREACHED where there is no cell or it lies outside M
__host__ __device__ static inline uint32_t hs_ro_cost(const hs_ro_field &F, float mx, float my)
{
    long long x, y;
    if (!hs_ro_cell_of(F, mx, my, &x, &y)) return HS_NAV_UNREACHED;
    if (x < 0 || x >= F.w || y < 0 || y >= F.h) return HS_NAV_UNREACHED;
    return F.cost[(size_t)y * F.w + (size_t)x];
}

// step 5: the record before any pose, and after free pose i whose centre costs `cost` (!= HS_NAV_UNREACHED)
__host__ __device__ static inline hs_ro_result hs_ro_begin(const hs_ro_pose &p0)
{
    hs_ro_result r;
    r.n_free = 0; r.min_step = -1; r.end_cost = HS_NAV_UNREACHED; r.min_cost = HS_NAV_UNREACHED;
    r.x = p0.x; r.y = p0.y; r.theta = p0.th;
    return r;
}
__host__ __device__ static inline void hs_ro_accept(hs_ro_result &r, int i, uint32_t cost, const hs_ro_pose &p)
{
    r.n_free = i + 1;
    if (cost < r.min_cost) { r.min_cost = cost; r.min_step = i; }         // (strictly: the first of equal costs stays)
    r.end_cost = cost;
    r.x = p.x; r.y = p.y; r.theta = p.th;
}

// step 6: a rollout's key in the call's summary
__host__ __device__ static inline unsigned long long hs_ro_key(uint32_t cost, int b) { return ((unsigned long long)cost << 32) | (unsigned long long)(uint32_t)b; }
