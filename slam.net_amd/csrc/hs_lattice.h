// hs_lattice.h -- the arithmetic of the pose-lattice search (K7, hs_lattice.hip) that host and device share: the kernel, the host
// helpers (slamhip_hs_lattice_node_pose, slamhip_hs_relocalise) and the test hook slamhip_debug_lattice_cells run this text.
// Definition: include/slamhip.h, slamhip_lattice_spec.  Every binary32 operation is rounded on its own: the build's
// -ffp-contract=off keeps multiply and add separate on both sides, as for the matcher and K1.
#pragma once
#include "common.h"
#include "det_trig.h"

#define HS_LAT_MAX_HALF 4096               // nx, ny
#define HS_LAT_MAX_THETA 4096
#define HS_LAT_MAX_NODES (1 << 26)
#define HS_LAT_IGNORED INT32_MIN           // what slamhip_debug_lattice_cells reports for an ignored point
#define K7_RECT_WORDS 12288                // words of the class map a workgroup stages in LDS (48 KB): k7_search, and K8's k8_trace

// one heading of the lattice on one level: the rotation and the centre in map coordinates
struct hs_lat_heading { float s, c, stm, cxm, cym; };

__host__ __device__ static inline float hs_lat_theta(const slamhip_lattice_spec &S, int k) { return S.centre[2] + (float)k * S.dtheta; }

__host__ __device__ static inline hs_lat_heading hs_lat_heading_of(float stm, float cx, float cy, float theta)
{
    hs_lat_heading H;
    sh_det_sincosf(theta, &H.s, &H.c);
    H.stm = stm;
    H.cxm = cx * stm; H.cym = cy * stm;
    return H;
}

// the cell of scan point (px, py) under heading H; false: the point is ignored for this heading (NaN, or |f| >= 2^24)
__host__ __device__ static inline bool hs_lat_point_cell(const hs_lat_heading &H, float px, float py, int *gx, int *gy)
{
    const float rx = H.c * px - H.s * py, ry = H.s * px + H.c * py;
    const float fx = rx * H.stm + H.cxm, fy = ry * H.stm + H.cym;
    if (!(fabsf(fx) < 16777216.0f && fabsf(fy) < 16777216.0f)) return false;
    *gx = (int)floorf(fx); *gy = (int)floorf(fy);
    return true;
}

// the class of a cell value in the packed map's two bits: 1 occupied (+1), 2 free (-1), 0 neither (+0, -0, NaN)
__host__ __device__ static inline uint32_t hs_lat_class_bits(float v) { return v > 0.0f ? 1u : v < 0.0f ? 2u : 0u; }
__host__ __device__ static inline int hs_lat_class_value(uint32_t bits) { return (int)(bits & 1u) - (int)(bits >> 1); }

__host__ __device__ static inline unsigned long long hs_lat_key(int score, uint32_t flat)
{
    return ((unsigned long long)((uint32_t)score ^ 0x80000000u) << 32) | (unsigned long long)(0xFFFFFFFFu - flat);
}
static inline int hs_lat_key_score(unsigned long long key) { return (int)((uint32_t)(key >> 32) ^ 0x80000000u); }
static inline uint32_t hs_lat_key_flat(unsigned long long key) { return 0xFFFFFFFFu - (uint32_t)key; }

// the node pose in the window's frame
static inline void hs_lat_node_pose(const slamhip_lattice_spec &S, float cell, float stm, int k, int ix, int iy, float out[3])
{
    const float cxm = S.centre[0] * stm, cym = S.centre[1] * stm;
    out[0] = (cxm + (float)ix) * cell;
    out[1] = (cym + (float)iy) * cell;
    out[2] = hs_lat_theta(S, k);
}
