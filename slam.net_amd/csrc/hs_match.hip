// hs_match.hip -- K4, the Gauss-Newton scan matcher of HectorSLAM, and its entry points (slamhip_hs_match*, slamhip_hs_hessian).
//
// K4 replaces ScanMatcher.MatchData / EstimateTransformationLogLh / GetCompleteHessianDerivs /
// InterpMapValueWithDerivatives (HectorSLAM/Matcher/ScanMatcher.cs:41-249): all pyramid levels and all
// iterations of one match run in ONE persistent workgroup (the reference fans out to ParallelWorker
// threads once per iteration, :154); the nine sums are accumulated per lane in fp32, reduced across the
// workgroup in fp64 and the 3x3 system is solved on the device with the BCL's cofactor formulas.  A single match is 512
// lanes with the scan's points in LDS, one barrier and one sine / cosine per iteration (hs_hessian_block: round 5).
// Occupancy probabilities exp(v)/(exp(v)+1) (OccGridMap.GetCachedProbability, OccGridMap.cs:97-107) are READ from a dense
// per-level grid `prob` that every writer of the log-odds grid keeps current (K5 for the cells it touches, upload and
// reset for all of them) -- by default the device's form of the reference's per-cell cache, without its epochs: the value
// always is the current cell's probability, also across Reset, where the reference's cache can serve pre-reset values
// (deviation D5: DESIGN.md sec.3 and include/slamhip.h, slamhip_hs_probability).  Opt-in (slamhip_hs_set_reference_cache):
// the reference's cache itself, CachedMapElement {Value, Index} per cell and a per-level epoch (hs_cache_taps), so that
// the matcher and slamhip_hs_probability serve what the reference serves, stale entries included.
// Float parity target: pose within 1e-4 m / 1e-4 rad (H6).
#include "hs_internal.h"

// ---- K4 device code ------------------------------------------------------------------------------------------

__device__ static inline float hs_prob_tap(float v)
{
#if HS_PROB_MODE == 2
    const float odds = __expf(v);
    return __fdividef(odds, odds + 1.0f);
#else
    return hs_prob_v(v);
#endif
}

// one DPP step of a binary64 value (the wave partials' tree in hs_hessian_block; no LDS permutes: a ds_bpermute costs ~100
// cycles of latency).  Lanes a step's row mask excludes receive zero (update_dpp's `old`).
template <int CTRL, int ROWS> __device__ static inline double hs_dpp_f64(double v)
{
    const int lo = __double2loint(v), hi = __double2hiint(v);
    return __hiloint2double(__builtin_amdgcn_update_dpp(0, hi, CTRL, ROWS, 0xf, false),
                            __builtin_amdgcn_update_dpp(0, lo, CTRL, ROWS, 0xf, false));
}

// one DPP step in binary32: the wave trees of the nine sums (butterfly inside each row of 16 lanes, then row_bcast:15 into rows
// 1 and 3 and row_bcast:31 into rows 2 and 3 -- the total is valid in lane 63).  (Nine binary64 wave sums per iteration -- two DPP
// moves and a double add per step, in dependent chains -- were half of the first matcher's run time; the reference itself sums
// these terms in binary32, sequentially per thread chunk, ScanMatcher.cs:166-180, so a binary32 tree over 64 lanes is at least
// as accurate as what it is compared with.  The wave partials are still added in binary64.)
template <int CTRL, int ROWS> __device__ static inline float hs_dpp_f32(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROWS, 0xf, false));
}

#ifdef K4_TIMES
// developer instrumentation (build with SLAMHIP_K4_TIMES=1): wall-clock ticks (100 MHz) per phase of an iteration,
// accumulated by thread 0 of workgroup 0
__device__ unsigned long long g_k4_times[16];
#define K4_STAMP(k) { if (threadIdx.x == 0 && blockIdx.x == 0) { const unsigned long long t_ = wall_clock64(); g_k4_times[k] += t_ - k4_last; k4_last = t_; } }
__device__ unsigned long long g_k4_last;
__device__ unsigned long long g_k4_pts[16];      // the points' phase per iteration of a match (coarse level first)
__device__ int g_k4_iter;
#define K4_STAMP_BEGIN unsigned long long k4_last = wall_clock64(); if (threadIdx.x == 0 && blockIdx.x == 0) { if (g_k4_last) g_k4_times[5] += k4_last - g_k4_last; }
#else
#define K4_STAMP(k) {}
#define K4_STAMP_BEGIN
#endif

// GetCompleteHessianDerivs (:135-204) for the whole workgroup; result (9 sums) in sums[], uniform in every wavefront.
// order: dTr.x, dTr.y, dTr.z, H11, H22, H33, H12, H13, H23
//
// Round 5: a single match is nine dependent iterations on ONE compute unit, and with 16 wavefronts (four per SIMD) it was
// bound by VALU issue, not by latency (profiles/r05_secondary_kernels.json: 475 VALU instructions per wavefront and iteration,
// 0.22 of a wavefront's cycles issuing VALU x 4 wavefronts per SIMD): every wavefront repeats the uniform part of an
// iteration -- Matrix3x2.CreateRotation's IEEERemainder, two binary64 sin/cos evaluations, the 3 x 3 inverse -- and three
// barriers.  Now
//  * FEW wavefronts with several points per lane (the single match runs 256 lanes x 5 points: one wavefront per SIMD, the
//    uniform part once per SIMD), the points of the scan in LDS, the taps of a lane's points requested together by a
//    branch-free interpolation (outside the grid: taps of cell 0, result selected to zero -- ScanMatcher.cs:216-219);
//  * ONE barrier per iteration: the wave partials go to one of two alternating LDS blocks, and after the barrier every
//    wavefront adds the partials itself -- lane k * NW + w loads partial w of sum k, a DPP row tree in binary64 (the same tree
//    and order as before), nine v_readlane;
//  * the rotation's sin/cos is the one the derivative needs (:145-146) whenever |angle| < pi (IEEERemainder returns its
//    argument there, exactly), so it is evaluated once.
// (Round 4, measured and rejected: a 4 x 4 window of probabilities per point kept in registers across a level's iterations, so
// that iterations 2 .. n read no memory -- 34.0 -> 37.1 us per match: the first iteration's 64 bytes per point in four unaligned
// 16-byte loads cost more than the later iterations' taps, which hit the L2 anyway.)

// Matrix3x2.CreateRotation (m3x2.h) given sin/cos of the SAME angle: valid for |radians| < pi, where IEEERemainder(radians,
// 2 pi) == radians
__device__ static inline sh_m3x2 hs_rotation_sc(float radians, float s_in, float c_in)
{
    const float pi = 3.14159274f;
    if (!(fabsf(radians) < pi)) return sh_m3x2_rotation(radians);
    const float epsilon = 0.001f * pi / 180.0f;
    float c = c_in, s = s_in;
    if (radians > -epsilon && radians < epsilon) { c = 1; s = 0; }
    else if (radians > pi / 2 - epsilon && radians < pi / 2 + epsilon) { c = 0; s = 1; }
    else if (radians < -pi + epsilon || radians > pi - epsilon) { c = -1; s = 0; }
    else if (radians > -pi / 2 - epsilon && radians < -pi / 2 + epsilon) { c = 0; s = -1; }
    sh_m3x2 r = { c, s, -s, c, 0.0f, 0.0f };
    return r;
}

template <int BDIM> struct hs_shape {
    static constexpr int NW = BDIM >> 6;                                   // wavefronts
    static constexpr int PU = BDIM >= 1024 ? 2 : BDIM >= 512 ? 3 : 5;      // points per lane and pass (1080 rays: one pass)
    static constexpr int RED = 9 * NW;                                     // doubles per reduction block
    static constexpr int RED_REP = 11 * NW;                                // ... of the match report's pass (hs_hessian_block<REP>)
};

// the per-iteration transform of GetCompleteHessianDerivs (:139-146), the same in every lane
struct hs_iter_xf { sh_m3x2 t; float sinRot, cosRot, limx, limy; };
__device__ static __forceinline__ hs_iter_xf hs_iter_transform(const hs_level_dev &L, const float pose[3])
{
    hs_iter_xf X;
    float s, c;
    sh_det_sincosf(pose[2], &s, &c);
    X.t = sh_m3x2_mul(sh_m3x2_mul(hs_rotation_sc(pose[2], s, c),
                                  sh_m3x2_translation(pose[0] * L.cell, pose[1] * L.cell)),
                      sh_m3x2_scale(L.stm));                               // :139-142
    X.sinRot = s * L.stm; X.cosRot = c * L.stm;                            // :145-146
    X.limx = (float)L.w - 2.0f; X.limy = (float)L.h - 2.0f;               // MapProperties.cs:42
    return X;
}

// ---- the reference's probability cache (slamhip_hs_set_reference_cache, opt-in) ------------------------------------------------
// OccGridMap.GetCachedProbability (:97-107) literally: cacheArray[i] = CachedMapElement {Value, Index} (OccGridMap.cs:16), epoch
// currCacheIndex.  A tap loads the entry; Index == epoch: Value (:106); else the current value's probability -- prob[i], which
// every writer of the cells keeps current -- is stored as {prob[i], epoch} (:101-103) and used.  Race-free without ordering:
// an entry a lane can observe is either its state before the launch or a fill {current probability, epoch}, and both give
// the reference's answer; a stale entry (Index == epoch before the launch) is never written.  So the order of fills inside
// an epoch does not matter, across workgroups, XCDs and batch entries alike.  What would break it is a read that joins one
// fill's Value to another's Index: the entry is ONE 8-byte word, loaded and stored whole (relaxed, global_load/store_dwordx2).
// (Workgroup scope: no lane needs another workgroup's fill to be visible -- an unseen fill only means the lane fills
// again, with the same value -- and the plain loads keep the taps in the L2.)
struct hs_cache_lv { unsigned long long *c; int epoch; };                 // one level's cacheArray and currCacheIndex
// the four taps of an in-range point at cell idx (:230-233) through the cache.  A point outside the map, a NaN point or a
// padding lane (ok false) reads and fills nothing: the reference returns before its first tap (:216-219).
// FILL false (the match report's taps, an evaluation the reference does not make): the cache is observed, never filled --
// an entry of this epoch is served, anything else is computed from the cell's current value and not recorded.
template <bool FILL = true>
__device__ static __forceinline__ void hs_cache_taps(const hs_cache_lv &C, const float *prob, int idx, int w, bool ok, float2 &r0, float2 &r1)
{
    float v[4] = { 0.f, 0.f, 0.f, 0.f };
    if (ok) {
        const int at[4] = { idx, idx + 1, idx + w, idx + w + 1 };
        unsigned long long e[4];
#pragma unroll
        for (int k = 0; k < 4; k++) e[k] = __hip_atomic_load(C.c + at[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        bool miss[4];
#pragma unroll
        for (int k = 0; k < 4; k++) { miss[k] = !hs_cache_entry_hit(e[k], C.epoch); v[k] = hs_cache_entry_value(e[k]); }
#pragma unroll
        for (int k = 0; k < 4; k++) if (miss[k]) v[k] = prob[at[k]];      // :101-102
        if constexpr (FILL) {
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (miss[k]) __hip_atomic_store(C.c + at[k], hs_cache_entry(v[k], C.epoch), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);   // :103
        }
    }
    r0 = make_float2(v[0], v[1]); r1 = make_float2(v[2], v[3]);
}

// one scan point i (i >= n: a padding lane, its terms are zero): the point and its four taps, requested without waiting.
// RC: the taps through the reference's cache (hs_cache_taps), FILL as there
struct hs_point { float2 p, r0, r1; float fx, fy; bool ok; };
template <bool RC, bool FILL = true>
__device__ static __forceinline__ void hs_point_taps(const hs_level_dev &L, const hs_cache_lv &C, const float2 *pts, int i, int n, const hs_iter_xf &X, hs_point &q)
{
    q.p = i < n ? pts[i] : make_float2(0.f, 0.f);
    float cx, cy;
    sh_v2_transform(q.p.x, q.p.y, X.t, &cx, &cy);                          // :161
    // InterpMapValueWithDerivatives (:211-249), MapProperties.cs:83-87
    q.ok = i < n && !(!(cx == cx) || !(cy == cy) || cx < 0.0f || cx > X.limx || cy < 0.0f || cy > X.limy);
    const float fxx = floorf(cx), fyy = floorf(cy);                        // :222
    const int ix = q.ok ? (int)fxx : 0, iy = q.ok ? (int)fyy : 0;
    q.fx = cx - fxx; q.fy = cy - fyy;                                      // :225
    const int idx = iy * L.w + ix;                                         // :227
#if HS_PROB_MODE == 0
    if constexpr (RC) hs_cache_taps<FILL>(C, L.prob, idx, L.w, q.ok, q.r0, q.r1);
    else {
        __builtin_memcpy(&q.r0, L.prob + idx, sizeof(float2));             // (two adjacent taps: one 8-byte load)
        __builtin_memcpy(&q.r1, L.prob + idx + L.w, sizeof(float2));
    }
#else
    int4 c0, c1;                                                           // (two adjacent cells {UpdateIndex, Value}: one 16-byte load)
    __builtin_memcpy(&c0, L.cells + idx, sizeof(int4));
    __builtin_memcpy(&c1, L.cells + idx + L.w, sizeof(int4));
    q.r0 = make_float2(hs_prob_tap(__int_as_float(c0.y)), hs_prob_tap(__int_as_float(c0.w)));
    q.r1 = make_float2(hs_prob_tap(__int_as_float(c1.y)), hs_prob_tap(__int_as_float(c1.w)));
#endif
}

// the point's nine terms (:162-180) in the order of sums[]: the interpolation and the products, each a binary32 rounding
// NT == 10 (the match report): tm[9] = funVal * funVal, the point's share of the residual
template <int NT = 9>
__device__ static __forceinline__ void hs_point_terms(const hs_point &q, const hs_iter_xf &X, float tm[NT])
{
    const float i0 = q.r0.x, i1 = q.r0.y, i2 = q.r1.x, i3 = q.r1.y;        // :230-233
    const float dx1 = i0 - i1, dx2 = i2 - i3, dy1 = i0 - i2, dy2 = i1 - i3;    // :235-239
    const float xi = 1.0f - q.fx, yi = 1.0f - q.fy;                        // :241-242
    float P = ((i0 * xi + i1 * q.fx) * yi) + ((i2 * xi + i3 * q.fx) * q.fy);   // :245-246
    float gx = -((dx1 * xi) + (dx2 * q.fx));                               // :247
    float gy = -((dy1 * yi) + (dy2 * q.fy));                               // :248
    if (!q.ok) { P = 0.0f; gx = 0.0f; gy = 0.0f; }                         // :216-219
    const float fun = 1.0f - P;                                            // :164
    const float rot = ((-X.sinRot * q.p.x - X.cosRot * q.p.y) * gx + (X.cosRot * q.p.x - X.sinRot * q.p.y) * gy);   // :169-170
    tm[0] = gx * fun;  tm[1] = gy * fun;  tm[2] = rot * fun;               // :166,:167,:172
    tm[3] = gx * gx;   tm[4] = gy * gy;   tm[5] = rot * rot;               // :174-176
    tm[6] = gx * gy;   tm[7] = gx * rot;  tm[8] = gy * rot;                // :178-180
    if constexpr (NT == 10) tm[9] = fun * fun;
}

// RC: the taps through the reference's cache (hs_cache_taps)
// REP (the match report, slamhip_match_report): two more accumulators through the same reduction -- the residual, the sum of
// funVal * funVal over ALL points (a point outside the map has M = 0 and adds exactly 1), as sum 9 in binary32 like the others,
// and the number of points inside the map as an integer, exact -- and with RC taps that fill nothing.  `red` then holds
// hs_shape::RED_REP doubles.
template <int BDIM, bool LDSP, bool RC, bool REP = false>
__device__ static __forceinline__ void hs_hessian_block(const hs_level_dev &L, const hs_cache_lv &C, const float2 *pts, int n, const float pose[3],
                                                        double *red /* [hs_shape::RED]: this iteration's block */, float sums[9],
                                                        float *residual = nullptr, int *n_in_map = nullptr)
{
    constexpr int NW = hs_shape<BDIM>::NW, PU = hs_shape<BDIM>::PU;
    constexpr int NS = REP ? 10 : 9;                                       // binary32 sums
    K4_STAMP_BEGIN
    float s, c;
    sh_det_sincosf(pose[2], &s, &c);
    const sh_m3x2 t = sh_m3x2_mul(sh_m3x2_mul(hs_rotation_sc(pose[2], s, c),
                                              sh_m3x2_translation(pose[0] * L.cell, pose[1] * L.cell)),
                                  sh_m3x2_scale(L.stm));                   // :139-142
    const float sinRot = s * L.stm, cosRot = c * L.stm;                    // :145-146
    const float limx = (float)L.w - 2.0f, limy = (float)L.h - 2.0f;       // MapProperties.cs:42
    K4_STAMP(0)                                                            // transform + trigonometry
    float acc[NS] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
    int cnt = 0;
    for (int base = 0; base < n; base += BDIM * PU) {
        float2 p[PU], r0[PU], r1[PU];
        float fx[PU], fy[PU];
        bool ok[PU];
#pragma unroll
        for (int u = 0; u < PU; u++) {
            const int i = base + (int)threadIdx.x + u * BDIM;
            p[u] = i < n ? pts[i] : make_float2(0.f, 0.f);
            float cx, cy;
            sh_v2_transform(p[u].x, p[u].y, t, &cx, &cy);                  // :161
            // InterpMapValueWithDerivatives (:211-249), MapProperties.cs:83-87
            ok[u] = i < n && !(!(cx == cx) || !(cy == cy) || cx < 0.0f || cx > limx || cy < 0.0f || cy > limy);
            const float fxx = floorf(cx), fyy = floorf(cy);                // :222
            const int ix = ok[u] ? (int)fxx : 0, iy = ok[u] ? (int)fyy : 0;
            fx[u] = cx - fxx; fy[u] = cy - fyy;                            // :225
            const int idx = iy * L.w + ix;                                 // :227
#if HS_PROB_MODE == 0
            if constexpr (RC) hs_cache_taps<!REP>(C, L.prob, idx, L.w, ok[u], r0[u], r1[u]);
            else {
                __builtin_memcpy(&r0[u], L.prob + idx, sizeof(float2));    // (two adjacent taps: one 8-byte load)
                __builtin_memcpy(&r1[u], L.prob + idx + L.w, sizeof(float2));
            }
#else
            int4 c0, c1;                                                   // (two adjacent cells {UpdateIndex, Value}: one 16-byte load)
            __builtin_memcpy(&c0, L.cells + idx, sizeof(int4));
            __builtin_memcpy(&c1, L.cells + idx + L.w, sizeof(int4));
            r0[u] = make_float2(hs_prob_tap(__int_as_float(c0.y)), hs_prob_tap(__int_as_float(c0.w)));
            r1[u] = make_float2(hs_prob_tap(__int_as_float(c1.y)), hs_prob_tap(__int_as_float(c1.w)));
#endif
        }
#pragma unroll
        for (int u = 0; u < PU; u++) {
            const float i0 = r0[u].x, i1 = r0[u].y, i2 = r1[u].x, i3 = r1[u].y;            // :230-233
            const float dx1 = i0 - i1, dx2 = i2 - i3, dy1 = i0 - i2, dy2 = i1 - i3;        // :235-239
            const float xi = 1.0f - fx[u], yi = 1.0f - fy[u];              // :241-242
            float P = ((i0 * xi + i1 * fx[u]) * yi) + ((i2 * xi + i3 * fx[u]) * fy[u]);   // :245-246
            float gx = -((dx1 * xi) + (dx2 * fx[u]));                      // :247
            float gy = -((dy1 * yi) + (dy2 * fy[u]));                      // :248
            if (!ok[u]) { P = 0.0f; gx = 0.0f; gy = 0.0f; }                // :216-219
            const float fun = 1.0f - P;                                    // :164
            const float rot = ((-sinRot * p[u].x - cosRot * p[u].y) * gx + (cosRot * p[u].x - sinRot * p[u].y) * gy);   // :169-170
            acc[0] += gx * fun;  acc[1] += gy * fun;  acc[2] += rot * fun; // :166,:167,:172
            acc[3] += gx * gx;   acc[4] += gy * gy;   acc[5] += rot * rot; // :174-176
            acc[6] += gx * gy;   acc[7] += gx * rot;  acc[8] += gy * rot;  // :178-180
            if constexpr (REP) {                                           // (a padding lane is no point: it adds nothing)
                if (base + (int)threadIdx.x + u * BDIM < n) acc[9] += fun * fun;
                cnt += ok[u] ? 1 : 0;
            }
        }
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#ifdef K4_TIMES
    if (threadIdx.x == 0 && blockIdx.x == 0) { g_k4_pts[g_k4_iter & 15] += wall_clock64() - k4_last; g_k4_iter++; }
#endif
    K4_STAMP(1)                                                            // points: taps, interpolation, products
    // the nine trees step by step side by side (independent adds between the steps of one tree), then one store block
#pragma unroll
    for (int k = 0; k < NS; k++) acc[k] += hs_dpp_f32<0xB1, 0xf>(acc[k]);          // quad_perm [1,0,3,2]
#pragma unroll
    for (int k = 0; k < NS; k++) acc[k] += hs_dpp_f32<0x4E, 0xf>(acc[k]);          // quad_perm [2,3,0,1]
#pragma unroll
    for (int k = 0; k < NS; k++) acc[k] += hs_dpp_f32<0x124, 0xf>(acc[k]);         // row_ror:4
#pragma unroll
    for (int k = 0; k < NS; k++) acc[k] += hs_dpp_f32<0x128, 0xf>(acc[k]);         // row_ror:8
#pragma unroll
    for (int k = 0; k < NS; k++) acc[k] += hs_dpp_f32<0x142, 0xa>(acc[k]);         // row_bcast:15 -> rows 1, 3
#pragma unroll
    for (int k = 0; k < NS; k++) acc[k] += hs_dpp_f32<0x143, 0xc>(acc[k]);         // row_bcast:31 -> rows 2, 3
    if constexpr (REP) cnt = sh_wave_scan_incl(cnt);                       // (lane 63: the wavefront's count)
    if (lane == 63) {
#pragma unroll
        for (int k = 0; k < NS; k++) red[k * NW + wid] = (double)acc[k];
        if constexpr (REP) red[NS * NW + wid] = (double)cnt;
    }
    K4_STAMP(2)                                                            // wave sums + store
    __syncthreads();
    K4_STAMP(3)                                                            // the barrier
    // every wavefront: nine sums over the NW wave partials; value v = k * NW + w sits in lane v & 63 of register v >> 6, so a
    // sum is one aligned group of NW lanes of a DPP row; after the tree the group's first lane holds it
    constexpr int NV = NS * NW, NR = (NV + 63) >> 6;
    double d[NR];
#pragma unroll
    for (int r = 0; r < NR; r++) d[r] = lane + 64 * r < NV ? red[lane + 64 * r] : 0.0;
#pragma unroll
    for (int r = 0; r < NR; r++) {
        if (NW >= 2) d[r] += hs_dpp_f64<0xB1, 0xf>(d[r]);
        if (NW >= 4) d[r] += hs_dpp_f64<0x4E, 0xf>(d[r]);
        if (NW == 8) d[r] += hs_dpp_f64<0x141, 0xf>(d[r]);             // row_half_mirror: the other quad of the group of 8
        if (NW >= 16) d[r] += hs_dpp_f64<0x124, 0xf>(d[r]);
        if (NW >= 16) d[r] += hs_dpp_f64<0x128, 0xf>(d[r]);
    }
    float f[NR];
#pragma unroll
    for (int r = 0; r < NR; r++) f[r] = (float)d[r];
#pragma unroll
    for (int k = 0; k < 9; k++)
        sums[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(f[(k * NW) >> 6]), (k * NW) & 63));
    if constexpr (REP) {
        *residual = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(f[(9 * NW) >> 6]), (9 * NW) & 63));
        int c = 0;
#pragma unroll
        for (int w = 0; w < NW; w++) c += (int)red[NS * NW + w];           // (integers below 2^31 in binary64: exact)
        *n_in_map = c;
    }
    K4_STAMP(4)                                                            // totals
#ifdef K4_TIMES
    if (threadIdx.x == 0 && blockIdx.x == 0) g_k4_last = k4_last;          // (stamp 5: from here to the next iteration's start: the step, the level change)
#endif
}

// ---- the reference's summation order (slamhip_hs_set_match_threads, opt-in) ---------------------------------------------------
// GetCompleteHessianDerivs with ScanMatcher(numThreads = T) (:149-195): the scan is cut into T chunks of ceil(n / T) points,
// chunk c = [c * chunk, min(n, (c + 1) * chunk)); each thread sums its chunk's nine terms point after point in binary32 from
// +0, and the nine totals are 0 + partial[0] + ... + partial[T - 1] in thread order.  Per window of W points (one pass of
// hs_hessian_block's loop) every lane forms its points' terms -- hs_point_taps / hs_point_terms, the same floats as the
// default order's -- into LDS as [9][WS]; then lane j < 9T runs chain (c = j / 9, k = j % 9) over the window's part of chunk c,
// its partial carried in a register from window to window.  No binary64, no tree: the result depends on T alone, not on the
// workgroup's width, so a batch of any size gives the single match's bits.
// The match report (REP, slamhip_match_report) carries a tenth row of terms, funVal * funVal, whose chains give the residual in
// the same chunk order (NR = 10 rows; a kernel that reports uses the ten-row block for its nine-row iterations too: one
// allocation), and counts the points inside the map per lane, wavefront and workgroup in integers.
template <int BDIM, int NR = 9> struct hs_ref_shape {
    static constexpr int W = BDIM * hs_shape<BDIM>::PU;                    // points per window (1080 rays: one window at any width)
    static constexpr int WS = W + 4;                                       // row stride in floats: rows 16-B aligned, and the nine rows
                                                                           // four banks apart (one chunk's nine chains: no conflict)
    static constexpr int CR = (NR * HS_REF_MAX_T + BDIM - 1) / BDIM;       // chains per lane
};
template <int N> struct hs_ref_cnt { int cnt[N]; };                       // (the report: the workgroup's count, then the wavefronts')
template <> struct hs_ref_cnt<0> {};
template <int BDIM, int NR = 9> struct __attribute__((aligned(16))) hs_ref_lds : hs_ref_cnt<NR == 9 ? 0 : 1 + hs_shape<BDIM>::NW> {
    float terms[NR * hs_ref_shape<BDIM>::WS];                              // 256 lanes: 46 KB -> 65 KB per workgroup, two per CU (ten rows: 51 KB -> 70 KB, still two)
    float part[NR * HS_REF_MAX_T];                                         // [c][k] the chunks' partials
    float sums[NR];
};
// the kernel's one block (a static in a device function: one allocation per kernel that calls it, none in the default kernels)
template <int BDIM, int NR = 9> __device__ static __forceinline__ hs_ref_lds<BDIM, NR> &hs_ref_lds_of()
{
    __shared__ hs_ref_lds<BDIM, NR> s;
    return s;
}

// acc + row[lo] + row[lo + 1] + ... + row[hi - 1], in that order.  Blocks of 32 in two register sets that take turns: the
// sixteen values of one set are requested while the other set's sixteen are added (no copies between the sets)
#define HS_ADD4(v) { acc += (v).x; acc += (v).y; acc += (v).z; acc += (v).w; }
__device__ static __forceinline__ float hs_chain(const float *row, int lo, int hi, float acc)
{
    int i = lo;
    for (; i < hi && (i & 3); i++) acc += row[i];
    if (i + 32 <= hi) {
        float4 a[4], b[4];
#pragma unroll
        for (int q = 0; q < 4; q++) { a[q] = *(const float4 *)(row + i + 4 * q); b[q] = *(const float4 *)(row + i + 16 + 4 * q); }
        for (i += 32; i + 32 <= hi; i += 32) {
#pragma unroll
            for (int q = 0; q < 4; q++) HS_ADD4(a[q]);
#pragma unroll
            for (int q = 0; q < 4; q++) a[q] = *(const float4 *)(row + i + 4 * q);
#pragma unroll
            for (int q = 0; q < 4; q++) HS_ADD4(b[q]);
#pragma unroll
            for (int q = 0; q < 4; q++) b[q] = *(const float4 *)(row + i + 16 + 4 * q);
        }
#pragma unroll
        for (int q = 0; q < 4; q++) HS_ADD4(a[q]);
#pragma unroll
        for (int q = 0; q < 4; q++) HS_ADD4(b[q]);
    }
    for (; i + 4 <= hi; i += 4) { const float4 v = *(const float4 *)(row + i); HS_ADD4(v); }
    for (; i < hi; i++) acc += row[i];
    return acc;
}
#undef HS_ADD4

// sums[9] in the order of hs_hessian_block, uniform in every thread; T in 1 .. HS_REF_MAX_T.  Barriers: one per window after the
// terms are stored (and one before the store of every window after the first), two for the totals.
// REP: as hs_hessian_block's (S is then the ten-row block)
template <int BDIM, bool RC, bool REP = false, int NRS = 9>
__device__ static __forceinline__ void hs_hessian_ref(const hs_level_dev &L, const hs_cache_lv &C, const float2 *pts, int n, const float pose[3], int T,
                                                      hs_ref_lds<BDIM, NRS> &S, float sums[9], float *residual = nullptr, int *n_in_map = nullptr)
{
    static_assert(!REP || NRS == 10, "the report's pass needs the ten-row block");
    constexpr int NR = REP ? 10 : 9;                                       // rows of terms = chains per chunk
    constexpr int PU = hs_shape<BDIM>::PU, W = hs_ref_shape<BDIM>::W, WS = hs_ref_shape<BDIM>::WS, CR = hs_ref_shape<BDIM, NR>::CR;
    const hs_iter_xf X = hs_iter_transform(L, pose);
    const int chunk = (n + T - 1) / T;                                     // :149
    const int tid = threadIdx.x;
    float part[CR];
#pragma unroll
    for (int r = 0; r < CR; r++) part[r] = 0.0f;                           // :156-157
    int cnt = 0;
    for (int base = 0; base < n; base += W) {
        hs_point q[PU];
#pragma unroll
        for (int u = 0; u < PU; u++) hs_point_taps<RC, !REP>(L, C, pts, base + tid + u * BDIM, n, X, q[u]);
        float tm[PU][NR];
#pragma unroll
        for (int u = 0; u < PU; u++) hs_point_terms<NR>(q[u], X, tm[u]);
        if constexpr (REP) {
#pragma unroll
            for (int u = 0; u < PU; u++) cnt += q[u].ok ? 1 : 0;
        }
        if (base > 0) __syncthreads();                                     // (the previous window's chains have read their terms)
#pragma unroll
        for (int u = 0; u < PU; u++)
#pragma unroll
            for (int k = 0; k < NR; k++) S.terms[k * WS + tid + u * BDIM] = tm[u][k];
        __syncthreads();
        const int end = min(n, base + W);
#pragma unroll
        for (int r = 0; r < CR; r++) {
            const int j = tid + r * BDIM;
            if (j < NR * T) {
                const int c = j / NR, k = j - NR * c;
                const int lo = max(c * chunk, base), hi = min(min(c * chunk + chunk, n), end);   // :159 Skip / Take
                if (lo < hi) part[r] = hs_chain(S.terms + k * WS, lo - base, hi - base, part[r]);   // :166-180
            }
        }
    }
#pragma unroll
    for (int r = 0; r < CR; r++) {
        const int j = tid + r * BDIM;
        if (j < NR * T) S.part[j] = part[r];
    }
    if constexpr (REP) {
        cnt = sh_wave_scan_incl(cnt);                                      // (lane 63: the wavefront's count)
        if ((tid & 63) == 63) S.cnt[1 + (tid >> 6)] = cnt;
    }
    __syncthreads();
    if (tid < NR) {
        float s = 0.0f;                                                    // :188-189
        for (int c = 0; c < T; c++) s += S.part[NR * c + tid];             // :191-195 (empty chunks: +0)
        S.sums[tid] = s;
    }
    if constexpr (REP) {
        if (tid == 64) { int c = 0; for (int w = 0; w < hs_shape<BDIM>::NW; w++) c += S.cnt[1 + w]; S.cnt[0] = c; }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 9; k++) sums[k] = S.sums[k];
    if constexpr (REP) { *residual = S.sums[9]; *n_in_map = S.cnt[0]; }
}

// EstimateTransformationLogLh (:93-125) applied by every thread identically (uniform registers)
__device__ static inline void hs_step(const float sums[9], float est[3])
{
    const float H[9] = { sums[3], sums[6], sums[7],  sums[6], sums[4], sums[8],  sums[7], sums[8], sums[5] };  // :198-200
    if (H[0] != 0.0f && H[4] != 0.0f) {                                    // :97
        float R[9];
        if (!sh_invert_h(H, R)) return;                                    // :99-103
        const float d0 = sums[0], d1 = sums[1], d2 = sums[2];
        float sx = (d0 * R[0]) + (d1 * R[3]) + (d2 * R[6]) + 0.0f;         // :105 Vector3.Transform(dTr, iH)
        float sy = (d0 * R[1]) + (d1 * R[4]) + (d2 * R[7]) + 0.0f;
        float sz = (d0 * R[2]) + (d1 * R[5]) + (d2 * R[8]) + 0.0f;
        if (sz > 0.2f) sz = 0.2f;                                          // :107-111
        else if (sz < -0.2f) sz = -0.2f;                                   // :113-117
        est[0] += sx; est[1] += sy; est[2] += sz;                          // :119
    }
}

// MatchData(MapRepMultiMap) (:41-54): one workgroup per hint; levels coarse -> fine.
// only_level >= 0 restricts to one level with `iters_override` iterations (MatchData(OccGridMap), :64-84).
// REF: the reference's summation order for ref_threads = T chunks (hs_hessian_ref); the default instantiations ignore ref_threads.
// RC: every tap through the reference's cache RCA (hs_cache_taps; the host launches no helper workgroups then); the default
// instantiations ignore RCA.
// REP: the match report (slamhip_match_report) -- after the level loop the workgroup evaluates GetCompleteHessianDerivs once more,
// at the pose the match ends on and on the report level (level 0, or only_level), with the residual and the in-map count riding
// through the same reduction (hs_hessian_block / hs_hessian_ref <REP>): one more pass over the points that are still in LDS, in
// the same launch.  With RC its taps observe the cache and fill nothing: the reference makes no such evaluation, and a fill
// would decide later answers across Reset.  Lane 0 stores the report to RP.out[b] -- for a single blocking match that is the
// pyramid's pinned report block, stored before the mailbox's sequence word is released -- and, for slamhip_hs_match_best, puts
// (bits(residual) << 32 | b) to a 64-bit minimum at agent scope: a residual is >= +0, so its bits order as its value does, a NaN
// sorts after every number, equal residuals go to the lowest index (K1's packed key).  The default instantiations ignore RP.
struct hs_report_arg { slamhip_match_report *out; unsigned long long *best_key; };
template <int BDIM, bool REF, bool RC, bool REP>
__global__ void __launch_bounds__(BDIM)
k4_match(hs_levels_arg A, const float2 *__restrict__ pts, int n, const float *__restrict__ hints, float3 hint1,
         float *__restrict__ out, int only_level, int iters_override, uint32_t *mail, uint32_t mail_seq,
         const float2 *up_src, float2 *up_dst, uint32_t *up_flag, uint32_t up_seq, int n_helpers_from, int ref_threads,
         hs_cache_arg RCA, hs_report_arg RP)
{
    __shared__ double red[2 * hs_shape<BDIM>::RED];
    static_assert(2 * hs_shape<BDIM>::RED >= hs_shape<BDIM>::RED_REP, "the report's pass reuses the iterations' reduction blocks");
    constexpr int NRS = REP ? 10 : 9;                                      // rows of the reference order's block (hs_ref_lds)
    __shared__ float2 pts_s[HS_LDS_PTS];
    const int b = blockIdx.x;
    if (n_helpers_from > 0 && b >= n_helpers_from) {
        // Round 6 -- the single match's HELPER workgroups.  In the per-scan flow the grid update has just rewritten the cached
        // probabilities from every XCD, and the first iteration on each level finds none of its taps in the L2 (the points' phase:
        // 14.0 us per match against 8.9 on a resting pyramid).  Requesting the finer levels' taps early from the matching
        // workgroup itself was measured a loss in round 5 (its own taps queue behind them).  Workgroups are dealt to the XCDs round
        // robin, so workgroup 8 of the launch shares its L2 with workgroup 0: it requests the lines of the FINER levels' taps at the
        // hint pose -- the match moves the pose by a cell or two, a line holds 32 -- while workgroup 0 iterates on the coarse level,
        // and leaves.  Workgroups 1 .. 7 (other XCDs) leave at once.  Nothing is written: a prefetch, never a result.
#ifndef K4_HELP_ALL
#define K4_HELP_ALL 0
#endif
        if ((!K4_HELP_ALL && (b & 7) != 0) || n <= 0 || only_level >= 0) return;
        // (The points are read from the DEVICE copy, never from the staging block: the host may refill -- or free and reallocate -- that
        // block as soon as workgroup 0 has read it, long before this workgroup runs; round 6's soak, seed 6105, a memory access fault.
        // On a freshly set scan the device copy still holds the previous scan, or a mixture while workgroup 0 stores the new one: end
        // points of consecutive scans fall on the same lines, and whatever floats are found there are range-tested like any point.)
        const float2 *src = pts;
        float acc = 0.f;
        for (int l = A.n - (K4_HELP_ALL == 2 ? 1 : 2); l >= 0; l--) {
            const hs_level_dev &L = A.lv[l];
            float est[3];
            sh_v2_transform(hint1.x, hint1.y, L.map_t_world, &est[0], &est[1]);
            est[2] = hint1.z;
            float s, c;
            sh_det_sincosf(est[2], &s, &c);
            const sh_m3x2 t = sh_m3x2_mul(sh_m3x2_mul(hs_rotation_sc(est[2], s, c), sh_m3x2_translation(est[0] * L.cell, est[1] * L.cell)), sh_m3x2_scale(L.stm));
            const float limx = (float)L.w - 2.0f, limy = (float)L.h - 2.0f;
            for (int i = threadIdx.x; i < n; i += BDIM) {
                const float2 p = src[i];
                float cx, cy;
                sh_v2_transform(p.x, p.y, t, &cx, &cy);
                const bool ok = !(!(cx == cx) || !(cy == cy) || cx < 0.0f || cx > limx || cy < 0.0f || cy > limy);
                const int idx = ok ? (int)floorf(cy) * L.w + (int)floorf(cx) : 0;
                acc += L.prob[idx] + L.prob[idx + L.w];
            }
        }
        asm volatile("" :: "v"(acc));                                       // (the loads are kept; their values are not)
        return;
    }
    float est_w[3] = { hint1.x, hint1.y, hint1.z };                         // :43 (a single hint travels in the launch arguments)
    if (hints) { est_w[0] = hints[3 * b]; est_w[1] = hints[3 * b + 1]; est_w[2] = hints[3 * b + 2]; }
#ifdef K4_TIMES
    if (threadIdx.x == 0 && blockIdx.x == 0) g_k4_iter = 0;
#endif
    const bool in_lds = n <= HS_LDS_PTS;
    if (up_src || in_lds) {
        // The scan's points into LDS, every lane's loads requested together (one memory round trip, not one per point).
        // up_src: a single match on a freshly set scan (one workgroup, n <= HS_LDS_PTS) reads them straight from the pinned
        // staging block -- this launch IS the scan upload -- and stores them to the device copy for the launches that follow
        // (grid update); the stores depend on the loads, so after the barrier the staging block has been read and the host may
        // refill it.
        constexpr int FU = HS_LDS_PTS / BDIM;
        const float2 *src = up_src ? up_src : pts;
        float2 v[FU];
#pragma unroll
        for (int u = 0; u < FU; u++) { const int i = threadIdx.x + u * BDIM; if (i < n) v[u] = src[i]; }
#pragma unroll
        for (int u = 0; u < FU; u++) {
            const int i = threadIdx.x + u * BDIM;
            if (i < n) { pts_s[i] = v[u]; if (up_src) up_dst[i] = v[u]; }
        }
        __syncthreads();
        if (up_src && threadIdx.x < SH_UPLOAD_PARTS) __hip_atomic_store(up_flag + threadIdx.x, up_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);   // (the words of sh_upload: common.h)
    }
    // (Round 5, measured and rejected: the finer levels' taps requested early -- one LDS-DMA word per point and row at the hint
    // pose, into a dump nobody reads, issued inside the first iteration so that their lines arrive while the coarse level
    // iterates.  In the per-scan flow the grid update has just rewritten the cached probabilities from every XCD and the points'
    // phase takes 14.0 us per match instead of 8.9 on a resting pyramid, but the requests cost more than the misses they avoid:
    // 23.6 -> 25.5 us per match stand-alone, 30.7 -> 34.0 us inside HectorSLAMProcessor.Update -- vector memory returns in
    // order, so the coarse level's own taps queue behind them, and twelve scattered 4-byte requests per lane are as much work
    // for the address unit as two iterations' taps.)
    if (n > 0) {                                                           // :66 (else: hint returned, :83)
        const int l_hi = only_level >= 0 ? only_level : A.n - 1;
        const int l_lo = only_level >= 0 ? only_level : 0;
        int par = 0;
        for (int l = l_hi; l >= l_lo; l--) {                               // :47
            const hs_level_dev &L = A.lv[l];
            hs_cache_lv C = { nullptr, 0 };
            if constexpr (RC) { C.c = RCA.c[l]; C.epoch = RCA.epoch[l]; }
            float est[3];
            sh_v2_transform(est_w[0], est_w[1], L.map_t_world, &est[0], &est[1]);   // :68 GetMapCoordsPose
            est[2] = est_w[2];
            const int iters = only_level >= 0 ? iters_override : L.iterations;
            for (int it = 0; it < iters; it++) {                           // :70-73
                float sums[9];
                if constexpr (REF) {
                    if (in_lds) hs_hessian_ref<BDIM, RC, false>(L, C, pts_s, n, est, ref_threads, hs_ref_lds_of<BDIM, NRS>(), sums);
                    else hs_hessian_ref<BDIM, RC, false>(L, C, pts, n, est, ref_threads, hs_ref_lds_of<BDIM, NRS>(), sums);
                } else {
                    if (in_lds) hs_hessian_block<BDIM, true, RC>(L, C, pts_s, n, est, red + par, sums);
                    else hs_hessian_block<BDIM, false, RC>(L, C, pts, n, est, red + par, sums);
                    par ^= hs_shape<BDIM>::RED;                            // (a block is written again two barriers after it was read)
                }
                hs_step(sums, est);
            }
            est[2] = sh_normalize_angle(est[2]);                           // :76
            sh_v2_transform(est[0], est[1], L.world_t_map, &est_w[0], &est_w[1]);   // :79 GetWorldCoordsPose
            est_w[2] = est[2];
        }
    }
    if constexpr (REP) {
        const int rl = only_level >= 0 ? only_level : 0;
        const hs_level_dev &L = A.lv[rl];
        hs_cache_lv C = { nullptr, 0 };
        if constexpr (RC) { C.c = RCA.c[rl]; C.epoch = RCA.epoch[rl]; }
        float pm[3];
        sh_v2_transform(est_w[0], est_w[1], L.map_t_world, &pm[0], &pm[1]);    // GetMapCoordsPose (GridMap.cs:133-137)
        pm[2] = est_w[2];
        float sums[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 }, residual = 0.0f;
        int n_in = 0;
        if (n > 0) {
            if constexpr (REF) {
                if (in_lds) hs_hessian_ref<BDIM, RC, true>(L, C, pts_s, n, pm, ref_threads, hs_ref_lds_of<BDIM, NRS>(), sums, &residual, &n_in);
                else hs_hessian_ref<BDIM, RC, true>(L, C, pts, n, pm, ref_threads, hs_ref_lds_of<BDIM, NRS>(), sums, &residual, &n_in);
            } else {
                __syncthreads();                                           // (every wavefront has read the last iteration's block)
                if (in_lds) hs_hessian_block<BDIM, true, RC, true>(L, C, pts_s, n, pm, red, sums, &residual, &n_in);
                else hs_hessian_block<BDIM, false, RC, true>(L, C, pts, n, pm, red, sums, &residual, &n_in);
            }
        }
        if (threadIdx.x == 0) {
            slamhip_match_report &R = RP.out[b];
            R.pose_map[0] = pm[0]; R.pose_map[1] = pm[1]; R.pose_map[2] = pm[2];
            R.H[0] = sums[3]; R.H[1] = sums[6]; R.H[2] = sums[7];          // :198-200, as k4_hessian lays it out
            R.H[3] = sums[6]; R.H[4] = sums[4]; R.H[5] = sums[8];
            R.H[6] = sums[7]; R.H[7] = sums[8]; R.H[8] = sums[5];
            R.dTr[0] = sums[0]; R.dTr[1] = sums[1]; R.dTr[2] = sums[2];
            R.residual = residual; R.n_in_map = n_in; R.n_points = n; R.level = rl;
            if (RP.best_key)
                __hip_atomic_fetch_min(RP.best_key, ((unsigned long long)__float_as_uint(residual) << 32) | (unsigned)b,
                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (threadIdx.x == 0) {
        out[3 * b] = est_w[0]; out[3 * b + 1] = est_w[1]; out[3 * b + 2] = est_w[2];
        if (mail) {                                                        // a single blocking match: the pose and the completion word into the context's mailbox (common.h)
            ((float *)mail)[0] = est_w[0]; ((float *)mail)[1] = est_w[1]; ((float *)mail)[2] = est_w[2];
            __hip_atomic_store(mail + 15, mail_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

template <bool REF, bool RC>
__global__ void __launch_bounds__(256)
k4_hessian(hs_levels_arg A, int level, const float2 *__restrict__ pts, int n, const float *__restrict__ pose_in,
           float *__restrict__ out12, int ref_threads, hs_cache_arg RCA)
{
    __shared__ double red[hs_shape<256>::RED];
    float pose[3] = { pose_in[0], pose_in[1], pose_in[2] };
    float sums[9];
    hs_cache_lv C = { nullptr, 0 };
    if constexpr (RC) { C.c = RCA.c[level]; C.epoch = RCA.epoch[level]; }
    if constexpr (REF) hs_hessian_ref<256, RC>(A.lv[level], C, pts, n, pose, ref_threads, hs_ref_lds_of<256>(), sums);
    else hs_hessian_block<256, false, RC>(A.lv[level], C, pts, n, pose, red, sums);
    if (threadIdx.x == 0) {
        out12[0] = sums[3]; out12[1] = sums[6]; out12[2] = sums[7];
        out12[3] = sums[6]; out12[4] = sums[4]; out12[5] = sums[8];
        out12[6] = sums[7]; out12[7] = sums[8]; out12[8] = sums[5];
        out12[9] = sums[0]; out12[10] = sums[1]; out12[11] = sums[2];
    }
}

// slamhip_hs_match_best: the winner of the batch that the launch in front of it matched -- the index in the key's low word (k4_match
// <REP>) -- with its pose and report copied to where the host reads them: four words (pose, index) and the report's nineteen, then
// the completion word if the call waits on the mailbox.  A launch of its own and not a last-arriving workgroup of the match: the
// kernel boundary orders every workgroup's report before this read with no fence or counter in the matcher, at the price of one
// launch boundary (~2 us) on a batch of B matches.  It also puts the key word back to "no candidate" for the next call, in-stream.
#define HS_KEY_NONE 0xFFFFFFFFFFFFFFFFull
__global__ void __launch_bounds__(64)
k4_best_pick(unsigned long long *key, const float *__restrict__ poses, const slamhip_match_report *__restrict__ reps,
             uint32_t *dst4, uint32_t *dst_report, uint32_t *mail, uint32_t mail_seq)
{
    const unsigned idx = (unsigned)*key;
    const int t = threadIdx.x;
    constexpr int RW = (int)(sizeof(slamhip_match_report) / 4);
    // every lane's word into a register first, stores behind the barrier: the destinations may overlap the sources (without the
    // mailbox the four words go to the head of the I/O block and the report to report 0)
    uint32_t w = idx;
    if (t < 3) w = __float_as_uint(poses[3 * (size_t)idx + t]);
    else if (t >= 32 && t < 32 + RW) w = ((const uint32_t *)(reps + idx))[t - 32];
    __syncthreads();
    if (t < 4) dst4[t] = w;
    else if (t >= 32 && t < 32 + RW) dst_report[t - 32] = w;
    __syncthreads();                                                       // (one wavefront: every lane has read the key and stored its word)
    if (t == 0) {
        *key = HS_KEY_NONE;
        if (mail) __hip_atomic_store(mail + 15, mail_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------
static hs_levels_arg levels_arg(slamhip_hs *hs)
{
    hs_levels_arg A;
    memset(&A, 0, sizeof(A));
    A.n = hs->n_levels;
    for (int l = 0; l < hs->n_levels; l++) {
        const hs_level &L = hs->lv[l];
        A.lv[l].w = L.w; A.lv[l].h = L.h; A.lv[l].cell = L.cell; A.lv[l].stm = L.stm;
        A.lv[l].map_t_world = L.map_t_world; A.lv[l].world_t_map = L.world_t_map;
        A.lv[l].prob = L.d_prob; A.lv[l].cells = L.d_cells; A.lv[l].iterations = L.iterations;
    }
    return A;
}

static hs_cache_arg cache_arg(slamhip_hs *hs)
{
    hs_cache_arg C;
    memset(&C, 0, sizeof(C));
    for (int l = 0; l < hs->n_levels; l++) { C.c[l] = hs->lv[l].d_cache; C.epoch[l] = hs->lv[l].curr_cache_index; }
    return C;
}

static int32_t ensure_io(slamhip_hs *hs, int floats)
{
    if (floats <= hs->cap_io) return SLAMHIP_OK;
    (void)hipFree(hs->d_io); (void)hipHostFree(hs->h_io);
    hs->d_io = nullptr; hs->h_io = nullptr; hs->cap_io = 0;
    SH_HIP(hipMalloc(&hs->d_io, sizeof(float) * (size_t)floats * 2));
    SH_HIP(hipHostMalloc(&hs->h_io, sizeof(float) * (size_t)floats * 2));
    hs->cap_io = floats * 2;
    return SLAMHIP_OK;
}

// room for B reports (device and pinned) and the best-of-batch key word, which starts as "no candidate" by a memset on the stream
static int32_t ensure_rep(slamhip_hs *hs, int B)
{
    if (!hs->d_best_key) {
        SH_HIP(hipMalloc(&hs->d_best_key, sizeof(unsigned long long)));
        SH_HIP(hipMemsetAsync(hs->d_best_key, 0xFF, sizeof(unsigned long long), hs->ctx->stream));
    }
    if (B <= hs->cap_rep) return SLAMHIP_OK;
    SH_HIP(hipStreamSynchronize(hs->ctx->stream));
    (void)hipFree(hs->d_rep);
    if (hs->h_rep) (void)hipHostFree(hs->h_rep);
    hs->d_rep = nullptr; hs->h_rep = nullptr; hs->cap_rep = 0;
    const int cap = B < 64 ? 64 : B + B / 4;
    SH_HIP(hipMalloc(&hs->d_rep, sizeof(slamhip_match_report) * (size_t)cap));
    SH_HIP(hipHostMalloc(&hs->h_rep, sizeof(slamhip_match_report) * (size_t)cap, hipHostMallocMapped | hipHostMallocCoherent));
    hs->cap_rep = cap;
    return SLAMHIP_OK;
}

// defer_seq: (single match through the mailbox only) return after the launch with the completion number in *defer_seq -- the
// caller holds the mailbox lock, enqueues what it wants behind the match and then calls hs_match_collect
int32_t hs_match_collect(slamhip_hs *hs, uint32_t seq, float *out, slamhip_match_report *out_report)
{
    slamhip_ctx *ctx = hs->ctx;
    SH_TRY(sh_flag_wait(ctx, ctx->mailbox + 15, seq));
    const volatile float *m = (const volatile float *)ctx->mailbox;
    out[0] = m[0]; out[1] = m[1]; out[2] = m[2];
    if (out_report) memcpy(out_report, hs->h_rep, sizeof(*out_report));    // (stored in front of the sequence word: k4_match <REP>)
    hs->launch_done = hs->match_launch_no;                                 // (the match has delivered: every launch before it has finished)
    return SLAMHIP_OK;
}

// every instantiation of k4_match, by [512 lanes?][REF][RC][REP] (one signature: the template arguments change the body only)
typedef decltype(&k4_match<256, false, false, false>) k4_match_fn;
static const k4_match_fn k4_match_tab[2][2][2][2] = {
    { { { k4_match<256, false, false, false>, k4_match<256, false, false, true> }, { k4_match<256, false, true, false>, k4_match<256, false, true, true> } },
      { { k4_match<256, true, false, false>, k4_match<256, true, false, true> }, { k4_match<256, true, true, false>, k4_match<256, true, true, true> } } },
    { { { k4_match<512, false, false, false>, k4_match<512, false, false, true> }, { k4_match<512, false, true, false>, k4_match<512, false, true, true> } },
      { { k4_match<512, true, false, false>, k4_match<512, true, false, true> }, { k4_match<512, true, true, false>, k4_match<512, true, true, true> } } },
};

int32_t hs_run_match(slamhip_hs *hs, const float *hints, int B, float *out, int only_level, int iters, uint32_t *defer_seq, const hs_report_req *rq)
{
    SH_HIP(hipSetDevice(hs->ctx->device));
    slamhip_ctx *ctx = hs->ctx;
    sh_mail_guard lock(ctx);                                              // (the mailbox is the context's: common.h)
    SH_TRY(ensure_io(hs, 6 * B));
    if (rq) SH_TRY(ensure_rep(hs, B));
    const bool best = rq && rq->best_index;                               // (its result is delivered by k4_best_pick, not by the match)
    float *d_in = hs->d_io, *d_out = hs->d_io + 3 * (size_t)B;
    const bool mail1 = B == 1 && !ctx->mail_off && !best;                 // one match: the kernel itself delivers the pose to the host
    // ... and pulls a freshly set scan from the staging block itself (k4_match): no upload launch in the per-scan chain
    const bool pull = B == 1 && hs->upload_pending && hs->n_points > 0 && hs->n_points <= HS_LDS_PTS;
    const float2 *up_src = nullptr; float2 *up_dst = nullptr; uint32_t *up_flag = nullptr; uint32_t up_seq = 0;
    if (pull) {                                                           // (committed below, once the launch is in the stream)
        up_src = (const float2 *)hs->h_pts; up_dst = hs->d_pts; up_flag = (uint32_t *)(hs->h_pts + 2 * (size_t)hs->cap_points);
        up_seq = hs->upload_seq + 1;
        hs->pts_use[hs->pts_buf] = ++hs->launch_count;
    } else SH_TRY(hs_flush_scan(hs));
    hs->match_launch_no = hs->launch_count;
    if (B > 1) {
        memcpy(hs->h_io, hints, sizeof(float) * 3 * (size_t)B);
        SH_HIP(hipMemcpyAsync(d_in, hs->h_io, sizeof(float) * 3 * (size_t)B, hipMemcpyHostToDevice, ctx->stream));
    }
    uint32_t mail_seq = 0;
    if (defer_seq && !mail1) SH_FAIL(SLAMHIP_ERR_STATE, "a deferred match is a single match through the mailbox");
    {
        sh_timer t(ctx, SLAMHIP_K_HS_MATCH);
        // a single match is a latency chain on one compute unit, bound by VALU issue: 512 lanes (two wavefronts per SIMD, three
        // scan points per lane at 1080 rays; hs_hessian_block -- rocprofv3, 1080 rays, 3 levels: 1024 lanes 33.7 us, 512 23.9,
        // 256 25.9); batches run 256 lanes per hint (many workgroups per CU)
        const float *d_hints = B > 1 ? (const float *)d_in : (const float *)nullptr;
        const float3 h1 = make_float3(hints[0], hints[1], hints[2]);
        uint32_t *mb = mail1 ? ctx->mailbox : (uint32_t *)nullptr;
        if (mail1) mail_seq = sh_mail_seq_next(ctx);
        const int lanes = B <= 8 ? 512 : 256;
        // (a single full match in the per-scan flow brings helper workgroups: k4_match)
        // (none with the reference's cache: a helper would have to read the cache entries, and must not fill them)
        static const int helpers_env = (int)sh_env_int("SLAMHIP_K4_HELPERS", 1);
        const bool rc = hs->ref_cache != 0;
        const int helpers = !rc && B == 1 && only_level < 0 && hs->n_levels > 1 && hs->n_points > 0 && helpers_env > 0 ? 8 * helpers_env : 0;
        const int T = hs->match_threads;
        // (the report of a single blocking match goes straight to the pinned block; a batch's stay on the device until they are asked for)
        hs_report_arg RP = { rq ? (mail1 ? hs->h_rep : hs->d_rep) : (slamhip_match_report *)nullptr, best ? hs->d_best_key : (unsigned long long *)nullptr };
        // (T > 0: the reference's order, the same bits at every width)
        hipLaunchKernelGGL(k4_match_tab[lanes == 512][T != 0][rc][rq != nullptr], dim3(B + helpers), dim3(lanes), 0, ctx->stream, levels_arg(hs), hs->d_pts, hs->n_points, d_hints,
                           h1, d_out, only_level, iters, mb, mail_seq, up_src, up_dst, up_flag, up_seq, helpers ? B : 0, T, cache_arg(hs), RP);
    }
    SH_HIP(hipGetLastError());
    if (pull) { hs->upload_pending = false; hs->upload_seq = up_seq; hs->pts_in_flight = true; }
#ifdef K4_TIMES
    {
        static thread_local int calls = 0;
        if (B == 1 && ++calls == 20) {
            (void)hipStreamSynchronize(ctx->stream);
            unsigned long long h[16];
            (void)hipMemcpyFromSymbol(h, HIP_SYMBOL(g_k4_times), sizeof(h));
            static const char *nm[7] = { "transform+trig", "points", "wave sums", "barrier", "totals", "step..next (and the gap between matches)", "-" };
            double tot = 0;
            for (int k = 0; k < 7; k++) tot += (double)h[k];
            fprintf(stderr, "[k4 times] %d matches, thread 0 of the workgroup, us per match:", calls);
            for (int k = 0; k < 7; k++) fprintf(stderr, " %s %.2f |", nm[k], (double)h[k] * 0.01 / calls);
            fprintf(stderr, " sum %.2f\n", tot * 0.01 / calls);
            unsigned long long hp[16];
            (void)hipMemcpyFromSymbol(hp, HIP_SYMBOL(g_k4_pts), sizeof(hp));
            fprintf(stderr, "[k4 times] the points' phase per iteration, us:");
            for (int k = 0; k < 12; k++) fprintf(stderr, " %.2f", (double)hp[k] * 0.01 / calls);
            fprintf(stderr, "\n");
        }
    }
#endif
    if (mail1 && !best) {
        if (defer_seq) { *defer_seq = mail_seq; return SLAMHIP_OK; }
        return hs_match_collect(hs, mail_seq, out, rq ? rq->out_reports : nullptr);
    }
    if (best) {
        // only the winner travels: k4_best_pick copies its pose, index and report out -- to the mailbox and the pinned report block,
        // with one wait on the sequence word, or (SLAMHIP_NO_HOSTWAIT) to device memory for a copy and a synchronise
        uint32_t *d4 = (uint32_t *)hs->d_io, *d19 = (uint32_t *)hs->d_rep;     // (the hints have been read; report 0 is copied in place when it wins)
        const uint32_t seq = ctx->mail_off ? 0 : sh_mail_seq_next(ctx);
        hipLaunchKernelGGL(k4_best_pick, dim3(1), dim3(64), 0, ctx->stream, hs->d_best_key, (const float *)d_out, (const slamhip_match_report *)hs->d_rep,
                           ctx->mail_off ? d4 : ctx->mailbox, ctx->mail_off ? d19 : (uint32_t *)hs->h_rep, ctx->mail_off ? (uint32_t *)nullptr : ctx->mailbox, seq);
        SH_HIP(hipGetLastError());
        uint32_t w[4];
        if (!ctx->mail_off) {
            SH_TRY(sh_flag_wait(ctx, ctx->mailbox + 15, seq));
            const volatile uint32_t *m = ctx->mailbox;
            for (int k = 0; k < 4; k++) w[k] = m[k];
            hs->launch_done = hs->match_launch_no;
        } else {
            SH_HIP(hipMemcpyAsync(hs->h_io, d4, sizeof(w), hipMemcpyDeviceToHost, ctx->stream));
            SH_HIP(hipMemcpyAsync(hs->h_rep, d19, sizeof(slamhip_match_report), hipMemcpyDeviceToHost, ctx->stream));
            SH_HIP(hipStreamSynchronize(ctx->stream));
            memcpy(w, hs->h_io, sizeof(w));
        }
        memcpy(out, w, sizeof(float) * 3);
        *rq->best_index = (int32_t)w[3];
        memcpy(rq->out_reports, hs->h_rep, sizeof(slamhip_match_report));
        return SLAMHIP_OK;
    }
    SH_HIP(hipMemcpyAsync(hs->h_io + 3 * (size_t)B, d_out, sizeof(float) * 3 * (size_t)B, hipMemcpyDeviceToHost, ctx->stream));
    if (rq) SH_HIP(hipMemcpyAsync(hs->h_rep, hs->d_rep, sizeof(slamhip_match_report) * (size_t)B, hipMemcpyDeviceToHost, ctx->stream));
    SH_HIP(hipStreamSynchronize(ctx->stream));
    memcpy(out, hs->h_io + 3 * (size_t)B, sizeof(float) * 3 * (size_t)B);
    if (rq) memcpy(rq->out_reports, hs->h_rep, sizeof(slamhip_match_report) * (size_t)B);
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_set_match_threads(slamhip_hs *hs, int32_t num_threads)
{
    SH_CHECK_ARG(hs && num_threads >= 0 && num_threads <= HS_REF_MAX_T);
    hs->match_threads = num_threads;                                      // (read by the next launch of K4: nothing on the device)
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_set_reference_cache(slamhip_hs *hs, int32_t on)
{
    SH_CHECK_ARG(hs && (on == 0 || on == 1));
#if HS_PROB_MODE != 0
    if (on) SH_FAIL(SLAMHIP_ERR_STATE, "the reference's cache needs the probability grids (HS_PROB_MODE 0)");
#endif
    if (on && !hs->ref_cache) {
        SH_HIP(hipSetDevice(hs->ctx->device));
        for (int l = 0; l < hs->n_levels; l++) {
            hs_level &L = hs->lv[l];
            if (L.d_cache) continue;
            if (hipMalloc(&L.d_cache, sizeof(unsigned long long) * (size_t)L.w * L.h) != hipSuccess) {
                (void)hipGetLastError();
                for (int k = 0; k < hs->n_levels; k++) { (void)hipFree(hs->lv[k].d_cache); hs->lv[k].d_cache = nullptr; }   // (the mode is off: nothing reads them)
                SH_FAIL(SLAMHIP_ERR_NOMEM, "device allocation of the reference's cache failed (level %d)", l);
            }
        }
        // every switch to on starts from a new OccGridMap's cache (:38-42): fills made while the mode was off were never recorded
        for (int l = 0; l < hs->n_levels; l++) hs_cache_clear_enqueue(hs, l);
        SH_HIP(hipGetLastError());
    }
    hs->ref_cache = on;                                                   // (read by the next launch of K4 and slamhip_hs_probability)
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_match(slamhip_hs *hs, const float hint[3], float out[3])
{
    SH_CHECK_ARG(hs && hint && out);
    return hs_run_match(hs, hint, 1, out, -1, 0);
}

extern "C" int32_t slamhip_hs_match_level(slamhip_hs *hs, int32_t level, const float hint[3], int32_t iterations, float out[3])
{
    SH_CHECK_ARG(hs && hint && out && level >= 0 && level < hs->n_levels && iterations >= 0);
    return hs_run_match(hs, hint, 1, out, level, iterations);
}

extern "C" int32_t slamhip_hs_match_batch(slamhip_hs *hs, const float *hints, int32_t B, float *out)
{
    SH_CHECK_ARG(hs && hints && out && B > 0);
    return hs_run_match(hs, hints, B, out, -1, 0);
}

extern "C" int32_t slamhip_hs_match_report(slamhip_hs *hs, const float hint[3], float out[3], slamhip_match_report *out_report)
{
    SH_CHECK_ARG(hs && hint && out && out_report);
    const hs_report_req rq = { out_report, nullptr };
    return hs_run_match(hs, hint, 1, out, -1, 0, nullptr, &rq);
}

extern "C" int32_t slamhip_hs_match_level_report(slamhip_hs *hs, int32_t level, const float hint[3], int32_t iterations, float out[3],
                                                 slamhip_match_report *out_report)
{
    SH_CHECK_ARG(hs && hint && out && out_report && level >= 0 && level < hs->n_levels && iterations >= 0);
    const hs_report_req rq = { out_report, nullptr };
    return hs_run_match(hs, hint, 1, out, level, iterations, nullptr, &rq);
}

extern "C" int32_t slamhip_hs_match_batch_report(slamhip_hs *hs, const float *hints, int32_t B, float *out, slamhip_match_report *out_reports)
{
    SH_CHECK_ARG(hs && hints && out && out_reports && B > 0);
    const hs_report_req rq = { out_reports, nullptr };
    return hs_run_match(hs, hints, B, out, -1, 0, nullptr, &rq);
}

extern "C" int32_t slamhip_hs_match_best(slamhip_hs *hs, const float *hints, int32_t B, float out[3], int32_t *out_index,
                                         slamhip_match_report *out_report)
{
    SH_CHECK_ARG(hs && hints && out && out_index && out_report && B > 0);
    const hs_report_req rq = { out_report, out_index };
    return hs_run_match(hs, hints, B, out, -1, 0, nullptr, &rq);
}

// ... and of k4_hessian, by [REF][RC]
typedef decltype(&k4_hessian<false, false>) k4_hessian_fn;
static const k4_hessian_fn k4_hessian_tab[2][2] = { { k4_hessian<false, false>, k4_hessian<false, true> }, { k4_hessian<true, false>, k4_hessian<true, true> } };

extern "C" int32_t slamhip_hs_hessian(slamhip_hs *hs, int32_t level, const float pose_map[3], float H[9], float dTr[3])
{
    SH_CHECK_ARG(hs && pose_map && H && dTr && level >= 0 && level < hs->n_levels);
    SH_HIP(hipSetDevice(hs->ctx->device));
    slamhip_ctx *ctx = hs->ctx;
    SH_TRY(ensure_io(hs, 32));
    SH_TRY(hs_flush_scan(hs));
    memcpy(hs->h_io, pose_map, sizeof(float) * 3);
    SH_HIP(hipMemcpyAsync(hs->d_io, hs->h_io, sizeof(float) * 3, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k4_hessian_tab[hs->match_threads != 0][hs->ref_cache != 0], dim3(1), dim3(256), 0, ctx->stream, levels_arg(hs), level, hs->d_pts, hs->n_points,
                       (const float *)hs->d_io, hs->d_io + 16, hs->match_threads, cache_arg(hs));
    SH_HIP(hipGetLastError());
    SH_HIP(hipMemcpyAsync(hs->h_io + 16, hs->d_io + 16, sizeof(float) * 12, hipMemcpyDeviceToHost, ctx->stream));
    SH_HIP(hipStreamSynchronize(ctx->stream));
    memcpy(H, hs->h_io + 16, sizeof(float) * 9);
    memcpy(dTr, hs->h_io + 25, sizeof(float) * 3);
    return SLAMHIP_OK;
}
