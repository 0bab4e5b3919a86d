// hs_update.hip -- K5, the log-odds grid update of HectorSLAM (slamhip_hs_update_by_scan).
//
// K5 replaces OccGridMap.UpdateByScan and friends (HectorSLAM/Map/OccGridMap.cs:114-239) for every level of
// the pyramid (MapRepMultiMap.cs:73-77) in one launch.  The once-per-scan guards make a cell's new value depend only on
// (a) whether it is touched as free, (b) whether it is an end point, and (c) whether the first free touch
// precedes the first end-point touch in ray order.  No atomics and no per-cell scratch: lines are sorted
// by direction class and slope (raster.h, shared with the HoleMap update); a cell has ONE writer -- the wavefront of a
// cell near the begin cell, or beyond that the lane of the lowest line index among the lines that touch it (one lane
// per (line, step), closed-form Bresenham position) -- which finds the first "free" line and the first line that ends
// in the cell and replays the at most two state transitions literally: bit-exact fp32 cell values and update indices.
// The cells are stored as the reference stores them, LogOddsCell {UpdateIndex, Value} (LogOddsCell.cs:16-21): one 8-byte access.
#include "hs_internal.h"
#include "raster.h"
#include <vector>
#include <atomic>

// ---- K5 device code --------------------------------------------------------------------------------------------
// One line of OccGridMap.UpdateByScan on one level: UpdateLineBresenhami (:155-190) + Bresenham2D (:220-239).
// The line has da "free" cells (steps i = 0..da-1, the end point excluded, :224-238) plus the occupied end cell; after
// i steps the walk has taken (e0 + i*db) / da minor steps, e0 = da / 2 (closed form of :228-235, db <= da;
// tests/test_closed_forms.py).  The update is CELL-centric (raster.h): a cell asks which lines draw it.  Lines are
// processed in index order by the reference, and a cell changes at most twice per update (BresenhamCellFree marks it,
// BresenhamCellOcc overrides the mark), so all a cell needs is the smallest index of a line that crosses it as "free",
// the smallest index of a line that ends in it, and their order -- no atomics, no per-cell scratch, coalesced rows.
struct k5_level { int w, h; sh_m3x2 t; slamhip_cell *cells; float *prob; int mark_free, mark_occ; int wg0, wgn; };
// a cell as one 8-byte word: update_index in the low half, the value's bits in the high half (slamhip_cell, include/slamhip.h)
__device__ static __forceinline__ void k5_load_cell(const slamhip_cell *c, float &v, int &u) { const int2 w = *(const int2 *)c; u = w.x; v = __int_as_float(w.y); }
__device__ static __forceinline__ void k5_store_cell(slamhip_cell *c, float v, int u) { *(int2 *)c = make_int2(u, __float_as_int(v)); }
struct k5_arg { k5_level lv[HS_MAX_LEVELS]; int n; };
struct k5_line { int da, sdb, ray, flags; };      // major length, signed minor length, line index, valid | major_x << 1 | (smaj + 1) << 2
#define K5_ZONE 16                     // Chebyshev radius around the begin cell handled one wavefront per cell
#define K5_HDR 8                       // ints per level: [0] begin x, [1] begin y, [2] longest line, [3] valid lines, [4] first valid line

// does the line draw cell (major offset a >= 1, signed minor offset b)?  1: as a free cell, 2: as its end cell, 0: no
__device__ static inline int k5_hit(const k5_line c, int a, int b)
{
    if (a > c.da) return 0;
    const int B = b < 0 ? -b : b, db = c.sdb < 0 ? -c.sdb : c.sdb;
    if (B > 0 && (c.sdb == 0 || (b > 0) != (c.sdb > 0))) return 0;
    if (a == c.da) return B == db ? 2 : 0;                                 // the end cell (:187), excluded from the free steps
    const int e = c.da / 2 + a * db;                                       // minor steps = e / da (maps <= 32768 a side: < 2^31)
    return (e >= B * c.da && e < (B + 1) * c.da) ? 1 : 0;
}

// per level (blockIdx.x): the lines of the scan, counting-sorted by (direction class, slope bucket)
__global__ void __launch_bounds__(1024)
k5_prepare(k5_arg A, const float2 *__restrict__ pts, int n, float ox, float oy, int cap, k5_line *__restrict__ byidx_all,
           k5_line *__restrict__ cand_all, int *__restrict__ start_all, int *__restrict__ hdr_all)
{
    __shared__ int hist[4 * RS_NBUCK];
    __shared__ int wsum[16];
    __shared__ int s_R, s_nv, s_first;
    const k5_level &L = A.lv[blockIdx.x];
    k5_line *byidx = byidx_all + (size_t)blockIdx.x * cap, *cand = cand_all + (size_t)blockIdx.x * cap;
    int *start = start_all + (size_t)blockIdx.x * (4 * RS_NBUCK + 1), *hdr = hdr_all + blockIdx.x * K5_HDR;
    const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
    for (int i = t; i < 4 * RS_NBUCK; i += 1024) hist[i] = 0;
    if (t == 0) { s_R = 0; s_nv = 0; s_first = 0x7fffffff; }
    __syncthreads();
    float bxf, byf;
    sh_v2_transform(ox, oy, L.t, &bxf, &byf);                              // :126
    const int bx = sh_f2i(rintf(bxf)), by = sh_f2i(rintf(byf));            // :127 ToRoundPoint (banker's, VectorEx.cs:183-186)
    int my_R = 0, my_nv = 0, my_first = 0x7fffffff;
    k5_line keep[2];                                                       // a thread's first two lines stay in registers for the second pass
    keep[0].flags = 0; keep[1].flags = 0;
    for (int i = t, it = 0; i < n; i += 1024, it++) {
        float exf, eyf;
        sh_v2_transform(pts[i].x, pts[i].y, L.t, &exf, &eyf);              // :133
        const int ex = sh_f2i(rintf(exf)), ey = sh_f2i(rintf(eyf));        // :134
        const bool same = (bx == ex) & (by == ey);                         // :137
        const bool inside = (bx >= 0) & (by >= 0) & (bx < L.w) & (by < L.h) & (ex >= 0) & (ey >= 0) & (ex < L.w) & (ey < L.h);   // :158-161
        k5_line e; e.da = 0; e.sdb = 0; e.ray = i; e.flags = 0;
        if (!same && inside) {
            const int dx = ex - bx, dy = ey - by;
            const int adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy;
            const bool major_x = adx >= ady;                               // :175
            e.da = major_x ? adx : ady;
            e.sdb = major_x ? dy : dx;                                     // minor extent with its sign (:169-170)
            const int smaj = sh_sign(major_x ? dx : dy);
            e.flags = 1 | (major_x ? 2 : 0) | ((smaj + 1) << 2);
            atomicAdd(&hist[rs_class(major_x, smaj) * RS_NBUCK + rs_bucket((float)e.sdb / (float)e.da)], 1);
            my_R = max(my_R, e.da);
            my_nv++;
            my_first = min(my_first, i);
        }
        byidx[i] = e;
        if (it == 0) keep[0] = e; else if (it == 1) keep[1] = e;
    }
    for (int off = 32; off > 0; off >>= 1) {
        my_R = max(my_R, __shfl_down(my_R, off, 64)); my_nv += __shfl_down(my_nv, off, 64); my_first = min(my_first, __shfl_down(my_first, off, 64));
    }
    if (lane == 0) { atomicMax(&s_R, my_R); atomicAdd(&s_nv, my_nv); atomicMin(&s_first, my_first); }
    __syncthreads();
    {   // exclusive prefix over the 4096 bins: 4 consecutive bins per thread
        int v[4], sum = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) { v[k] = hist[4 * t + k]; sum += v[k]; }
        int incl = sum;
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_up(incl, off, 64);
            if (lane >= off) incl += o;
        }
        if (lane == 63) wsum[wid] = incl;
        __syncthreads();
        int base = incl - sum;
        for (int w = 0; w < wid; w++) base += wsum[w];
#pragma unroll
        for (int k = 0; k < 4; k++) { start[4 * t + k] = base; hist[4 * t + k] = base; base += v[k]; }
        if (t == 1023) start[4 * RS_NBUCK] = base;
    }
    __syncthreads();
    for (int i = t, it = 0; i < n; i += 1024, it++) {
        const k5_line e = it == 0 ? keep[0] : it == 1 ? keep[1] : byidx[i];      // (its own store: no other thread wrote byidx[i])
        if (e.flags & 1) {
            const int smaj = ((e.flags >> 2) & 3) - 1;
            const int pos = atomicAdd(&hist[rs_class((e.flags & 2) != 0, smaj) * RS_NBUCK + rs_bucket((float)e.sdb / (float)e.da)], 1);
            cand[pos] = e;
        }
    }
    if (t == 0) { hdr[0] = bx; hdr[1] = by; hdr[2] = s_R; hdr[3] = s_nv; hdr[4] = s_first; }
}

// the state transitions of one cell: BresenhamCellFree (:192-199) by the first line that crosses it, then
// BresenhamCellOcc (:201-218) by the first line that ends in it; a cell first touched by an end point is not
// marked free any more (the mark_occ update index is above mark_free)
// (hs_render.h holds a TWIN of this function, hs_cell_transition, and of the line-making of k5_prepare / k5_cells<true>, hs_line_make,
// for K20: change one and change the other -- DESIGN.md section 4 "K20" says why they are two; tests/test_gpu_hector_render.py holds
// them to == on every cell)
__device__ static inline void k5_transition(const k5_level &L, float &v, int &u, int first_free, int first_occ, float lo_free, float lo_occ)
{
    if (first_free < first_occ && u < L.mark_free) { v += lo_free; u = L.mark_free; }     // :192-199
    if (first_occ != 0x7fffffff && u < L.mark_occ) {                       // :201-218
        if (u == L.mark_free) v -= lo_free;                                // :206-209
        if (v < 50.0f) v += lo_occ;                                        // :211-214
        u = L.mark_occ;                                                    // :216
    }
}

// wave-wide minimum by DPP (butterfly in rows of 16, row_bcast:15 / :31): valid in lane 63
template <int CTRL, int ROWS> __device__ static inline int k5_dpp(int v) { return __builtin_amdgcn_update_dpp(v, v, CTRL, ROWS, 0xf, false); }
__device__ static inline int k5_wave_min(int x)
{
    x = min(x, (k5_dpp<0xB1, 0xf>(x))); x = min(x, (k5_dpp<0x4E, 0xf>(x)));
    x = min(x, (k5_dpp<0x124, 0xf>(x))); x = min(x, (k5_dpp<0x128, 0xf>(x)));
    x = min(x, (k5_dpp<0x142, 0xa>(x))); x = min(x, (k5_dpp<0x143, 0xc>(x)));
    return x;
}

// all levels in ONE launch.  BUILD (scans of up to K5_LDS_LINES points): every workgroup makes the line tables of ITS level
// itself, in LDS -- the transform of :133-134 per point, the counting sort by (direction class, slope bucket) -- instead of
// reading what a k5_prepare launch left in memory (5 us plus a launch boundary for a microsecond of arithmetic).  The order of
// the lines inside a bucket then differs from workgroup to workgroup (LDS atomics), so the work that is shared out between
// workgroups goes by LINE INDEX (byidx), never by table position.
#define K5_LDS_FIXED ((4 * RS_NBUCK + 4) * 4)
#ifndef K5_EXP
#define K5_EXP 0
#endif
#ifdef K5_TIMES
// developer instrumentation (build with SLAMHIP_K5_TIMES=1): 100 MHz wall-clock stamps per workgroup: start, tables, zone, end
__device__ unsigned long long g_k5_times[1024 * 4];
#define K5_STAMP(k) { if (threadIdx.x == 0 && blockIdx.x < 1024) g_k5_times[blockIdx.x * 4 + (k)] = wall_clock64(); }
__device__ unsigned long long g_k5_sub[1024 * 8];    // table phase, thread 0: behind the 1st barrier, the lines, the bins' prefix (2 stamps), the scatter
#define K5_SUB(k) { if (threadIdx.x == 0 && blockIdx.x < 1024) g_k5_sub[blockIdx.x * 8 + (k)] = wall_clock64(); }
#else
#define K5_STAMP(k) {}
#define K5_SUB(k) {}
#endif
#define K5_SEC 16                      // ints per level of the sector record: [0] the scan's line count, [1..9] the bounds of the eight sectors
// The sector bounds for the NEXT update, by the level's first workgroup when it has drawn its last cell (its tables still stand
// in LDS): a line's weight is its blocks of 64 steps beyond the zone (x 8) plus the fetch every line costs; an inclusive scan
// of the weights by line index (DPP wave scans, one wavefront for the wave totals); sector k starts behind the line in which the
// running weight passes k/8 of the total.  All 1024 threads of the workgroup call it.
template <int RPT>
__device__ static inline void k5_sector_bounds(const k5_line *__restrict__ byidx_s, int n_pts, int *s_wtot, int *s_wsum_all, int *s_bound,
                                               int *__restrict__ rec_out)
{
    const int t = threadIdx.x, lane_ = t & 63, wid = t >> 6;
    int wgt[RPT], wincl[RPT];
    if (t < 9) s_bound[t] = t == 0 ? 0 : n_pts;
#pragma unroll
    for (int it = 0; it < RPT; it++) {
        const int i = t + it * 1024;
        int w = 0;
        if (i < n_pts) {
            const k5_line ee = byidx_s[i];
            const int bl = ((ee.flags & 1) && ee.da >= K5_ZONE) ? (ee.da - K5_ZONE) / 64 + 1 : 0;
            w = 8 * bl + 2;
        }
        int incl = w;
        incl += __builtin_amdgcn_update_dpp(0, incl, 0x111, 0xf, 0xf, true);   // row_shr:1
        incl += __builtin_amdgcn_update_dpp(0, incl, 0x112, 0xf, 0xf, true);   // row_shr:2
        incl += __builtin_amdgcn_update_dpp(0, incl, 0x114, 0xf, 0xf, true);   // row_shr:4
        incl += __builtin_amdgcn_update_dpp(0, incl, 0x118, 0xf, 0xf, true);   // row_shr:8
        incl += __builtin_amdgcn_update_dpp(0, incl, 0x142, 0xa, 0xf, false);  // row_bcast:15 -> rows 1, 3
        incl += __builtin_amdgcn_update_dpp(0, incl, 0x143, 0xc, 0xf, false);  // row_bcast:31 -> rows 2, 3
        wgt[it] = w; wincl[it] = incl;
        if (lane_ == 63) s_wtot[it * 16 + wid] = incl;
    }
    __syncthreads();
    if (wid == 0) {        // the (at most 48) wave totals into their exclusive prefix; the total behind them
        constexpr int NT = RPT * 16;
        static_assert(NT <= 63, "the wave totals and their sum fit one wavefront");
        const int v = lane_ < NT ? s_wtot[lane_] : 0;
        int incl = v;
        incl += __builtin_amdgcn_update_dpp(0, incl, 0x111, 0xf, 0xf, true);
        incl += __builtin_amdgcn_update_dpp(0, incl, 0x112, 0xf, 0xf, true);
        incl += __builtin_amdgcn_update_dpp(0, incl, 0x114, 0xf, 0xf, true);
        incl += __builtin_amdgcn_update_dpp(0, incl, 0x118, 0xf, 0xf, true);
        incl += __builtin_amdgcn_update_dpp(0, incl, 0x142, 0xa, 0xf, false);
        incl += __builtin_amdgcn_update_dpp(0, incl, 0x143, 0xc, 0xf, false);
        if (lane_ < NT) s_wtot[lane_] = incl - v;
        if (lane_ == 63) *s_wsum_all = incl;
    }
    __syncthreads();
    const int run = *s_wsum_all;
#pragma unroll
    for (int it = 0; it < RPT; it++) {
        const int i = t + it * 1024;
        if (i < n_pts) {
            const int incl = s_wtot[it * 16 + wid] + wincl[it], excl = incl - wgt[it];
#pragma unroll
            for (int k = 1; k < 8; k++) {
                const int ck = (k * run + 7) >> 3;
                if (excl < ck && ck <= incl) s_bound[k] = i + 1;           // (exactly one line per threshold: the weights are positive)
            }
        }
    }
    __syncthreads();
    if (t == 0) rec_out[0] = n_pts;
    if (t < 9) rec_out[1 + t] = s_bound[t];
}
static inline size_t k5_lds_bytes(bool build, int n) { return (size_t)K5_LDS_FIXED + (build ? (size_t)4 * RS_NBUCK * 4 + (size_t)32 * (size_t)((n + 3) & ~3) : 0); }
template <bool BUILD>
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(8, 8)))
k5_cells(k5_arg A, int cap, const float2 *__restrict__ pts, int n_pts, float ox, float oy,
         const k5_line *__restrict__ byidx_all, const k5_line *__restrict__ cand_all,
         const int *__restrict__ start_all, const int *__restrict__ hdr_all, float lo_free, float lo_occ,
         const int *__restrict__ sec_in, int *__restrict__ sec_out, const k5_gate gate)
{
    extern __shared__ __attribute__((aligned(16))) char k5_smem[];
    int *start = (int *)k5_smem;
    int *pos_s = (int *)(k5_smem + K5_LDS_FIXED);
    const int n4 = (n_pts + 3) & ~3;
    k5_line *cand_s = (k5_line *)(pos_s + (BUILD ? 4 * RS_NBUCK : 0));
    k5_line *byidx_s = cand_s + (BUILD ? n4 : 0);
    __shared__ __attribute__((aligned(16))) int wsum[16];
    __shared__ int s_R, s_nv, s_first;
    __shared__ int s_bound[9], s_rec[10], s_wsum_all, s_wtot[((K5_LDS_LINES + 1023) / 1024) * 16];   // BUILD: the sectors of phase 2 (below)
    // workgroups are shared out over the levels (host: wg0, wgn)
    int lvl = 0;
    for (int l = 1; l < A.n; l++) if ((int)blockIdx.x >= A.lv[l].wg0) lvl = l;
    const k5_level &L = A.lv[lvl];
    int bx, by, R, nv, first_line;
    K5_STAMP(0)
    sh_m3x2 T = L.t;
    if (BUILD && gate.on) {                                                 // (uniform: scalar loads, every wavefront the same answer)
        const float pose[3] = { gate.d_pose[0], gate.d_pose[1], gate.d_pose[2] };
        if (!hs_moved_enough(pose, gate.last, gate.min_dist, gate.min_angle)) return;
        T = sh_m3x2_mul(sh_m3x2_mul(sh_m3x2_rotation(pose[2]), sh_m3x2_translation(pose[0], pose[1])), sh_m3x2_scale(gate.stm[lvl]));   // OccGridMap.cs:120-123
    }
    if (BUILD) {
        const int t = threadIdx.x, lane_ = t & 63, wid = t >> 6;
        constexpr int RPT = (K5_LDS_LINES + 1023) / 1024;
        float2 p_next = make_float2(0.f, 0.f);
        if (t < n_pts) p_next = pts[t];
        for (int i = t; i < 4 * RS_NBUCK; i += 1024) start[i] = 0;          // (the histogram, then the bucket table)
        if (t == 0) { s_R = 0; s_nv = 0; s_first = 0x7fffffff; }
        int rec_v = -1;                                                     // (the sectors the level's first workgroup left last time: below;
        if (t < 10 && sec_in) rec_v = sec_in[lvl * K5_SEC + t];            //  requested here, stored behind the lines loop: no wait of its own)
        __syncthreads();
        K5_SUB(0)
        float bxf, byf;
        sh_v2_transform(ox, oy, T, &bxf, &byf);                            // :126
        bx = sh_f2i(rintf(bxf)); by = sh_f2i(rintf(byf));                  // :127 ToRoundPoint (banker's, VectorEx.cs:183-186)
        int bkt[RPT];
#pragma unroll
        for (int k = 0; k < RPT; k++) bkt[k] = -1;
        int my_R = 0, my_nv = 0, my_first = 0x7fffffff;
#pragma unroll 1
        for (int it = 0; it * 1024 < n_pts; it++) {
            const int i = t + it * 1024;
            int bb = -1;
            const float2 p = p_next;
            if (i + 1024 < n_pts) p_next = pts[i + 1024];
            if (i < n_pts) {
                float exf, eyf;
                sh_v2_transform(p.x, p.y, T, &exf, &eyf);                  // :133
                const int ex = sh_f2i(rintf(exf)), ey = sh_f2i(rintf(eyf));    // :134
                const bool same = (bx == ex) & (by == ey);                 // :137
                const bool inside = (bx >= 0) & (by >= 0) & (bx < L.w) & (by < L.h) & (ex >= 0) & (ey >= 0) & (ex < L.w) & (ey < L.h);   // :158-161
                k5_line e; e.da = 0; e.sdb = 0; e.ray = i; e.flags = 0;
                if (!same && inside) {
                    const int dx = ex - bx, dy = ey - by;
                    const int adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy;
                    const bool major_x = adx >= ady;                       // :175
                    e.da = major_x ? adx : ady;
                    e.sdb = major_x ? dy : dx;                             // minor extent with its sign (:169-170)
                    const int smaj = sh_sign(major_x ? dx : dy);
                    e.flags = 1 | (major_x ? 2 : 0) | ((smaj + 1) << 2);
                    bb = rs_class(major_x, smaj) * RS_NBUCK + rs_bucket((float)e.sdb / (float)e.da);
                    atomicAdd(&start[bb], 1);
                    my_R = max(my_R, e.da);
                    my_nv++;
                    my_first = min(my_first, i);
                }
                byidx_s[i] = e;
            }
#pragma unroll
            for (int k = 0; k < RPT; k++) if (k == it) bkt[k] = bb;
        }
        // (wave reductions by DPP, common.h: eighteen shuffles -- ds_bpermute, ~100 cycles each, on an LDS pipe that 32 wavefronts
        // of the compute unit use at once in this phase -- were a microsecond of it)
        my_R = sh_wave_max_to_lane63(my_R); my_nv = sh_wave_scan_incl(my_nv); my_first = sh_wave_min_all(my_first);
        if (lane_ == 63) { atomicMax(&s_R, my_R); atomicAdd(&s_nv, my_nv); atomicMin(&s_first, my_first); }
        if (t < 10) s_rec[t] = rec_v;
        __syncthreads();
        K5_SUB(1)
        // Phase 2's sectors: the lines go to the XCDs in eight ranges of consecutive indices (locality: see phase 2) that hold EQUAL
        // WORK, not equal counts -- with equal counts the sectors of the benchmark scan took 3.9 .. 13.6 us on level 0 (the long
        // corridor against the near wall; SLAMHIP_K5_TIMES) and the launch waited for the slowest.  The bounds are those the level's
        // first workgroup worked out during the LAST update (k5_sector_bounds at the end of this kernel; consecutive scans look
        // alike, and any partition is correct -- only the balance depends on it): making them here, in every workgroup, cost the
        // table phase 2 us (eight wavefronts per SIMD run that phase at once: an instruction more in it is 15 ns more).
        {   // exclusive prefix over the 4096 bins: 4 consecutive bins per thread
            int v[4], sum = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) { v[k] = start[4 * t + k]; sum += v[k]; }
            const int incl = sh_wave_scan_incl(sum);
            if (lane_ == 63) wsum[wid] = incl;
            __syncthreads();                                               // (every thread has read its bins)
        K5_SUB(2)
            int base = incl - sum;
            {   // the wave totals in front of this one: four 16-byte reads, not up to fifteen dependent ones
                const int4 *w4 = (const int4 *)wsum;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int4 x = w4[q];
                    base += (4 * q + 0 < wid ? x.x : 0) + (4 * q + 1 < wid ? x.y : 0) + (4 * q + 2 < wid ? x.z : 0) + (4 * q + 3 < wid ? x.w : 0);
                }
            }
#pragma unroll
            for (int k = 0; k < 4; k++) { start[4 * t + k] = base; pos_s[4 * t + k] = base; base += v[k]; }
            if (t == 1023) start[4 * RS_NBUCK] = base;
        }
        __syncthreads();
        K5_SUB(3)
#pragma unroll
        for (int it = 0; it < RPT; it++) {
            const int i = t + it * 1024;
            if (i < n_pts && bkt[it] >= 0) cand_s[atomicAdd(&pos_s[bkt[it]], 1)] = byidx_s[i];      // (this thread's own store)
        }
        R = s_R; nv = s_nv; first_line = s_first;
        __syncthreads();
        K5_SUB(4)
        if (nv == 0) {
            if (sec_out && (int)blockIdx.x == L.wg0 && t == 0) sec_out[lvl * K5_SEC] = -1;      // (no record for the next update)
            return;
        }
        // From which step on is a line ALONE on its cells (round 5; K2's finding, holemap.hip)?  Step a of a line lies at minor offset
        // floor(a * slope + h), h = (da / 2) / da in [1/2 - 1/(2 da), 1/2] (:228-235), so two lines of a class -- signed slopes: a
        // cell of minor offset 0 is shared across the sign -- meet at major offset a only if a * |slope difference| < 1 + 1/(2 da):
        // beyond the zone (da >= 16) never from a = 1.0625 / g + 2 on, g the smallest slope difference to any other line of the class.
        // A thread per line looks at the twelve buckets either side of the line's own (no line in sight: g >= 10 bucket widths) and leaves
        // the step in bits 5 .. 17 of the line's flags; from there on the line's step lanes of phase 2 look nothing up (a cell on
        // the diagonal, which the quadrant's other class touches too, excepted).  No barrier: a lane that reads the word before it
        // is written finds zero = "not known" and takes the lookup -- slower, never wrong.
        // Only the lines of this workgroup's own sector (phase 2 below) are asked about.
        {
            const int wg_l_ = (int)blockIdx.x - L.wg0, xcd_ = wg_l_ & 7;
            const bool rec_ok_ = s_rec[0] == n_pts;
            const int c0_ = xcd_ == 0 ? 0 : rec_ok_ ? s_rec[1 + xcd_] : (int)(((long long)n_pts * xcd_) >> 3);
            const int c1_ = xcd_ == 7 ? n_pts : rec_ok_ ? s_rec[2 + xcd_] : (int)(((long long)n_pts * (xcd_ + 1)) >> 3);
            for (int i = c0_ + t; i < c1_; i += 1024) {
                const k5_line e = byidx_s[i];
                if (!(e.flags & 1) || e.da < K5_ZONE) continue;
                const float sl = (float)e.sdb * __builtin_amdgcn_rcpf((float)e.da);
                const int smaj = ((e.flags >> 2) & 3) - 1;
                const int cb = rs_class((e.flags & 2) != 0, smaj) * RS_NBUCK, bk = cb + rs_bucket(sl);
                const int w0 = start[max(bk - 12, cb)], w1 = start[min(bk + 12, cb + RS_NBUCK - 1) + 1];    // (the table's buckets come from the exact quotient: one bucket of slack)
                float g = 10.0f * (2.0f / (float)RS_NBUCK);
                int same = 0;                                              // (lines with this very slope: its own, and any other -> never alone)
                for (int ci = w0; ci < w1; ci++) {
                    const k5_line c = cand_s[ci];
                    const float d = fabsf((float)c.sdb * __builtin_amdgcn_rcpf((float)c.da) - sl);
                    same += d == 0.0f ? 1 : 0;
                    g = d > 0.0f && d < g ? d : g;
                }
                // (slopes by the hardware reciprocal: each within 2.5e-7 of the quotient; equal quotients that come out an ulp apart
                // make g tiny, i.e. "never alone")
                const int xa = same == 1 && g > 4.0e-6f ? min((int)(1.0625f * __builtin_amdgcn_rcpf(g - 1.0e-6f) * 1.0001f) + 2, 8191) : 8191;
                byidx_s[i].flags = e.flags | (xa << 5);
            }
        }
    } else {
        const int *start_g = start_all + (size_t)lvl * (4 * RS_NBUCK + 1), *hdr = hdr_all + lvl * K5_HDR;
        bx = hdr[0]; by = hdr[1]; R = hdr[2]; nv = hdr[3]; first_line = hdr[4];
        if (nv == 0) return;
        for (int i = threadIdx.x; i <= 4 * RS_NBUCK; i += 1024) start[i] = start_g[i];
        __syncthreads();
    }
    K5_STAMP(1)
#if K5_EXP == 1                          // developer experiment (wrong results): the launch with its table phase alone
    return;
#endif
    const k5_line *cand = BUILD ? cand_s : cand_all + (size_t)lvl * cap;
    const k5_line *byidx = BUILD ? byidx_s : byidx_all + (size_t)lvl * cap;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int gw = ((int)blockIdx.x - L.wg0) * 16 + wv, nw = L.wgn * 16;
    // (1) the zone around the begin cell, where a cell has many candidate lines: one wavefront per cell, one candidate
    //     per lane and trip, the smallest indices by wave reduction.  The begin cell itself is step 0 of every line.
    const int Z = K5_ZONE - 1 < R ? K5_ZONE - 1 : R;
    const int side = 2 * Z + 1;
    for (int item = gw; item < side * side; item += nw) {
        const int X = bx - Z + item % side, Y = by - Z + item / side;
        if (X < 0 || X >= L.w || Y < 0 || Y >= L.h) continue;              // wave-uniform
        const int dx = X - bx, dy = Y - by;
        const int cell = Y * L.w + X;
        float v; int u;
        k5_load_cell(L.cells + cell, v, u);                                // (requested now, needed after the search)
        int first_free = 0x7fffffff, first_occ = 0x7fffffff;
        if (dx == 0 && dy == 0) first_free = first_line;
        else {
            int cls[2], a[2], b[2];
            const int ncls = rs_classes(dx, dy, cls, a, b);
            for (int k = 0; k < ncls; k++) {
                int lo, hi;
                rs_range(start, cls[k], a[k], b[k], 0.5f, lo, hi);
                for (int ci = lo + lane; ci < hi; ci += 64) {
                    const k5_line c = cand[ci];
                    const int h = k5_hit(c, a[k], b[k]);
                    if (h == 1) first_free = min(first_free, c.ray);
                    else if (h == 2) first_occ = min(first_occ, c.ray);
                }
            }
            first_free = k5_wave_min(first_free);                          // valid in lane 63
            first_occ = k5_wave_min(first_occ);
        }
        if (lane == 63 && (first_free != 0x7fffffff || first_occ != 0x7fffffff)) {
            k5_transition(L, v, u, first_free, first_occ, lo_free, lo_occ);
            k5_store_cell(L.cells + cell, v, u);
#if HS_PROB_MODE == 0
            L.prob[cell] = hs_prob_v(v);
#endif
        }
    }
    // (2) beyond the zone: one lane per (line, step) -- work proportional to the cells the scan touches, not to the scan's
    //     bounding square (rounds 1-2 visited every cell of the square: ~5 M lanes for ~1.1 M touched cells over three levels of
    //     a 2048^2 pyramid).  Step i of a line lies at major offset i (its Chebyshev distance from the begin cell) and minor
    //     offset floor((da / 2 + i * db) / da) (:220-239; k5_hit is the same closed form), the end cell at i = da.  The lane
    //     asks, like a cell-centric lane would, which lines touch its cell -- one contiguous range of the slope-sorted table;
    //     nearly always the range holds the lane's own line and nothing else, and the cell is updated at once.  Otherwise the
    //     candidates are tested and the lane of the LOWEST line index among the touching lines owns the cell (every touching
    //     line has a lane on it, and all of them see the same candidates): it applies the transitions, the others drop it.
    //     Lines are dealt by index (a scan's points come in order of their angle), to the XCDs by sector: a line's cells share
    //     their 128-byte rows with its neighbours'.
    K5_STAMP(2)
#if K5_EXP == 2                          // developer experiment (wrong results): tables and the zone, no lines beyond it
    return;
#endif
    if (R < K5_ZONE) {
        if (BUILD && sec_out && (int)blockIdx.x == L.wg0 && threadIdx.x == 0) sec_out[lvl * K5_SEC] = -1;
        return;
    }
    const int wg_l = (int)blockIdx.x - L.wg0;                              // workgroup within the level
    const int xcd = wg_l & 7, wgs_x = (L.wgn - xcd + 7) >> 3, wg_x = wg_l >> 3;
    // (BUILD: the sectors hold equal work, and a sector's blocks end with ITS longest line -- see the tables above)
    const int nblk = (R - K5_ZONE) / 64 + 1;
    const bool rec_ok = BUILD && s_rec[0] == n_pts;                        // (a record of a scan with as many lines: its bounds are a partition of this one's)
    const int c0 = xcd == 0 ? 0 : rec_ok ? s_rec[1 + xcd] : (int)(((long long)n_pts * xcd) >> 3);
    const int n_sec = (xcd == 7 ? n_pts : rec_ok ? s_rec[2 + xcd] : (int)(((long long)n_pts * (xcd + 1)) >> 3)) - c0;
    const int items = nblk * n_sec;
    // (software pipeline: a cell's value and update index are requested when its item is fetched, two iterations before its
    // turn -- the cells and probabilities of a 2048^2 level are 48 MB, a microsecond or two away; two ahead against one: 32.6 -> 32.2 us,
    // and the kernel's 64 VGPRs leave no room for a third)
    struct k5_item { int cell, dx, dy, ray, end, xalone; float v; int u; };
#define K5_FETCH(it, item_)                                                                         \
    {                                                                                               \
        (it).cell = -1;                                                                             \
        if ((item_) < items) {                                                                      \
            const int blk_ = (item_) / n_sec, ci0_ = c0 + ((item_) - blk_ * n_sec);                 \
            const k5_line me_ = byidx[ci0_];               /* (uniform: a broadcast) */              \
            const int i_ = K5_ZONE + blk_ * 64 + lane;                                              \
            if ((me_.flags & 1) && i_ <= me_.da) {                                                                     \
                const int db_ = me_.sdb < 0 ? -me_.sdb : me_.sdb;                                   \
                const int e_ = me_.da / 2 + i_ * db_;      /* (maps <= 32768 a side: < 2^31) */      \
                int m_;                                                                             \
                if (L.w <= 2048 && L.h <= 2048) {          /* e < 2^24: the float estimate of e / da is within one; settled exactly */ \
                    m_ = (int)((float)e_ * __builtin_amdgcn_rcpf((float)me_.da));                   \
                    const int r_ = e_ - m_ * me_.da;                                                \
                    if (r_ < 0) m_--; else if (r_ >= me_.da) m_++;                                  \
                } else m_ = e_ / me_.da;                                                            \
                const int smaj_ = ((me_.flags >> 2) & 3) - 1;                                       \
                const int am_ = smaj_ < 0 ? -i_ : i_, bm_ = me_.sdb < 0 ? -m_ : m_;                 \
                (it).dx = (me_.flags & 2) ? am_ : bm_; (it).dy = (me_.flags & 2) ? bm_ : am_;       \
                (it).ray = me_.ray; (it).end = i_ == me_.da;                                        \
                { const int xa_ = (me_.flags >> 5) & 8191; (it).xalone = (xa_ == 0 || xa_ == 8191) ? 0x7fffffff : xa_; } \
                (it).cell = (by + (it).dy) * L.w + (bx + (it).dx);                                  \
                k5_load_cell(L.cells + (it).cell, (it).v, (it).u);                                  \
            }                                                                                       \
        }                                                                                           \
    }
    k5_item cur, nxt, nx2;
    cur.cell = -1; cur.dx = cur.dy = cur.ray = cur.end = cur.u = 0; cur.xalone = 0x7fffffff; cur.v = 0.f; nxt = cur; nx2 = cur;
    int item = wg_x * 16 + wv;
    K5_FETCH(cur, item)
    K5_FETCH(nxt, item + wgs_x * 16)
    for (; item < items; item += wgs_x * 16) {
        K5_FETCH(nx2, item + 2 * wgs_x * 16)
        if (cur.cell >= 0) {
            const int dx = cur.dx, dy = cur.dy;
            const int adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy;
            int first_free = 0x7fffffff, first_occ = 0x7fffffff;
            int lo = 0, hi = 2;
            const bool lone = K5_EXP == 3 || (K5_EXP != 4 && adx != ady && (adx > ady ? adx : ady) >= cur.xalone);     // (K5_EXP 3: every lane takes the lone path -- wrong results; 4: none does)
                // (beyond the step from which the line shares no cell: the table phase)
            if (adx != ady && !lone) {                                     // (a diagonal cell: the quadrant's other class touches it too)
                const bool xm = adx > ady;
                rs_range(start, xm ? (dx > 0 ? 0 : 1) : (dy > 0 ? 2 : 3), xm ? adx : ady, xm ? dy : dx, 0.5f, lo, hi);
            }
            bool mine = true;
            if (lone || hi - lo == 1) { if (cur.end) first_occ = cur.ray; else first_free = cur.ray; }
            else {
                int cls[2], a[2], b[2];
                const int ncls = rs_classes(dx, dy, cls, a, b);
                for (int k = 0; k < ncls; k++) {
                    rs_range(start, cls[k], a[k], b[k], 0.5f, lo, hi);
                    for (int ci = lo; ci < hi; ci++) {
                        const k5_line c = cand[ci];
                        const int h = k5_hit(c, a[k], b[k]);
                        if (h == 1) first_free = min(first_free, c.ray);
                        else if (h == 2) first_occ = min(first_occ, c.ray);
                    }
                }
                mine = min(first_free, first_occ) == cur.ray;              // else another line's lane owns this cell
            }
            if (mine) {
                float v = cur.v;
                int u = cur.u;
                k5_transition(L, v, u, first_free, first_occ, lo_free, lo_occ);
                k5_store_cell(L.cells + cur.cell, v, u);
#if HS_PROB_MODE == 0
                L.prob[cur.cell] = hs_prob_v(v);
#endif
            }
        }
        cur = nxt; nxt = nx2;
    }
#undef K5_FETCH
    if (BUILD && sec_out && (int)blockIdx.x == L.wg0) {                    // (uniform: the level's first workgroup)
        __syncthreads();
        k5_sector_bounds<(K5_LDS_LINES + 1023) / 1024>(byidx_s, n_pts, s_wtot, &s_wsum_all, s_bound, sec_out + lvl * K5_SEC);
    }
#ifdef K5_TIMES
    __syncthreads();                                                       // (the workgroup's last wavefront)
    K5_STAMP(3)
#endif
}

// ---- host side ---------------------------------------------------------------------------------------------------
// the launches of UpdateByScan on the operator's stream; nothing comes back to the host
// gate_in: the device-gated form (k5_gate) -- `pose` is then only a stand-in, and the update indices are advanced by
// hs_update_commit once the host knows that the update took place.  (The cache epoch can live on the host: no launch that reads
// probabilities is ever enqueued between an update and its commit -- the gated form's match is enqueued IN FRONT of its update.)
void hs_update_commit(slamhip_hs *hs)
{
    for (int l = 0; l < hs->n_levels; l++) {
        hs->lv[l].curr_update_index += 3;                                  // :144
        hs->lv[l].curr_cache_index++;                                      // :147
    }
    if (hs->k5_toggle_pending) hs->k5_sec_parity ^= 1;       // (the one-launch form wrote the other record set)
    hs->k5_toggle_pending = false;
}
static bool k5_two_launches() { static const bool v = sh_env_set("SLAMHIP_K5_TWO_LAUNCHES"); return v; }   // (tests: the large-scan path on ordinary scans)
bool hs_update_gateable(slamhip_hs *hs)
{
    static const bool off = sh_env_set("SLAMHIP_HS_NO_GATED_UPDATE");
    return !off && !k5_two_launches() && hs->n_points > 0 && hs->n_points <= K5_LDS_LINES && hs->ctx->timing == 0 && !hs->ctx->mail_off;
}
int32_t hs_update_enqueue(slamhip_hs *hs, const float pose[3], const k5_gate *gate_in)
{
    SH_CHECK_ARG(hs && pose);
    SH_HIP(hipSetDevice(hs->ctx->device));
    slamhip_ctx *ctx = hs->ctx;
    const int n = hs->n_points;
    k5_arg A;
    memset(&A, 0, sizeof(A));
    A.n = hs->n_levels;
    for (int l = 0; l < hs->n_levels; l++) {
        hs_level &L = hs->lv[l];
        A.lv[l].w = L.w; A.lv[l].h = L.h;
        A.lv[l].t = sh_m3x2_mul(sh_m3x2_mul(sh_m3x2_rotation(pose[2]), sh_m3x2_translation(pose[0], pose[1])),
                                sh_m3x2_scale(L.stm));                    // OccGridMap.cs:120-123
        A.lv[l].cells = L.d_cells; A.lv[l].prob = L.d_prob;
        A.lv[l].mark_free = L.curr_update_index + 1;                      // :116
        A.lv[l].mark_occ = L.curr_update_index + 2;                       // :117
    }
    if (n > 0) {
        SH_TRY(hs_flush_scan(hs));
        if (n > hs->cap_lines || !hs->d_k5_hdr) {
            (void)hipFree(hs->d_k5_byidx); (void)hipFree(hs->d_k5_cand); (void)hipFree(hs->d_k5_start); (void)hipFree(hs->d_k5_hdr);
            hs->d_k5_byidx = hs->d_k5_cand = nullptr; hs->d_k5_start = hs->d_k5_hdr = nullptr; hs->cap_lines = 0;
            const int cap = n + n / 4 + 64;
            SH_HIP(hipMalloc(&hs->d_k5_byidx, sizeof(k5_line) * (size_t)cap * HS_MAX_LEVELS));
            SH_HIP(hipMalloc(&hs->d_k5_cand, sizeof(k5_line) * (size_t)cap * HS_MAX_LEVELS));
            SH_HIP(hipMalloc(&hs->d_k5_start, sizeof(int) * (4 * RS_NBUCK + 1) * HS_MAX_LEVELS));
            SH_HIP(hipMalloc(&hs->d_k5_hdr, sizeof(int) * K5_HDR * HS_MAX_LEVELS));
            if (!hs->d_k5_sec) {
                SH_HIP(hipMalloc(&hs->d_k5_sec, sizeof(int) * 2 * HS_MAX_LEVELS * K5_SEC));
                SH_HIP(hipMemsetAsync(hs->d_k5_sec, 0xFF, sizeof(int) * 2 * HS_MAX_LEVELS * K5_SEC, ctx->stream));     // (no record: line count -1)
            }
            hs->cap_lines = cap;
        }
        int cgrid_x = 0;
        sh_timer t(ctx, SLAMHIP_K_HS_UPDATE);
        {   // ONE round of resident workgroups (two per CU: 512), shared out over the levels by the work they hold -- the cells a
            // scan touches, which halve from level to level (the zone around the begin cell is the same on every level: a floor
            // of 1/16 each).  (Round 2 shared them out by cell count with a floor of 1/8: 551 workgroups, i.e. a second round that
            // started when the first drained -- half of the kernel's 35 us.)
            // (every level needs a workgroup on each of the eight XCD sectors its lines are dealt to: at least 8 per level)
            constexpr int wgs = 512;
            double tot = 0.0;
            for (int l = 0; l < hs->n_levels; l++) tot += (double)hs->lv[l].w + (double)hs->lv[l].h;
            int first = 0, left = wgs;
            for (int l = 0; l < hs->n_levels; l++) {
                const int floor_k = wgs / 16;
                int k = (int)((double)wgs * ((double)hs->lv[l].w + (double)hs->lv[l].h) / tot);
                if (k < floor_k) k = floor_k;
                const int must_leave = (hs->n_levels - 1 - l) * floor_k;   // (the levels still to come keep their floor)
                if (k > left - must_leave) k = left - must_leave > 1 ? left - must_leave : 1;
                if (k < 8) k = 8;                                  // (one workgroup per XCD sector at least, whatever the shares)
                A.lv[l].wg0 = first; A.lv[l].wgn = k;
                first += k; left -= k;
            }
            cgrid_x = first;
        }
        const dim3 cgrid(cgrid_x);
        const bool build = n <= K5_LDS_LINES && !k5_two_launches();
        static std::atomic<unsigned long long> attr_set{0};                                             // one bit per device (the attribute is the device's)
        if (!((attr_set.load(std::memory_order_acquire) >> (ctx->device & 63)) & 1ull)) { (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k5_cells<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)k5_lds_bytes(true, K5_LDS_LINES)); attr_set.fetch_or(1ull << (ctx->device & 63), std::memory_order_release); }
        if (!build)      // all levels in every launch (MapRepMultiMap.cs:76)
            hipLaunchKernelGGL(k5_prepare, dim3(hs->n_levels), dim3(1024), 0, ctx->stream, A, (const float2 *)hs->d_pts, n, hs->origin[0],
                               hs->origin[1], hs->cap_lines, (k5_line *)hs->d_k5_byidx, (k5_line *)hs->d_k5_cand, hs->d_k5_start, hs->d_k5_hdr);
        static const bool no_sectors = sh_env_set("SLAMHIP_K5_EQUAL_SECTORS");       // (tuning: the sectors of phase 2 by count, as scans too large for the LDS tables have them)
        hs->k5_toggle_pending = build;
        k5_gate gate;
        memset(&gate, 0, sizeof(gate));
        if (gate_in) {
            if (!build) SH_FAIL(SLAMHIP_ERR_STATE, "the gated update needs the one-launch form");
            gate = *gate_in; gate.on = 1;
            for (int l = 0; l < hs->n_levels; l++) gate.stm[l] = hs->lv[l].stm;
        }
        if (build) {
            const int *sec_in = no_sectors ? nullptr : hs->d_k5_sec + (size_t)hs->k5_sec_parity * HS_MAX_LEVELS * K5_SEC;
            int *sec_out = no_sectors ? nullptr : hs->d_k5_sec + (size_t)(hs->k5_sec_parity ^ 1) * HS_MAX_LEVELS * K5_SEC;
            hipLaunchKernelGGL(k5_cells<true>, cgrid, dim3(1024), k5_lds_bytes(true, n), ctx->stream, A, hs->cap_lines, (const float2 *)hs->d_pts, n,
                               hs->origin[0], hs->origin[1], (const k5_line *)hs->d_k5_byidx, (const k5_line *)hs->d_k5_cand, (const int *)hs->d_k5_start,
                               (const int *)hs->d_k5_hdr, hs->lo_free, hs->lo_occ, sec_in, sec_out, gate);
        } else
            hipLaunchKernelGGL(k5_cells<false>, cgrid, dim3(1024), k5_lds_bytes(false, n), ctx->stream, A, hs->cap_lines, (const float2 *)hs->d_pts, n,
                               hs->origin[0], hs->origin[1], (const k5_line *)hs->d_k5_byidx, (const k5_line *)hs->d_k5_cand, (const int *)hs->d_k5_start,
                               (const int *)hs->d_k5_hdr, hs->lo_free, hs->lo_occ, (const int *)nullptr, (int *)nullptr, gate);
    }
    SH_HIP(hipGetLastError());
#ifdef K5_TIMES
    {
        static thread_local int calls = 0;
        if (n > 0 && ++calls == 12) {
            (void)hipStreamSynchronize(ctx->stream);
            std::vector<unsigned long long> h(1024 * 4);
            (void)hipMemcpyFromSymbol(h.data(), HIP_SYMBOL(g_k5_times), sizeof(unsigned long long) * h.size());
            unsigned long long t0 = ~0ull, t1 = 0;
            for (int i = 0; i < 1024; i++) if (h[i * 4] && h[i * 4 + 3] >= h[i * 4]) { t0 = std::min(t0, h[i * 4]); t1 = std::max(t1, h[i * 4 + 3]); }
            fprintf(stderr, "[k5 times] span %.2f us; per level, first thread of each workgroup, mean (max) us:\n", (double)(t1 - t0) * 0.01);
            std::vector<unsigned long long> hsub(1024 * 8);
            (void)hipMemcpyFromSymbol(hsub.data(), HIP_SYMBOL(g_k5_sub), sizeof(unsigned long long) * hsub.size());
            for (int l = 0; l < hs->n_levels; l++) {
                {   // the table phase in parts, mean over the level's workgroups: start -> barrier 1 -> lines -> prefix a -> prefix b -> scatter -> tables done
                    double part[6] = { 0, 0, 0, 0, 0, 0 }; int cc = 0;
                    for (int i = A.lv[l].wg0; i < A.lv[l].wg0 + A.lv[l].wgn && i < 1024; i++) if (h[i * 4] && hsub[i * 8 + 4] >= h[i * 4]) {
                        unsigned long long prev = h[i * 4];
                        for (int k = 0; k < 5; k++) { part[k] += (double)(hsub[i * 8 + k] - prev) * 0.01; prev = hsub[i * 8 + k]; }
                        part[5] += (double)(h[i * 4 + 1] - prev) * 0.01; cc++;
                    }
                    if (cc) fprintf(stderr, "   level %d table phase: zero+barrier %.2f | lines+reductions+barrier %.2f | prefix a %.2f | prefix b %.2f | scatter+barrier %.2f | alone pass + rest %.2f\n",
                                    l, part[0] / cc, part[1] / cc, part[2] / cc, part[3] / cc, part[4] / cc, part[5] / cc);
                }
                double acc[3] = { 0, 0, 0 }, mx[3] = { 0, 0, 0 }, end = 0, endmx = 0, st = 0; int c = 0;
                for (int i = A.lv[l].wg0; i < A.lv[l].wg0 + A.lv[l].wgn && i < 1024; i++) if (h[i * 4] && h[i * 4 + 3] >= h[i * 4]) {
                    for (int k = 0; k < 3; k++) { const double d = (double)(h[i * 4 + k + 1] - h[i * 4 + k]) * 0.01; acc[k] += d; mx[k] = std::max(mx[k], d); }
                    const double e = (double)(h[i * 4 + 3] - t0) * 0.01; end += e; endmx = std::max(endmx, e); st += (double)(h[i * 4] - t0) * 0.01; c++;
                }
                {   // per XCD sector of the level (workgroup w of the level draws sector w % 8): mean time beyond the zone
                    fprintf(stderr, "   level %d, beyond + drain per sector:", l);
                    for (int x = 0; x < 8; x++) {
                        double a2 = 0; int c2 = 0;
                        for (int i = A.lv[l].wg0 + x; i < A.lv[l].wg0 + A.lv[l].wgn && i < 1024; i += 8) if (h[i * 4] && h[i * 4 + 3] >= h[i * 4]) { a2 += (double)(h[i * 4 + 3] - h[i * 4 + 2]) * 0.01; c2++; }
                        fprintf(stderr, " %.1f", c2 ? a2 / c2 : 0.0);
                    }
                    fprintf(stderr, "\n");
                }
                if (c) fprintf(stderr, "   level %d (%d workgroups): start +%.2f | tables %.2f (%.2f) | zone %.2f (%.2f) | beyond + drain %.2f (%.2f) | end +%.2f (%.2f)\n",
                               l, c, st / c, acc[0] / c, mx[0], acc[1] / c, mx[1], acc[2] / c, mx[2], end / c, endmx);
            }
        }
    }
#endif
    if (!gate_in) hs_update_commit(hs);
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_update_by_scan(slamhip_hs *hs, const float pose[3])
{
    SH_CHECK_ARG(hs);
    sh_mail_guard lock(hs->ctx);
    SH_TRY(hs_update_enqueue(hs, pose));
    SH_TRY(sh_publish(hs->ctx, nullptr, 0));
    return sh_host_wait(hs->ctx);
}
