// hs_render.h -- the render of stored scans, ONE text for its two units: K20 (hs_render.hip), which draws into the levels of the window, and
// K25 (hs_render_world.hip), which draws into the whole world behind it.  Three sections.  Host and device: the line
// OccGridMap.UpdateByScan draws for one scan point under a bound given as a policy, the steps of that line that fall into a rectangle of
// cells, and the two state transitions of a cell.  Device: the boxes kernel and the body of the block kernel -- the units add where a
// cell of a block lives and which blocks there are.  Host: the refusals, the staging of a chunk of scans, the frame that walks a range
// in chunks, and the walk of one line that the two hooks (slamhip_debug_render, slamhip_debug_render_world) define the result by.
// Definition: include/slamhip.h (slamhip_hs_render, slamhip_hs_render_world).  K5 (hs_update.hip) keeps its own copy of the line-making
// and of the transitions: DESIGN.md section 4 "K20" says why; the GPU tests hold the two to == on every cell.
#pragma once
#include "hs_blocks.h"
#include "hs_scans.h"
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

// The bound of a line's begin and end cell, a policy with ok(x, y): a level's w x h, beyond which the line is dropped (:158-161) -- K20 --
// or the world bound, +-HS_WORLD_BOUND cells of window cell (0, 0) on the unbounded grid of the world, beyond which the callers REFUSE
// the whole render (`refuses`) -- K25.  Under either a cell beyond the bound makes the line not valid here.
#define HS_WORLD_BOUND (1 << 20)
__host__ __device__ static inline bool hs_world_cell_ok(int x, int y)
{
    return (x >= -HS_WORLD_BOUND) & (x <= HS_WORLD_BOUND) & (y >= -HS_WORLD_BOUND) & (y <= HS_WORLD_BOUND);
}
struct hs_bound_level {
    static constexpr bool refuses = false;
    int w, h;
    __host__ __device__ __forceinline__ bool ok(int x, int y) const { return (x >= 0) & (y >= 0) & (x < w) & (y < h); }
};
struct hs_bound_world {
    static constexpr bool refuses = true;
    __host__ __device__ __forceinline__ bool ok(int x, int y) const { return hs_world_cell_ok(x, y); }
};

// the line to the end point (px, py) under the bound `in`; *ex, *ey: its end cell, whether the line is valid or not.  rintf is right for
// the world's negative coordinates as it is; under the world bound |dx|, |dy| <= 2^21.
template <class Bound>
__host__ __device__ static inline hs_line hs_line_make(float px, float py, const sh_m3x2 &t, int bx, int by, const Bound &in, int *ex_out, int *ey_out)
{
    float exf, eyf;
    sh_v2_transform(px, py, t, &exf, &eyf);                                // :133
    const int ex = sh_f2i(rintf(exf)), ey = sh_f2i(rintf(eyf));            // :134
    const bool same = (bx == ex) & (by == ey);                             // :137
    const bool b_ok = in.ok(bx, by), e_ok = in.ok(ex, ey), inside = b_ok & e_ok;   // :158-161
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

// ---- what a launch is given: the part of the argument K20 and K25 share (k20_arg, k25_arg: { hs_render_args P; <levels> lv[]; ...; bound(l) }) ----
// The record of a (scan, level), in cells of the level (K25: window-frame cells): the begin cell, the box of the begin cell and the valid
// end cells, the number of valid lines and the largest da; nv == 0: no valid line, the rest is not read; nv < 0: a cell beyond a bound
// that refuses.  Two layouts, a template parameter of the kernels: K25's, which its host reads back, and K20's narrow one -- under a
// level's bound every value of a valid line is below 32768 and nobody asks for da (DESIGN.md section 4 "K20" has the two figures
// that keep it: every tile reads every scan's record).
struct hs_box {
    int x0, y0, x1, y1, bx, by, nv, da;
    __device__ void set(int x0_, int y0_, int x1_, int y1_, int bx_, int by_, int nv_, int da_) { x0 = x0_; y0 = y0_; x1 = x1_; y1 = y1_; bx = bx_; by = by_; nv = nv_; da = da_; }
};
struct hs_box16 {
    short x0, y0, x1, y1, bx, by; int nv;
    __device__ void set(int x0_, int y0_, int x1_, int y1_, int bx_, int by_, int nv_, int) { x0 = (short)x0_; y0 = (short)y0_; x1 = (short)x1_; y1 = (short)y1_; bx = (short)bx_; by = (short)by_; nv = nv_; }
};
static_assert(sizeof(hs_box) == 32 && sizeof(hs_box16) == 16, "the records the kernels and the host read");
struct hs_render_level { int w, h; slamhip_cell *cells; float *prob; int base; };  // the window on this level; base: the level's update index in front of the launch's first scan
template <class Box>
struct hs_render_args {
    int n_levels, n_scans, keep; float lo_free, lo_occ;
    const float2 *pool; const k20_scan *scans; const sh_m3x2 *mats; Box *boxes;        // mats, boxes: [scan][level]
};

// ---- device side -----------------------------------------------------------------------------------------------------------------------
#define HS_RENDER_LANES 256
#define HS_RENDER_NONE 0xFFFFFFFFu

// A wavefront per (scan, level): the scan's box under the bound.  No line record is ever written to memory: the block kernel makes a
// line again from its point and matrix.  (Under a level's bound nothing refuses and a valid line is at most 32767 cells long: K20 reads
// neither nv < 0 nor da.)
template <class Arg>
__global__ void __launch_bounds__(64) hs_render_boxes(const Arg A)
{
    const auto &P = A.P;
    const int k = (int)blockIdx.x / P.n_levels, lvl = (int)blockIdx.x - k * P.n_levels, lane = threadIdx.x;
    const auto in = A.bound(lvl);
    typedef decltype(A.bound(lvl)) Bound;
    const k20_scan S = P.scans[k];
    const sh_m3x2 M = P.mats[(size_t)k * P.n_levels + lvl];
    int bx, by;
    hs_line_begin(S.ox, S.oy, M, &bx, &by);
    int x0 = 0x7fffffff, y0 = 0x7fffffff, x1 = -0x7fffffff, y1 = -0x7fffffff, nv = 0, da = 0;
    int far = (Bound::refuses && S.n > 0 && !in.ok(bx, by)) ? 1 : 0;       // (a scan of 0 points draws nothing: its begin cell is not asked)
    for (int i = lane; i < S.n; i += 64) {
        const float2 p = P.pool[S.off + i];
        int ex, ey;
        const hs_line ln = hs_line_make(p.x, p.y, M, bx, by, in, &ex, &ey);
        if (Bound::refuses && !in.ok(ex, ey)) far = 1;
        if (ln.flags & 1) { x0 = min(x0, ex); y0 = min(y0, ey); x1 = max(x1, ex); y1 = max(y1, ey); nv++; da = max(da, ln.da); }
    }
    for (int off = 32; off > 0; off >>= 1) {
        x0 = min(x0, __shfl_xor(x0, off, 64)); y0 = min(y0, __shfl_xor(y0, off, 64));
        x1 = max(x1, __shfl_xor(x1, off, 64)); y1 = max(y1, __shfl_xor(y1, off, 64));
        nv += __shfl_xor(nv, off, 64); da = max(da, __shfl_xor(da, off, 64)); far |= __shfl_xor(far, off, 64);
    }
    if (lane == 0) {
        const bool any = nv && !far;                                       // (else an empty box; under a level's bound the begin cell of a valid line lies inside the level)
        P.boxes[(size_t)k * P.n_levels + lvl].set(any ? min(x0, bx) : 1, any ? min(y0, by) : 1, any ? max(x1, bx) : 0, any ? max(y1, by) : 0, bx, by, far ? -1 : nv, da);
    }
}

// The body of a block kernel: a workgroup of HS_RENDER_LANES lanes on a block of S x S cells of level `lvl` whose first cell is
// (x0, y0) and of which the rectangle [x0, x1] x [y0, y1] is drawn into (K20: the tile clipped to the level; K25: the whole block).
// at(c, &cell, &prob) says where cell c = row * S + column of the block and its probability live; false: nowhere -- such a cell is
// neither read nor stored.  The block's cells (value, update index) stay in LDS for the whole launch; the scans pass over it IN ORDER.
// A scan whose box misses the rectangle costs one uniform test.  Otherwise a lane per line clips its line to the rectangle
// (hs_line_clip: one interval of steps, integers only) and leaves, per step, key = line index << 1 | (1 for the line's end cell) in
// the cell's scratch word by an LDS atomic min, and for an end cell a bit in the block's "ended in" words by an LDS atomic or.  (Two
// atomic mins, the smallest crossing and the smallest ending index, would cost a second word per cell and a second atomic per step.
// The smallest key tells which kind of line touched the cell FIRST, which is all the free transition asks; the bit tells whether the
// occupied transition takes place at all.)  Behind a barrier a lane per cell applies hs_cell_transition with that scan's marks and
// rests the scratch; behind another the next scan follows.  At the end every cell of the block is stored ONCE, with its probability.
// No global atomic, no wait on another workgroup: a cell has one writer.
template <int S, class Box, class Bound, class Cells>
__device__ static __forceinline__ void hs_render_block(const hs_render_args<Box> &P, int lvl, int base, const Bound &in, const Cells &at, int x0, int y0, int x1, int y1)
{
    __shared__ float val_s[S * S];
    __shared__ int idx_s[S * S];
    __shared__ unsigned key_s[S * S];
    __shared__ unsigned end_s[(S * S + 31) / 32];
    const int tid = threadIdx.x;
    for (int c = tid; c < S * S; c += HS_RENDER_LANES) {
        slamhip_cell cell = hs_reset_cell();
        slamhip_cell *pc; float *pp;
        if (P.keep && at(c, &pc, &pp)) cell = *pc;
        val_s[c] = cell.value; idx_s[c] = cell.update_index; key_s[c] = HS_RENDER_NONE;
    }
    if (tid < (S * S + 31) / 32) end_s[tid] = 0u;
    bool dirty = !P.keep;                                                  // (uniform: is the block to be stored?)
    __syncthreads();
    for (int k = 0; k < P.n_scans; k++) {
        const Box B = P.boxes[(size_t)k * P.n_levels + lvl];               // (uniform)
        if ((Bound::refuses ? B.nv <= 0 : B.nv == 0) || B.x1 < x0 || B.x0 > x1 || B.y1 < y0 || B.y0 > y1) continue;
        const k20_scan Sc = P.scans[k];
        const sh_m3x2 M = P.mats[(size_t)k * P.n_levels + lvl];
        const int bx = B.bx, by = B.by;
        int touched = 0;
        for (int i = tid; i < Sc.n; i += HS_RENDER_LANES) {
            const float2 p = P.pool[Sc.off + i];
            int ex, ey;
            const hs_line ln = hs_line_make(p.x, p.y, M, bx, by, in, &ex, &ey);
            // hs_line_clip's 32-bit proof asks da <= HS_LINE_MAX_DA: K25's host has refused a longer line; under a level's bound (at most
            // 32768 cells a side) the test is vacuous, and so is nv < 0 above -- neither is compiled where nothing refuses
            if (!(ln.flags & 1) || (Bound::refuses && ln.da > HS_LINE_MAX_DA)) continue;
            if (max(bx, ex) < x0 || min(bx, ex) > x1 || max(by, ey) < y0 || min(by, ey) > y1) continue;     // (the line's own box misses the rectangle)
            const bool mx = (ln.flags & 2) != 0;
            const int smaj = ((ln.flags >> 2) & 3) - 1, smin = ln.sdb < 0 ? -1 : 1, da = ln.da, db = ln.sdb < 0 ? -ln.sdb : ln.sdb;
            const int bM = mx ? bx : by, bm = mx ? by : bx;
            const int tM0 = mx ? x0 : y0, tM1 = mx ? x1 : y1, tm0 = mx ? y0 : x0, tm1 = mx ? y1 : x1;
            const int A0 = smaj > 0 ? tM0 - bM : bM - tM1, A1 = smaj > 0 ? tM1 - bM : bM - tM0;
            const int B0 = smin > 0 ? tm0 - bm : bm - tm1, B1 = smin > 0 ? tm1 - bm : bm - tm0;
            int i0, i1;
            hs_line_clip(da, db, A0, A1, B0, B1, &i0, &i1);
            if (i0 > i1) continue;
            touched = 1;
            const int e = da / 2 + i0 * db;                                // (< 2^31: hs_line_clip)
            int m = e / da, r = e - m * da;
            for (int s = i0; s <= i1; s++) {
                const int cM = bM + smaj * s, cm = bm + smin * m;
                const int cx = (mx ? cM : cm) - x0, cy = (mx ? cm : cM) - y0;
                if ((unsigned)cx < (unsigned)S && (unsigned)cy < (unsigned)S) {    // (always, by hs_line_clip: the LDS arrays' own guard)
                    const int c = cy * S + cx;
                    if (s == da) { atomicMin(&key_s[c], ((unsigned)i << 1) | 1u); atomicOr(&end_s[c >> 5], 1u << (c & 31)); }
                    else atomicMin(&key_s[c], (unsigned)i << 1);
                }
                r += db;
                if (r >= da) { r -= da; m++; }                             // :231-235
            }
        }
        if (!__syncthreads_or(touched)) continue;                          // (uniform; no lane has written anything)
        dirty = true;
        const int mark_free = base + 3 * k + 1, mark_occ = base + 3 * k + 2;          // :116-117, :144
        for (int c = tid; c < S * S; c += HS_RENDER_LANES) {
            const unsigned key = key_s[c];
            if (key == HS_RENDER_NONE) continue;
            const bool ended = (end_s[c >> 5] >> (c & 31)) & 1u;
            float v = val_s[c]; int u = idx_s[c];
            // first touched by a crossing line: the free transition, then the occupied one if a line ends here at all;
            // first touched by an ending line: the occupied transition alone
            const bool cross_first = !(key & 1u);
            hs_cell_transition(v, u, mark_free, mark_occ, cross_first ? 0 : 0x7fffffff, cross_first ? (ended ? 1 : 0x7fffffff) : 0, P.lo_free, P.lo_occ);
            val_s[c] = v; idx_s[c] = u; key_s[c] = HS_RENDER_NONE;
            if (ended) atomicAnd(&end_s[c >> 5], ~(1u << (c & 31)));       // (this cell's own bit: the word's other cells belong to other lanes)
        }
        __syncthreads();
    }
    if (!dirty) return;
    for (int c = tid; c < S * S; c += HS_RENDER_LANES) {
        slamhip_cell *pc; float *pp;
        if (!at(c, &pc, &pp)) continue;
        slamhip_cell cell; cell.update_index = idx_s[c]; cell.value = val_s[c];
        *pc = cell;
#if HS_PROB_MODE == 0
        *pp = hs_prob_v(cell.value);
#endif
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------
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

// k20_check for a render on the handle's store and levels, and what such a render refuses for the reference's cache
static inline int32_t hs_render_check(const char *who, const slamhip_hs *hs, int32_t first, int32_t last, const float *poses, int32_t flags)
{
    int base[HS_MAX_LEVELS];
    for (int l = 0; l < hs->n_levels; l++) base[l] = hs->lv[l].curr_update_index;
    return k20_check(who, first, last, hs->scn ? (int)hs->scn->recs.size() : 0, poses, flags, base, hs->n_levels);
}
static inline int32_t hs_render_check_cache(const char *who, const slamhip_hs *hs)
{
    if (hs->ref_cache)
        SH_FAIL(SLAMHIP_ERR_INVALID, "%s: the reference's cache is on (slamhip_hs_set_reference_cache) -- its literal stale entries have "
                "no meaning under an operation the reference lacks; turn it off first", who);
    return SLAMHIP_OK;
}

// The frame of a render behind its refusals.  _begin: the blocking call opened, the store's unit, the range cut into chunks, and the
// fields of the launch argument A that come from the handle.  _lay: the blocks as they lie with `more` bytes of the unit's own behind
// the boxes -- records | matrices | boxes | more in device memory (boxes and more on 32-byte boundaries); the pinned block holds the
// records and matrices, and with `mirror` the rest as well (K25 reads the boxes back into it and sends its jobs from it).
struct hs_render_frame {
    slamhip_hs *hs; hs_scans *g; const char *who; const float *poses; int first, N, NL, chunk; bool keep;
    size_t scan_bytes, in_bytes, box_bytes;
};
template <class Arg>
static inline int32_t hs_render_begin(hs_render_frame &F, Arg &A, const char *who, slamhip_hs *hs, int32_t first, int32_t last, const float *poses, int32_t flags)
{
    SH_TRY(hs_call_begin(hs));
    SH_TRY(hs_unit<&slamhip_hs::scn>(hs));
    F.hs = hs; F.g = hs->scn; F.who = who; F.poses = poses; F.first = first; F.N = last - first; F.NL = hs->n_levels;
    F.keep = (flags & SLAMHIP_RENDER_KEEP) != 0;
    F.chunk = std::min(k20_chunk(), std::max(F.N, 1));
    F.scan_bytes = sizeof(k20_scan) * (size_t)F.chunk;
    F.in_bytes = (F.scan_bytes + sizeof(sh_m3x2) * (size_t)F.chunk * F.NL + 31) & ~(size_t)31;
    F.box_bytes = sizeof(*A.P.boxes) * (size_t)F.chunk * F.NL;
    memset(&A, 0, sizeof(A));
    A.P.n_levels = F.NL; A.P.lo_free = hs->lo_free; A.P.lo_occ = hs->lo_occ; A.P.pool = F.g->d_pool;
    for (int l = 0; l < F.NL; l++) { const hs_level &L = hs->lv[l]; A.lv[l].w = L.w; A.lv[l].h = L.h; A.lv[l].cells = L.d_cells; A.lv[l].prob = L.d_prob; }
    return SLAMHIP_OK;
}
template <class Box>
static inline int32_t hs_render_lay(const hs_render_frame &F, hs_render_args<Box> &P, size_t more, bool mirror)
{
    hs_scans *g = F.g;
    const size_t all = F.in_bytes + F.box_bytes + more;
    SH_TRY(g->d_in.grow(all, F.who));
    SH_TRY(g->h_io.grow(mirror ? all : F.in_bytes, F.who));
    P.scans = (const k20_scan *)g->d_in.p; P.mats = (const sh_m3x2 *)(g->d_in + F.scan_bytes); P.boxes = (Box *)(g->d_in + F.in_bytes);
    return SLAMHIP_OK;
}

// chunk [c0, c0 + nc) of the range staged: its records and per-level matrices into the pinned block, the copy, the boxes made
template <class Arg>
static inline int32_t hs_render_stage(const hs_render_frame &F, Arg &A, int c0, int nc)
{
    k20_scan *hr = (k20_scan *)F.g->h_io.p;
    sh_m3x2 *hm = (sh_m3x2 *)(F.g->h_io + F.scan_bytes);
    for (int k = 0; k < nc; k++) {
        hr[k] = F.g->recs[(size_t)(F.first + c0 + k)];
        for (int l = 0; l < F.NL; l++) hm[(size_t)k * F.NL + l] = k20_matrix(F.poses + 3 * (size_t)(c0 + k), F.hs->lv[l].stm);
    }
    A.P.n_scans = nc;
    hipStream_t st = F.hs->ctx->stream;
    SH_HIP(hipMemcpyAsync(F.g->d_in, F.g->h_io, F.scan_bytes + sizeof(sh_m3x2) * (size_t)nc * F.NL, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(hs_render_boxes<Arg>, dim3((unsigned)(nc * F.NL)), dim3(64), 0, st, A);
    SH_HIP(hipGetLastError());
    return SLAMHIP_OK;
}

// The range drawn chunk by chunk: each chunk staged, launch(c0) -- the unit's block kernel on A -- and the call's wait (the staging
// block is the next chunk's; a wait that times out poisons the context).  A later chunk is a KEEP render of its own.  The indices as
// they will stand are kept beside the handle's: the handle's own change only behind a launch that went into the stream (a call
// refused or failed before that leaves everything as it was).
template <class Arg, class Launch>
static inline int32_t hs_render_chunks(const hs_render_frame &F, Arg &A, Launch launch)
{
    slamhip_hs *hs = F.hs;
    int cur_ui[HS_MAX_LEVELS], cur_ci[HS_MAX_LEVELS];
    for (int l = 0; l < F.NL; l++) { cur_ui[l] = F.keep ? hs->lv[l].curr_update_index : 0; cur_ci[l] = F.keep ? hs->lv[l].curr_cache_index : 0; }
    for (int c0 = 0; c0 < F.N || c0 == 0; c0 += F.chunk) {                 // (N == 0 without KEEP: one launch that clears)
        const int nc = std::min(F.chunk, F.N - c0);
        A.P.n_scans = nc; A.P.keep = (F.keep || c0 > 0) ? 1 : 0;
        for (int l = 0; l < F.NL; l++) A.lv[l].base = cur_ui[l];
        if (nc > 0) SH_TRY(hs_render_stage(F, A, c0, nc));
        SH_TRY(launch(c0));
        for (int l = 0; l < F.NL; l++) {                                   // :144, :147 per scan; without KEEP from 0, as slamhip_hs_reset leaves them
            cur_ui[l] += 3 * nc; cur_ci[l] += nc;
            hs->lv[l].curr_update_index = cur_ui[l]; hs->lv[l].curr_cache_index = cur_ci[l];
        }
        SH_TRY(hs_call_finish(hs));
    }
    return SLAMHIP_OK;
}

// ---- the two hooks' definition, line by line as the reference walks (UpdateLineBresenhami :155-190, Bresenham2D :220-239) -- NOT the
// closed form the kernels clip by: the two are two statements of one rule ---------------------------------------------------------------
static inline int32_t hs_render_check_offsets(const char *who, const float *xy, const int32_t *offsets, int N)
{
    if (!N) return SLAMHIP_OK;
    if (offsets[0] != 0) SH_FAIL(SLAMHIP_ERR_INVALID, "%s: offsets[0] = %d must be 0", who, offsets[0]);
    for (int k = 0; k < N; k++)
        if (offsets[k + 1] < offsets[k]) SH_FAIL(SLAMHIP_ERR_INVALID, "%s: offsets[%d] = %d below offsets[%d] = %d", who, k + 1, offsets[k + 1], k, offsets[k]);
    SH_CHECK_ARG(xy || offsets[N] == 0);
    return SLAMHIP_OK;
}

// one valid line from (bx, by) to (ex, ey) over the row-major rectangle C of width w whose first cell is (X0, Y0), which holds both
static inline void hs_line_walk(slamhip_cell *C, int w, int X0, int Y0, const hs_line &ln, int bx, int by, int ex, int ey, int mark_free, int mark_occ, float lo_free, float lo_occ)
{
    const bool mx = (ln.flags & 2) != 0;
    const int smaj = ((ln.flags >> 2) & 3) - 1, smin = sh_sign(ln.sdb), da = ln.da, db = ln.sdb < 0 ? -ln.sdb : ln.sdb;
    const int step_a = mx ? smaj : smaj * w, step_b = mx ? smin * w : smin;
    int offset = (by - Y0) * w + (bx - X0), error_b = da / 2;              // :175-185
    for (int s = 0; s < da; s++) {                                         // :222-238: da free cells, the end cell excluded
        slamhip_cell &c = C[offset];
        if (c.update_index < mark_free) { c.value += lo_free; c.update_index = mark_free; }     // :192-199
        offset += step_a;
        error_b += db;
        if (error_b >= da) { offset += step_b; error_b -= da; }                                 // :231-235
    }
    slamhip_cell &c = C[(ey - Y0) * w + (ex - X0)];                        // :187-189
    if (c.update_index < mark_occ) {                                       // :201-218
        if (c.update_index == mark_free) c.value -= lo_free;
        if (c.value < 50.0f) c.value += lo_occ;
        c.update_index = mark_occ;
    }
}
