// hs_trace.hip -- K8, the beam trace of HectorSLAM: what the map of one level holds ALONG every beam of the scan, at many poses
// (slamhip_hs_trace, slamhip_debug_trace_lines, slamhip_debug_trace_cells).  No reference counterpart.  Definition:
// include/slamhip.h (slamhip_trace_beam); the arithmetic host and device share: hs_trace.h.
//
// The class map is K7's (hs_lattice.hip), re-packed on every call: k7_pack for the window, the memset and k7_pack_world for the
// world, whose rectangle R starts at cell (x0, y0) of the window's frame; the window is the case R = the window, (x0, y0) = (0, 0).
// ONE launch then, k8_trace.  The grid is poses x beam chunks, flattened with the chunk running fastest (a pose count of 65536 is
// more than a grid's second dimension takes); a workgroup of 256 lanes owns K8_LANES consecutive beams of one pose, a beam per lane.
//  * Lane 0 forms the pose's transform t (hs_trace_transform: the text the debug hook runs) into LDS; every lane then forms its
//    beam's line.
//  * The rectangle of the class map the workgroup's beams can touch -- the bounding box of b and of the chunk's e (a line stays in
//    the box of its ends), clipped to the map, in whole words -- is staged in LDS when it fits K7_RECT_WORDS (48 KB: three
//    workgroups per compute unit, under the 64 KB of a static allocation); otherwise the SAME loop (k8_walk<false>) reads the
//    packed map from global memory with the map's own extent as its rectangle (K7's LDSR idea, decided per workgroup).  A cell
//    outside the rectangle lies outside the map by construction, and the padding bits of a row's last word are zero, so the
//    out-of-map test is the rectangle test and is exact on both paths.
//  * The walk is Bresenham2D's own recurrence (hs_trace_walk): an add and a compare per cell, no division, K8_AHEAD steps at a
//    time with their look-ups issued together.  A lane stops at the first occupied cell; end_class then costs one more look-up.
//    Lanes of a wavefront walk beams of unequal length: the wavefront runs as long as its longest beam that meets nothing.
//  * The summary: ballots and one wave sum, the wavefronts' counts through LDS, then ONE set of agent-scope atomic adds per
//    workgroup into the pose's record, which a memset zeroed in-stream ahead of the launch.
#include "hs_blocks.h"
#include "hs_lattice.h"
#include "hs_trace.h"

#define K8_LANES 256
#define K8_AHEAD 8                         // steps of a walk whose look-ups are issued together
#define HS_TRACE_MAX_POSES 65536
#define HS_TRACE_LOG2_MAX_BEAMS 20         // B * n_points with per-beam records (24 MB of them)

static_assert(sizeof(slamhip_trace_beam) == 24 && sizeof(slamhip_trace_summary) == 32, "the records of include/slamhip.h");

struct k8_arg {
    const float2 *pts; int n; float ox, oy;   // the scan and its origin
    const float *poses; int chunks;        // B x 3, window frame; workgroups per pose
    const uint32_t *cls; int w, h, wpr;    // the packed class map: the level's, or R's
    int x0, y0;                            // the map's first cell in the window's frame: (0, 0), or R's origin
    float stm;
    slamhip_trace_summary *sums; slamhip_trace_beam *beams;   // beams: nullptr, or B x n records
};

// the class bits of cell (x, y), coordinates relative to the rectangle's first cell, which is rwc x rh cells in rows of rwpr words.
// LDSR: the rectangle is `rect` in LDS; otherwise the whole packed map in global memory.  A cell outside reads word 0 and is class 0.
template <bool LDSR>
__device__ static __forceinline__ uint32_t k8_class(const uint32_t *__restrict__ gmap, const uint32_t *rect, int x, int y, int rwc, int rh, int rwpr)
{
    const bool in = (unsigned)x < (unsigned)rwc && (unsigned)y < (unsigned)rh;
    const int o = in ? y * rwpr + (x >> 4) : 0;
    uint32_t word;
    if constexpr (LDSR) word = rect[o];
    else word = gmap[o];
    return in ? (word >> ((x & 15) * 2)) & 3u : 0u;
}

// the record of one walked beam (l.da >= 1); (fx, fy): the rectangle's first cell in the window's frame
template <bool LDSR>
__device__ static __forceinline__ slamhip_trace_beam k8_walk(const hs_trace_line l, const uint32_t *__restrict__ gmap, const uint32_t *rect,
                                                             int fx, int fy, int rwc, int rh, int rwpr)
{
    slamhip_trace_beam r;
    r.da = l.da; r.first = -1; r.n_unknown = 0; r.end_class = 0; r.hx = 0; r.hy = 0;
    hs_trace_walk w = hs_trace_walk_begin(l);
    uint32_t c = 0;
    // K8_AHEAD steps at a time: their cells first, then their look-ups -- none waits for the class of the one before, which is what
    // a lane's time went into (one L2 round trip per cell) -- then the classes in order.  Steps past da repeat e and are not read.
    for (bool done = false; !done;) {                                      // (w.a goes up by K8_AHEAD per turn and ends at da <= 32768)
        int xs[K8_AHEAD], ys[K8_AHEAD];
        uint32_t cs[K8_AHEAD];
        const int a0 = w.a;
#pragma unroll
        for (int u = 0; u < K8_AHEAD; u++) {
            xs[u] = w.x; ys[u] = w.y;
            if (w.a < w.da) hs_trace_walk_next(w);
        }
#pragma unroll
        for (int u = 0; u < K8_AHEAD; u++) cs[u] = k8_class<LDSR>(gmap, rect, xs[u] - fx, ys[u] - fy, rwc, rh, rwpr);
#pragma unroll
        for (int u = 0; u < K8_AHEAD; u++) {
            if (done || a0 + u > l.da) continue;
            c = cs[u];
            if (c == 1u) { r.first = a0 + u; r.hx = xs[u]; r.hy = ys[u]; done = true; }
            else r.n_unknown += (c == 0u);
        }
        if (a0 + K8_AHEAD > l.da) done = true;                             // (step da has been read; else w stands at step a0 + K8_AHEAD)
    }
    if (r.first < 0) r.end_class = (int32_t)c;                             // (the last cell looked at was e)
    else if (r.first == l.da) r.end_class = 1;
    else r.end_class = (int32_t)k8_class<LDSR>(gmap, rect, l.ex - fx, l.ey - fy, rwc, rh, rwpr);
    return r;
}

__global__ void __launch_bounds__(K8_LANES) k8_trace(const k8_arg A)
{
    __shared__ uint32_t rect_s[K7_RECT_WORDS];
    __shared__ sh_m3x2 t_s;
    __shared__ int bb_s[4];
    __shared__ int red_s[K8_LANES / 64][8];
    const int tid = threadIdx.x;
    const int pose = blockIdx.x / A.chunks, chunk = blockIdx.x - pose * A.chunks;
    if (tid == 0) t_s = hs_trace_transform(A.stm, A.poses[3 * pose], A.poses[3 * pose + 1], A.poses[3 * pose + 2]);
    if (tid < 4) bb_s[tid] = (tid & 1) ? INT_MIN : INT_MAX;                // {min x, max x, min y, max y}
    __syncthreads();
    const int i = chunk * K8_LANES + tid;
    const bool have = i < A.n;
    hs_trace_line l = { 0, 0, 0, 0, -1 };
    if (have) {
        const float2 p = A.pts[i];
        l = hs_trace_line_of(t_s, A.ox, A.oy, p.x, p.y);
    }
    const bool walked = have && l.da >= 1;
    // the bounding box of the chunk's walked lines, in the map's cells (|cell| <= 2^24, -2^28 < x0 <= 0: no overflow)
    if (walked) {
        atomicMin(&bb_s[0], min(l.bx, l.ex) - A.x0); atomicMax(&bb_s[1], max(l.bx, l.ex) - A.x0);
        atomicMin(&bb_s[2], min(l.by, l.ey) - A.y0); atomicMax(&bb_s[3], max(l.by, l.ey) - A.y0);
    }
    __syncthreads();
    // the rectangle of the class map these beams can touch, clipped to the map, in whole words; none: every cell is class 0
    int rx0 = 0, ry0 = 0, rwpr = 0, rh = 0;
    bool in_lds = true;
    if (bb_s[0] <= bb_s[1]) {
        const int x_lo = max(bb_s[0], 0), x_hi = min(bb_s[1], A.w - 1);
        const int y_lo = max(bb_s[2], 0), y_hi = min(bb_s[3], A.h - 1);
        if (x_lo <= x_hi && y_lo <= y_hi) {
            const int w0 = x_lo >> 4;
            rwpr = (x_hi >> 4) - w0 + 1; rh = y_hi - y_lo + 1;
            rx0 = w0 * 16; ry0 = y_lo;
            in_lds = rwpr * rh <= K7_RECT_WORDS;                           // (at most 2^28 cells in rows of whole words: no overflow)
            if (in_lds) {
                const uint32_t *src = A.cls + (size_t)y_lo * A.wpr + w0;
                for (int j = tid; j < rwpr * rh; j += K8_LANES) {
                    const int r = j / rwpr;
                    rect_s[j] = src[(size_t)r * A.wpr + (j - r * rwpr)];
                }
            } else { rx0 = 0; ry0 = 0; rwpr = A.wpr; rh = A.h; }           // the whole packed map, from global memory
        }
    }
    __syncthreads();                                                       // (the rectangle)
    const int rwc = rwpr * 16;                                             // (cells past the map's width in the last word: zero bits)
    slamhip_trace_beam r;
    r.da = l.da; r.first = -1; r.n_unknown = 0; r.end_class = 0; r.hx = 0; r.hy = 0;
    if (walked) {
        if (in_lds) r = k8_walk<true>(l, A.cls, rect_s, A.x0 + rx0, A.y0 + ry0, rwc, rh, rwpr);
        else r = k8_walk<false>(l, A.cls, rect_s, A.x0 + rx0, A.y0 + ry0, rwc, rh, rwpr);
    }
    if (have && A.beams) {
        int2 *o = (int2 *)(A.beams + ((size_t)pose * (size_t)A.n + (size_t)i));    // (24-byte records: 8-byte aligned)
        o[0] = make_int2(r.da, r.first); o[1] = make_int2(r.n_unknown, r.end_class); o[2] = make_int2(r.hx, r.hy);
    }
    // the summary of the workgroup's beams
    const int cnt[6] = { (int)__popcll(__ballot(walked)), (int)__popcll(__ballot(have && l.da == 0)), (int)__popcll(__ballot(have && l.da < 0)),
                         (int)__popcll(__ballot(walked && r.first == r.da)), (int)__popcll(__ballot(walked && r.first >= 0 && r.first < r.da)),
                         (int)__popcll(__ballot(walked && r.first < 0 && r.end_class == 2)) };
    int unk = r.n_unknown;                                                 // (at most 32769 per lane: a workgroup's sum stays below 2^24)
    for (int off = 32; off > 0; off >>= 1) unk += __shfl_down(unk, off, 64);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 6; k++) red_s[tid >> 6][k] = cnt[k];
        red_s[tid >> 6][6] = unk;
    }
    __syncthreads();
    if (tid < 7) {
        int v = 0;
        for (int wv = 0; wv < K8_LANES / 64; wv++) v += red_s[wv][tid];
        slamhip_trace_summary *S = A.sums + pose;
        if (tid < 6) { if (v) __hip_atomic_fetch_add(&S->n_walked + tid, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
        else if (v) __hip_atomic_fetch_add((unsigned long long *)&S->unknown_cells, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------
// What a trace needs, made by the first one and kept: hs->trc, the blocks of a pose batch (hs_blocks.h) -- B summaries, then the
// beam records.
int32_t hs_trc_check(int n_levels, int32_t level, int32_t B, int32_t world, bool want_beams, int n_points, bool scan_is_set)
{
    if (level < 0 || level >= n_levels) SH_FAIL(SLAMHIP_ERR_INVALID, "trace: level %d of %d", level, n_levels);
    return hs_pose_batch_check("trace", B, HS_TRACE_MAX_POSES, world, "per-beam", want_beams, n_points, scan_is_set, HS_TRACE_LOG2_MAX_BEAMS);
}

extern "C" int32_t slamhip_hs_trace(slamhip_hs *hs, int32_t level, const float *poses, int32_t B, int32_t world,
                                    slamhip_trace_summary *out_summaries, slamhip_trace_beam *out_beams)
{
    SH_CHECK_ARG(hs && poses && out_summaries);
    SH_TRY(hs_trc_check(hs->n_levels, level, B, world, out_beams != nullptr, hs->n_points, true));
    const int n = hs->n_points;
    SH_TRY(hs_call_begin(hs));
    int chunks;
    SH_TRY(hs_pose_batch_chunks("trace", B, n, K8_LANES, &chunks));
    hs_class_map M;
    SH_TRY(hs_lat_pack_prepare(hs, level, world != 0, &M));                // (the world's plan refuses before anything is launched)
    SH_TRY(hs_unit<&slamhip_hs::trc>(hs));
    hs_pose_batch *tr = hs->trc;
    const size_t sum_bytes = sizeof(slamhip_trace_summary) * (size_t)B;
    const size_t beam_bytes = out_beams ? sizeof(slamhip_trace_beam) * (size_t)B * n : 0;   // (both multiples of 8)
    SH_TRY(hs_pose_batch_begin(hs, tr, "trace", poses, B, sum_bytes, beam_bytes));
    SH_TRY(hs_lat_pack_enqueue(hs, level, world != 0, &M));
    k8_arg A;
    A.pts = hs->d_pts; A.n = n; A.ox = hs->origin[0]; A.oy = hs->origin[1];
    A.poses = tr->d_poses; A.chunks = chunks;
    A.cls = M.cls; A.w = M.w; A.h = M.h; A.wpr = M.wpr;
    A.x0 = M.x0; A.y0 = M.y0;
    A.stm = hs->lv[level].stm;
    A.sums = (slamhip_trace_summary *)tr->d_out.p;
    A.beams = out_beams ? (slamhip_trace_beam *)(tr->d_out + sum_bytes) : (slamhip_trace_beam *)nullptr;
    hipLaunchKernelGGL(k8_trace, dim3((unsigned)(B * chunks)), dim3(K8_LANES), 0, hs->ctx->stream, A);    // (no timing class of its own)
    SH_HIP(hipGetLastError());
    return hs_pose_batch_finish(hs, tr, sum_bytes, beam_bytes, out_summaries, out_beams);
}

// CPU-side test hooks: hs_trace_line_of and hs_trace_walk, the text the kernel runs
extern "C" int32_t slamhip_debug_trace_lines(float stm, const float pose[3], const float origin[2], const float *xy, int32_t n, int32_t *out)
{
    SH_CHECK_ARG(pose && origin && n >= 0 && ((xy && out) || n == 0));
    const sh_m3x2 t = hs_trace_transform(stm, pose[0], pose[1], pose[2]);
    for (int i = 0; i < n; i++) {
        const hs_trace_line l = hs_trace_line_of(t, origin[0], origin[1], xy[2 * i], xy[2 * i + 1]);
        out[5 * i] = l.bx; out[5 * i + 1] = l.by; out[5 * i + 2] = l.ex; out[5 * i + 3] = l.ey; out[5 * i + 4] = l.da;
    }
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_debug_trace_cells(int32_t bx, int32_t by, int32_t ex, int32_t ey, int32_t *out_xy, int32_t cap, int32_t *out_n)
{
    SH_CHECK_ARG(out_n && cap >= 0 && (out_xy || cap == 0));
    *out_n = 0;
    const int32_t lim = 1 << 24;
    SH_CHECK_ARG(bx > -lim && bx < lim && by > -lim && by < lim && ex > -lim && ex < lim && ey > -lim && ey < lim);
    hs_trace_line l = { bx, by, ex, ey, 0 };
    const int adx = ex < bx ? bx - ex : ex - bx, ady = ey < by ? by - ey : ey - by;
    l.da = adx >= ady ? adx : ady;
    if (l.da < 1 || l.da > SLAMHIP_TRACE_MAX_DA) SH_FAIL(SLAMHIP_ERR_INVALID, "trace cells: da = %d, no walked beam has such a line", l.da);
    *out_n = l.da + 1;
    if (*out_n > cap) SH_FAIL(SLAMHIP_ERR_INVALID, "trace cells: %d cells, room for %d", *out_n, cap);
    hs_trace_walk w = hs_trace_walk_begin(l);
    for (;;) {
        out_xy[2 * w.a] = w.x; out_xy[2 * w.a + 1] = w.y;
        if (w.a >= w.da) break;
        hs_trace_walk_next(w);
    }
    return SLAMHIP_OK;
}
