// hs_mcl.hip -- K13, one particle-filter localisation step on the distance field of HectorSLAM's map: a particle set owned by the hs
// and resident in device memory is moved by odometry with noise, weighed by the scan against K9's field and resampled
// (slamhip_hs_mcl_set, slamhip_hs_mcl_step, slamhip_hs_mcl_get, slamhip_debug_mcl_step).  No reference counterpart.  Definition:
// include/slamhip.h (slamhip_hs_mcl_step); the arithmetic host and device share: hs_mcl.h.
//
// The field is K9's (hs_dfield.hip), built by the functions slamhip_hs_distance_score builds it with (hs_df_field_prepare,
// hs_df_field_enqueue), on every step.  Behind it:
//  * k13_score: a workgroup of four wavefronts copies the scan into LDS once, then each wavefront takes one particle at a time --
//    particle i = 4 * workgroup + wavefront, then on by 4 * workgroups.  Every lane forms the noise, the predicted pose and the
//    transform of ITS wavefront's particle (the same bits in all 64 lanes: nothing is exchanged), the lanes stride the points and
//    gather F, the sum and the ignored count are reduced over the wavefront, lane 0 stores the predicted pose over the particle
//    (in place: no other wavefront reads it) and a_i; min a, cost_min and cost_max go out as one 64-bit agent-scope atomic each
//    per wavefront at the end.
//  * k13_weigh: a lane per particle -- acc', w, h and the scaled integers; nine sums and the key reduced over the wavefront by
//    shuffles, one atomic per wavefront per sum that is not zero.
//  * k13_scan: ONE workgroup of 1024 lanes, the inclusive uint64 scan of w in chunks of 4096 (four consecutive weights per lane,
//    a shuffle scan per wavefront, sixteen wavefront totals through LDS, the carry in a register).  It returns at once when the
//    decision, read from the counters, is not to resample.
//  * k13_resample: a lane per new particle -- the decision again, the tooth of the comb, a binary search over C, the particle
//    copied into the OTHER buffer; anc_k != anc_k-1 counted by ballots (lane 0 of a wavefront searches for tooth k - 1 itself).  A
//    ticket taken per workgroup tells the last one to finish, which stores the summary to pinned memory.
#include "hs_blocks.h"
#include "hs_mcl.h"
#include <algorithm>
#include <stddef.h>
#include <vector>

#define K13_LANES 256
#define K13_SCORE_MAX_BLOCKS 2048          // workgroups of k13_score: beyond that a wavefront takes several particles
#define K13_SCAN_LANES 1024
#define K13_SCAN_CHUNK (4 * K13_SCAN_LANES)
// the counter block, unsigned long long each: the first three start at UINT64_MAX, the others at 0
#define K13_C_MIN_A 0
#define K13_C_KEY 1
#define K13_C_CMIN 2
#define K13_C_CMAX 3
#define K13_C_W 4
#define K13_C_A 5
#define K13_C_Q 6
#define K13_C_SHX 7
#define K13_C_SHY 8
#define K13_C_SHC 9
#define K13_C_SHS 10
#define K13_C_UNPLACED 11
#define K13_C_DISTINCT 12
#define K13_C_TICKET 13
#define K13_CTRS 16

static_assert(sizeof(slamhip_mcl_spec) == 72 && sizeof(slamhip_mcl_summary) == 96, "the records of include/slamhip.h");
static_assert(HS_MCL_MAX_POINTS * sizeof(float2) + 1024 <= 65536, "the scan in LDS");

typedef unsigned long long k13_u64;

struct k13_score_arg {
    const float2 *pts; int n;
    float *part; int N;                    // N x 3, predicted in place
    const k13_u64 *acc; k13_u64 *a;
    float stm; uint32_t r2;
    hs_field E;
    hs_mcl_motion mo;
    k13_u64 *ctr;
};

__global__ void __launch_bounds__(K13_LANES) k13_score(const k13_score_arg A)
{
    extern __shared__ float2 k13_pts_s[];                                  // n points
    const int tid = threadIdx.x, lane = tid & 63;
    for (int j = tid; j < A.n; j += K13_LANES) k13_pts_s[j] = A.pts[j];
    __syncthreads();
    k13_u64 min_a = ~0ull, cmin = ~0ull, cmax = 0ull;
    const int stride = (int)gridDim.x * (K13_LANES / 64);
    for (int i = (int)blockIdx.x * (K13_LANES / 64) + (tid >> 6); i < A.N; i += stride) {   // (uniform over the wavefront)
        hs_mcl_pose p;
        p.x = A.part[3 * i]; p.y = A.part[3 * i + 1]; p.th = A.part[3 * i + 2];
        float z[3];
        hs_mcl_noise(A.mo, i, z);
        const hs_mcl_pose q = hs_mcl_predict(A.mo, p, z);
        const sh_m3x2 t = hs_trace_transform(A.stm, q.x, q.y, q.th);
        uint32_t sum = 0, ign = 0;                                         // (at most 7680 * 65025 < 2^29)
        for (int j = lane; j < A.n; j += 64) {
            const float2 pt = k13_pts_s[j];
            uint32_t F;
            if (hs_mcl_point(A.E, t, pt.x, pt.y, &F)) sum += F; else ign++;
        }
        for (int off = 32; off > 0; off >>= 1) { sum += __shfl_xor(sum, off, 64); ign += __shfl_xor(ign, off, 64); }
        const k13_u64 cost = (k13_u64)sum + (k13_u64)A.r2 * (k13_u64)ign;
        const k13_u64 a = A.acc[i] + cost;
        if (lane == 0) {
            A.part[3 * i] = q.x; A.part[3 * i + 1] = q.y; A.part[3 * i + 2] = q.th;
            A.a[i] = a;
        }
        min_a = a < min_a ? a : min_a; cmin = cost < cmin ? cost : cmin; cmax = cost > cmax ? cost : cmax;
    }
    if (lane == 0 && cmin != ~0ull) {                                      // (the wavefront had a particle)
        __hip_atomic_fetch_min(A.ctr + K13_C_MIN_A, min_a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_min(A.ctr + K13_C_CMIN, cmin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_max(A.ctr + K13_C_CMAX, cmax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__device__ static __forceinline__ k13_u64 k13_wave_sum(k13_u64 v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;                                                              // (lane 0 holds the sum)
}

__global__ void __launch_bounds__(K13_LANES) k13_weigh(const float *__restrict__ part, const k13_u64 *__restrict__ a, int N, uint32_t beta,
                                                       k13_u64 *__restrict__ acc, uint32_t *__restrict__ w_out, k13_u64 *ctr)
{
    const int i = (int)blockIdx.x * K13_LANES + (int)threadIdx.x;
    const bool have = i < N;
    const k13_u64 min_a = ctr[K13_C_MIN_A];                                // (final: k13_score has ended)
    k13_u64 w = 0, h = 0, key = ~0ull;
    long long ix = 0, iy = 0;
    int ic = 0, is = 0;
    bool placed = false;
    if (have) {
        const k13_u64 ai = a[i], accp = ai - min_a;
        acc[i] = accp;
        w = hs_mcl_weight(accp, beta);
        w_out[i] = (uint32_t)w;
        h = w >> 20;
        key = (ai << 16) | (k13_u64)i;
        hs_mcl_pose q;
        q.x = part[3 * i]; q.y = part[3 * i + 1]; q.th = part[3 * i + 2];
        placed = hs_mcl_moments(q, &ix, &iy, &ic, &is);
        if (!placed) { ix = 0; iy = 0; ic = 0; is = 0; }
    }
    const k13_u64 hp = placed ? h : 0ull;
    // (the int64 sums as uint64: two's complement addition is the same operation)
    const k13_u64 s_w = k13_wave_sum(w), s_a = k13_wave_sum(h), s_q = k13_wave_sum(h * h);
    const k13_u64 s_x = k13_wave_sum(hp * (k13_u64)ix), s_y = k13_wave_sum(hp * (k13_u64)iy);
    const k13_u64 s_c = k13_wave_sum(hp * (k13_u64)(long long)ic), s_s = k13_wave_sum(hp * (k13_u64)(long long)is);
    const k13_u64 n_un = (k13_u64)__popcll(__ballot(have && !placed));
    for (int off = 32; off > 0; off >>= 1) { const k13_u64 o = __shfl_down(key, off, 64); key = o < key ? o : key; }
    if ((threadIdx.x & 63) == 0 && key != ~0ull) {                         // (the wavefront had a particle)
        const k13_u64 v[8] = { s_w, s_a, s_q, s_x, s_y, s_c, s_s, n_un };
#pragma unroll
        for (int k = 0; k < 8; k++)
            if (v[k]) __hip_atomic_fetch_add(ctr + K13_C_W + k, v[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_min(ctr + K13_C_KEY, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
static_assert(K13_C_A == K13_C_W + 1 && K13_C_Q == K13_C_W + 2 && K13_C_SHX == K13_C_W + 3 && K13_C_SHY == K13_C_W + 4 && K13_C_SHC == K13_C_W + 5 &&
              K13_C_SHS == K13_C_W + 6 && K13_C_UNPLACED == K13_C_W + 7, "k13_weigh's eight sums are consecutive counters");

__global__ void __launch_bounds__(K13_SCAN_LANES) k13_scan(const uint32_t *__restrict__ w, int N, int n_eff_min, const k13_u64 *__restrict__ ctr,
                                                           k13_u64 *__restrict__ C)
{
    __shared__ k13_u64 wave_s[K13_SCAN_LANES / 64];
    if (!hs_mcl_decide(ctr[K13_C_A], ctr[K13_C_Q], n_eff_min)) return;     // (uniform over the workgroup)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    k13_u64 carry = 0;
    for (int base = 0; base < N; base += K13_SCAN_CHUNK) {
        const int i0 = base + 4 * tid;
        k13_u64 v[4];
#pragma unroll
        for (int c = 0; c < 4; c++) v[c] = (i0 + c < N) ? (k13_u64)w[i0 + c] : 0ull;
        v[1] += v[0]; v[2] += v[1]; v[3] += v[2];
        k13_u64 inc = v[3];
        for (int off = 1; off < 64; off <<= 1) { const k13_u64 o = __shfl_up(inc, off, 64); if (lane >= off) inc += o; }
        if (lane == 63) wave_s[wave] = inc;
        __syncthreads();
        k13_u64 before = 0, all = 0;
        for (int k = 0; k < K13_SCAN_LANES / 64; k++) { const k13_u64 t = wave_s[k]; if (k < wave) before += t; all += t; }
        const k13_u64 excl = carry + before + (inc - v[3]);
#pragma unroll
        for (int c = 0; c < 4; c++) if (i0 + c < N) C[i0 + c] = excl + v[c];
        carry += all;
        __syncthreads();                                                   // (wave_s is written again by the next chunk)
    }
}

struct k13_res_arg {
    const float *pred; float *out; int N;
    const k13_u64 *C; k13_u64 *acc; int32_t *anc;
    int n_eff_min; hs_mcl_motion mo;
    k13_u64 *ctr;
    slamhip_mcl_summary *summary;          // pinned, device-visible
};

__global__ void __launch_bounds__(K13_LANES) k13_resample(const k13_res_arg A)
{
    __shared__ int last_s;
    const int tid = threadIdx.x, lane = tid & 63;
    const int k = (int)blockIdx.x * K13_LANES + tid;
    const bool have = k < A.N;
    const k13_u64 W = A.ctr[K13_C_W];
    const bool resample = hs_mcl_decide(A.ctr[K13_C_A], A.ctr[K13_C_Q], A.n_eff_min);   // (final: k13_weigh has ended; uniform)
    if (resample) {
        const k13_u64 u = hs_mcl_comb_offset(A.mo, W);
        const int kk = have ? k : A.N - 1;                                 // (a lane past the end searches for the last tooth and stores nothing)
        const int anc = hs_mcl_ancestor(A.C, A.N, (k13_u64)kk * W + u);
        int prev = __shfl_up(anc, 1, 64);
        if (lane == 0) prev = kk > 0 ? hs_mcl_ancestor(A.C, A.N, (k13_u64)(kk - 1) * W + u) : -1;
        const int n_new = (int)__popcll(__ballot(have && anc != prev));
        if (have) {
            A.out[3 * k] = A.pred[3 * anc]; A.out[3 * k + 1] = A.pred[3 * anc + 1]; A.out[3 * k + 2] = A.pred[3 * anc + 2];
            A.acc[k] = 0ull;
            A.anc[k] = anc;
        }
        if (lane == 0 && n_new) __hip_atomic_fetch_add(A.ctr + K13_C_DISTINCT, (k13_u64)n_new, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else if (have) {
        A.out[3 * k] = A.pred[3 * k]; A.out[3 * k + 1] = A.pred[3 * k + 1]; A.out[3 * k + 2] = A.pred[3 * k + 2];
        A.anc[k] = k;
    }
    // the last workgroup to get here emits the summary: every wavefront's atomic add is ordered before its workgroup's ticket
    __syncthreads();
    if (tid == 0) {
        const k13_u64 ticket = __hip_atomic_fetch_add(A.ctr + K13_C_TICKET, 1ull, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        last_s = ticket == (k13_u64)gridDim.x - 1ull;
    }
    __syncthreads();
    if (!last_s || tid != 0) return;
    slamhip_mcl_summary S;
    S.W = W;
    S.A = A.ctr[K13_C_A]; S.Q = A.ctr[K13_C_Q]; S.key_best = A.ctr[K13_C_KEY];
    S.sum_hx = (int64_t)A.ctr[K13_C_SHX]; S.sum_hy = (int64_t)A.ctr[K13_C_SHY];
    S.sum_hc = (int64_t)A.ctr[K13_C_SHC]; S.sum_hs = (int64_t)A.ctr[K13_C_SHS];
    S.cost_min = A.ctr[K13_C_CMIN]; S.cost_max = A.ctr[K13_C_CMAX];
    S.resampled = resample ? 1 : 0;
    S.n_distinct = resample ? (int32_t)__hip_atomic_load(A.ctr + K13_C_DISTINCT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : A.N;
    S.n_unplaced = (int32_t)A.ctr[K13_C_UNPLACED];
    S.n_particles = A.N;
    *A.summary = S;
}

// ---- host side ---------------------------------------------------------------------------------------------------
// What the filter needs beyond the field's blocks, made by the first slamhip_hs_mcl_set and kept, all sized for HS_MCL_MAX_N: the
// two particle buffers used in turn, acc, a, w, C, the ancestors and the counters in device memory, a pinned block the set and the
// get pass through, and a pinned, device-visible record k13_resample stores the summary in.
struct hs_mcl {
    hs_block<float, HS_MEM_DEVICE> d_part[2]; int cur;
    hs_block<k13_u64, HS_MEM_DEVICE> d_acc, d_a, d_C, d_ctr;
    hs_block<uint32_t, HS_MEM_DEVICE> d_w; hs_block<int32_t, HS_MEM_DEVICE> d_anc;
    hs_block<unsigned char, HS_MEM_PINNED> h_io;
    hs_block<slamhip_mcl_summary, HS_MEM_PINNED_VISIBLE> h_sum;
    int N;                                 // 0: no set
};
#define HS_MCL_IO_BYTES ((size_t)HS_MCL_MAX_N * (3 * sizeof(float) + sizeof(k13_u64) + sizeof(int32_t)))

static int32_t hs_mcl_blocks(slamhip_hs *hs)
{
    SH_TRY(hs_unit<&slamhip_hs::mcl>(hs));
    hs_mcl *m = hs->mcl;
    const size_t n = HS_MCL_MAX_N;
    const char *who = "localisation";
    // (fixed sizes: a block that is there is large enough)
    SH_TRY(m->d_part[0].grow(n * 3 * sizeof(float), who));
    SH_TRY(m->d_part[1].grow(n * 3 * sizeof(float), who));
    SH_TRY(m->d_acc.grow(n * sizeof(k13_u64), who));
    SH_TRY(m->d_a.grow(n * sizeof(k13_u64), who));
    SH_TRY(m->d_C.grow(n * sizeof(k13_u64), who));
    SH_TRY(m->d_ctr.grow(K13_CTRS * sizeof(k13_u64), who));
    SH_TRY(m->d_w.grow(n * sizeof(uint32_t), who));
    SH_TRY(m->d_anc.grow(n * sizeof(int32_t), who));
    SH_TRY(m->h_io.grow(HS_MCL_IO_BYTES, who));
    SH_TRY(m->h_sum.grow(sizeof(slamhip_mcl_summary), who));
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_mcl_set(slamhip_hs *hs, const float *poses, int32_t N)
{
    SH_CHECK_ARG(hs && poses);
    if (N < 1 || N > HS_MCL_MAX_N) SH_FAIL(SLAMHIP_ERR_INVALID, "localisation: N = %d particles must lie in [1, %d]", N, HS_MCL_MAX_N);
    for (int i = 0; i < 3 * N; i++)
        if (!isfinite(poses[i])) SH_FAIL(SLAMHIP_ERR_INVALID, "localisation: particle %d, (%g, %g, %g), is not finite", i / 3, poses[i - i % 3],
                                         poses[i - i % 3 + 1], poses[i - i % 3 + 2]);
    SH_TRY(hs_call_begin(hs));
    SH_TRY(hs_mcl_blocks(hs));
    hs_mcl *m = hs->mcl;
    m->N = 0;                                                              // (no set until this one has landed)
    // (the blocks are idle: every call waits for its own launches, and a call that timed out has poisoned the context)
    const size_t pose_bytes = sizeof(float) * 3 * (size_t)N, anc_bytes = sizeof(int32_t) * (size_t)N;
    memcpy(m->h_io, poses, pose_bytes);
    int32_t *h_anc = (int32_t *)(m->h_io + pose_bytes);
    for (int i = 0; i < N; i++) h_anc[i] = i;
    hipStream_t st = hs->ctx->stream;
    SH_HIP(hipMemcpyAsync(m->d_part[m->cur], m->h_io, pose_bytes, hipMemcpyHostToDevice, st));
    SH_HIP(hipMemcpyAsync(m->d_anc, h_anc, anc_bytes, hipMemcpyHostToDevice, st));
    SH_HIP(hipMemsetAsync(m->d_acc, 0, sizeof(k13_u64) * (size_t)N, st));
    SH_TRY(hs_call_finish(hs));
    m->N = N;
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_mcl_get(slamhip_hs *hs, float *poses, uint64_t *acc, int32_t *ancestors, int32_t N)
{
    SH_CHECK_ARG(hs);
    hs_mcl *m = hs->mcl;
    if (!m || m->N == 0) SH_FAIL(SLAMHIP_ERR_STATE, "localisation: no particle set (slamhip_hs_mcl_set first)");
    if (N != m->N) SH_FAIL(SLAMHIP_ERR_INVALID, "localisation: N = %d, but the set holds %d particles", N, m->N);
    SH_TRY(hs_call_begin(hs));
    const size_t pose_bytes = sizeof(float) * 3 * (size_t)N, acc_bytes = sizeof(k13_u64) * (size_t)N, anc_bytes = sizeof(int32_t) * (size_t)N;
    unsigned char *h_acc = m->h_io, *h_pose = h_acc + acc_bytes, *h_anc = h_pose + pose_bytes;   // (the 8-byte records first)
    hipStream_t st = hs->ctx->stream;
    if (poses) SH_HIP(hipMemcpyAsync(h_pose, m->d_part[m->cur], pose_bytes, hipMemcpyDeviceToHost, st));
    if (acc) SH_HIP(hipMemcpyAsync(h_acc, m->d_acc, acc_bytes, hipMemcpyDeviceToHost, st));
    if (ancestors) SH_HIP(hipMemcpyAsync(h_anc, m->d_anc, anc_bytes, hipMemcpyDeviceToHost, st));
    SH_TRY(hs_call_finish(hs));
    if (poses) memcpy(poses, h_pose, pose_bytes);
    if (acc) memcpy(acc, h_acc, acc_bytes);
    if (ancestors) memcpy(ancestors, h_anc, anc_bytes);
    return SLAMHIP_OK;
}

// what every entry point refuses for the spec alone (N: the set's size)
int32_t hs_mcl_check_spec(int n_levels, const slamhip_mcl_spec *spec, int N)
{
    SH_TRY(hs_df_check("distance field", n_levels, spec->level, spec->world, spec->site_mask, spec->radius));
    const float *f = spec->delta;                                          // delta, sigma, frame_offset: eight consecutive floats
    static_assert(offsetof(slamhip_mcl_spec, frame_offset) + 2 * sizeof(float) == offsetof(slamhip_mcl_spec, delta) + 8 * sizeof(float), "eight floats");
    for (int i = 0; i < 8; i++)
        if (!isfinite(f[i])) SH_FAIL(SLAMHIP_ERR_INVALID, "localisation: float %d of delta, sigma, frame_offset is %g, not finite", i, f[i]);
    if (spec->beta == 0) SH_FAIL(SLAMHIP_ERR_INVALID, "localisation: beta = 0 weighs every particle alike");
    if (spec->n_eff_min < 0 || spec->n_eff_min > N + 1)
        SH_FAIL(SLAMHIP_ERR_INVALID, "localisation: n_eff_min = %d must lie in [0, N + 1 = %d]", spec->n_eff_min, N + 1);
    return SLAMHIP_OK;
}

static hs_mcl_motion hs_mcl_motion_of(const slamhip_mcl_spec *spec)
{
    hs_mcl_motion m;
    m.dx = spec->delta[0]; m.dy = spec->delta[1]; m.dth = spec->delta[2];
    m.sx = spec->sigma[0]; m.sy = spec->sigma[1]; m.sth = spec->sigma[2];
    m.fox = spec->frame_offset[0]; m.foy = spec->frame_offset[1];
    m.key0 = (uint32_t)spec->seed; m.key1 = (uint32_t)(spec->seed >> 32);
    m.str0 = (uint32_t)spec->stream; m.str1 = (uint32_t)(spec->stream >> 32);
    return m;
}

int32_t hs_mcl_check_step(const slamhip_hs *hs, const slamhip_mcl_spec *spec, int n_points, bool scan_is_set)
{
    const hs_mcl *m = hs->mcl;
    SH_TRY(hs_mcl_check_spec(hs->n_levels, spec, (m && m->N) ? m->N : HS_MCL_MAX_N));
    if (n_points > HS_MCL_MAX_POINTS)
        SH_FAIL(SLAMHIP_ERR_INVALID, "localisation: a scan of %d points; at most %d fit the 64 KB of LDS a workgroup may allocate", n_points, HS_MCL_MAX_POINTS);
    if (!m || m->N == 0) SH_FAIL(SLAMHIP_ERR_STATE, "localisation: no particle set (slamhip_hs_mcl_set first)");
    if (scan_is_set && n_points <= 0) SH_FAIL(SLAMHIP_ERR_STATE, "localisation: no scan (slamhip_hs_set_scan first)");
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_mcl_step(slamhip_hs *hs, const slamhip_mcl_spec *spec, slamhip_mcl_summary *out)
{
    SH_CHECK_ARG(hs && spec && out);
    SH_TRY(hs_mcl_check_step(hs, spec, hs->n_points, true));
    SH_TRY(hs_call_begin(hs));
    hs_mcl *m = hs->mcl;
    const int N = m->N, n = hs->n_points, r = spec->radius;
    hs_class_map M; hs_field E;
    SH_TRY(hs_df_field_prepare(hs, spec->level, spec->world != 0, spec->site_mask, r, &M, &E));
    hipStream_t st = hs->ctx->stream;
    SH_TRY(hs_flush_scan(hs));
    // (the blocks are idle: every call waits for its own launches, and a call that timed out has poisoned the context)
    SH_HIP(hipMemsetAsync(m->d_ctr, 0xFF, sizeof(k13_u64) * 3, st));      // min a, key_best, cost_min: UINT64_MAX
    SH_HIP(hipMemsetAsync(m->d_ctr + 3, 0, sizeof(k13_u64) * (K13_CTRS - 3), st));
    SH_TRY(hs_df_field_enqueue(hs, spec->level, spec->world != 0, &M, &E, spec->site_mask));
    float *pred = m->d_part[m->cur], *next = m->d_part[m->cur ^ 1];
    k13_score_arg A;
    A.pts = hs->d_pts; A.n = n;
    A.part = pred; A.N = N;
    A.acc = m->d_acc; A.a = m->d_a;
    A.stm = hs->lv[spec->level].stm; A.r2 = (uint32_t)(r * r);
    A.E = E;
    A.mo = hs_mcl_motion_of(spec);
    A.ctr = m->d_ctr;
    const int score_blocks = std::min(sh_div_up(N, K13_LANES / 64), K13_SCORE_MAX_BLOCKS), blocks = sh_div_up(N, K13_LANES);
    // k13_score predicts in place and the buffers change names only after the wait: from here until then the set is neither the old
    // one nor the new one, so a step that fails on the way leaves NO set (slamhip_hs_mcl_set again)
    m->N = 0;
    hipLaunchKernelGGL(k13_score, dim3((unsigned)score_blocks), dim3(K13_LANES), sizeof(float2) * (size_t)n, st, A);
    SH_HIP(hipGetLastError());
    hipLaunchKernelGGL(k13_weigh, dim3((unsigned)blocks), dim3(K13_LANES), 0, st, (const float *)pred, (const k13_u64 *)m->d_a, N, spec->beta, m->d_acc, m->d_w,
                       m->d_ctr);
    SH_HIP(hipGetLastError());
    hipLaunchKernelGGL(k13_scan, dim3(1), dim3(K13_SCAN_LANES), 0, st, (const uint32_t *)m->d_w, N, spec->n_eff_min, (const k13_u64 *)m->d_ctr, m->d_C);
    SH_HIP(hipGetLastError());
    k13_res_arg R;
    R.pred = pred; R.out = next; R.N = N;
    R.C = m->d_C; R.acc = m->d_acc; R.anc = m->d_anc;
    R.n_eff_min = spec->n_eff_min; R.mo = A.mo;
    R.ctr = m->d_ctr; R.summary = m->h_sum;
    hipLaunchKernelGGL(k13_resample, dim3((unsigned)blocks), dim3(K13_LANES), 0, st, R);
    SH_HIP(hipGetLastError());
    SH_TRY(hs_call_finish(hs));
    m->cur ^= 1;
    m->N = N;
    *out = *m->h_sum;
    return SLAMHIP_OK;
}

// CPU-side test hook: the field by slamhip_debug_distance_field over E, the step by hs_mcl.h -- the text the kernels run -- one
// particle after the other, one point after the other.
extern "C" int32_t slamhip_debug_mcl_step(const uint8_t *cls, int32_t cw, int32_t ch, float stm, const float *points, int32_t n_points,
                                          const float *particles_in, const uint64_t *acc_in, int32_t N, const slamhip_mcl_spec *spec,
                                          float *particles_out, uint64_t *acc_out, int32_t *ancestors_out, slamhip_mcl_summary *summary)
{
    SH_CHECK_ARG(cls && points && particles_in && spec && particles_out && acc_out && ancestors_out && summary && cw >= 1 && ch >= 1);
    if (!(isfinite(stm) && stm > 0.0f)) SH_FAIL(SLAMHIP_ERR_INVALID, "localisation: stm = %g must be finite and positive", stm);
    if (n_points < 1 || n_points > HS_MCL_MAX_POINTS) SH_FAIL(SLAMHIP_ERR_INVALID, "localisation: n_points = %d must lie in [1, %d]", n_points, HS_MCL_MAX_POINTS);
    if (N < 1 || N > HS_MCL_MAX_N) SH_FAIL(SLAMHIP_ERR_INVALID, "localisation: N = %d particles must lie in [1, %d]", N, HS_MCL_MAX_N);
    for (int i = 0; i < 3 * N; i++)
        if (!isfinite(particles_in[i])) SH_FAIL(SLAMHIP_ERR_INVALID, "localisation: particle %d is not finite", i / 3);
    SH_TRY(hs_mcl_check_spec(1, spec, N));                                 // (the hook has one level)
    const int r = spec->radius;
    hs_field E;
    E.ew = cw + 2 * r; E.eh = ch + 2 * r; E.pitch = E.ew; E.e_x0 = -r; E.e_y0 = -r; E.outside = hs_df_outside(spec->site_mask, r);
    std::vector<uint16_t> field((size_t)E.ew * (size_t)E.eh);
    SH_TRY(slamhip_debug_distance_field(cls, cw, ch, spec->site_mask, r, -r, -r, E.ew, E.eh, field.data()));
    E.f = field.data();
    const hs_mcl_motion mo = hs_mcl_motion_of(spec);
    std::vector<hs_mcl_pose> pred((size_t)N);
    std::vector<k13_u64> a((size_t)N), C((size_t)N);
    std::vector<uint32_t> w((size_t)N);
    slamhip_mcl_summary S;
    memset(&S, 0, sizeof(S));
    S.cost_min = ~0ull; S.key_best = ~0ull; S.n_particles = N;
    k13_u64 min_a = ~0ull;
    for (int i = 0; i < N; i++) {
        const hs_mcl_pose p = { particles_in[3 * i], particles_in[3 * i + 1], particles_in[3 * i + 2] };
        float z[3];
        hs_mcl_noise(mo, i, z);
        pred[i] = hs_mcl_predict(mo, p, z);
        const sh_m3x2 t = hs_trace_transform(stm, pred[i].x, pred[i].y, pred[i].th);
        k13_u64 cost = 0;
        for (int j = 0; j < n_points; j++) {
            uint32_t F;
            cost += hs_mcl_point(E, t, points[2 * j], points[2 * j + 1], &F) ? (k13_u64)F : (k13_u64)(r * r);
        }
        a[i] = (acc_in ? (k13_u64)acc_in[i] : 0ull) + cost;
        min_a = std::min(min_a, a[i]);
        S.cost_min = std::min<uint64_t>(S.cost_min, cost); S.cost_max = std::max<uint64_t>(S.cost_max, cost);
        S.key_best = std::min<uint64_t>(S.key_best, (a[i] << 16) | (k13_u64)i);
    }
    for (int i = 0; i < N; i++) {
        a[i] -= min_a;                                                     // acc'
        w[i] = hs_mcl_weight(a[i], spec->beta);
        S.W += w[i];
        C[i] = S.W;
        const k13_u64 h = w[i] >> 20;
        S.A += h; S.Q += h * h;
        long long ix, iy; int ic, is;
        if (hs_mcl_moments(pred[i], &ix, &iy, &ic, &is)) {
            S.sum_hx += (int64_t)h * ix; S.sum_hy += (int64_t)h * iy; S.sum_hc += (int64_t)h * ic; S.sum_hs += (int64_t)h * is;
        } else
            S.n_unplaced++;
    }
    S.resampled = hs_mcl_decide(S.A, S.Q, spec->n_eff_min) ? 1 : 0;
    if (S.resampled) {
        const k13_u64 u = hs_mcl_comb_offset(mo, S.W);
        for (int k = 0; k < N; k++) {
            const int anc = hs_mcl_ancestor(C.data(), N, (k13_u64)k * S.W + u);
            if (k == 0 || anc != ancestors_out[k - 1]) S.n_distinct++;
            ancestors_out[k] = anc;
            particles_out[3 * k] = pred[anc].x; particles_out[3 * k + 1] = pred[anc].y; particles_out[3 * k + 2] = pred[anc].th;
            acc_out[k] = 0;
        }
    } else {
        S.n_distinct = N;
        for (int k = 0; k < N; k++) {
            ancestors_out[k] = k;
            particles_out[3 * k] = pred[k].x; particles_out[3 * k + 1] = pred[k].y; particles_out[3 * k + 2] = pred[k].th;
            acc_out[k] = a[k];
        }
    }
    *summary = S;
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_debug_mcl_table(uint32_t out[64])
{
    SH_CHECK_ARG(out);
    for (int f = 0; f < 64; f++) out[f] = hs_mcl_table(f);
    return SLAMHIP_OK;
}
