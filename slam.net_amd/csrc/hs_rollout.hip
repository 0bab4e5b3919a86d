// hs_rollout.hip -- K12, command rollouts over the cost-to-go field of HectorSLAM's map: B sequences of velocity commands rolled
// forward from one pose by explicit Euler steps, each cut where the body first touches an untraversable cell, with the field's
// cost along and at the end of each (slamhip_hs_rollouts, slamhip_debug_rollouts).  No reference counterpart.  Definition:
// include/slamhip.h (slamhip_hs_rollouts); the arithmetic host and device share: hs_rollout.h.
//
// The field is K11's (hs_nav.hip), built by the function slamhip_hs_nav_field builds it with (hs_nav_field_for_rollouts): the
// traversable words and the costs of M stay in device memory, and the stream has drained when it returns.  Behind it:
//  * k12_count: a lane per cell of M, n_reached and max_cost_reached into K11's counter block (k11_dirs is not run).
//  * k12_rollout<SG, STAGED>: SG lanes per rollout, SG a power of two in [1, 64]; lane l of them tests items l, l + SG, ... of the
//    P + 1 items of a pose -- item 0 the centre's cost, item p + 1 body point p's traversable bit.  THE PRODUCT RUNS SG = 1,
//    STAGED = false: a lane walks its rollout alone, over global memory.  The other instances are the two developer experiments
//    (SLAMHIP_ROLLOUT_SG, SLAMHIP_ROLLOUT_LDS; EXPERIMENTS.md): with SG >= P + 1 a lane has one item, every lane of the sub-group
//    integrates the same state (hs_ro_step: bit-identical across it) and the sub-group's AND is a ballot masked to its lanes.  A
//    rollout whose pose is not free goes idle, and the loop -- bounded by T -- ends for the wavefront once all its rollouts
//    have.  The loop is wavefront-uniform, so every ballot is executed by all 64 lanes.  Lane 0 of a rollout's lanes keeps the
//    record (hs_ro_accept) and stores it; the two keys are reduced over the wavefront by shuffles and merged by one 64-bit
//    agent-scope atomic minimum each per wavefront, the complete rollouts counted by one atomic add.
//  * k12_emit, one workgroup: K11's counters, C at P_0's centre, n_complete and the keys into pinned memory.
// Commands and body points go through the pinned block into device memory with one copy, as K8's poses do; the records come
// back through the same block.
#include "hs_blocks.h"
#include "hs_nav_host.h"
#include "hs_rollout.h"

#define K12_LANES 256
#define K12_SQ 256                         // the staged square's side in cells (the developer experiment k12_rollout<SG, true>): 256 rows of 8 words, 8 KB of LDS
#define K12_SQ_WORDS (K12_SQ / 32)
// the summary block k12_emit stores: K11's counters, then
#define K12_H_START (K11_CTRS + 0)
#define K12_H_COMPLETE (K11_CTRS + 1)
#define K12_H_KEYS (K11_CTRS + 2)          // key_end, key_min: two words each, low first
#define K12_HEAD_WORDS (K11_CTRS + 6)

static_assert(sizeof(slamhip_rollout_result) == 28 && sizeof(slamhip_rollout_summary) == 64 && sizeof(hs_ro_result) == sizeof(slamhip_rollout_result),
              "the records of include/slamhip.h");
static_assert(HS_RO_MAX_POINTS + 1 <= 64, "a rollout's items fit a wavefront");

struct k12_arg {
    hs_ro_field F;
    hs_ro_pose p0; float dt;
    const float *body; int P;              // P pairs
    const float *cmds; int B, n_cmd, hold, T;
    hs_ro_result *out;                     // B records
    unsigned long long *keys;              // key_end, key_min
    uint32_t *n_complete;
};

__global__ void __launch_bounds__(256) k12_count(const uint32_t *__restrict__ cost, int n, uint32_t *__restrict__ ctr)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    const uint32_t c = t < n ? cost[t] : HS_NAV_UNREACHED;
    const bool reached = c != HS_NAV_UNREACHED;
    const int n_r = (int)__popcll(__ballot(reached));
    uint32_t mx = reached ? c : 0u;
    for (int off = 32; off > 0; off >>= 1) { const uint32_t o = __shfl_down(mx, off, 64); mx = o > mx ? o : mx; }
    if ((threadIdx.x & 63) == 0 && n_r) {
        __hip_atomic_fetch_add(ctr + K11_C_REACHED, (uint32_t)n_r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_max(ctr + K11_C_MAXCOST, mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// STAGED (a developer experiment, SLAMHIP_ROLLOUT_LDS = 1; measured and not adopted, EXPERIMENTS.md): the traversable words of a
// square of K12_SQ x K12_SQ cells around P_0's centre cell, its first column a multiple of 32 in M's frame, are copied into LDS by
// every workgroup -- zeros where the square leaves M, where no cell is traversable anyway -- and a body point whose cell lies in
// the square reads its bit there; any other cell goes to global memory as in the plain form.
template <int SG, bool STAGED>
__global__ void __launch_bounds__(K12_LANES) k12_rollout(const k12_arg A)
{
    __shared__ uint32_t sq_s[STAGED ? K12_SQ * K12_SQ_WORDS : 1];
    long long sqx = 0, sqy = 0;                                            // the square's first cell in M's frame
    if (STAGED) {
        long long cx = 0, cy = 0;
        if (!hs_ro_cell_of(A.F, A.p0.x, A.p0.y, &cx, &cy)) { cx = 0; cy = 0; }   // (no cell: any square will do)
        sqx = ((cx - K12_SQ / 2) >> 5) << 5; sqy = cy - K12_SQ / 2;        // (an arithmetic shift: rounds down below 0 too)
        for (int j = threadIdx.x; j < K12_SQ * K12_SQ_WORDS; j += K12_LANES) {
            const long long y = sqy + j / K12_SQ_WORDS, wi = (sqx >> 5) + j % K12_SQ_WORDS;
            sq_s[j] = (y >= 0 && y < A.F.h && wi >= 0 && wi < A.F.twpr) ? A.F.tw[(size_t)y * A.F.twpr + (size_t)wi] : 0u;
        }
        __syncthreads();
    }
    const int t = blockIdx.x * K12_LANES + threadIdx.x;                    // (at most 65536 * 64 lanes)
    const int b = t / SG, li = t & (SG - 1), lane = threadIdx.x & 63;
    const unsigned long long gm = (SG == 64 ? ~0ull : ((1ull << (SG & 63)) - 1ull)) << (lane & ~(SG - 1));   // the sub-group's lanes in a ballot
    const bool mine = b < A.B;
    bool alive = mine;
    hs_ro_pose p = A.p0;
    hs_ro_result r = hs_ro_begin(p);
    const float *cmd = A.cmds + 2 * (size_t)(mine ? b : 0) * (size_t)A.n_cmd;
    int ci = 0, held = 0;
    for (int i = 0; i <= A.T; i++) {                                       // poses P_0 .. P_T
        if (!__any(alive)) break;                                          // (uniform over the wavefront)
        float s, c;
        sh_det_sincosf(p.th, &s, &c);
        bool ok = true;
        uint32_t cost = HS_NAV_UNREACHED;
        if (alive)
            for (int k = li; k <= A.P; k += SG) {                          // (P <= 32)
                if (k == 0) {
                    cost = hs_ro_cost(A.F, p.x, p.y);
                    ok = ok && cost != HS_NAV_UNREACHED;
                } else {
                    float wx, wy;
                    hs_ro_body(p, s, c, A.body[2 * (k - 1)], A.body[2 * (k - 1) + 1], &wx, &wy);
                    if (STAGED) {
                        long long x, y;
                        bool tr = false;
                        if (hs_ro_cell_of(A.F, wx, wy, &x, &y)) {
                            const long long lx = x - sqx, ly = y - sqy;
                            if (lx >= 0 && lx < K12_SQ && ly >= 0 && ly < K12_SQ) tr = (sq_s[(int)ly * K12_SQ_WORDS + ((int)lx >> 5)] >> ((int)lx & 31)) & 1u;
                            else tr = hs_ro_trav_at(A.F, x, y);
                        }
                        ok = ok && tr;
                    } else
                        ok = ok && hs_ro_traversable(A.F, wx, wy);
                }
            }
        const bool free_pose = (__ballot(ok) & gm) == gm;                  // (an idle sub-group's answer is not used)
        if (alive) {
            if (free_pose) hs_ro_accept(r, i, cost, p); else alive = false;
        }
        if (alive && i < A.T) {
            p = hs_ro_step(p, s, c, cmd[2 * ci], cmd[2 * ci + 1], A.dt);
            if (++held == A.hold) { held = 0; ci++; }
        }
    }
    const bool leader = mine && li == 0;
    if (leader) A.out[b] = r;
    const bool complete = leader && r.n_free == A.T + 1;
    unsigned long long ke = complete ? hs_ro_key(r.end_cost, b) : ~0ull, km = (leader && r.n_free >= 1) ? hs_ro_key(r.min_cost, b) : ~0ull;
    const int n_c = (int)__popcll(__ballot(complete));
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long oe = __shfl_down(ke, off, 64), om = __shfl_down(km, off, 64);
        ke = oe < ke ? oe : ke; km = om < km ? om : km;
    }
    if (lane == 0) {
        if (ke != ~0ull) __hip_atomic_fetch_min(A.keys, ke, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (km != ~0ull) __hip_atomic_fetch_min(A.keys + 1, km, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (n_c) __hip_atomic_fetch_add(A.n_complete, (uint32_t)n_c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ void __launch_bounds__(64) k12_emit(const hs_ro_field F, const hs_ro_pose p0, const uint32_t *__restrict__ ctr, const unsigned long long *__restrict__ keys,
                                               const uint32_t *__restrict__ n_complete, uint32_t *__restrict__ out)
{
    const int t = threadIdx.x;
    if (t < K11_CTRS) out[t] = ctr[t];
    else if (t == K12_H_START) out[t] = hs_ro_cost(F, p0.x, p0.y);
    else if (t == K12_H_COMPLETE) out[t] = *n_complete;
    else if (t < K12_HEAD_WORDS) { const int j = t - K12_H_KEYS; out[t] = (uint32_t)(keys[j >> 1] >> (32 * (j & 1))); }
}

// ---- host side ---------------------------------------------------------------------------------------------------
// What the rollouts need beyond the field's blocks, made by the first call and kept: the commands and body points in device
// memory, the records, the keys and the count of complete rollouts, a pinned block the inputs leave and the records reach the
// host through, and a pinned, device-visible block for what k12_emit stores.
struct hs_rollout {
    hs_block<float, HS_MEM_DEVICE> d_in;            // the commands, then the body points
    hs_block<unsigned char, HS_MEM_DEVICE> d_out;  // key_end, key_min, n_complete (24 bytes with padding), then B records
    hs_block<unsigned char, HS_MEM_PINNED> h_io;    // the records; behind them the inputs
    hs_block<uint32_t, HS_MEM_PINNED_VISIBLE> h_head;
};
#define HS_RO_OUT_HEAD 32                  // bytes in front of the records in d_out

// what both entry points refuse for the rollouts' own arguments
static int32_t hs_ro_check(const float *start_pose, float dt, const float *body, int32_t P, const float *cmds, int32_t B, int32_t n_cmd, int32_t hold,
                           const void *out_results)
{
    if (B < 1 || B > HS_RO_MAX_B) SH_FAIL(SLAMHIP_ERR_INVALID, "rollouts: B = %d must lie in [1, %d]", B, HS_RO_MAX_B);
    if (n_cmd < 1 || n_cmd > HS_RO_MAX_CMD) SH_FAIL(SLAMHIP_ERR_INVALID, "rollouts: n_cmd = %d must lie in [1, %d]", n_cmd, HS_RO_MAX_CMD);
    if (hold < 1 || hold > HS_RO_MAX_CMD) SH_FAIL(SLAMHIP_ERR_INVALID, "rollouts: hold = %d must lie in [1, %d]", hold, HS_RO_MAX_CMD);
    if (n_cmd * hold > HS_RO_MAX_T) SH_FAIL(SLAMHIP_ERR_INVALID, "rollouts: T = n_cmd * hold = %d * %d exceeds %d", n_cmd, hold, HS_RO_MAX_T);
    if ((int64_t)B * n_cmd > HS_RO_MAX_PAIRS) SH_FAIL(SLAMHIP_ERR_INVALID, "rollouts: B * n_cmd = %d * %d exceeds 2^22", B, n_cmd);
    if (P < 0 || P > HS_RO_MAX_POINTS) SH_FAIL(SLAMHIP_ERR_INVALID, "rollouts: P = %d body points must lie in [0, %d]", P, HS_RO_MAX_POINTS);
    if (!start_pose || !cmds || !out_results || (P > 0 && !body)) SH_FAIL(SLAMHIP_ERR_INVALID, "rollouts: start_pose, cmds, out_results or (with P = %d) body is NULL", P);
    if (!(isfinite(start_pose[0]) && isfinite(start_pose[1]) && isfinite(start_pose[2])))
        SH_FAIL(SLAMHIP_ERR_INVALID, "rollouts: the start pose (%g, %g, %g) is not finite", start_pose[0], start_pose[1], start_pose[2]);
    if (!isfinite(dt)) SH_FAIL(SLAMHIP_ERR_INVALID, "rollouts: dt = %g is not finite", dt);
    for (int i = 0; i < 2 * P; i++)
        if (!isfinite(body[i])) SH_FAIL(SLAMHIP_ERR_INVALID, "rollouts: body point %d, (%g, %g), is not finite", i / 2, body[i & ~1], body[i | 1]);
    return SLAMHIP_OK;
}

static void hs_ro_summary_of(const uint32_t *head, int x0, int y0, int w, int h, int rounds, slamhip_rollout_summary *S)
{
    S->nav.mx0 = x0; S->nav.my0 = y0; S->nav.mw = w; S->nav.mh = h;
    S->nav.n_traversable = (int32_t)head[K11_C_TRAV]; S->nav.n_reached = (int32_t)head[K11_C_REACHED];
    S->nav.n_sources_used = (int32_t)head[K11_C_USED]; S->nav.n_sources_blocked = (int32_t)head[K11_C_BLOCKED];
    S->nav.max_cost_reached = head[K11_C_MAXCOST]; S->nav.rounds = rounds;
    S->start_cost = head[K12_H_START]; S->n_complete = (int32_t)head[K12_H_COMPLETE];
    S->key_end = (uint64_t)head[K12_H_KEYS] | ((uint64_t)head[K12_H_KEYS + 1] << 32);
    S->key_min = (uint64_t)head[K12_H_KEYS + 2] | ((uint64_t)head[K12_H_KEYS + 3] << 32);
}

// Lanes per rollout.  The default is ONE: a lane walks its rollout alone and tests the P + 1 items of a pose one after the other
// (measured against a sub-group per rollout: EXPERIMENTS.md).  SLAMHIP_ROLLOUT_SG, a developer experiment, sets any power of two in
// [1, 64]; 0 asks for the next power of two >= P + 1, a lane per item.
static int hs_ro_subgroup(int P)
{
    const long long e = sh_env_int("SLAMHIP_ROLLOUT_SG", 1);
    if (e == 0) {
        int sg = 1;
        while (sg < P + 1) sg <<= 1;
        return sg;
    }
    return (e >= 1 && e <= 64 && (e & (e - 1)) == 0) ? (int)e : 1;
}

template <bool STAGED>
static void hs_ro_launch(int sg, unsigned blocks, hipStream_t st, const k12_arg &A)
{
    switch (sg) {
    case 1:  hipLaunchKernelGGL((k12_rollout<1, STAGED>), dim3(blocks), dim3(K12_LANES), 0, st, A); break;
    case 2:  hipLaunchKernelGGL((k12_rollout<2, STAGED>), dim3(blocks), dim3(K12_LANES), 0, st, A); break;
    case 4:  hipLaunchKernelGGL((k12_rollout<4, STAGED>), dim3(blocks), dim3(K12_LANES), 0, st, A); break;
    case 8:  hipLaunchKernelGGL((k12_rollout<8, STAGED>), dim3(blocks), dim3(K12_LANES), 0, st, A); break;
    case 16: hipLaunchKernelGGL((k12_rollout<16, STAGED>), dim3(blocks), dim3(K12_LANES), 0, st, A); break;
    case 32: hipLaunchKernelGGL((k12_rollout<32, STAGED>), dim3(blocks), dim3(K12_LANES), 0, st, A); break;
    default: hipLaunchKernelGGL((k12_rollout<64, STAGED>), dim3(blocks), dim3(K12_LANES), 0, st, A); break;
    }
}

extern "C" int32_t slamhip_hs_rollouts(slamhip_hs *hs, const slamhip_nav_spec *spec, const int32_t *sources, int32_t S, const float start_pose[3],
                                       float dt, const float *body, int32_t P, const float *cmds, int32_t B, int32_t n_cmd, int32_t hold,
                                       slamhip_rollout_result *out_results, slamhip_rollout_summary *out_summary)
{
    SH_CHECK_ARG(hs && spec && out_summary);
    SH_TRY(hs_nav_check_field(hs->n_levels, spec, sources, S));
    SH_TRY(hs_ro_check(start_pose, dt, body, P, cmds, B, n_cmd, hold, out_results));
    slamhip_ctx *ctx = hs->ctx;
    SH_TRY(hs_call_begin(hs));
    SH_TRY(hs_unit<&slamhip_hs::rol>(hs));
    hs_rollout *ro = hs->rol;
    const size_t cmd_bytes = sizeof(float) * 2 * (size_t)B * (size_t)n_cmd, body_bytes = sizeof(float) * 2 * (size_t)P;
    const size_t in_bytes = cmd_bytes + body_bytes + 8;                    // (never empty, and the body block aligned)
    const size_t rec_bytes = sizeof(slamhip_rollout_result) * (size_t)B, rec_pad = (rec_bytes + 15) & ~(size_t)15;
    SH_TRY(ro->d_in.grow(in_bytes, "rollouts"));
    SH_TRY(ro->d_out.grow(HS_RO_OUT_HEAD + rec_bytes, "rollouts"));
    SH_TRY(ro->h_io.grow(rec_pad + in_bytes, "rollouts"));
    SH_TRY(ro->h_head.grow(sizeof(uint32_t) * K12_HEAD_WORDS, "rollouts"));
    hs_nav_view V;
    SH_TRY(hs_nav_field_for_rollouts(hs, spec, sources, S, &V));
    hipStream_t st = ctx->stream;
    unsigned char *h_in = ro->h_io + rec_pad;
    memcpy(h_in, cmds, cmd_bytes);
    if (P) memcpy(h_in + cmd_bytes, body, body_bytes);
    SH_HIP(hipMemcpyAsync(ro->d_in, h_in, cmd_bytes + body_bytes, hipMemcpyHostToDevice, st));
    SH_HIP(hipMemsetAsync(ro->d_out, 0xFF, 16, st));                       // the keys: UINT64_MAX
    SH_HIP(hipMemsetAsync(ro->d_out + 16, 0, 16, st));                     // n_complete
    const int64_t cells = (int64_t)V.M.w * V.M.h;
    hipLaunchKernelGGL(k12_count, dim3((unsigned)sh_div_up((int)cells, 256)), dim3(256), 0, st, V.cost, (int)cells, V.ctr);
    SH_HIP(hipGetLastError());
    k12_arg A;
    A.F.tw = V.tw; A.F.cost = V.cost; A.F.twpr = V.twpr; A.F.w = V.M.w; A.F.h = V.M.h; A.F.x0 = V.M.x0; A.F.y0 = V.M.y0;
    A.F.stm = hs->lv[spec->level].stm;
    A.p0.x = start_pose[0]; A.p0.y = start_pose[1]; A.p0.th = start_pose[2]; A.dt = dt;
    A.cmds = ro->d_in; A.body = ro->d_in + 2 * (size_t)B * (size_t)n_cmd; A.P = P;
    A.B = B; A.n_cmd = n_cmd; A.hold = hold; A.T = n_cmd * hold;
    A.keys = (unsigned long long *)ro->d_out.p; A.n_complete = (uint32_t *)(ro->d_out + 16);
    A.out = (hs_ro_result *)(ro->d_out + HS_RO_OUT_HEAD);
    const int sg = hs_ro_subgroup(P);
    const unsigned blocks = (unsigned)sh_div_up((int)((int64_t)B * sg), K12_LANES);
    if (sh_env_int("SLAMHIP_ROLLOUT_LDS", 0) == 1) hs_ro_launch<true>(sg, blocks, st, A);
    else hs_ro_launch<false>(sg, blocks, st, A);    // (at most 2^22 lanes; no timing class of its own)
    SH_HIP(hipGetLastError());
    hipLaunchKernelGGL(k12_emit, dim3(1), dim3(64), 0, st, A.F, A.p0, (const uint32_t *)V.ctr, (const unsigned long long *)A.keys,
                       (const uint32_t *)A.n_complete, ro->h_head);
    SH_HIP(hipGetLastError());
    SH_HIP(hipMemcpyAsync(ro->h_io, ro->d_out + HS_RO_OUT_HEAD, rec_bytes, hipMemcpyDeviceToHost, st));
    SH_TRY(hs_call_finish(hs));
    memcpy(out_results, ro->h_io, rec_bytes);
    hs_ro_summary_of(ro->h_head, V.M.x0, V.M.y0, V.M.w, V.M.h, V.rounds, out_summary);
    return SLAMHIP_OK;
}

// CPU-side test hook: the field by hs_nav_debug_costs (a sequential Dijkstra), the rollouts by hs_rollout.h -- the text the kernel
// runs -- one rollout after the other, one item after the other.
extern "C" int32_t slamhip_debug_rollouts(const uint8_t *cls, int32_t cw, int32_t ch, int32_t site_mask, int32_t clearance, uint32_t max_cost,
                                          const int32_t *sources, int32_t S, float stm, const float start_pose[3], float dt, const float *body,
                                          int32_t P, const float *cmds, int32_t B, int32_t n_cmd, int32_t hold,
                                          slamhip_rollout_result *out_results, slamhip_rollout_summary *out_summary)
{
    SH_CHECK_ARG(cls && out_summary);
    if (cw < 1 || ch < 1 || (int64_t)cw * ch > HS_NAV_MAX_M)
        SH_FAIL(SLAMHIP_ERR_INVALID, "rollouts: a class array of %d x %d cells; cw, ch >= 1 and cw * ch <= 2^25", cw, ch);
    if (!(isfinite(stm) && stm > 0.0f)) SH_FAIL(SLAMHIP_ERR_INVALID, "rollouts: stm = %g must be finite and positive", stm);
    const slamhip_nav_spec spec = { 0, 0, site_mask, clearance, max_cost };   // (the hook has one level)
    SH_TRY(hs_nav_check_field(1, &spec, sources, S));
    SH_TRY(hs_ro_check(start_pose, dt, body, P, cmds, B, n_cmd, hold, out_results));
    std::vector<uint32_t> tw, cost;
    uint32_t head[K12_HEAD_WORDS] = { 0 };
    SH_TRY(hs_nav_debug_costs(cls, cw, ch, site_mask, clearance, max_cost, sources, S, tw, cost, head));
    for (size_t i = 0; i < cost.size(); i++)
        if (cost[i] != HS_NAV_UNREACHED) { head[K11_C_REACHED]++; head[K11_C_MAXCOST] = cost[i] > head[K11_C_MAXCOST] ? cost[i] : head[K11_C_MAXCOST]; }
    hs_ro_field F;
    F.tw = tw.data(); F.cost = cost.data(); F.twpr = (cw + 31) / 32; F.w = cw; F.h = ch; F.x0 = 0; F.y0 = 0; F.stm = stm;
    const hs_ro_pose p0 = { start_pose[0], start_pose[1], start_pose[2] };
    const int T = n_cmd * hold;
    unsigned long long key_end = ~0ull, key_min = ~0ull;
    for (int b = 0; b < B; b++) {
        hs_ro_pose p = p0;
        hs_ro_result r = hs_ro_begin(p);
        const float *cmd = cmds + 2 * (size_t)b * (size_t)n_cmd;
        for (int i = 0; i <= T; i++) {
            float s, c;
            sh_det_sincosf(p.th, &s, &c);
            const uint32_t k = hs_ro_cost(F, p.x, p.y);
            bool ok = k != HS_NAV_UNREACHED;
            for (int q = 0; q < P && ok; q++) {
                float wx, wy;
                hs_ro_body(p, s, c, body[2 * q], body[2 * q + 1], &wx, &wy);
                ok = hs_ro_traversable(F, wx, wy);
            }
            if (!ok) break;
            hs_ro_accept(r, i, k, p);
            if (i < T) p = hs_ro_step(p, s, c, cmd[2 * (i / hold)], cmd[2 * (i / hold) + 1], dt);
        }
        memcpy(out_results + b, &r, sizeof(r));
        if (r.n_free == T + 1) { head[K12_H_COMPLETE]++; key_end = std::min(key_end, hs_ro_key(r.end_cost, b)); }
        if (r.n_free >= 1) key_min = std::min(key_min, hs_ro_key(r.min_cost, b));
    }
    head[K12_H_START] = hs_ro_cost(F, p0.x, p0.y);
    head[K12_H_KEYS] = (uint32_t)key_end; head[K12_H_KEYS + 1] = (uint32_t)(key_end >> 32);
    head[K12_H_KEYS + 2] = (uint32_t)key_min; head[K12_H_KEYS + 3] = (uint32_t)(key_min >> 32);
    hs_ro_summary_of(head, 0, 0, cw, ch, 0, out_summary);
    return SLAMHIP_OK;
}
