// hs_scanmatch.hip -- K21, stored scans matched pairwise for loop edges (slamhip_hs_scans_match, slamhip_hs_scans_edges,
// slamhip_debug_scans_match).  No reference counterpart.  Definition: include/slamhip.h (slamhip_hs_scans_match); the arithmetic host
// and device share: hs_scanmatch.h, and for the query's cells K7's hs_lattice.h.  The scans are those of K20's store (hs_scans.h).
//
// Two launches of ONE kernel per call on the operator's stream, grid (blocks of headings, pairs), 256 lanes:
//  * k21_pass<false>: the workgroup builds the pair's reference raster in LDS -- 2 bits per cell, 16 cells per word, 36 KB at H = 192:
//    the words zeroed, a lane per reference point ORs the cell's hit bit in (LDS atomic), and behind a barrier a lane per word ORs the
//    near bits of its 16 cells in (hs_sm_dilate_word reads hit bits alone, which no longer change: in place, no second plane).  Then,
//    per heading of its block, the query's cells are staged in LDS in chunks of K21_CHUNK points (k7_search's scheme), and a lane
//    takes one translation of a tile of 256 at a time -- flat over (iy, ix), consecutive lanes consecutive ix -- and walks the chunk:
//    one broadcast read of the point, one read of the raster word.  With more than one chunk a tile stages the chunks again (the
//    staging costs 4 points per lane against a walk of 1024).  The lane keeps the largest packed key of its nodes; a wave maximum by
//    shuffles, the waves' maxima through LDS, ONE 64-bit maximum at agent scope on the pair's key.  The block of heading -nt also
//    leaves n_ref.
//  * k21_pass<true>: the same decomposition and the same scores, formed again (a kept volume would be up to 2^26 int32 per call, 256 MB
//    written and read: DESIGN.md section 4 "K21").  It reads the pair's finished key, adds a node of N to ten int64 in registers, reduces
//    them by shuffles and through LDS, and issues one 64-bit atomic add per workgroup and non-zero field.  The block that holds the best
//    heading counts n_query while it stages that heading.
// Integers throughout: no result depends on the grid, on the headings per block or on the order of the atomics.
// LDS: 36 KB raster + 8 KB points + 384 B = 44.4 KB static per workgroup, under 64 KB; three workgroups per compute unit.
#include "hs_blocks.h"
#include "hs_scans.h"
#include "hs_scanmatch.h"
#include <algorithm>
#include <cmath>
#include <vector>

#define K21_LANES 256
#define K21_CHUNK 1024                     // query points per LDS chunk (8 KB)
#define K21_TARGET_WGS 2048                // workgroups a launch aims at when it cuts the headings into blocks

struct k21_pair { long long roff, qoff; int rn, qn; float guess[3]; int pad; };       // a pair as the kernel reads it: where the two scans lie in the pool
struct k21_acc { unsigned long long key; long long m[HS_SM_SUMS]; int n_ref, n_query; };   // a pair's results in device memory, zeroed in-stream
static_assert(sizeof(k21_pair) == 40 && sizeof(k21_acc) == 96, "the records the kernel reads and writes");

struct k21_arg {
    const float2 *pool; const k21_pair *pairs; k21_acc *acc;
    slamhip_scanmatch_spec S;
    int kb;                                // headings per block
};

template <bool MOMENTS>
__global__ void __launch_bounds__(K21_LANES) k21_pass(const k21_arg A)
{
    __shared__ uint32_t ras_s[HS_SM_MAX_WORDS];
    __shared__ int2 pts_s[K21_CHUNK];
    __shared__ unsigned long long wmax_s[K21_LANES / 64];
    __shared__ long long sum_s[K21_LANES / 64][HS_SM_SUMS];
    __shared__ int cnt_s;
    const int tid = threadIdx.x, pair = blockIdx.y, hb = blockIdx.x;
    const k21_pair P = A.pairs[pair];
    const slamhip_scanmatch_spec S = A.S;
    const int H = S.half, wpr = hs_sm_wpr(H), W = 2 * H, words = W * wpr;  // (words <= HS_SM_MAX_WORDS: the host refuses H > 192)
    const int NX = 2 * S.nx + 1, NY = 2 * S.ny + 1, NT = NX * NY;
    const int k0 = -S.nt + hb * A.kb, k1 = min(k0 + A.kb - 1, S.nt);       // this block's headings

    // ---- rule 1: the reference raster ----
    for (int i = tid; i < words; i += K21_LANES) ras_s[i] = 0u;
    if (tid == 0) cnt_s = 0;
    __syncthreads();
    {
        int used = 0;
        for (int i = tid; i < P.rn; i += K21_LANES) {
            const float2 p = A.pool[P.roff + i];
            int x, y;
            if (!hs_sm_ref_cell(p.x, p.y, S.scale, H, &x, &y)) continue;
            used++;
            if ((unsigned)x < (unsigned)W && (unsigned)y < (unsigned)W) atomicOr(&ras_s[y * wpr + (x >> 4)], hs_sm_hit_bit(x));
        }
        if (!MOMENTS && hb == 0) {                                         // (uniform)
            for (int off = 32; off > 0; off >>= 1) used += __shfl_xor(used, off, 64);
            if ((tid & 63) == 0 && used) atomicAdd(&cnt_s, used);
        }
    }
    __syncthreads();
    for (int i = tid; i < words; i += K21_LANES) {
        const int r = i / wpr;
        const uint32_t nb = hs_sm_dilate_word(ras_s, H, r, i - r * wpr);
        if (nb) ras_s[i] |= nb;                                            // (this lane's own word; the others read its hit bits, which stay)
    }
    __syncthreads();
    if (!MOMENTS && hb == 0 && tid == 0) A.acc[pair].n_ref = cnt_s;

    int b = 0, bk = 0;
    if (MOMENTS) {
        const unsigned long long best = A.acc[pair].key;                   // (the first launch's: final)
        b = (int)((uint32_t)(best >> 32) ^ 0x80000000u);
        int biy, bix;
        hs_sm_unflat(S, 0xFFFFFFFFu - (uint32_t)best, &bk, &biy, &bix);
    }

    // ---- rules 2 - 4: the headings of this block ----
    unsigned long long key = 0ull;                                         // (a node's key is never 0: its high word is at least 0x80000000)
    long long m[HS_SM_SUMS];
#pragma unroll
    for (int f = 0; f < HS_SM_SUMS; f++) m[f] = 0;
    int nq = 0;
    const bool one_chunk = P.qn <= K21_CHUNK;
    for (int k = k0; k <= k1; k++) {
        const hs_lat_heading Hd = hs_sm_heading(S, P.guess, k);
        for (int t0 = 0; t0 < NT; t0 += K21_LANES) {
            const int t = t0 + tid;
            const bool active = t < NT;
            const int ty = t / NX;
            const int dx = (t - ty * NX) - S.nx, dy = ty - S.ny;           // the lane's translation (ix, iy)
            int score = 0;
            for (int base = 0; base < P.qn; base += K21_CHUNK) {
                const int n = min(K21_CHUNK, P.qn - base);
                if (!(one_chunk && t0 > 0)) {                              // (uniform; a scan of one chunk is staged once per heading)
                    __syncthreads();                                       // (what was staged before has been walked)
                    for (int i = tid; i < n; i += K21_LANES) {
                        const float2 p = A.pool[P.qoff + base + i];
                        int gx, gy;
                        if (!hs_sm_query_cell(Hd, H, p.x, p.y, &gx, &gy)) { gx = HS_SM_IGNORED; gy = HS_SM_IGNORED; }
                        else if (MOMENTS && k == bk && t0 == 0) nq++;
                        pts_s[i] = make_int2(gx, gy);
                    }
                    __syncthreads();
                }
                if (active) {
#pragma unroll 4
                    for (int j = 0; j < n; j++) {
                        const int2 g = pts_s[j];
                        const int x = g.x + dx, y = g.y + dy;
                        const bool in = (unsigned)x < (unsigned)W && (unsigned)y < (unsigned)W;
                        const uint32_t word = ras_s[in ? y * wpr + (x >> 4) : 0];
                        score += in ? (int)((word >> (2 * (x & 15))) & 3u) : 0;
                    }
                }
            }
            if (active) {
                if (!MOMENTS) {
                    const unsigned long long kk = hs_lat_key(score, hs_sm_flat(S, k, dy, dx));
                    key = kk > key ? kk : key;
                } else if (hs_sm_in_set(score, b, S.margin)) hs_sm_moments_add(m, k, dy, dx);
            }
        }
    }

    if (!MOMENTS) {
        for (int msk = 1; msk < 64; msk <<= 1) {
            const unsigned long long o = __shfl_xor(key, msk, 64);
            key = o > key ? o : key;
        }
        if ((tid & 63) == 0) wmax_s[tid >> 6] = key;
        __syncthreads();
        if (tid == 0) {
            for (int v = 1; v < K21_LANES / 64; v++) key = wmax_s[v] > key ? wmax_s[v] : key;
            __hip_atomic_fetch_max(&A.acc[pair].key, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    } else {
#pragma unroll
        for (int f = 0; f < HS_SM_SUMS; f++) {
            long long v = m[f];
            for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
            if ((tid & 63) == 0) sum_s[tid >> 6][f] = v;
        }
        const bool mine = bk >= k0 && bk <= k1;                            // (uniform: this block staged the best heading)
        if (mine) {
            for (int off = 32; off > 0; off >>= 1) nq += __shfl_xor(nq, off, 64);
            if ((tid & 63) == 0 && nq) atomicAdd(&cnt_s, nq);              // (cnt_s: 0 since the top, not used by this launch's raster)
        }
        __syncthreads();
        if (tid < HS_SM_SUMS) {
            long long v = 0;
            for (int w = 0; w < K21_LANES / 64; w++) v += sum_s[w][tid];
            if (v) atomicAdd((unsigned long long *)&A.acc[pair].m[tid], (unsigned long long)v);     // (two's complement: a negative sum adds as it should)
        }
        if (mine && tid == 0) A.acc[pair].n_query = cnt_s;                 // (one block per pair holds the best heading)
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------
// What the unit keeps: one device block -- the pairs, then the results -- and its pinned twin.
struct hs_scanmatch {
    hs_block<unsigned char, HS_MEM_DEVICE> d_io;
    hs_block<unsigned char, HS_MEM_PINNED> h_io;
};

// rule 7 for the spec, the count and the guesses (slamhip_hs_scans_edges stops here) ...
static int32_t k21_check_args(const char *who, const slamhip_scanmatch_spec *S, const slamhip_scan_pair *pairs, int32_t n_pairs)
{
    if (!hs_sm_spec_ok(*S))
        SH_FAIL(SLAMHIP_ERR_INVALID, "%s: scale = %g finite and > 0, half = %d a multiple of 16 in [16, 192], nx = %d, ny = %d, nt = %d in [0, 64], dtheta = %g finite, "
                "margin = %d >= 0, reserved = %d zero", who, (double)S->scale, S->half, S->nx, S->ny, S->nt, (double)S->dtheta, S->margin, S->reserved);
    if (n_pairs < 1 || n_pairs > HS_SM_MAX_PAIRS) SH_FAIL(SLAMHIP_ERR_INVALID, "%s: %d pairs, must lie in [1, %d]", who, n_pairs, HS_SM_MAX_PAIRS);
    const long long nodes = hs_sm_nodes(*S);
    if (nodes > HS_SM_MAX_NODES) SH_FAIL(SLAMHIP_ERR_INVALID, "%s: %lld nodes per pair, more than 2^20", who, nodes);
    if (nodes * n_pairs > HS_SM_MAX_CALL_NODES) SH_FAIL(SLAMHIP_ERR_INVALID, "%s: %lld nodes in the call, more than 2^26", who, nodes * n_pairs);
    for (int i = 0; i < n_pairs; i++)
        for (int a = 0; a < 3; a++)
            if (!std::isfinite(pairs[i].guess[a])) SH_FAIL(SLAMHIP_ERR_INVALID, "%s: component %d of the guess of pair %d is not finite", who, a, i);
    return SLAMHIP_OK;
}
// ... and for the store of `count` scans
static int32_t k21_check(const char *who, const slamhip_scanmatch_spec *S, const slamhip_scan_pair *pairs, int32_t n_pairs, int count)
{
    SH_TRY(k21_check_args(who, S, pairs, n_pairs));
    if (count <= 0) SH_FAIL(SLAMHIP_ERR_STATE, "%s: no scan store (slamhip_hs_scans_add first)", who);
    for (int i = 0; i < n_pairs; i++)
        if (pairs[i].ref < 0 || pairs[i].ref >= count || pairs[i].query < 0 || pairs[i].query >= count)
            SH_FAIL(SLAMHIP_ERR_INVALID, "%s: pair %d names scans %d and %d of %d", who, i, pairs[i].ref, pairs[i].query, count);
    return SLAMHIP_OK;
}

// rule 5 from a pair's key and sums
static slamhip_scanmatch_result k21_result(const slamhip_scanmatch_spec &S, unsigned long long key, const long long m[HS_SM_SUMS], int n_ref, int n_query)
{
    slamhip_scanmatch_result R;
    memset(&R, 0, sizeof(R));
    hs_sm_unflat(S, hs_lat_key_flat(key), &R.k, &R.iy, &R.ix);
    R.score = hs_lat_key_score(key);
    R.n_ref = n_ref; R.n_query = n_query; R.cnt = (int32_t)m[0];
    R.sum_x = m[1]; R.sum_y = m[2]; R.sum_k = m[3];
    R.sum_xx = m[4]; R.sum_yy = m[5]; R.sum_kk = m[6];
    R.sum_xy = m[7]; R.sum_xk = m[8]; R.sum_yk = m[9];
    return R;
}

// headings per workgroup: as many blocks per pair as bring the launch to K21_TARGET_WGS workgroups, one heading at the least.  No
// result depends on it (SLAMHIP_K21_HEADINGS: tests choose it, to put a tie across two blocks and to cut the headings unevenly).
static int k21_headings_per_block(int n_pairs, int nth)
{
    const long long env = sh_env_int("SLAMHIP_K21_HEADINGS", 0);
    if (env >= 1) return (int)std::min<long long>(env, nth);
    const int blocks = std::min(std::max(sh_div_up(K21_TARGET_WGS, n_pairs), 1), nth);
    return sh_div_up(nth, blocks);
}

extern "C" int32_t slamhip_hs_scans_match(slamhip_hs *hs, const slamhip_scanmatch_spec *spec, const slamhip_scan_pair *pairs, int32_t n_pairs,
                                          slamhip_scanmatch_result *out_results)
{
    SH_CHECK_ARG(hs && spec && pairs && out_results);
    const int count = hs->scn ? (int)hs->scn->recs.size() : 0;
    SH_TRY(k21_check("slamhip_hs_scans_match", spec, pairs, n_pairs, count));
    slamhip_ctx *ctx = hs->ctx;
    SH_TRY(hs_call_begin(hs));
    SH_TRY(hs_unit<&slamhip_hs::smt>(hs));
    hs_scanmatch *u = hs->smt;
    const hs_scans *g = hs->scn;
    const size_t pair_bytes = sizeof(k21_pair) * (size_t)n_pairs, acc_bytes = sizeof(k21_acc) * (size_t)n_pairs;
    SH_TRY(u->d_io.grow(pair_bytes + acc_bytes, "slamhip_hs_scans_match"));
    SH_TRY(u->h_io.grow(pair_bytes + acc_bytes, "slamhip_hs_scans_match"));
    k21_pair *hp = (k21_pair *)u->h_io.p;
    for (int i = 0; i < n_pairs; i++) {
        const k20_scan &R = g->recs[(size_t)pairs[i].ref], &Q = g->recs[(size_t)pairs[i].query];
        k21_pair p;
        p.roff = R.off; p.rn = R.n; p.qoff = Q.off; p.qn = Q.n; p.pad = 0;
        memcpy(p.guess, pairs[i].guess, sizeof(p.guess));
        hp[i] = p;
    }
    k21_arg A;
    A.pool = g->d_pool; A.pairs = (const k21_pair *)u->d_io.p; A.acc = (k21_acc *)(u->d_io + pair_bytes);
    A.S = *spec;
    const int nth = 2 * spec->nt + 1;
    A.kb = k21_headings_per_block(n_pairs, nth);
    const dim3 grid((unsigned)sh_div_up(nth, A.kb), (unsigned)n_pairs);
    SH_HIP(hipMemcpyAsync(u->d_io, u->h_io, pair_bytes, hipMemcpyHostToDevice, ctx->stream));
    SH_HIP(hipMemsetAsync(u->d_io + pair_bytes, 0, acc_bytes, ctx->stream));
    hipLaunchKernelGGL(k21_pass<false>, grid, dim3(K21_LANES), 0, ctx->stream, A);
    SH_HIP(hipGetLastError());
    hipLaunchKernelGGL(k21_pass<true>, grid, dim3(K21_LANES), 0, ctx->stream, A);
    SH_HIP(hipGetLastError());
    SH_HIP(hipMemcpyAsync(u->h_io + pair_bytes, u->d_io + pair_bytes, acc_bytes, hipMemcpyDeviceToHost, ctx->stream));
    SH_TRY(hs_call_finish(hs));
    const k21_acc *ha = (const k21_acc *)(u->h_io + pair_bytes);
    for (int i = 0; i < n_pairs; i++) out_results[i] = k21_result(*spec, ha[i].key, ha[i].m, ha[i].n_ref, ha[i].n_query);
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_scans_edges(const slamhip_scanmatch_spec *spec, const slamhip_scan_pair *pairs, const slamhip_scanmatch_result *results,
                                          int32_t n, double *out_z, double *out_w, int32_t *out_valid)
{
    SH_CHECK_ARG(spec && pairs && results && out_z && out_w && out_valid);
    SH_TRY(k21_check_args("slamhip_hs_scans_edges", spec, pairs, n));
    for (int i = 0; i < n; i++) {
        const slamhip_scanmatch_result &R = results[i];
        if (R.k < -spec->nt || R.k > spec->nt || R.ix < -spec->nx || R.ix > spec->nx || R.iy < -spec->ny || R.iy > spec->ny || R.cnt < 0)
            SH_FAIL(SLAMHIP_ERR_INVALID, "slamhip_hs_scans_edges: result %d names node (%d, %d, %d) outside the lattice, or cnt = %d", i, R.k, R.iy, R.ix, R.cnt);
    }
    for (int i = 0; i < n; i++) hs_sm_edge(*spec, pairs[i], results[i], out_z + 3 * (size_t)i, out_w + 3 * (size_t)i, out_valid + i);
    return SLAMHIP_OK;
}

// CPU-side test hook: hs_scanmatch.h -- the text the kernel runs -- in plain loops
extern "C" int32_t slamhip_debug_scans_match(const float *xy, const int32_t *offsets, int32_t N, const slamhip_scanmatch_spec *spec,
                                             const slamhip_scan_pair *pairs, int32_t n_pairs, slamhip_scanmatch_result *out_results)
{
    SH_CHECK_ARG(spec && pairs && out_results && N >= 0 && (N == 0 || offsets));
    if (N) {
        if (offsets[0] != 0) SH_FAIL(SLAMHIP_ERR_INVALID, "scans match: offsets[0] = %d must be 0", offsets[0]);
        for (int k = 0; k < N; k++)
            if (offsets[k + 1] < offsets[k]) SH_FAIL(SLAMHIP_ERR_INVALID, "scans match: offsets[%d] = %d below offsets[%d] = %d", k + 1, offsets[k + 1], k, offsets[k]);
        SH_CHECK_ARG(xy || offsets[N] == 0);
    }
    SH_TRY(k21_check("scans match", spec, pairs, n_pairs, N));
    const slamhip_scanmatch_spec S = *spec;
    const int H = S.half, wpr = hs_sm_wpr(H), W = 2 * H;
    const int nth = 2 * S.nt + 1;
    std::vector<uint32_t> ras((size_t)W * wpr);
    std::vector<int> cells, scores((size_t)hs_sm_nodes(S)), used((size_t)nth);
    for (int p = 0; p < n_pairs; p++) {
        const slamhip_scan_pair &P = pairs[p];
        std::fill(ras.begin(), ras.end(), 0u);
        int n_ref = 0;
        for (int i = offsets[P.ref]; i < offsets[P.ref + 1]; i++) {        // rule 1
            int x, y;
            if (!hs_sm_ref_cell(xy[2 * (size_t)i], xy[2 * (size_t)i + 1], S.scale, H, &x, &y)) continue;
            n_ref++;
            if ((unsigned)x < (unsigned)W && (unsigned)y < (unsigned)W) ras[(size_t)y * wpr + (x >> 4)] |= hs_sm_hit_bit(x);
        }
        for (int r = 0; r < W; r++)
            for (int j = 0; j < wpr; j++) ras[(size_t)r * wpr + j] |= hs_sm_dilate_word(ras.data(), H, r, j);
        const int q0 = offsets[P.query], qn = offsets[P.query + 1] - q0;
        unsigned long long best = 0ull;
        for (int k = -S.nt; k <= S.nt; k++) {                              // rules 2 and 3
            const hs_lat_heading Hd = hs_sm_heading(S, P.guess, k);
            cells.clear();
            for (int i = 0; i < qn; i++) {
                int gx, gy;
                if (hs_sm_query_cell(Hd, H, xy[2 * (size_t)(q0 + i)], xy[2 * (size_t)(q0 + i) + 1], &gx, &gy)) { cells.push_back(gx); cells.push_back(gy); }
            }
            used[(size_t)(k + S.nt)] = (int)cells.size() / 2;
            for (int iy = -S.ny; iy <= S.ny; iy++)
                for (int ix = -S.nx; ix <= S.nx; ix++) {
                    int score = 0;
                    for (size_t c = 0; c < cells.size(); c += 2) score += hs_sm_val(ras.data(), H, cells[c] + ix, cells[c + 1] + iy);
                    const uint32_t flat = hs_sm_flat(S, k, iy, ix);
                    scores[flat] = score;
                    const unsigned long long key = hs_lat_key(score, flat);
                    if (key > best) best = key;
                }
        }
        const int b = hs_lat_key_score(best);
        long long m[HS_SM_SUMS] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
        for (int k = -S.nt; k <= S.nt; k++)                                // rule 4
            for (int iy = -S.ny; iy <= S.ny; iy++)
                for (int ix = -S.nx; ix <= S.nx; ix++)
                    if (hs_sm_in_set(scores[hs_sm_flat(S, k, iy, ix)], b, S.margin)) hs_sm_moments_add(m, k, iy, ix);
        int bk, biy, bix;
        hs_sm_unflat(S, hs_lat_key_flat(best), &bk, &biy, &bix);
        out_results[p] = k21_result(S, best, m, n_ref, used[(size_t)(bk + S.nt)]);
    }
    return SLAMHIP_OK;
}
