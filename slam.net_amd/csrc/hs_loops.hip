// hs_loops.hip -- K23, the consistent set of loop edges (slamhip_hs_loops_consistent, slamhip_hs_loops_clear,
// slamhip_debug_loops_consistent).  No reference counterpart.  Definition: include/slamhip.h (slamhip_hs_loops_consistent); the
// arithmetic host and device share: hs_loops.h.
//
// Five launches per call on the operator's stream:
//  * k23_edges: a lane per edge forms rule 1's record from the edge and its two poses (gathered by the host: N never reaches the device).
//  * k23_pairs: grid (blocks of 256 columns, tiles of 64 rows), 256 lanes.  The tile's 64 row records are staged in LDS (7 KB); a lane
//    keeps the record of its column b in registers and walks the rows, each row record read as a broadcast; the wavefront's ballot of
//    the test is the row's word, stored once by lane 0.  Every pair is tested twice, once from each side, by the same call of
//    hs_lp_d2 on (min, max): the matrix is symmetric by construction.  Every word of the matrix is written: no clear, no atomics.
//  * k23_degree: ONE workgroup of 1024 lanes; a lane per row sums the popcounts of its words, then R rounds of a workgroup maximum of
//    the packed keys (deg << 32) | (0xFFFFFFFF - v) in LDS name the starts.  It leaves n_pairs, n_used and R in the info record.
//  * k23_clique<RESIDENT>: a workgroup of 1024 lanes per start.  S and Q are bit rows in LDS; a round gives every v of S to a lane,
//    which sums popcount(adj[v] & S) over the words, and takes the maximum of the packed keys (shuffles, then the waves' maxima
//    through LDS); lanes k < W then AND row v into S.  RESIDENT: the whole matrix is copied to LDS first, its rows padded to an odd
//    number of words (a lane per row: consecutive rows on different banks); it is chosen where those rows take at most 144 KB
//    (hs_lp_resident: L <= 1084), else rows are read from global memory, which the L2 holds (2 MB at L = 4096).
//  * k23_finish: ONE workgroup; rule 6.
// No workgroup waits on another; integers throughout behind d2 <= gamma: no result depends on the grid or on RESIDENT.
#include "hs_blocks.h"
#include "hs_loops.h"
#include <algorithm>
#include <cmath>
#include <vector>

#define K23_LANES 256                      // k23_edges, k23_pairs, k23_finish
#define K23_ROWS 64                        // rows of a k23_pairs tile
#define K23_WIDE 1024                      // k23_degree, k23_clique
#define K23_REC_WORDS (sizeof(hs_lp_rec) / 8)
static_assert(sizeof(hs_lp_in) == 112 && sizeof(hs_lp_rec) == 112 && sizeof(slamhip_loops_spec) == 40 && sizeof(slamhip_loops_info) == 32,
              "the records the kernels read and write");

struct k23_arg {
    const hs_lp_in *in; hs_lp_rec *rec; hs_lp_u64 *adj; int32_t *deg; int32_t *starts; int32_t *qsize; hs_lp_u64 *qbits;
    uint8_t *keep; slamhip_loops_info *info;
    int L, W, R;                           // R: rule 4's count, known to the host from the use bytes
    slamhip_loops_spec S;
};

__global__ void __launch_bounds__(K23_LANES) k23_edges(const k23_arg A)
{
    const int a = blockIdx.x * K23_LANES + threadIdx.x;
    if (a >= A.L) return;
    hs_lp_rec R;
    hs_lp_edge(A.in[a], &R);
    A.rec[a] = R;
}

__global__ void __launch_bounds__(K23_LANES) k23_pairs(const k23_arg A)
{
    __shared__ hs_lp_rec row_s[K23_ROWS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int b = blockIdx.x * K23_LANES + tid, row0 = blockIdx.y * K23_ROWS;
    const int rows = min(K23_ROWS, A.L - row0);
    {
        const hs_lp_u64 *src = (const hs_lp_u64 *)(A.rec + row0);
        hs_lp_u64 *dst = (hs_lp_u64 *)row_s;
        for (int k = tid; k < rows * (int)K23_REC_WORDS; k += K23_LANES) dst[k] = src[k];
    }
    const hs_lp_rec C = A.rec[min(b, A.L - 1)];                             // (a column past L reads the last record; its bit is 0)
    __syncthreads();
    const int word = b >> 6;                                               // (uniform over the wavefront)
    if (word >= A.W) return;
    const double q_t = A.S.q_t, q_theta = A.S.q_theta, gamma = A.S.gamma;
    for (int k = 0; k < rows; k++) {
        const int a = row0 + k;
        const bool bit = b < A.L && a != b && hs_lp_bit(row_s[k], a, C, b, q_t, q_theta, gamma);
        const hs_lp_u64 m = __ballot(bit);
        if (lane == 0) A.adj[(size_t)a * A.W + word] = m;
    }
}

// the workgroup's maximum of a packed key, in every lane (wmax_s: K23_WIDE / 64 words; the caller's barrier follows before it is written again)
__device__ static inline hs_lp_u64 k23_wg_max(hs_lp_u64 key, hs_lp_u64 *wmax_s)
{
    for (int msk = 1; msk < 64; msk <<= 1) {
        const hs_lp_u64 o = __shfl_xor(key, msk, 64);
        key = o > key ? o : key;
    }
    if ((threadIdx.x & 63) == 0) wmax_s[threadIdx.x >> 6] = key;
    __syncthreads();
    for (int v = 0; v < K23_WIDE / 64; v++) key = wmax_s[v] > key ? wmax_s[v] : key;
    return key;
}

__global__ void __launch_bounds__(K23_WIDE) k23_degree(const k23_arg A)
{
    __shared__ hs_lp_u64 key_s[HS_LP_MAX_EDGES];
    __shared__ hs_lp_u64 wmax_s[K23_WIDE / 64];
    __shared__ long long pairs_s[K23_WIDE / 64];
    __shared__ int used_s[K23_WIDE / 64];
    const int tid = threadIdx.x;
    long long pairs = 0; int used = 0;
    for (int v = tid; v < A.L; v += K23_WIDE) {                            // rule 3
        const hs_lp_u64 *row = A.adj + (size_t)v * A.W;
        int d = 0;
        for (int k = 0; k < A.W; k++) d += hs_lp_popc(row[k]);
        A.deg[v] = d;
        const int u = A.rec[v].use;
        key_s[v] = u ? hs_lp_key(d, v) : 0ull;
        pairs += d; used += u;
    }
    for (int off = 32; off > 0; off >>= 1) { pairs += __shfl_xor(pairs, off, 64); used += __shfl_xor(used, off, 64); }
    if ((tid & 63) == 0) { pairs_s[tid >> 6] = pairs; used_s[tid >> 6] = used; }
    __syncthreads();
    pairs = 0; used = 0;
    for (int v = 0; v < K23_WIDE / 64; v++) { pairs += pairs_s[v]; used += used_s[v]; }
    const int R = min(A.S.n_starts, used);                                 // rule 4 (uniform; equals A.R)
    if (tid == 0) { A.info->n_pairs = pairs / 2; A.info->n_used = used; A.info->n_starts = R; }
    for (int r = 0; r < R; r++) {
        hs_lp_u64 key = 0ull;
        for (int v = tid; v < A.L; v += K23_WIDE) key = key_s[v] > key ? key_s[v] : key;
        key = k23_wg_max(key, wmax_s);                                     // (never 0: fewer than `used` keys have been taken)
        __syncthreads();
        if (tid == 0 && key != 0ull) { const int v = hs_lp_key_index(key); A.starts[r] = v; key_s[v] = 0ull; }
        __syncthreads();
    }
}

template <bool RESIDENT>
__global__ void __launch_bounds__(K23_WIDE) k23_clique(const k23_arg A)
{
    extern __shared__ __attribute__((aligned(16))) hs_lp_u64 k23_lds[];
    hs_lp_u64 *S_s = k23_lds, *Q_s = k23_lds + HS_LP_MAX_WORDS, *wmax_s = k23_lds + 2 * HS_LP_MAX_WORDS;
    hs_lp_u64 *adj_s = k23_lds + 2 * HS_LP_MAX_WORDS + K23_WIDE / 64;
    const int tid = threadIdx.x, r = blockIdx.x, L = A.L, W = A.W;
    const int Wp = RESIDENT ? hs_lp_stride(L) : W;
    const hs_lp_u64 *M = RESIDENT ? adj_s : A.adj;
    const int v0 = A.starts[r];
    if (RESIDENT)
        for (int k = tid; k < L * W; k += K23_WIDE) {
            const int row = k / W;
            adj_s[row * Wp + (k - row * W)] = A.adj[k];
        }
    if (tid < W) {                                                         // rule 5: Q = {v0}, S = adj[v0]
        S_s[tid] = A.adj[(size_t)v0 * W + tid];
        Q_s[tid] = tid == (v0 >> 6) ? 1ull << (v0 & 63) : 0ull;
    }
    __syncthreads();
    int size = 1;
    for (;;) {
        hs_lp_u64 key = 0ull;
        for (int v = tid; v < L; v += K23_WIDE) {
            if (!((S_s[v >> 6] >> (v & 63)) & 1ull)) continue;
            const hs_lp_u64 *row = M + (size_t)v * Wp;
            int g = 0;
            for (int k = 0; k < W; k++) g += hs_lp_popc(row[k] & S_s[k]);
            const hs_lp_u64 kk = hs_lp_key(g, v);
            key = kk > key ? kk : key;
        }
        key = k23_wg_max(key, wmax_s);
        if (key == 0ull) break;                                            // (uniform: S is empty)
        const int v = hs_lp_key_index(key);
        __syncthreads();                                                   // (S and the waves' maxima have been read)
        if (tid < W) {
            S_s[tid] &= M[(size_t)v * Wp + tid];                           // (the diagonal is 0: v leaves S)
            if (tid == (v >> 6)) Q_s[tid] |= 1ull << (v & 63);
        }
        size++;
        __syncthreads();
    }
    if (tid < W) A.qbits[(size_t)r * W + tid] = Q_s[tid];
    if (tid == 0) A.qsize[r] = size;
}

__global__ void __launch_bounds__(K23_LANES) k23_finish(const k23_arg A)
{
    __shared__ int best_s[2];
    const int tid = threadIdx.x;
    if (tid == 0) {                                                        // rule 6: the largest, ties to the lower rank
        int bs = 0, br = -1;
        for (int r = 0; r < A.R; r++)
            if (A.qsize[r] > bs) { bs = A.qsize[r]; br = r; }
        best_s[0] = bs; best_s[1] = br;
        A.info->size = bs; A.info->rank = br; A.info->start = br >= 0 ? A.starts[br] : -1; A.info->reserved = 0;
    }
    __syncthreads();
    const int bs = best_s[0], br = best_s[1];
    const bool any = br >= 0 && bs >= A.S.min_clique;
    for (int v = tid; v < A.L; v += K23_LANES)
        A.keep[v] = any ? (uint8_t)((A.qbits[(size_t)br * A.W + (v >> 6)] >> (v & 63)) & 1ull) : (uint8_t)0;
}

// ---- host side ---------------------------------------------------------------------------------------------------
// What the unit keeps: one device block -- the edges, the records, the searches' rows, then the results -- and its pinned twin of
// the edges and the results.
struct hs_loops {
    hs_block<unsigned char, HS_MEM_DEVICE> d_io;
    hs_block<unsigned char, HS_MEM_PINNED> h_io;
};

// rule 7
static int32_t k23_check(const char *who, const double *poses, int32_t N, const int32_t *ij, const double *z, const double *w, int32_t L,
                         const slamhip_loops_spec *sp, const uint64_t *out_adj)
{
    if (L < 1 || L > HS_LP_MAX_EDGES) SH_FAIL(SLAMHIP_ERR_INVALID, "%s: L = %d must lie in [1, %d]", who, L, HS_LP_MAX_EDGES);
    if (N < 1 || N > HS_LP_MAX_NODES) SH_FAIL(SLAMHIP_ERR_INVALID, "%s: N = %d must lie in [1, 2^20]", who, N);
    if (!hs_lp_spec_ok(sp))
        SH_FAIL(SLAMHIP_ERR_INVALID, "%s: gamma = %g, q_t = %g, q_theta = %g finite and >= 0, n_starts = %d in [1, %d], min_clique = %d >= 1, flags = %d in {0, %d}, "
                "reserved = %d zero", who, sp->gamma, sp->q_t, sp->q_theta, sp->n_starts, HS_LP_MAX_STARTS, sp->min_clique, sp->flags, SLAMHIP_LOOPS_ADJ, sp->reserved);
    if ((sp->flags & SLAMHIP_LOOPS_ADJ) && !out_adj) SH_FAIL(SLAMHIP_ERR_INVALID, "%s: SLAMHIP_LOOPS_ADJ without out_adj", who);
    for (int n = 0; n < N; n++) {
        const double *p = poses + 3 * (size_t)n;
        if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !(fabs(p[2]) <= HS_LP_MAX_THETA))
            SH_FAIL(SLAMHIP_ERR_INVALID, "%s: node %d = (%g, %g, %g) must be finite with |theta| <= 32768", who, n, p[0], p[1], p[2]);
    }
    for (int e = 0; e < L; e++) {
        const int i = ij[2 * (size_t)e], j = ij[2 * (size_t)e + 1];
        if (i < 0 || i >= N || j < 0 || j >= N) SH_FAIL(SLAMHIP_ERR_INVALID, "%s: edge %d = (%d, %d) of %d nodes", who, e, i, j, N);
        for (int a = 0; a < 3; a++) {
            const double zz = z[3 * (size_t)e + a], ww = w[3 * (size_t)e + a];
            if (!std::isfinite(zz) || (a == 2 && !(fabs(zz) <= HS_LP_MAX_THETA)))
                SH_FAIL(SLAMHIP_ERR_INVALID, "%s: edge %d has a measurement that is not finite, or a heading above 32768", who, e);
            if (!std::isfinite(ww) || !(ww > 0.0)) SH_FAIL(SLAMHIP_ERR_INVALID, "%s: edge %d has the weight %g: it must be finite and > 0", who, e, ww);
        }
    }
    return SLAMHIP_OK;
}

// an edge with its two poses, as k23_edges and the hook read it
static inline hs_lp_in k23_gather(const double *poses, const int32_t *ij, const double *z, const double *w, const uint8_t *use, int e)
{
    hs_lp_in E;
    E.i = ij[2 * (size_t)e]; E.j = ij[2 * (size_t)e + 1];
    E.use = use ? use[e] != 0 : 1; E.pad = 0;
    memcpy(E.pi, poses + 3 * (size_t)E.i, sizeof(E.pi));
    memcpy(E.pj, poses + 3 * (size_t)E.j, sizeof(E.pj));
    memcpy(E.z, z + 3 * (size_t)e, sizeof(E.z));
    memcpy(E.w, w + 3 * (size_t)e, sizeof(E.w));
    return E;
}

static inline size_t k23_up8(size_t n) { return (n + 7) & ~(size_t)7; }

extern "C" int32_t slamhip_hs_loops_consistent(slamhip_hs *hs, const double *poses, int32_t N, const int32_t *ij, const double *z, const double *w,
                                               const uint8_t *use, int32_t L, const slamhip_loops_spec *spec, uint8_t *out_keep, int32_t *out_deg,
                                               slamhip_loops_info *out_info, uint64_t *out_adj)
{
    SH_CHECK_ARG(hs && poses && ij && z && w && spec && out_keep && out_deg && out_info);
    SH_TRY(k23_check("slamhip_hs_loops_consistent", poses, N, ij, z, w, L, spec, out_adj));
    slamhip_ctx *ctx = hs->ctx;
    SH_TRY(hs_call_begin(hs));
    SH_TRY(hs_unit<&slamhip_hs::lps>(hs));
    hs_loops *u = hs->lps;
    const int W = hs_lp_words(L);
    const bool want_adj = (spec->flags & SLAMHIP_LOOPS_ADJ) != 0;
    const bool resident = hs_lp_resident(L) && !sh_env_set("SLAMHIP_K23_GLOBAL");
    // the device block: edges | records | starts | sizes | the searches' Q rows | info | deg | keep | matrix -- the last four are what comes back
    const size_t in_bytes = sizeof(hs_lp_in) * (size_t)L, rec_bytes = sizeof(hs_lp_rec) * (size_t)L;
    const size_t idx_bytes = sizeof(int32_t) * HS_LP_MAX_STARTS, q_bytes = 8 * (size_t)HS_LP_MAX_STARTS * W;
    const size_t deg_bytes = k23_up8(sizeof(int32_t) * (size_t)L), keep_bytes = k23_up8((size_t)L), adj_bytes = 8 * (size_t)L * W;
    const size_t o_rec = in_bytes, o_starts = o_rec + rec_bytes, o_qsize = o_starts + idx_bytes, o_qbits = o_qsize + idx_bytes;
    const size_t o_info = o_qbits + q_bytes, o_deg = o_info + sizeof(slamhip_loops_info), o_keep = o_deg + deg_bytes, o_adj = o_keep + keep_bytes;
    const size_t res_bytes = (o_adj - o_info) + (want_adj ? adj_bytes : 0);
    SH_TRY(u->d_io.grow(o_adj + adj_bytes, "slamhip_hs_loops_consistent"));
    SH_TRY(u->h_io.grow(in_bytes + (o_adj - o_info) + adj_bytes, "slamhip_hs_loops_consistent"));
    hs_lp_in *hin = (hs_lp_in *)u->h_io.p;
    int n_used = 0;
    for (int e = 0; e < L; e++) { hin[e] = k23_gather(poses, ij, z, w, use, e); n_used += hin[e].use; }
    k23_arg A;
    A.in = (const hs_lp_in *)u->d_io.p; A.rec = (hs_lp_rec *)(u->d_io + o_rec); A.starts = (int32_t *)(u->d_io + o_starts);
    A.qsize = (int32_t *)(u->d_io + o_qsize); A.qbits = (hs_lp_u64 *)(u->d_io + o_qbits); A.info = (slamhip_loops_info *)(u->d_io + o_info);
    A.deg = (int32_t *)(u->d_io + o_deg); A.keep = (uint8_t *)(u->d_io + o_keep); A.adj = (hs_lp_u64 *)(u->d_io + o_adj);
    A.L = L; A.W = W; A.R = std::min(spec->n_starts, n_used); A.S = *spec;
    const size_t lds = 8 * (size_t)(2 * HS_LP_MAX_WORDS + K23_WIDE / 64) + (resident ? 8 * (size_t)L * hs_lp_stride(L) : 0);
    if (resident && A.R > 0)
        SH_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k23_clique<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    SH_HIP(hipMemcpyAsync(u->d_io, u->h_io, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k23_edges, dim3((unsigned)sh_div_up(L, K23_LANES)), dim3(K23_LANES), 0, ctx->stream, A);
    SH_HIP(hipGetLastError());
    hipLaunchKernelGGL(k23_pairs, dim3((unsigned)sh_div_up(L, K23_LANES), (unsigned)sh_div_up(L, K23_ROWS)), dim3(K23_LANES), 0, ctx->stream, A);
    SH_HIP(hipGetLastError());
    hipLaunchKernelGGL(k23_degree, dim3(1), dim3(K23_WIDE), 0, ctx->stream, A);
    SH_HIP(hipGetLastError());
    if (A.R > 0) {
        if (resident) hipLaunchKernelGGL(k23_clique<true>, dim3((unsigned)A.R), dim3(K23_WIDE), lds, ctx->stream, A);
        else hipLaunchKernelGGL(k23_clique<false>, dim3((unsigned)A.R), dim3(K23_WIDE), lds, ctx->stream, A);
        SH_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k23_finish, dim3(1), dim3(K23_LANES), 0, ctx->stream, A);
    SH_HIP(hipGetLastError());
    unsigned char *hres = u->h_io + in_bytes;
    SH_HIP(hipMemcpyAsync(hres, u->d_io + o_info, res_bytes, hipMemcpyDeviceToHost, ctx->stream));
    SH_TRY(hs_call_finish(hs));
    memcpy(out_info, hres, sizeof(slamhip_loops_info));
    memcpy(out_deg, hres + (o_deg - o_info), sizeof(int32_t) * (size_t)L);
    memcpy(out_keep, hres + (o_keep - o_info), (size_t)L);
    if (want_adj) memcpy(out_adj, hres + (o_adj - o_info), adj_bytes);
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_loops_clear(slamhip_hs *hs)
{
    SH_CHECK_ARG(hs);
    SH_HIP(hipSetDevice(hs->ctx->device));
    SH_HIP(hipStreamSynchronize(hs->ctx->stream));
    hs_unit_drop<&slamhip_hs::lps>(hs);
    return SLAMHIP_OK;
}

// CPU-side test hook: hs_loops.h -- the text the kernels run -- in plain loops
extern "C" int32_t slamhip_debug_loops_consistent(const double *poses, int32_t N, const int32_t *ij, const double *z, const double *w,
                                                  const uint8_t *use, int32_t L, const slamhip_loops_spec *spec, uint8_t *out_keep, int32_t *out_deg,
                                                  slamhip_loops_info *out_info, uint64_t *out_adj, double *out_d2)
{
    SH_CHECK_ARG(poses && ij && z && w && spec && out_keep && out_deg && out_info);
    SH_TRY(k23_check("loops consistent", poses, N, ij, z, w, L, spec, out_adj));
    const slamhip_loops_spec S = *spec;
    const int W = hs_lp_words(L);
    std::vector<hs_lp_rec> rec((size_t)L);
    int n_used = 0;
    for (int e = 0; e < L; e++) {                                          // rule 1
        hs_lp_edge(k23_gather(poses, ij, z, w, use, e), &rec[(size_t)e]);
        n_used += rec[(size_t)e].use;
    }
    std::vector<hs_lp_u64> adj((size_t)L * W, 0ull);
    for (int a = 0; a < L; a++)                                            // rule 2
        for (int b = 0; b < L; b++) {
            if (a == b) { if (out_d2) out_d2[(size_t)a * L + b] = 0.0; continue; }
            if (out_d2) out_d2[(size_t)a * L + b] = a < b ? hs_lp_d2(rec[(size_t)a], rec[(size_t)b], S.q_t, S.q_theta) : hs_lp_d2(rec[(size_t)b], rec[(size_t)a], S.q_t, S.q_theta);
            if (hs_lp_bit(rec[(size_t)a], a, rec[(size_t)b], b, S.q_t, S.q_theta, S.gamma)) adj[(size_t)a * W + (b >> 6)] |= 1ull << (b & 63);
        }
    long long pairs = 0;
    std::vector<hs_lp_u64> keys((size_t)L);
    for (int v = 0; v < L; v++) {                                          // rule 3
        int d = 0;
        for (int k = 0; k < W; k++) d += hs_lp_popc(adj[(size_t)v * W + k]);
        out_deg[v] = d;
        pairs += d;
        keys[(size_t)v] = rec[(size_t)v].use ? hs_lp_key(d, v) : 0ull;
    }
    const int R = std::min(S.n_starts, n_used);
    std::vector<hs_lp_u64> Sb((size_t)W), Q((size_t)W), bestQ((size_t)W, 0ull);
    int bs = 0, br = -1, bstart = -1;
    for (int r = 0; r < R; r++) {
        hs_lp_u64 key = 0ull;                                              // rule 4
        for (int v = 0; v < L; v++) key = keys[(size_t)v] > key ? keys[(size_t)v] : key;
        const int v0 = hs_lp_key_index(key);
        keys[(size_t)v0] = 0ull;
        for (int k = 0; k < W; k++) { Sb[(size_t)k] = adj[(size_t)v0 * W + k]; Q[(size_t)k] = 0ull; }   // rule 5
        Q[(size_t)(v0 >> 6)] = 1ull << (v0 & 63);
        int size = 1;
        for (;;) {
            hs_lp_u64 best = 0ull;
            for (int v = 0; v < L; v++) {
                if (!((Sb[(size_t)(v >> 6)] >> (v & 63)) & 1ull)) continue;
                int g = 0;
                for (int k = 0; k < W; k++) g += hs_lp_popc(adj[(size_t)v * W + k] & Sb[(size_t)k]);
                const hs_lp_u64 kk = hs_lp_key(g, v);
                best = kk > best ? kk : best;
            }
            if (best == 0ull) break;
            const int v = hs_lp_key_index(best);
            for (int k = 0; k < W; k++) Sb[(size_t)k] &= adj[(size_t)v * W + k];
            Q[(size_t)(v >> 6)] |= 1ull << (v & 63);
            size++;
        }
        if (size > bs) { bs = size; br = r; bstart = v0; bestQ = Q; }      // rule 6
    }
    const bool any = br >= 0 && bs >= S.min_clique;
    for (int v = 0; v < L; v++) out_keep[v] = any ? (uint8_t)((bestQ[(size_t)(v >> 6)] >> (v & 63)) & 1ull) : (uint8_t)0;
    slamhip_loops_info I;
    I.n_pairs = pairs / 2; I.n_used = n_used; I.size = bs; I.start = bstart; I.rank = br; I.n_starts = R; I.reserved = 0;
    *out_info = I;
    if (out_adj) memcpy(out_adj, adj.data(), 8 * (size_t)L * W);
    return SLAMHIP_OK;
}
