// hs_sig.hip -- K18, rotation-invariant signatures of scans and a device-resident store of keyframe signatures for loop candidates:
// the signature of a scan (rings x 64 sectors of occupied cells round the sensor, a 64-bit word per ring, so that a turn of the
// scan by one sector is a rotate of every word by one bit), the store, the search of one scan against the store over all 64
// headings and the search of the store against itself (slamhip_hs_sig_configure, _sig_add, _sig_add_scans, _sig_query, _sig_self,
// _sig_count, _sig_download, _sig_upload, _sig_set_poses, _sig_clear, slamhip_debug_sig_table, _sig, _sig_ring, _sig_sector, _sig_search).  No
// reference counterpart.  Definition: include/slamhip.h (slamhip_hs_sig_add); the arithmetic host and device share: hs_sig.h.
//
// The store: blocks of 64 keyframes; within a block ring r of the 64 keyframes is contiguous (sig[block][r][64], hs_sig_at), so a
// wavefront that holds a key per lane loads a ring as 512 contiguous bytes, and a store that grows appends blocks -- the old ones are
// copied as they are.  n_set is a uint16 array beside the blocks; the poses stay on the host.
//  * k18_sig: a workgroup of 256 lanes per scan, a point per lane and pass; the table and the n_ring words in LDS, the words filled by
//    64-bit LDS atomic OR, the counts by ballot; the words go to the store with their popcount and / or to a key-major array.
//  * k18_query<RG>: a key per lane (RG: n_ring rounded up to a multiple of 8; the key's words in registers, zero beyond n_ring).  The
//    64 rotations of the query lie in LDS (64 x RG words) and are read as broadcasts; the lane keeps (inter, shift), ties to the
//    smaller s, and divides once.  Each wavefront's B best by repeated arg-max on hs_sig_rank, then the workgroup's B best of those
//    (4 x 16 candidates: a lane each).  k18_query_finish, one workgroup, picks the B best of all workgroups' lists.
//  * k18_self<RG>: the grid is (tile of 64 queries, tile of 64 keys); a tile pair no query of which may see a key of leaves at once.
//    The key tile lies in LDS; a query per lane rotates its own words in registers (64 rotates by one bit are the identity, so the
//    words serve every key); the four wavefronts share the tile's keys.  The best per query is merged by a 64-bit agent-scope atomic
//    max on hs_sig_pack; k18_self_finish unpacks the winners and forms inter and uni again.
// Integers throughout: every order of atomics and reductions gives the same bits.
#include "hs_blocks.h"
#include "hs_sig.h"
#include <algorithm>
#include <vector>

#define K18_LANES 256

static_assert(sizeof(slamhip_sig_hit) == 16 && sizeof(slamhip_sig_info) == 16 && sizeof(slamhip_sig_spec) == 12, "the records of include/slamhip.h");
static_assert(SLAMHIP_SIG_SECTORS == HS_SG_SECTORS && HS_SG_BLOCK == 64 && HS_SG_MAX_B == 16, "a ring is a word, a block a wavefront, 4 x 16 candidates a wavefront");
static_assert(HS_SG_PK_VALID_BIT < 64 && (1 << HS_SG_PK_INDEX_BITS) == HS_SG_MAX_KEYS && (1 << (HS_SG_PK_SCORE_BITS - 1)) == 65536, "the packed key's fields");

typedef unsigned long long k18_u64;

struct k18_sig_arg {
    const float2 *pts; const int32_t *offsets; int n;      // offsets: nullptr -- one scan of n points -- or scans + 1 entries
    float scale; int n_ring, ring_cells;
    const int32_t *cs;                                     // C[64], S[64]
    k18_u64 *store; uint16_t *nset; int first;             // nullptr: nothing is appended; else scan b becomes keyframe first + b
    k18_u64 *lin;                                          // nullptr, or [scans][n_ring]
    int32_t *info;                                         // nullptr, or [scans][4]
};

__global__ void __launch_bounds__(K18_LANES) k18_sig(const k18_sig_arg A)
{
    __shared__ int32_t cs_s[2 * HS_SG_SECTORS];
    __shared__ k18_u64 sig_s[HS_SG_MAX_RING];
    __shared__ int cnt_s[K18_LANES / 64][2];
    const int tid = threadIdx.x, scan = blockIdx.x;
    const int p0 = A.offsets ? A.offsets[scan] : 0;
    const int n = A.offsets ? A.offsets[scan + 1] - p0 : A.n;
    if (tid < 2 * HS_SG_SECTORS) cs_s[tid] = A.cs[tid];
    if (tid < HS_SG_MAX_RING) sig_s[tid] = 0ull;
    __syncthreads();
    int n_ign = 0, n_far = 0;                                              // (the same in every lane of a wavefront)
    for (int base = 0; base < n; base += K18_LANES) {
        const int i = base + tid;
        bool ign = false, far = false;
        if (i < n) {
            const float2 p = A.pts[p0 + i];
            int u, v;
            if (!hs_sig_cell(p.x, p.y, A.scale, &u, &v)) ign = true;
            else {
                const int ring = hs_sig_ring(u * u + v * v, A.n_ring, A.ring_cells);
                if (ring == A.n_ring) far = true;
                else atomicOr(&sig_s[ring], 1ull << hs_sig_sector(cs_s, u, v));
            }
        }
        n_ign += (int)__popcll(__ballot(ign));
        n_far += (int)__popcll(__ballot(far));
    }
    if ((tid & 63) == 0) { cnt_s[tid >> 6][0] = n_ign; cnt_s[tid >> 6][1] = n_far; }
    __syncthreads();
    if (tid < 64) {
        const k18_u64 w = tid < A.n_ring ? sig_s[tid] : 0ull;
        int total = (int)__popcll(w);
        for (int off = 32; off > 0; off >>= 1) total += __shfl_xor(total, off, 64);
        if (tid < A.n_ring) {
            if (A.store) A.store[hs_sig_at(A.first + scan, tid, A.n_ring)] = w;
            if (A.lin) A.lin[(size_t)scan * A.n_ring + tid] = w;
        }
        if (tid == 0) {
            if (A.store) A.nset[A.first + scan] = (uint16_t)total;
            if (A.info) {
                int ig = 0, fr = 0;
                for (int wv = 0; wv < K18_LANES / 64; wv++) { ig += cnt_s[wv][0]; fr += cnt_s[wv][1]; }
                int32_t *o = A.info + 4 * (size_t)scan;
                o[0] = n; o[1] = ig; o[2] = fr; o[3] = total;
            }
        }
    }
}

// the wavefront's largest key (0: none)
__device__ static inline k18_u64 k18_wave_max(k18_u64 key)
{
    for (int off = 32; off > 0; off >>= 1) {
        const k18_u64 o = __shfl_xor(key, off, 64);
        key = o > key ? o : key;
    }
    return key;
}
__device__ static inline k18_u64 k18_hit_rank(const slamhip_sig_hit &h) { return h.index >= 0 ? hs_sig_rank(h.score, h.index) : 0ull; }

struct k18_query_arg {
    const k18_u64 *store; const uint16_t *nset; int n_ring;
    int first, last, base;                                 // base: first rounded down to a block
    const k18_u64 *q; const int32_t *qinfo;                // the query's words and its slamhip_sig_info
    int B;
    slamhip_sig_hit *part;                                 // [workgroups][B]
};

template <int RG>
__global__ void __launch_bounds__(K18_LANES) k18_query(const k18_query_arg A)
{
    __shared__ k18_u64 rot_s[HS_SG_SECTORS * RG];
    __shared__ slamhip_sig_hit cand_s[(K18_LANES / 64) * HS_SG_MAX_B];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < HS_SG_SECTORS * RG; i += K18_LANES) {
        const int s = i / RG, r = i - s * RG;
        rot_s[i] = r < A.n_ring ? hs_sig_rotr(A.q[r], s) : 0ull;
    }
    if (tid < (K18_LANES / 64) * HS_SG_MAX_B) cand_s[tid] = hs_sig_no_hit();
    const int g = A.base + (int)blockIdx.x * K18_LANES + tid;
    const bool valid = g >= A.first && g < A.last;
    k18_u64 kw[RG];
#pragma unroll
    for (int r = 0; r < RG; r++) kw[r] = (valid && r < A.n_ring) ? A.store[hs_sig_at(g, r, A.n_ring)] : 0ull;
    __syncthreads();
    int best = -1, shift = 0;
    for (int s = 0; s < HS_SG_SECTORS; s++) {
        const k18_u64 *rq = rot_s + s * RG;                                // (the same words in every lane: broadcasts)
        int inter = 0;
#pragma unroll
        for (int r = 0; r < RG; r++) inter += (int)__popcll(kw[r] & rq[r]);
        if (inter > best) { best = inter; shift = s; }
    }
    slamhip_sig_hit hit = valid ? hs_sig_make_hit(g, shift, best, A.qinfo[3], (int)A.nset[g]) : hs_sig_no_hit();
    k18_u64 key = k18_hit_rank(hit);
    for (int b = 0; b < A.B; b++) {
        const k18_u64 m = k18_wave_max(key);
        if (m == 0ull) break;                                              // (uniform over the wavefront)
        if (key == m) { cand_s[wave * HS_SG_MAX_B + b] = hit; key = 0ull; }   // (one lane: an index makes a key unique)
    }
    __syncthreads();
    if (wave == 0) {
        hit = cand_s[lane];
        key = k18_hit_rank(hit);
        slamhip_sig_hit *out = A.part + (size_t)blockIdx.x * A.B;
        for (int b = 0; b < A.B; b++) {
            const k18_u64 m = k18_wave_max(key);
            if (m == 0ull) { if (lane == 0) out[b] = hs_sig_no_hit(); }
            else if (key == m) { out[b] = hit; key = 0ull; }
        }
    }
}

__global__ void __launch_bounds__(K18_LANES) k18_query_finish(const slamhip_sig_hit *__restrict__ part, int n_part, int B, slamhip_sig_hit *__restrict__ out,
                                                              int32_t *__restrict__ out_n)
{
    __shared__ k18_u64 wk_s[K18_LANES / 64];
    __shared__ int wi_s[K18_LANES / 64];
    const int tid = threadIdx.x;
    k18_u64 prev = ~0ull;
    int count = 0;
    for (int b = 0; b < B; b++) {
        k18_u64 best = 0ull;
        int bi = -1;
        for (int i = tid; i < n_part; i += K18_LANES) {
            const k18_u64 key = k18_hit_rank(part[i]);
            if (key < prev && key > best) { best = key; bi = i; }
        }
        for (int off = 32; off > 0; off >>= 1) {
            const k18_u64 ok = __shfl_xor(best, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            if (ok > best) { best = ok; bi = oi; }
        }
        if ((tid & 63) == 0) { wk_s[tid >> 6] = best; wi_s[tid >> 6] = bi; }
        __syncthreads();
        best = 0ull; bi = -1;
        for (int wv = 0; wv < K18_LANES / 64; wv++)
            if (wk_s[wv] > best) { best = wk_s[wv]; bi = wi_s[wv]; }
        __syncthreads();
        if (best == 0ull) break;                                           // (uniform over the workgroup)
        if (tid == 0) out[b] = part[bi];
        prev = best;
        count++;
    }
    if (tid == 0) {
        for (int b = count; b < B; b++) out[b] = hs_sig_no_hit();
        *out_n = count;
    }
}

struct k18_self_arg {
    const k18_u64 *store; const uint16_t *nset; int n_ring;
    int first, last, min_gap, tile0;                       // tile0: first's block
    k18_u64 *best;                                         // [last - first], zeroed
};

template <int RG>
__global__ void __launch_bounds__(K18_LANES) k18_self(const k18_self_arg A)
{
    __shared__ k18_u64 key_s[HS_SG_BLOCK * RG];
    __shared__ int nk_s[HS_SG_BLOCK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tq = A.tile0 + (int)blockIdx.x, tk = A.tile0 + (int)blockIdx.y;
    const int i_max = min(tq * HS_SG_BLOCK + HS_SG_BLOCK - 1, A.last - 1);
    if (tk > tq || i_max - A.min_gap < max(tk * HS_SG_BLOCK, A.first)) return;   // (uniform: no query of the tile may see a key of this one)
    for (int i = tid; i < HS_SG_BLOCK * RG; i += K18_LANES) {
        const int r = i >> 6, j = i & 63, g = tk * HS_SG_BLOCK + j;        // (consecutive lanes consecutive keys of one ring)
        key_s[j * RG + r] = (r < A.n_ring && g < A.last) ? A.store[hs_sig_at(g, r, A.n_ring)] : 0ull;
    }
    if (tid < HS_SG_BLOCK) { const int g = tk * HS_SG_BLOCK + tid; nk_s[tid] = g < A.last ? (int)A.nset[g] : 0; }
    const int qi = tq * HS_SG_BLOCK + lane;
    const bool qvalid = qi >= A.first && qi < A.last;
    k18_u64 w[RG];
#pragma unroll
    for (int r = 0; r < RG; r++) w[r] = (qvalid && r < A.n_ring) ? A.store[hs_sig_at(qi, r, A.n_ring)] : 0ull;
    const int nq = qvalid ? (int)A.nset[qi] : 0;
    __syncthreads();
    k18_u64 mine = 0ull;
    for (int jj = 0; jj < HS_SG_BLOCK / (K18_LANES / 64); jj++) {
        const int j = wave * (HS_SG_BLOCK / (K18_LANES / 64)) + jj, g = tk * HS_SG_BLOCK + j;
        const bool active = qvalid && g >= A.first && g <= qi - A.min_gap;
        if (!__any(active)) continue;                                      // (uniform over the wavefront)
        const k18_u64 *kk = key_s + j * RG;                                // (the same words in every lane: broadcasts)
        int best = -1, shift = 0;
        for (int s = 0; s < HS_SG_SECTORS; s++) {                          // w holds rotr(query, s); after the 64th rotate the query again
            int inter = 0;
#pragma unroll
            for (int r = 0; r < RG; r++) { inter += (int)__popcll(w[r] & kk[r]); w[r] = (w[r] >> 1) | (w[r] << 63); }
            if (inter > best) { best = inter; shift = s; }
        }
        if (active) {
            const k18_u64 key = hs_sig_pack(hs_sig_score(best, nq, nk_s[j]), g, shift);
            mine = key > mine ? key : mine;
        }
    }
    if (mine) (void)__hip_atomic_fetch_max(A.best + (qi - A.first), mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(K18_LANES) k18_self_finish(const k18_u64 *__restrict__ store, const uint16_t *__restrict__ nset, int n_ring, int first, int last,
                                                             const k18_u64 *__restrict__ best, slamhip_sig_hit *__restrict__ out)
{
    const int i = first + (int)blockIdx.x * K18_LANES + (int)threadIdx.x;
    if (i >= last) return;
    const k18_u64 key = best[i - first];
    if (key == 0ull) { out[i - first] = hs_sig_no_hit(); return; }
    uint32_t score; int j, shift;
    hs_sig_unpack(key, &score, &j, &shift);
    int inter = 0;
    for (int r = 0; r < n_ring; r++) inter += (int)__popcll(store[hs_sig_at(i, r, n_ring)] & hs_sig_rotl(store[hs_sig_at(j, r, n_ring)], shift));
    out[i - first] = hs_sig_make_hit(j, shift, inter, (int)nset[i], (int)nset[j]);
}

// key-major words -> the store, with the popcounts counted here (slamhip_hs_sig_upload); and back (slamhip_hs_sig_download)
__global__ void __launch_bounds__(K18_LANES) k18_put(const k18_u64 *__restrict__ lin, int n, int n_ring, int first, k18_u64 *__restrict__ store,
                                                     uint16_t *__restrict__ nset)
{
    const int i = (int)blockIdx.x * K18_LANES + (int)threadIdx.x;
    if (i >= n) return;
    int total = 0;
    for (int r = 0; r < n_ring; r++) {
        const k18_u64 w = lin[(size_t)i * n_ring + r];
        store[hs_sig_at(first + i, r, n_ring)] = w;
        total += (int)__popcll(w);
    }
    nset[first + i] = (uint16_t)total;
}
__global__ void __launch_bounds__(K18_LANES) k18_get(const k18_u64 *__restrict__ store, int n, int n_ring, int first, k18_u64 *__restrict__ lin)
{
    const int i = (int)blockIdx.x * K18_LANES + (int)threadIdx.x;
    if (i >= n) return;
    for (int r = 0; r < n_ring; r++) lin[(size_t)i * n_ring + r] = store[hs_sig_at(first + i, r, n_ring)];
}

// ---- host side ---------------------------------------------------------------------------------------------------
// What the unit keeps, made by slamhip_hs_sig_configure: the spec, the table in device memory, the store (whole blocks, grown by
// doubling) with its n_set array, the poses on the host; the query's words and info, the partial lists, the self search's keys, the
// results and the staging of scans and words in device memory; the pinned block all of that reaches and leaves the host through.
struct hs_sig {
    bool configured;
    slamhip_sig_spec spec;
    int count, cap_blocks;
    hs_block<k18_u64, HS_MEM_DEVICE> d_store; hs_block<uint16_t, HS_MEM_DEVICE> d_nset;
    std::vector<float> poses;
    hs_block<int32_t, HS_MEM_DEVICE> d_cs;
    hs_block<unsigned char, HS_MEM_DEVICE> d_q;          // the scans' words [scans][n_ring], then their infos
    hs_block<unsigned char, HS_MEM_DEVICE> d_work;    // partial lists / packed keys
    hs_block<unsigned char, HS_MEM_DEVICE> d_out;      // hits and the count
    hs_block<unsigned char, HS_MEM_DEVICE> d_in;        // points and offsets of add_scans; words of upload / download
    hs_block<unsigned char, HS_MEM_PINNED> h_io;
};

void hs_sg_reset(slamhip_hs *hs)
{
    if (!hs->sig) return;
    hs->sig->count = 0;
    hs->sig->poses.clear();
}

static int32_t hs_sg_check_spec(float scale, int32_t n_ring, int32_t ring_cells)
{
    if (!hs_sig_spec_ok(scale, n_ring, ring_cells))
        SH_FAIL(SLAMHIP_ERR_INVALID, "signature: scale = %g must be finite and > 0, n_ring = %d in [1, %d], ring_cells = %d >= 1 with 2 * ring_cells * n_ring <= %d",
                (double)scale, n_ring, HS_SG_MAX_RING, ring_cells, HS_SG_MAX_REACH);
    return SLAMHIP_OK;
}

static int32_t hs_sg_need(const slamhip_hs *hs, const char *who)
{
    if (!hs->sig || !hs->sig->configured) SH_FAIL(SLAMHIP_ERR_STATE, "%s: no signature spec (slamhip_hs_sig_configure first)", who);
    return SLAMHIP_OK;
}

// room for `keys` keyframes: whole blocks; a larger store is a new allocation whose front is the old one, block for block
static int32_t hs_sg_reserve(slamhip_hs *hs, int keys)
{
    hs_sig *g = hs->sig;
    const int blocks = sh_div_up(keys, HS_SG_BLOCK);
    if (blocks <= g->cap_blocks) return SLAMHIP_OK;
    const int max_blocks = HS_SG_MAX_KEYS / HS_SG_BLOCK;
    int cap = std::max(std::max(blocks, 2 * g->cap_blocks), 16);
    if (cap > max_blocks) cap = max_blocks;
    const size_t words = (size_t)cap * g->spec.n_ring * HS_SG_BLOCK, old_words = (size_t)g->cap_blocks * g->spec.n_ring * HS_SG_BLOCK;
    hs_block<k18_u64, HS_MEM_DEVICE> ns; hs_block<uint16_t, HS_MEM_DEVICE> nn;   // (an early return frees them)
    SH_TRY(ns.grow(sizeof(k18_u64) * words, "signature store"));
    SH_TRY(nn.grow(sizeof(uint16_t) * (size_t)cap * HS_SG_BLOCK, "signature store"));
    hipStream_t st = hs->ctx->stream;
    hipError_t e = hipMemsetAsync(ns, 0, sizeof(k18_u64) * words, st);
    if (e == hipSuccess) e = hipMemsetAsync(nn, 0, sizeof(uint16_t) * (size_t)cap * HS_SG_BLOCK, st);
    if (e == hipSuccess && old_words) e = hipMemcpyAsync(ns, g->d_store, sizeof(k18_u64) * old_words, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess && old_words) e = hipMemcpyAsync(nn, g->d_nset, sizeof(uint16_t) * (size_t)g->cap_blocks * HS_SG_BLOCK, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);                     // (the old blocks are idle behind it)
    SH_HIP(e);
    g->d_store.swap(ns); g->d_nset.swap(nn); g->cap_blocks = cap;          // (the old blocks go with ns and nn)
    return SLAMHIP_OK;
}

// what slamhip_hs_sig_add and _sig_query refuse before they launch anything
int32_t hs_sg_check_add(const slamhip_hs *hs)
{
    SH_TRY(hs_sg_need(hs, "signature add"));
    if (hs->sig->count >= HS_SG_MAX_KEYS) SH_FAIL(SLAMHIP_ERR_INVALID, "signature add: the store holds 2^20 keyframes");
    return SLAMHIP_OK;
}
int32_t hs_sg_check_query(const slamhip_hs *hs, int32_t first, int32_t last, int32_t B)
{
    if (B < 1 || B > HS_SG_MAX_B) SH_FAIL(SLAMHIP_ERR_INVALID, "signature query: B = %d must lie in [1, %d]", B, HS_SG_MAX_B);
    SH_TRY(hs_sg_need(hs, "signature query"));
    if (first < 0 || last < first || last > hs->sig->count)
        SH_FAIL(SLAMHIP_ERR_INVALID, "signature query: the range [%d, %d) of %d keyframes", first, last, hs->sig->count);
    return SLAMHIP_OK;
}

static inline int hs_sg_rg(int n_ring) { return (n_ring + 7) & ~7; }

extern "C" int32_t slamhip_hs_sig_configure(slamhip_hs *hs, const slamhip_sig_spec *spec)
{
    SH_CHECK_ARG(hs && spec);
    SH_TRY(hs_sg_check_spec(spec->scale, spec->n_ring, spec->ring_cells));
    slamhip_ctx *ctx = hs->ctx;
    SH_TRY(hs_call_begin(hs));
    SH_TRY(hs_unit<&slamhip_hs::sig>(hs));
    hs_sig *g = hs->sig;
    const bool relay = g->configured && g->spec.n_ring != spec->n_ring;    // (the blocks' size depends on n_ring)
    g->configured = false;
    SH_TRY(g->d_cs.grow(sizeof(int32_t) * 2 * HS_SG_SECTORS, "signature"));
    SH_TRY(g->h_io.grow(sizeof(int32_t) * 2 * HS_SG_SECTORS, "signature"));
    hs_sig_table((int32_t *)g->h_io.p);
    SH_HIP(hipMemcpyAsync(g->d_cs, g->h_io, sizeof(int32_t) * 2 * HS_SG_SECTORS, hipMemcpyHostToDevice, ctx->stream));
    SH_TRY(hs_call_finish(hs));
    if (relay) {
        g->d_store.release();
        g->d_nset.release();
        g->cap_blocks = 0;
    }
    g->spec = *spec;
    g->count = 0;
    g->poses.clear();
    g->configured = true;
    return SLAMHIP_OK;
}

// the launch of k18_sig over the scan slamhip_hs_set_scan took: the words to g->d_q (and to the store as keyframe `first` when append)
static int32_t hs_sg_enqueue_scan(slamhip_hs *hs, bool append, int first)
{
    hs_sig *g = hs->sig;
    const size_t sig_bytes = sizeof(k18_u64) * (size_t)g->spec.n_ring;
    SH_TRY(g->d_q.grow(sig_bytes + sizeof(slamhip_sig_info), "signature"));
    if (hs->n_points > 0) SH_TRY(hs_flush_scan(hs));
    k18_sig_arg A;
    A.pts = hs->n_points > 0 ? hs->d_pts : (const float2 *)nullptr; A.offsets = nullptr; A.n = hs->n_points;
    A.scale = g->spec.scale; A.n_ring = g->spec.n_ring; A.ring_cells = g->spec.ring_cells;
    A.cs = g->d_cs;
    A.store = append ? g->d_store : (k18_u64 *)nullptr; A.nset = g->d_nset; A.first = first;
    A.lin = (k18_u64 *)g->d_q.p; A.info = (int32_t *)(g->d_q + sig_bytes);
    hipLaunchKernelGGL(k18_sig, dim3(1), dim3(K18_LANES), 0, hs->ctx->stream, A);
    SH_HIP(hipGetLastError());
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_sig_add(slamhip_hs *hs, const float pose[3], int32_t *out_index, uint64_t *out_sig, slamhip_sig_info *out_info)
{
    SH_CHECK_ARG(hs && pose);
    SH_TRY(hs_sg_check_add(hs));
    hs_sig *g = hs->sig;
    SH_TRY(hs_call_begin(hs));
    SH_TRY(hs_sg_reserve(hs, g->count + 1));
    const size_t io_bytes = sizeof(k18_u64) * (size_t)g->spec.n_ring + sizeof(slamhip_sig_info);
    SH_TRY(g->h_io.grow(io_bytes, "signature add"));
    SH_TRY(hs_sg_enqueue_scan(hs, true, g->count));
    SH_HIP(hipMemcpyAsync(g->h_io, g->d_q, io_bytes, hipMemcpyDeviceToHost, hs->ctx->stream));
    SH_TRY(hs_call_finish(hs));
    if (out_index) *out_index = g->count;
    if (out_sig) memcpy(out_sig, g->h_io, io_bytes - sizeof(slamhip_sig_info));
    if (out_info) memcpy(out_info, g->h_io + io_bytes - sizeof(slamhip_sig_info), sizeof(slamhip_sig_info));
    g->poses.insert(g->poses.end(), pose, pose + 3);
    g->count++;
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_sig_add_scans(slamhip_hs *hs, const float *xy, const int32_t *offsets, int32_t B, const float *poses, int32_t *out_first)
{
    SH_CHECK_ARG(hs && offsets && poses);
    if (B < 1 || B > HS_SG_MAX_SCANS) SH_FAIL(SLAMHIP_ERR_INVALID, "signature add_scans: B = %d must lie in [1, %d]", B, HS_SG_MAX_SCANS);
    if (offsets[0] != 0) SH_FAIL(SLAMHIP_ERR_INVALID, "signature add_scans: offsets[0] = %d must be 0", offsets[0]);
    for (int b = 0; b < B; b++)
        if (offsets[b + 1] < offsets[b]) SH_FAIL(SLAMHIP_ERR_INVALID, "signature add_scans: offsets[%d] = %d below offsets[%d] = %d", b + 1, offsets[b + 1], b, offsets[b]);
    const int total = offsets[B];
    if (total > HS_SG_MAX_POINTS) SH_FAIL(SLAMHIP_ERR_INVALID, "signature add_scans: %d points, more than 2^24", total);
    SH_CHECK_ARG(xy || total == 0);
    SH_TRY(hs_sg_need(hs, "signature add_scans"));
    hs_sig *g = hs->sig;
    if (g->count + B > HS_SG_MAX_KEYS) SH_FAIL(SLAMHIP_ERR_INVALID, "signature add_scans: %d + %d keyframes, more than 2^20", g->count, B);
    slamhip_ctx *ctx = hs->ctx;
    SH_TRY(hs_call_begin(hs));
    SH_TRY(hs_sg_reserve(hs, g->count + B));
    const size_t pts_bytes = (sizeof(float) * 2 * (size_t)total + 7) & ~(size_t)7, off_bytes = sizeof(int32_t) * ((size_t)B + 1);
    SH_TRY(g->d_in.grow(pts_bytes + off_bytes, "signature add_scans"));
    SH_TRY(g->h_io.grow(pts_bytes + off_bytes, "signature add_scans"));
    if (total) memcpy(g->h_io, xy, sizeof(float) * 2 * (size_t)total);
    memcpy(g->h_io + pts_bytes, offsets, off_bytes);
    SH_HIP(hipMemcpyAsync(g->d_in, g->h_io, pts_bytes + off_bytes, hipMemcpyHostToDevice, ctx->stream));
    k18_sig_arg A;
    A.pts = (const float2 *)g->d_in.p; A.offsets = (const int32_t *)(g->d_in + pts_bytes); A.n = 0;
    A.scale = g->spec.scale; A.n_ring = g->spec.n_ring; A.ring_cells = g->spec.ring_cells;
    A.cs = g->d_cs;
    A.store = g->d_store; A.nset = g->d_nset; A.first = g->count;
    A.lin = nullptr; A.info = nullptr;
    hipLaunchKernelGGL(k18_sig, dim3((unsigned)B), dim3(K18_LANES), 0, ctx->stream, A);
    SH_HIP(hipGetLastError());
    SH_TRY(hs_call_finish(hs));
    if (out_first) *out_first = g->count;
    g->poses.insert(g->poses.end(), poses, poses + 3 * (size_t)B);
    g->count += B;
    return SLAMHIP_OK;
}

template <int RG>
static void hs_sg_launch_query(hipStream_t st, int wgs, const k18_query_arg &Q) { hipLaunchKernelGGL(k18_query<RG>, dim3((unsigned)wgs), dim3(K18_LANES), 0, st, Q); }
template <int RG>
static void hs_sg_launch_self(hipStream_t st, int tiles, const k18_self_arg &S) { hipLaunchKernelGGL(k18_self<RG>, dim3((unsigned)tiles, (unsigned)tiles), dim3(K18_LANES), 0, st, S); }

extern "C" int32_t slamhip_hs_sig_query(slamhip_hs *hs, int32_t first, int32_t last, int32_t B, slamhip_sig_hit *out_hits, int32_t *out_n, uint64_t *out_sig,
                                        slamhip_sig_info *out_info)
{
    SH_CHECK_ARG(hs && out_hits && out_n);
    SH_TRY(hs_sg_check_query(hs, first, last, B));
    hs_sig *g = hs->sig;
    slamhip_ctx *ctx = hs->ctx;
    SH_TRY(hs_call_begin(hs));
    const int n_ring = g->spec.n_ring, base = first & ~(HS_SG_BLOCK - 1);
    const int wgs = last > first ? sh_div_up(last - base, K18_LANES) : 0;
    const size_t sig_bytes = sizeof(k18_u64) * (size_t)n_ring, q_bytes = sig_bytes + sizeof(slamhip_sig_info);
    const size_t hit_bytes = sizeof(slamhip_sig_hit) * (size_t)B, out_bytes = hit_bytes + 8;
    SH_TRY(g->d_work.grow(sizeof(slamhip_sig_hit) * (size_t)B * std::max(wgs, 1), "signature query"));
    SH_TRY(g->d_out.grow(out_bytes, "signature query"));
    SH_TRY(g->h_io.grow(out_bytes + q_bytes, "signature query"));
    SH_TRY(hs_sg_enqueue_scan(hs, false, 0));
    if (wgs) {
        k18_query_arg Q;
        Q.store = g->d_store; Q.nset = g->d_nset; Q.n_ring = n_ring;
        Q.first = first; Q.last = last; Q.base = base;
        Q.q = (const k18_u64 *)g->d_q.p; Q.qinfo = (const int32_t *)(g->d_q + sig_bytes);
        Q.B = B;
        Q.part = (slamhip_sig_hit *)g->d_work.p;
        // (at most 4096 workgroups)
        switch (hs_sg_rg(n_ring)) {
        case 8: hs_sg_launch_query<8>(ctx->stream, wgs, Q); break;
        case 16: hs_sg_launch_query<16>(ctx->stream, wgs, Q); break;
        case 24: hs_sg_launch_query<24>(ctx->stream, wgs, Q); break;
        default: hs_sg_launch_query<32>(ctx->stream, wgs, Q); break;
        }
        SH_HIP(hipGetLastError());
        hipLaunchKernelGGL(k18_query_finish, dim3(1), dim3(K18_LANES), 0, ctx->stream, (const slamhip_sig_hit *)g->d_work.p, wgs * B, B, (slamhip_sig_hit *)g->d_out.p,
                           (int32_t *)(g->d_out + hit_bytes));
        SH_HIP(hipGetLastError());
        SH_HIP(hipMemcpyAsync(g->h_io, g->d_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    }
    SH_HIP(hipMemcpyAsync(g->h_io + out_bytes, g->d_q, q_bytes, hipMemcpyDeviceToHost, ctx->stream));
    SH_TRY(hs_call_finish(hs));
    int32_t n = 0;
    if (wgs) memcpy(&n, g->h_io + hit_bytes, sizeof(n));
    if (n) memcpy(out_hits, g->h_io, sizeof(slamhip_sig_hit) * (size_t)n);
    *out_n = n;
    if (out_sig) memcpy(out_sig, g->h_io + out_bytes, sig_bytes);
    if (out_info) memcpy(out_info, g->h_io + out_bytes + sig_bytes, sizeof(slamhip_sig_info));
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_sig_self(slamhip_hs *hs, int32_t first, int32_t last, int32_t min_gap, slamhip_sig_hit *out_hits)
{
    SH_CHECK_ARG(hs && out_hits);
    if (min_gap < 1) SH_FAIL(SLAMHIP_ERR_INVALID, "signature self search: min_gap = %d must be at least 1", min_gap);
    SH_TRY(hs_sg_need(hs, "signature self search"));
    hs_sig *g = hs->sig;
    if (first < 0 || last < first || last > g->count) SH_FAIL(SLAMHIP_ERR_INVALID, "signature self search: the range [%d, %d) of %d keyframes", first, last, g->count);
    if (last == first) return SLAMHIP_OK;
    slamhip_ctx *ctx = hs->ctx;
    SH_TRY(hs_call_begin(hs));
    const int n = last - first, n_ring = g->spec.n_ring;
    const int tile0 = first / HS_SG_BLOCK, tiles = (last - 1) / HS_SG_BLOCK - tile0 + 1;
    SH_TRY(g->d_work.grow(sizeof(k18_u64) * (size_t)n, "signature self search"));
    SH_TRY(g->d_out.grow(sizeof(slamhip_sig_hit) * (size_t)n, "signature self search"));
    SH_TRY(g->h_io.grow(sizeof(slamhip_sig_hit) * (size_t)n, "signature self search"));
    SH_HIP(hipMemsetAsync(g->d_work, 0, sizeof(k18_u64) * (size_t)n, ctx->stream));
    k18_self_arg S;
    S.store = g->d_store; S.nset = g->d_nset; S.n_ring = n_ring;
    S.first = first; S.last = last; S.min_gap = min_gap; S.tile0 = tile0;
    S.best = (k18_u64 *)g->d_work.p;
    // (at most 16384 x 16384 tile pairs; those above the band leave at once)
    switch (hs_sg_rg(n_ring)) {
    case 8: hs_sg_launch_self<8>(ctx->stream, tiles, S); break;
    case 16: hs_sg_launch_self<16>(ctx->stream, tiles, S); break;
    case 24: hs_sg_launch_self<24>(ctx->stream, tiles, S); break;
    default: hs_sg_launch_self<32>(ctx->stream, tiles, S); break;
    }
    SH_HIP(hipGetLastError());
    hipLaunchKernelGGL(k18_self_finish, dim3((unsigned)sh_div_up(n, K18_LANES)), dim3(K18_LANES), 0, ctx->stream, (const k18_u64 *)g->d_store,
                       (const uint16_t *)g->d_nset, n_ring, first, last, (const k18_u64 *)g->d_work.p, (slamhip_sig_hit *)g->d_out.p);
    SH_HIP(hipGetLastError());
    SH_HIP(hipMemcpyAsync(g->h_io, g->d_out, sizeof(slamhip_sig_hit) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    SH_TRY(hs_call_finish(hs));
    memcpy(out_hits, g->h_io, sizeof(slamhip_sig_hit) * (size_t)n);
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_sig_count(slamhip_hs *hs, int32_t *out_count)
{
    SH_CHECK_ARG(hs && out_count);
    SH_TRY(hs_sg_need(hs, "signature count"));
    *out_count = hs->sig->count;
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_sig_download(slamhip_hs *hs, int32_t first, int32_t n, uint64_t *sig, float *poses)
{
    SH_CHECK_ARG(hs && (sig || poses));
    SH_TRY(hs_sg_need(hs, "signature download"));
    hs_sig *g = hs->sig;
    if (first < 0 || n < 0 || first > g->count || n > g->count - first)
        SH_FAIL(SLAMHIP_ERR_INVALID, "signature download: %d keyframes from %d of %d", n, first, g->count);
    if (n == 0) return SLAMHIP_OK;
    if (poses) memcpy(poses, g->poses.data() + 3 * (size_t)first, sizeof(float) * 3 * (size_t)n);
    if (!sig) return SLAMHIP_OK;
    slamhip_ctx *ctx = hs->ctx;
    SH_TRY(hs_call_begin(hs));
    const size_t bytes = sizeof(k18_u64) * (size_t)n * g->spec.n_ring;
    SH_TRY(g->d_in.grow(bytes, "signature download"));
    SH_TRY(g->h_io.grow(bytes, "signature download"));
    hipLaunchKernelGGL(k18_get, dim3((unsigned)sh_div_up(n, K18_LANES)), dim3(K18_LANES), 0, ctx->stream, (const k18_u64 *)g->d_store, n, g->spec.n_ring, first,
                       (k18_u64 *)g->d_in.p);
    SH_HIP(hipGetLastError());
    SH_HIP(hipMemcpyAsync(g->h_io, g->d_in, bytes, hipMemcpyDeviceToHost, ctx->stream));
    SH_TRY(hs_call_finish(hs));
    memcpy(sig, g->h_io, bytes);
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_sig_set_poses(slamhip_hs *hs, int32_t first, int32_t n, const float *poses)
{
    SH_CHECK_ARG(hs && (poses || n == 0));
    SH_TRY(hs_sg_need(hs, "signature set_poses"));
    hs_sig *g = hs->sig;
    if (first < 0 || n < 0 || first > g->count || n > g->count - first)
        SH_FAIL(SLAMHIP_ERR_INVALID, "signature set_poses: %d keyframes from %d of %d", n, first, g->count);
    if (n) memcpy(g->poses.data() + 3 * (size_t)first, poses, sizeof(float) * 3 * (size_t)n);   // (host-side books: nothing is launched)
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_sig_upload(slamhip_hs *hs, int32_t n, const uint64_t *sig, const float *poses)
{
    SH_CHECK_ARG(hs && sig && poses);
    SH_TRY(hs_sg_need(hs, "signature upload"));
    hs_sig *g = hs->sig;
    if (n < 0 || n > HS_SG_MAX_KEYS - g->count) SH_FAIL(SLAMHIP_ERR_INVALID, "signature upload: %d + %d keyframes, more than 2^20", g->count, n);
    if (n == 0) return SLAMHIP_OK;
    slamhip_ctx *ctx = hs->ctx;
    SH_TRY(hs_call_begin(hs));
    SH_TRY(hs_sg_reserve(hs, g->count + n));
    const size_t bytes = sizeof(k18_u64) * (size_t)n * g->spec.n_ring;
    SH_TRY(g->d_in.grow(bytes, "signature upload"));
    SH_TRY(g->h_io.grow(bytes, "signature upload"));
    memcpy(g->h_io, sig, bytes);
    SH_HIP(hipMemcpyAsync(g->d_in, g->h_io, bytes, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k18_put, dim3((unsigned)sh_div_up(n, K18_LANES)), dim3(K18_LANES), 0, ctx->stream, (const k18_u64 *)g->d_in.p, n, g->spec.n_ring, g->count,
                       g->d_store, g->d_nset);
    SH_HIP(hipGetLastError());
    SH_TRY(hs_call_finish(hs));
    g->poses.insert(g->poses.end(), poses, poses + 3 * (size_t)n);
    g->count += n;
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_sig_clear(slamhip_hs *hs)
{
    SH_CHECK_ARG(hs);
    if (!hs->sig) return SLAMHIP_OK;
    SH_TRY(hs_call_begin(hs));
    SH_TRY(hs_call_finish(hs));                                            // (the blocks are idle behind it)
    hs_unit_drop<&slamhip_hs::sig>(hs);
    return SLAMHIP_OK;
}

// ---- CPU-side test hooks: hs_sig.h -- the text the kernels run -- in plain loops ----------------------------------------------------
extern "C" int32_t slamhip_debug_sig_table(int32_t out_cs[128])
{
    SH_CHECK_ARG(out_cs);
    hs_sig_table(out_cs);
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_debug_sig_ring(const int32_t *d2, int32_t n, int32_t n_ring, int32_t ring_cells, int32_t *out_ring)
{
    SH_CHECK_ARG(d2 && out_ring && n >= 0);
    SH_TRY(hs_sg_check_spec(1.0f, n_ring, ring_cells));
    for (int i = 0; i < n; i++) {
        if (d2[i] < 0) SH_FAIL(SLAMHIP_ERR_INVALID, "signature ring: d2[%d] = %d is negative", i, d2[i]);
        out_ring[i] = hs_sig_ring(d2[i], n_ring, ring_cells);
    }
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_debug_sig_sector(const int32_t *uv, int32_t n, int32_t *out_sector)
{
    SH_CHECK_ARG(uv && out_sector && n >= 0);
    int32_t cs[2 * HS_SG_SECTORS];
    hs_sig_table(cs);
    for (int i = 0; i < n; i++) {
        const int u = uv[2 * i], v = uv[2 * i + 1];
        if (!(u & 1) || !(v & 1) || u < -32767 || u > 32767 || v < -32767 || v > 32767)
            SH_FAIL(SLAMHIP_ERR_INVALID, "signature sector: (u, v)[%d] = (%d, %d) must be odd and within +-32767", i, u, v);
        out_sector[i] = hs_sig_sector(cs, u, v);
    }
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_debug_sig(const float *xy, int32_t n, const slamhip_sig_spec *spec, uint64_t *out_sig, slamhip_sig_info *out_info)
{
    SH_CHECK_ARG(spec && out_sig && n >= 0 && (xy || n == 0));
    SH_TRY(hs_sg_check_spec(spec->scale, spec->n_ring, spec->ring_cells));
    int32_t cs[2 * HS_SG_SECTORS];
    hs_sig_table(cs);
    slamhip_sig_info I = { n, 0, 0, 0 };
    for (int r = 0; r < spec->n_ring; r++) out_sig[r] = 0;
    for (int i = 0; i < n; i++) {
        int u, v;
        if (!hs_sig_cell(xy[2 * i], xy[2 * i + 1], spec->scale, &u, &v)) { I.n_ignored++; continue; }
        const int ring = hs_sig_ring(u * u + v * v, spec->n_ring, spec->ring_cells);
        if (ring == spec->n_ring) { I.n_far++; continue; }
        out_sig[ring] |= 1ull << hs_sig_sector(cs, u, v);
    }
    for (int r = 0; r < spec->n_ring; r++) I.n_set += hs_sig_popc(out_sig[r]);
    if (out_info) *out_info = I;
    return SLAMHIP_OK;
}

// rule 6 for one pair of key-major words
static slamhip_sig_hit hs_sg_pair(const uint64_t *q, int nq, const uint64_t *k, int nk, int index, int n_ring)
{
    int best = -1, shift = 0;
    for (int s = 0; s < HS_SG_SECTORS; s++) {
        int inter = 0;
        for (int r = 0; r < n_ring; r++) inter += hs_sig_popc(q[r] & hs_sig_rotl(k[r], s));
        if (inter > best) { best = inter; shift = s; }
    }
    return hs_sig_make_hit(index, shift, best, nq, nk);
}

extern "C" int32_t slamhip_debug_sig_search(const uint64_t *query_sig, const uint64_t *store_sig, const uint16_t *n_set, int32_t N, int32_t n_ring,
                                            int32_t first, int32_t last, int32_t min_gap, int32_t B, slamhip_sig_hit *out_hits, int32_t *out_n)
{
    SH_CHECK_ARG(out_hits && out_n && N >= 0 && (N == 0 || (store_sig && n_set)));
    if (n_ring < 1 || n_ring > HS_SG_MAX_RING) SH_FAIL(SLAMHIP_ERR_INVALID, "signature search: n_ring = %d must lie in [1, %d]", n_ring, HS_SG_MAX_RING);
    if (N > HS_SG_MAX_KEYS) SH_FAIL(SLAMHIP_ERR_INVALID, "signature search: %d keyframes, more than 2^20", N);
    if (first < 0 || last < first || last > N) SH_FAIL(SLAMHIP_ERR_INVALID, "signature search: the range [%d, %d) of %d keyframes", first, last, N);
    if (query_sig && (B < 1 || B > HS_SG_MAX_B)) SH_FAIL(SLAMHIP_ERR_INVALID, "signature search: B = %d must lie in [1, %d]", B, HS_SG_MAX_B);
    if (!query_sig && min_gap < 1) SH_FAIL(SLAMHIP_ERR_INVALID, "signature search: min_gap = %d must be at least 1", min_gap);
    for (int i = first; i < last; i++) {
        int pc = 0;
        for (int r = 0; r < n_ring; r++) pc += hs_sig_popc(store_sig[(size_t)i * n_ring + r]);
        if (pc != (int)n_set[i]) SH_FAIL(SLAMHIP_ERR_INVALID, "signature search: n_set[%d] = %d, but its words hold %d bits", i, (int)n_set[i], pc);
    }
    if (query_sig) {
        int nq = 0;
        for (int r = 0; r < n_ring; r++) nq += hs_sig_popc(query_sig[r]);
        std::vector<slamhip_sig_hit> all;
        all.reserve((size_t)(last - first));
        for (int i = first; i < last; i++) all.push_back(hs_sg_pair(query_sig, nq, store_sig + (size_t)i * n_ring, (int)n_set[i], i, n_ring));
        std::sort(all.begin(), all.end(), [](const slamhip_sig_hit &a, const slamhip_sig_hit &b) { return hs_sig_rank(a.score, a.index) > hs_sig_rank(b.score, b.index); });
        const int n = std::min<int>(B, (int)all.size());
        for (int i = 0; i < n; i++) out_hits[i] = all[(size_t)i];
        *out_n = n;
        return SLAMHIP_OK;
    }
    for (int i = first; i < last; i++) {
        unsigned long long best = 0ull;
        for (int j = first; j <= i - min_gap; j++) {
            const slamhip_sig_hit h = hs_sg_pair(store_sig + (size_t)i * n_ring, (int)n_set[i], store_sig + (size_t)j * n_ring, (int)n_set[j], j, n_ring);
            const unsigned long long key = hs_sig_pack(h.score, j, h.shift);
            best = key > best ? key : best;
        }
        if (!best) { out_hits[i - first] = hs_sig_no_hit(); continue; }
        uint32_t score; int j, shift;
        hs_sig_unpack(best, &score, &j, &shift);
        const uint64_t *qi = store_sig + (size_t)i * n_ring, *kj = store_sig + (size_t)j * n_ring;
        int inter = 0;
        for (int r = 0; r < n_ring; r++) inter += hs_sig_popc(qi[r] & hs_sig_rotl(kj[r], shift));
        out_hits[i - first] = hs_sig_make_hit(j, shift, inter, (int)n_set[i], (int)n_set[j]);
    }
    *out_n = last - first;
    return SLAMHIP_OK;
}
