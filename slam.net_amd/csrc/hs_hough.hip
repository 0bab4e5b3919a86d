// hs_hough.hip -- K17, the Hough transform of HectorSLAM's map and what a scan-free alignment of two maps takes from it: the votes
// H[k][p] of a map's sites over T angles, the spectrum HS[k] = sum_p H[k][p]^2, the circular correlation of two spectra (the relative
// rotation) and the correlation of matching Hough rows over rho (the translation along a direction), after Carpin, "Fast and accurate
// map merging for multi-robot systems" (2008) (slamhip_hs_hough, _hough_rotation, _hough_shifts, _hough_clear, slamhip_debug_hough_table,
// slamhip_debug_hough, slamhip_debug_hough_xcorr).  No reference counterpart.  Definition: include/slamhip.h (slamhip_hs_hough); the
// arithmetic host and device share: hs_hough.h, on top of hs_dfield.h's site words.
//
// Two slots: slot 0 is K7's class map of a level (the window's or the world's, re-packed on every call), slot 1 the packed classes of
// K14's merge source.  A slot keeps H, its spectrum and the non-zero extent of every row in device memory until it is filled again.
//  * k17_vote: the grid is (tiles of 64 x 64 cells of M, chunks of K17_ANGLES angles).  The tile's 128 site words go to LDS; a tile
//    without a site leaves at once.  The sites are compacted into a list in LDS (any order).  For one angle the votes of a tile span at
//    most (91 >> q) + 2 consecutive bins, so the workgroup keeps one histogram of K17_SPAN bins per angle, based at the least bin of
//    the tile's four corners (the bin is monotone in i and in j).  A wavefront takes one site at a time and its 64 lanes the 64
//    angles: the lanes add into 64 DIFFERENT histograms, whose rows are K17_HSTRIDE = 97 words apart, so lanes whose bins lie near each
//    other fall on different banks and no two lanes ever share an address.  The non-zero bins are flushed with 32-bit agent-scope
//    atomic adds whose result is not used, consecutive lanes consecutive bins.  H is zeroed by a memset in front.
//  * k17_spectrum: a workgroup per angle: the squares' sum, the row's sum (n_sites) and the first and last non-zero bin.
//  * k17_xcorr: the grid is (pair, block of 256 shifts), a shift per lane.  Both rows are trimmed to their non-zero extents; a block
//    none of whose shifts lets the extents meet does no arithmetic.  B's extent goes through LDS in pieces of K17X_BCH words, flipped
//    on the way in; a zero of B is skipped by the whole workgroup; each lane runs along A, consecutive lanes consecutive words.
//    32 x 32 -> 64-bit products.  Each block leaves a partial record (best, smallest shift, ties, sum).
//  * k17_xcorr_finish: a wavefront per pair merges the partial records by hs_hough_rec_add and stores the 24-byte record.
// Integers throughout: every vote order, reduction tree and atomic order gives the same bits.
#include "hs_blocks.h"
#include "hs_hough.h"
#include <limits.h>
#include <vector>

#define K17_LANES 256
#define K17_TILE 64
#define K17_ANGLES 64                      // angles of a workgroup: one per lane of each wavefront
#define K17_SPAN 96                        // bins a tile's votes can span at one angle: 63 * (|C| + |S|) / 16384 < 90 cells, so at most 91
#define K17_HSTRIDE 97                     // words between two angles' histograms, odd
#define K17X_LANES 256
#define K17X_BCH 2048                      // words of B in LDS at a time

static_assert(sizeof(slamhip_hough_shift) == 24, "the record of include/slamhip.h");
static_assert(K17_TILE == 64 && K17_ANGLES == 64 && K17_LANES == 256 && K17_HSTRIDE > K17_SPAN, "a site word pair per tile row; a lane per angle");

typedef unsigned long long k17_u64;

struct k17_vote_arg {
    const uint32_t *cls; int w, h, wpr;    // M
    int mask, T, q, D, N;
    const int32_t *cs;                     // C[T], S[T]
    int tiles_x;
    uint32_t *H;                           // T x N, zeroed
};

__global__ void __launch_bounds__(K17_LANES) k17_vote(const k17_vote_arg A)
{
    __shared__ uint16_t site_s[K17_TILE * K17_TILE];
    __shared__ uint32_t hist_s[K17_ANGLES * K17_HSTRIDE];
    __shared__ int base_s[K17_ANGLES];
    __shared__ int n_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ty = blockIdx.x / A.tiles_x, tx = blockIdx.x - ty * A.tiles_x;
    const int x0 = tx * K17_TILE, y0 = ty * K17_TILE;
    uint32_t word = 0;
    if (tid < 2 * K17_TILE) {                                              // tile row tid / 2, its left or right 32 cells
        const int y = y0 + (tid >> 1);
        const uint32_t *row = y < A.h ? A.cls + (size_t)y * A.wpr : (const uint32_t *)nullptr;
        word = hs_hough_site_word(row, A.w, x0 + 32 * (tid & 1), A.mask);
    }
    if (tid == 0) n_s = 0;
    if (!__syncthreads_or(word != 0u)) return;                             // (uniform: most of a map is such tiles)
    if (word) {
        int at = atomicAdd(&n_s, __popc(word));                            // (at most 4096 sites: the list's size)
        const int r = tid >> 1, cx = 32 * (tid & 1);
        while (word) {
            const int b = hs_df_ctz(word);
            word &= word - 1u;
            site_s[at++] = (uint16_t)((r << 6) | (cx + b));
        }
    }
    for (int i = tid; i < K17_ANGLES * K17_HSTRIDE; i += K17_LANES) hist_s[i] = 0u;
    const int k0 = blockIdx.y * K17_ANGLES;
    const int ka = min(K17_ANGLES, A.T - k0);
    const bool on = lane < ka;
    const int c = on ? A.cs[k0 + lane] : 0, s = on ? A.cs[A.T + k0 + lane] : 0;
    const int x1 = min(x0 + K17_TILE - 1, A.w - 1), y1 = min(y0 + K17_TILE - 1, A.h - 1);
    const uint32_t b00 = hs_hough_bin(x0, y0, c, s, A.D, A.q), b10 = hs_hough_bin(x1, y0, c, s, A.D, A.q);
    const uint32_t b01 = hs_hough_bin(x0, y1, c, s, A.D, A.q), b11 = hs_hough_bin(x1, y1, c, s, A.D, A.q);
    const int base = (int)min(min(b00, b10), min(b01, b11));
    if (wave == 0) base_s[lane] = base;
    __syncthreads();
    const int ns = n_s;
    if (on) {
        uint32_t *mine = hist_s + lane * K17_HSTRIDE;
        for (int i = wave; i < ns; i += K17_LANES / 64) {
            const int st = (int)site_s[i];                                 // (the same word in every lane: a broadcast)
            const int p = (int)hs_hough_bin(x0 + (st & 63), y0 + (st >> 6), c, s, A.D, A.q);
            atomicAdd(mine + (p - base), 1u);                              // (0 <= p - base < K17_SPAN)
        }
    }
    __syncthreads();
    for (int i = tid; i < ka * K17_HSTRIDE; i += K17_LANES) {
        const uint32_t v = hist_s[i];
        if (v) {
            const int a = i / K17_HSTRIDE, p = base_s[a] + (i - a * K17_HSTRIDE);
            if (p < A.N) (void)__hip_atomic_fetch_add(A.H + (size_t)(k0 + a) * A.N + p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// spec: HS[T], then the rows' sums [T]; ext: (first, last) non-zero bin of every row, (N, -1) for an empty row
__global__ void __launch_bounds__(256) k17_spectrum(const uint32_t *__restrict__ H, int N, int T, k17_u64 *__restrict__ spec, int2 *__restrict__ ext)
{
    __shared__ k17_u64 sq_s[4], sm_s[4];
    __shared__ int lo_s[4], hi_s[4];
    const int tid = threadIdx.x, k = blockIdx.x;
    const uint32_t *row = H + (size_t)k * N;
    k17_u64 sq = 0, sm = 0;
    int lo = N, hi = -1;
    for (int p = tid; p < N; p += 256) {
        const uint32_t v = row[p];
        sq += (k17_u64)v * v; sm += v;
        if (v) { lo = min(lo, p); hi = max(hi, p); }
    }
    for (int off = 32; off > 0; off >>= 1) {
        sq += __shfl_down(sq, off, 64); sm += __shfl_down(sm, off, 64);
        lo = min(lo, __shfl_down(lo, off, 64)); hi = max(hi, __shfl_down(hi, off, 64));
    }
    if ((tid & 63) == 0) { sq_s[tid >> 6] = sq; sm_s[tid >> 6] = sm; lo_s[tid >> 6] = lo; hi_s[tid >> 6] = hi; }
    __syncthreads();
    if (tid == 0) {
        for (int wv = 1; wv < 4; wv++) { sq += sq_s[wv]; sm += sm_s[wv]; lo = min(lo, lo_s[wv]); hi = max(hi, hi_s[wv]); }
        spec[k] = sq; spec[T + k] = sm;
        ext[k] = make_int2(lo, hi);
    }
}

struct k17x_part { k17_u64 best, sum; int shift, ties; };

struct k17x_arg {
    const uint32_t *Hd, *Hs; int Nd, Ns, T;
    const int2 *extd, *exts;
    const int32_t *pairs; int blocks;      // P x 2; blocks of 256 shifts per pair
    k17_u64 *xc;                           // nullptr, or P x (Nd + Ns - 1)
    k17x_part *part;                       // P x blocks
};

__global__ void __launch_bounds__(K17X_LANES) k17_xcorr(const k17x_arg X)
{
    __shared__ uint32_t b_s[K17X_BCH];
    __shared__ k17x_part w_s[K17X_LANES / 64];
    const int tid = threadIdx.x;
    const int pair = blockIdx.x / X.blocks, blk = blockIdx.x - pair * X.blocks;
    const int NX = X.Nd + X.Ns - 1;
    const int e = blk * K17X_LANES + tid;                                  // the shift's index: d = e - (Ns - 1)
    const bool valid = e < NX;
    const int d = e - (X.Ns - 1);
    int kk, f;
    const int k = X.pairs[2 * pair + 1];
    hs_hough_pair(X.T, X.pairs[2 * pair], k, &kk, &f);
    const uint32_t *A = X.Hd + (size_t)k * X.Nd, *B = X.Hs + (size_t)kk * X.Ns;
    const int2 ea = X.extd[k], eb = X.exts[kk];
    const int alo = ea.x, ahi = ea.y;                                      // (an empty row: alo > ahi)
    const int blo = f ? X.Ns - 1 - eb.y : eb.x, bhi = f ? X.Ns - 1 - eb.x : eb.y;
    // the p' some shift of this block needs: p' + d in [alo, ahi] for a d in [d0, d0 + 255]
    const int d0 = blk * K17X_LANES - (X.Ns - 1);
    const int pl = max(blo, alo - (d0 + K17X_LANES - 1)), ph = min(bhi, ahi - d0);
    k17_u64 acc = 0;
    if (alo <= ahi && eb.x <= eb.y)
        for (int c0 = pl; c0 <= ph; c0 += K17X_BCH) {                      // (uniform over the workgroup)
            const int cnt = min(K17X_BCH, ph - c0 + 1);
            __syncthreads();
            for (int j = tid; j < cnt; j += K17X_LANES) b_s[j] = B[hs_hough_b_index(X.Ns, f, c0 + j)];   // (blo <= c0 + j <= bhi: inside the row)
            __syncthreads();
            for (int j = 0; j < cnt; j++) {
                const uint32_t b = b_s[j];
                if (b == 0u) continue;                                     // (the same in every lane)
                const int ai = c0 + j + d;
                const uint32_t a = (ai >= alo && ai <= ahi) ? A[ai] : 0u;  // (0 <= alo, ahi < Nd)
                acc += (k17_u64)a * b;
            }
        }
    if (X.xc && valid) X.xc[(size_t)pair * NX + e] = acc;
    // the wavefront's record: its shifts rise with the lane, so the smallest shift at the maximum is the ballot's lowest bit
    k17_u64 mx = valid ? acc : 0ull, sum = valid ? acc : 0ull;
    for (int off = 32; off > 0; off >>= 1) {
        const k17_u64 o = __shfl_xor(mx, off, 64);
        mx = o > mx ? o : mx;
        sum += __shfl_xor(sum, off, 64);
    }
    const k17_u64 tie = __ballot(valid && acc == mx);
    if ((tid & 63) == 0) {
        k17x_part w;
        w.best = mx; w.sum = sum;
        w.ties = (int)__popcll(tie);
        w.shift = tie ? d + (int)(__ffsll((long long)tie) - 1) : 0;
        w_s[tid >> 6] = w;
    }
    __syncthreads();
    if (tid == 0) {
        k17x_part r = { 0ull, 0ull, 0, 0 };
        for (int wv = 0; wv < K17X_LANES / 64; wv++) {
            hs_hough_rec_add(&r.best, &r.shift, &r.ties, w_s[wv].best, w_s[wv].shift, w_s[wv].ties);
            r.sum += w_s[wv].sum;
        }
        X.part[(size_t)pair * X.blocks + blk] = r;
    }
}

__global__ void __launch_bounds__(64) k17_xcorr_finish(const k17x_part *__restrict__ part, int blocks, slamhip_hough_shift *__restrict__ out)
{
    const int pair = blockIdx.x, lane = threadIdx.x;
    k17_u64 best = 0, sum = 0;
    int shift = 0, ties = 0;
    for (int b = lane; b < blocks; b += 64) {
        const k17x_part p = part[(size_t)pair * blocks + b];
        hs_hough_rec_add(&best, &shift, &ties, p.best, p.shift, p.ties);
        sum += p.sum;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const k17_u64 ob = __shfl_down(best, off, 64);
        const int os = __shfl_down(shift, off, 64), ot = __shfl_down(ties, off, 64);
        hs_hough_rec_add(&best, &shift, &ties, ob, os, ot);
        sum += __shfl_down(sum, off, 64);
    }
    if (lane == 0) {
        slamhip_hough_shift r;
        r.best_shift = shift; r.n_ties = ties; r.best_value = best; r.sum = sum;
        out[pair] = r;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------
// What the unit keeps, made by the first slamhip_hs_hough: per slot H, the spectrum block (HS, the rows' sums) and the rows' extents in
// device memory with a host copy of HS; the table, the pairs and the results' block of a hough_shifts call; the pinned block that
// tables and pairs leave and results reach the host through.
struct hs_hough_slot {
    bool have;
    int level, world, mask, T, q;
    int w, h, x0, y0, D, N;
    int64_t n_sites;
    hs_block<uint32_t, HS_MEM_DEVICE> d_H;
    hs_block<k17_u64, HS_MEM_DEVICE> d_spec;
    hs_block<int2, HS_MEM_DEVICE> d_ext;
    std::vector<k17_u64> spec;             // HS[T]
};
struct hs_hough {
    hs_hough_slot slot[2];
    hs_block<int32_t, HS_MEM_DEVICE> d_cs;
    hs_block<int32_t, HS_MEM_DEVICE> d_pairs;
    hs_block<unsigned char, HS_MEM_DEVICE> d_out;  // records, XC arrays, partial records
    hs_block<unsigned char, HS_MEM_PINNED> h_io;
};

void hs_hg_drop_slot(slamhip_hs *hs, int slot) { if (hs->hgh) hs->hgh->slot[slot].have = false; }

static int32_t hs_hg_check_T_q(int32_t T, int32_t q)
{
    if (T < HS_HG_MIN_T || T > HS_HG_MAX_T || (T & 3)) SH_FAIL(SLAMHIP_ERR_INVALID, "hough: T = %d must be a multiple of 4 in [4, %d]", T, HS_HG_MAX_T);
    if (q < 0 || q > HS_HG_MAX_Q) SH_FAIL(SLAMHIP_ERR_INVALID, "hough: q = %d must lie in [0, %d]", q, HS_HG_MAX_Q);
    return SLAMHIP_OK;
}

// what slamhip_hs_hough_rotation and _shifts need: both slots filled with equal level, T, q
static int32_t hs_hg_check_both(const slamhip_hs *hs)
{
    const hs_hough *g = hs->hgh;
    if (!g || !g->slot[0].have || !g->slot[1].have) SH_FAIL(SLAMHIP_ERR_STATE, "hough: both slots must be filled (slamhip_hs_hough with slot 0 and with slot 1 first)");
    const hs_hough_slot &a = g->slot[0], &b = g->slot[1];
    if (a.level != b.level || a.T != b.T || a.q != b.q)
        SH_FAIL(SLAMHIP_ERR_STATE, "hough: the slots differ: level %d / %d, T %d / %d, q %d / %d", a.level, b.level, a.T, b.T, a.q, b.q);
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_hough(slamhip_hs *hs, int32_t level, int32_t slot, int32_t world, int32_t site_mask, int32_t T, int32_t q,
                                    int32_t out_info[7], uint64_t *out_spectrum, uint32_t *out_H)
{
    SH_CHECK_ARG(hs && out_info && out_spectrum);
    if (level < 0 || level >= hs->n_levels) SH_FAIL(SLAMHIP_ERR_INVALID, "hough: level %d of %d", level, hs->n_levels);
    if (slot != 0 && slot != 1) SH_FAIL(SLAMHIP_ERR_INVALID, "hough: slot = %d must be 0 (the map) or 1 (the merge source)", slot);
    if (world != 0 && world != 1) SH_FAIL(SLAMHIP_ERR_INVALID, "hough: world = %d must be 0 or 1", world);
    if (site_mask < 1 || site_mask > 7) SH_FAIL(SLAMHIP_ERR_INVALID, "hough: site_mask = %d must lie in [1, 7]", site_mask);
    SH_TRY(hs_hg_check_T_q(T, q));
    hs_class_map M;
    if (slot == 1) {
        if (world) SH_FAIL(SLAMHIP_ERR_INVALID, "hough: slot 1 is the merge source, which has no world: world must be 0");
        int src_level;
        SH_TRY(hs_merge_source_map(hs, &M, &src_level));
        if (level != src_level) SH_FAIL(SLAMHIP_ERR_INVALID, "hough: slot 1 holds a source of level %d, not %d", src_level, level);
    }
    slamhip_ctx *ctx = hs->ctx;
    SH_TRY(hs_call_begin(hs));
    if (slot == 0) SH_TRY(hs_lat_pack_prepare(hs, level, world != 0, &M));
    if (M.w > HS_HG_MAX_DIM || M.h > HS_HG_MAX_DIM) SH_FAIL(SLAMHIP_ERR_INVALID, "hough: a map of %d x %d cells; at most %d each way", M.w, M.h, HS_HG_MAX_DIM);
    const int D = hs_hough_D(M.w, M.h), N = hs_hough_N(D, q);
    if ((int64_t)T * N > HS_HG_MAX_BINS) SH_FAIL(SLAMHIP_ERR_INVALID, "hough: T * N = %d * %d bins, more than 2^24", T, N);
    SH_TRY(hs_unit<&slamhip_hs::hgh>(hs));
    hs_hough *g = hs->hgh;
    hs_hough_slot &S = g->slot[slot];
    const size_t cs_bytes = sizeof(int32_t) * 2 * (size_t)T, spec_bytes = sizeof(k17_u64) * 2 * (size_t)T;
    const size_t H_bytes = sizeof(uint32_t) * (size_t)T * (size_t)N;
    SH_TRY(g->d_cs.grow(cs_bytes, "hough"));
    SH_TRY(g->h_io.grow(cs_bytes + spec_bytes + (out_H ? H_bytes : 0), "hough"));
    S.have = false;                                                        // (nothing in the slot until this fill has landed)
    SH_TRY(S.d_H.grow(H_bytes, "hough"));
    SH_TRY(S.d_spec.grow(spec_bytes, "hough"));
    SH_TRY(S.d_ext.grow(sizeof(int2) * (size_t)T, "hough"));
    hs_hough_table(T, (int32_t *)g->h_io.p);
    SH_HIP(hipMemcpyAsync(g->d_cs, g->h_io, cs_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (slot == 0) SH_TRY(hs_lat_pack_enqueue(hs, level, world != 0, &M));
    SH_HIP(hipMemsetAsync(S.d_H, 0, H_bytes, ctx->stream));
    k17_vote_arg A;
    A.cls = M.cls; A.w = M.w; A.h = M.h; A.wpr = M.wpr;
    A.mask = site_mask; A.T = T; A.q = q; A.D = D; A.N = N;
    A.cs = g->d_cs;
    A.tiles_x = sh_div_up(M.w, K17_TILE);
    A.H = S.d_H;
    // (at most 256 x 256 tiles and 16 chunks)
    hipLaunchKernelGGL(k17_vote, dim3((unsigned)(A.tiles_x * sh_div_up(M.h, K17_TILE)), (unsigned)sh_div_up(T, K17_ANGLES)), dim3(K17_LANES), 0, ctx->stream, A);
    SH_HIP(hipGetLastError());
    hipLaunchKernelGGL(k17_spectrum, dim3((unsigned)T), dim3(256), 0, ctx->stream, (const uint32_t *)S.d_H, N, T, S.d_spec, S.d_ext);
    SH_HIP(hipGetLastError());
    unsigned char *h_spec = g->h_io + cs_bytes;
    SH_HIP(hipMemcpyAsync(h_spec, S.d_spec, spec_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (out_H) SH_HIP(hipMemcpyAsync(h_spec + spec_bytes, S.d_H, H_bytes, hipMemcpyDeviceToHost, ctx->stream));
    SH_TRY(hs_call_finish(hs));
    const k17_u64 *sp = (const k17_u64 *)h_spec;
    S.spec.assign(sp, sp + T);
    S.level = level; S.world = world; S.mask = site_mask; S.T = T; S.q = q;
    S.w = M.w; S.h = M.h; S.x0 = M.x0; S.y0 = M.y0; S.D = D; S.N = N;
    S.n_sites = (int64_t)sp[T];                                            // (every row's sum is the number of sites; at most 2^28)
    S.have = true;
    out_info[0] = S.w; out_info[1] = S.h; out_info[2] = S.x0; out_info[3] = S.y0; out_info[4] = D; out_info[5] = N; out_info[6] = (int32_t)S.n_sites;
    memcpy(out_spectrum, sp, sizeof(k17_u64) * (size_t)T);
    if (out_H) memcpy(out_H, h_spec + spec_bytes, H_bytes);
    return SLAMHIP_OK;
}

// step 4 over two spectra of T entries
static void hs_hg_rotation(const k17_u64 *hd, const k17_u64 *hsrc, int T, uint64_t *out_cc)
{
    int sh[2] = { 0, 0 };
    const k17_u64 *sp[2] = { hd, hsrc };
    for (int s = 0; s < 2; s++) {
        k17_u64 mx = 0;
        for (int k = 0; k < T; k++) mx = sp[s][k] > mx ? sp[s][k] : mx;
        while ((mx >> sh[s]) >= (1ull << 26)) sh[s]++;
    }
    for (int m = 0; m < T; m++) {
        k17_u64 cc = 0;
        for (int k = 0; k < T; k++) cc += (hd[k] >> sh[0]) * (hsrc[(k - m + T) % T] >> sh[1]);
        out_cc[m] = cc;
    }
}

extern "C" int32_t slamhip_hs_hough_rotation(slamhip_hs *hs, uint64_t *out_cc)
{
    SH_CHECK_ARG(hs && out_cc);
    SH_TRY(hs_hg_check_both(hs));
    const hs_hough *g = hs->hgh;
    hs_hg_rotation(g->slot[0].spec.data(), g->slot[1].spec.data(), g->slot[0].T, out_cc);
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_hough_shifts(slamhip_hs *hs, const int32_t *pairs, int32_t P, slamhip_hough_shift *out_shifts, uint64_t *out_xc)
{
    SH_CHECK_ARG(hs && pairs && out_shifts);
    if (P < 1 || P > HS_HG_MAX_PAIRS) SH_FAIL(SLAMHIP_ERR_INVALID, "hough shifts: P = %d must lie in [1, %d]", P, HS_HG_MAX_PAIRS);
    SH_TRY(hs_hg_check_both(hs));
    hs_hough *g = hs->hgh;
    const hs_hough_slot &Sd = g->slot[0], &Ss = g->slot[1];
    const int T = Sd.T;
    for (int i = 0; i < P; i++)
        if (pairs[2 * i] < 0 || pairs[2 * i] >= 2 * T || pairs[2 * i + 1] < 0 || pairs[2 * i + 1] >= T)
            SH_FAIL(SLAMHIP_ERR_INVALID, "hough shifts: pair %d = (%d, %d); m must lie in [0, %d), k in [0, %d)", i, pairs[2 * i], pairs[2 * i + 1], 2 * T, T);
    const int NX = Sd.N + Ss.N - 1;
    if (out_xc && (int64_t)P * NX > HS_HG_MAX_XC) SH_FAIL(SLAMHIP_ERR_INVALID, "hough shifts: the XC arrays of %d pairs x %d shifts, more than 2^22", P, NX);
    slamhip_ctx *ctx = hs->ctx;
    SH_TRY(hs_call_begin(hs));
    const int blocks = sh_div_up(NX, K17X_LANES);
    const size_t pair_bytes = sizeof(int32_t) * 2 * (size_t)P, rec_bytes = sizeof(slamhip_hough_shift) * (size_t)P;
    const size_t xc_bytes = out_xc ? sizeof(k17_u64) * (size_t)P * NX : 0, part_bytes = sizeof(k17x_part) * (size_t)P * blocks;
    SH_TRY(g->d_pairs.grow(pair_bytes, "hough shifts"));
    SH_TRY(g->d_out.grow(rec_bytes + xc_bytes + part_bytes, "hough shifts"));   // (every part a multiple of 8 bytes)
    SH_TRY(g->h_io.grow(rec_bytes + xc_bytes + pair_bytes, "hough shifts"));
    int32_t *h_pairs = (int32_t *)(g->h_io + rec_bytes + xc_bytes);
    memcpy(h_pairs, pairs, pair_bytes);
    SH_HIP(hipMemcpyAsync(g->d_pairs, h_pairs, pair_bytes, hipMemcpyHostToDevice, ctx->stream));
    k17x_arg X;
    X.Hd = Sd.d_H; X.Hs = Ss.d_H; X.Nd = Sd.N; X.Ns = Ss.N; X.T = T;
    X.extd = Sd.d_ext; X.exts = Ss.d_ext;
    X.pairs = g->d_pairs; X.blocks = blocks;
    X.xc = out_xc ? (k17_u64 *)(g->d_out + rec_bytes) : (k17_u64 *)nullptr;
    X.part = (k17x_part *)(g->d_out + rec_bytes + xc_bytes);
    // (at most 256 pairs x 513 blocks)
    hipLaunchKernelGGL(k17_xcorr, dim3((unsigned)(P * blocks)), dim3(K17X_LANES), 0, ctx->stream, X);
    SH_HIP(hipGetLastError());
    hipLaunchKernelGGL(k17_xcorr_finish, dim3((unsigned)P), dim3(64), 0, ctx->stream, (const k17x_part *)X.part, blocks, (slamhip_hough_shift *)g->d_out.p);
    SH_HIP(hipGetLastError());
    SH_HIP(hipMemcpyAsync(g->h_io, g->d_out, rec_bytes + xc_bytes, hipMemcpyDeviceToHost, ctx->stream));
    SH_TRY(hs_call_finish(hs));
    memcpy(out_shifts, g->h_io, rec_bytes);
    if (out_xc) memcpy(out_xc, g->h_io + rec_bytes, xc_bytes);
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_hs_hough_clear(slamhip_hs *hs)
{
    SH_CHECK_ARG(hs);
    if (!hs->hgh) return SLAMHIP_OK;
    SH_TRY(hs_call_begin(hs));
    SH_TRY(hs_call_finish(hs));                                            // (the blocks are idle behind it)
    hs_unit_drop<&slamhip_hs::hgh>(hs);
    return SLAMHIP_OK;
}

// ---- CPU-side test hooks: hs_hough.h -- the text the kernels run -- in plain loops -----------------------------------------------
extern "C" int32_t slamhip_debug_hough_table(int32_t T, int32_t *out_cs)
{
    SH_CHECK_ARG(out_cs);
    SH_TRY(hs_hg_check_T_q(T, 0));
    hs_hough_table(T, out_cs);
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_debug_hough(const uint8_t *cls, int32_t cw, int32_t ch, int32_t site_mask, int32_t T, int32_t q, uint32_t *out_H,
                                       uint64_t *out_spectrum)
{
    SH_CHECK_ARG(cls && (out_H || out_spectrum) && cw >= 1 && ch >= 1 && cw <= HS_HG_MAX_DIM && ch <= HS_HG_MAX_DIM);
    if (site_mask < 1 || site_mask > 7) SH_FAIL(SLAMHIP_ERR_INVALID, "hough: site_mask = %d must lie in [1, 7]", site_mask);
    SH_TRY(hs_hg_check_T_q(T, q));
    const int D = hs_hough_D(cw, ch), N = hs_hough_N(D, q);
    if ((int64_t)T * N > HS_HG_MAX_BINS) SH_FAIL(SLAMHIP_ERR_INVALID, "hough: T * N = %d * %d bins, more than 2^24", T, N);
    const int wpr = (cw + 15) / 16;
    std::vector<uint32_t> packed((size_t)wpr * ch, 0u);
    for (int cy = 0; cy < ch; cy++)
        for (int cx = 0; cx < cw; cx++) packed[(size_t)cy * wpr + (cx >> 4)] |= (uint32_t)(cls[(size_t)cy * cw + cx] & 3u) << (2 * (cx & 15));
    std::vector<int32_t> cs(2 * (size_t)T);
    hs_hough_table(T, cs.data());
    std::vector<uint32_t> H((size_t)T * N, 0u);
    for (int y = 0; y < ch; y++)
        for (int x32 = 0; x32 < cw; x32 += 32) {
            uint32_t word = hs_hough_site_word(packed.data() + (size_t)y * wpr, cw, x32, site_mask);
            while (word) {
                const int x = x32 + hs_df_ctz(word);
                word &= word - 1u;
                for (int k = 0; k < T; k++) H[(size_t)k * N + hs_hough_bin(x, y, cs[k], cs[T + k], D, q)]++;
            }
        }
    if (out_H) memcpy(out_H, H.data(), sizeof(uint32_t) * H.size());
    if (out_spectrum)
        for (int k = 0; k < T; k++) {
            uint64_t s = 0;
            for (int p = 0; p < N; p++) s += (uint64_t)H[(size_t)k * N + p] * H[(size_t)k * N + p];
            out_spectrum[k] = s;
        }
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_debug_hough_rotation(const uint64_t *spectrum_d, const uint64_t *spectrum_s, int32_t T, uint64_t *out_cc)
{
    SH_CHECK_ARG(spectrum_d && spectrum_s && out_cc);
    SH_TRY(hs_hg_check_T_q(T, 0));
    static_assert(sizeof(k17_u64) == sizeof(uint64_t), "one 64-bit word");
    hs_hg_rotation((const k17_u64 *)spectrum_d, (const k17_u64 *)spectrum_s, T, out_cc);
    return SLAMHIP_OK;
}

extern "C" int32_t slamhip_debug_hough_xcorr(const uint32_t *A, int32_t Nd, const uint32_t *B, int32_t Ns, int32_t flip, uint64_t *out_xc,
                                             slamhip_hough_shift *out_shift)
{
    SH_CHECK_ARG(A && B && out_shift && Nd >= 1 && Ns >= 1 && Nd <= 65537 && Ns <= 65537 && (flip == 0 || flip == 1));
    k17_u64 best = 0, sum = 0;
    int shift = 0, ties = 0;
    for (int d = -(Ns - 1); d <= Nd - 1; d++) {
        k17_u64 v = 0;
        const int p0 = d < 0 ? -d : 0, p1 = Ns - 1 < Nd - 1 - d ? Ns - 1 : Nd - 1 - d;      // p' + d in [0, Nd)
        for (int pp = p0; pp <= p1; pp++) v += (k17_u64)A[pp + d] * B[hs_hough_b_index(Ns, flip, pp)];
        if (out_xc) out_xc[d + Ns - 1] = v;
        hs_hough_rec_add(&best, &shift, &ties, v, d, 1);
        sum += v;
    }
    out_shift->best_shift = shift; out_shift->n_ties = ties; out_shift->best_value = best; out_shift->sum = sum;
    return SLAMHIP_OK;
}
