// hs_blocks.h -- what the host halves of the Hector units K7 .. K27 share: the owning block a unit keeps its device and pinned
// memory in (hs_block), the unit's struct made on first use and the table it is dropped through (hs_unit, hs_unit_drop,
// hs_units_drop_all), the count of live blocks, the frame of a blocking call, and the frame of a pose batch (K8, K9, K16).
// Host code only.
#pragma once
#include "hs_internal.h"
#include <atomic>
#include <new>
#include <type_traits>
#include <utility>

// the three kinds of memory a unit's block lives in
enum hs_mem {
    HS_MEM_DEVICE,                         // hipMalloc
    HS_MEM_PINNED,                         // hipHostMallocDefault: what copies leave from and arrive in
    HS_MEM_PINNED_VISIBLE,                 // hipHostMallocMapped | hipHostMallocCoherent: what a kernel stores into and the host reads
};

// the four allocation calls of a block; tests/blocks_selftest.hip alone defines HS_BLOCKS_SELFTEST and its own counting stand-ins
#ifdef HS_BLOCKS_SELFTEST
#define HS_BLOCK_MALLOC selftest_malloc
#define HS_BLOCK_HOST_MALLOC selftest_host_malloc
#define HS_BLOCK_FREE selftest_free
#define HS_BLOCK_HOST_FREE selftest_host_free
#else
#define HS_BLOCK_MALLOC hipMalloc
#define HS_BLOCK_HOST_MALLOC hipHostMalloc
#define HS_BLOCK_FREE hipFree
#define HS_BLOCK_HOST_FREE hipHostFree
#endif

// the live blocks of every hs of the process and their bytes (hector.hip; slamhip_debug_live_blocks)
extern std::atomic<int64_t> hs_live_blocks, hs_live_bytes;

static inline void hs_block_free(void *p, size_t cap, hs_mem kind)
{
    if (kind == HS_MEM_DEVICE) (void)HS_BLOCK_FREE(p); else (void)HS_BLOCK_HOST_FREE(p);
    hs_live_blocks.fetch_sub(1, std::memory_order_relaxed);
    hs_live_bytes.fetch_sub((int64_t)cap, std::memory_order_relaxed);
}
static inline int32_t hs_block_alloc(void **p, size_t want, hs_mem kind, const char *who)
{
    const hipError_t e = kind == HS_MEM_DEVICE ? HS_BLOCK_MALLOC(p, want)
                       : HS_BLOCK_HOST_MALLOC(p, want, kind == HS_MEM_PINNED_VISIBLE ? (hipHostMallocMapped | hipHostMallocCoherent) : hipHostMallocDefault);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        *p = nullptr;
        SH_FAIL(SLAMHIP_ERR_NOMEM, "%s: allocation of %zu bytes of %s memory failed", who, want, kind == HS_MEM_DEVICE ? "device" : "pinned host");
    }
    hs_live_blocks.fetch_add(1, std::memory_order_relaxed);
    hs_live_bytes.fetch_add((int64_t)want, std::memory_order_relaxed);
    return SLAMHIP_OK;
}

// A block of T in memory of one KIND, owned: the pointer and the capacity in bytes, released by the destructor, not copyable.
// It reads as the pointer wherever one is wanted (a kernel's argument record, pointer arithmetic, memcpy).
template <typename T, hs_mem KIND>
struct hs_block {
    T *p = nullptr; size_t cap = 0;
    hs_block() = default;
    hs_block(const hs_block &) = delete;
    hs_block &operator=(const hs_block &) = delete;
    ~hs_block() { release(); }
    operator T *() const { return p; }
    void release() { if (p) hs_block_free(p, cap, KIND); p = nullptr; cap = 0; }
    void swap(hs_block &o) { std::swap(p, o.p); std::swap(cap, o.cap); }
    // At least `want` bytes: the block that is there if it is large enough, else a new one -- what the old one held is gone, and
    // after a failure the block is empty.  The caller's blocks are idle: every blocking call waits for its own launches, and one
    // that timed out has poisoned the context.
    int32_t grow(size_t want, const char *who)
    {
        if (cap >= want) return SLAMHIP_OK;
        release();
        void *q = nullptr;
        SH_TRY(hs_block_alloc(&q, want, KIND, who));
        p = (T *)q; cap = want;
        return SLAMHIP_OK;
    }
};

// A unit's struct, made by its first use and kept (value-initialised: nothing allocated yet), and how it is dropped: deleted --
// its blocks go by their destructors -- and the slot nulled.  The first use records the drop in the table of slamhip_hs, a slot
// once however often it is dropped and made again; hs_units_drop_all is slamhip_hs_destroy's walk (the caller has drained the
// stream), and a *_clear entry point calls hs_unit_drop behind its own wait.
template <auto SLOT>
void hs_unit_drop(slamhip_hs *hs)
{
    delete (hs->*SLOT);
    hs->*SLOT = nullptr;
}
template <auto SLOT>
static inline int32_t hs_unit(slamhip_hs *hs)
{
    if (hs->*SLOT) return SLAMHIP_OK;
    typedef std::remove_pointer_t<std::remove_reference_t<decltype(hs->*SLOT)>> T;
    int i = 0;
    while (i < hs->n_units && hs->unit_drop[i] != &hs_unit_drop<SLOT>) i++;
    if (i == HS_MAX_UNITS) SH_FAIL(SLAMHIP_ERR_STATE, "the unit table is full");
    hs->*SLOT = new (std::nothrow) T();
    if (!(hs->*SLOT)) SH_FAIL(SLAMHIP_ERR_NOMEM, "out of host memory");
    if (i == hs->n_units) hs->unit_drop[hs->n_units++] = &hs_unit_drop<SLOT>;
    return SLAMHIP_OK;
}
static inline void hs_units_drop_all(slamhip_hs *hs)
{
    for (int i = 0; i < hs->n_units; i++) hs->unit_drop[i](hs);
    hs->n_units = 0;
}

// The frame of a blocking call.  _begin: after the call's own argument refusals, before anything is planned or allocated.
// _finish: behind the call's last launch or copy -- when it returns the operator's stream has drained up to there, which the books
// of the scan's two device blocks (pts_use, slamhip_hs_set_scan) are told here and nowhere else.
static inline int32_t hs_call_begin(slamhip_hs *hs)
{
    if (hs->ctx->poisoned) SH_FAIL(SLAMHIP_ERR_TIMEOUT, "the context was poisoned by a blocking wait that timed out; destroy it");
    SH_HIP(hipSetDevice(hs->ctx->device));
    return SLAMHIP_OK;
}
static inline int32_t hs_call_finish(slamhip_hs *hs)
{
    SH_HIP(hipEventRecord(hs->ev_call, hs->ctx->stream));
    SH_TRY(sh_event_wait(hs->ctx, hs->ev_call));
    hs->launch_done = hs->launch_count;
    return SLAMHIP_OK;
}

// ---- a pose batch: K8's trace, K9's score, K16's pairs ---------------------------------------------------------------
// One launch on B poses x chunks of the scan's points, which leaves B summaries (zeroed in-stream, added to by the workgroups) and,
// if asked for, a record per pose and point behind them.  The blocks: the poses in device memory, the device block of the results
// (a field call's rectangle too), and the pinned block the results reach the host through, the poses staged behind them.
struct hs_pose_batch {
    hs_block<float, HS_MEM_DEVICE> d_poses;
    hs_block<unsigned char, HS_MEM_DEVICE> d_out;
    hs_block<unsigned char, HS_MEM_PINNED> h_io;
};

// What such a call refuses for B, the scan and the records, for a scan of n_points (scan_is_set false: the caller is about to set
// one, so its absence is no error).  K8 refuses `world` between B and the scan; K9 and K16 have refused it before they come here.
static inline int32_t hs_pose_batch_check(const char *who, int32_t B, int max_poses, int32_t world, const char *records, bool want_records,
                                          int n_points, bool scan_is_set, int log2_max_records)
{
    if (B < 1 || B > max_poses) SH_FAIL(SLAMHIP_ERR_INVALID, "%s: B = %d must lie in [1, %d]", who, B, max_poses);
    if (world != 0 && world != 1) SH_FAIL(SLAMHIP_ERR_INVALID, "%s: world = %d must be 0 (the window) or 1 (the world)", who, world);
    if (scan_is_set && n_points <= 0) SH_FAIL(SLAMHIP_ERR_STATE, "%s: no scan (slamhip_hs_set_scan first)", who);
    if (want_records && (int64_t)B * n_points > ((int64_t)1 << log2_max_records))
        SH_FAIL(SLAMHIP_ERR_INVALID, "%s: %s records of %d poses x %d points, more than 2^%d", who, records, B, n_points, log2_max_records);
    return SLAMHIP_OK;
}

// the launch's workgroups per pose, refused if B times that is more than a grid takes: behind hs_call_begin, ahead of the call's plan
static inline int32_t hs_pose_batch_chunks(const char *who, int B, int n_points, int lanes, int *chunks)
{
    *chunks = sh_div_up(n_points, lanes);
    if ((int64_t)B * *chunks > (int64_t)INT32_MAX)
        SH_FAIL(SLAMHIP_ERR_INVALID, "%s: %d poses x %d points, more workgroups than one launch takes", who, B, n_points);
    return SLAMHIP_OK;
}

// _begin, behind the call's plan: the blocks grown, the poses staged behind the 8-byte-rounded results and sent, the scan flushed,
// the summaries zeroed.  The caller enqueues what its kernel reads and the kernel; the summaries are d_out, the records d_out +
// sum_bytes.  _finish: the results fetched, the call's wait, the caller's arrays filled (rec_bytes 0: no records were asked for).
static inline int32_t hs_pose_batch_begin(slamhip_hs *hs, hs_pose_batch *pb, const char *who, const float *poses, int B, size_t sum_bytes, size_t rec_bytes)
{
    const size_t pose_bytes = sizeof(float) * 3 * (size_t)B;
    const size_t out_bytes = (sum_bytes + rec_bytes + 7) & ~(size_t)7;
    SH_TRY(pb->d_poses.grow(pose_bytes, who));
    SH_TRY(pb->d_out.grow(out_bytes, who));
    SH_TRY(pb->h_io.grow(out_bytes + pose_bytes, who));
    float *h_poses = (float *)(pb->h_io + out_bytes);
    memcpy(h_poses, poses, pose_bytes);
    SH_TRY(hs_flush_scan(hs));
    SH_HIP(hipMemcpyAsync(pb->d_poses, h_poses, pose_bytes, hipMemcpyHostToDevice, hs->ctx->stream));
    SH_HIP(hipMemsetAsync(pb->d_out, 0, sum_bytes, hs->ctx->stream));
    return SLAMHIP_OK;
}
static inline int32_t hs_pose_batch_finish(slamhip_hs *hs, hs_pose_batch *pb, size_t sum_bytes, size_t rec_bytes, void *out_summaries, void *out_records)
{
    SH_HIP(hipMemcpyAsync(pb->h_io, pb->d_out, sum_bytes + rec_bytes, hipMemcpyDeviceToHost, hs->ctx->stream));
    SH_TRY(hs_call_finish(hs));
    memcpy(out_summaries, pb->h_io, sum_bytes);
    if (rec_bytes) memcpy(out_records, pb->h_io + sum_bytes, rec_bytes);
    return SLAMHIP_OK;
}
