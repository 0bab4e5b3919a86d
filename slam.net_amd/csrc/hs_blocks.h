// hs_blocks.h -- what the host halves of the Hector units K7 .. K19 share: the blocks a unit keeps between calls, the unit's struct
// made on first use, the frame of a blocking call, and the frame of a pose batch (K8, K9, K16).  Host code only.
#pragma once
#include "hs_internal.h"
#include <new>

// the three kinds of memory a unit's block lives in
enum hs_mem {
    HS_MEM_DEVICE,                         // hipMalloc
    HS_MEM_PINNED,                         // hipHostMallocDefault: what copies leave from and arrive in
    HS_MEM_PINNED_VISIBLE,                 // hipHostMallocMapped | hipHostMallocCoherent: what a kernel stores into and the host reads
};

static inline void hs_release(void **p, size_t *cap, hs_mem kind)          // (cap: nullptr for a block of fixed size)
{
    if (*p) { if (kind == HS_MEM_DEVICE) (void)hipFree(*p); else (void)hipHostFree(*p); }
    *p = nullptr;
    if (cap) *cap = 0;
}

// A block of at least `want` bytes: the one that is there if it is large enough, else a new one -- what the old one held is gone.
// The caller's blocks are idle: every blocking call waits for its own launches, and one that timed out has poisoned the context.
static inline int32_t hs_grow(void **p, size_t *cap, size_t want, hs_mem kind, const char *who)
{
    if (*cap >= want) return SLAMHIP_OK;
    hs_release(p, cap, kind);
    const hipError_t e = kind == HS_MEM_DEVICE ? hipMalloc(p, want)
                       : hipHostMalloc(p, want, kind == HS_MEM_PINNED_VISIBLE ? (hipHostMallocMapped | hipHostMallocCoherent) : hipHostMallocDefault);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        *p = nullptr;
        SH_FAIL(SLAMHIP_ERR_NOMEM, "%s: allocation of %zu bytes of %s memory failed", who, want, kind == HS_MEM_DEVICE ? "device" : "pinned host");
    }
    *cap = want;
    return SLAMHIP_OK;
}

// a unit's struct, made by its first use and kept (value-initialised: nothing allocated yet)
template <typename T>
static inline int32_t hs_unit(T **slot)
{
    if (!*slot) *slot = new (std::nothrow) T();
    if (!*slot) SH_FAIL(SLAMHIP_ERR_NOMEM, "out of host memory");
    return SLAMHIP_OK;
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
    float *d_poses; size_t cap_poses;
    unsigned char *d_out; size_t cap_out;
    unsigned char *h_io; size_t cap_h;
};

static inline void hs_pose_batch_release(hs_pose_batch *pb)
{
    hs_release((void **)&pb->d_poses, &pb->cap_poses, HS_MEM_DEVICE);
    hs_release((void **)&pb->d_out, &pb->cap_out, HS_MEM_DEVICE);
    hs_release((void **)&pb->h_io, &pb->cap_h, HS_MEM_PINNED);
}

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
    SH_TRY(hs_grow((void **)&pb->d_poses, &pb->cap_poses, pose_bytes, HS_MEM_DEVICE, who));
    SH_TRY(hs_grow((void **)&pb->d_out, &pb->cap_out, out_bytes, HS_MEM_DEVICE, who));
    SH_TRY(hs_grow((void **)&pb->h_io, &pb->cap_h, out_bytes + pose_bytes, HS_MEM_PINNED, who));
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
