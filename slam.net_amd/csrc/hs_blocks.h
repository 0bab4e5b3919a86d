// hs_blocks.h -- what the host halves of the Hector units K7 .. K15 share: the blocks a unit keeps between calls, the unit's struct
// made on first use, and the frame of a blocking call.  Host code only.
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
