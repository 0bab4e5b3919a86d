// hs_scans.h -- the store of keyframe scans (slamhip_hs_scans_add) as its two users see it: K20 (hs_render.hip), which owns and
// fills it, and K21 (hs_scanmatch.hip), which reads the pool and the records.  Host code only.
#pragma once
#include "hs_blocks.h"
#include <vector>

struct k20_scan { long long off; int n; float ox, oy; int pad; };          // a stored scan: where its points lie in the pool, how many, its origin
static_assert(sizeof(k20_scan) == 24, "the record the kernels read");

// What the store keeps: the records, the pool, and the blocks of a render -- the launch's records, matrices and boxes in device
// memory and the pinned block the first two leave the host through (a download's points arrive in it).
struct hs_scans {
    std::vector<k20_scan> recs;
    hs_block<float2, HS_MEM_DEVICE> d_pool; size_t cap_pts, used_pts;   // (points; the block's own cap is bytes)
    hs_block<unsigned char, HS_MEM_DEVICE> d_in;
    hs_block<unsigned char, HS_MEM_PINNED> h_io;
};
