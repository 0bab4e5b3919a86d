// hs_nav_host.h -- host-only declarations that hs_nav.hip and hs_rollout.hip share (the part of hs_internal.h's hs_nav section that
// needs <vector>).
#pragma once
#include "hs_internal.h"
#include <vector>

// hs_nav.hip: steps 1 to 4 of slamhip_hs_nav_field over a caller's class array for the two hooks (slamhip_debug_nav_field,
// slamhip_debug_rollouts): the traversable words, the costs by a sequential Dijkstra, and the counters K11_C_TRAV, K11_C_USED and
// K11_C_BLOCKED.  The arguments are checked by the caller.
int32_t hs_nav_debug_costs(const uint8_t *cls, int32_t cw, int32_t ch, int32_t site_mask, int32_t clearance, uint32_t max_cost, const int32_t *sources,
                           int32_t S, std::vector<uint32_t> &tw, std::vector<uint32_t> &cost, uint32_t ctr[K11_CTRS]);
