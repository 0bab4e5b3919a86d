// hs_tiles.h -- what the scrolling window's enqueue-only path (hs_window.hip) and the blocking world calls (hs_world.hip) share:
// the tile slot's layout, the row cutter of their job tables, and the backing store's books with the directory's three operations.
#pragma once
#include "hs_internal.h"
#include "backing_plan.h"
#include <map>
#include <tuple>

// the slot layout, t2 = T * T: where the probabilities start, and the whole slot
__host__ __device__ static inline size_t k6p_slot_prob_offset(size_t t2) { return sizeof(slamhip_cell) * t2; }
__host__ __device__ static inline size_t k6p_slot_bytes(size_t t2) { return k6p_slot_prob_offset(t2) + sizeof(float) * t2; }

// THE row cutter: a job of nx x ny cells goes to the device as pieces of whole rows, at most K6P_CELLS cells each (a job wider
// than that: one row per piece), a workgroup per piece.  fn(r0, rows): the piece's first row in the job and how many it has.
#define K6P_CELLS 2048
static inline int hs_piece_rows(int nx) { return K6P_CELLS / nx > 0 ? K6P_CELLS / nx : 1; }
static inline size_t hs_piece_count(int nx, int ny) { return (size_t)((ny + hs_piece_rows(nx) - 1) / hs_piece_rows(nx)); }
template <typename F>
static inline void hs_cut_rows(int nx, int ny, F &&fn)
{
    const int rows = hs_piece_rows(nx);
    for (int r0 = 0; r0 < ny; r0 += rows) fn(r0, ny - r0 < rows ? ny - r0 : rows);
}

// a slot for a new tile, initialised on the stream before its first use; nullptr if none can be had (hs_window.hip)
unsigned char *hs_bk_slot(slamhip_hs *hs);
// n more slots in the pool, all or none: SLAMHIP_ERR_NOMEM leaves the pool and its books as they were (hs_window.hip)
int32_t hs_bk_reserve(slamhip_hs *hs, size_t n);

// the backing store's books: the pool (chunks of slots), the directory (level, ty, tx) -> slot, and the pinned ring the job
// tables reach the device from -- a block of the ring is refilled only after the launch that read it has finished (an event per
// block, the context's bounded wait; with HS_BK_RING launches in flight at most, in steady state that costs no wait)
#define HS_BK_RING 4
struct k6p_job;
struct hs_bk_block { k6p_job *h; size_t cap; hipEvent_t ev; bool in_flight; };
struct hs_bk_chunk { unsigned char *base; size_t slots; };
typedef std::tuple<int, int64_t, int64_t> hs_tile_key;                     // (level, ty, tx)
struct hs_backing {
    int T; uint64_t max_bytes; size_t slot_bytes;
    std::vector<hs_bk_chunk> chunks;
    std::vector<unsigned char *> free_slots;                               // a stack: the lowest address of the newest chunk on top
    std::map<hs_tile_key, unsigned char *> dir;
    int64_t bytes, evicted, restored, dropped;
    hs_bk_block ring[HS_BK_RING]; unsigned ring_next;
    std::vector<slamhip_backing_job> plan;
    std::vector<k6p_job> pieces;

    // the slot of tile (level, ty, tx); nullptr: there is no such tile
    unsigned char *find(int level, int64_t ty, int64_t tx) const
    {
        auto it = dir.find(hs_tile_key(level, ty, tx));
        return it != dir.end() ? it->second : nullptr;
    }
    // ... taking a new one if needed; nullptr: there is none and none can be had (the caller drops the cells)
    unsigned char *find_or_take(slamhip_hs *hs, int level, int64_t ty, int64_t tx)
    {
        unsigned char *slot = find(level, ty, tx);
        if (!slot && (slot = hs_bk_slot(hs)) != nullptr) dir[hs_tile_key(level, ty, tx)] = slot;
        return slot;
    }
    // fn(ty, tx, slot) for every tile of one level, row-major
    template <typename F>
    void for_each_tile(int level, F &&fn) const
    {
        for (auto it = dir.lower_bound(hs_tile_key(level, INT64_MIN, INT64_MIN)); it != dir.end() && std::get<0>(it->first) == level; ++it)
            fn(std::get<1>(it->first), std::get<2>(it->first), it->second);
    }
};
