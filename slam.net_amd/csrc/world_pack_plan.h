// world_pack_plan.h -- the planner of the WORLD class map of the pose-lattice search (k7_pack_world, hs_lattice.hip;
// slamhip_hs_world_lattice_search): which rectangle R of one level the map covers, and which pieces of the window and of the
// level's tiles are packed into it.  Pure host code, no HIP, as world_plan.h is for the world upload (whose cutter it uses): the
// host knows the origin and the tile directory, so nothing is read from the device to plan a search.
//
// The level's window is w x h cells whose cell (0, 0) is world cell (OX, OY) = (win_ox >> level, win_oy >> level); a tile (ty, tx)
// holds world cells [tx T, tx T + T) x [ty T, ty T + T).  R is the bounding box, in WINDOW-FRAME cells, of the window and of every
// tile given, so x0 <= 0, y0 <= 0 and the window always lies in it.  What R does not cover is class 0 by the definition, and so is
// every cell of R that no job writes (a hole between tiles).
// A job is nx x ny cells from cell (sx, sy) of R that come from the window (kind SLAMHIP_WORLD_WINDOW: the whole window, (lx, ly) =
// (0, 0), tx = ty = 0) or from one tile OUTSIDE the window (SLAMHIP_WORLD_TILE: (lx, ly) the first cell in the tile's local
// coordinates) -- the window wins over a tile's older copy, as in the world download.
// Order: the window job first; then the tiles in the order given (the directory's: row-major by (ty, tx)), each tile as the frame
// and the window as the kept rectangle of bp_cut_tiles -- band above the window, band below it, left strip, right strip; a tile
// that lies wholly under the window gives no job.  Jobs are disjoint in cells of R, but their edges fall anywhere in a packed word.
#pragma once
#include "backing_plan.h"

#define WPP_MAX_CELLS ((int64_t)1 << 28)   // of R, its rows padded to whole 16-cell words: 64 MB of packed map

struct wpp_rect { int64_t x0, y0, w, h; };                                // [x0, x0 + w) x [y0, y0 + h), window-frame cells

// tiles: n pairs (ty, tx)
static inline wpp_rect wpp_bounds(int w, int h, int64_t OX, int64_t OY, int T, const int64_t *tiles, size_t n)
{
    int64_t x0 = 0, y0 = 0, x1 = w, y1 = h;
    for (size_t i = 0; i < n; i++) {
        const int64_t ty0 = tiles[2 * i] * T - OY, tx0 = tiles[2 * i + 1] * T - OX;
        x0 = std::min(x0, tx0); x1 = std::max(x1, tx0 + T);
        y0 = std::min(y0, ty0); y1 = std::max(y1, ty0 + T);
    }
    return { x0, y0, x1 - x0, y1 - y0 };
}

// (each side first: the product of two sides of up to 2^61 cells would overflow)
static inline bool wpp_fits(const wpp_rect &R)
{
    return R.w <= WPP_MAX_CELLS && R.h <= WPP_MAX_CELLS && (R.w + 15) / 16 * 16 * R.h <= WPP_MAX_CELLS;
}

// the jobs of an R that fits
static inline void wpp_plan(int w, int h, int64_t OX, int64_t OY, int T, const int64_t *tiles, size_t n, const wpp_rect &R,
                            std::vector<slamhip_world_job> &out)
{
    out.clear();
    slamhip_world_job j;
    j.kind = SLAMHIP_WORLD_WINDOW; j.sx = (int32_t)-R.x0; j.sy = (int32_t)-R.y0; j.nx = w; j.ny = h;
    j.lx = 0; j.ly = 0; j.pad = 0; j.tx = 0; j.ty = 0;
    out.push_back(j);
    for (size_t i = 0; i < n; i++) {
        const int64_t ty = tiles[2 * i], tx = tiles[2 * i + 1];
        const int64_t X0 = tx * T, Y0 = ty * T;
        // the window in the tile's coordinates, clamped to the tile
        const int kx0 = (int)std::min<int64_t>(T, std::max<int64_t>(0, OX - X0)), kx1 = (int)std::max<int64_t>(0, std::min<int64_t>(T, OX + w - X0));
        const int ky0 = (int)std::min<int64_t>(T, std::max<int64_t>(0, OY - Y0)), ky1 = (int)std::max<int64_t>(0, std::min<int64_t>(T, OY + h - Y0));
        bp_cut_tiles(T, T, X0, Y0, kx0, kx1, ky0, ky1, T, [&](const bp_piece &p) {
            slamhip_world_job q;
            q.kind = SLAMHIP_WORLD_TILE;
            q.sx = (int32_t)(X0 + p.x0 - OX - R.x0); q.sy = (int32_t)(Y0 + p.y0 - OY - R.y0);
            q.nx = p.nx; q.ny = p.ny; q.lx = p.lx; q.ly = p.ly; q.pad = 0; q.tx = p.tx; q.ty = p.ty;
            out.push_back(q);
        });
    }
}
