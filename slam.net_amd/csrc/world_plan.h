// world_plan.h -- the planner of slamhip_hs_world_cells_upload: which cells of the caller's rectangle go into the window, which
// into which world tile.  Pure host code, no HIP, as backing_plan.h is for the shift (whose floor division it uses): the host
// knows the origin and the tile directory, so nothing is read from the device to plan an upload.
//
// The rectangle is rw x rh cells of ONE level whose cell (0, 0) is world cell (x0, y0); the level's window is w x h cells whose
// cell (0, 0) is world cell (OX, OY) = (win_ox >> level, win_oy >> level).  A job is a piece of the rectangle, nx x ny cells from
// rectangle cell (sx, sy), that lies wholly in the window (kind SLAMHIP_WORLD_WINDOW: (lx, ly) its first cell in window
// coordinates; tx = ty = 0) or wholly in one tile and outside the window (kind SLAMHIP_WORLD_TILE: tile (tx, ty) by floor
// division, (lx, ly) its first cell in the tile's local coordinates).
// Order: the window job first (at most one).  Then the rectangle as the frame and the window as the kept rectangle, cut by
// bp_cut_tiles in the order stated at the top of backing_plan.h.  T = 0 (backing off): the window job alone.
#pragma once
#include "backing_plan.h"

static inline void wp_plan(int w, int h, int64_t OX, int64_t OY, int64_t x0, int64_t y0, int rw, int rh, int T,
                           std::vector<slamhip_world_job> &out)
{
    out.clear();
    // the window in rectangle coordinates, clamped to the rectangle: [kx0, kx1) x [ky0, ky1)
    const int kx0 = (int)std::min<int64_t>(rw, std::max<int64_t>(0, OX - x0)), kx1 = (int)std::max<int64_t>(0, std::min<int64_t>(rw, OX + w - x0));
    const int ky0 = (int)std::min<int64_t>(rh, std::max<int64_t>(0, OY - y0)), ky1 = (int)std::max<int64_t>(0, std::min<int64_t>(rh, OY + h - y0));
    if (kx0 < kx1 && ky0 < ky1) {
        slamhip_world_job j;
        j.kind = SLAMHIP_WORLD_WINDOW; j.sx = kx0; j.sy = ky0; j.nx = kx1 - kx0; j.ny = ky1 - ky0;
        j.lx = (int32_t)(x0 + kx0 - OX); j.ly = (int32_t)(y0 + ky0 - OY); j.pad = 0; j.tx = 0; j.ty = 0;
        out.push_back(j);
    }
    if (T <= 0) return;
    bp_cut_tiles(rw, rh, x0, y0, kx0, kx1, ky0, ky1, T, [&](const bp_piece &p) {
        slamhip_world_job j;
        j.kind = SLAMHIP_WORLD_TILE; j.sx = p.x0; j.sy = p.y0; j.nx = p.nx; j.ny = p.ny;
        j.lx = p.lx; j.ly = p.ly; j.pad = 0; j.tx = p.tx; j.ty = p.ty;
        out.push_back(j);
    });
}
