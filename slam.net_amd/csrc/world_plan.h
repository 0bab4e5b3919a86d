// world_plan.h -- the planner of slamhip_hs_world_cells_upload: which cells of the caller's rectangle go into the window, which
// into which world tile.  Pure host code, no HIP, as backing_plan.h is for the shift (whose floor division it uses): the host
// knows the origin and the tile directory, so nothing is read from the device to plan an upload.
//
// The rectangle is rw x rh cells of ONE level whose cell (0, 0) is world cell (x0, y0); the level's window is w x h cells whose
// cell (0, 0) is world cell (OX, OY) = (win_ox >> level, win_oy >> level).  A job is a piece of the rectangle, nx x ny cells from
// rectangle cell (sx, sy), that lies wholly in the window (kind SLAMHIP_WORLD_WINDOW: (lx, ly) its first cell in window
// coordinates; tx = ty = 0) or wholly in one tile and outside the window (kind SLAMHIP_WORLD_TILE: tile (tx, ty) by floor
// division, (lx, ly) its first cell in the tile's local coordinates).
// Order: the window job first (at most one).  Then the part of the rectangle outside the window, cut as the backing planner cuts
// a region -- the band above the window over the rectangle's full width, the band below it, the strip left of it, the strip right
// of it (the whole rectangle if it misses the window) -- row-major by tile (ty, tx); the jobs of one tile in that rectangle
// order.  T = 0 (backing off): the window job alone.
#pragma once
#include "backing_plan.h"

static inline void wp_plan(int w, int h, int64_t OX, int64_t OY, int64_t x0, int64_t y0, int rw, int rh, int T,
                           std::vector<slamhip_world_job> &out)
{
    out.clear();
    // the window in rectangle coordinates, clamped to the rectangle: [kx0, kx1) x [ky0, ky1)
    const int kx0 = (int)std::min<int64_t>(rw, std::max<int64_t>(0, OX - x0)), kx1 = (int)std::max<int64_t>(0, std::min<int64_t>(rw, OX + w - x0));
    const int ky0 = (int)std::min<int64_t>(rh, std::max<int64_t>(0, OY - y0)), ky1 = (int)std::max<int64_t>(0, std::min<int64_t>(rh, OY + h - y0));
    const bool meets = kx0 < kx1 && ky0 < ky1;
    if (meets) {
        slamhip_world_job j;
        j.kind = SLAMHIP_WORLD_WINDOW; j.sx = kx0; j.sy = ky0; j.nx = kx1 - kx0; j.ny = ky1 - ky0;
        j.lx = (int32_t)(x0 + kx0 - OX); j.ly = (int32_t)(y0 + ky0 - OY); j.pad = 0; j.tx = 0; j.ty = 0;
        out.push_back(j);
    }
    if (T <= 0) return;
    bp_rect rects[4];
    int nr = 0;
    if (!meets) rects[nr++] = { 0, 0, rw, rh };
    else {
        if (ky0 > 0) rects[nr++] = { 0, 0, rw, ky0 };
        if (ky1 < rh) rects[nr++] = { 0, ky1, rw, rh };
        if (kx0 > 0) rects[nr++] = { 0, ky0, kx0, ky1 };
        if (kx1 < rw) rects[nr++] = { kx1, ky0, rw, ky1 };
    }
    std::vector<slamhip_world_job> row;
    const int64_t ty_first = bp_floor_div(y0, T), ty_last = bp_floor_div(y0 + rh - 1, T);
    for (int64_t ty = ty_first; ty <= ty_last; ty++) {
        const int64_t ty0 = ty * T - y0;                                  // the tile's first row in rectangle coordinates
        row.clear();
        for (int r = 0; r < nr; r++) {
            const bp_rect &R = rects[r];
            const int ry0 = (int)std::max<int64_t>(R.y0, ty0), ry1 = (int)std::min<int64_t>(R.y1, ty0 + T);
            if (ry0 >= ry1) continue;
            const int64_t tx_first = bp_floor_div(x0 + R.x0, T), tx_last = bp_floor_div(x0 + R.x1 - 1, T);
            for (int64_t tx = tx_first; tx <= tx_last; tx++) {
                const int64_t tx0 = tx * T - x0;
                const int rx0 = (int)std::max<int64_t>(R.x0, tx0), rx1 = (int)std::min<int64_t>(R.x1, tx0 + T);
                slamhip_world_job j;
                j.kind = SLAMHIP_WORLD_TILE; j.sx = rx0; j.sy = ry0; j.nx = rx1 - rx0; j.ny = ry1 - ry0;
                j.lx = (int32_t)(rx0 - tx0); j.ly = (int32_t)(ry0 - ty0); j.pad = 0; j.tx = tx; j.ty = ty;
                row.push_back(j);
            }
        }
        std::stable_sort(row.begin(), row.end(), [](const slamhip_world_job &a, const slamhip_world_job &b) { return a.tx < b.tx; });
        out.insert(out.end(), row.begin(), row.end());
    }
}
