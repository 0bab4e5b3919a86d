// backing_plan.h -- the planner of the scrolling window's backing store (slamhip_hs_set_backing): which cells leave the window
// with a shift, which come into it, and which world tile each of them belongs to.  Pure host code, no HIP: the directory of the
// tiles lives on the host, which knows the origin and every shift, so nothing is read from the device to plan a shift.
//
// World cell of window cell (x, y) on level l: X = (ox >> l) + x, Y = (oy >> l) + y (origins are multiples of 1 << (levels - 1):
// the shift is exact).  A tile is T x T cells of one level, T a power of two; tile index floor(X / T), local coordinate
// X - T * floor(X / T) -- floor division and floor modulus, origins go negative.
// A job is the intersection of one tile with one rectangle of the departing region (cells of the OLD window whose new coordinates
// fall outside the level, in the old window's coordinates: evict jobs) or of the arriving region (cells of the NEW window whose
// source falls outside the level, in the new window's coordinates: restore jobs).  A region is the window minus the rectangle
// both windows share -- up to four rectangles: the band above it and the band below it over the full width, and the strips left
// and right of it -- so a tile in the region's corner gives more than one job.  World coordinates use the unclamped dx >> l: a
// move by a level's size or more makes the whole old window depart and the whole new one arrive.
// Order: level 0 first; within a level evict jobs, then restore jobs; within each, row-major by tile (ty, tx); jobs of one tile
// in the order band above, band below, left strip, right strip.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "../../include/slamhip.h"

static inline int64_t bp_floor_div(int64_t a, int64_t b)                  // b > 0
{
    const int64_t q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

struct bp_rect { int x0, y0, x1, y1; };                                   // [x0, x1) x [y0, y1), window coordinates

// The jobs of one region of one level: the window w x h, whose cell (0, 0) is world cell (OX, OY), minus the kept rectangle
// [kx0, kx1) x [ky0, ky1) (empty: the whole window).
static inline void bp_region_jobs(int level, int kind, int w, int h, int64_t OX, int64_t OY, int kx0, int kx1, int ky0, int ky1,
                                  int T, std::vector<slamhip_backing_job> &out)
{
    bp_rect rects[4];
    int nr = 0;
    if (kx0 >= kx1 || ky0 >= ky1) rects[nr++] = { 0, 0, w, h };
    else {
        if (ky0 > 0) rects[nr++] = { 0, 0, w, ky0 };
        if (ky1 < h) rects[nr++] = { 0, ky1, w, h };
        if (kx0 > 0) rects[nr++] = { 0, ky0, kx0, ky1 };
        if (kx1 < w) rects[nr++] = { kx1, ky0, w, ky1 };
    }
    std::vector<slamhip_backing_job> row;
    const int64_t ty_first = bp_floor_div(OY, T), ty_last = bp_floor_div(OY + h - 1, T);
    for (int64_t ty = ty_first; ty <= ty_last; ty++) {
        const int64_t ty0 = ty * T - OY;                                  // the tile's first row in window coordinates
        row.clear();
        for (int r = 0; r < nr; r++) {
            const bp_rect &R = rects[r];
            const int y0 = (int)std::max<int64_t>(R.y0, ty0), y1 = (int)std::min<int64_t>(R.y1, ty0 + T);
            if (y0 >= y1) continue;
            const int64_t tx_first = bp_floor_div(OX + R.x0, T), tx_last = bp_floor_div(OX + R.x1 - 1, T);
            for (int64_t tx = tx_first; tx <= tx_last; tx++) {
                const int64_t tx0 = tx * T - OX;
                const int x0 = (int)std::max<int64_t>(R.x0, tx0), x1 = (int)std::min<int64_t>(R.x1, tx0 + T);
                slamhip_backing_job j;
                j.level = level; j.kind = kind;
                j.wx = x0; j.wy = y0; j.nx = x1 - x0; j.ny = y1 - y0;
                j.tx = tx; j.ty = ty;
                j.lx = (int32_t)(x0 - tx0); j.ly = (int32_t)(y0 - ty0);
                row.push_back(j);
            }
        }
        std::stable_sort(row.begin(), row.end(), [](const slamhip_backing_job &a, const slamhip_backing_job &b) { return a.tx < b.tx; });
        out.insert(out.end(), row.begin(), row.end());
    }
}

// The job list of one shift by (dx, dy) level-0 cells of a pyramid whose level 0 is w0 x h0 (every further level half of it,
// rounded down) and whose window lies at (ox, oy) BEFORE the shift.
static inline void bp_plan(int levels, int w0, int h0, int64_t ox, int64_t oy, int32_t dx, int32_t dy, int T,
                           std::vector<slamhip_backing_job> &out)
{
    out.clear();
    int w = w0, h = h0;
    for (int l = 0; l < levels; l++) {
        const int64_t sx = dx >> l, sy = dy >> l;                         // (arithmetic shifts: floor)
        const int64_t OX = ox >> l, OY = oy >> l;
        // old cell (x, y) stays if 0 <= x - sx < w: x in [sx, w + sx); new cell (x, y) has a source if 0 <= x + sx < w
        const int ex0 = (int)std::min<int64_t>(w, std::max<int64_t>(0, sx)), ex1 = (int)std::max<int64_t>(0, std::min<int64_t>(w, w + sx));
        const int ey0 = (int)std::min<int64_t>(h, std::max<int64_t>(0, sy)), ey1 = (int)std::max<int64_t>(0, std::min<int64_t>(h, h + sy));
        bp_region_jobs(l, SLAMHIP_BACKING_EVICT, w, h, OX, OY, ex0, ex1, ey0, ey1, T, out);
        const int rx0 = (int)std::min<int64_t>(w, std::max<int64_t>(0, -sx)), rx1 = (int)std::max<int64_t>(0, std::min<int64_t>(w, w - sx));
        const int ry0 = (int)std::min<int64_t>(h, std::max<int64_t>(0, -sy)), ry1 = (int)std::max<int64_t>(0, std::min<int64_t>(h, h - sy));
        bp_region_jobs(l, SLAMHIP_BACKING_RESTORE, w, h, OX + sx, OY + sy, rx0, rx1, ry0, ry1, T, out);
        w /= 2; h /= 2;
    }
}
