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
// in the order band above, band below, left strip, right strip.  Stated here only, produced by bp_cut_tiles only
// (the shift's regions below, the world upload's rectangle in world_plan.h).
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

struct bp_rect { int x0, y0, x1, y1; };                                   // [x0, x1) x [y0, y1), frame coordinates

// A frame of w x h cells minus the kept rectangle [kx0, kx1) x [ky0, ky1) (empty: the whole frame), in the order above.  -> how many
static inline int bp_frame_rects(int w, int h, int kx0, int kx1, int ky0, int ky1, bp_rect out[4])
{
    int nr = 0;
    if (kx0 >= kx1 || ky0 >= ky1) out[nr++] = { 0, 0, w, h };
    else {
        if (ky0 > 0) out[nr++] = { 0, 0, w, ky0 };
        if (ky1 < h) out[nr++] = { 0, ky1, w, h };
        if (kx0 > 0) out[nr++] = { 0, ky0, kx0, ky1 };
        if (kx1 < w) out[nr++] = { kx1, ky0, w, ky1 };
    }
    return nr;
}

// nx x ny cells from frame cell (x0, y0), which is cell (lx, ly) of tile (tx, ty)
struct bp_piece { int x0, y0, nx, ny, lx, ly; int64_t tx, ty; };

// THE tile cutter: the frame w x h, whose cell (0, 0) is world cell (X0, Y0), minus the kept rectangle, cut by tiles of T cells;
// emit(const bp_piece &) for every piece, row-major by tile, one tile's pieces in rectangle order.
template <typename F>
static inline void bp_cut_tiles(int w, int h, int64_t X0, int64_t Y0, int kx0, int kx1, int ky0, int ky1, int T, F &&emit)
{
    bp_rect rects[4];
    const int nr = bp_frame_rects(w, h, kx0, kx1, ky0, ky1, rects);
    std::vector<bp_piece> row;
    const int64_t ty_first = bp_floor_div(Y0, T), ty_last = bp_floor_div(Y0 + h - 1, T);
    for (int64_t ty = ty_first; ty <= ty_last; ty++) {
        const int64_t ty0 = ty * T - Y0;                                  // the tile's first row in frame coordinates
        row.clear();
        for (int r = 0; r < nr; r++) {
            const bp_rect &R = rects[r];
            const int y0 = (int)std::max<int64_t>(R.y0, ty0), y1 = (int)std::min<int64_t>(R.y1, ty0 + T);
            if (y0 >= y1) continue;
            const int64_t tx_first = bp_floor_div(X0 + R.x0, T), tx_last = bp_floor_div(X0 + R.x1 - 1, T);
            for (int64_t tx = tx_first; tx <= tx_last; tx++) {
                const int64_t tx0 = tx * T - X0;
                const int x0 = (int)std::max<int64_t>(R.x0, tx0), x1 = (int)std::min<int64_t>(R.x1, tx0 + T);
                row.push_back({ x0, y0, x1 - x0, y1 - y0, (int)(x0 - tx0), (int)(y0 - ty0), tx, ty });
            }
        }
        std::stable_sort(row.begin(), row.end(), [](const bp_piece &a, const bp_piece &b) { return a.tx < b.tx; });
        for (const bp_piece &p : row) emit(p);
    }
}

// The jobs of one region of one level: the window w x h, whose cell (0, 0) is world cell (OX, OY), minus the kept rectangle.
static inline void bp_region_jobs(int level, int kind, int w, int h, int64_t OX, int64_t OY, int kx0, int kx1, int ky0, int ky1,
                                  int T, std::vector<slamhip_backing_job> &out)
{
    bp_cut_tiles(w, h, OX, OY, kx0, kx1, ky0, ky1, T, [&](const bp_piece &p) {
        slamhip_backing_job j;
        j.level = level; j.kind = kind; j.wx = p.x0; j.wy = p.y0; j.nx = p.nx; j.ny = p.ny;
        j.tx = p.tx; j.ty = p.ty; j.lx = p.lx; j.ly = p.ly;
        out.push_back(j);
    });
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
