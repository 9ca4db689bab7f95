// topo_summits.h -- the summits of the drawn mesh (topo_summits_*) and the snapping of given peaks to them (topo_summit_snap_*): the
// rule, the window that the kernels (kernels_summits.h) and the emulation's fast path enumerate, and the same answers by brute force.
//
// Posts.  A post is (tile rank, vx, vy) with h = heights[vy * w + vx]; its index is vy * w + vx.  It EXISTS iff surface_tile_ok(tile) and
// surface_height_ok(h): finite sentinels (-32768) are geometry, as everywhere else.  Its direction u is the f64 unit vector
// (cos lat cos lon, cos lat sin lon, sin lat) from the tile's (cos, sin) tables (LosScene::trig), the one ground_vertex_from scales by
// R0 + h; its longitude and latitude are where the mesh puts the vertex: the f32 tile transform widened, f64 from there on
// (summit_lon, summit_lat: only + - x, so device and host agree bit for bit).
//
// Distance.  Between two directions it is R0 |u_a - u_b|: the chord over the sphere, difference first and norm after.  1 - u_a . u_b
// would cancel to nothing for neighbouring posts (topo_cull.h says why: the cosine of 1e-5 rad differs from 1 by 5e-11, and f64 keeps
// five digits of that); the difference of the components keeps them all.  The expression is + - x sqrt only: with -ffp-contract=off on
// both sides, device and g++ agree bit for bit on equal tables.
//
// Domination.  Q dominates P iff both exist and h_Q > h_P, or h_Q == h_P and (rank_Q, index_Q) < (rank_P, index_P).  A strict total
// order: a plateau has exactly one undominated post, its lowest (rank, index), and a post duplicated by an overlapping tile is
// dominated by its lower-rank copy at distance about 0.
//
// Isolation of P: the smallest distance to a post that dominates it among all existing posts of all resident tiles within radius_m
// (d <= radius_m) of P; +inf if there is none.  The nearest dominator is that post; on equal distance the lower (rank, index).  P is a
// SUMMIT of a call iff it exists, h_P >= min_height_m and isolation >= min_isolation_m.  Only resident posts count: near the mosaic's
// border a higher post may stand just outside it, so an isolation reported there is an UPPER BOUND of the true one.
//
// Snap.  For a point (lon, lat) with direction surface_direction(lon, lat) the target is the best existing post within radius_m of it:
// the highest h; on equal h the nearer one, then the lower (rank, index).  None in range: NONE; !surface_point_valid: INVALID.
//
// The window (summit_window): the vertex columns and rows of a tile that can hold a post within `radius` of a centre (lon, lat).  Let
// theta = 2 asin(radius / 2 R0) be the angle the chord `radius` spans.
//   rows     the angular distance of two directions is at least the difference of their latitudes (the meridian arc is the shortest
//            way between two parallels), so a post within theta lies within theta / |scale_y| rows of fy = (model_y - lat) / scale_y
//            + raster_y, formed as surface_lookup forms it.
//   columns  the cap of angular radius theta around a centre of latitude phi touches the meridians at a longitude difference of
//            asin(sin theta / cos phi) -- the right spherical triangle pole / centre / tangent point -- as long as the cap does not
//            hold a pole: sin theta < cos phi and theta < 90 degrees.  Then every post within theta lies within that many degrees
//            / |scale_x| columns of fx = wrap180(lon - model_x) / scale_x + raster_x.  wrap180 takes the tile's columns to lie within 180
//            degrees of its model_x (surface_lookup's reading); a window that would reach across the +-180 seam of that reading, a cap
//            that holds a pole (polar tiles, huge radii) and a ratio within 1e-6 of 1 (where asin is steep) take EVERY column.
//   Both ranges are padded by 1/64 cell -- the f64 rounding of fx, fy, theta, the sines and the tables' entries is 1e-11 of a cell --
//   rounded outwards (floor of the low end, floor of the high end: vertex v lies in [lo, hi] only if floor(lo) <= v <= floor(hi)) and
//   clamped with los_cells.  An empty range skips the tile; anything non-finite selects the whole tile (its posts then decide for
//   themselves: a post of a tile with a NaN model point has a NaN direction, and no distance test holds for it).
//   The window only ENUMERATES: whether a post is in range is decided by its chord alone, so the answer does not depend on how far
//   the window overshoots.  For the same reason a nearest-dominator search may shrink its window to the best distance found so far:
//   the window of radius d holds every post within d (d included, so an equally near post of a lower index is still met).
//
// Blocks.  Block (bx, by) of the raster (kLosBCX x kLosBCY cells, TileDev::block_minmax over its 61 x 16 vertices) OWNS the vertices
// x in [60 bx, 60 bx + 59], y in [15 by, 15 by + 14], the last block of a row or column also the tile's last column or row: every post
// has one owner, and the owner's max bounds it.  A block whose bounds are ordered, finite and not absurd and whose max < h_P holds no
// dominator of P (domination needs h_Q >= h_P); for the snap, a max < the best height so far holds no better target.  Unordered (a
// void block), non-finite or absurd bounds reject nothing.
//
// Pure functions (TOPO_HD), as topo_surface.h: the kernels call the per-post tests and the window for every post they visit, and
// tests/summits_emul.cpp runs the same code under g++ -- windowed (summit_nearest, summit_snap) and over every post of every tile
// (summits_all, snap_all: the emulation's check of the window and the block test; never on the device).
#pragma once

#include "topo_surface.h"

namespace topo {

constexpr int32_t kSnapFound = 1, kSnapNone = 0, kSnapInvalid = -1;
constexpr uint32_t kSummitOrderTile = 0, kSummitOrderHeight = 1, kSummitOrderIsolation = 2;
constexpr double kSummitMaxRadius = 1.0e6;
constexpr double kSummitPad = 1.0 / 64.0;
constexpr double kSummitHalfPi = 1.5707963267948966;

struct SummitBest {        // the best post so far of a search: the nearest dominator, or the snap target
    double d;
    uint32_t rank, idx;
    float h;
    bool found;
};

struct SummitWindow {      // vertex columns x0 .. x1 and rows y0 .. y1, inclusive; any == false: none
    uint32_t x0, x1, y0, y1;
    bool any;
};

TOPO_HD double summit_lon(const TileDev& t, uint32_t vx) { return ((double)vx - (double)t.raster_x) * (double)t.scale_x + (double)t.model_x; }
TOPO_HD double summit_lat(const TileDev& t, uint32_t vy) { return ((double)vy - (double)t.raster_y) * -(double)t.scale_y + (double)t.model_y; }

// The direction of post (vx, vy) of tile `rank` from the tile's tables; false (and u = 0): the index check failed.
template <class Check>
TOPO_HD bool summit_direction(const LosScene& S, uint32_t rank, uint32_t vx, uint32_t vy, double u[3], Check&& chk) {
    const size_t tab = (size_t)rank * ground_table_doubles(S.tile_w, S.tile_h);
    const size_t lo = tab + 2 * (size_t)vx, la = tab + 2 * ((size_t)S.tile_w + vy);
    const bool ok = rank < S.n_tiles && vx < S.tile_w && vy < S.tile_h && la + 1 < S.trig_doubles;
    u[0] = u[1] = u[2] = 0.0;
    if (!(chk(ok, ((uint64_t)vy << 32) | vx) && ok)) return false;
    const double clo = S.trig[lo], slo = S.trig[lo + 1], cla = S.trig[la], sla = S.trig[la + 1];
    u[0] = cla * clo;
    u[1] = cla * slo;
    u[2] = sla;
    return true;
}

TOPO_HD double summit_chord(const double a[3], const double b[3]) {
    const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return kGroundR0 * sqrt(dx * dx + dy * dy + dz * dz);
}

// (existence is the caller's to test)
TOPO_HD bool summit_dominates(float hq, uint32_t rank_q, uint32_t idx_q, float hp, uint32_t rank_p, uint32_t idx_p) {
    return hq > hp || (hq == hp && (rank_q < rank_p || (rank_q == rank_p && idx_q < idx_p)));
}

TOPO_HD bool summit_nearer(double d, uint32_t rank, uint32_t idx, const SummitBest& b) {
    return !b.found || d < b.d || (d == b.d && (rank < b.rank || (rank == b.rank && idx < b.idx)));
}
TOPO_HD bool snap_better(float h, double d, uint32_t rank, uint32_t idx, const SummitBest& b) {
    return !b.found || h > b.h || (h == b.h && (d < b.d || (d == b.d && (rank < b.rank || (rank == b.rank && idx < b.idx)))));
}
TOPO_HD void summit_merge(SummitBest& b, const SummitBest& o, bool snap) {
    const bool better = o.found && (snap ? snap_better(o.h, o.d, o.rank, o.idx, b) : summit_nearer(o.d, o.rank, o.idx, b));
    b = better ? o : b;
}

// The window of tile t around the centre (lon, lat) degrees for `radius` metres (header comment).
TOPO_HD SummitWindow summit_window(const LosScene& S, const TileDev& t, double lon, double lat, double radius) {
    SummitWindow w{0u, S.tile_w - 1, 0u, S.tile_h - 1, surface_tile_ok(t) && S.tile_w > 0 && S.tile_h > 0};
    if (!w.any) return w;
    const double sx = (double)t.scale_x, sy = (double)t.scale_y;
    const double dlon = los_wrap180(lon - (double)t.model_x);
    const double fx = dlon / sx + (double)t.raster_x;
    const double fy = ((double)t.model_y - lat) / sy + (double)t.raster_y;
    double s = radius / (2.0 * kGroundR0);
    s = s > 1.0 ? 1.0 : s;
    const double theta = 2.0 * asin(s);
    const double rows = theta * kGroundDeg / fabs(sy);
    if (!ground_finite(fx) || !ground_finite(fy) || !ground_finite(rows)) return w;
    uint32_t i0, i1;
    los_cells(fy - rows - kSummitPad, fy + rows + kSummitPad, 0u, S.tile_h, i0, i1);
    if (i0 > i1) {
        w.any = false;
        return w;
    }
    w.y0 = i0;
    w.y1 = i1;
    const double ratio = sin(theta) / cos(lat * kGroundRad);
    if (!(theta < kSummitHalfPi && ratio >= 0.0 && ratio < 0.999999)) return w;      // (every column; false for a NaN too)
    const double span = asin(ratio) * kGroundDeg;
    if (!(fabs(dlon) + span < 180.0)) return w;
    const double cols = span / fabs(sx);
    if (!ground_finite(cols)) return w;
    los_cells(fx - cols - kSummitPad, fx + cols + kSummitPad, 0u, S.tile_w, i0, i1);
    if (i0 > i1) {
        w.any = false;
        return w;
    }
    w.x0 = i0;
    w.x1 = i1;
    return w;
}

// The smaller of two windows of one tile (a shrunken search radius): never larger than either.
TOPO_HD SummitWindow summit_window_cut(const SummitWindow& a, const SummitWindow& b) {
    SummitWindow w{a.x0 > b.x0 ? a.x0 : b.x0, a.x1 < b.x1 ? a.x1 : b.x1, a.y0 > b.y0 ? a.y0 : b.y0, a.y1 < b.y1 ? a.y1 : b.y1, a.any && b.any};
    w.any = w.any && w.x0 <= w.x1 && w.y0 <= w.y1;
    return w;
}

// The block that owns vertex column x (row y likewise with kLosBCY and by_count).
TOPO_HD uint32_t summit_block_of(uint32_t v, uint32_t cells, uint32_t count) {
    const uint32_t b = v / cells;
    return b < count ? b : count - 1;
}
// The vertices block b owns along one axis, cut to [lo, hi]: v0 .. v1 inclusive, v0 > v1 for none.
TOPO_HD void summit_block_span(uint32_t b, uint32_t cells, uint32_t count, uint32_t n_vertices, uint32_t lo, uint32_t hi, uint32_t& v0, uint32_t& v1) {
    v0 = b * cells;
    v1 = b + 1 == count ? n_vertices - 1 : v0 + cells - 1;
    v0 = v0 > lo ? v0 : lo;
    v1 = v1 < hi ? v1 : hi;
}

// True: every post of block blk of t is lower than h (header comment: blocks).
template <class Check>
TOPO_HD bool summit_block_below(const LosScene& S, const TileDev& t, uint32_t blk, float h, Check&& chk) {
    const bool ok = blk < S.bx_count * S.by_count;
    if (!(chk(ok, blk) && ok)) return false;
    const double mn = (double)t.block_minmax[2 * (size_t)blk], mx = (double)t.block_minmax[2 * (size_t)blk + 1];
    return mn <= mx && fabs(mn) < kLosAbsurd && fabs(mx) < kLosAbsurd && mx < (double)h;      // (false for a NaN bound)
}

// Post (vx, vy) of tile `rank` as a dominator of P = (hp, rank_p, idx_p, direction up) within `radius` (strict: d < radius, the
// any-hit test against min_isolation_m; else d <= radius): the nearer of it and `best` stays in `best`.
template <class Check>
TOPO_HD void summit_try_dominator(const LosScene& S, const TileDev& t, uint32_t rank, uint32_t vx, uint32_t vy, float hp, uint32_t rank_p, uint32_t idx_p, const double up[3],
                                  double radius, bool strict, SummitBest& best, Check&& chk) {
    const bool ok = vx < S.tile_w && vy < S.tile_h;
    if (!(chk(ok, ((uint64_t)vy << 32) | vx) && ok)) return;
    const uint32_t idx = vy * S.tile_w + vx;
    const float h = TOPO_GLOBAL_F32(t.heights)[idx];
    if (!surface_height_ok(h) || !summit_dominates(h, rank, idx, hp, rank_p, idx_p)) return;
    double u[3];
    if (!summit_direction(S, rank, vx, vy, u, chk)) return;
    const double d = summit_chord(up, u);
    if (!(strict ? d < radius : d <= radius)) return;      // (false for a NaN)
    if (summit_nearer(d, rank, idx, best)) best = SummitBest{d, rank, idx, h, true};
}

// Post (vx, vy) of tile `rank` as the snap target of the direction uc within `radius`.
template <class Check>
TOPO_HD void summit_try_snap(const LosScene& S, const TileDev& t, uint32_t rank, uint32_t vx, uint32_t vy, const double uc[3], double radius, SummitBest& best, Check&& chk) {
    const bool ok = vx < S.tile_w && vy < S.tile_h;
    if (!(chk(ok, ((uint64_t)vy << 32) | vx) && ok)) return;
    const uint32_t idx = vy * S.tile_w + vx;
    const float h = TOPO_GLOBAL_F32(t.heights)[idx];
    if (!surface_height_ok(h)) return;
    double u[3];
    if (!summit_direction(S, rank, vx, vy, u, chk)) return;
    const double d = summit_chord(uc, u);
    if (!(d <= radius)) return;
    if (snap_better(h, d, rank, idx, best)) best = SummitBest{d, rank, idx, h, true};
}

// An upper bound of the distance between a post of tile t and any of its eight in-tile neighbours: the chord is at most the arc, and
// the arc at most the way along the post's meridian to the neighbour's latitude and along that parallel to it,
// R0 (|scale_y| + cos(lat) |scale_x|) pi / 180 <= R0 (|scale_y| + |scale_x|) pi / 180; a part in a million on top covers the rounding of
// the tables (1e-16) many times over.  A min_isolation beyond it makes EVERY dominating neighbour a nearer one: the prefilter then
// needs no chord at all (at 90 m posts the bound is 185 m).
TOPO_HD double summit_neighbour_reach(const TileDev& t) { return kGroundR0 * kGroundRad * (fabs((double)t.scale_x) + fabs((double)t.scale_y)) * 1.000001; }

// The prefilter of k_summit_candidates: true iff one of the eight in-tile neighbours of post (vx, vy) of tile `rank` dominates it at
// a distance < min_isolation -- then its isolation is < min_isolation, whatever else there is.  Exact for any min_isolation: below the
// post spacing no neighbour is that near, and nothing is dropped.
template <class Check>
TOPO_HD bool summit_neighbour_rejects(const LosScene& S, const TileDev& t, uint32_t rank, uint32_t vx, uint32_t vy, float hp, double min_isolation, Check&& chk) {
    if (!(min_isolation > 0.0)) return false;
    double up[3];
    if (!summit_direction(S, rank, vx, vy, up, chk)) return false;
    SummitBest best{0.0, 0u, 0u, 0.0f, false};
    const uint32_t idx_p = vy * S.tile_w + vx;
    const bool all_near = min_isolation > summit_neighbour_reach(t);      // (false for a NaN)
    for (uint32_t dy = 0; dy < 3; ++dy)
        for (uint32_t dx = 0; dx < 3; ++dx) {
            const uint32_t qx = vx + dx - 1, qy = vy + dy - 1;      // (wraps to a huge value below 0)
            if ((dx == 1 && dy == 1) || qx >= S.tile_w || qy >= S.tile_h) continue;
            if (all_near) {
                const float hq = TOPO_GLOBAL_F32(t.heights)[qy * S.tile_w + qx];
                if (surface_height_ok(hq) && summit_dominates(hq, rank, qy * S.tile_w + qx, hp, rank, idx_p)) return true;
            } else {
                summit_try_dominator(S, t, rank, qx, qy, hp, rank, idx_p, up, min_isolation, true, best, chk);
            }
        }
    return best.found;
}

// The nearest dominator of P = post idx_p of tile rank_p (height hp, which exists) within `radius`, over the windows (header
// comment).  kAny: any dominator at d < radius will do, and the first one found ends the search.
template <bool kAny, class Check>
TOPO_HD void summit_nearest(const LosScene& S, uint32_t rank_p, uint32_t idx_p, float hp, double radius, SummitBest& best, Check&& chk) {
    best = SummitBest{0.0, 0u, 0u, 0.0f, false};
    if (!(chk(rank_p < S.n_tiles && S.tile_w > 0, rank_p) && rank_p < S.n_tiles && S.tile_w > 0)) return;
    const uint32_t px = idx_p % S.tile_w, py = idx_p / S.tile_w;
    double up[3];
    if (!summit_direction(S, rank_p, px, py, up, chk)) return;
    const double lon = summit_lon(S.tiles[rank_p], px), lat = summit_lat(S.tiles[rank_p], py);
    for (uint32_t rank = 0; rank < S.n_tiles; ++rank) {
        const TileDev& t = S.tiles[rank];
        SummitWindow w = summit_window(S, t, lon, lat, best.found ? best.d : radius);
        if (!w.any || S.bx_count == 0 || S.by_count == 0) continue;
        const uint32_t bx0 = summit_block_of(w.x0, kLosBCX, S.bx_count), bx1 = summit_block_of(w.x1, kLosBCX, S.bx_count);
        const uint32_t by0 = summit_block_of(w.y0, kLosBCY, S.by_count), by1 = summit_block_of(w.y1, kLosBCY, S.by_count);
        for (uint32_t by = by0; by <= by1; ++by)
            for (uint32_t bx = bx0; bx <= bx1; ++bx) {
                if (summit_block_below(S, t, by * S.bx_count + bx, hp, chk)) continue;
                uint32_t x0, x1, y0, y1;
                summit_block_span(bx, kLosBCX, S.bx_count, S.tile_w, w.x0, w.x1, x0, x1);
                summit_block_span(by, kLosBCY, S.by_count, S.tile_h, w.y0, w.y1, y0, y1);
                const bool had = best.found;
                const double was = best.d;
                for (uint32_t y = y0; y <= y1 && y < S.tile_h; ++y)
                    for (uint32_t x = x0; x <= x1 && x < S.tile_w; ++x) summit_try_dominator(S, t, rank, x, y, hp, rank_p, idx_p, up, radius, kAny, best, chk);
                if (kAny && best.found) return;
                if (best.found && (!had || best.d < was)) w = summit_window_cut(w, summit_window(S, t, lon, lat, best.d));
                if (!w.any) break;
            }
    }
}

// The same by brute force: every post of every tile.
template <class Check>
TOPO_HD void summits_all(const LosScene& S, uint32_t rank_p, uint32_t idx_p, float hp, double radius, bool strict, SummitBest& best, Check&& chk) {
    best = SummitBest{0.0, 0u, 0u, 0.0f, false};
    double up[3];
    if (!summit_direction(S, rank_p, idx_p % S.tile_w, idx_p / S.tile_w, up, chk)) return;
    for (uint32_t rank = 0; rank < S.n_tiles; ++rank) {
        if (!surface_tile_ok(S.tiles[rank])) continue;
        for (uint32_t y = 0; y < S.tile_h; ++y)
            for (uint32_t x = 0; x < S.tile_w; ++x) summit_try_dominator(S, S.tiles[rank], rank, x, y, hp, rank_p, idx_p, up, radius, strict, best, chk);
    }
}

// The snap target of (lon, lat) degrees within `radius`, over the windows; best.found == false: none in range.
template <class Check>
TOPO_HD void summit_snap(const LosScene& S, double lon, double lat, double radius, SummitBest& best, Check&& chk) {
    best = SummitBest{0.0, 0u, 0u, 0.0f, false};
    double uc[3];
    surface_direction(lon, lat, uc);
    for (uint32_t rank = 0; rank < S.n_tiles; ++rank) {
        const TileDev& t = S.tiles[rank];
        const SummitWindow w = summit_window(S, t, lon, lat, radius);
        if (!w.any || S.bx_count == 0 || S.by_count == 0) continue;
        const uint32_t bx0 = summit_block_of(w.x0, kLosBCX, S.bx_count), bx1 = summit_block_of(w.x1, kLosBCX, S.bx_count);
        const uint32_t by0 = summit_block_of(w.y0, kLosBCY, S.by_count), by1 = summit_block_of(w.y1, kLosBCY, S.by_count);
        for (uint32_t by = by0; by <= by1; ++by)
            for (uint32_t bx = bx0; bx <= bx1; ++bx) {
                if (best.found && summit_block_below(S, t, by * S.bx_count + bx, best.h, chk)) continue;
                uint32_t x0, x1, y0, y1;
                summit_block_span(bx, kLosBCX, S.bx_count, S.tile_w, w.x0, w.x1, x0, x1);
                summit_block_span(by, kLosBCY, S.by_count, S.tile_h, w.y0, w.y1, y0, y1);
                for (uint32_t y = y0; y <= y1 && y < S.tile_h; ++y)
                    for (uint32_t x = x0; x <= x1 && x < S.tile_w; ++x) summit_try_snap(S, t, rank, x, y, uc, radius, best, chk);
            }
    }
}

template <class Check>
TOPO_HD void snap_all(const LosScene& S, double lon, double lat, double radius, SummitBest& best, Check&& chk) {
    best = SummitBest{0.0, 0u, 0u, 0.0f, false};
    double uc[3];
    surface_direction(lon, lat, uc);
    for (uint32_t rank = 0; rank < S.n_tiles; ++rank) {
        if (!surface_tile_ok(S.tiles[rank])) continue;
        for (uint32_t y = 0; y < S.tile_h; ++y)
            for (uint32_t x = 0; x < S.tile_w; ++x) summit_try_snap(S, S.tiles[rank], rank, x, y, uc, radius, best, chk);
    }
}

}  // namespace topo
