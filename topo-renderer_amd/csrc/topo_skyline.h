// topo_skyline.h -- the terrain horizon by azimuth from a point (topo_skyline_*): the rule, the winner and the traversal of k_skyline.
//
// "How high does the terrain stand above the horizontal in each direction from here, and which ridge forms that line?" -- without
// a frame, its rows or its field of view.  The definition is exact: the kernel, the g++ build of this header and its loop over
// every triangle agree bit for bit.
//
// Observer.  A topo_observer, resolved by visibility_observer exactly as for the visibility queries (topo_visibility.h): O, and
// rho = |O|.  The frame at O is that of topo_pixel_angles and the unwrap: up = O / rho, east = z x up = (-up_y, up_x, 0) normalised,
// north = up x east.  An unusable observer, and one whose east does not come out finite and non-zero (on the polar axis, at the
// centre), is kSkyNoObserver for all its azimuths.
//
// Azimuth.  a_k = az0 + k daz (degrees, clockwise from north; one rounded product and one rounded sum, as the grids),
// h = cos a north + sin a east, m = h x up: m points to the observer's right.  The half-plane {O + s h + z up, s > 0} lies in a plane
// through the Earth's centre (it holds O and up = O / rho); the traversal relies on that.
//
// Mesh.  That of the rays (topo_los.h), with the rays' rule of existence, los_cell's: a triangle exists iff its three vertex
// heights are finite (a finite sentinel is geometry).  The surface's narrower rule (topo_surface.h) is NOT used: what a ray from O
// can hit is what can stand on O's horizon.
//
// Crossing.  For each of the three edges of every existing triangle -- edge e joins vertices e and (e + 1) % 3 of triangle_vertices --
// with the endpoints in canonical order, the lower vertex index vy * w + vx first (two triangles that share an edge compute identical
// bits), translated by O first as los_triangle's are (a = A - O, b = B - O): da = m . a, db = m . b; the edge crosses iff
// (da < 0) != (db < 0) -- half-open: a vertex on the plane belongs to the right side; X = a + (da / (da - db)) (b - a), s = h . X,
// z = up . X; the crossing counts iff min_range <= s <= max_range and z / s is a number.  In the (s, z) plane the elevation angle along
// a straight segment is monotone, so the highest point of any triangle's cut is at an edge crossing: the crossings carry the answer.
//
// Winner.  The largest z / s (f64), then the smaller s, then the lower tile rank, then the lower triangle index, then the lower edge:
// a function of the observer, the azimuth and the tile set, not of the traversal.  No crossing: kSkyNone.
//
// Traversal (skyline_cast): tiles and raster blocks by their sphere, blocks by height, the cells of a surviving block by the
// longitude / latitude range of its part of the half-plane.  Why each step keeps every crossing that could win:
//   sphere   a crossing point P = O + X lies on an edge of a triangle of the block, whose vertices lie inside the block's (padded)
//            sphere (c, r); a sphere is convex, so |P - c| <= r.  m, h, up are orthonormal and m . X = 0, so
//            (m . (c - O))^2 + (h . (P - c))^2 + (up . (P - c))^2 <= r^2: a sphere with |m . (c - O)| > r holds no crossing, and with
//            rr^2 = r^2 - (m . (c - O))^2 a crossing's s lies in h . (c - O) -+ rr and its up . P in up . c -+ rr.  A sphere whose s
//            interval misses [min_range, max_range] holds no crossing that counts.  The radius is padded by kSkyPad for the rounding
//            of X (about 1e-9 m).  A tile's sphere is the one around its block centres plus the largest block radius.
//   height   |P| is at most the largest |vertex| of the edge (|.| is convex), at most Rtop = max(|R0 + hmin|, |R0 + hmax|) of the
//            block, and |P|^2 = (rho + z)^2 + s^2, so z / s <= f(s) = (sqrt(Rtop^2 - s^2) - rho) / s.  f'(s) has the sign of
//            rho - Rtop^2 / sqrt(Rtop^2 - s^2): for rho <= Rtop f falls, and its maximum over the block's s interval is at the near
//            end; for rho > Rtop (an observer above the block's shell) f is NOT monotone -- it rises to the tangent point
//            s_t = (Rtop / rho) sqrt(rho^2 - Rtop^2) and falls behind it -- so the maximum is at s_t clamped to the interval.  A
//            block whose bound lies below the best z / s so far holds neither the winner nor a tie (Rtop carries kLosShellPad, a
//            centimetre: 0.01 / s in the bound, against a rounding of z / s of about 1e-9 / s).  Bounds that are not finite, not
//            ordered (a void block) or absurd are not used.
//   cells    the plane passes through the centre, so a point of the half-plane at ground angle psi from O has the direction of
//            O + rho tan(psi) h, whatever its z: the directions of the crossings are those of the horizontal ray from O along h, and
//            los_cell_range applies to it unchanged, with t = rho tan(psi) = rho s / (rho + z) = rho s / (up . P) over the sphere's
//            intervals of s and up . P.  The crossing point lies on an edge of its triangle, so on the border or inside of its cell's
//            spherical quadrilateral; the paddings of topo_los.h (1/64 cell, the parallels' bulge) apply.  An interval that does not
//            come out finite and positive (up . c - rr <= 0: a block at 90 degrees of ground angle) selects the whole block.
//   A pruning comparison that does not come out finite prunes nothing: each is written so that a NaN fails it.
// skyline_all is the same crossing test and order over every triangle of every tile (the emulation's check; never on the device).
//
// Pure functions (TOPO_HD), as topo_los.h: k_skyline (kernels_skyline.h) takes the same steps a wave at a time, and
// tests/skyline_emul.cpp runs this code under g++.
#pragma once

#include "topo_visibility.h"

namespace topo {

constexpr int32_t kSkyNone = 0, kSkyTerrain = 1, kSkyNoObserver = 4;      // (kSkyNoObserver = kVisNoObserver)
constexpr double kSkyMaxRange = 1.0e6;              // metres: the largest max_range a call may ask for
constexpr double kSkyPad = 0.01;                    // metres over a sphere's radius in the plane and range tests
constexpr uint32_t kSkyMaxObservers = kVisMaxObservers;

static_assert(kSkyNoObserver == kVisNoObserver, "an unusable observer has one number");

struct SkyFrame {          // the frame at a resolved observer
    double o[3], up[3], east[3], north[3], rho;
    uint32_t usable;
};

struct SkyDir {            // an azimuth in that frame
    double h[3], m[3];
};

struct SkyBest {
    double ratio, s, z;    // z / s, and its parts
    uint32_t rank, tri, edge;
    bool hit;
};

struct SkyPoint {          // what a winner reports of its crossing point P = O + X
    double elevation_deg, range_m, lon_deg, lat_deg, height_m;
};

TOPO_HD double sky_dot(const double a[3], const double b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// The frame at a resolved observer (header comment: observer).
TOPO_HD void skyline_frame(const VisEye& eye, SkyFrame& F) {
    F = SkyFrame{{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, 0.0, 0u};
    if (!eye.usable) return;
    const double rho = sqrt(sky_dot(eye.p, eye.p));
    const double up[3] = {eye.p[0] / rho, eye.p[1] / rho, eye.p[2] / rho};
    const double n = sqrt(up[1] * up[1] + up[0] * up[0]);
    const double east[3] = {-up[1] / n, up[0] / n, 0.0};
    if (!(n > 0.0) || !ground_finite(east[0]) || !ground_finite(east[1]) || !ground_finite(up[2])) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        F.o[k] = eye.p[k];
        F.up[k] = up[k];
        F.east[k] = east[k];
    }
    F.north[0] = up[1] * east[2] - up[2] * east[1];
    F.north[1] = up[2] * east[0] - up[0] * east[2];
    F.north[2] = up[0] * east[1] - up[1] * east[0];
    F.rho = rho;
    F.usable = 1u;
}

TOPO_HD double skyline_azimuth(double az0_deg, double daz_deg, uint32_t k) { return az0_deg + (double)k * daz_deg; }

TOPO_HD void skyline_direction(const SkyFrame& F, double az_deg, SkyDir& D) {
    const double a = az_deg * kGroundRad;
    const double ca = cos(a), sa = sin(a);
#pragma unroll
    for (int k = 0; k < 3; ++k) D.h[k] = ca * F.north[k] + sa * F.east[k];
    D.m[0] = D.h[1] * F.up[2] - D.h[2] * F.up[1];
    D.m[1] = D.h[2] * F.up[0] - D.h[0] * F.up[2];
    D.m[2] = D.h[0] * F.up[1] - D.h[1] * F.up[0];
}

TOPO_HD bool sky_better(double ratio, double s, uint32_t rank, uint32_t tri, uint32_t edge, const SkyBest& b) {
    if (!b.hit || ratio > b.ratio) return true;
    if (!(ratio == b.ratio)) return false;
    if (s != b.s) return s < b.s;
    if (rank != b.rank) return rank < b.rank;
    if (tri != b.tri) return tri < b.tri;
    return edge < b.edge;
}

// The crossing of the edge a -> b (canonical order, translated by O; da = m . a, db = m . b of different sign classes).
TOPO_HD void sky_edge_point(const double a[3], const double b[3], double da, double db, double X[3]) {
    const double f = da / (da - db);
#pragma unroll
    for (int k = 0; k < 3; ++k) X[k] = a[k] + f * (b[k] - a[k]);
}

// The place of corner `at` = 2 a + b of a cell (vertex (i + a, j + b)) in the order of the vertex indices vy * w + vx: b first.
TOPO_HD uint32_t sky_corner_key(uint32_t at) { return ((at & 1u) << 1) | (at >> 1); }

// One cell (i, j) of tile `rank`: the crossings of the edges of its two triangles, the best of them and `best` in `best`.
// chk(ok, value): the caller's index check (the bounds-checking build).
template <class Check>
TOPO_HD void sky_cell(const LosScene& S, const TileDev& t, uint32_t rank, uint32_t i, uint32_t j, const SkyFrame& F, const SkyDir& D, double min_range,
                      double max_range, SkyBest& best, Check&& chk) {
    const uint32_t hm1 = S.tile_h - 1;
    const size_t tab = (size_t)rank * ground_table_doubles(S.tile_w, S.tile_h);
    const size_t lo = tab + 2 * (size_t)i, la = tab + 2 * ((size_t)S.tile_w + j);
    if (!(chk(i + 1 < S.tile_w && j + 1 < S.tile_h && la + 3 < S.trig_doubles, ((uint64_t)j << 32) | i) && i + 1 < S.tile_w && j + 1 < S.tile_h)) return;
    double c[4][3], dm[4];      // corner (a, b) = vertex (i + a, j + b) at [2 a + b]; dm = m . corner
    bool ok[4];
    const auto hts = TOPO_GLOBAL_F32(t.heights);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t a = (uint32_t)k >> 1, b = (uint32_t)k & 1u;
        const float h = hts[(size_t)(j + b) * S.tile_w + (i + a)];
        ok[k] = ground_finite((double)h);
        ground_vertex_from(h, S.trig[lo + 2 * a], S.trig[lo + 2 * a + 1], S.trig[la + 2 * b], S.trig[la + 2 * b + 1], c[k]);
#pragma unroll
        for (int m = 0; m < 3; ++m) c[k][m] -= F.o[m];
        dm[k] = sky_dot(D.m, c[k]);
    }
    // (all four corners on one side: no edge of the cell crosses)
    const bool r0 = dm[0] < 0.0;
    if ((dm[1] < 0.0) == r0 && (dm[2] < 0.0) == r0 && (dm[3] < 0.0) == r0) return;
    const uint32_t cell = i * hm1 + j;
#pragma unroll
    for (uint32_t k = 0; k < 2; ++k) {
        const uint32_t tri = 2 * cell + k;
        uint32_t vx[3], vy[3], at[3];
        triangle_vertices(tri, hm1, vx, vy);
        bool exists = true;
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            at[m] = (2 * (vx[m] - i) + (vy[m] - j)) & 3u;
            exists = exists && ok[at[m]];
        }
        if (!exists) continue;
#pragma unroll
        for (uint32_t e = 0; e < 3; ++e) {
            uint32_t p = at[e], q = at[e == 2 ? 0 : e + 1];
            if (sky_corner_key(p) > sky_corner_key(q)) {
                const uint32_t x = p;
                p = q;
                q = x;
            }
            const double da = dm[p], db = dm[q];
            if ((da < 0.0) == (db < 0.0)) continue;
            double X[3];
            sky_edge_point(c[p], c[q], da, db, X);
            const double s = sky_dot(D.h, X), z = sky_dot(F.up, X);
            const double ratio = z / s;
            if (!(s >= min_range && s <= max_range && ratio == ratio)) continue;
            const bool better = sky_better(ratio, s, rank, tri, e, best);
            best.ratio = better ? ratio : best.ratio;
            best.s = better ? s : best.s;
            best.z = better ? z : best.z;
            best.rank = better ? rank : best.rank;
            best.tri = better ? tri : best.tri;
            best.edge = better ? e : best.edge;
            best.hit = true;
        }
    }
}

// The s interval [s_lo, s_hi] cut down to that of the sphere (c, r) in the half-plane, and the interval [q_lo, q_hi] of up . P over
// it (header comment: sphere); false: the sphere holds no crossing that counts.  A test that does not come out finite cuts nothing.
TOPO_HD bool sky_clip_sphere(const SkyFrame& F, const SkyDir& D, const double c[3], double r, double& s_lo, double& s_hi, double& q_lo, double& q_hi) {
    const double x[3] = {c[0] - F.o[0], c[1] - F.o[1], c[2] - F.o[2]};
    const double w = sky_dot(D.m, x), a = sky_dot(D.h, x), q = sky_dot(F.up, x) + F.rho, rp = r + kSkyPad;
    q_lo = q_hi = __builtin_nan("");
    if (fabs(w) > rp) return false;
    const double rr = sqrt(rp * rp - w * w);
    if (a + rr < s_lo || a - rr > s_hi) return false;
    if (a - rr > s_lo) s_lo = a - rr;
    if (a + rr < s_hi) s_hi = a + rr;
    q_lo = q - rr;
    q_hi = q + rr;
    return true;
}

// The largest z / s a point of the half-plane with |O + X| <= top and s in [s_lo, s_hi] can have (header comment: height).
TOPO_HD double sky_bound(double rho, double top, double s_lo, double s_hi) {
    double s = s_lo;
    if (rho > top) {
        const double st = (top / rho) * sqrt((rho - top) * (rho + top));
        s = st < s_lo ? s_lo : (st > s_hi ? s_hi : st);
    }
    return (sqrt((top - s) * (top + s)) - rho) / s;
}

// A block of tile t against the half-plane: false when it holds no crossing that counts; otherwise `bound`, the largest z / s it can
// hold (+inf: unknown), and [ta, tb], its part of the horizontal ray from O along h (NaN: the whole block).
TOPO_HD bool sky_block(const SkyFrame& F, const SkyDir& D, const TileDev& t, uint32_t blk, double min_range, double max_range, double& bound, double& ta, double& tb) {
    const double* const bs = t.block_bounds + 4 * (size_t)blk;
    const double hmin = (double)t.block_minmax[2 * (size_t)blk], hmax = (double)t.block_minmax[2 * (size_t)blk + 1];
    double s_lo = min_range, s_hi = max_range, q_lo = __builtin_nan(""), q_hi = q_lo;
    bound = __builtin_inf();
    ta = tb = __builtin_nan("");
    if (bs[3] < kLosAbsurd && !sky_clip_sphere(F, D, bs, bs[3], s_lo, s_hi, q_lo, q_hi)) return false;
    if (hmin <= hmax) {
        const double r0 = fabs(kGroundR0 + hmin), r1 = fabs(kGroundR0 + hmax), top = (r0 > r1 ? r0 : r1) + kLosShellPad;
        const double f = sky_bound(F.rho, top, s_lo, s_hi);
        if (top < kLosAbsurd && f == f) bound = f;
    }
    if (q_lo > 0.0) {
        ta = F.rho * s_lo / q_hi;
        tb = F.rho * s_hi / q_lo;
    }
    return true;
}

// The cells of block (bx, by) of tile t that [ta, tb] of the horizontal ray selects (header comment: cells): ix0 .. ix1, iy0 .. iy1
// inclusive; false: none.
TOPO_HD bool sky_block_cells(const LosScene& S, const TileDev& t, const SkyFrame& F, const SkyDir& D, double oo, double od, double dd, double pad_y, uint32_t bx,
                             uint32_t by, double ta, double tb, uint32_t& ix0, uint32_t& ix1, uint32_t& iy0, uint32_t& iy1) {
    const uint32_t cells_x = S.tile_w - 1, cells_y = S.tile_h - 1;
    const uint32_t cx0 = bx * kLosBCX, cy0 = by * kLosBCY;
    const uint32_t cx1 = cx0 + kLosBCX < cells_x ? cx0 + kLosBCX : cells_x, cy1 = cy0 + kLosBCY < cells_y ? cy0 + kLosBCY : cells_y;
    ix0 = cx0; ix1 = cx1 - 1; iy0 = cy0; iy1 = cy1 - 1;
    if (ground_finite(ta) && ground_finite(tb)) los_cell_range(t, F.o, D.h, oo, od, dd, ta, tb, pad_y, cx0, cx1, cy0, cy1, ix0, ix1, iy0, iy1);
    return !(ix0 > ix1 || iy0 > iy1 || ix1 >= cx1 || iy1 >= cy1);
}

// A tile's sphere against the half-plane; false: the tile holds no crossing that counts.
TOPO_HD bool sky_tile(const LosScene& S, const SkyFrame& F, const SkyDir& D, uint32_t rank, double min_range, double max_range) {
    const double* const ts = S.spheres + (size_t)kLosSphereDoubles * rank;
    double s_lo = min_range, s_hi = max_range, q_lo, q_hi;
    return !(ts[3] >= 0.0 && ts[4] >= 0.0) || sky_clip_sphere(F, D, ts, ts[3] + ts[4], s_lo, s_hi, q_lo, q_hi);
}

TOPO_HD double sky_pad_y(const TileDev& t) {      // los_cast's
    const double sx = (double)t.scale_x, sy = (double)t.scale_y;
    return 1.0 / 64.0 + fabs(0.25 * kGroundRad * sx * sx / sy);
}

// The skyline of one azimuth: the winner (header comment) in `best`.
template <class Check>
TOPO_HD void skyline_cast(const LosScene& S, const SkyFrame& F, const SkyDir& D, double min_range, double max_range, SkyBest& best, Check&& chk) {
    best = SkyBest{0.0, 0.0, 0.0, 0u, 0u, 0u, false};
    const double oo = sky_dot(F.o, F.o), od = sky_dot(F.o, D.h), dd = sky_dot(D.h, D.h);
    for (uint32_t rank = 0; rank < S.n_tiles; ++rank) {
        if (!sky_tile(S, F, D, rank, min_range, max_range)) continue;
        const TileDev& t = S.tiles[rank];
        const double pad_y = sky_pad_y(t);
        for (uint32_t by = 0; by < S.by_count; ++by)
            for (uint32_t bx = 0; bx < S.bx_count; ++bx) {
                double bound, ta, tb;
                if (!sky_block(F, D, t, by * S.bx_count + bx, min_range, max_range, bound, ta, tb)) continue;
                if (best.hit && bound < best.ratio) continue;
                uint32_t ix0, ix1, iy0, iy1;
                if (!sky_block_cells(S, t, F, D, oo, od, dd, pad_y, bx, by, ta, tb, ix0, ix1, iy0, iy1)) continue;
                for (uint32_t i = ix0; i <= ix1; ++i)
                    for (uint32_t j = iy0; j <= iy1; ++j) sky_cell(S, t, rank, i, j, F, D, min_range, max_range, best, chk);
            }
    }
}

// The same answer by brute force: every triangle of every tile (the emulation's check of the traversal; never on the device).
template <class Check>
TOPO_HD void skyline_all(const LosScene& S, const SkyFrame& F, const SkyDir& D, double min_range, double max_range, SkyBest& best, Check&& chk) {
    best = SkyBest{0.0, 0.0, 0.0, 0u, 0u, 0u, false};
    for (uint32_t rank = 0; rank < S.n_tiles; ++rank)
        for (uint32_t i = 0; i + 1 < S.tile_w; ++i)
            for (uint32_t j = 0; j + 1 < S.tile_h; ++j) sky_cell(S, S.tiles[rank], rank, i, j, F, D, min_range, max_range, best, chk);
}

// What a winner reports: its crossing point computed again from (rank, tri, edge) -- the same operations on the same numbers as in
// sky_cell, so the same bits -- then elevation = atan2(z, s), range = |X|, and longitude, latitude and height over the sphere of
// P = O + X as los_hit_point has them.  false: the index check failed.
template <class Check>
TOPO_HD bool skyline_point(const LosScene& S, const SkyFrame& F, const SkyDir& D, const SkyBest& b, SkyPoint& out, Check&& chk) {
    out = SkyPoint{0.0, 0.0, 0.0, 0.0, 0.0};
    uint32_t vx[3], vy[3];
    triangle_vertices(b.tri, S.tile_h - 1, vx, vy);
    const size_t tab = (size_t)b.rank * ground_table_doubles(S.tile_w, S.tile_h);
    bool ok = b.rank < S.n_tiles && b.edge < 3u;
#pragma unroll
    for (int m = 0; m < 3; ++m) ok = ok && vx[m] < S.tile_w && vy[m] < S.tile_h && tab + 2 * ((size_t)S.tile_w + vy[m]) + 1 < S.trig_doubles;
    if (!(chk(ok, ((uint64_t)b.rank << 32) | b.tri) && ok)) return false;
    uint32_t p = b.edge, q = b.edge == 2 ? 0 : b.edge + 1;
    if ((size_t)vy[p] * S.tile_w + vx[p] > (size_t)vy[q] * S.tile_w + vx[q]) {
        const uint32_t x = p;
        p = q;
        q = x;
    }
    const auto hts = TOPO_GLOBAL_F32(S.tiles[b.rank].heights);
    double e[2][3], dm[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const uint32_t v = k == 0 ? p : q;
        const size_t lo = tab + 2 * (size_t)vx[v], la = tab + 2 * ((size_t)S.tile_w + vy[v]);
        ground_vertex_from(hts[(size_t)vy[v] * S.tile_w + vx[v]], S.trig[lo], S.trig[lo + 1], S.trig[la], S.trig[la + 1], e[k]);
#pragma unroll
        for (int m = 0; m < 3; ++m) e[k][m] -= F.o[m];
        dm[k] = sky_dot(D.m, e[k]);
    }
    double X[3];
    sky_edge_point(e[0], e[1], dm[0], dm[1], X);
    const double P[3] = {F.o[0] + X[0], F.o[1] + X[1], F.o[2] + X[2]};
    const double norm = sqrt(sky_dot(P, P));
    out.elevation_deg = atan2(b.z, b.s) * kGroundDeg;
    out.range_m = sqrt(sky_dot(X, X));
    out.lon_deg = atan2(P[1], P[0]) * kGroundDeg;
    out.lat_deg = asin(P[2] / norm) * kGroundDeg;
    out.height_m = norm - kGroundR0;
    return true;
}

}  // namespace topo
