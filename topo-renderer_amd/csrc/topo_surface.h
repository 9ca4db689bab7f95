// topo_surface.h -- the drawn terrain under a longitude and latitude (topo_surface_*, topo_profile_*): the rule, the lookup of
// k_surface / k_surface_grid / k_profile, and the reduction of a profile.
//
// The mesh is that of the rays (topo_los.h): vertex (vx, vy) of a tile at ground_vertex_from with the tile's f64 (cos, sin) tables,
// triangles and their vertex order from triangle_vertices.  A triangle EXISTS for these queries iff each of its three vertex heights
// is finite, < 1e9 and > -R0: only then does every vertex lie over its own longitude and latitude.  Finite sentinels (-32768) are
// geometry, as in the frame.
//
// The line.  For a direction u (unit, f64) the line is o = R0 u, d = u: t IS the height over the sphere.  The triangle test is
// los_triangle's arithmetic on vertices translated by o, with TOLERANT edges: hit iff u >= -e, v >= -e, u + v <= 1 + e with e = 2^-30,
// t finite and -R0 < t < 1e9.  A ray may fall into the crack two independently rounded triangles leave along their common edge and
// report what lies behind; a height has nothing behind it, so here the edges overlap by e instead (1e-9 of a cell: 0.1 micrometres
// at 90 m posts), which makes interior edges and vertices watertight and lets a query at an exact DEM post on the mesh border hit.
// The winner, among all triangles of all resident tiles, is the LARGEST t (the surface seen from above); on equal t the lower tile
// rank (draw order), then the lower triangle index: a function of the point and the tile set, not of the lookup.
//
// The lookup (surface_lookup).  Per tile fx = wrap180(lon - model_x) / scale_x + raster_x, fy = (model_y - lat) / scale_y + raster_y
// with lon = atan2(y, x), lat = asin(z / |u|); the candidate cells are floor(fx -+ 1/64) x floor(fy -+ pad_y), pad_y as los_cast has
// it, clamped to the tile; a tile none of whose cells is a candidate is skipped.  Why this set holds every hit -- the "cells"
// argument of topo_los.h for a radial line: every vertex of an existing triangle has a positive radius, so the line through the
// centre along u meets the triangle iff u lies in the spherical triangle of its vertices' directions, and that lies in the spherical
// quadrilateral of its cell.  The cell's meridian edges lie in planes through the polar axis (one longitude exactly), so the
// longitude of u lies between the cell's columns: fx in [i, i + 1].  The great-circle arc between two vertices of one latitude bulges
// towards the pole by at most dlon / 16 of a row, so fy in [j - bulge, j + 1 + bulge].  The tolerance e moves a hit at most e of a
// cell past an edge and the f64 rounding of lon, lat, fx, fy about 1e-11 of one; 1/64 (and 1/64 plus four times the bulge) covers
// both, so the cell of every hit has floor(fx - 1/64) <= i <= floor(fx + 1/64), and likewise j: at most 2 x 2 cells unless the bulge
// term is large (coarse test tiles).  A tile whose pixel scale is zero or not finite in x or y HAS NO SURFACE (surface_tile_ok: its
// columns or rows fall onto one meridian or parallel, or nowhere; it is part of the rule, for surface_all too), and a tile whose
// coordinates still do not come out finite (a NaN model point) is skipped: none of its vertices is finite, and no comparison with a
// NaN holds in the test.  So a lane never walks a whole tile.  A direction whose longitude or latitude is not finite has no terrain
// under it for the same reason.
// wrap180 takes the columns of a tile to lie within 180 degrees of its model_x.  Every resident tile is examined: tiles may overlap
// or leave gaps, a tile's transform is the caller's.  surface_all is the same test and order over every triangle, for the emulation.
//
// Slope and aspect of the winner: n = (v1 - v0) x (v2 - v0), flipped if n . u < 0; slope = the angle between n and u (acos(n^ . u),
// evaluated as atan2(|n x u|, n . u), which keeps its digits on flat ground); aspect = the azimuth, clockwise from north in
// [0, 360), of the horizontal part of n^ -- the downslope direction -- in the east / north / up frame of topo_sun_direction at the
// point (east = (-y, x, 0) / |(x, y)|, (0, 1, 0) on the polar axis; north = u x east), 0 when the horizontal part vanishes.
//
// Profiles.  Sample k of m of a segment (a topo_ray with finite bounds) is at t_k = t_min + (t_max - t_min) (k / (m - 1)),
// p = o + t_k d, every step rounded; the surface is looked up under p / |p| directly; line = |p| - R0.  Terrain and line are rounded
// once to f32 (a quiet NaN terrain where there is none), and the clearance of a sample is the f32 difference line - terrain of the
// values as stored, so that a summary can be recomputed from the samples bit for bit.  The summary of a segment is the smallest
// clearance over the samples that have terrain; on equal values the lowest sample index.
//
// Pure functions (TOPO_HD), as topo_los.h: the kernels (kernels_surface.h) call them for every point, and tests/surface_emul.cpp runs
// the same code under g++.
#pragma once

#include "topo_los.h"

namespace topo {

constexpr int32_t kSurfaceTerrain = 1, kSurfaceNone = 0, kSurfaceInvalid = -1;
constexpr double kSurfaceEdge = 9.313225746154785e-10;      // 2^-30
constexpr double kSurfacePadX = 1.0 / 64.0;
constexpr uint32_t kProfileNoSample = 0xFFFFFFFFu;
constexpr uint32_t kProfileMinSamples = 2, kProfileMaxSamples = 65536;

struct SurfaceHit {
    double t, u, v;        // t: the height; u, v: weights of the triangle's second and third vertex
    uint32_t rank, tri;
    bool hit;
};

struct ProfileBest {       // a partial reduction of a segment's samples
    float clearance;
    uint32_t sample, n_terrain;      // sample == kProfileNoSample: none with terrain yet
};

TOPO_HD bool surface_point_valid(double lon_deg, double lat_deg) { return ground_finite(lon_deg) && fabs(lat_deg) <= 90.0; }      // (false for a NaN latitude)
TOPO_HD bool surface_segment_valid(const LosRay& r) { return los_ray_valid(r) && ground_finite(r.tmin) && ground_finite(r.tmax); }
TOPO_HD bool surface_height_ok(float h) { return (double)h < kLosAbsurd && (double)h > -kGroundR0; }      // (false for NaN; -inf and +inf fail a bound)

TOPO_HD bool surface_tile_ok(const TileDev& t) {      // a pixel scale that is finite and not zero, both ways
    const double sx = (double)t.scale_x, sy = (double)t.scale_y;
    return ground_finite(sx) && ground_finite(sy) && sx != 0.0 && sy != 0.0;
}

TOPO_HD void surface_direction(double lon_deg, double lat_deg, double u[3]) {
    const double lo = lon_deg * kGroundRad, la = lat_deg * kGroundRad;
    const double cla = cos(la);
    u[0] = cla * cos(lo);
    u[1] = cla * sin(lo);
    u[2] = sin(la);
}

TOPO_HD bool surface_better(double t, uint32_t rank, uint32_t tri, const SurfaceHit& b) {
    return !b.hit || t > b.t || (t == b.t && (rank < b.rank || (rank == b.rank && tri < b.tri)));
}

// One cell (i, j) of tile `rank` against the line through o = R0 u along u: the better of its two triangles and `best` stays in `best`.
// chk(ok, value): the caller's index check (the bounds-checking build).
template <class Check>
TOPO_HD void surface_cell(const LosScene& S, const TileDev& t, uint32_t rank, uint32_t i, uint32_t j, const double u[3], const double o[3], SurfaceHit& best,
                          Check&& chk) {
    const uint32_t hm1 = S.tile_h - 1;
    const size_t tab = (size_t)rank * ground_table_doubles(S.tile_w, S.tile_h);
    const size_t lo = tab + 2 * (size_t)i, la = tab + 2 * ((size_t)S.tile_w + j);
    if (!(chk(i + 1 < S.tile_w && j + 1 < S.tile_h && la + 3 < S.trig_doubles, ((uint64_t)j << 32) | i) && i + 1 < S.tile_w && j + 1 < S.tile_h)) return;
    double c[4][3];      // corner (a, b) = vertex (i + a, j + b) at [2 a + b]
    bool ok[4];
    const auto hts = TOPO_GLOBAL_F32(t.heights);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t a = (uint32_t)k >> 1, b = (uint32_t)k & 1u;
        const float h = hts[(size_t)(j + b) * S.tile_w + (i + a)];
        ok[k] = surface_height_ok(h);
        ground_vertex_from(h, S.trig[lo + 2 * a], S.trig[lo + 2 * a + 1], S.trig[la + 2 * b], S.trig[la + 2 * b + 1], c[k]);
#pragma unroll
        for (int m = 0; m < 3; ++m) c[k][m] -= o[m];
    }
    const uint32_t cell = i * hm1 + j;
#pragma unroll
    for (uint32_t k = 0; k < 2; ++k) {
        const uint32_t tri = 2 * cell + k;
        uint32_t vx[3], vy[3];
        triangle_vertices(tri, hm1, vx, vy);
        double q[3][3];
        bool exists = true;
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            const uint32_t at = 2 * (vx[m] - i) + (vy[m] - j);
            exists = exists && ok[at & 3u];
#pragma unroll
            for (int n = 0; n < 3; ++n) q[m][n] = c[at & 3u][n];
        }
        double tt, bu, bv;
        (void)los_triangle(q, u, 0.0, 0.0, tt, bu, bv);      // (its arithmetic; the edges and the interval are decided here)
        const bool hit = exists && bu >= -kSurfaceEdge && bv >= -kSurfaceEdge && bu + bv <= 1.0 + kSurfaceEdge && ground_finite(tt) && tt > -kGroundR0 && tt < kLosAbsurd;
        const bool better = hit && surface_better(tt, rank, tri, best);
        best.t = better ? tt : best.t;
        best.u = better ? bu : best.u;
        best.v = better ? bv : best.v;
        best.rank = better ? rank : best.rank;
        best.tri = better ? tri : best.tri;
        best.hit = best.hit || hit;
    }
}

// The terrain under the direction u (header comment: the lookup).
template <class Check>
TOPO_HD void surface_lookup(const LosScene& S, const double u[3], SurfaceHit& best, Check&& chk) {
    best = SurfaceHit{0.0, 0.0, 0.0, 0u, 0u, false};
    const double norm = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
    double sl = u[2] / norm;
    sl = sl > 1.0 ? 1.0 : (sl < -1.0 ? -1.0 : sl);      // (a unit vector on the axis may come out an ulp long)
    const double lon = atan2(u[1], u[0]) * kGroundDeg, lat = asin(sl) * kGroundDeg;
    if (!ground_finite(lon) || !ground_finite(lat)) return;
    const double o[3] = {kGroundR0 * u[0], kGroundR0 * u[1], kGroundR0 * u[2]};
    const uint32_t cells_x = S.tile_w - 1, cells_y = S.tile_h - 1;
    for (uint32_t rank = 0; rank < S.n_tiles; ++rank) {
        const TileDev& t = S.tiles[rank];
        const double sx = (double)t.scale_x, sy = (double)t.scale_y;
        const double pad_y = 1.0 / 64.0 + fabs(0.25 * kGroundRad * sx * sx / sy);
        const double fx = los_wrap180(lon - (double)t.model_x) / sx + (double)t.raster_x;
        const double fy = ((double)t.model_y - lat) / sy + (double)t.raster_y;
        if (!surface_tile_ok(t)) continue;
        // (a NaN model point: no vertex of the tile is finite, and no test against one holds)
        if (!ground_finite(fx) || !ground_finite(fy) || !ground_finite(pad_y)) continue;
        uint32_t ix0, ix1, iy0, iy1;
        los_cells(fx - kSurfacePadX, fx + kSurfacePadX, 0u, cells_x, ix0, ix1);
        los_cells(fy - pad_y, fy + pad_y, 0u, cells_y, iy0, iy1);
        for (uint32_t i = ix0; i <= ix1 && i < cells_x; ++i)
            for (uint32_t j = iy0; j <= iy1 && j < cells_y; ++j) surface_cell(S, t, rank, i, j, u, o, best, chk);
    }
}

// The same answer by brute force: every triangle of every tile (the emulation's check of the candidate set; never on the device).
template <class Check>
TOPO_HD void surface_all(const LosScene& S, const double u[3], SurfaceHit& best, Check&& chk) {
    best = SurfaceHit{0.0, 0.0, 0.0, 0u, 0u, false};
    const double o[3] = {kGroundR0 * u[0], kGroundR0 * u[1], kGroundR0 * u[2]};
    for (uint32_t rank = 0; rank < S.n_tiles; ++rank) {
        if (!surface_tile_ok(S.tiles[rank])) continue;
        for (uint32_t i = 0; i + 1 < S.tile_w; ++i)
            for (uint32_t j = 0; j + 1 < S.tile_h; ++j) surface_cell(S, S.tiles[rank], rank, i, j, u, o, best, chk);
    }
}

// Slope and aspect (degrees) of triangle `tri` of tile `rank` seen from the direction u (header comment).
template <class Check>
TOPO_HD void surface_slope_aspect(const LosScene& S, uint32_t rank, uint32_t tri, const double u[3], double& slope_deg, double& aspect_deg, Check&& chk) {
    slope_deg = 0.0;
    aspect_deg = 0.0;
    uint32_t vx[3], vy[3];
    triangle_vertices(tri, S.tile_h - 1, vx, vy);
    const size_t tab = (size_t)rank * ground_table_doubles(S.tile_w, S.tile_h);
    bool ok = rank < S.n_tiles;
#pragma unroll
    for (int m = 0; m < 3; ++m) ok = ok && vx[m] < S.tile_w && vy[m] < S.tile_h && tab + 2 * ((size_t)S.tile_w + vy[m]) + 1 < S.trig_doubles;
    if (!(chk(ok, ((uint64_t)rank << 32) | tri) && ok)) return;
    const auto hts = TOPO_GLOBAL_F32(S.tiles[rank].heights);
    double p[3][3];
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        const size_t lo = tab + 2 * (size_t)vx[m], la = tab + 2 * ((size_t)S.tile_w + vy[m]);
        ground_vertex_from(hts[(size_t)vy[m] * S.tile_w + vx[m]], S.trig[lo], S.trig[lo + 1], S.trig[la], S.trig[la + 1], p[m]);
    }
    const double e1[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
    const double e2[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
    double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    double nu = n[0] * u[0] + n[1] * u[1] + n[2] * u[2];
    if (nu < 0.0) {
        n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2];
        nu = -nu;
    }
    const double cr[3] = {n[1] * u[2] - n[2] * u[1], n[2] * u[0] - n[0] * u[2], n[0] * u[1] - n[1] * u[0]};
    slope_deg = atan2(sqrt(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2]), nu) * kGroundDeg;
    const double hxy = sqrt(u[0] * u[0] + u[1] * u[1]);
    double east[3] = {0.0, 1.0, 0.0};
    if (hxy > 0.0) {
        east[0] = -u[1] / hxy;
        east[1] = u[0] / hxy;
    }
    const double north[3] = {u[1] * east[2] - u[2] * east[1], u[2] * east[0] - u[0] * east[2], u[0] * east[1] - u[1] * east[0]};
    const double ne = n[0] * east[0] + n[1] * east[1] + n[2] * east[2], nn = n[0] * north[0] + n[1] * north[1] + n[2] * north[2];
    double az = (ne == 0.0 && nn == 0.0) ? 0.0 : atan2(ne, nn) * kGroundDeg;
    if (az < 0.0) az += 360.0;
    aspect_deg = az < 360.0 ? az : 0.0;      // (false for NaN)
    if (!ground_finite(slope_deg)) slope_deg = 0.0;
}

// The aspect as the record's f32: a value that rounds up to 360 is 0.
TOPO_HD float surface_aspect_f32(double aspect_deg) {
    const float a = (float)aspect_deg;
    return a < 360.0f ? a : 0.0f;
}

// Sample k of m of segment r: where it lies (p), its direction from the centre (u = p / |p|) and its height over the sphere (line).
TOPO_HD void profile_sample_point(const LosRay& r, uint32_t k, uint32_t m, double u[3], double& line) {
    const double f = (double)k / (double)(m - 1);
    const double span = r.tmax - r.tmin;
    const double tk = r.tmin + span * f;
    const double p[3] = {r.o[0] + tk * r.d[0], r.o[1] + tk * r.d[1], r.o[2] + tk * r.d[2]};
    const double norm = sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
    u[0] = p[0] / norm;
    u[1] = p[1] / norm;
    u[2] = p[2] / norm;
    line = norm - kGroundR0;
}

// Sample k of m of segment r as it is stored: the terrain under it (a quiet NaN where there is none) and the line's height.
template <class Check>
TOPO_HD void profile_sample(const LosScene& S, const LosRay& r, uint32_t k, uint32_t m, float& terrain, float& line, Check&& chk) {
    double u[3], l;
    profile_sample_point(r, k, m, u, l);
    SurfaceHit h;
    surface_lookup(S, u, h, chk);
    terrain = h.hit ? (float)h.t : __builtin_nanf("");
    line = (float)l;
}

// A sample into a partial reduction; samples arrive in ascending order within one partial.
TOPO_HD void profile_take(ProfileBest& b, uint32_t k, float terrain, float line) {
    if (terrain != terrain) return;
    const float c = line - terrain;
    ++b.n_terrain;
    const bool better = b.sample == kProfileNoSample || c < b.clearance;
    b.clearance = better ? c : b.clearance;
    b.sample = better ? k : b.sample;
}

// Two partials into one: the smaller clearance, on equal values the lower sample.
TOPO_HD void profile_merge(ProfileBest& b, const ProfileBest& other) {
    const bool better = other.sample != kProfileNoSample && (b.sample == kProfileNoSample || other.clearance < b.clearance || (other.clearance == b.clearance && other.sample < b.sample));
    b.clearance = better ? other.clearance : b.clearance;
    b.sample = better ? other.sample : b.sample;
    b.n_terrain += other.n_terrain;
}

}  // namespace topo
