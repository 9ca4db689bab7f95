// topo_refraction.h -- what an observer sees along sight lines bent by atmospheric refraction (topo_visibility_refracted_*): the
// rule, and the steps k_visibility_refracted_grid / k_visibility_refracted_list take for every target.
//
// The rule.  Surveyors, radio planners and viewshed tools bend the sight line with one coefficient k (0.13 is the standard
// atmosphere; GDAL's viewshed calls it -cc 0.857 = 1 - k): seen from O, terrain at distance s appears raised by k s^2 / (2 R0).
// Here the refracted query of observer O with coefficient k IS the plain visibility query (topo_visibility.h) on the mesh LIFTED
// for O:
//   lift     every vertex v of the rays' mesh keeps its direction and gains radius: v' = v + (c |v - O|^2 / |v|) v, c = k / (2 R0),
//            |v - O| the f64 chord from the UNLIFTED vertex to O.  The radius grows by c |v - O|^2 exactly: it does not depend on |v|.
//            With u = v / |v| this is v' = v + (c |v - O|^2) u, and a mesh vertex has its u at hand -- the products of the tile's
//            (cos, sin) tables that ground_vertex_from scales by R0 + h -- so the kernels evaluate that form (refraction_lift_along:
//            no square root, no division per vertex; the c4 map of DESIGN.md cost 408 ms with them and 367 ms without).
//            topo_refraction_lift knows only the point and divides by |v| (refraction_lift); the two agree to an ulp of the radius.
//            O itself is resolved on the unlifted mesh, by visibility_observer / k_visibility_observers, unchanged (the lift
//            vanishes at O, to second order).  The corners of the cell under O are lifted by c (cell)^2 -- 0.1 mm at 90 m posts,
//            centimetres on the coarse test tiles -- so an observer ON the ground (height 0) lies that far beneath the lifted
//            triangle: beyond kVisMinRange it no longer "sits at" the target under it and sees that triangle from below.
//   the rest is topo_visibility.h on the lifted vertices: the target under (lon, lat) is found by the surface rule on the lifted
//            triangles (so T lies on the lifted mesh), the AWAY test takes the lifted triangle's normal, the mast height h is added
//            on top, and the sight line is the any-hit ray from T to O with the same bounds and the same skipped triangle.  Classes
//            and error codes are the existing five.  Which triangles EXIST is decided on the unlifted heights (finite for the rays;
//            finite, < 1e9 and > -R0 for the surface), as before.
//   k = 0    gives the bytes of topo_visibility_*, bit for bit: the lift leaves the vertex untouched when c is not > 0 (no
//            0 * inf, no x + 0 x), and every bound below is widened by exactly 0.
//
// Why pruning survives the lift.
//   cells    the lift is radial: a vertex keeps its longitude and latitude, a triangle's directions stay the spherical triangle of
//            its vertices' directions.  The "cells" arguments of topo_los.h (a straight ray) and topo_surface.h (the radial line)
//            speak of directions only and hold unchanged; the candidate cells are computed as before.
//   sphere   the lift is >= 0 and, for a vertex inside a sphere (c_b, r_b) at distance D = |c_b - O|, it lies between
//            l0 = c max(D - r_b, 0)^2 and l = c (D + r_b)^2, so the lifted vertex lies inside (c_b, r_b + l) (refraction_bound; the
//            product carries a factor 1 + 1e-9 for its own rounding).  That sphere is safe and loose: 300 km out l is 900 m around a
//            block of 3 km, although the block's vertices all rise by nearly the same amount.  The test therefore uses the sphere
//            MOVED with them (refraction_sphere): centre c_b' = c_b + m c_b / |c_b| with m = (l0 + l) / 2, and for every vertex
//            |v' - c_b'| <= |v - c_b| + |lift(v) - m| + m |v / |v| - c_b / |c_b|| <= r_b + (l - l0) / 2 + m (2 r_b / |c_b|)
//            (|x / |x| - y / |y|| <= 2 |x - y| / max(|x|, |y|)): the 900 m become 18 m.  On the c4 map this took the call from 367 ms
//            to 183 ms.
//   height   |v'| = |v| + lift <= Rtop + l: the block's shell uses Rtop + l (+ kLosShellPad, as before).
//   tile     a tile's vertices lie within ts[3] + ts[4] of its centre (sphere around the block centres, largest block radius): the
//            same moved sphere with r_b = ts[3] + ts[4].
//   A bound that is not finite or absurd is not used to clip, exactly as before (los_clip_sphere cuts nothing when its test does
//   not come out finite).
//
// The cell tests here are second copies of los_cell<true> and surface_cell with one statement added (the lift, between
// ground_vertex_from and the translation by the origin: refraction_vertex).  They are copies and not a hook in topo_los.h /
// topo_surface.h on purpose: every other translation unit's code stays byte for byte what it was.
//
// Pure functions (TOPO_HD), as topo_visibility.h: a traversal form and an every-triangle form (kAll), as los_cast / los_cast_all
// and surface_lookup / surface_all; the kernels (kernels_refraction.h) call the former for every target, and
// tests/refraction_emul.cpp runs both under g++.
#pragma once

#include "topo_visibility.h"

namespace topo {

constexpr double kRefractionStandard = 0.13;

struct RefLift {           // the lift of one observer: O and c = k / (2 R0)
    double O[3];
    double c;
};

TOPO_HD bool refraction_k_valid(double k) { return k >= 0.0 && k < 1.0; }      // (false for NaN)

TOPO_HD RefLift refraction_make(const double O[3], double k) { return RefLift{{O[0], O[1], O[2]}, k / (2.0 * kGroundR0)}; }

// v -> v' (header comment: lift).  c == 0 leaves v exactly as it was.
TOPO_HD void refraction_lift(const RefLift& L, double v[3]) {
    if (!(L.c > 0.0)) return;
    const double x[3] = {v[0] - L.O[0], v[1] - L.O[1], v[2] - L.O[2]};
    const double s2 = x[0] * x[0] + x[1] * x[1] + x[2] * x[2];
    const double f = L.c * s2 / sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = v[k] + f * v[k];
}

// The same for a vertex whose unit direction u is known: v' = v + (c |v - O|^2) u.  c == 0 leaves v exactly as it was.
TOPO_HD void refraction_lift_along(const RefLift& L, const double u[3], double v[3]) {
    if (!(L.c > 0.0)) return;
    const double x[3] = {v[0] - L.O[0], v[1] - L.O[1], v[2] - L.O[2]};
    const double lift = L.c * (x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = v[k] + lift * u[k];
}

// Vertex (vx, vy) of a tile from its height and the (cos, sin) entries of its column (at lo) and row (at la), lifted.
TOPO_HD void refraction_vertex(const LosScene& S, const RefLift& L, float h, size_t lo, size_t la, double p[3]) {
    const double clo = S.trig[lo], slo = S.trig[lo + 1], cla = S.trig[la], sla = S.trig[la + 1];
    ground_vertex_from(h, clo, slo, cla, sla, p);
    const double u[3] = {cla * clo, cla * slo, sla};
    refraction_lift_along(L, u, p);
}

// No vertex inside the sphere (centre, radius) is lifted by more than this (header comment: sphere).  0 exactly for c == 0.
TOPO_HD double refraction_bound(const RefLift& L, const double centre[3], double radius) {
    if (!(L.c > 0.0)) return 0.0;
    const double x[3] = {centre[0] - L.O[0], centre[1] - L.O[1], centre[2] - L.O[2]};
    const double s = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]) + radius;
    return L.c * s * s * (1.0 + 1.0e-9);
}

// The sphere (centre, radius) moved and widened so that it holds every lifted vertex of the sphere it was (header comment: sphere);
// returns the new radius, the new centre in `moved`.  c == 0: the sphere itself.
TOPO_HD double refraction_sphere(const RefLift& L, const double centre[3], double radius, double moved[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) moved[k] = centre[k];
    if (!(L.c > 0.0)) return radius;
    const double x[3] = {centre[0] - L.O[0], centre[1] - L.O[1], centre[2] - L.O[2]};
    const double dist = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]), near = dist > radius ? dist - radius : 0.0, far = dist + radius;
    const double l0 = L.c * near * near, l1 = L.c * far * far, mid = 0.5 * (l0 + l1);
    const double norm = sqrt(centre[0] * centre[0] + centre[1] * centre[1] + centre[2] * centre[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) moved[k] = centre[k] + (mid / norm) * centre[k];
    return (radius + 0.5 * (l1 - l0) + mid * (2.0 * radius / norm)) * (1.0 + 1.0e-9);
}

// The four corners of cell (i, j) of tile `rank`, lifted, then translated by o: corner (a, b) = vertex (i + a, j + b) at [2 a + b],
// and their heights as stored.  false: the index check failed.
template <class Check>
TOPO_HD bool refraction_corners(const LosScene& S, const TileDev& t, uint32_t rank, uint32_t i, uint32_t j, const RefLift& L, const double o[3], double c[4][3],
                                float h[4], Check&& chk) {
    const size_t tab = (size_t)rank * ground_table_doubles(S.tile_w, S.tile_h);
    const size_t lo = tab + 2 * (size_t)i, la = tab + 2 * ((size_t)S.tile_w + j);
    if (!(chk(i + 1 < S.tile_w && j + 1 < S.tile_h && la + 3 < S.trig_doubles, ((uint64_t)j << 32) | i) && i + 1 < S.tile_w && j + 1 < S.tile_h)) return false;
    const auto hts = TOPO_GLOBAL_F32(t.heights);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t a = (uint32_t)k >> 1, b = (uint32_t)k & 1u;
        h[k] = hts[(size_t)(j + b) * S.tile_w + (i + a)];
        refraction_vertex(S, L, h[k], lo + 2 * a, la + 2 * b, c[k]);
#pragma unroll
        for (int m = 0; m < 3; ++m) c[k][m] -= o[m];
    }
    return true;
}

// Triangle `tri` (one of the two of cell (i, j)) out of the cell's corners; returns whether its three vertices are ok.
TOPO_HD bool refraction_pick(uint32_t tri, uint32_t hm1, uint32_t i, uint32_t j, const double c[4][3], const bool ok[4], double q[3][3]) {
    uint32_t vx[3], vy[3];
    triangle_vertices(tri, hm1, vx, vy);
    bool exists = true;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        const uint32_t at = 2 * (vx[m] - i) + (vy[m] - j);
        exists = exists && ok[at & 3u];
#pragma unroll
        for (int n = 0; n < 3; ++n) q[m][n] = c[at & 3u][n];
    }
    return exists;
}

// surface_cell on the lifted corners.
template <class Check>
TOPO_HD void refraction_surface_cell(const LosScene& S, const TileDev& t, uint32_t rank, uint32_t i, uint32_t j, const RefLift& L, const double u[3], const double o[3],
                                     SurfaceHit& best, Check&& chk) {
    double c[4][3];
    float h[4];
    if (!refraction_corners(S, t, rank, i, j, L, o, c, h, chk)) return;
    const bool ok[4] = {surface_height_ok(h[0]), surface_height_ok(h[1]), surface_height_ok(h[2]), surface_height_ok(h[3])};
    const uint32_t hm1 = S.tile_h - 1, cell = i * hm1 + j;
#pragma unroll
    for (uint32_t k = 0; k < 2; ++k) {
        const uint32_t tri = 2 * cell + k;
        double q[3][3];
        const bool exists = refraction_pick(tri, hm1, i, j, c, ok, q);
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

// The lifted terrain under the direction u: surface_lookup's candidate cells (kAll: surface_all's loop) with the lifted cell test.
template <bool kAll, class Check>
TOPO_HD void refraction_surface(const LosScene& S, const RefLift& L, const double u[3], SurfaceHit& best, Check&& chk) {
    best = SurfaceHit{0.0, 0.0, 0.0, 0u, 0u, false};
    const double o[3] = {kGroundR0 * u[0], kGroundR0 * u[1], kGroundR0 * u[2]};
    if constexpr (kAll) {
        for (uint32_t rank = 0; rank < S.n_tiles; ++rank) {
            if (!surface_tile_ok(S.tiles[rank])) continue;
            for (uint32_t i = 0; i + 1 < S.tile_w; ++i)
                for (uint32_t j = 0; j + 1 < S.tile_h; ++j) refraction_surface_cell(S, S.tiles[rank], rank, i, j, L, u, o, best, chk);
        }
    } else {
        const double norm = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
        double sl = u[2] / norm;
        sl = sl > 1.0 ? 1.0 : (sl < -1.0 ? -1.0 : sl);
        const double lon = atan2(u[1], u[0]) * kGroundDeg, lat = asin(sl) * kGroundDeg;
        if (!ground_finite(lon) || !ground_finite(lat)) return;
        const uint32_t cells_x = S.tile_w - 1, cells_y = S.tile_h - 1;
        for (uint32_t rank = 0; rank < S.n_tiles; ++rank) {
            const TileDev& t = S.tiles[rank];
            const double sx = (double)t.scale_x, sy = (double)t.scale_y;
            const double pad_y = 1.0 / 64.0 + fabs(0.25 * kGroundRad * sx * sx / sy);
            const double fx = los_wrap180(lon - (double)t.model_x) / sx + (double)t.raster_x;
            const double fy = ((double)t.model_y - lat) / sy + (double)t.raster_y;
            if (!surface_tile_ok(t)) continue;
            if (!ground_finite(fx) || !ground_finite(fy) || !ground_finite(pad_y)) continue;
            uint32_t ix0, ix1, iy0, iy1;
            los_cells(fx - kSurfacePadX, fx + kSurfacePadX, 0u, cells_x, ix0, ix1);
            los_cells(fy - pad_y, fy + pad_y, 0u, cells_y, iy0, iy1);
            for (uint32_t i = ix0; i <= ix1 && i < cells_x; ++i)
                for (uint32_t j = iy0; j <= iy1 && j < cells_y; ++j) refraction_surface_cell(S, t, rank, i, j, L, u, o, best, chk);
        }
    }
}

// los_cell<true> on the lifted corners: whether the ray (o, d, [tmin, tmax]) meets a triangle of the cell but skip_tri.
template <class Check>
TOPO_HD bool refraction_los_cell(const LosScene& S, const TileDev& t, uint32_t rank, uint32_t i, uint32_t j, const RefLift& L, const double o[3], const double d[3],
                                 double tmin, double tmax, uint32_t skip_tri, Check&& chk) {
    double c[4][3];
    float h[4];
    if (!refraction_corners(S, t, rank, i, j, L, o, c, h, chk)) return false;
    const bool ok[4] = {ground_finite((double)h[0]), ground_finite((double)h[1]), ground_finite((double)h[2]), ground_finite((double)h[3])};
    const uint32_t hm1 = S.tile_h - 1, cell = i * hm1 + j;
#pragma unroll
    for (uint32_t k = 0; k < 2; ++k) {
        const uint32_t tri = 2 * cell + k;
        if (tri == skip_tri) continue;
        double q[3][3];
        const bool exists = refraction_pick(tri, hm1, i, j, c, ok, q);
        double tt, u, v;
        if (exists && los_triangle(q, d, tmin, tmax, tt, u, v)) return true;
    }
    return false;
}

// The three rejections of a block before its cells, widened for the lift (header comment: sphere, height): false when the ray
// cannot meet a lifted triangle of block `blk` of tile t for t in [ta, tb]; otherwise [ta, tb] cut down to where it can.
TOPO_HD bool refraction_block(const TileDev& t, uint32_t blk, const RefLift& L, const double o[3], const double d[3], double dd, double& ta, double& tb) {
    const double* const bs = t.block_bounds + 4 * (size_t)blk;
    const double hmin = (double)t.block_minmax[2 * (size_t)blk], hmax = (double)t.block_minmax[2 * (size_t)blk + 1];
    const double origin[3] = {0.0, 0.0, 0.0};
    double ell = 0.0;
    if (bs[3] < kLosAbsurd) {
        double moved[3];
        const double r = refraction_sphere(L, bs, bs[3], moved);
        if (!los_clip_sphere(o, d, dd, moved, r, ta, tb)) return false;
        ell = refraction_bound(L, bs, bs[3]);
    }
    if (hmin <= hmax) {
        const double r0 = fabs(kGroundR0 + hmin), r1 = fabs(kGroundR0 + hmax), top = (r0 > r1 ? r0 : r1) + kLosShellPad;
        // (a shell needs the block's sphere for its l: without one it is not used once there is a lift)
        if (top < kLosAbsurd && (bs[3] < kLosAbsurd || !(L.c > 0.0)) && !los_clip_sphere(o, d, dd, origin, top + ell, ta, tb)) return false;
    }
    return true;
}

// Whether the tile's (widened) sphere lets the ray through at all.
TOPO_HD bool refraction_tile(const double* ts, const RefLift& L, const double o[3], const double d[3], double dd, double tmin, double tmax) {
    if (!(ts[3] >= 0.0 && ts[4] >= 0.0)) return true;
    double moved[3];
    const double r = refraction_sphere(L, ts, ts[3] + ts[4], moved);
    return los_clip_sphere(o, d, dd, moved, r, tmin, tmax);
}

// los_cast<true> on the lifted mesh: any hit of r but (skip_rank, skip_tri); kAll: every triangle (los_cast_all<true>).
template <bool kAll, class Check>
TOPO_HD bool refraction_any_hit(const LosScene& S, const RefLift& L, const LosRay& r, uint32_t skip_rank, uint32_t skip_tri, Check&& chk) {
    const double* const o = r.o;
    const double* const d = r.d;
    if constexpr (kAll) {
        for (uint32_t rank = 0; rank < S.n_tiles; ++rank)
            for (uint32_t i = 0; i + 1 < S.tile_w; ++i)
                for (uint32_t j = 0; j + 1 < S.tile_h; ++j)
                    if (refraction_los_cell(S, S.tiles[rank], rank, i, j, L, o, d, r.tmin, r.tmax, rank == skip_rank ? skip_tri : kLosNoTri, chk)) return true;
        return false;
    } else {
        const double oo = o[0] * o[0] + o[1] * o[1] + o[2] * o[2], od = o[0] * d[0] + o[1] * d[1] + o[2] * d[2], dd = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
        const uint32_t cells_x = S.tile_w - 1, cells_y = S.tile_h - 1;
        for (uint32_t rank = 0; rank < S.n_tiles; ++rank) {
            if (!refraction_tile(S.spheres + (size_t)kLosSphereDoubles * rank, L, o, d, dd, r.tmin, r.tmax)) continue;
            const TileDev& t = S.tiles[rank];
            const double sx = (double)t.scale_x, sy = (double)t.scale_y;
            const double pad_y = 1.0 / 64.0 + fabs(0.25 * kGroundRad * sx * sx / sy);
            const uint32_t skip = rank == skip_rank ? skip_tri : kLosNoTri;
            for (uint32_t by = 0; by < S.by_count; ++by)
                for (uint32_t bx = 0; bx < S.bx_count; ++bx) {
                    double ta = r.tmin, tb = r.tmax;
                    if (!refraction_block(t, by * S.bx_count + bx, L, o, d, dd, ta, tb)) continue;
                    const uint32_t cx0 = bx * kLosBCX, cy0 = by * kLosBCY;
                    const uint32_t cx1 = cx0 + kLosBCX < cells_x ? cx0 + kLosBCX : cells_x, cy1 = cy0 + kLosBCY < cells_y ? cy0 + kLosBCY : cells_y;
                    uint32_t ix0 = cx0, ix1 = cx1 - 1, iy0 = cy0, iy1 = cy1 - 1;
                    if (ground_finite(ta) && ground_finite(tb)) los_cell_range(t, o, d, oo, od, dd, ta, tb, pad_y, cx0, cx1, cy0, cy1, ix0, ix1, iy0, iy1);
                    for (uint32_t i = ix0; i <= ix1 && i < cx1; ++i)
                        for (uint32_t j = iy0; j <= iy1 && j < cy1; ++j)
                            if (refraction_los_cell(S, t, rank, i, j, L, o, d, r.tmin, r.tmax, skip, chk)) return true;
                }
        }
        return false;
    }
}

// visibility_facing on the lifted triangle.
template <class Check>
TOPO_HD bool refraction_facing(const LosScene& S, const RefLift& L, uint32_t rank, uint32_t tri, const double u[3], const double D[3], double& nd, Check&& chk) {
    nd = 0.0;
    uint32_t vx[3], vy[3];
    triangle_vertices(tri, S.tile_h - 1, vx, vy);
    const size_t tab = (size_t)rank * ground_table_doubles(S.tile_w, S.tile_h);
    bool ok = rank < S.n_tiles;
#pragma unroll
    for (int m = 0; m < 3; ++m) ok = ok && vx[m] < S.tile_w && vy[m] < S.tile_h && tab + 2 * ((size_t)S.tile_w + vy[m]) + 1 < S.trig_doubles;
    if (!(chk(ok, ((uint64_t)rank << 32) | tri) && ok)) return false;
    const auto hts = TOPO_GLOBAL_F32(S.tiles[rank].heights);
    double p[3][3];
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        const size_t lo = tab + 2 * (size_t)vx[m], la = tab + 2 * ((size_t)S.tile_w + vy[m]);
        refraction_vertex(S, L, hts[(size_t)vy[m] * S.tile_w + vx[m]], lo, la, p[m]);
    }
    const double e1[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
    const double e2[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
    const double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const double nu = n[0] * u[0] + n[1] * u[1] + n[2] * u[2];
    nd = n[0] * D[0] + n[1] * D[1] + n[2] * D[2];
    if (nu < 0.0) nd = -nd;
    return true;
}

// visibility_target on the lifted mesh: steps 1 and 2 of a target, or kVisCast with the ray of step 3 and the skipped triangle.
template <bool kAll, class Check>
TOPO_HD uint8_t refraction_target(const LosScene& S, const VisEye& eye, const RefLift& L, double lon_deg, double lat_deg, double h, LosRay& r, uint32_t& skip_rank,
                                  uint32_t& skip_tri, Check&& chk) {
    skip_rank = skip_tri = kLosNoTri;
    if (!eye.usable) return kVisNoObserver;
    if (!surface_point_valid(lon_deg, lat_deg)) return kVisNone;
    double u[3];
    surface_direction(lon_deg, lat_deg, u);
    SurfaceHit best;
    refraction_surface<kAll>(S, L, u, best, chk);
    if (!best.hit || !(chk(best.rank < S.n_tiles, best.rank) && best.rank < S.n_tiles)) return kVisNone;
    const double rad = (kGroundR0 + best.t) + h;
    double D[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        r.o[k] = rad * u[k];
        D[k] = eye.p[k] - r.o[k];
    }
    const double len = sqrt(D[0] * D[0] + D[1] * D[1] + D[2] * D[2]);
    if (!(len > kVisMinRange)) return kVisVisible;
    if (h == 0.0) {
        double nd;
        if (!refraction_facing(S, L, best.rank, best.tri, u, D, nd, chk)) return kVisNone;
        if (!(nd > 0.0)) return kVisAway;
        skip_rank = best.rank;
        skip_tri = best.tri;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) r.d[k] = D[k] / len;
    r.tmin = kSunTMin;
    r.tmax = len;
    return kVisCast;
}

// The class of a target under coefficient k: steps 1 to 3, a lane's work from end to end.
template <bool kAll, class Check>
TOPO_HD uint8_t refraction_class(const LosScene& S, const VisEye& eye, double k, double lon_deg, double lat_deg, double h, Check&& chk) {
    const RefLift L = refraction_make(eye.p, k);
    LosRay r;
    uint32_t skip_rank, skip_tri;
    const uint8_t c = refraction_target<kAll>(S, eye, L, lon_deg, lat_deg, h, r, skip_rank, skip_tri, chk);
    if (c != kVisCast) return c;
    return refraction_any_hit<kAll>(S, L, r, skip_rank, skip_tri, chk) ? kVisHidden : kVisVisible;
}

}  // namespace topo
