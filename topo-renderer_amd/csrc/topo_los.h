// topo_los.h -- rays against the resident terrain (topo_raycast_*): the mesh, the hit rule and the traversal of k_raycast.
//
// The mesh is every triangle of every resident tile: vertex (vx, vy) of a tile at ground_vertex (topo_ground.h: the f32 tile transform
// and the f32 height widened, f64 from there on), triangles and their vertex order from triangle_vertices (topo_pipeline.h).  A
// triangle with a non-finite vertex height does not exist; a finite sentinel is geometry.  A ray is p(t) = origin + t dir with t in
// units of |dir| (dir = B - A, t in [0, 1]: the segment from A to B).
//
// Hit rule: Moeller-Trumbore in f64 on vertices translated by the origin first (the products of 6.4e6 m terms would cost millimetres
// otherwise), both faces; hit iff u >= 0, v >= 0, u + v <= 1, t_min <= t <= t_max, t finite.  The winner is the smallest t, then the
// lower tile rank, then the lower triangle index: a function of the ray and the tile set, not of the traversal.
//
// Traversal (los_cast): tiles by their sphere, raster blocks (kLosBCX x kLosBCY cells) by their bounding sphere and by height, the
// cells of a surviving block by the longitude / latitude range of the part of the ray that is left.  Why each step keeps every hit:
//   sphere   a hit point lies on a triangle of the block, all of whose vertices lie inside the block's (padded) sphere; a sphere is
//            convex, so the point does too, and t lies in the ray's interval inside the sphere.
//   height   |q| of a point q of a flat triangle is at most the largest |vertex| (|.| is convex), and |vertex| = |R0 + h| is at most
//            max(|R0 + hmin|, |R0 + hmax|) =: Rtop; |p(t)|^2 is a convex quadratic in t, so the t with |p(t)| <= Rtop + 1 cm form one
//            interval, and a hit's t lies in it.  A block whose bounds are not finite, not ordered (a void block) or absurd is not clipped.
//   cells    along a straight line, d(lon)/dt = (ox dy - oy dx) / (x^2 + y^2) keeps its sign (the longitude is monotone and sweeps
//            less than 180 degrees), and z / |p| has at most one interior extremum, at t_e = -(dz o.o - oz o.d) / (dz o.d - oz d.d).
//            So the longitudes and latitudes of the interval are bounded by those at its ends and at t_e.  A triangle's directions
//            lie in the spherical triangle of its vertices' directions.  Its meridian edges lie in a plane through the polar axis
//            (one longitude exactly); the great-circle arc between two vertices of one latitude bulges towards the pole by about
//            (dlon^2 / 8) sin(lat) cos(lat) radians -- sub-millimetre at 90 m cells, decimetres at the coarse test tiles -- that is
//            at most dlon / 16 of a row for square cells.  The range is padded by 1/64 cell plus four times that bulge and rounded
//            outwards, so a triangle is never assigned to exactly one longitude / latitude cell.
//   Whatever comes out non-finite (a ray through the polar axis or the centre, an unbounded interval) selects the whole block.
//
// Pure functions (TOPO_HD), as topo_ground.h: k_raycast calls los_cast for every ray, and tests/los_emul.cpp runs the same code
// under g++ -- the traversal, and a brute-force loop over every triangle with the same triangle test and ordering.
#pragma once

#include "topo_ground.h"

namespace topo {

constexpr int32_t kRayHit = 1, kRayMiss = 0, kRayInvalid = -1;
constexpr uint32_t kLosBCX = 60, kLosBCY = 15;      // the raster blocks' cells (= kBCX, kBCY: topo_kernels.h)
constexpr uint32_t kLosSphereDoubles = 5;           // per tile: the centre and radius of the sphere around its block centres, the largest block radius
constexpr double kLosShellPad = 0.01;               // metres over the highest vertex radius of a block
constexpr double kLosAbsurd = 1.0e9;                // a block radius or vertex radius beyond this (a float-nodata sentinel) is not used to clip
constexpr uint32_t kLosNoTri = 0xFFFFFFFFu;

struct LosRay {            // = topo_ray (64 bytes)
    double o[3], d[3], tmin, tmax;
};

struct LosHit {
    double t, u, v;        // u, v: weights of the triangle's second and third vertex
    uint32_t rank, tri, front;
    bool hit;
};

struct LosScene {          // what a traversal reads: the resident tiles and their tables
    const TileDev* tiles;      // n_tiles entries, draw order (rank)
    const double* trig;        // the tiles' f64 (cos, sin) tables (topo_ground.h: ground_table_doubles each)
    const double* spheres;     // kLosSphereDoubles per tile; a radius < 0: unknown
    size_t trig_doubles;
    uint32_t n_tiles, tile_w, tile_h;
    uint32_t bx_count, by_count;
};

TOPO_HD bool los_ray_valid(const LosRay& r) {
    for (int k = 0; k < 3; ++k)
        if (!ground_finite(r.o[k]) || !ground_finite(r.d[k])) return false;
    if (r.d[0] == 0.0 && r.d[1] == 0.0 && r.d[2] == 0.0) return false;
    return r.tmin <= r.tmax;      // (false for a NaN bound)
}

// The triangle q[0], q[1], q[2] -- already translated by the ray's origin -- against the ray t d.
TOPO_HD bool los_triangle(const double q[3][3], const double d[3], double tmin, double tmax, double& t, double& u, double& v) {
    const double e1[3] = {q[1][0] - q[0][0], q[1][1] - q[0][1], q[1][2] - q[0][2]};
    const double e2[3] = {q[2][0] - q[0][0], q[2][1] - q[0][1], q[2][2] - q[0][2]};
    const double pv[3] = {d[1] * e2[2] - d[2] * e2[1], d[2] * e2[0] - d[0] * e2[2], d[0] * e2[1] - d[1] * e2[0]};
    const double det = e1[0] * pv[0] + e1[1] * pv[1] + e1[2] * pv[2];
    const double inv = 1.0 / det;
    const double tv[3] = {-q[0][0], -q[0][1], -q[0][2]};
    u = (tv[0] * pv[0] + tv[1] * pv[1] + tv[2] * pv[2]) * inv;
    const double qv[3] = {tv[1] * e1[2] - tv[2] * e1[1], tv[2] * e1[0] - tv[0] * e1[2], tv[0] * e1[1] - tv[1] * e1[0]};
    v = (d[0] * qv[0] + d[1] * qv[1] + d[2] * qv[2]) * inv;
    t = (e2[0] * qv[0] + e2[1] * qv[1] + e2[2] * qv[2]) * inv;
    return u >= 0.0 && v >= 0.0 && u + v <= 1.0 && t >= tmin && t <= tmax && ground_finite(t);
}

// 1 when the ray meets the side the renderer draws: N . d < 0 with N = (v1 - v0) x (v2 - v0)
TOPO_HD uint32_t los_front(const double q[3][3], const double d[3]) {
    const double e1[3] = {q[1][0] - q[0][0], q[1][1] - q[0][1], q[1][2] - q[0][2]};
    const double e2[3] = {q[2][0] - q[0][0], q[2][1] - q[0][1], q[2][2] - q[0][2]};
    const double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    return n[0] * d[0] + n[1] * d[1] + n[2] * d[2] < 0.0 ? 1u : 0u;
}

TOPO_HD bool los_better(double t, uint32_t rank, uint32_t tri, const LosHit& b) {
    return !b.hit || t < b.t || (t == b.t && (rank < b.rank || (rank == b.rank && tri < b.tri)));
}

// [ta, tb] cut down to the t with |o + t d - c| <= r (dd = d . d); false: nothing is left.  A test that does not come out finite
// cuts nothing.
TOPO_HD bool los_clip_sphere(const double o[3], const double d[3], double dd, const double c[3], double r, double& ta, double& tb) {
    const double x[3] = {o[0] - c[0], o[1] - c[1], o[2] - c[2]};
    const double b = x[0] * d[0] + x[1] * d[1] + x[2] * d[2];
    const double cc = (x[0] * x[0] + x[1] * x[1] + x[2] * x[2]) - r * r;
    const double disc = b * b - dd * cc;
    if (!ground_finite(disc)) return true;
    if (disc < 0.0) return false;
    const double s = sqrt(disc), t0 = (-b - s) / dd, t1 = (-b + s) / dd;
    if (!ground_finite(t0) || !ground_finite(t1)) return true;
    if (t0 > ta) ta = t0;
    if (t1 < tb) tb = t1;
    return ta <= tb;
}

// Cells [c0, c1) cut down to those a coordinate range [lo, hi] (cells, already padded) touches: i0 .. i1 inclusive, i0 > i1 for
// none.  NaN selects them all.
TOPO_HD void los_cells(double lo, double hi, uint32_t c0, uint32_t c1, uint32_t& i0, uint32_t& i1) {
    const double a = floor(lo), b = floor(hi);
    i0 = c0;
    i1 = c1 - 1;
    if (a > (double)c0) i0 = a >= (double)c1 ? c1 : (uint32_t)a;
    if (b < (double)(c1 - 1)) {
        if (b < (double)c0) i0 = c1;
        else i1 = (uint32_t)b;
    }
}

TOPO_HD void los_lon_lat(const double o[3], const double d[3], double t, double& lon_deg, double& lat_deg) {
    const double p[3] = {o[0] + t * d[0], o[1] + t * d[1], o[2] + t * d[2]};
    lon_deg = atan2(p[1], p[0]) * kGroundDeg;
    lat_deg = asin(p[2] / sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2])) * kGroundDeg;
}
TOPO_HD double los_wrap180(double deg) { return deg - 360.0 * floor((deg + 180.0) / 360.0); }      // into [-180, 180)

// The cell ranges of block cells [cx0, cx1) x [cy0, cy1) of tile t that the ray can reach for t in [ta, tb] (header comment: cells).
TOPO_HD void los_cell_range(const TileDev& t, const double o[3], const double d[3], double oo, double od, double dd, double ta, double tb, double pad_y,
                            uint32_t cx0, uint32_t cx1, uint32_t cy0, uint32_t cy1, uint32_t& ix0, uint32_t& ix1, uint32_t& iy0, uint32_t& iy1) {
    double lon0, lat0, lon1, lat1;
    los_lon_lat(o, d, ta, lon0, lat0);
    los_lon_lat(o, d, tb, lon1, lat1);
    double la_lo = lat0 < lat1 ? lat0 : lat1, la_hi = lat0 < lat1 ? lat1 : lat0;
    if (!(la_lo <= la_hi)) la_lo = la_hi = __builtin_nan("");      // (min / max above drop a NaN)
    const double te = -(d[2] * oo - o[2] * od) / (d[2] * od - o[2] * dd);
    if (te > ta && te < tb) {
        double lone, late;
        los_lon_lat(o, d, te, lone, late);
        if (late < la_lo) la_lo = late;
        if (late > la_hi) la_hi = late;
        if (!ground_finite(late)) la_lo = la_hi = __builtin_nan("");
    }
    const double sx = (double)t.scale_x, sy = (double)t.scale_y;
    const double fx0 = los_wrap180(lon0 - (double)t.model_x) / sx + (double)t.raster_x;
    const double fx1 = fx0 + los_wrap180(lon1 - lon0) / sx;
    const double fy0 = ((double)t.model_y - la_lo) / sy + (double)t.raster_y, fy1 = ((double)t.model_y - la_hi) / sy + (double)t.raster_y;
    const double pad_x = 1.0 / 64.0;
    if (ground_finite(fx0) && ground_finite(fx1)) los_cells((fx0 < fx1 ? fx0 : fx1) - pad_x, (fx0 < fx1 ? fx1 : fx0) + pad_x, cx0, cx1, ix0, ix1);
    else { ix0 = cx0; ix1 = cx1 - 1; }
    if (ground_finite(fy0) && ground_finite(fy1)) los_cells((fy0 < fy1 ? fy0 : fy1) - pad_y, (fy0 < fy1 ? fy1 : fy0) + pad_y, cy0, cy1, iy0, iy1);
    else { iy0 = cy0; iy1 = cy1 - 1; }
}

// One cell (i, j) of tile `rank`: its four corners, translated by the origin, and its two triangles against the ray.  kAny: the
// first hit ends the search (true); otherwise the best hit so far is kept in `best` and tmax shrinks to it.  skip_tri: a triangle
// of this tile that does not count (kLosNoTri: none).  chk(ok, value): the caller's index check (the bounds-checking build).
template <bool kAny, class Check>
TOPO_HD bool los_cell(const LosScene& S, const TileDev& t, uint32_t rank, uint32_t i, uint32_t j, const double o[3], const double d[3], double tmin,
                      double& tmax, uint32_t skip_tri, LosHit& best, Check&& chk) {
    const uint32_t hm1 = S.tile_h - 1;
    const size_t tab = (size_t)rank * ground_table_doubles(S.tile_w, S.tile_h);
    const size_t lo = tab + 2 * (size_t)i, la = tab + 2 * ((size_t)S.tile_w + j);
    if (!(chk(i + 1 < S.tile_w && j + 1 < S.tile_h && la + 3 < S.trig_doubles, ((uint64_t)j << 32) | i) && i + 1 < S.tile_w && j + 1 < S.tile_h)) return false;
    double c[4][3];      // corner (a, b) = vertex (i + a, j + b) at [2 a + b]
    bool ok[4];
    const auto hts = TOPO_GLOBAL_F32(t.heights);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t a = (uint32_t)k >> 1, b = (uint32_t)k & 1u;
        const float h = hts[(size_t)(j + b) * S.tile_w + (i + a)];
        ok[k] = ground_finite((double)h);
        ground_vertex_from(h, S.trig[lo + 2 * a], S.trig[lo + 2 * a + 1], S.trig[la + 2 * b], S.trig[la + 2 * b + 1], c[k]);
#pragma unroll
        for (int m = 0; m < 3; ++m) c[k][m] -= o[m];
    }
    const uint32_t cell = i * hm1 + j;
#pragma unroll
    for (uint32_t k = 0; k < 2; ++k) {
        const uint32_t tri = 2 * cell + k;
        if (tri == skip_tri) continue;
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
        double tt, u, v;
        if (!exists || !los_triangle(q, d, tmin, tmax, tt, u, v)) continue;
        if (kAny) {
            best = LosHit{tt, u, v, rank, tri, los_front(q, d), true};
            return true;
        }
        // (field by field, as selects: one flag decides every field of the record and t_max alike)
        const bool better = los_better(tt, rank, tri, best);
        const uint32_t front = los_front(q, d);
        best.t = better ? tt : best.t;
        best.u = better ? u : best.u;
        best.v = better ? v : best.v;
        best.rank = better ? rank : best.rank;
        best.tri = better ? tri : best.tri;
        best.front = better ? front : best.front;
        best.hit = true;
        tmax = better ? tt : tmax;
    }
    return false;
}

// The ray against the scene.  kAny false: the winner (header comment) in `best`; true: any hit at all (returns at the first).
// skip_rank / skip_tri: one triangle that does not count (a ray that starts on it), kLosNoTri for none.
template <bool kAny, class Check>
TOPO_HD void los_cast(const LosScene& S, const LosRay& r, uint32_t skip_rank, uint32_t skip_tri, LosHit& best, Check&& chk) {
    best = LosHit{0.0, 0.0, 0.0, 0u, 0u, 0u, false};
    const double* const o = r.o;
    const double* const d = r.d;
    const double oo = o[0] * o[0] + o[1] * o[1] + o[2] * o[2], od = o[0] * d[0] + o[1] * d[1] + o[2] * d[2], dd = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    const double origin[3] = {0.0, 0.0, 0.0};
    double tmax = r.tmax;
    const uint32_t cells_x = S.tile_w - 1, cells_y = S.tile_h - 1;
    for (uint32_t rank = 0; rank < S.n_tiles; ++rank) {
        const double* const ts = S.spheres + (size_t)kLosSphereDoubles * rank;
        {
            double ta = r.tmin, tb = tmax;
            if (ts[3] >= 0.0 && ts[4] >= 0.0 && !los_clip_sphere(o, d, dd, ts, ts[3] + ts[4], ta, tb)) continue;
        }
        const TileDev& t = S.tiles[rank];
        const double sx = (double)t.scale_x, sy = (double)t.scale_y;
        const double pad_y = 1.0 / 64.0 + fabs(0.25 * kGroundRad * sx * sx / sy);
        const uint32_t skip = rank == skip_rank ? skip_tri : kLosNoTri;
        for (uint32_t by = 0; by < S.by_count; ++by)
            for (uint32_t bx = 0; bx < S.bx_count; ++bx) {
                const uint32_t blk = by * S.bx_count + bx;
                const double* const bs = t.block_bounds + 4 * (size_t)blk;
                const double hmin = (double)t.block_minmax[2 * (size_t)blk], hmax = (double)t.block_minmax[2 * (size_t)blk + 1];
                double ta = r.tmin, tb = tmax;
                if (bs[3] < kLosAbsurd && !los_clip_sphere(o, d, dd, bs, bs[3], ta, tb)) continue;
                if (hmin <= hmax) {
                    const double r0 = fabs(kGroundR0 + hmin), r1 = fabs(kGroundR0 + hmax), top = (r0 > r1 ? r0 : r1) + kLosShellPad;
                    if (top < kLosAbsurd && !los_clip_sphere(o, d, dd, origin, top, ta, tb)) continue;
                }
                const uint32_t cx0 = bx * kLosBCX, cy0 = by * kLosBCY;
                const uint32_t cx1 = cx0 + kLosBCX < cells_x ? cx0 + kLosBCX : cells_x, cy1 = cy0 + kLosBCY < cells_y ? cy0 + kLosBCY : cells_y;
                uint32_t ix0 = cx0, ix1 = cx1 - 1, iy0 = cy0, iy1 = cy1 - 1;
                if (ground_finite(ta) && ground_finite(tb)) los_cell_range(t, o, d, oo, od, dd, ta, tb, pad_y, cx0, cx1, cy0, cy1, ix0, ix1, iy0, iy1);
                for (uint32_t i = ix0; i <= ix1 && i < cx1; ++i)
                    for (uint32_t j = iy0; j <= iy1 && j < cy1; ++j)
                        if (los_cell<kAny>(S, t, rank, i, j, o, d, r.tmin, tmax, skip, best, chk)) return;
            }
    }
}

// The same answer by brute force: every triangle of every tile (the emulation's check of the traversal; never on the device).
template <bool kAny, class Check>
TOPO_HD void los_cast_all(const LosScene& S, const LosRay& r, uint32_t skip_rank, uint32_t skip_tri, LosHit& best, Check&& chk) {
    best = LosHit{0.0, 0.0, 0.0, 0u, 0u, 0u, false};
    double tmax = r.tmax;
    for (uint32_t rank = 0; rank < S.n_tiles; ++rank)
        for (uint32_t i = 0; i + 1 < S.tile_w; ++i)
            for (uint32_t j = 0; j + 1 < S.tile_h; ++j) {
                double keep = r.tmax;      // (no shrinking: every triangle meets the caller's own interval)
                if (los_cell<kAny>(S, S.tiles[rank], rank, i, j, r.o, r.d, r.tmin, kAny ? tmax : keep, rank == skip_rank ? skip_tri : kLosNoTri, best, chk)) return;
            }
}

// ---- sunlit (topo_sunlit_map_device) ----
// The class of a ground point -- the plane point of triangle p[0..2] (triangle `tri` of tile `rank`) with plane weights w1, w2, as
// ground_solve finds it -- under a sun in direction `sun` (unit, towards the sun).  The weights are clamped to >= 0 and renormalised
// first, so that the origin lies ON the triangle: the 1/256 px snapping can put the plane point marginally past an edge, beneath the
// neighbour across a concave fold.  A triangle that faces away from the sun (N . sun <= 0) is kSunAway; otherwise any hit of the ray
// from the origin along `sun` with 1e-3 m < t <= 1e6 m on a triangle other than its own is kSunShadow (the lower bound drops the
// zero-length contact with the neighbours that share an edge), none is kSunLit.
constexpr uint8_t kSunNone = 0, kSunLit = 1, kSunAway = 2, kSunShadow = 3;
constexpr double kSunTMin = 1.0000000000000002e-3;      // the double after 1e-3: t > 1e-3
constexpr double kSunTMax = 1.0e6;

template <class Check>
TOPO_HD uint8_t los_sunlit(const LosScene& S, const double p[3][3], double w1, double w2, uint32_t rank, uint32_t tri, const double sun[3], Check&& chk) {
    double w0 = 1.0 - w1 - w2;
    w0 = w0 > 0.0 ? w0 : 0.0;
    w1 = w1 > 0.0 ? w1 : 0.0;
    w2 = w2 > 0.0 ? w2 : 0.0;
    const double sum = w0 + w1 + w2;
    w0 /= sum; w1 /= sum; w2 /= sum;
    const double e1[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
    const double e2[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
    const double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    if (!(n[0] * sun[0] + n[1] * sun[1] + n[2] * sun[2] > 0.0)) return kSunAway;
    LosRay r;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        r.o[k] = w0 * p[0][k] + w1 * p[1][k] + w2 * p[2][k];
        r.d[k] = sun[k];
    }
    r.tmin = kSunTMin;
    r.tmax = kSunTMax;
    if (!los_ray_valid(r)) return kSunNone;
    LosHit h;
    los_cast<true>(S, r, rank, tri, h, chk);
    return h.hit ? kSunShadow : kSunLit;
}

// What a hit reports of its point p = o + t d: longitude, latitude (degrees), height over the sphere.
TOPO_HD void los_hit_point(const LosRay& r, double t, double& lon_deg, double& lat_deg, double& height) {
    const double p[3] = {r.o[0] + t * r.d[0], r.o[1] + t * r.d[1], r.o[2] + t * r.d[2]};
    const double norm = sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
    lon_deg = atan2(p[1], p[0]) * kGroundDeg;
    lat_deg = asin(p[2] / norm) * kGroundDeg;
    height = norm - kGroundR0;
}

}  // namespace topo
