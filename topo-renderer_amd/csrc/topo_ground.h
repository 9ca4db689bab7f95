// topo_ground.h -- the ground point under a pixel (topo_ground_*): the arithmetic of k_ground and k_ground_map.
//
// A pixel's visibility key names the triangle that won it.  The ground point is the unique point of that triangle's PLANE which the
// view's camera_proj maps to the pixel centre (x + 0.5, y + 0.5) -- marginally outside the triangle where the 1/256 px snapping moved
// an edge; a near-clipped piece answers with its original triangle's plane.  Everything is f64: the six f32 tile values, the f32
// height, the 16 f32 matrix entries and the f32 eye are widened exactly and taken as exact (the frame's own f32 depth is only good
// to about 2 / w -- hundreds of metres of range at 20 km -- and gives no position at all).
//
// Pure functions (TOPO_HD), as topo_pipeline.h: the two kernels call ground_solve for every pixel they answer, and
// tests/ground_emul.cpp runs the same code under g++.
#pragma once

#include "topo_pipeline.h"

namespace topo {

constexpr double kGroundR0 = 6371000.0;                     // kR0, widened
constexpr double kGroundRad = 0.017453292519943295;         // pi / 180
constexpr double kGroundDeg = 57.29577951308232;            // 180 / pi

// kinds of a ground record (topo_ground_point.kind)
constexpr int32_t kGroundTerrain = 1, kGroundSky = 0, kGroundOutside = -1, kGroundIncomplete = -2, kGroundDegenerate = -3;

struct GroundView {        // what a view contributes: camera_proj (column-major) and the eye, as the caller's topo_uniforms hold them
    float proj[16];
    float pos[3];
    float pad_;
};

struct GroundTri {         // a key's low word, decoded (draw = rank * tris_per_tile + triangle, as k_viewshed / k_horizon)
    uint32_t rank, tri, cell_x, cell_y, fan;
};

struct GroundResult {
    double lon_deg, lat_deg, height, range, w1, w2;
    bool ok;               // every value finite (a void vertex or a vanishing determinant: not)
};

TOPO_HD GroundTri ground_decode(uint32_t id, uint32_t tris_per_tile, uint32_t hm1) {
    GroundTri g;
    const uint32_t draw = id >> 1;
    g.fan = id & 1u;
    g.rank = draw / tris_per_tile;
    g.tri = draw - g.rank * tris_per_tile;
    const uint32_t cell = g.tri >> 1;
    g.cell_x = cell / hm1;
    g.cell_y = cell - g.cell_x * hm1;
    return g;
}

TOPO_HD bool ground_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }      // (false for NaN)

// ECEF position of a vertex: vertex_lon / vertex_lat / world_from_sincos of the frame path, in f64.  Longitude depends only on the
// vertex column and latitude only on its row, so the kernels read (cos, sin) of both from per-tile tables (k_ground_tables: one entry
// per column and per row, these very functions) instead of evaluating four f64 sin / cos per vertex and pixel.
TOPO_HD void ground_trig_lon(const TileDev& t, uint32_t vx, double& c, double& s) {
    const double lon = (((double)vx - (double)t.raster_x) * (double)t.scale_x + (double)t.model_x) * kGroundRad;
    c = cos(lon);
    s = sin(lon);
}
TOPO_HD void ground_trig_lat(const TileDev& t, uint32_t vy, double& c, double& s) {
    const double lat = (((double)vy - (double)t.raster_y) * -(double)t.scale_y + (double)t.model_y) * kGroundRad;
    c = cos(lat);
    s = sin(lat);
}
TOPO_HD void ground_vertex_from(float h, double clo, double slo, double cla, double sla, double p[3]) {
    const double r = kGroundR0 + (double)h;
    p[0] = r * cla * clo;
    p[1] = r * cla * slo;
    p[2] = r * sla;
}
TOPO_HD void ground_vertex(const TileDev& t, uint32_t vx, uint32_t vy, float h, double p[3]) {
    double clo, slo, cla, sla;
    ground_trig_lon(t, vx, clo, slo);
    ground_trig_lat(t, vy, cla, sla);
    ground_vertex_from(h, clo, slo, cla, sla, p);
}
// A tile's table: (cos, sin) of the longitude of column x at [2 x], [2 x + 1], then of the latitude of row y at [2 (w + y)], [2 (w + y) + 1].
TOPO_HD size_t ground_table_doubles(uint32_t tile_w, uint32_t tile_h) { return 2 * ((size_t)tile_w + tile_h); }

// The point of the plane through p[0], p[1], p[2] that `view` maps to NDC (gx, gy).  clip() is affine in the point, so with
// barycentric weights l (sum 1) clip(sum l_i p_i) = sum l_i clip_i, and the two conditions clip.x = gx clip.w, clip.y = gy clip.w read
// l . a = 0, l . b = 0 with a_i = clip_i.x - gx clip_i.w, b_i = clip_i.y - gy clip_i.w: l is a x b, scaled to sum 1 (the adjugate
// weights of clip space).  a_i and b_i are metres across the view at the vertex's depth -- the size of the triangle when the pixel
// lies in it -- formed from sums of terms of 6.4e6 m: good to about 1e-9 m in f64.
TOPO_HD GroundResult ground_solve(const double p[3][3], const GroundView& view, double gx, double gy) {
    const float* m = view.proj;
    double a[3], b[3];
    for (int i = 0; i < 3; ++i) {
        const double X = p[i][0], Y = p[i][1], Z = p[i][2];
        const double cx = (double)m[0] * X + (double)m[4] * Y + (double)m[8] * Z + (double)m[12];
        const double cy = (double)m[1] * X + (double)m[5] * Y + (double)m[9] * Z + (double)m[13];
        const double cw = (double)m[3] * X + (double)m[7] * Y + (double)m[11] * Z + (double)m[15];
        a[i] = cx - gx * cw;
        b[i] = cy - gy * cw;
    }
    const double q0 = a[1] * b[2] - a[2] * b[1], q1 = a[2] * b[0] - a[0] * b[2], q2 = a[0] * b[1] - a[1] * b[0];
    const double s = q0 + q1 + q2;
    GroundResult r;
    r.w1 = q1 / s;
    r.w2 = q2 / s;
    double g[3];
    for (int k = 0; k < 3; ++k) g[k] = p[0][k] + r.w1 * (p[1][k] - p[0][k]) + r.w2 * (p[2][k] - p[0][k]);
    const double norm = sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
    const double dx = g[0] - (double)view.pos[0], dy = g[1] - (double)view.pos[1], dz = g[2] - (double)view.pos[2];
    r.lon_deg = atan2(g[1], g[0]) * kGroundDeg;
    r.lat_deg = asin(g[2] / norm) * kGroundDeg;
    r.height = norm - kGroundR0;
    r.range = sqrt(dx * dx + dy * dy + dz * dz);
    r.ok = ground_finite(r.lon_deg) && ground_finite(r.lat_deg) && ground_finite(r.height) && ground_finite(r.range) && ground_finite(r.w1) &&
           ground_finite(r.w2);
    return r;
}

// NDC of the centre of pixel (x, y) of a W x H target (framebuffer y runs down)
TOPO_HD double ground_ndc_x(uint32_t x, uint32_t W) { return ((double)x + 0.5) * 2.0 / (double)W - 1.0; }
TOPO_HD double ground_ndc_y(uint32_t y, uint32_t H) { return 1.0 - ((double)y + 0.5) * 2.0 / (double)H; }

}  // namespace topo
