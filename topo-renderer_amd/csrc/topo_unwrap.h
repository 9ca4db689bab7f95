// topo_unwrap.h -- unwrapping a strip of perspective views into one azimuth / elevation image (topo_unwrap_*): the arithmetic of
// k_unwrap.
//
// The views share one eye and differ by a rotation about it, so a direction d in the eye's local east / north / up frame is all an
// output pixel needs: view k sees it at clip coordinates m_k (d, 0) -- only the direction part of camera_proj, its translation
// column is never read and the f32 eye does not enter.  Everything up to the source texel is f64.
//
// The tables (one block of doubles, built on the host in f64 -- host_math.cpp: unwrap_tables -- so that the device and the g++ build
// of this header see identical bits):
//     [0, 3)                            up = eye / |eye|
//     [kUnwrapViewsAt + 12 k, + 9)      view k: rows 0, 1 and 3 of camera_proj's 3 x 3 direction block, widened; row r's three
//                                       entries at + 3 r' (r' = 0, 1, 2 for rows 0, 1, 3)
//     [unwrap_cols_at(n), + 3 c ..)     column c: h[c] = sin(az) east + cos(az) north, az = az0 + (c + 0.5) az_span / out_w; the
//                                       table is padded to a multiple of four columns (zeros)
//     [unwrap_rows_at(n, out_w), ..)    row r: (cos el, sin el); the projection (equirectangular or cylindrical) is in this table
//                                       alone -- the kernel does not know it
//
// Per output pixel (c, r):   d = ce[r] h[c] + se[r] up                                            (unwrap_dir)
//     view k:  cx, cy, cw = rows 0, 1, 3 applied to d, each (m0 dx + m1 dy) + m2 dz              (unwrap_row)
//              px = (cx / cw + 1) (src_w / 2),  py = (1 - cy / cw) (src_h / 2)                   (unwrap_project)
//              k CONTAINS the pixel iff cw > 0, 0 <= px < src_w, 0 <= py < src_h
//     source view = the containing view with the largest cw (the one whose axis is nearest); on a tie the lowest index; none: no source.
//     unwrap_locate evaluates that as: the view with the largest cw of all first, and the scan over every view (unwrap_scan) only
//     when that one does not contain the pixel -- the same answer, because a containing view that is also the overall maximum is
//     the maximum among the containing ones, with the same tie rule.
//     nearest:   texel (floor px, floor py)
//     bilinear:  colour only (depth and the source map stay nearest).  u = px - 0.5, v = py - 0.5, x0 = floor u, y0 = floor v,
//                fx = floor((u - x0) 256), fy likewise: 8-bit weights.  The four taps come from the SAME view, their coordinates
//                clamped to the view: a seam is clamped, never crossed.  Each channel is decoded (*Srgb formats: the sRGB decode
//                table, else c / 255), blended in f32 in this order
//                    top = t00 (1 - wx) + t10 wx,  bot = t01 (1 - wx) + t11 wx,  out = top (1 - wy) + bot wy      (w = f / 256)
//                and encoded (srgb_encode / to_unorm8); alpha, byte 3, is a plain unorm in every format, so B G R A needs no case.
//     no source: rgba 0 0 0 0, depth a quiet NaN, source map -1.
//
// Pure functions (TOPO_HD), as topo_ground.h: k_unwrap calls them for every pixel, tests/unwrap_emul.cpp runs the same code under g++.
#pragma once

#include "topo_pipeline.h"

namespace topo {

constexpr uint32_t kUnwrapMaxViews = 64;
constexpr uint32_t kUnwrapViewsAt = 4, kUnwrapViewDoubles = 12;
constexpr uint32_t kUnwrapNoDepthBits = 0x7FC00000u;      // the quiet NaN of a pixel without a source
constexpr double kUnwrapRad = 0.017453292519943295;       // pi / 180

TOPO_HD size_t unwrap_cols_at(uint32_t n_views) { return kUnwrapViewsAt + (size_t)kUnwrapViewDoubles * n_views; }
TOPO_HD size_t unwrap_padded_w(uint32_t out_w) { return ((size_t)out_w + 3) & ~(size_t)3; }
TOPO_HD size_t unwrap_rows_at(uint32_t n_views, uint32_t out_w) { return unwrap_cols_at(n_views) + 3 * unwrap_padded_w(out_w); }
TOPO_HD size_t unwrap_table_doubles(uint32_t n_views, uint32_t out_w, uint32_t out_h) { return unwrap_rows_at(n_views, out_w) + 2 * (size_t)out_h; }

// ---- the tables' entries (host only: sin / cos / tan are the C library's) -------------------------------------------------------
// Column c of out_w over [az0, az0 + span) degrees, clockwise from north.
inline void unwrap_column(double az0_deg, double az_span_deg, uint32_t out_w, uint32_t c, const double east[3], const double north[3], double h[3]) {
    const double az = (az0_deg + ((double)c + 0.5) * az_span_deg / (double)out_w) * kUnwrapRad;
    const double s = sin(az), co = cos(az);
    for (int k = 0; k < 3; ++k) h[k] = s * east[k] + co * north[k];
}
// Row r of out_h between el_top and el_bottom (degrees): linear in the elevation, or (cylindrical) in its tangent.
inline void unwrap_row_entry(bool cylindrical, double el_top_deg, double el_bottom_deg, uint32_t out_h, uint32_t r, double& ce, double& se) {
    const double f = ((double)r + 0.5) / (double)out_h;
    if (cylindrical) {
        const double tt = tan(el_top_deg * kUnwrapRad), tb = tan(el_bottom_deg * kUnwrapRad);
        const double t = tt - f * (tt - tb), n = sqrt(1.0 + t * t);
        ce = 1.0 / n;
        se = t / n;
    } else {
        const double el = (el_top_deg - f * (el_top_deg - el_bottom_deg)) * kUnwrapRad;
        ce = cos(el);
        se = sin(el);
    }
}

// ---- per pixel ------------------------------------------------------------------------------------------------------------------
struct UnwrapSource {
    int32_t view;          // -1: no source
    double px, py;         // the pixel-space point of `view` the output pixel's direction maps to
};

TOPO_HD void unwrap_dir(double ce, double se, const double h[3], const double up[3], double d[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = ce * h[k] + se * up[k];
}
// One row of a view's direction block applied to d.  P: a pointer to doubles (the device reads the views through the constant
// address space).
template <class P>
TOPO_HD double unwrap_row(P m, const double d[3]) { return (m[0] * d[0] + m[1] * d[1]) + m[2] * d[2]; }
// (px, py) of direction d in the view at `m` whose cw is given; true iff the view contains the pixel.
template <class P>
TOPO_HD bool unwrap_project(P m, const double d[3], double cw, uint32_t src_w, uint32_t src_h, double& px, double& py) {
    const double cx = unwrap_row(m, d), cy = unwrap_row(m + 3, d);
    px = (cx / cw + 1.0) * (0.5 * (double)src_w);
    py = (1.0 - cy / cw) * (0.5 * (double)src_h);
    return cw > 0.0 && px >= 0.0 && px < (double)src_w && py >= 0.0 && py < (double)src_h;      // (NaN: not contained)
}
// The containing view with the largest cw among all n_views (ties: the lowest index), or none.
template <class P>
TOPO_HD UnwrapSource unwrap_scan(P views, uint32_t n_views, uint32_t src_w, uint32_t src_h, const double d[3]) {
    UnwrapSource s{-1, 0.0, 0.0};
    double best = 0.0;
    for (uint32_t k = 0; k < n_views; ++k) {
        const P m = views + (size_t)kUnwrapViewDoubles * k;
        const double cw = unwrap_row(m + 6, d);
        double px, py;
        if (cw > best && unwrap_project(m, d, cw, src_w, src_h, px, py)) {
            best = cw;
            s.view = (int32_t)k;
            s.px = px;
            s.py = py;
        }
    }
    return s;
}
template <class P>
TOPO_HD UnwrapSource unwrap_locate(P views, uint32_t n_views, uint32_t src_w, uint32_t src_h, const double d[3]) {
    uint32_t kb = 0;
    double best = unwrap_row(views + 6, d);
    for (uint32_t k = 1; k < n_views; ++k) {
        const double cw = unwrap_row(views + (size_t)kUnwrapViewDoubles * k + 6, d);
        if (cw > best) { best = cw; kb = k; }
    }
    UnwrapSource s{(int32_t)kb, 0.0, 0.0};
    if (unwrap_project(views + (size_t)kUnwrapViewDoubles * kb, d, best, src_w, src_h, s.px, s.py)) return s;
    return unwrap_scan(views, n_views, src_w, src_h, d);
}

// the source map's entry of texel (sx, sy) of `view`
TOPO_HD int32_t unwrap_source_index(uint32_t view, uint32_t sx, uint32_t sy, uint32_t src_w, uint32_t src_h) {
    return (int32_t)((view * src_h + sy) * src_w + sx);
}

// The bilinear footprint of (px, py): the clamped tap columns x[0], x[1], rows y[0], y[1] and the 8-bit weights.
struct UnwrapTaps {
    uint32_t x[2], y[2], fx, fy;
};
TOPO_HD UnwrapTaps unwrap_taps(double px, double py, uint32_t src_w, uint32_t src_h) {
    const double u = px - 0.5, v = py - 0.5, x0 = floor(u), y0 = floor(v);
    UnwrapTaps t;
    t.fx = (uint32_t)floor((u - x0) * 256.0);
    t.fy = (uint32_t)floor((v - y0) * 256.0);
    const int32_t ix = (int32_t)x0, iy = (int32_t)y0, mx = (int32_t)src_w - 1, my = (int32_t)src_h - 1;      // (x0 >= -1: px >= 0)
    t.x[0] = (uint32_t)(ix < 0 ? 0 : ix);
    t.x[1] = (uint32_t)(ix + 1 > mx ? mx : ix + 1);
    t.y[0] = (uint32_t)(iy < 0 ? 0 : iy);
    t.y[1] = (uint32_t)(iy + 1 > my ? my : iy + 1);
    return t;
}
// The blended texel of taps t00 (x[0], y[0]), t10 (x[1], y[0]), t01, t11, in memory order; thresh / decode: the sRGB tables
// (read only when srgb).
TOPO_HD uint32_t unwrap_blend(uint32_t t00, uint32_t t10, uint32_t t01, uint32_t t11, uint32_t fx, uint32_t fy, bool srgb, const float* thresh,
                              const float* decode) {
    const float wx = (float)fx * (1.0f / 256.0f), wy = (float)fy * (1.0f / 256.0f);
    uint32_t out = 0;
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
        const uint32_t sh = 8u * ch;
        const uint32_t c00 = (t00 >> sh) & 255u, c10 = (t10 >> sh) & 255u, c01 = (t01 >> sh) & 255u, c11 = (t11 >> sh) & 255u;
        const bool lin = !srgb || ch == 3;
        const float a = lin ? from_unorm8(c00) : decode[c00], b = lin ? from_unorm8(c10) : decode[c10];
        const float c = lin ? from_unorm8(c01) : decode[c01], e = lin ? from_unorm8(c11) : decode[c11];
        const float top = a * (1.0f - wx) + b * wx, bot = c * (1.0f - wx) + e * wx;
        const float v = top * (1.0f - wy) + bot * wy;
        out |= (lin ? to_unorm8(v) : srgb_encode(thresh, v)) << sh;
    }
    return out;
}

}  // namespace topo
