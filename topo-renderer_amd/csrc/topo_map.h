// topo_map.h -- the map view over a longitude / latitude grid (topo_map_*): the rule, the pieces k_map (kernels_map.h) puts together for
// every pixel, and the box test that lets a wave search the tile table once.
//
// The picture.  Pixel (c, r), c < nx, r < ny, lies at lon0 + c dlon, lat0 + r dlat: one rounded product and one rounded sum each, as
// topo_surface_grid_device.  Its terrain is what surface_lookup (topo_surface.h) finds there -- the same validity of the point, the
// same tolerant edges, the largest t, then draw order, then triangle index.  An invalid point or one with no terrain is VOID.  A
// terrain pixel has a tile rank, a cell, a triangle, the weights u, v and the height t (f64).
//
// Relief.  The three packed normals of the winning triangle's vertices (triangle_vertices' order, the order of the weights) come from
// the tile's normals texture and are unpacked and rotated as the frame does for a vertex (vertex_normal: 2 c / 255 - 1 per channel,
// then the tile's normal_to_world rotation as one fma chain per row).  The weights are w0 = (float)((1 - u) - v) -- the f64 difference
// rounded once -- w1 = (float)u, w2 = (float)v, and each component is n = fmaf(n2, w2, fmaf(n1, w1, n0 * w0)): interpolate_q's chain
// without its division, which normalize3 makes redundant.  The linear value is shade_fragment's view_mode == 1 result for that normal
// and the call's sun_direction, 0.01 + 0.7 max(n^ . sun, 0): the function itself is called, so a map pixel has the grey the frame
// gives the same normal under the same sun, less the dither (which depends on the fragment's position).  The code is srgb_encode of
// it through the frame's threshold table.  Every operation is IEEE binary32, contractions only where fmaf is written
// (-ffp-contract=off on both compilers): hipcc and g++ produce the same code for the same weights and texels.
//
// Contours.  With an interval > 0 the LEVEL of a terrain pixel is floor(t / interval) as a signed 64-bit integer (clamped to +-2^62:
// an interval of 1e-300 m must not overflow the conversion; no real interval comes near).  A pixel is on a contour iff its level
// differs from that of its east neighbour (c + 1, r) or its south neighbour (c, r + 1); a neighbour outside the grid or void takes no
// part.  With index_every = n > 0 it is on an INDEX contour iff for one differing pair a multiple of n lies in (min, max] of the two
// levels: floor_div(max, n) > floor_div(min, n), floor division towards minus infinity.  Levels that differ by more than one (steep
// ground, a small interval) are still one contour pixel.
//
// Seen.  A terrain pixel is seen iff the viewshed masks exist and the bit of (winning tile, winning cell) is set in the tile's mask:
// bit = cell = x (h - 1) + y, what topo_viewshed_read reports.  Either triangle of the cell counts, as in the masks.
//
// Outputs.  flags: bit 0 terrain, bit 1 contour, bit 2 index contour (implies bit 1), bit 3 seen; 0 for a void pixel.  rgba (R G B A in
// memory): void_rgba for a void pixel; else (g, g, g, 255) with g the relief code, 255 with the relief layer off; then, if seen,
// blended with seen_rgba by its alpha in integers, (c (255 - a) + s a + 127) / 255 per colour channel; then, on a contour, blended the
// same way with contour_rgba, or index_rgba on an index contour.  Alpha stays 255 for terrain.  A layer that is off costs nothing and
// sets no flag.
//
// The lookup per tile (map_surface_tile) restates the body of surface_lookup's loop over the tiles, operation for operation, so that a
// caller can run it over a LIST of tiles: surface_lookup itself stays as it is (its translation unit's code must not move).  The order
// in which tiles are examined does not matter: surface_better is a total order on (t, rank, triangle).  tests/map_emul.cpp holds the
// listed form against every tile and against surface_all, bit for bit.
//
// The box test (map_box, map_box_tile): which tiles can hold a pixel of columns [ca, cb] x rows [ra, rb].  The argument:
//  * The pixels.  (double)c dlon is a correctly rounded product and lon0 + that a correctly rounded sum; rounding is monotone, so the
//    longitudes of columns ca .. cb lie between those of ca and cb whatever the sign of dlon (dlon = 0: all equal), and likewise the
//    latitudes of the rows.  The box is [min, max] of the two end values, each computed by the pixel's own expression.
//  * What the lookup sees.  It does not see the pixel's lon and lat but those of its direction: lon' = atan2(u1, u0), lat' = asin(u2).
//    lon' equals lon modulo 360 up to the rounding of sin, cos and atan2 on arguments of magnitude |lon| rad: below 1e-9 degrees while
//    |lon| <= 1e6 degrees.  A box that reaches beyond 1e6 degrees in longitude is taken to hold every longitude (wide).  lat' equals lat
//    up to the conditioning of asin at the poles: asin(1 - e) = pi / 2 - sqrt(2 e), so an ulp of the sine moves the latitude by at most
//    1.5e-8 rad = 8.5e-7 degrees, and by far less away from the poles.  A pixel with |lat| > 90 or a non-finite coordinate is void
//    whatever the list holds.
//  * The tile.  A tile holds a candidate cell for the lookup only if fx = wrap180(lon' - model_x) / scale_x + raster_x lies in
//    [-1/64, cells_x + 1/64) and fy = (model_y - lat') / scale_y + raster_y in [-pad_y, cells_y + pad_y) (los_cells of surface_lookup's
//    ranges selects no cell otherwise).  So the tile's longitudes lie, relative to model_x, between (-p - raster_x) scale_x and
//    (cells_x + p - raster_x) scale_x (sorted: scale_x may be negative) and its latitudes between model_y - (-q - raster_y) scale_y and
//    model_y - (cells_y + q - raster_y) scale_y, with p = 1/32 and q = pad_y + 1/64: twice the lookup's pad in x and 1/64 of a cell
//    more in y, which covers the roundings of fx and fy (1e-11 of a cell) many times.
//  * The test.  Latitude: the two intervals, the box widened by kMapMargin = 1e-4 degrees (a hundred times the polar bound above),
//    must overlap.  Longitude: modulo 360.  With W the box's width, s the tile's span and g = (tile's start - box's end) reduced into
//    [0, 360), the copy of the tile that starts at or behind the box's end begins g behind it and the copy before that ends
//    360 - s - g before it; the box meets no copy iff g > margin and g < 360 - s - W - margin.  wrap180 puts lon' - model_x into
//    [-180, 180): the lookup sees ONE copy of the tile, the test all of them -- it keeps a tile too many at worst.  Wrap-around, a
//    tile whose columns cross the antimeridian and a box that does are all the same case modulo 360; W + s >= 360 rejects nothing.
//  * Every comparison is written so that a NaN (a tile with a non-finite model point, an overflowed box) REJECTS NOTHING; the per-tile
//    lookup then skips what surface_lookup skips.  A tile surface_tile_ok refuses has no surface and is dropped.
//  A wave's list holds at most kMapListCap tiles; a wave whose box meets more examines every tile (map_surface over all ranks), which
//  is the same answer.
//
// Pure functions (TOPO_HD), as topo_surface.h: k_map calls them for every pixel and tests/map_emul.cpp runs the same code under g++.
#pragma once

#include "topo_surface.h"

namespace topo {

constexpr uint32_t kMapRelief = 1u, kMapContours = 2u, kMapSeen = 4u, kMapLayers = 7u;                        // = TOPO_MAP_*
constexpr uint32_t kMapFlagTerrain = 1u, kMapFlagContour = 2u, kMapFlagIndex = 4u, kMapFlagSeen = 8u;         // the flags byte
#ifndef TOPO_MAP_ROWS
#define TOPO_MAP_ROWS 4      // measured on c4: 8 is 4 % ahead on a 1024 x 1024 map and takes 1.7 x as long on a 256 x 256 one, 16 loses on both
#endif
constexpr uint32_t kMapRows = TOPO_MAP_ROWS;      // R: output rows per wave (a wave owns 64 columns x R rows)
constexpr uint32_t kMapListCap = 64;              // tiles a wave's list holds: one per lane
constexpr double kMapMargin = 1.0e-4;             // degrees (header comment: the box test)
constexpr double kMapPadX = 1.0 / 32.0;
constexpr double kMapWideLon = 1.0e6;             // degrees
constexpr double kMapLevelLimit = 4611686018427387904.0;      // 2^62
// what an index check of these functions is about: the kernel's tags are 45 + kind
constexpr uint32_t kMapChkTile = 0, kMapChkVertex = 1, kMapChkMask = 2, kMapChkList = 3;

struct MapCall {           // topo_map_params as the kernel takes it, and the viewshed masks
    double lon0, lat0, dlon, dlat, interval;
    uint32_t nx, ny, index_every, layers;      // layers: kMapContours only with interval > 0, kMapSeen only with masks
    float sun[3];
    uint32_t void_rgba, seen_rgba, contour_rgba, index_rgba;      // R G B A from the low byte
    const uint32_t* const* masks;              // rank -> the tile's mask, or null
    uint32_t mask_words;                       // words of each mask
};

struct MapBox {            // where the pixels of a block of columns and rows lie
    double lon_lo, lon_hi, lat_lo, lat_hi;
    bool wide;             // every longitude
};

struct MapLevel {
    int64_t level;
    bool terrain;
};

// The call topo_map_params stand for (Params: topo_map_params, checked by the caller), over n_tiles resident tiles with the mask table
// `masks` (null: accumulation was never enabled).  A contour layer without a positive interval and a seen layer without tiles or
// masks are off.  The host's map_device and the emulation both come through here.
template <class Params>
inline MapCall map_call(const Params& p, const uint32_t* const* masks, uint32_t mask_words, size_t n_tiles) {
    auto colour = [](const uint8_t c[4]) { return (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16) | ((uint32_t)c[3] << 24); };
    MapCall m{};
    m.lon0 = p.lon0_deg; m.lat0 = p.lat0_deg; m.dlon = p.dlon_deg; m.dlat = p.dlat_deg;
    m.interval = p.contour_interval_m;
    m.nx = p.nx; m.ny = p.ny; m.index_every = p.index_every;
    m.layers = p.layers & kMapLayers;
    if (!(m.interval > 0.0)) m.layers &= ~kMapContours;
    if (n_tiles == 0 || !masks) m.layers &= ~kMapSeen;
    for (int k = 0; k < 3; ++k) m.sun[k] = p.sun_direction[k];
    m.void_rgba = colour(p.void_rgba); m.seen_rgba = colour(p.seen_rgba); m.contour_rgba = colour(p.contour_rgba); m.index_rgba = colour(p.index_rgba);
    m.masks = (m.layers & kMapSeen) ? masks : nullptr;
    m.mask_words = mask_words;
    return m;
}

TOPO_HD double map_lon(const MapCall& M, uint32_t c) { return M.lon0 + (double)c * M.dlon; }
TOPO_HD double map_lat(const MapCall& M, uint32_t r) { return M.lat0 + (double)r * M.dlat; }

TOPO_HD MapBox map_box(const MapCall& M, uint32_t ca, uint32_t cb, uint32_t ra, uint32_t rb) {
    const double la = map_lon(M, ca), lb = map_lon(M, cb), pa = map_lat(M, ra), pb = map_lat(M, rb);
    MapBox b;
    b.lon_lo = la < lb ? la : lb;
    b.lon_hi = la < lb ? lb : la;
    b.lat_lo = pa < pb ? pa : pb;
    b.lat_hi = pa < pb ? pb : pa;
    b.wide = !(fabs(la) <= kMapWideLon && fabs(lb) <= kMapWideLon);
    return b;
}

// May tile t hold a pixel of the box?  (header comment: the box test)
TOPO_HD bool map_box_tile(const MapBox& b, const TileDev& t, uint32_t cells_x, uint32_t cells_y) {
    if (!surface_tile_ok(t)) return false;
    const double sx = (double)t.scale_x, sy = (double)t.scale_y, rx = (double)t.raster_x, ry = (double)t.raster_y;
    const double x0 = (-kMapPadX - rx) * sx, x1 = ((double)cells_x + kMapPadX - rx) * sx;
    const double xa = x0 < x1 ? x0 : x1, xb = x0 < x1 ? x1 : x0;
    const double g0 = xa - (b.lon_hi - (double)t.model_x);
    const double g = g0 - 360.0 * floor(g0 / 360.0);
    const bool miss_lon = !b.wide && g > kMapMargin && g < 360.0 - (xb - xa) - (b.lon_hi - b.lon_lo) - kMapMargin;
    const double q = 1.0 / 32.0 + fabs(0.25 * kGroundRad * sx * sx / sy);      // surface_lookup's pad_y and 1/64 more
    const double y0 = (double)t.model_y - (-q - ry) * sy, y1 = (double)t.model_y - ((double)cells_y + q - ry) * sy;
    const double ya = y0 < y1 ? y0 : y1, yb = y0 < y1 ? y1 : y0;
    const bool miss_lat = b.lat_hi + kMapMargin < ya || b.lat_lo - kMapMargin > yb;
    return !(miss_lon || miss_lat);
}

// Tile `rank` against the line under the direction u whose longitude and latitude (surface_lookup's own: of u) are lon, lat: the body
// of surface_lookup's loop.  chk(ok, value, kind).
template <class Check>
TOPO_HD void map_surface_tile(const LosScene& S, uint32_t rank, double lon, double lat, const double u[3], const double o[3], SurfaceHit& best, Check&& chk) {
    const TileDev& t = S.tiles[rank];
    const uint32_t cells_x = S.tile_w - 1, cells_y = S.tile_h - 1;
    const double sx = (double)t.scale_x, sy = (double)t.scale_y;
    const double pad_y = 1.0 / 64.0 + fabs(0.25 * kGroundRad * sx * sx / sy);
    const double fx = los_wrap180(lon - (double)t.model_x) / sx + (double)t.raster_x;
    const double fy = ((double)t.model_y - lat) / sy + (double)t.raster_y;
    if (!surface_tile_ok(t)) return;
    if (!ground_finite(fx) || !ground_finite(fy) || !ground_finite(pad_y)) return;
    uint32_t ix0, ix1, iy0, iy1;
    los_cells(fx - kSurfacePadX, fx + kSurfacePadX, 0u, cells_x, ix0, ix1);
    los_cells(fy - pad_y, fy + pad_y, 0u, cells_y, iy0, iy1);
    auto cell_chk = [&](bool ok, uint64_t value) { return chk(ok, value, kMapChkVertex); };
    for (uint32_t i = ix0; i <= ix1 && i < cells_x; ++i)
        for (uint32_t j = iy0; j <= iy1 && j < cells_y; ++j) surface_cell(S, t, rank, i, j, u, o, best, cell_chk);
}

// The terrain under (lon_deg, lat_deg) among the n tiles tiles(0) .. tiles(n - 1) (ranks): surface_lookup over a list.
template <class Tiles, class Check>
TOPO_HD void map_surface(const LosScene& S, double lon_deg, double lat_deg, uint32_t n, Tiles&& tiles, SurfaceHit& best, Check&& chk) {
    best = SurfaceHit{0.0, 0.0, 0.0, 0u, 0u, false};
    if (!surface_point_valid(lon_deg, lat_deg)) return;
    double u[3];
    surface_direction(lon_deg, lat_deg, u);
    const double norm = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
    double sl = u[2] / norm;
    sl = sl > 1.0 ? 1.0 : (sl < -1.0 ? -1.0 : sl);
    const double lon = atan2(u[1], u[0]) * kGroundDeg, lat = asin(sl) * kGroundDeg;
    if (!ground_finite(lon) || !ground_finite(lat)) return;
    const double o[3] = {kGroundR0 * u[0], kGroundR0 * u[1], kGroundR0 * u[2]};
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t rank = tiles(k);
        if (!(chk(rank < S.n_tiles, rank, kMapChkTile) && rank < S.n_tiles)) continue;
        map_surface_tile(S, rank, lon, lat, u, o, best, chk);
    }
}

TOPO_HD MapLevel map_level(const MapCall& M, const SurfaceHit& h) {
    if (!h.hit) return MapLevel{0, false};
    double q = floor(h.t / M.interval);
    q = q > kMapLevelLimit ? kMapLevelLimit : (q < -kMapLevelLimit ? -kMapLevelLimit : q);
    return MapLevel{(int64_t)q, true};
}

TOPO_HD int64_t map_floor_div(int64_t a, int64_t n) {      // n > 0
    const int64_t q = a / n;
    return a - q * n < 0 ? q - 1 : q;
}

// The contour bits a pixel gets from ONE neighbour.
TOPO_HD uint32_t map_contour_bits(uint32_t index_every, const MapLevel& own, const MapLevel& other) {
    if (!own.terrain || !other.terrain || own.level == other.level) return 0u;
    const int64_t lo = own.level < other.level ? own.level : other.level, hi = own.level < other.level ? other.level : own.level;
    const bool index = index_every != 0 && map_floor_div(hi, (int64_t)index_every) > map_floor_div(lo, (int64_t)index_every);
    return kMapFlagContour | (index ? kMapFlagIndex : 0u);
}

// The relief code of a hit: `thresh` = the 256 sRGB thresholds as floats (entry 255 = +inf).  A vertex index out of range: 255.
template <class Check>
TOPO_HD uint32_t map_relief(const MapCall& M, const LosScene& S, const SurfaceHit& h, const float* thresh, Check&& chk) {
    const TileDev& t = S.tiles[h.rank];
    uint32_t vx[3], vy[3];
    triangle_vertices(h.tri, S.tile_h - 1, vx, vy);
    bool ok = true;
#pragma unroll
    for (int m = 0; m < 3; ++m) ok = ok && vx[m] < S.tile_w && vy[m] < S.tile_h;
    if (!(chk(ok, ((uint64_t)h.rank << 32) | h.tri, kMapChkVertex) && ok)) return 255u;
    const auto nrm = TOPO_GLOBAL_U32(t.normals);
    const uint32_t p0 = nrm[(size_t)vy[0] * S.tile_w + vx[0]], p1 = nrm[(size_t)vy[1] * S.tile_w + vx[1]], p2 = nrm[(size_t)vy[2] * S.tile_w + vx[2]];
    const f3 n0 = vertex_normal(t, p0), n1 = vertex_normal(t, p1), n2 = vertex_normal(t, p2);
    const float w0 = (float)((1.0 - h.u) - h.v), w1 = (float)h.u, w2 = (float)h.v;
    const f3 n = {fmaf(n2.x, w2, fmaf(n1.x, w1, n0.x * w0)), fmaf(n2.y, w2, fmaf(n1.y, w1, n0.y * w0)), fmaf(n2.z, w2, fmaf(n1.z, w1, n0.z * w0))};
    float lin[4];
    shade_fragment(1, f3{M.sun[0], M.sun[1], M.sun[2]}, 0.0f, 0.0f, 0.0f, 0.0f, f3{0.0f, 0.0f, 0.0f}, n, lin);
    return srgb_encode(thresh, lin[0]);
}

// Is the cell of a hit marked in its tile's mask?  (M.masks is not null)
template <class Check>
TOPO_HD bool map_seen(const MapCall& M, const SurfaceHit& h, Check&& chk) {
    const uint32_t cell = h.tri >> 1, word = cell >> 5;
    if (!(chk(word < M.mask_words, cell, kMapChkMask) && word < M.mask_words)) return false;
    const auto mask = TOPO_GLOBAL_U32(M.masks[h.rank]);
    return ((mask[word] >> (cell & 31u)) & 1u) != 0;
}

// What a pixel knows from its own lookup: the terrain and seen flags, the relief code, the level.
struct MapPixel {
    MapLevel level;
    uint32_t flags, grey;
};
template <class Check>
TOPO_HD MapPixel map_pixel(const MapCall& M, const LosScene& S, const SurfaceHit& h, const float* thresh, Check&& chk) {
    MapPixel p{MapLevel{0, false}, 0u, 255u};
    // (the rank is tested in the product build too: what it indexes is a table)
    if (!h.hit || !(chk(h.rank < S.n_tiles, h.rank, kMapChkTile) && h.rank < S.n_tiles)) return p;
    p.flags = kMapFlagTerrain;
    if (M.layers & kMapContours) p.level = map_level(M, h);
    if (M.layers & kMapRelief) p.grey = map_relief(M, S, h, thresh, chk);
    if ((M.layers & kMapSeen) && map_seen(M, h, chk)) p.flags |= kMapFlagSeen;
    return p;
}

TOPO_HD uint32_t map_blend(uint32_t c, uint32_t s) {      // c's colour channels blended with s by s's alpha; c's alpha stays
    const uint32_t a = s >> 24;
    uint32_t out = c & 0xFF000000u;
#pragma unroll
    for (uint32_t k = 0; k < 24; k += 8) out |= ((((c >> k) & 255u) * (255u - a) + ((s >> k) & 255u) * a + 127u) / 255u) << k;
    return out;
}

TOPO_HD uint32_t map_compose(const MapCall& M, uint32_t flags, uint32_t grey) {
    if (!(flags & kMapFlagTerrain)) return M.void_rgba;
    uint32_t c = grey | (grey << 8) | (grey << 16) | 0xFF000000u;
    if (flags & kMapFlagSeen) c = map_blend(c, M.seen_rgba);
    if (flags & kMapFlagContour) c = map_blend(c, (flags & kMapFlagIndex) ? M.index_rgba : M.contour_rgba);
    return c;
}

// The inverse of the pixel positions (topo_map_xy): fractional (c, r) of a longitude and latitude, the longitude taken modulo 360 to
// the copy nearest the grid's centre column; NaN for an invalid point, and for a coordinate whose step is zero.
TOPO_HD void map_xy(double lon0, double lat0, double dlon, double dlat, uint32_t nx, double lon_deg, double lat_deg, double xy[2]) {
    const double nan = __builtin_nan("");
    xy[0] = xy[1] = nan;
    if (!surface_point_valid(lon_deg, lat_deg)) return;
    const double centre = lon0 + 0.5 * (double)(nx - 1) * dlon;
    const double d = lon_deg - centre;
    const double lon = centre + (d - 360.0 * floor((d + 180.0) / 360.0));
    if (dlon != 0.0) xy[0] = (lon - lon0) / dlon;
    if (dlat != 0.0) xy[1] = (lat_deg - lat0) / dlat;
    if (!ground_finite(xy[0])) xy[0] = nan;
    if (!ground_finite(xy[1])) xy[1] = nan;
}

}  // namespace topo
