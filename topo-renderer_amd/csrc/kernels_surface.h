// kernels_surface.h -- the drawn terrain under a longitude and latitude (topo_surface.hip: a translation unit of its own, as
// topo_rays.hip, so that the frame path's unit and the rays' stay exactly what they were).
//
//   k_surface        per (lon, lat) of a list, the record of the terrain under it (f64: topo_surface.h)
//   k_surface_grid   the heights over a regular lon / lat raster, f32
//   k_profile        per segment, m samples of the terrain under it and of its own height, and the smallest clearance
//
// All three read the tile table, the DEMs and the tiles' f64 tables (RayParams, as k_raycast; the block tables and spheres are not
// touched) and write only their outputs.  A point costs one to four cells per tile it lies over and a dozen f64 operations per tile
// it does not: there is no loop worth a wave, so k_surface and k_surface_grid give a point to a lane.
#pragma once

#include "kernels_common.h"
#include "topo_surface.h"

namespace topo {
namespace {

__device__ __forceinline__ void surface_store(SurfacePoint* dst, double h, float slope, float aspect, int32_t kind, int32_t tlat, int32_t tlon, uint32_t cx,
                                              uint32_t cy, uint32_t tri, float w1, float w2) {
    int4* d = reinterpret_cast<int4*>(dst);
    d[0] = make_int4(__double2loint(h), __double2hiint(h), __float_as_int(slope), __float_as_int(aspect));
    d[1] = make_int4(kind, tlat, tlon, (int32_t)cx);
    d[2] = make_int4((int32_t)cy, (int32_t)tri, __float_as_int(w1), __float_as_int(w2));
}

// One lane per point.  The point is two doubles (one 16-byte load), the record three 16-byte stores.
__global__ __launch_bounds__(256) void k_surface(RayParams P, const double2* __restrict__ lonlat, SurfacePoint* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const double2 ll = lonlat[i];
    if (!surface_point_valid(ll.x, ll.y)) {
        surface_store(out + i, 0.0, 0.0f, 0.0f, kSurfaceInvalid, 0, 0, 0u, 0u, 0u, 0.0f, 0.0f);
        return;
    }
    auto chk = [&](bool ok, uint64_t value) { return TOPO_CHK(P.check, ok, 22u, value); };
    double u[3];
    surface_direction(ll.x, ll.y, u);
    SurfaceHit best;
    surface_lookup(P.s, u, best, chk);
    // (the rank is tested in the product build too: what it indexes is a table)
    if (!best.hit || !(TOPO_CHK(P.check, best.rank < P.s.n_tiles, 22u, best.rank) && best.rank < P.s.n_tiles)) {
        surface_store(out + i, 0.0, 0.0f, 0.0f, kSurfaceNone, 0, 0, 0u, 0u, 0u, 0.0f, 0.0f);
        return;
    }
    double slope, aspect;
    surface_slope_aspect(P.s, best.rank, best.tri, u, slope, aspect, chk);
    const uint32_t cell = best.tri >> 1, hm1 = P.s.tile_h - 1, cx = cell / hm1, cy = cell - cx * hm1;
    surface_store(out + i, best.t, (float)slope, surface_aspect_f32(aspect), kSurfaceTerrain, P.tile_ll[2 * (size_t)best.rank], P.tile_ll[2 * (size_t)best.rank + 1], cx,
                  cy, best.tri & 1u, (float)best.u, (float)best.v);
}

// The dense form: a wave takes 64 consecutive columns of a row (one contiguous 256-byte store), four waves to a workgroup.  Column
// c lies at lon0 + c dlon and row r at lat0 + r dlat, one rounded product and one rounded sum each: the list call on the same
// numbers gives the same height, bit for bit.  No terrain or an invalid point: a quiet NaN.
__global__ __launch_bounds__(256) void k_surface_grid(RayParams P, double lon0, double lat0, double dlon, double dlat, uint32_t nx, uint32_t ny, uint32_t waves_per_row,
                                                      uint8_t* __restrict__ out, size_t pitch) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = wave_first(blockIdx.x * 4u + (threadIdx.x >> 6));
    const uint32_t r = wave / waves_per_row, c = (wave - r * waves_per_row) * 64u + lane;
    if (r >= ny || c >= nx) return;
    const double lon = lon0 + (double)c * dlon, lat = lat0 + (double)r * dlat;
    float h = __builtin_nanf("");
    if (surface_point_valid(lon, lat)) {
        double u[3];
        surface_direction(lon, lat, u);
        SurfaceHit best;
        surface_lookup(P.s, u, best, [&](bool ok, uint64_t value) { return TOPO_CHK(P.check, ok, 23u, value); });
        if (best.hit) h = (float)best.t;
    }
    *reinterpret_cast<float*>(out + (size_t)r * pitch + 4 * (size_t)c) = h;
}

// One WAVE per segment: lane l takes samples l, l + 64, ... (a wave's 64 samples are one contiguous 512-byte store), keeps its own
// smallest clearance -- its samples come in ascending order, so the first of equal values stays -- and six exchange steps merge the
// lanes' partials under (clearance, sample).  No atomics, no LDS.  samples: null, or segment i's m (terrain, line) pairs at
// samples + i * stride.
__global__ __launch_bounds__(256) void k_profile(RayParams P, const LosRay* __restrict__ segs, uint32_t n, uint32_t m, uint8_t* __restrict__ samples, size_t stride,
                                                 ProfileSummary* __restrict__ summary) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t i = wave_first(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (i >= n) return;
    const double2* const src = reinterpret_cast<const double2*>(segs + i);
    const double2 a = src[0], b = src[1], c = src[2], e = src[3];
    const LosRay r{{a.x, a.y, b.x}, {b.y, c.x, c.y}, e.x, e.y};
    float2* const row = samples ? reinterpret_cast<float2*>(samples + (size_t)i * stride) : nullptr;
    int4* const sum = reinterpret_cast<int4*>(summary + i);
    if (!surface_segment_valid(r)) {
        const float nan = __builtin_nanf("");
        if (row)
            for (uint32_t k = lane; k < m; k += 64) row[k] = make_float2(nan, nan);
        if (lane == 0) *sum = make_int4(0, 0, 0, kSurfaceInvalid);
        return;
    }
    auto chk = [&](bool ok, uint64_t value) { return TOPO_CHK(P.check, ok, 24u, value); };
    ProfileBest best{0.0f, kProfileNoSample, 0u};
    for (uint32_t k = lane; k < m; k += 64) {
        float terrain, line;
        profile_sample(P.s, r, k, m, terrain, line, chk);
        if (row) row[k] = make_float2(terrain, line);
        profile_take(best, k, terrain, line);
    }
#pragma unroll
    for (int s = 32; s; s >>= 1) {
        ProfileBest other;
        other.clearance = __shfl_xor(best.clearance, s);
        other.sample = (uint32_t)__shfl_xor((int)best.sample, s);
        other.n_terrain = (uint32_t)__shfl_xor((int)best.n_terrain, s);
        profile_merge(best, other);
    }
    if (lane != 0) return;
    const float least = best.sample == kProfileNoSample ? __builtin_nanf("") : best.clearance;
    *sum = make_int4(__float_as_int(least), (int32_t)best.sample, (int32_t)best.n_terrain, best.n_terrain ? kSurfaceTerrain : kSurfaceNone);
}

}  // namespace
}  // namespace topo
