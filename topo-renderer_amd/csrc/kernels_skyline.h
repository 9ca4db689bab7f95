// kernels_skyline.h -- the terrain horizon by azimuth from a point (topo_skyline.hip: a translation unit of its own, as
// topo_rays.hip, topo_surface.hip and topo_visibility.hip, so that the frame path's unit and theirs stay exactly what they were).
//
//   k_skyline   per (observer, azimuth), the highest terrain crossing of the vertical half-plane from the observer along that azimuth
//               (f64: topo_skyline.h), as a record and / or an f32 elevation
//
// It reads the tile table, the DEMs, the block tables, the tiles' f64 tables and the tile spheres (RayParams, as k_raycast) and the
// context's table of resolved observers (k_visibility_observers: the observer rule is not repeated here), and writes only its
// outputs: no atomics, no LDS.
#pragma once

#include "kernels_common.h"
#include "topo_skyline.h"

namespace topo {
namespace {

__device__ __forceinline__ void sky_store(SkySample* dst, double el, double range, double lon, double lat, float h, int32_t kind, int32_t tlat, int32_t tlon,
                                          uint32_t cx, uint32_t cy, uint32_t tri, uint32_t edge) {
    int4* d = reinterpret_cast<int4*>(dst);
    d[0] = make_int4(__double2loint(el), __double2hiint(el), __double2loint(range), __double2hiint(range));
    d[1] = make_int4(__double2loint(lon), __double2hiint(lon), __double2loint(lat), __double2hiint(lat));
    d[2] = make_int4(__float_as_int(h), kind, tlat, tlon);
    d[3] = make_int4((int32_t)cx, (int32_t)cy, (int32_t)tri, (int32_t)edge);
}

// An azimuth without a crossing, or of an unusable observer: a quiet NaN elevation, every other field 0.
__device__ __forceinline__ void sky_store_none(const SkyOut& O, uint32_t ob, uint32_t k, int32_t kind) {
    const double nan = __builtin_nan("");
    if (O.elevation) reinterpret_cast<float*>(O.elevation + (size_t)ob * O.elevation_stride)[k] = (float)nan;
    if (O.samples) sky_store(reinterpret_cast<SkySample*>(O.samples + (size_t)ob * O.samples_stride) + k, nan, 0.0, 0.0, 0.0, 0.0f, kind, 0, 0, 0u, 0u, 0u, 0u);
}

// One WAVE per (observer, azimuth), in the launch shape of k_raycast: wave w has observer w / n_az and azimuth w % n_az, four waves
// to a workgroup.  The lanes take 64 raster blocks of a tile at a time (sky_block: their spheres and heights, one coalesced read),
// the survivors are ballotted and taken one by one, a survivor's cells are dealt out to the lanes, every lane keeps its own best
// crossing under the rule's order, and after each block the wave's best z / s is exchanged: the height test of the blocks that
// follow -- and of the survivors still waiting -- is made against it.  At the end the wave's winner is found with six exchange
// steps.  The answer is skyline_cast's, byte for byte: the same rejections, the same crossing test, the same order.
__global__ __launch_bounds__(256) void k_skyline(RayParams P, const VisEye* __restrict__ eyes, uint32_t n_observers, double az0, double daz, uint32_t n_az,
                                                 double min_range, double max_range, SkyOut O) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t w = wave_first(blockIdx.x * 4u + (threadIdx.x >> 6));
    const uint32_t ob = w / n_az, k = w - ob * n_az;
    if (ob >= n_observers) return;      // (the last workgroup's spare waves)
    const LosScene& S = P.s;
    SkyFrame F;
    skyline_frame(eyes[ob], F);
    if (!F.usable) {
        if (lane == 0) sky_store_none(O, ob, k, kSkyNoObserver);
        return;
    }
    SkyDir D;
    skyline_direction(F, skyline_azimuth(az0, daz, k), D);
    auto chk = [&](bool ok, uint64_t value) { return TOPO_CHK(P.check, ok, 27u, value); };
    const double oo = sky_dot(F.o, F.o), od = sky_dot(F.o, D.h), dd = sky_dot(D.h, D.h);
    SkyBest best{0.0, 0.0, 0.0, 0u, 0u, 0u, false};
    double top = -__builtin_inf();      // the wave's best z / s so far
    const uint32_t nb = S.bx_count * S.by_count;
    for (uint32_t rank = 0; rank < S.n_tiles; ++rank) {
        if (!sky_tile(S, F, D, rank, min_range, max_range)) continue;
        const TileDev& t = S.tiles[rank];
        const double pad_y = sky_pad_y(t);
        for (uint32_t b0 = 0; b0 < nb; b0 += 64) {
            const uint32_t blk = b0 + lane;
            double bound = 0.0, ta = 0.0, tb = 0.0;
            const bool keep = blk < nb && sky_block(F, D, t, blk, min_range, max_range, bound, ta, tb) && !(bound < top);
            uint64_t todo = __ballot(keep);
            while (todo) {
                const int j = (int)pop_bit(todo);
                if (lane_f64(bound, j) < top) continue;      // (the best may have risen since the block was tested)
                const uint32_t bj = b0 + (uint32_t)j, by = bj / S.bx_count, bx = bj - by * S.bx_count;
                uint32_t ix0, ix1, iy0, iy1;
                if (!sky_block_cells(S, t, F, D, oo, od, dd, pad_y, bx, by, lane_f64(ta, j), lane_f64(tb, j), ix0, ix1, iy0, iy1)) continue;
                const uint32_t ncy = iy1 - iy0 + 1, total = (ix1 - ix0 + 1) * ncy;
                for (uint32_t c = lane; c < total; c += 64) {
                    const uint32_t ci = c / ncy;
                    sky_cell(S, t, rank, ix0 + ci, iy0 + (c - ci * ncy), F, D, min_range, max_range, best, chk);
                }
                double mine = best.hit ? best.ratio : -__builtin_inf();
#pragma unroll
                for (int m = 32; m; m >>= 1) {      // the wave's largest z / s
                    const double other = shfl_xor_f64(mine, m);
                    mine = other > mine ? other : mine;
                }
                top = mine;
            }
        }
    }
#pragma unroll
    for (int m = 32; m; m >>= 1) {      // the wave's winner under the rule's order
        SkyBest other;
        other.ratio = shfl_xor_f64(best.ratio, m);
        other.s = shfl_xor_f64(best.s, m);
        other.z = shfl_xor_f64(best.z, m);
        other.rank = (uint32_t)__shfl_xor((int)best.rank, m);
        other.tri = (uint32_t)__shfl_xor((int)best.tri, m);
        other.edge = (uint32_t)__shfl_xor((int)best.edge, m);
        other.hit = __shfl_xor((int)best.hit, m) != 0;
        if (other.hit && sky_better(other.ratio, other.s, other.rank, other.tri, other.edge, best)) best = other;
    }
    if (lane != 0) return;
    SkyPoint p;
    // (the rank is tested in the product build too: what it indexes is a table)
    if (!best.hit || !(TOPO_CHK(P.check, best.rank < S.n_tiles, 27u, best.rank) && best.rank < S.n_tiles) || !skyline_point(S, F, D, best, p, chk)) {
        sky_store_none(O, ob, k, kSkyNone);
        return;
    }
    if (O.elevation) reinterpret_cast<float*>(O.elevation + (size_t)ob * O.elevation_stride)[k] = (float)p.elevation_deg;
    if (O.samples) {
        const uint32_t cell = best.tri >> 1, hm1 = S.tile_h - 1, cx = cell / hm1, cy = cell - cx * hm1;
        sky_store(reinterpret_cast<SkySample*>(O.samples + (size_t)ob * O.samples_stride) + k, p.elevation_deg, p.range_m, p.lon_deg, p.lat_deg, (float)p.height_m,
                  kSkyTerrain, P.tile_ll[2 * (size_t)best.rank], P.tile_ll[2 * (size_t)best.rank + 1], cx, cy, best.tri & 1u, best.edge);
    }
}

}  // namespace
}  // namespace topo
