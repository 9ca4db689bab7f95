// kernels_visibility.h -- what an observer sees, as a map or over a list (topo_visibility.hip: a translation unit of its own, as
// topo_rays.hip and topo_surface.hip, so that the frame path's unit, the rays' and the surface's stay exactly what they were).
//
//   k_visibility_observers   per observer, its point O and whether it can be used (topo_visibility.h), into the context's table
//   k_visibility_grid        one byte (kVis*) per (observer, row, column) of a regular lon / lat raster
//   k_visibility_list        the same per (observer, entry) of a list of (lon, lat)
//
// They read the tile table, the DEMs, the block tables, the tiles' f64 tables and the tile spheres (RayParams, as k_raycast) and
// write only the observer table and their outputs: no atomics, no LDS.
//
// Launch shape.  A wave owns 64 consecutive targets of one observer (64 columns of a row; 64 entries of the list), so its answer is
// one contiguous 64-byte store.  Every lane first looks up its own target and settles what needs no ray (visibility_target: no
// observer, no terrain, the observer at the target, ground that faces away) -- lane work, as k_surface_grid's.  The lanes that
// still need a ray are ballotted, and the WAVE takes their rays one at a time with k_raycast's traversal: 64 block spheres per
// step, the surviving blocks' cells dealt out to the lanes, and the ray is left as soon as any lane has a hit.  The sight lines
// are the expensive rays of DESIGN.md section 5 -- near-horizontal, from the ground -- whose cost is the cells of the blocks they
// graze; in the lane-per-target form (visibility_class<false>: los_cast<true> as it stands) a wave waits for its slowest lane.
// -DTOPO_VISIBILITY_LANE builds that form instead, for the measurement (tools/visibility_profile.py); both give the same bytes.
#pragma once

#include "kernels_common.h"
#include "topo_visibility.h"

namespace topo {
namespace {

// One lane per observer (at most kVisMaxObservers: one wave).
__global__ __launch_bounds__(64) void k_visibility_observers(RayParams P, const VisObserver* __restrict__ obs, VisEye* __restrict__ eyes, uint32_t n) {
    const uint32_t i = threadIdx.x;
    if (i >= n) return;
    VisEye eye;
    visibility_observer<false>(P.s, obs[i], eye, [&](bool ok, uint64_t value) { return TOPO_CHK(P.check, ok, 25u, value); });
    eyes[i] = eye;
}

#ifndef TOPO_VISIBILITY_LANE
// Whether the wave-uniform ray r meets any triangle but (skip_rank, skip_tri): los_cast<true>'s answer, found by the whole wave as
// k_raycast finds its first hit -- the same rejections, the same triangle test -- except that nothing shrinks and the first hit
// of any lane ends the search.
template <uint32_t kTag>
__device__ __forceinline__ bool wave_any_hit(const RayParams& P, const LosRay& r, uint32_t skip_rank, uint32_t skip_tri, uint32_t lane) {
    const LosScene& S = P.s;
    auto chk = [&](bool ok, uint64_t value) { return TOPO_CHK(P.check, ok, kTag, value); };
    const double* const o = r.o;
    const double* const d = r.d;
    const double oo = o[0] * o[0] + o[1] * o[1] + o[2] * o[2], od = o[0] * d[0] + o[1] * d[1] + o[2] * d[2], dd = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    const double origin[3] = {0.0, 0.0, 0.0};
    const uint32_t cells_x = S.tile_w - 1, cells_y = S.tile_h - 1, nb = S.bx_count * S.by_count;
    for (uint32_t rank = 0; rank < S.n_tiles; ++rank) {
        const double* const ts = S.spheres + (size_t)kLosSphereDoubles * rank;
        {
            double ta = r.tmin, tb = r.tmax;
            if (ts[3] >= 0.0 && ts[4] >= 0.0 && !los_clip_sphere(o, d, dd, ts, ts[3] + ts[4], ta, tb)) continue;
        }
        const TileDev& t = S.tiles[rank];
        const double sx = (double)t.scale_x, sy = (double)t.scale_y;
        const double pad_y = 1.0 / 64.0 + fabs(0.25 * kGroundRad * sx * sx / sy);
        const uint32_t skip = rank == skip_rank ? skip_tri : kLosNoTri;
        for (uint32_t b0 = 0; b0 < nb; b0 += 64) {
            const uint32_t blk = b0 + lane;
            double ta = r.tmin, tb = r.tmax;
            bool keep = blk < nb;
            if (keep) {
                const double* const bs = t.block_bounds + 4 * (size_t)blk;
                const double hmin = (double)t.block_minmax[2 * (size_t)blk], hmax = (double)t.block_minmax[2 * (size_t)blk + 1];
                if (bs[3] < kLosAbsurd && !los_clip_sphere(o, d, dd, bs, bs[3], ta, tb)) keep = false;
                if (keep && hmin <= hmax) {
                    const double r0 = fabs(kGroundR0 + hmin), r1 = fabs(kGroundR0 + hmax), top = (r0 > r1 ? r0 : r1) + kLosShellPad;
                    if (top < kLosAbsurd && !los_clip_sphere(o, d, dd, origin, top, ta, tb)) keep = false;
                }
            }
            uint64_t todo = __ballot(keep);
            while (todo) {
                const int j = (int)pop_bit(todo);
                const double ja = lane_f64(ta, j), jb = lane_f64(tb, j);
                const uint32_t bj = b0 + (uint32_t)j, by = bj / S.bx_count, bx = bj - by * S.bx_count;
                const uint32_t cx0 = bx * kLosBCX, cy0 = by * kLosBCY;
                const uint32_t cx1 = cx0 + kLosBCX < cells_x ? cx0 + kLosBCX : cells_x, cy1 = cy0 + kLosBCY < cells_y ? cy0 + kLosBCY : cells_y;
                uint32_t ix0 = cx0, ix1 = cx1 - 1, iy0 = cy0, iy1 = cy1 - 1;
                if (ground_finite(ja) && ground_finite(jb)) los_cell_range(t, o, d, oo, od, dd, ja, jb, pad_y, cx0, cx1, cy0, cy1, ix0, ix1, iy0, iy1);
                if (ix0 > ix1 || iy0 > iy1 || ix1 >= cx1 || iy1 >= cy1) continue;
                const uint32_t ncy = iy1 - iy0 + 1, total = (ix1 - ix0 + 1) * ncy;
                bool hit = false;
                for (uint32_t k = lane; k < total && !hit; k += 64) {
                    const uint32_t ci = k / ncy;
                    LosHit h;
                    double tmax = r.tmax;
                    hit = los_cell<true>(S, t, rank, ix0 + ci, iy0 + (k - ci * ncy), o, d, r.tmin, tmax, skip, h, chk);
                }
                if (__ballot(hit) != 0) return true;
            }
        }
    }
    return false;
}
#endif

// The class of this lane's target (active: it has one) seen from `eye`; the whole wave must call it.
template <uint32_t kTag>
__device__ __forceinline__ uint8_t wave_visibility(const RayParams& P, const VisEye& eye, bool active, double lon, double lat, double h, uint32_t lane) {
    auto chk = [&](bool ok, uint64_t value) { return TOPO_CHK(P.check, ok, kTag, value); };
#ifdef TOPO_VISIBILITY_LANE
    return active ? visibility_class<false>(P.s, eye, lon, lat, h, chk) : kVisNone;
#else
    LosRay r{{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, 0.0, 0.0};
    uint32_t skip_rank = kLosNoTri, skip_tri = kLosNoTri;
    uint8_t cls = active ? visibility_target<false>(P.s, eye, lon, lat, h, r, skip_rank, skip_tri, chk) : kVisNone;
    uint64_t todo = __ballot(cls == kVisCast);
    while (todo) {
        const int j = (int)pop_bit(todo);
        const LosRay q{{lane_f64(r.o[0], j), lane_f64(r.o[1], j), lane_f64(r.o[2], j)}, {lane_f64(r.d[0], j), lane_f64(r.d[1], j), lane_f64(r.d[2], j)},
                       lane_f64(r.tmin, j), lane_f64(r.tmax, j)};
        const uint32_t qr = (uint32_t)__builtin_amdgcn_readlane((int)skip_rank, j), qt = (uint32_t)__builtin_amdgcn_readlane((int)skip_tri, j);
        const bool hit = wave_any_hit<kTag>(P, q, qr, qt, lane);
        if (lane == (uint32_t)j) cls = hit ? kVisHidden : kVisVisible;
    }
    return cls;
#endif
}

// The dense form.  Wave w: observer w / (waves_per_row ny), row and 64 columns from the rest, four waves to a workgroup.  Column c
// lies at lon0 + c dlon and row r at lat0 + r dlat, one rounded product and one rounded sum each, as k_surface_grid: the list call
// on the same numbers gives the same byte.
__global__ __launch_bounds__(256) void k_visibility_grid(RayParams P, const VisEye* __restrict__ eyes, uint32_t n_observers, double lon0, double lat0, double dlon,
                                                         double dlat, uint32_t nx, uint32_t ny, uint32_t waves_per_row, double h, uint8_t* __restrict__ out,
                                                         size_t layer_stride, size_t pitch) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = wave_first(blockIdx.x * 4u + (threadIdx.x >> 6));
    const uint32_t per_layer = waves_per_row * ny;
    const uint32_t ob = wave / per_layer, rem = wave - ob * per_layer;
    const uint32_t r = rem / waves_per_row, c = (rem - r * waves_per_row) * 64u + lane;
    if (ob >= n_observers) return;      // (the last workgroup's spare waves)
    const VisEye eye = eyes[ob];
    const bool active = c < nx;
    const double lon = lon0 + (double)c * dlon, lat = lat0 + (double)r * dlat;
    const uint8_t cls = wave_visibility<25u>(P, eye, active, lon, lat, h, lane);
    if (active) out[(size_t)ob * layer_stride + (size_t)r * pitch + c] = cls;
}

// The list form.  Wave w: observer w / waves_per_list and 64 consecutive entries; a target is two doubles (one 16-byte load).
__global__ __launch_bounds__(256) void k_visibility_list(RayParams P, const VisEye* __restrict__ eyes, uint32_t n_observers, const double2* __restrict__ lonlat,
                                                         uint32_t n, uint32_t waves_per_list, double h, uint8_t* __restrict__ out, size_t list_stride) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = wave_first(blockIdx.x * 4u + (threadIdx.x >> 6));
    const uint32_t ob = wave / waves_per_list, i = (wave - ob * waves_per_list) * 64u + lane;
    if (ob >= n_observers) return;      // (the last workgroup's spare waves)
    const VisEye eye = eyes[ob];
    const bool active = i < n;
    const double2 ll = active ? lonlat[i] : make_double2(0.0, 0.0);
    const uint8_t cls = wave_visibility<26u>(P, eye, active, ll.x, ll.y, h, lane);
    if (active) out[(size_t)ob * list_stride + i] = cls;
}

}  // namespace
}  // namespace topo
