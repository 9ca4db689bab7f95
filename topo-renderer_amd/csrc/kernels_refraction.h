// kernels_refraction.h -- what an observer sees along refracted sight lines, as a map or over a list (topo_refraction.hip: a
// translation unit of its own, as topo_visibility.hip, so that every other unit stays exactly what it was).
//
//   k_visibility_refracted_grid   one byte (kVis*) per (observer, row, column) of a regular lon / lat raster
//   k_visibility_refracted_list   the same per (observer, entry) of a list of (lon, lat)
//
// They read what k_visibility_grid reads (RayParams) and the context's table of resolved observers (k_visibility_observers: the
// observer rule is not repeated here), and write only their outputs: no atomics, no LDS.
//
// Launch shape: k_visibility_grid's.  A wave owns 64 consecutive targets of one observer, so the observer's lift (O and c) is
// wave-uniform.  Every lane first settles its own target with the lifted lookup (refraction_target); the lanes that still need a
// ray are ballotted, and the WAVE takes their rays one at a time: 64 blocks per step against the widened spheres and shells
// (refraction_block), the surviving blocks' cells dealt out to the lanes with their corners lifted (refraction_los_cell), and the
// first hit of any lane ends the ray.
#pragma once

#include "kernels_common.h"
#include "topo_refraction.h"

namespace topo {
namespace {

// Whether the wave-uniform ray r meets any lifted triangle but (skip_rank, skip_tri): refraction_any_hit<false>'s answer, found
// by the whole wave as wave_any_hit (kernels_visibility.h) finds the plain one.
template <uint32_t kTag>
__device__ __forceinline__ bool wave_refracted_hit(const RayParams& P, const RefLift& L, const LosRay& r, uint32_t skip_rank, uint32_t skip_tri, uint32_t lane) {
    const LosScene& S = P.s;
    auto chk = [&](bool ok, uint64_t value) { return TOPO_CHK(P.check, ok, kTag, value); };
    const double* const o = r.o;
    const double* const d = r.d;
    const double oo = o[0] * o[0] + o[1] * o[1] + o[2] * o[2], od = o[0] * d[0] + o[1] * d[1] + o[2] * d[2], dd = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    const uint32_t cells_x = S.tile_w - 1, cells_y = S.tile_h - 1, nb = S.bx_count * S.by_count;
    for (uint32_t rank = 0; rank < S.n_tiles; ++rank) {
        if (!refraction_tile(S.spheres + (size_t)kLosSphereDoubles * rank, L, o, d, dd, r.tmin, r.tmax)) continue;
        const TileDev& t = S.tiles[rank];
        const double sx = (double)t.scale_x, sy = (double)t.scale_y;
        const double pad_y = 1.0 / 64.0 + fabs(0.25 * kGroundRad * sx * sx / sy);
        const uint32_t skip = rank == skip_rank ? skip_tri : kLosNoTri;
        for (uint32_t b0 = 0; b0 < nb; b0 += 64) {
            const uint32_t blk = b0 + lane;
            double ta = r.tmin, tb = r.tmax;
            const bool keep = blk < nb && refraction_block(t, blk, L, o, d, dd, ta, tb);
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
                    hit = refraction_los_cell(S, t, rank, ix0 + ci, iy0 + (k - ci * ncy), L, o, d, r.tmin, r.tmax, skip, chk);
                }
                if (__ballot(hit) != 0) return true;
            }
        }
    }
    return false;
}

// The class of this lane's target (active: it has one) seen from `eye` under the lift L; the whole wave must call it.
template <uint32_t kTag>
__device__ __forceinline__ uint8_t wave_refracted(const RayParams& P, const VisEye& eye, const RefLift& L, bool active, double lon, double lat, double h, uint32_t lane) {
    auto chk = [&](bool ok, uint64_t value) { return TOPO_CHK(P.check, ok, kTag, value); };
    LosRay r{{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, 0.0, 0.0};
    uint32_t skip_rank = kLosNoTri, skip_tri = kLosNoTri;
    uint8_t cls = active ? refraction_target<false>(P.s, eye, L, lon, lat, h, r, skip_rank, skip_tri, chk) : kVisNone;
    uint64_t todo = __ballot(cls == kVisCast);
    while (todo) {
        const int j = (int)pop_bit(todo);
        const LosRay q{{lane_f64(r.o[0], j), lane_f64(r.o[1], j), lane_f64(r.o[2], j)}, {lane_f64(r.d[0], j), lane_f64(r.d[1], j), lane_f64(r.d[2], j)},
                       lane_f64(r.tmin, j), lane_f64(r.tmax, j)};
        const uint32_t qr = (uint32_t)__builtin_amdgcn_readlane((int)skip_rank, j), qt = (uint32_t)__builtin_amdgcn_readlane((int)skip_tri, j);
        const bool hit = wave_refracted_hit<kTag>(P, L, q, qr, qt, lane);
        if (lane == (uint32_t)j) cls = hit ? kVisHidden : kVisVisible;
    }
    return cls;
}

// The dense form: k_visibility_grid's waves, columns and rows (one rounded product and one rounded sum each).
__global__ __launch_bounds__(256) void k_visibility_refracted_grid(RayParams P, const VisEye* __restrict__ eyes, uint32_t n_observers, double lon0, double lat0,
                                                                   double dlon, double dlat, uint32_t nx, uint32_t ny, uint32_t waves_per_row, double h, double k,
                                                                   uint8_t* __restrict__ out, size_t layer_stride, size_t pitch) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = wave_first(blockIdx.x * 4u + (threadIdx.x >> 6));
    const uint32_t per_layer = waves_per_row * ny;
    const uint32_t ob = wave / per_layer, rem = wave - ob * per_layer;
    const uint32_t r = rem / waves_per_row, c = (rem - r * waves_per_row) * 64u + lane;
    if (ob >= n_observers) return;      // (the last workgroup's spare waves)
    const VisEye eye = eyes[ob];
    const RefLift L = refraction_make(eye.p, k);
    const bool active = c < nx;
    const double lon = lon0 + (double)c * dlon, lat = lat0 + (double)r * dlat;
    const uint8_t cls = wave_refracted<48u>(P, eye, L, active, lon, lat, h, lane);
    if (active) out[(size_t)ob * layer_stride + (size_t)r * pitch + c] = cls;
}

// The list form: k_visibility_list's waves; a target is two doubles (one 16-byte load).
__global__ __launch_bounds__(256) void k_visibility_refracted_list(RayParams P, const VisEye* __restrict__ eyes, uint32_t n_observers,
                                                                   const double2* __restrict__ lonlat, uint32_t n, uint32_t waves_per_list, double h, double k,
                                                                   uint8_t* __restrict__ out, size_t list_stride) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = wave_first(blockIdx.x * 4u + (threadIdx.x >> 6));
    const uint32_t ob = wave / waves_per_list, i = (wave - ob * waves_per_list) * 64u + lane;
    if (ob >= n_observers) return;      // (the last workgroup's spare waves)
    const VisEye eye = eyes[ob];
    const RefLift L = refraction_make(eye.p, k);
    const bool active = i < n;
    const double2 ll = active ? lonlat[i] : make_double2(0.0, 0.0);
    const uint8_t cls = wave_refracted<49u>(P, eye, L, active, ll.x, ll.y, h, lane);
    if (active) out[(size_t)ob * list_stride + i] = cls;
}

}  // namespace
}  // namespace topo
