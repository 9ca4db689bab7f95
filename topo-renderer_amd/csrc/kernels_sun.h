// kernels_sun.h -- a day of sun and shadow over points of the drawn terrain, as a map or over a list (topo_sun.hip: a translation
// unit of its own, as every query family's, so that the other units stay exactly what they were).
//
//   k_sun_exposure_grid      per (row, column) of a regular lon / lat raster: the LIT and SHADOW masks over the call's suns and the
//                            weighted exposure (topo_sun.h)
//   k_sun_exposure_list      the same per entry of a list of (lon, lat)
//
// They read what the rays read (RayParams) and the call's suns (at most kSunMaxSuns, wave-uniform: scalar loads) and write only their
// outputs: no atomics, no LDS.
//
// Launch shape, as k_visibility_grid's.  A wave owns 64 consecutive targets (64 columns of a row; 64 entries of the list).  Every
// lane looks up its own target ONCE (sun_target) and keeps T, u and the turned N in registers for all the suns.  Then, sun by sun in
// ascending order: the lanes settle NIGHT and AWAY themselves (sun_settle: two dot products), the lanes that still need a ray are
// ballotted, and the WAVE takes their rays one at a time with wave_sun_hit -- the visibility kernels' traversal with the tiles'
// spheres tested lane-parallel.  Each lane gathers its bits and its f64 sum in registers, so the wave's answer is one contiguous
// 512-byte store per mask and one 256-byte store of exposures.
// -DTOPO_SUN_LANE builds the lane-per-target form instead (sun_class<false>: los_cast<true> as it stands), for the measurement
// (tools/sun_exposure_profile.py); both give the same bytes.
#pragma once

#include "kernels_common.h"
#include "topo_sun.h"

namespace topo {
namespace {

struct SunOut {            // each null or: entry i of the wave's row at + 8 i (masks), + 4 i (exposure)
    uint64_t* lit;
    uint64_t* shadow;
    float* exposure;
};

#ifndef TOPO_SUN_LANE
// Whether the wave-uniform ray r meets any triangle of tile `rank` but (skip_rank, skip_tri): 64 block spheres per step, the surviving
// blocks' cells dealt out to the lanes, left at the first hit of any lane.  oo, od, dd: o . o, o . d, d . d of the ray.
// A COPY of the walk inside wave_any_hit (kernels_visibility.h), statement for statement: shared through a header the visibility
// kernels keep their registers but not their instructions, and that unit is to stay what it was.
template <uint32_t kTag>
__device__ __forceinline__ bool wave_sun_hit_tile(const RayParams& P, const LosRay& r, double oo, double od, double dd, uint32_t rank, uint32_t skip_rank,
                                                  uint32_t skip_tri, uint32_t lane) {
    const LosScene& S = P.s;
    auto chk = [&](bool ok, uint64_t value) { return TOPO_CHK(P.check, ok, kTag, value); };
    const double* const o = r.o;
    const double* const d = r.d;
    const double origin[3] = {0.0, 0.0, 0.0};
    const uint32_t cells_x = S.tile_w - 1, cells_y = S.tile_h - 1, nb = S.bx_count * S.by_count;
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
    return false;
}

// Whether the wave-uniform ray r meets any triangle but (skip_rank, skip_tri): los_cast<true>'s answer, found by the whole wave as
// wave_any_hit finds it -- the same rejections, the same triangle test, the first hit of any lane ends the search -- except that the
// tiles' spheres are tested 64 at a time, a tile to a lane, and only the tiles that pass are walked: the same test on the same numbers,
// so the same tiles.  (A sun's ray misses nearly every tile of a mosaic and, unlike a sight line, nearly always runs to its end:
// measured on the c4 mosaic, 1746 ms with the tiles tested one after the other, 1171 ms so.)
template <uint32_t kTag>
__device__ __forceinline__ bool wave_sun_hit(const RayParams& P, const LosRay& r, uint32_t skip_rank, uint32_t skip_tri, uint32_t lane) {
    const LosScene& S = P.s;
    const double* const o = r.o;
    const double* const d = r.d;
    const double oo = o[0] * o[0] + o[1] * o[1] + o[2] * o[2], od = o[0] * d[0] + o[1] * d[1] + o[2] * d[2], dd = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    for (uint32_t r0 = 0; r0 < S.n_tiles; r0 += 64) {
        const uint32_t mine = r0 + lane;
        bool keep = mine < S.n_tiles;
        if (keep) {
            const double* const ts = S.spheres + (size_t)kLosSphereDoubles * mine;
            double ta = r.tmin, tb = r.tmax;
            if (ts[3] >= 0.0 && ts[4] >= 0.0 && !los_clip_sphere(o, d, dd, ts, ts[3] + ts[4], ta, tb)) keep = false;
        }
        uint64_t tiles = __ballot(keep);
        while (tiles) {
            const uint32_t rank = r0 + pop_bit(tiles);
            if (wave_sun_hit_tile<kTag>(P, r, oo, od, dd, rank, skip_rank, skip_tri, lane)) return true;
        }
    }
    return false;
}

#endif

// This lane's target (active: it has one) under the n_suns suns, stored at entry `at` of `out`; the whole wave must call it.
template <uint32_t kTag>
__device__ __forceinline__ void wave_sun_exposure(const RayParams& P, const SunDir* __restrict__ suns, uint32_t n_suns, bool active, double lon, double lat, uint32_t lane,
                                                  const SunOut& out, size_t at) {
    auto chk = [&](bool ok, uint64_t value) { return TOPO_CHK(P.check, ok, kTag, value); };
    SunTarget g{{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, 0.0, kLosNoTri, kLosNoTri, false};
    if (active) sun_target<false>(P.s, lon, lat, g, chk);
    SunSums a{0ull, 0ull, 0.0};
    for (uint32_t k = 0; k < n_suns; ++k) {
        const double s[3] = {suns[k].d[0], suns[k].d[1], suns[k].d[2]};
        const double weight = suns[k].weight;
        double ns = 0.0;
#ifdef TOPO_SUN_LANE
        const uint8_t cls = sun_class<false>(P.s, g, s, ns, chk);
#else
        uint8_t cls = g.terrain ? sun_settle(g, s, ns) : kSunNone;
        uint64_t todo = __ballot(cls == kSunCast);
        while (todo) {
            const int j = (int)pop_bit(todo);
            const LosRay q{{lane_f64(g.T[0], j), lane_f64(g.T[1], j), lane_f64(g.T[2], j)}, {s[0], s[1], s[2]}, kSunTMin, kSunTMax};
            const uint32_t qr = (uint32_t)__builtin_amdgcn_readlane((int)g.rank, j), qt = (uint32_t)__builtin_amdgcn_readlane((int)g.tri, j);
            const bool hit = wave_sun_hit<kTag>(P, q, qr, qt, lane);
            if (lane == (uint32_t)j) cls = hit ? kSunShadow : kSunLit;
        }
#endif
        sun_take(a, g, k, cls, weight, ns);
    }
    if (!active) return;
    if (out.lit) out.lit[at] = a.lit;
    if (out.shadow) out.shadow[at] = a.shadow;
    if (out.exposure) out.exposure[at] = sun_exposure_f32(g, a);
}

// Row r of an output whose rows lie `pitch` bytes apart (null stays null).
template <class T>
__device__ __forceinline__ T* sun_row(T* base, uint32_t r, size_t pitch) {
    return base ? reinterpret_cast<T*>(reinterpret_cast<uint8_t*>(base) + (size_t)r * pitch) : nullptr;
}

// The dense form.  Wave w: row w / waves_per_row and 64 columns from the rest, four waves to a workgroup.  Column c lies at
// lon0 + c dlon and row r at lat0 + r dlat, one rounded product and one rounded sum each, as k_visibility_grid: the list call on the
// same numbers gives the same answers.
__global__ __launch_bounds__(256) void k_sun_exposure_grid(RayParams P, const SunDir* __restrict__ suns, uint32_t n_suns, double lon0, double lat0, double dlon, double dlat,
                                                           uint32_t nx, uint32_t ny, uint32_t waves_per_row, SunOut out, size_t mask_pitch, size_t exposure_pitch) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = wave_first(blockIdx.x * 4u + (threadIdx.x >> 6));
    const uint32_t r = wave / waves_per_row, c = (wave - r * waves_per_row) * 64u + lane;
    if (r >= ny) return;      // (the last workgroup's spare waves)
    const double lon = lon0 + (double)c * dlon, lat = lat0 + (double)r * dlat;
    const SunOut row{sun_row(out.lit, r, mask_pitch), sun_row(out.shadow, r, mask_pitch), sun_row(out.exposure, r, exposure_pitch)};
    wave_sun_exposure<28u>(P, suns, n_suns, c < nx, lon, lat, lane, row, c);
}

// The list form.  Wave w: 64 consecutive entries; a target is two doubles (one 16-byte load).
__global__ __launch_bounds__(256) void k_sun_exposure_list(RayParams P, const SunDir* __restrict__ suns, uint32_t n_suns, const double2* __restrict__ lonlat, uint32_t n,
                                                           SunOut out) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = wave_first(blockIdx.x * 4u + (threadIdx.x >> 6));
    const uint64_t i = (uint64_t)wave * 64u + lane;
    if ((uint64_t)wave * 64u >= n) return;      // (the last workgroup's spare waves)
    const bool active = i < n;
    const double2 ll = active ? lonlat[i] : make_double2(0.0, 0.0);
    wave_sun_exposure<29u>(P, suns, n_suns, active, ll.x, ll.y, lane, out, (size_t)i);
}

}  // namespace
}  // namespace topo
