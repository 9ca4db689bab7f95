// kernels_map.h -- the map view over a longitude / latitude grid (topo_map.hip: a translation unit of its own, as topo_surface.hip,
// so that every other unit's code stays exactly what it was).
//
//   k_map   per pixel of a regular lon / lat raster: relief grey, contour and index-contour bits, the viewshed bit -- as RGBA and as
//           a flags byte (topo_map.h states the rule)
//
// A wave owns 64 consecutive columns and kMapRows rows.
//   Tiles.  Before any pixel work the wave tests the tile table against the box of its pixels (map_box_tile), a tile a lane, 64 tiles
//   a step, and keeps the ranks that pass, one per lane of a register (a ballot, then a scalar loop over its bits: the kept tiles are
//   one to four).  The pixels run the per-tile part of the lookup over that list only: k_surface_grid walks the whole table in every
//   lane.  More than kMapListCap kept tiles: the wave walks the whole table, which is the same answer.
//   Neighbours.  The wave does its rows from north to south; the lookup of row r + 1 is made before row r is finished, so the south
//   level is at hand, and the east level comes from the next lane (one DPP shift per word).  The row below the wave's last costs one
//   more lookup per lane (the south halo) and the column right of lane 63 one pass in which lane j looks up row j of that column (the
//   east halo): R + 2 passes for R rows.  -DTOPO_MAP_RECOMPUTE is the other way, three lookups per pixel and no exchange, and
//   -DTOPO_MAP_ALL_TILES the lookup over every tile; DESIGN.md has the three next to each other.  With the contour layer off there is
//   no halo and no second lookup.
//   Memory.  A row of the wave is one contiguous 256-byte store of RGBA and one 64-byte store of flags.  Normals are three 4-byte
//   loads per pixel and the mask is one word per pixel; neighbouring pixels share both.  The sRGB thresholds are staged in LDS once
//   per workgroup (1 KiB), as k_resolve has them.
// Every lane stays active to the end of the wave (a column beyond nx looks up an invalid point, which costs nothing): the DPP shift
// reads its neighbour whatever the width of the grid.
#pragma once

#include "kernels_common.h"
#include "topo_map.h"

namespace topo {
namespace {

static_assert(kMapRows >= 1 && kMapRows <= 64 && kMapListCap == 64, "a lane per row of the east halo, a lane per listed tile");

__device__ __forceinline__ uint32_t map_from_right(uint32_t v, uint32_t last) {      // lane i: lane i + 1's v; lane 63: `last`
    return (uint32_t)__builtin_amdgcn_update_dpp((int32_t)last, (int32_t)v, 0x130 /* wave_shl:1 */, 0xF, 0xF, false);
}
__device__ __forceinline__ uint32_t map_lane(uint32_t v, uint32_t src) {      // lane `src`'s v for a wave-uniform src
    return (uint32_t)__builtin_amdgcn_readlane((int32_t)v, (int32_t)wave_first(src));
}

__global__ __launch_bounds__(256) void k_map(RayParams P, MapCall M, uint32_t waves_x, uint32_t n_waves, uint8_t* __restrict__ rgba, size_t rgba_pitch,
                                             uint8_t* __restrict__ flags, size_t flags_pitch) {
    __shared__ float s_thresh[256];      // sRGB code boundaries, entry 255 = +inf
    s_thresh[threadIdx.x] = bits_f(TOPO_SRGB_THRESH_BITS[threadIdx.x]);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = wave_first(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (wave >= n_waves) return;      // (the last workgroup's spare waves)
    const uint32_t band = wave / waves_x, c0 = (wave - band * waves_x) * 64u, r0 = band * kMapRows;
    const uint32_t r1 = r0 + kMapRows < M.ny ? r0 + kMapRows : M.ny;
    const uint32_t c = c0 + lane;
    const bool in = c < M.nx, contours = (M.layers & kMapContours) != 0;
    const LosScene& S = P.s;
    auto chk = [&](bool ok, uint64_t value, uint32_t kind) { return TOPO_CHK(P.check, ok, 45u + kind, value); };
    const double nan = __builtin_nan("");
    const bool east = (uint64_t)c0 + 64 < M.nx;      // a column right of the wave (64 bits: c0 + 64 may pass 2^32)

    // the wave's tiles: lane k of `list` holds the k-th kept rank
    uint32_t list = 0, count = 0;
#ifndef TOPO_MAP_ALL_TILES
    {
        const MapBox box = map_box(M, c0, east ? c0 + 64 : M.nx - 1, r0, r1 < M.ny ? r1 : M.ny - 1);      // with both halos
        for (uint32_t base = 0; base < S.n_tiles; base += 64) {
            const uint32_t rank = base + lane;
            const bool keep = rank < S.n_tiles && map_box_tile(box, S.tiles[rank], S.tile_w - 1, S.tile_h - 1);
            uint64_t m = __builtin_amdgcn_ballot_w64(keep);
            while (m) {
                const uint32_t j = pop_bit(m);
                list = lane == count ? base + j : list;      // (beyond the last lane: dropped, and the wave walks every tile)
                ++count;
            }
        }
    }
    const bool all = count > kMapListCap;
#else
    const bool all = true;
#endif
    const uint32_t n = all ? S.n_tiles : count;
    auto tiles = [&](uint32_t k) { return all ? k : ((void)chk(k < kMapListCap, k, kMapChkList), map_lane(list, k & (kMapListCap - 1))); };
    auto lookup = [&](bool wanted, uint32_t col, uint32_t row, SurfaceHit& h) { map_surface(S, wanted ? map_lon(M, col) : nan, map_lat(M, row), n, tiles, h, chk); };
    const MapLevel none{0, false};
    const uint32_t rows = r1 - r0;
    auto store = [&](uint32_t r, uint32_t f, uint32_t grey) {
        if (!in) return;
        if (rgba) *reinterpret_cast<uint32_t*>(rgba + (size_t)r * rgba_pitch + 4 * (size_t)c) = map_compose(M, f, grey);
        if (flags) flags[(size_t)r * flags_pitch + c] = (uint8_t)f;
    };

#ifndef TOPO_MAP_RECOMPUTE
    // Pass -1: the east halo (lane j: column c0 + 64 of row r0 + j).  Pass k = 0 .. rows: row r0 + k (k == rows: the south halo);
    // the row before it is finished once its south level is known.  One lookup site for all of them.
    const int32_t first = contours && east ? -1 : 0, last = (int32_t)rows - (contours && r1 < M.ny ? 0 : 1);
    MapLevel halo = none;
    MapPixel pend{none, 0u, 255u};
    auto east_of = [&](const MapLevel& own, uint32_t k) {      // the level right of each lane's, for row r0 + k: the next lane's, the halo's for lane 63
        const uint64_t lv = (uint64_t)own.level, hv = (uint64_t)halo.level;
        const uint32_t lo = map_from_right((uint32_t)lv, map_lane((uint32_t)hv, k)), hi = map_from_right((uint32_t)(lv >> 32), map_lane((uint32_t)(hv >> 32), k));
        return MapLevel{(int64_t)(((uint64_t)hi << 32) | lo), map_from_right(own.terrain ? 1u : 0u, map_lane(halo.terrain ? 1u : 0u, k)) != 0};
    };
    for (int32_t pass = first; pass <= last; ++pass) {
        const bool east_pass = pass < 0;
        const uint32_t k = east_pass ? 0u : (uint32_t)pass;
        SurfaceHit h;
        lookup(east_pass ? lane < rows : in, east_pass ? c0 + 64 : c, east_pass ? r0 + lane : r0 + k, h);
        if (east_pass) {
            halo = map_level(M, h);
            continue;
        }
        if (k > 0) {      // finish row r0 + k - 1
            uint32_t f = pend.flags;
            if (contours) {
                const MapLevel east = east_of(pend.level, k - 1);
                const MapLevel south = r0 + k < M.ny ? map_level(M, h) : none;
                f |= map_contour_bits(M.index_every, pend.level, east) | map_contour_bits(M.index_every, pend.level, south);
            }
            store(r0 + k - 1, f, pend.grey);
        }
        if (k < rows) pend = map_pixel(M, S, h, s_thresh, chk);
    }
    if (last + 1 == (int32_t)rows) {      // no pass below the last row: it has no south neighbour (the grid's last row, or no contours)
        uint32_t f = pend.flags;
        if (contours) f |= map_contour_bits(M.index_every, pend.level, east_of(pend.level, rows - 1));
        store(r1 - 1, f, pend.grey);
    }
#else
    for (uint32_t r = r0; r < r1; ++r) {
        SurfaceHit cur;
        lookup(in, c, r, cur);
        const MapPixel p = map_pixel(M, S, cur, s_thresh, chk);
        uint32_t f = p.flags;
        if (contours) {
            SurfaceHit e, s;
            lookup(in && c + 1 < M.nx, c + 1, r, e);
            lookup(in && r + 1 < M.ny, c, r + 1, s);
            f |= map_contour_bits(M.index_every, p.level, map_level(M, e)) | map_contour_bits(M.index_every, p.level, map_level(M, s));
        }
        store(r, f, p.grey);
    }
#endif
}

}  // namespace
}  // namespace topo
