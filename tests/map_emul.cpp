// map_emul.cpp -- TEST-ONLY g++ build of the product's map rule (topo-renderer_amd/csrc/topo_map.h), run three ways
// (tests/map_emul.py, tests/test_map_cpu.py, tests/test_map_gpu.py):
//   mode 0  as k_map runs it: waves of 64 columns x R rows, each with the tile list its box test keeps, the east halo as a pass of
//           its own, the south level from the row done next, the east level from the next lane
//   mode 1  the same waves over every tile instead of the list
//   mode 2  a plain loop: every pixel and both its neighbours looked up on their own with surface_all (every triangle of every tile)
// The three must produce the same bytes.  The tables the lookup reads are built here on the host with the functions k_ground_tables calls.
#include <cmath>
#include <vector>

#include "../include/topo_hip.h"
#include "../topo-renderer_amd/csrc/topo_map.h"
#include "emul_tiles.h"

using namespace topo;

static_assert(sizeof(topo_map_params) == 88, "topo_map_params");

namespace {

struct Scene {
    std::vector<TileDev> dev;
    std::vector<double> trig;
    LosScene S;
    Scene(const EmulTile* tiles, uint32_t n_tiles, uint32_t tile_w, uint32_t tile_h) {
        const size_t tab = ground_table_doubles(tile_w, tile_h);
        dev.resize(n_tiles);
        trig.assign(tab * n_tiles + 2, 0.0);
        for (uint32_t r = 0; r < n_tiles; ++r) {
            dev[r] = make_dev(tiles[r]);
            fill_trig(dev[r], tile_w, tile_h, trig.data() + tab * r);
        }
        S = LosScene{dev.data(), trig.data(), nullptr, tab * n_tiles, n_tiles, tile_w, tile_h, 0u, 0u};
    }
};

void put(const MapCall& M, uint32_t c, uint32_t r, uint32_t f, uint32_t grey, uint8_t* rgba, uint8_t* flags) {
    const size_t i = (size_t)r * M.nx + c;
    if (rgba) {
        const uint32_t px = map_compose(M, f, grey);
        for (int k = 0; k < 4; ++k) rgba[4 * i + k] = (uint8_t)(px >> (8 * k));
    }
    if (flags) flags[i] = (uint8_t)f;
}

}  // namespace

// stats (may be null): [0] the tiles listed, summed over the waves; [1] the waves; [2] the waves whose list overflowed.  Returns the
// number of index checks that failed.
extern "C" int emul_map(const EmulTile* tiles, uint32_t n_tiles, uint32_t tile_w, uint32_t tile_h, const uint32_t* const* masks, uint32_t mask_words,
                        const topo_map_params* params, int mode, uint32_t rows_per_wave, uint8_t* rgba, uint8_t* flags, uint64_t* stats) {
    Scene scene(tiles, n_tiles, tile_w, tile_h);
    const LosScene& S = scene.S;
    const MapCall M = map_call(*params, masks, mask_words, n_tiles);      // as TerrainRenderer::map_device makes it
    const bool contours = (M.layers & kMapContours) != 0;
    const double nan = std::nan("");
    const MapLevel none{0, false};
    int bad = 0;
    auto chk = [&](bool ok, uint64_t, uint32_t) { if (!ok) ++bad; return ok; };
    float thresh[256];
    for (int i = 0; i < 256; ++i) thresh[i] = bits_f(TOPO_SRGB_THRESH_BITS[i]);
    uint64_t st[3] = {0, 0, 0};

    if (mode == 2) {
        auto plain = [&](bool ok, uint64_t) { if (!ok) ++bad; return ok; };
        auto brute = [&](uint32_t c, uint32_t r, SurfaceHit& h) {
            h = SurfaceHit{0.0, 0.0, 0.0, 0u, 0u, false};
            const double lon = map_lon(M, c), lat = map_lat(M, r);
            if (c >= M.nx || r >= M.ny || !surface_point_valid(lon, lat)) return;
            double u[3];
            surface_direction(lon, lat, u);
            surface_all(S, u, h, plain);
        };
        for (uint32_t r = 0; r < M.ny; ++r)
            for (uint32_t c = 0; c < M.nx; ++c) {
                SurfaceHit h, e, s;
                brute(c, r, h);
                const MapPixel p = map_pixel(M, S, h, thresh, chk);
                uint32_t f = p.flags;
                if (contours) {
                    brute(c + 1, r, e);
                    brute(c, r + 1, s);
                    f |= map_contour_bits(M.index_every, p.level, map_level(M, e)) | map_contour_bits(M.index_every, p.level, map_level(M, s));
                }
                put(M, c, r, f, p.grey, rgba, flags);
            }
        return bad;
    }

    const uint32_t R = rows_per_wave;
    const uint32_t waves_x = M.nx / 64 + (M.nx % 64 != 0), bands = M.ny / R + (M.ny % R != 0);
    for (uint32_t band = 0; band < bands; ++band)
        for (uint32_t wx = 0; wx < waves_x; ++wx) {
            const uint32_t c0 = wx * 64, r0 = band * R, r1 = r0 + R < M.ny ? r0 + R : M.ny, rows = r1 - r0;
            // the wave's tiles
            uint32_t list[kMapListCap], count = 0;
            const bool east = (uint64_t)c0 + 64 < M.nx;      // a column right of the wave (64 bits: c0 + 64 may pass 2^32)
            const MapBox box = map_box(M, c0, east ? c0 + 64 : M.nx - 1, r0, r1 < M.ny ? r1 : M.ny - 1);
            for (uint32_t rank = 0; rank < n_tiles; ++rank)
                if (map_box_tile(box, S.tiles[rank], tile_w - 1, tile_h - 1)) {
                    if (count < kMapListCap) list[count] = rank;
                    ++count;
                }
            const bool all = mode == 1 || count > kMapListCap;
            const uint32_t n = all ? n_tiles : count;
            st[0] += count < kMapListCap ? count : kMapListCap;
            st[1] += 1;
            st[2] += count > kMapListCap;
            auto tile_at = [&](uint32_t k) { return all ? k : (chk(k < kMapListCap, k, kMapChkList) ? list[k & (kMapListCap - 1)] : 0u); };
            auto lookup = [&](bool wanted, uint32_t col, uint32_t row, SurfaceHit& h) { map_surface(S, wanted ? map_lon(M, col) : nan, map_lat(M, row), n, tile_at, h, chk); };
            const int32_t first = contours && east ? -1 : 0, last = (int32_t)rows - (contours && r1 < M.ny ? 0 : 1);
            MapLevel halo[64];
            MapPixel pend[64];
            for (uint32_t lane = 0; lane < 64; ++lane) {
                halo[lane] = none;
                pend[lane] = MapPixel{none, 0u, 255u};
            }
            auto east_of = [&](uint32_t lane, uint32_t k) { return lane < 63 ? pend[lane + 1].level : halo[k]; };
            for (int32_t pass = first; pass <= last; ++pass) {
                const bool east_pass = pass < 0;
                const uint32_t k = east_pass ? 0u : (uint32_t)pass;
                SurfaceHit h[64];
                for (uint32_t lane = 0; lane < 64; ++lane) {
                    const bool in = c0 + lane < M.nx;
                    lookup(east_pass ? lane < rows : in, east_pass ? c0 + 64 : c0 + lane, east_pass ? r0 + lane : r0 + k, h[lane]);
                }
                if (east_pass) {
                    for (uint32_t lane = 0; lane < 64; ++lane) halo[lane] = map_level(M, h[lane]);
                    continue;
                }
                if (k > 0)
                    for (uint32_t lane = 0; lane < 64; ++lane) {
                        uint32_t f = pend[lane].flags;
                        if (contours) {
                            const MapLevel south = r0 + k < M.ny ? map_level(M, h[lane]) : none;
                            f |= map_contour_bits(M.index_every, pend[lane].level, east_of(lane, k - 1)) | map_contour_bits(M.index_every, pend[lane].level, south);
                        }
                        if (c0 + lane < M.nx) put(M, c0 + lane, r0 + k - 1, f, pend[lane].grey, rgba, flags);
                    }
                if (k < rows)
                    for (uint32_t lane = 0; lane < 64; ++lane) pend[lane] = map_pixel(M, S, h[lane], thresh, chk);
            }
            if (last + 1 == (int32_t)rows)
                for (uint32_t lane = 0; lane < 64; ++lane) {
                    uint32_t f = pend[lane].flags;
                    if (contours) f |= map_contour_bits(M.index_every, pend[lane].level, east_of(lane, rows - 1));
                    if (c0 + lane < M.nx) put(M, c0 + lane, r1 - 1, f, pend[lane].grey, rgba, flags);
                }
        }
    if (stats)
        for (int k = 0; k < 3; ++k) stats[k] = st[k];
    return bad;
}

// Is tile `rank` kept by the box test of columns [ca, cb] x rows [ra, rb]?
extern "C" int emul_map_box_tile(const EmulTile* tiles, uint32_t rank, uint32_t tile_w, uint32_t tile_h, const topo_map_params* params, uint32_t ca, uint32_t cb, uint32_t ra,
                                 uint32_t rb) {
    const MapCall M = map_call(*params, nullptr, 0, 1);
    return map_box_tile(map_box(M, ca, cb, ra, rb), make_dev(tiles[rank]), tile_w - 1, tile_h - 1) ? 1 : 0;
}

extern "C" uint32_t emul_map_rows() { return kMapRows; }
extern "C" uint32_t emul_map_blend(uint32_t c, uint32_t s) { return map_blend(c, s); }
extern "C" int64_t emul_map_floor_div(int64_t a, int64_t n) { return map_floor_div(a, n); }
