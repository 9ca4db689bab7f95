// surface_emul.cpp -- TEST-ONLY g++ build of the product's surface rule and lookup (topo-renderer_amd/csrc/topo_surface.h):
// surface_lookup, the function k_surface / k_surface_grid / k_profile call for every point, surface_all, the same triangle test and
// order over every triangle, and a profile's samples and reduction in the lanes' order of k_profile (tests/surface_emul.py,
// tests/test_surface_cpu.py).  The tables the lookup reads are built here on the host with the functions k_ground_tables calls.
#include <cmath>
#include <vector>

#include "../topo-renderer_amd/csrc/topo_surface.h"
#include "emul_tiles.h"

using namespace topo;

struct EmulSurfaceOut {    // topo_surface_point's fields, the computed ones in f64, plus the winner's rank and triangle
    double height, slope_deg, aspect_deg, w1, w2;
    int32_t kind, tile_lat, tile_lon;
    uint32_t cell_x, cell_y, tri, rank, triangle;
};

struct EmulSummary {       // = topo_profile_summary
    float min_clearance;
    uint32_t min_sample, n_terrain;
    int32_t kind;
};

struct EmulSurfaceScene {
    std::vector<TileDev> dev;
    std::vector<double> trig;
    LosScene S;
    EmulSurfaceScene(const EmulGeoTile* tiles, uint32_t n_tiles, uint32_t tile_w, uint32_t tile_h) {
        const size_t tab = ground_table_doubles(tile_w, tile_h);
        dev.resize(n_tiles);
        trig.assign(tab * n_tiles + 2, 0.0);
        for (uint32_t r = 0; r < n_tiles; ++r) {
            dev[r] = make_dev(tiles[r]);
            fill_trig(dev[r], tile_w, tile_h, trig.data() + tab * r);
        }
        S = LosScene{dev.data(), trig.data(), nullptr, tab * n_tiles, n_tiles, tile_w, tile_h, 0u, 0u};      // (no block tables, no spheres: not read)
    }
};

// mode 0: the lookup; 1: every triangle.  Returns the number of index checks that failed.
extern "C" int emul_surface(const EmulGeoTile* tiles, uint32_t n_tiles, uint32_t tile_w, uint32_t tile_h, const double* lonlat, uint32_t n, int mode,
                            EmulSurfaceOut* out) {
    EmulSurfaceScene scene(tiles, n_tiles, tile_w, tile_h);
    const LosScene& S = scene.S;
    int bad = 0;
    auto chk = [&](bool ok, uint64_t) { if (!ok) ++bad; return ok; };
    const uint32_t hm1 = tile_h - 1;
    for (uint32_t i = 0; i < n; ++i) {
        EmulSurfaceOut o{};
        const double lon = lonlat[2 * (size_t)i], lat = lonlat[2 * (size_t)i + 1];
        if (!surface_point_valid(lon, lat)) {
            o.kind = kSurfaceInvalid;
        } else {
            double u[3];
            surface_direction(lon, lat, u);
            SurfaceHit best;
            if (mode == 0) surface_lookup(S, u, best, chk);
            else surface_all(S, u, best, chk);
            if (best.hit) {
                o.kind = kSurfaceTerrain;
                o.height = best.t;
                surface_slope_aspect(S, best.rank, best.tri, u, o.slope_deg, o.aspect_deg, chk);
                o.w1 = best.u; o.w2 = best.v;
                o.tile_lat = tiles[best.rank].lat; o.tile_lon = tiles[best.rank].lon;
                const uint32_t cell = best.tri >> 1;
                o.cell_x = cell / hm1; o.cell_y = cell - o.cell_x * hm1;
                o.tri = best.tri & 1u; o.rank = best.rank; o.triangle = best.tri;
            }
        }
        out[i] = o;
    }
    return bad;
}

// n segments of m samples each: samples (n x m x (terrain, line), f32) and summaries, reduced as k_profile reduces them (64 partials
// that take every 64th sample, merged pairwise over six exchange steps).  Returns the number of index checks that failed.
extern "C" int emul_profile(const EmulGeoTile* tiles, uint32_t n_tiles, uint32_t tile_w, uint32_t tile_h, const LosRay* segs, uint32_t n, uint32_t m,
                            float* samples, EmulSummary* summary) {
    EmulSurfaceScene scene(tiles, n_tiles, tile_w, tile_h);
    int bad = 0;
    auto chk = [&](bool ok, uint64_t) { if (!ok) ++bad; return ok; };
    for (uint32_t i = 0; i < n; ++i) {
        float* row = samples + 2 * (size_t)i * m;
        if (!surface_segment_valid(segs[i])) {
            for (uint32_t k = 0; k < 2 * m; ++k) row[k] = NAN;
            summary[i] = EmulSummary{0.0f, 0u, 0u, kSurfaceInvalid};
            continue;
        }
        ProfileBest lanes[64];
        for (uint32_t lane = 0; lane < 64; ++lane) {
            lanes[lane] = ProfileBest{0.0f, kProfileNoSample, 0u};
            for (uint32_t k = lane; k < m; k += 64) {
                profile_sample(scene.S, segs[i], k, m, row[2 * k], row[2 * k + 1], chk);
                profile_take(lanes[lane], k, row[2 * k], row[2 * k + 1]);
            }
        }
        for (int s = 32; s; s >>= 1) {
            ProfileBest next[64];
            for (int lane = 0; lane < 64; ++lane) {
                next[lane] = lanes[lane];
                profile_merge(next[lane], lanes[lane ^ s]);
            }
            for (int lane = 0; lane < 64; ++lane) lanes[lane] = next[lane];
        }
        const ProfileBest& b = lanes[0];
        summary[i] = EmulSummary{b.sample == kProfileNoSample ? NAN : b.clearance, b.sample, b.n_terrain, b.n_terrain ? kSurfaceTerrain : kSurfaceNone};
    }
    return bad;
}
