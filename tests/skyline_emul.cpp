// skyline_emul.cpp -- TEST-ONLY g++ build of the product's skyline rule (topo-renderer_amd/csrc/topo_skyline.h): skyline_frame,
// skyline_direction, skyline_cast -- the steps k_skyline takes a wave at a time -- and skyline_all, the same crossing test and order
// over every triangle (tests/skyline_emul.py, tests/test_skyline_cpu.py).  The tables are those of the ray emulation, built on the
// host; the observers are resolved by visibility_observer, as k_visibility_observers resolves them.
#include "../topo-renderer_amd/csrc/topo_skyline.h"
#include "los_emul.cpp"      // EmulScene: the tables the traversal reads

struct EmulSkyOut {        // topo_skyline_sample's fields in f64, plus the winner's rank, triangle, s, z and z / s
    double elevation_deg, range_m, lon_deg, lat_deg, height_m, s, z, ratio;
    int32_t kind, tile_lat, tile_lon;
    uint32_t cell_x, cell_y, tri, edge, rank, triangle, _pad;
};
static_assert(sizeof(EmulSkyOut) == 104, "tests/skyline_emul.py declares the same record");

// n_obs observers x n_az azimuths az0 + k daz -> out[o * n_az + k].  mode 0: the traversal; 1: every triangle (the observers too).
// Returns the number of index checks that failed.
extern "C" int emul_skyline(const EmulGeoTile* tiles, uint32_t n_tiles, uint32_t tile_w, uint32_t tile_h, const VisObserver* obs, uint32_t n_obs, double az0, double daz,
                            uint32_t n_az, double min_range, double max_range, int mode, EmulSkyOut* out) {
    EmulScene scene(tiles, n_tiles, tile_w, tile_h);
    const LosScene& S = scene.S;
    int bad = 0;
    auto chk = [&](bool ok, uint64_t) { if (!ok) ++bad; return ok; };
    const uint32_t hm1 = tile_h - 1;
    for (uint32_t o = 0; o < n_obs; ++o) {
        VisEye eye;
        if (mode == 0) visibility_observer<false>(S, obs[o], eye, chk);
        else visibility_observer<true>(S, obs[o], eye, chk);
        SkyFrame F;
        skyline_frame(eye, F);
        for (uint32_t k = 0; k < n_az; ++k) {
            EmulSkyOut r{};
            r.elevation_deg = NAN;
            r.kind = kSkyNoObserver;
            if (F.usable) {
                SkyDir D;
                skyline_direction(F, skyline_azimuth(az0, daz, k), D);
                SkyBest best;
                if (mode == 0) skyline_cast(S, F, D, min_range, max_range, best, chk);
                else skyline_all(S, F, D, min_range, max_range, best, chk);
                SkyPoint p;
                r.kind = kSkyNone;
                if (best.hit && skyline_point(S, F, D, best, p, chk)) {
                    r.kind = kSkyTerrain;
                    r.elevation_deg = p.elevation_deg; r.range_m = p.range_m; r.lon_deg = p.lon_deg; r.lat_deg = p.lat_deg; r.height_m = p.height_m;
                    r.s = best.s; r.z = best.z; r.ratio = best.ratio;
                    r.tile_lat = tiles[best.rank].lat; r.tile_lon = tiles[best.rank].lon;
                    const uint32_t cell = best.tri >> 1;
                    r.cell_x = cell / hm1; r.cell_y = cell - r.cell_x * hm1;
                    r.tri = best.tri & 1u; r.edge = best.edge; r.rank = best.rank; r.triangle = best.tri;
                }
            }
            out[(size_t)o * n_az + k] = r;
        }
    }
    return bad;
}
