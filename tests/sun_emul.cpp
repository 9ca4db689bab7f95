// sun_emul.cpp -- TEST-ONLY g++ build of the product's sun exposure rule (topo-renderer_amd/csrc/topo_sun.h): sun_target, sun_class,
// sun_take and sun_exposure_f32, the functions k_sun_exposure_grid / k_sun_exposure_list call, with the lookup and the traversal
// (mode 0) and over every triangle (mode 1: surface_all and los_cast_all<true>) (tests/sun_emul.py, tests/test_sun_cpu.py).  The
// tables are those of the ray emulation, built on the host.
#include "../topo-renderer_amd/csrc/topo_sun.h"
#include "los_emul.cpp"      // EmulScene: the tables los_cast reads

static_assert(sizeof(SunDir) == 32, "sun records");

// n_suns suns (unit directions) x n targets (lon, lat) -> cls[k * n + i], lit[i], shadow[i], exposure[i].
// Returns the number of index checks that failed.
extern "C" int emul_sun_exposure(const EmulGeoTile* tiles, uint32_t n_tiles, uint32_t tile_w, uint32_t tile_h, const SunDir* suns, uint32_t n_suns, const double* lonlat,
                                 uint32_t n, int mode, uint8_t* cls, uint64_t* lit, uint64_t* shadow, float* exposure) {
    EmulScene scene(tiles, n_tiles, tile_w, tile_h);
    const LosScene& S = scene.S;
    int bad = 0;
    auto chk = [&](bool ok, uint64_t) { if (!ok) ++bad; return ok; };
    for (uint32_t i = 0; i < n; ++i) {
        const double lon = lonlat[2 * (size_t)i], lat = lonlat[2 * (size_t)i + 1];
        SunTarget g;
        if (mode == 0) sun_target<false>(S, lon, lat, g, chk);
        else sun_target<true>(S, lon, lat, g, chk);
        SunSums a{0ull, 0ull, 0.0};
        for (uint32_t k = 0; k < n_suns && k < kSunMaxSuns; ++k) {
            double ns;
            const uint8_t c = mode == 0 ? sun_class<false>(S, g, suns[k].d, ns, chk) : sun_class<true>(S, g, suns[k].d, ns, chk);
            sun_take(a, g, k, c, suns[k].weight, ns);
            cls[(size_t)k * n + i] = c;
        }
        lit[i] = a.lit;
        shadow[i] = a.shadow;
        exposure[i] = sun_exposure_f32(g, a);
    }
    return bad;
}

extern "C" void emul_sun_constants(uint32_t out[8]) {
    out[0] = kSunNone; out[1] = kSunLit; out[2] = kSunAway; out[3] = kSunShadow; out[4] = kSunNight; out[5] = kSunMaxSuns;
    out[6] = (uint32_t)sizeof(SunDir); out[7] = 0;
}
