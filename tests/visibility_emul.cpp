// visibility_emul.cpp -- TEST-ONLY g++ build of the product's visibility rule (topo-renderer_amd/csrc/topo_visibility.h):
// visibility_observer and visibility_class, the functions k_visibility_observers / k_visibility_grid / k_visibility_list call, with
// the lookup and the traversal (mode 0) and over every triangle (mode 1: surface_all and los_cast_all<true>) (tests/visibility_emul.py,
// tests/test_visibility_cpu.py).  The tables are those of the ray emulation, built on the host.
#include "../topo-renderer_amd/csrc/topo_visibility.h"
#include "los_emul.cpp"      // EmulScene: the tables los_cast reads

static_assert(sizeof(VisObserver) == 32 && sizeof(VisEye) == 32, "observer records");

// n_obs observers x n targets (lon, lat) at height h -> out[o * n + i]; eyes: null, or the n_obs resolved observers.
// Returns the number of index checks that failed.
extern "C" int emul_visibility(const EmulGeoTile* tiles, uint32_t n_tiles, uint32_t tile_w, uint32_t tile_h, const VisObserver* obs, uint32_t n_obs, const double* lonlat,
                               uint32_t n, double h, int mode, uint8_t* out, VisEye* eyes) {
    EmulScene scene(tiles, n_tiles, tile_w, tile_h);
    const LosScene& S = scene.S;
    int bad = 0;
    auto chk = [&](bool ok, uint64_t) { if (!ok) ++bad; return ok; };
    for (uint32_t o = 0; o < n_obs; ++o) {
        VisEye eye;
        if (mode == 0) visibility_observer<false>(S, obs[o], eye, chk);
        else visibility_observer<true>(S, obs[o], eye, chk);
        if (eyes) eyes[o] = eye;
        for (uint32_t i = 0; i < n; ++i) {
            const double lon = lonlat[2 * (size_t)i], lat = lonlat[2 * (size_t)i + 1];
            out[(size_t)o * n + i] = mode == 0 ? visibility_class<false>(S, eye, lon, lat, h, chk) : visibility_class<true>(S, eye, lon, lat, h, chk);
        }
    }
    return bad;
}
