// TEST-ONLY g++ build of the product's host-side tile prefilter (topo-renderer_amd/csrc/host_math.cpp: tile_prefilter), so that the
// CPU suite can call it without a GPU or the HIP library (tests/test_tile_prefilter_cpu.py).
#include "../topo-renderer_amd/csrc/host_math.hpp"

extern "C" uint32_t shim_tile_prefilter(const topo_uniforms* views, uint32_t n_views, const double* spheres, uint32_t n_tiles, uint16_t* out, uint32_t cap) {
    return topo::tile_prefilter(views, n_views, spheres, n_tiles, out, cap);
}
extern "C" uint32_t shim_tile_sphere_doubles() { return topo::kTileSphereDoubles; }
