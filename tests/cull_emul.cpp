// cull_emul.cpp -- TEST-ONLY g++ build of the load phase's block bounds (topo-renderer_amd/csrc/topo_cull.h: block_bounds_store, the
// function k_block_tables and k_block_bounds call for every raster block) with the host's f64 sin / cos in the device's place
// (tests/cull_emul.py, tests/test_cull_cpu.py).  The angles are formed as the kernels form them (kernels_load.h: block_lat64,
// block_lon64, the first / last / centre vertex row and column of a block, clipped at the tile's last ones).
#include <cmath>

#include "../topo-renderer_amd/csrc/topo_cull.h"

using namespace topo;

constexpr uint32_t kEmulBCX = 60, kEmulBCY = 15;      // = kBCX, kBCY (topo_kernels.h): the cells of a raster block

static SinCos64 sc(double a) { SinCos64 r; r.s = std::sin(a); r.c = std::cos(a); return r; }

// transform: raster_x, raster_y, model_x, model_y, scale_x, scale_y (the tile's f32 values); minmax: 2 floats per block;
// bounds: 18 doubles per block, laid out as TileDev::block_bounds.  Returns the number of blocks.
extern "C" uint32_t emul_block_bounds(const float transform[6], uint32_t w, uint32_t h, const float* minmax, double* bounds) {
    const uint32_t bxc = (w - 1 + kEmulBCX - 1) / kEmulBCX, byc = (h - 1 + kEmulBCY - 1) / kEmulBCY, n = bxc * byc;
    auto lat = [&](double vy) { return ((vy - (double)transform[1]) * -(double)transform[5] + (double)transform[3]) * 0.017453292519943295; };
    auto lon = [&](double vx) { return ((vx - (double)transform[0]) * (double)transform[4] + (double)transform[2]) * 0.017453292519943295; };
    for (uint32_t blk = 0; blk < n; ++blk) {
        const uint32_t by = blk / bxc, bx = blk - by * bxc;
        const double yy0 = (double)(by * kEmulBCY), xx0 = (double)(bx * kEmulBCX);
        double yy1 = yy0 + (double)kEmulBCY, xx1 = xx0 + (double)kEmulBCX;
        if (yy1 > (double)(h - 1)) yy1 = (double)(h - 1);
        if (xx1 > (double)(w - 1)) xx1 = (double)(w - 1);
        const SinCos64 la[2] = {sc(lat(yy0)), sc(lat(yy1))}, lo[2] = {sc(lon(xx0)), sc(lon(xx1))};
        block_bounds_store(bounds, n, blk, minmax[2 * blk], minmax[2 * blk + 1], lo, la, sc(lon(0.5 * (xx0 + xx1))), sc(lat(0.5 * (yy0 + yy1))));
    }
    return n;
}
