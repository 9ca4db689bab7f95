// topo_cull.h -- the view-independent half of the cull as pure functions (TOPO_HD, as topo_los.h and topo_surface.h): what the load
// phase stores per raster block.  k_block_tables and k_block_bounds call block_bounds_store for every block (kernels_load.h, with
// the device's f64 sin / cos), tests/cull_emul.cpp runs the same expressions on the host for the no-GPU suite
// (tests/test_cull_cpu.py).  The view-dependent half -- the far box and depth bound of phase B of cull_body, kernels_frame.h --
// stays in its kernel: it shares its loop's registers with the lane's list bookkeeping, and a change of its code generation is a
// change of k_cull that wants a measurement of its own.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "topo_math.h"

namespace topo {

struct SinCos64 { double s, c; };

// The view-independent half of the cull for one raster block, in f64: the bounding sphere of the block's patch, the unit
// directions of its four corners, the sagitta of the patch over their flat hull and the sideways bulge of its equator-side edge
// out of it (4 + 12 + 1 + 1 doubles per block, each part contiguous over the blocks).  lo / la: sin/cos of the block's first and
// last longitude / latitude, loc / lac: of its centre.
TOPO_HD void block_bounds_store(double* bounds, uint32_t blocks_per_tile, uint32_t blk, float bmn, float bmx, const SinCos64 lo[2],
                                                   const SinCos64 la[2], const SinCos64& loc, const SinCos64& lac) {
    const double hmin = (double)bmn, hmax = (double)bmx, hmid = 0.5 * (hmin + hmax);
    double* bs = bounds + (size_t)blk * 4;                                              // sphere
    double* bb = bounds + (size_t)blocks_per_tile * 4 + (size_t)blk * 12;               // corner directions
    double u[4][3];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const SinCos64 &o = lo[k & 1], &a = la[k >> 1];
        u[k][0] = a.c * o.c; u[k][1] = a.c * o.s; u[k][2] = a.s;
        bb[3 * k] = u[k][0]; bb[3 * k + 1] = u[k][1]; bb[3 * k + 2] = u[k][2];
    }
    const double Rm = (double)kR0 + hmid;
    const double c[3] = {Rm * lac.c * loc.c, Rm * lac.c * loc.s, Rm * lac.s};
    double r2 = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double dx = Rm * u[k][0] - c[0], dy = Rm * u[k][1] - c[1], dz = Rm * u[k][2] - c[2];
        const double d2 = dx * dx + dy * dy + dz * dz;
        r2 = d2 > r2 ? d2 : r2;
    }
    // every direction of the patch lies within the angular distance of the farthest corner from the centre direction,
    // so the corners' chord distance bounds the sphere; + half the height range + margin
    bs[0] = c[0]; bs[1] = c[1]; bs[2] = c[2];
    bs[3] = sqrt(r2) + 0.5 * (hmax - hmin) + 8.0 + 64.0;
    // How far the curved patch can stick out of the flat-faced hull of its eight slab corners RADIALLY, over the top face: at
    // most the sagitta of the farthest corner's arc, R (1 - cos theta_max).  0.3 .. 0.7 m for a 60 x 15 cell block of a 1200-px
    // tile, hundreds of metres for the blocks of a coarse tile: the occlusion filter pads its slab by this and only takes blocks
    // where it is <= 1 m.  (Sideways is another quantity: the bulge, below.)
    // (1 - cos theta as |u - uc|^2 / 2: the difference of the two unit vectors keeps its digits where 1 - u . uc, a difference of
    // two numbers next to 1, is only good to 1e-16 -- a part in 1e9 of a sliver block's 1e-7)
    double d2max = 0.0;
    const double uc[3] = {lac.c * loc.c, lac.c * loc.s, lac.s};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double dx = u[k][0] - uc[0], dy = u[k][1] - uc[1], dz = u[k][2] - uc[2];
        const double d2 = dx * dx + dy * dy + dz * dz;
        d2max = d2 > d2max ? d2 : d2max;
    }
    const double sagitta = ((double)kR0 + (hmax > 0.0 ? hmax : 0.0) + 2.0) * (0.5 * d2max);
    bounds[(size_t)blocks_per_tile * 16 + blk] = sagitta;
    // The sagitta is radial.  SIDEWAYS the patch leaves the hull through the face along its equator-side parallel: the face is the
    // plane through the Earth's centre and the edge's two end corners, the edge follows the parallel, and its middle lies
    // R |n . m| beyond the plane (n: the plane's unit normal, m: the direction of the parallel's middle) -- about
    // R (dlon^2 / 8) sin lat cos lat, which exceeds the sagitta wherever tan(lat) x the cell aspect does (2.3 m against 0.4 m in the
    // 5x width band at 81 degrees).  The larger of the two parallels' values, at the slab's top radius: the far box's margin takes it.
    double bulge = 0.0;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const double* a = u[2 * k];
        const double* b = u[2 * k + 1];
        const double n[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
        const double nn = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        const double e = fabs(n[0] * la[k].c * loc.c + n[1] * la[k].c * loc.s + n[2] * la[k].s);
        if (nn > 0.0 && e > bulge * nn) bulge = e / nn;
    }
    bounds[(size_t)blocks_per_tile * 17 + blk] = ((double)kR0 + (hmax > 0.0 ? hmax : 0.0) + 2.0 + sagitta) * bulge;
}

}  // namespace topo
