// topo_skyline.hip -- the device translation unit of the skyline queries (topo_skyline_*): kernels_skyline.h and its launcher.
// Apart from topo_kernels.hip, topo_rays.hip, topo_surface.hip and topo_visibility.hip on purpose: their code comes out as before,
// whatever is added here.  Compiled with -ffp-contract=off, as everything.
#include "kernels_skyline.h"

namespace topo {

static_assert(sizeof(SkySample) == 64, "skyline record: four 16-byte stores");

// (the caller has checked that the waves number less than 2^32: at most 2^30 workgroups)
void launch_skyline(const RayParams& p, const VisEye* eyes, uint32_t n_observers, double az0, double daz, uint32_t n_az, double min_range, double max_range,
                    const SkyOut& out, hipStream_t s) {
    if (n_observers == 0 || n_az == 0) return;
    const uint64_t waves = (uint64_t)n_observers * n_az;
    hipLaunchKernelGGL(k_skyline, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, p, eyes, n_observers, az0, daz, n_az, min_range, max_range, out);
}

}  // namespace topo
