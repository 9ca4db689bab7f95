// topo_surface.hip -- the device translation unit of the surface queries (topo_surface_*, topo_profile_*): kernels_surface.h and
// its launchers.  Apart from topo_kernels.hip and topo_rays.hip on purpose: their code comes out as before, whatever is added here.
// Compiled with -ffp-contract=off, as everything.
#include "kernels_surface.h"

namespace topo {

void launch_surface(const RayParams& p, const double* lonlat, SurfacePoint* out, uint32_t n, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_surface, dim3(n / 256 + (n % 256 != 0)), dim3(256), 0, s, p, reinterpret_cast<const double2*>(lonlat), out, n);
}

// (the caller has checked that the rows' waves number less than 2^32)
void launch_surface_grid(const RayParams& p, double lon0, double lat0, double dlon, double dlat, uint32_t nx, uint32_t ny, float* out, size_t pitch, hipStream_t s) {
    if (nx == 0 || ny == 0) return;
    const uint32_t waves_per_row = nx / 64 + (nx % 64 != 0);
    const uint64_t waves = (uint64_t)waves_per_row * ny;
    hipLaunchKernelGGL(k_surface_grid, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, p, lon0, lat0, dlon, dlat, nx, ny, waves_per_row,
                       reinterpret_cast<uint8_t*>(out), pitch);
}

void launch_profile(const RayParams& p, const LosRay* segs, uint32_t n, uint32_t m, float* samples, size_t stride, ProfileSummary* summary, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_profile, dim3(n / 4 + (n % 4 != 0)), dim3(256), 0, s, p, segs, n, m, reinterpret_cast<uint8_t*>(samples), stride, summary);      // a wave per segment
}

}  // namespace topo
