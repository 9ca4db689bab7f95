// topo_refraction.hip -- the device translation unit of the refracted visibility queries (topo_visibility_refracted_*):
// kernels_refraction.h and its launchers.  Apart from topo_visibility.hip and every other unit on purpose: their code comes out as
// before, whatever is added here.  Compiled with -ffp-contract=off, as everything.
#include "kernels_refraction.h"

namespace topo {

// (the caller has checked k and that the waves number less than 2^32)
void launch_visibility_refracted_grid(const RayParams& p, const VisEye* eyes, uint32_t n_observers, double lon0, double lat0, double dlon, double dlat, uint32_t nx,
                                      uint32_t ny, double target_height, double k, uint8_t* out, size_t layer_stride, size_t pitch, hipStream_t s) {
    if (nx == 0 || ny == 0 || n_observers == 0) return;
    const uint32_t waves_per_row = nx / 64 + (nx % 64 != 0);
    const uint64_t waves = (uint64_t)waves_per_row * ny * n_observers;
    hipLaunchKernelGGL(k_visibility_refracted_grid, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, p, eyes, n_observers, lon0, lat0, dlon, dlat, nx, ny,
                       waves_per_row, target_height, k, out, layer_stride, pitch);
}

void launch_visibility_refracted_list(const RayParams& p, const VisEye* eyes, uint32_t n_observers, const double* lonlat, uint32_t n, double target_height, double k,
                                      uint8_t* out, size_t list_stride, hipStream_t s) {
    if (n == 0 || n_observers == 0) return;
    const uint32_t waves_per_list = n / 64 + (n % 64 != 0);
    const uint64_t waves = (uint64_t)waves_per_list * n_observers;
    hipLaunchKernelGGL(k_visibility_refracted_list, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, p, eyes, n_observers, reinterpret_cast<const double2*>(lonlat),
                       n, waves_per_list, target_height, k, out, list_stride);
}

}  // namespace topo
