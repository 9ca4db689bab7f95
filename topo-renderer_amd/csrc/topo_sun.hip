// topo_sun.hip -- the device translation unit of the sun exposure queries (topo_sun_exposure_*): kernels_sun.h and its launchers.
// Apart from the other units on purpose: their code comes out as before, whatever is added here.  Compiled with -ffp-contract=off, as
// everything.
#include "kernels_sun.h"

namespace topo {

static_assert(sizeof(SunDir) == 32, "sun records");

// (the caller has checked that the waves number less than 2^32)
void launch_sun_exposure_grid(const RayParams& p, const SunDir* suns, uint32_t n_suns, double lon0, double lat0, double dlon, double dlat, uint32_t nx, uint32_t ny,
                              uint64_t* lit, uint64_t* shadow, float* exposure, size_t mask_pitch, size_t exposure_pitch, hipStream_t s) {
    if (nx == 0 || ny == 0 || n_suns == 0 || n_suns > kSunMaxSuns) return;
    const uint32_t waves_per_row = nx / 64 + (nx % 64 != 0);
    const uint64_t waves = (uint64_t)waves_per_row * ny;
    hipLaunchKernelGGL(k_sun_exposure_grid, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, p, suns, n_suns, lon0, lat0, dlon, dlat, nx, ny, waves_per_row,
                       SunOut{lit, shadow, exposure}, mask_pitch, exposure_pitch);
}

void launch_sun_exposure_list(const RayParams& p, const SunDir* suns, uint32_t n_suns, const double* lonlat, uint32_t n, uint64_t* lit, uint64_t* shadow, float* exposure,
                              hipStream_t s) {
    if (n == 0 || n_suns == 0 || n_suns > kSunMaxSuns) return;
    const uint32_t waves = n / 64 + (n % 64 != 0);
    hipLaunchKernelGGL(k_sun_exposure_list, dim3((waves + 3) / 4), dim3(256), 0, s, p, suns, n_suns, reinterpret_cast<const double2*>(lonlat), n,
                       SunOut{lit, shadow, exposure});
}

}  // namespace topo
