// topo_rays.hip -- the device translation unit of the ray queries (topo_raycast_*, topo_sunlit_map_device): kernels_rays.h and its
// launchers.  Apart from topo_kernels.hip on purpose: that unit's code comes out as before, whatever is added here.
// Compiled with -ffp-contract=off, as everything.
#include "kernels_rays.h"

namespace topo {

void launch_raycast(const RayParams& p, const LosRay* rays, RayHit* out, uint32_t n, hipStream_t s) {
    if (n == 0) return;
#ifdef TOPO_RAYCAST_LANE
    hipLaunchKernelGGL(k_raycast_lane, dim3(n / 256 + (n % 256 != 0)), dim3(256), 0, s, p, rays, out, n);
#else
    hipLaunchKernelGGL(k_raycast, dim3(n / 4 + (n % 4 != 0)), dim3(256), 0, s, p, rays, out, n);      // a wave per ray: at most 2^30 workgroups
#endif
}

void launch_sunlit_map(const GroundParams& p, const LosScene& scene, const double sun[3], uint8_t* out, size_t view_stride, size_t pitch, hipStream_t s) {
    const uint64_t view_keys = (uint64_t)p.q.W * p.q.H, k0 = p.q.first_view * view_keys, k1 = k0 + p.q.n_views * view_keys;
    if (k1 == k0) return;
    const uint64_t waves = ((k1 + 63) >> 6) - (k0 >> 6);      // one per 64-key segment the views touch; past 2^20 workgroups they stride
    const uint64_t blocks = (waves + 3) / 4;
    hipLaunchKernelGGL(k_sunlit_map, dim3((unsigned)(blocks < (1u << 20) ? blocks : (1u << 20))), dim3(256), 0, s, p, scene, sun[0], sun[1], sun[2], out, view_stride,
                       pitch);
}

}  // namespace topo
