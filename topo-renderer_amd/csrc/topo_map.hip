// topo_map.hip -- the device translation unit of the map view (topo_map_*): kernels_map.h and its launcher.  Apart from every other
// unit on purpose: their code comes out as before, whatever is added here.  Compiled with -ffp-contract=off, as everything.
#include "kernels_map.h"

namespace topo {

uint32_t map_rows_per_wave() { return kMapRows; }

// (the caller has checked that the grid's waves number less than 2^32; rgba and flags: each null or device memory)
void launch_map(const RayParams& p, const MapCall& m, uint8_t* rgba, size_t rgba_pitch, uint8_t* flags, size_t flags_pitch, hipStream_t s) {
    if (m.nx == 0 || m.ny == 0 || (!rgba && !flags)) return;
    const uint32_t waves_x = m.nx / 64 + (m.nx % 64 != 0), bands = m.ny / kMapRows + (m.ny % kMapRows != 0);
    const uint64_t waves = (uint64_t)waves_x * bands;
    hipLaunchKernelGGL(k_map, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, p, m, waves_x, (uint32_t)waves, rgba, rgba_pitch, flags, flags_pitch);
}

}  // namespace topo
