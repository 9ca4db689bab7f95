// topo_labels.hip -- the device translation unit of the peak labels (topo_labels_*): kernels_labels.h and its launcher.  Apart from
// the other units on purpose: their code comes out as before, whatever is added here.  Compiled with -ffp-contract=off, as
// everything.
#include "kernels_labels.h"

namespace topo {

static_assert(sizeof(LabelRec) == 32, "label records");

// (the caller has checked the grid's limits: max_rows <= kLabelMaxRows, views_per_image * width * max_rows <= kLabelMaxGridBits)
void launch_labels(LabelParams p, hipStream_t s) {
    if (p.n_images == 0 || p.max_rows == 0 || p.max_rows > kLabelMaxRows || (uint64_t)p.views_per_image * p.width * p.max_rows > kLabelMaxGridBits) return;
    const uint32_t grid_bytes = label_grid_words(p.views_per_image * p.width, p.max_rows) * 4u;      // <= 64 KiB
    const uint32_t fit = 65536u / grid_bytes;
    p.waves = fit >= 4u ? 4u : fit;
    hipLaunchKernelGGL(k_labels, dim3((p.n_images + p.waves - 1) / p.waves), dim3(64u * p.waves), (size_t)grid_bytes * p.waves, s, p);
}

}  // namespace topo
