// labels_emul.cpp -- TEST-ONLY g++ build of the product's peak-label rule (topo-renderer_amd/csrc/topo_labels.h): label_candidate over a
// depth array on the host (the projection is the product's project_peak) and labels_image, the serial form of what k_labels does wave
// by wave (tests/labels_emul.py, tests/test_labels_cpu.py).
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../topo-renderer_amd/csrc/topo_labels.h"

using namespace topo;

static_assert(sizeof(LabelRec) == 32, "label records");

// The layout alone: positions already known.  row_out[j]: the row, -1 no row free, -2 unusable width.  Returns the number placed.
extern "C" int emul_label_layout(uint32_t n, const uint32_t* x, const float* widths, uint32_t Wi, float row_height, uint32_t max_rows, int32_t* row_out, LabelRec* out) {
    std::vector<uint32_t> grid(label_grid_words(Wi, max_rows));
    std::vector<uint8_t> state(n);
    std::vector<LabelRec> recs(n);
    // one "view" as wide as the image: the candidate of label j is column x[j]
    const uint32_t placed = labels_image(n, widths, Wi, 1u, row_height, max_rows, n, grid.data(),
                                         [&](uint32_t p, uint32_t& view, uint32_t& x_pos, uint32_t& y_pos) { view = 0; x_pos = x[p]; y_pos = 0; return true; },
                                         recs.data(), state.data());
    for (uint32_t j = 0, k = 0; j < n; ++j) {
        row_out[j] = state[j] == kLabelPlaced ? (int32_t)recs[k].row : state[j] == kLabelNoRow ? -1 : -2;
        if (state[j] == kLabelPlaced) out[k] = recs[k], ++k;
    }
    return (int)placed;
}

// n_views views of width x height, their matrices at projs (16 floats each) and their depth at depth + v * view_stride floats, rows
// pitch floats apart -> image i: labels at labels + i * cap (the first cap), counts[i], state[i * n_peaks + p].
extern "C" void emul_labels(uint32_t n_views, const float* projs, uint32_t width, uint32_t height, const float* depth, size_t view_stride, size_t pitch, uint32_t n_peaks,
                            const float* peaks, const float* widths, uint32_t views_per_image, float row_height, uint32_t max_rows, uint32_t cap, LabelRec* labels,
                            uint32_t* counts, uint8_t* state) {
    std::vector<uint32_t> grid(label_grid_words(views_per_image * width, max_rows));
    for (uint32_t i = 0; i < n_views / views_per_image; ++i) {
        const uint32_t view0 = i * views_per_image;
        auto depth_at = [&](uint32_t v, uint32_t x, uint32_t y) { return depth[(size_t)(view0 + v) * view_stride + (size_t)y * pitch + x]; };
        auto cand = [&](uint32_t p, uint32_t& view, uint32_t& x_pos, uint32_t& y_pos) {
            return label_candidate(projs + 16 * (size_t)view0, views_per_image, peaks[3 * (size_t)p], peaks[3 * (size_t)p + 1], peaks[3 * (size_t)p + 2], width, height,
                                   depth_at, view, x_pos, y_pos);
        };
        counts[i] = labels_image(n_peaks, widths, width, views_per_image, row_height, max_rows, cap, grid.data(), cand, labels + (size_t)i * cap,
                                 state + (size_t)i * n_peaks);
    }
}

extern "C" void emul_label_constants(uint32_t out[8]) {
    out[0] = kLabelHidden; out[1] = kLabelPlaced; out[2] = kLabelNoRow; out[3] = kLabelBadWidth; out[4] = kLabelMaxRows; out[5] = kLabelMaxGridBits;
    out[6] = (uint32_t)sizeof(LabelRec); out[7] = 0;
}
