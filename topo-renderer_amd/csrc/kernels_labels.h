// kernels_labels.h -- peak labels over whole submissions (topo_labels.hip: a translation unit of its own, as topo_rays.hip,
// topo_surface.hip, topo_visibility.hip, topo_skyline.hip and topo_sun.hip, so that the frame path's unit and theirs stay exactly what
// they were).
//
//   k_labels   per image (views_per_image consecutive views), the peaks it shows and the label row of each (topo_labels.h)
//
// It reads the views' matrices (a device table the host fills), the caller's depth images, peaks and widths, and writes only its
// outputs: no atomics; the row occupancy of an image lives in LDS.
#pragma once

#include "kernels_common.h"
#include "topo_labels.h"

namespace topo {
namespace {

// One WAVE per image, P.waves waves to a workgroup (the launcher: as many as fit their grids into 64 KiB of LDS, four at the most).
// The wave clears its grid, then walks the peaks in chunks of 64: each lane finds its peak's candidate (label_candidate's loop, taken
// view by view for the whole wave, the view's matrix in scalar registers), the candidates are ballotted and taken in lane order -- the
// peak order -- and one at a time: peak_x and the width come out of the candidate's lane (readlane), and the span's (row, word) pairs
// are dealt out to the lanes, lane = part * R + row with R = max_rows rounded up to a power of two: a lane tests the words part,
// part + 64 / R, ... of its row against its masks, the ballot of the lanes that met a taken bit folds to the rows that collide, the
// first clear bit is the row, and that row's lanes OR their masks in (distinct words: no lane meets another's).
//
// Only the owning wave touches its grid, so no workgroup barrier stands inside the loop (the one barrier-free exit: a spare wave of
// the last workgroup returns at once).  A candidate's LDS writes are seen by the next candidate's reads because a wave's LDS
// operations are issued and completed in order; the compiler is held to that order by wave_lds_fence() between the write phase and
// the reads that follow -- after the clear, and after every candidate's ORs.
__global__ __launch_bounds__(256) void k_labels(LabelParams P) {
    extern __shared__ uint32_t s_label_grid[];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = wave_first((uint32_t)(threadIdx.x >> 6));
    const uint32_t img = wave_first(blockIdx.x * P.waves + wave);
    if (img >= P.n_images) return;      // (the last workgroup's spare waves)
    const uint32_t Wi = P.views_per_image * P.width, words = label_grid_words(Wi, P.max_rows);
    auto chk = [&](bool ok, uint64_t value) { return TOPO_CHK(P.check, ok, 29u, value); };
    (void)chk;
    uint32_t* const grid = s_label_grid + (size_t)wave * words;
    for (uint32_t j = lane; j < words; j += 64u) grid[j] = 0u;
    wave_lds_fence();

    // lane = part * R + row
    uint32_t R = 1u;
    while (R < P.max_rows) R <<= 1;
    const uint32_t shift = (uint32_t)__builtin_ctz(R), parts = 64u >> shift, row = lane & (R - 1u), part = lane >> shift;
    const uint64_t rows_mask = P.max_rows == 64u ? ~0ull : (1ull << P.max_rows) - 1ull;

    const uint32_t view0 = img * P.views_per_image;
    const float* const projs = P.projs + 16 * (size_t)view0;
    LabelRec* const out = P.labels + (size_t)img * P.cap;
    uint32_t count = 0;      // wave-uniform
    for (uint32_t p0 = 0; p0 < P.n_peaks; p0 += 64u) {
        const uint32_t p = p0 + lane;
        const bool live = p < P.n_peaks;
        float x = 0.0f, y = 0.0f, z = 0.0f, w = 0.0f;
        if (live && chk(3 * (size_t)p + 2 < 3 * (size_t)P.n_peaks, p)) {
            x = P.peaks[3 * (size_t)p];
            y = P.peaks[3 * (size_t)p + 1];
            z = P.peaks[3 * (size_t)p + 2];
            w = P.widths[p];
        }
        // label_candidate, view by view: the lanes still without a view try view v
        bool found = false;
        uint32_t view = 0, x_pos = 0, y_pos = 0;
        for (uint32_t v = 0; v < P.views_per_image; ++v) {
            if (__ballot(live && !found) == 0ull) break;
            float m[16];
            const auto mv = const_space(projs + 16 * (size_t)v);
#pragma unroll
            for (int k = 0; k < 16; ++k) m[k] = mv[k];
            if (live && !found) {
                uint32_t xp = 0, yp = 0;
                float peak_dist = 0.0f;
                if (project_peak(m, x, y, z, (float)P.width, (float)P.height, xp, yp, peak_dist) && xp < P.width && yp < P.height &&
                    chk(view0 + v < P.n_views, view0 + v)) {
                    const float d = *reinterpret_cast<const float*>(P.depth + (size_t)(view0 + v) * P.depth_view_stride + (size_t)yp * P.depth_pitch + (size_t)xp * 4);
                    if (peak_dist - 10.0f < linear_depth(d)) {
                        found = true;
                        view = v;
                        x_pos = xp;
                        y_pos = yp;
                    }
                }
            }
        }
        const uint32_t peak_x = view * P.width + x_pos;
        uint8_t st = kLabelHidden;
        uint64_t todo = __ballot(found);
        while (todo) {
            const int j = (int)pop_bit(todo);
            const uint32_t l = (uint32_t)__builtin_amdgcn_readlane((int32_t)peak_x, j);
            const float wj = wave_lane(w, j);
            if (!label_width_usable(wj)) {
                if (lane == (uint32_t)j) st = kLabelBadWidth;
                continue;
            }
            const uint32_t r = label_right(l, wj, Wi);
            const uint32_t first = row * Wi + l, last = row * Wi + r;      // this lane's row's span (rows >= max_rows: not tested)
            const uint32_t w0 = first >> 5, w1 = last >> 5;
            const uint32_t steps = ((r - l) >> 5) + 2u;      // wave-uniform: no row's span has more words
            bool hit = false;
            if (row < P.max_rows)
                for (uint32_t s = part; s < steps; s += parts) {
                    const uint32_t word = w0 + s;
                    if (word <= w1 && chk(word < words, word)) hit = hit || (grid[word] & label_word_mask(word, first, last)) != 0u;
                }
            uint64_t busy = __ballot(hit);
            for (uint32_t s = 32u; s >= R; s >>= 1) busy |= busy >> s;      // lanes part * R + row -> row
            const uint64_t free_rows = ~busy & rows_mask;
            if (free_rows == 0ull) {
                if (lane == (uint32_t)j) st = kLabelNoRow;
                continue;
            }
            const uint32_t k = (uint32_t)__builtin_ctzll(free_rows);
            if (row == k)
                for (uint32_t s = part; s < steps; s += parts) {
                    const uint32_t word = w0 + s;
                    if (word <= w1 && chk(word < words, word)) grid[word] |= label_word_mask(word, first, last);
                }
            wave_lds_fence();
            if (lane == (uint32_t)j) {
                st = kLabelPlaced;
                if (count < P.cap) out[count] = LabelRec{p, view, k, (float)peak_x, label_y(P.row_height, k), w, (float)peak_x, (float)y_pos};
            }
            ++count;
        }
        if (P.state && live) P.state[(size_t)img * P.n_peaks + p] = st;
    }
    if (lane == 0u) P.counts[img] = count;
}

}  // namespace
}  // namespace topo
