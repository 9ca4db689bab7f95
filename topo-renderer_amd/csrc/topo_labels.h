// topo_labels.h -- peak labels (topo_label_layout, topo_labels_*): which peaks an image shows and the label row each of them gets, so
// that no two labels of a row overlap -- steps 1 and 2 of the reference's labelled panorama (get_visible_labels, render_engine.rs:338-396;
// layout_labels / process_label_layout, text_renderer.rs:300-372), the second restated on an occupancy grid.
//
// Image.  views_per_image consecutive views of width x height, side by side: columns 0 .. Wi - 1, Wi = views_per_image * width.  One
// view is the reference's frame, eight are a panorama strip -- the one image the viewer sees, so labels do not collide across a seam.
//
// Candidate.  For peak p (ECEF f32 xyz) the image's views are taken in ascending order; the first view v in which the peak passes
// k_visible_peaks' test -- project_peak through that view's camera_proj, x_pos < width && y_pos < height, peak_dist - 10 <
// linear_depth(depth[v][y_pos][x_pos]) -- makes it a candidate at peak_x = v * width + x_pos, peak_y = y_pos (label_candidate; the
// projection and the depth are topo_pipeline.h's and topo_math.h's, not restated).
//
// Layout.  Candidates are taken in ascending peak index: the caller's order stands for the reference's BTreeMap iteration and is the
// priority order.  w = widths[p]; a w that is not finite or < 0 is never labelled (kLabelBadWidth; the reference's shaper yields none).
// Else l = peak_x, r = min(sat_u32(ceil((float)peak_x + w)), Wi - 1) (f32 sum and ceil; sat_u32 is Rust's `as u32`), and the label takes
// the LOWEST row k < max_rows in which no column of the closed range [l, r] is taken, and takes those columns in that row; touching
// counts (r of one equal to l of the next collides).  No free row: kLabelNoRow.  label_x = (float)peak_x, label_y = row_height *
// (0.5f + (float)k) -- one f32 add, one f32 multiply --, label_width = w.
//
// Why the grid decides as the reference's sorted edge sets do.  The reference keeps per row a BTreeSet of Left(l) / Right(r) edges,
// Left(p) < Right(p), and calls a row free when (a) no edge lies in [Left(l), Right(r)] and (b) the next edge at or after Right(r) is
// not a Right edge.
//   1  A row holds disjoint closed intervals: a label enters a row only where (a) and (b) held, and 2 and 3 show that is disjointness.
//   2  An edge inside [Left(l), Right(r)] is an endpoint e of an existing interval with l <= e <= r -- Left(l) sorts at or before every
//      edge at l, Right(r) at or after every edge at r -- so (a) fails exactly when an existing interval has an endpoint in [l, r].
//   3  With (a) holding, an existing interval that meets [l, r] has no endpoint in it and so encloses it: l' < l, r < r'.  The intervals
//      being disjoint, the first edge after Right(r) is then that interval's Right(r'): (b) fails.  Conversely a Right edge that is the
//      first after Right(r) has its Left before it, and by (a) not inside [l, r]: before l -- it encloses.  So (a) and (b) hold exactly
//      when no existing interval shares a column with [l, r], which is what the grid tests.
//   4  Every l is < Wi, so clamping r to Wi - 1 keeps every intersection: [l, r] and [l', r'] meet iff max(l, l') <= min(r, r'), the
//      left side is < Wi, and two intervals that both run past the edge both hold column Wi - 1.
//   5  The reference's ninth row is created empty, is never inserted into and so answers None for ever: "no row free".
//
// The grid.  Row k's column c is bit k * Wi + c of one bit string -- rows packed without padding, so max_rows * Wi <= kLabelMaxGridBits
// bits are never more than 64 KiB -- in 32-bit words, bit b of word j standing for bit 32 j + b.  A span is the bits [k * Wi + l,
// k * Wi + r] of row k, met word by word through label_word_mask.
//
// Pure functions (TOPO_HD): k_labels calls them, host_math.cpp's topo_label_layout and tests/labels_emul.cpp run labels_image and
// label_place under g++.
#pragma once

#include "topo_pipeline.h"

namespace topo {

constexpr uint32_t kLabelMaxRows = 64;
constexpr uint32_t kLabelMaxGridBits = 524288;      // max_rows * Wi: 64 KiB of bits
constexpr uint8_t kLabelHidden = 0, kLabelPlaced = 1, kLabelNoRow = 2, kLabelBadWidth = 3;

struct LabelRec {          // = topo_label (32 bytes)
    uint32_t peak, view, row;
    float label_x, label_y, label_width, peak_x, peak_y;
};

// finite and >= 0 (NaN fails both comparisons)
TOPO_HD bool label_width_usable(float w) { return w >= 0.0f && w <= 3.402823466e+38f; }

// Rust's `f32 as u32`: toward zero, saturating, NaN -> 0
TOPO_HD uint32_t label_sat_u32(float v) {
    if (!(v > 0.0f)) return 0u;
    if (v >= 4294967296.0f) return 0xFFFFFFFFu;
    return (uint32_t)v;
}

// the last column of a label at peak_x of a usable width w in an image of Wi columns
TOPO_HD uint32_t label_right(uint32_t peak_x, float w, uint32_t Wi) {
    const uint32_t r = label_sat_u32(__builtin_ceilf((float)peak_x + w));
    return r < Wi - 1u ? r : Wi - 1u;
}

TOPO_HD float label_y(float row_height, uint32_t row) { return row_height * (0.5f + (float)row); }

// the words of the grid: ceil(max_rows * Wi / 32)
TOPO_HD uint32_t label_grid_words(uint32_t Wi, uint32_t max_rows) { return (uint32_t)(((uint64_t)Wi * max_rows + 31u) >> 5); }

// the bits of word `word` that lie in the bit range [first, last] (first <= last; word in [first >> 5, last >> 5])
TOPO_HD uint32_t label_word_mask(uint32_t word, uint32_t first, uint32_t last) {
    const uint32_t lo = word == (first >> 5) ? (first & 31u) : 0u, hi = word == (last >> 5) ? (last & 31u) : 31u;
    return (0xFFFFFFFFu >> (31u - hi)) & (0xFFFFFFFFu << lo);
}

// The lowest row of `grid` (zeroed label_grid_words words at the start of an image) in which [l, r] is free, taken; -1: none.
TOPO_HD int32_t label_place(uint32_t* grid, uint32_t Wi, uint32_t max_rows, uint32_t l, uint32_t r) {
    for (uint32_t k = 0; k < max_rows; ++k) {
        const uint32_t first = k * Wi + l, last = k * Wi + r;
        bool taken = false;
        for (uint32_t j = first >> 5; j <= (last >> 5) && !taken; ++j) taken = (grid[j] & label_word_mask(j, first, last)) != 0u;
        if (taken) continue;
        for (uint32_t j = first >> 5; j <= (last >> 5); ++j) grid[j] |= label_word_mask(j, first, last);
        return (int32_t)k;
    }
    return -1;
}

// The candidate rule for one peak: m = the image's views_per_image matrices (16 floats each, column-major), depth_at(v, x, y) the
// depth of the image's view v at pixel (x, y).  true: the peak shows in view `view` at (x_pos, y_pos) of that view.
template <class Depth>
TOPO_HD bool label_candidate(const float* m, uint32_t views_per_image, float x, float y, float z, uint32_t width, uint32_t height, Depth&& depth_at, uint32_t& view,
                             uint32_t& x_pos, uint32_t& y_pos) {
    for (uint32_t v = 0; v < views_per_image; ++v) {
        float peak_dist = 0.0f;
        if (project_peak(m + 16 * (size_t)v, x, y, z, (float)width, (float)height, x_pos, y_pos, peak_dist) && x_pos < width && y_pos < height &&
            peak_dist - 10.0f < linear_depth(depth_at(v, x_pos, y_pos))) {
            view = v;
            return true;
        }
    }
    return false;
}

// What one image's labels are, given each peak's candidate: cand(p, view, x_pos, y_pos) -> bool.  grid: label_grid_words words, zeroed
// here.  labels: the first `cap` placed, in placement order (nullable); state: n_peaks bytes (nullable).  Returns the number placed.
template <class Candidate>
TOPO_HD uint32_t labels_image(uint32_t n_peaks, const float* widths, uint32_t width, uint32_t views_per_image, float row_height, uint32_t max_rows, uint32_t cap,
                              uint32_t* grid, Candidate&& cand, LabelRec* labels, uint8_t* state) {
    const uint32_t Wi = views_per_image * width, words = label_grid_words(Wi, max_rows);
    for (uint32_t j = 0; j < words; ++j) grid[j] = 0u;
    uint32_t count = 0;
    for (uint32_t p = 0; p < n_peaks; ++p) {
        uint32_t view = 0, x_pos = 0, y_pos = 0;
        uint8_t st = kLabelHidden;
        if (cand(p, view, x_pos, y_pos)) {
            const float w = widths[p];
            const uint32_t peak_x = view * width + x_pos;
            if (!label_width_usable(w)) st = kLabelBadWidth;
            else {
                const int32_t k = label_place(grid, Wi, max_rows, peak_x, label_right(peak_x, w, Wi));
                st = k < 0 ? kLabelNoRow : kLabelPlaced;
                if (k >= 0) {
                    if (labels && count < cap) labels[count] = LabelRec{p, view, (uint32_t)k, (float)peak_x, label_y(row_height, (uint32_t)k), w, (float)peak_x, (float)y_pos};
                    ++count;
                }
            }
        }
        if (state) state[p] = st;
    }
    return count;
}

}  // namespace topo
