/* topo_hip_test.h -- TEST HOOKS of libtopo_hip.so.  Not part of the drop-in boundary (include/topo_hip.h): nothing here
 * has a counterpart in the reference, a host application has no use for any of it, and the Rust bindings
 * (rust/topo-hip-sys, generated from topo_hip.h) do not declare it.  The library exports these symbols so that the parity
 * tests (tests/test_gpu_parity.py, through the ctypes binding) can drive the product's own code paths: the queue overflow
 * branches, the device forms of the arithmetic spec, the normal texture as the kernels left it, and the synthetic
 * COP90-shaped tiles of the benchmark. */
#ifndef TOPO_HIP_TEST_H
#define TOPO_HIP_TEST_H

#include "topo_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Test hook: capacities (entries) of the big-triangle and rare-triangle queues; 0 restores the default (4 Mi each,
 * the rare queue growing on demand under topo_render).  Lets the tests drive the overflow paths: a full big queue is
 * handled exactly (slower); a full rare queue of an explicitly set capacity drops triangles and makes the call that waits
 * for the frame fail with TOPO_ERR_CAPACITY.  rare_cap with bit 31 set = "start at (rare_cap & 0x7FFFFFFF) entries and
 * grow on demand", i.e. the default behaviour from a small starting size. */
int topo_debug_set_queue_caps(topo_ctx* ctx, uint32_t big_cap, uint32_t rare_cap);

/* Test accessor: 1 if the last submission launched its far phase (occlusion test + second raster pass), 0 if the host could
 * prove that no block lies beyond the occlusion split (a lone tile around the viewpoint) and left the four launches out.
 * TOPO_FAR_SKIP=0 in the environment always launches it. */
int topo_debug_far_phase_launched(topo_ctx* ctx, int32_t* out);

/* Test hooks of the cull's tile prefilter: the host drops the (view, tile) pairs whose tile lies wholly outside the view's frustum
 * and launches the cull over the rest (TOPO_TILE_PREFILTER=0 in the environment: over every pair, as does on = 0 here, from the next
 * submission on).  topo_debug_cull_pairs: out[0] = pairs the last submission's cull was launched over, out[1] = pairs in all
 * (views x tiles); equal when the prefilter is off or the kept pairs' list does not fit the launch's arguments. */
int topo_debug_set_tile_prefilter(topo_ctx* ctx, int32_t on);
int topo_debug_cull_pairs(topo_ctx* ctx, uint32_t out[2]);

/* Test accessor: the covered regions of the last frame (waits for it).  In the near phase a triangle that covers every pixel of a
 * 64 x 64 px region inside the target may claim the region; k_raster_cover then writes it with plain stores instead of atomics.
 * out[0] = items that covered their region (candidates), out[1] = claims won (one per region at most), out[2] = claims lost (the
 * region was taken: the item went the atomic way).  TOPO_COVER=0 in the environment switches the path off: all three are 0; TOPO_COVER=1 takes it for
 * every submission (by default only submissions of more than 2^25 pixels take it). */
int topo_debug_cover_stats(topo_ctx* ctx, uint32_t out[3]);

/* Test hooks of the owned strips.  k_raster_cover leaves a record for each of the eight 64 x 8 px strips of a region it draws; k_resolve
 * takes a strip whose record is this frame's and all of whose pixels inside the target the region's owner has won straight from that
 * record (no listing of winners, no record pass).  The path follows the covered regions' switch (TOPO_COVER);
 * TOPO_RESOLVE_OWNED=0 in the environment switches it alone off, as does on = 0 here, from the next submission on.
 * topo_debug_owned_strips (waits for the last frame, counts on the host from its keys and the table): out[0] = strips that pass the
 * ownership test, out[1] = strips with a record of this frame (8 per claimed region, fewer where the target's lower edge cuts it).
 * Both 0 when the path is off. */
int topo_debug_set_resolve_owned(topo_ctx* ctx, int32_t on);
int topo_debug_owned_strips(topo_ctx* ctx, uint32_t out[2]);

/* Test accessor: what the last submission's cull and occlusion test decided (waits for it).  Count, then fill: counts_out[0..2] =
 * entries of the near work list, of the far candidates (the sub-lists one behind the other) and of the far survivors; [3], [4] = the
 * frame's far_tested and far_survived counters.  near_out / survivors_out: 2 words per entry (view << 16 | tile rank, block | first
 * cell row << 24 | rows << 28; rows 0 = the whole block); far_out: 5 words per entry (view << 16 | rank, block, x0 | x1 << 16,
 * y0 | y1 << 16, the f32 bits of zmin).  Each list is filled up to its *_room entries; any pointer but counts_out may be null.
 * The lists and the frame's counter set are left alone until the next submission (the counter sets alternate and a frame's clear
 * zeroes the other one; the queries behind a frame only read).  TOPO_ERR_INVALID at a pipeline depth other than 1, and before the
 * first submission (one that failed while it was queued, or was made before the pipeline depth last changed, does not count). */
int topo_debug_read_cull_lists(topo_ctx* ctx, uint32_t* near_out, uint32_t near_room, uint32_t* far_out, uint32_t far_room, uint32_t* survivors_out,
                               uint32_t survivors_room, uint32_t counts_out[5]);

/* Test accessor: what k_viewshed did since accumulation was first enabled or last reset (waits for the frames in flight):
 * out[0] = terrain keys it read, out[1] = mask-word updates left after combining neighbouring lanes, out[2] = atomics issued
 * (updates that set at least one new bit).  All 0 before accumulation was ever enabled. */
int topo_debug_viewshed_stats(topo_ctx* ctx, uint64_t out[3]);

/* Test hook: the band height of the summit calls -- they work through each tile in bands of this many vertex rows, and a small scene
 * crosses several bands only with a small value.  0 restores the default (as many rows as hold at most 2^22 posts).  The results do
 * not depend on it. */
int topo_debug_set_summit_band_rows(topo_ctx* ctx, uint32_t rows);

/* Test accessor: what the last topo_summits_* call of the context counted (waits for the stream): out[0] = posts that passed
 * k_summit_candidates, out[1] = those that also passed k_summit_reject (the summits), summed over the bands. */
int topo_debug_summit_counts(topo_ctx* ctx, uint64_t out[2]);

/* Test accessor: R, the rows a wave of the map kernel owns (csrc/topo_map.h: kMapRows).  The map tests size their grids by it: R and
 * R + 1 rows are the two sides of the south halo. */
uint32_t topo_map_rows_per_wave(void);

/* Test accessor: the tile's Rgba8Unorm normal texture, w*h*4 bytes, host pointer. */
int topo_read_normals(topo_ctx* ctx, int32_t lat_deg, int32_t lon_deg, uint8_t* out);

/* The load-time tables of a tile, read back (unit tests: the two load paths must leave the same tables).  minmax_out: 2 floats per
 * raster block (60 x 15 cells); trig_out: 2 (w + h) floats, the (sin, cos) pairs of the w vertex longitudes, then of the h vertex
 * latitudes; bounds_out: 18 doubles per raster block (4 sphere | 12 corner directions | 1 sagitta | 1 sideways bulge, each part
 * contiguous over the blocks).  Any pointer may be null.  n_blocks_out: the number of raster blocks. */
int topo_read_tile_tables(topo_ctx* ctx, int32_t lat_deg, int32_t lon_deg, float* minmax_out, float* trig_out, double* bounds_out, uint32_t* n_blocks_out);

/* Synthetic COP90-shaped tile for tests and benches (integer-hash fBm): w*h floats. */
void topo_synth_tile(int32_t lat_deg, int32_t lon_deg, uint32_t w, uint32_t h, uint32_t seed, float* out);

/* GPU unit-test probe: the device sin/cos of the arithmetic spec over n host floats. */
int topo_probe_sincos(topo_ctx* ctx, const float* x, float* s, float* c, size_t n);

/* GPU unit-test probe: the device forms of the spec's IEEE divisions over n host floats.  kind 0: x / y (general
 * form, operands inside 2^-96 .. 2^96); kind 1: x / 255; kind 2: x / (0.15f - 0.05f); kind 3: sqrt(x) (y ignored for 1..5);
 * kind 4: the v_fract_f32 instruction; kind 5: the spec's x - floor(x); kinds 6..8: channel kind - 6 of fs_main's mode-0 colour
 * (render_shader.wgsl:75-87,106) for the dither argument p = (x, y) and a shading of 0.25. */
int topo_probe_div(topo_ctx* ctx, int32_t kind, const float* x, const float* y, float* out, size_t n);

#ifdef __cplusplus
}
#endif

#endif /* TOPO_HIP_TEST_H */
