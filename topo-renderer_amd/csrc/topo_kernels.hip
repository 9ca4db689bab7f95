// topo_kernels.hip -- the one device translation unit of the terrain path: gfx950 (CDNA4, wave64) kernels, one file per phase,
// included here in the order the kernels are defined in, and their launchers.
//
//   kernels_common.h    the visibility buffer's key and marks, the bounds-check build, wave helpers
//   kernels_load.h      load phase (once per add_terrain): block tables, sin/cos tables, cull bounds, normals
//   kernels_frame.h     frame phase: view constants, clear, cull, occlusion filter, the raster kernels
//   kernels_resolve.h   k_resolve: shading of each pixel's winner + the post pass
//   kernels_query.h     viewshed, horizon and ground points, over a finished frame's visibility buffer; the unwrap of finished images
//   kernels_overlay.h   pixelise post pass, line / glyph overlays, visible peaks
//   kernels_tiff.h      GeoTIFF rows, unit-test probes
//
// A frame:  [k_put_views ->] k_clear_cull (or k_clear -> k_cull) -> [near] k_raster -> k_raster_rare -> k_raster_cover -> k_raster_big ->
//           [k_occlusion -> [far survivors] k_raster -> k_raster_rare -> k_raster_big ->] k_resolve (one launch or several)
//           [-> k_post_pixelize] [-> k_viewshed]
// A load:   k_trig_tables -> k_normals_rolling<.., true> -> k_block_bounds, or k_block_tables -> k_normals_interior /
//           k_normals_rolling<.., false>; then k_normals_border
//
// One translation unit on purpose: the kernels share force-inlined helpers, and splitting the unit changes the code that comes out.
// Compiled with -ffp-contract=off: results must match the arithmetic spec bit for bit.
#include <algorithm>
#include <atomic>
#include <cstring>

#include "kernels_common.h"
#include "kernels_load.h"
#include "kernels_frame.h"
#include "kernels_resolve.h"
#include "kernels_query.h"
#include "kernels_overlay.h"
#include "kernels_tiff.h"

namespace topo {

// ---- launch helpers --------------------------------------------------------------------------------------

// A launch whose own start / end time an event takes (hipExtLaunchKernel: the dispatch's completion signal carries both, no marker
// packet stands between two kernels); a plain launch when no event is asked for.
template <typename K, typename... Args>
static inline void launch_timed(K kernel, dim3 grid, dim3 block, hipStream_t s, hipEvent_t start, hipEvent_t stop, const Args&... args) {
    if (start || stop) hipExtLaunchKernelGGL(kernel, grid, block, 0, s, start, stop, 0, args...);
    else hipLaunchKernelGGL(kernel, grid, block, 0, s, args...);
}

// the raster-block grid of a w x h tile
struct BlockGrid { uint32_t bxc, byc; };
static inline BlockGrid block_grid(uint32_t w, uint32_t h) { return {(w - 1 + kBCX - 1) / kBCX, (h - 1 + kBCY - 1) / kBCY}; }

// Persistent-style grids: exactly as many workgroups as are resident at once (occupancy x CUs), each wave striding
// over its queue, so there is no partially filled second round of workgroups.
// The size is a property of (kernel, device): cached per device id, so one process can drive several GPUs.
template <int kSite, typename K>
static unsigned resident_grid(K kernel, unsigned fallback) {
    constexpr int kMaxDev = 64;
    static std::atomic<unsigned> cache[kMaxDev];      // 0 = not computed yet; one array per call site (kSite)
    int dev = 0, cus = 0, per_cu = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDev) return fallback;
    if (unsigned g = cache[dev].load(std::memory_order_relaxed)) return g;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) return fallback;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 256, 0) != hipSuccess || per_cu <= 0) return fallback;
    const unsigned g = (unsigned)(cus * per_cu);
    cache[dev].store(g, std::memory_order_relaxed);
    return g;
}

// ---- load phase ------------------------------------------------------------------------------------------

void launch_block_tables(const TileDev* tiles, uint32_t first, uint32_t count, uint32_t w, uint32_t h, hipStream_t s) {
    if (count == 0) return;
    const auto [bxc, byc] = block_grid(w, h);
    const uint32_t runs = (bxc + kTblBlocks - 1) / kTblBlocks * byc;
    hipLaunchKernelGGL(k_block_tables, dim3((runs + 3) / 4, count), dim3(256), 0, s, tiles, first, w, h, bxc, byc);
}

// The load path that reads the DEM once (normals_tables_fused()): sin/cos tables -> normals + block minima / maxima -> f64 bounds.
bool normals_tables_fused(uint32_t w, uint32_t h, int lds_rows) {
    static const bool off = getenv("TOPO_LOAD_FUSED") && atoi(getenv("TOPO_LOAD_FUSED")) == 0;      // experiments: the separate kernels
    return !off && lds_rows == 0 && w >= 4 * kBCX && w % (4 * kBCX) == 0 && h >= 3;
}
void launch_trig_tables(const TileDev* tiles, uint32_t first, uint32_t count, uint32_t w, uint32_t h, hipStream_t s) {
    if (count == 0) return;
    hipLaunchKernelGGL(k_trig_tables, dim3((w + h + 255) / 256, count), dim3(256), 0, s, tiles, first, w, h);
}
void launch_normals_tables(const TileDev* tiles, uint32_t first, uint32_t count, uint32_t w, uint32_t h, hipStream_t s) {
    if (count == 0) return;
    const auto [bxc, byc] = block_grid(w, h);
    const uint32_t pieces = (w / (4 * kBCX)) * ((h + kBCY - 1) / kBCY) * count;
    // rows per wave x waves of the 15-row workgroup (TOPO_FUSED_SHAPE = rows * 10 + waves; a wave's rows are loaded in one round)
    static const int shape = getenv("TOPO_FUSED_SHAPE") ? atoi(getenv("TOPO_FUSED_SHAPE")) : 44;
    const dim3 grid(((pieces + 7) / 8) * 8);
    switch (shape) {
        case 53: hipLaunchKernelGGL((k_normals_rolling<5, 3, true, 5>), grid, dim3(192), 0, s, tiles, first, count, (int)w, (int)h, bxc, byc); break;
        case 35: hipLaunchKernelGGL((k_normals_rolling<3, 5, true, 3>), grid, dim3(320), 0, s, tiles, first, count, (int)w, (int)h, bxc, byc); break;
        case 82: hipLaunchKernelGGL((k_normals_rolling<8, 2, true, 4>), grid, dim3(128), 0, s, tiles, first, count, (int)w, (int)h, bxc, byc); break;
        case 151: hipLaunchKernelGGL((k_normals_rolling<15, 1, true, 5>), grid, dim3(64), 0, s, tiles, first, count, (int)w, (int)h, bxc, byc); break;
        default: hipLaunchKernelGGL((k_normals_rolling<4, 4, true, 4>), grid, dim3(256), 0, s, tiles, first, count, (int)w, (int)h, bxc, byc); break;
    }
}
void launch_block_bounds(const TileDev* tiles, uint32_t first, uint32_t count, uint32_t w, uint32_t h, hipStream_t s) {
    if (count == 0) return;
    const auto [bxc, byc] = block_grid(w, h);
    if (count <= 4) hipLaunchKernelGGL(k_block_bounds<8>, dim3((bxc * byc + 31) / 32, count), dim3(256), 0, s, tiles, first, w, h, bxc, byc);      // latency
    else hipLaunchKernelGGL(k_block_bounds<1>, dim3((bxc * byc + 255) / 256, count), dim3(256), 0, s, tiles, first, w, h, bxc, byc);               // throughput
}

void launch_normals_interior(const TileDev* tiles, uint32_t first, uint32_t count, uint32_t w, uint32_t h, int lds_rows,
                             hipStream_t s) {
    if (count == 0) return;
    const dim3 block(256);
    if (lds_rows == 0 && w % 4 == 0) {      // the register-rolling form: no LDS tile
        // rows per wave x waves per workgroup.  Measured on the c4 load phase (tools/exp_roll.py, ms for K1-K3 of 100 tiles, +-2 %):
        // 4x1 0.211, 4x4 0.217, 8x1 0.222, 8x4 0.223, 16x4 0.238, 48x4 0.242; one row per wave 0.232; the LDS form with 32 rows
        // 0.225-0.233.  Short-lived single-wave workgroups stream best (a plain 16-byte copy of the same bytes: 6.3 TB/s as one
        // load and one store per thread, 5.0-5.3 as a grid-stride loop: tools/calib.hip copy).  TOPO_ROLL_SHAPE = rows * 10 + waves.
        static const int shape = getenv("TOPO_ROLL_SHAPE") ? atoi(getenv("TOPO_ROLL_SHAPE")) : 41;
#define TOPO_ROLL(R, WV) hipLaunchKernelGGL((k_normals_rolling<R, WV, false>), dim3(((((w + 255) / 256) * (((h + (R)-1) / (R) + (WV)-1) / (WV)) * count + 7) / 8) * 8), dim3(64 * (WV)), 0, s, tiles, first, count, (int)w, (int)h, 0u, 0u)
        switch (shape) {
            case 44: TOPO_ROLL(4, 4); break;
            case 81: TOPO_ROLL(8, 1); break;
            case 84: TOPO_ROLL(8, 4); break;
            case 164: TOPO_ROLL(16, 4); break;
            case 484: TOPO_ROLL(48, 4); break;
            default: TOPO_ROLL(4, 1); break;
        }
#undef TOPO_ROLL
        return;
    }
#define TOPO_K1(R)                                                                                                                    \
    hipLaunchKernelGGL(k_normals_interior<R>, dim3(((((w + 127) / 128) * ((h + (R)-1) / (R)) * count + 7) / 8) * 8), block, 0, s, tiles, first, \
                       count, (int)w, (int)h)
    switch (lds_rows) {
        case 4: TOPO_K1(4); break;
        case 8: TOPO_K1(8); break;
        case 16: TOPO_K1(16); break;
        case 64: TOPO_K1(64); break;
        default: TOPO_K1(32); break;
    }
#undef TOPO_K1
}

void launch_normals_border(const TileDev* tiles, const EdgeJob* edges, uint32_t n_edges, const CornerJob* corners, uint32_t n_corners, uint32_t w,
                           uint32_t h, hipStream_t s) {
    const uint32_t chunks = (w + 63) / 64, blocks = chunks * n_edges + (n_corners + 63) / 64;
    if (blocks == 0) return;
    hipLaunchKernelGGL(k_normals_border, dim3(blocks), dim3(64), 0, s, tiles, edges, n_edges, chunks, corners, n_corners, (int)w, (int)h);
}

void launch_clear(const FrameParams& p, uint32_t* zero, hipStream_t s, hipEvent_t start) {
    const size_t n = (size_t)p.n_views * p.W * p.H;
    launch_timed(k_clear, dim3(2048), dim3(256), s, start, nullptr, p.vis, p.dirty, n, p.counters, zero);
}
void launch_put_views(const ViewPack& pack, uint32_t n, ViewDev* dst, hipStream_t s) {
    // (hipExtAnyOrderLaunch, which would let this launch pass under the tail of the frame before, is not honoured on gfx9: measured, no change)
    hipLaunchKernelGGL(k_put_views, dim3(1), dim3(256), 0, s, pack, n * (uint32_t)(sizeof(ViewDev) / 4), (uint32_t*)dst);
}

// The cull's grid and pair list as its two launchers pass them.
namespace {
struct CullGrid {
    unsigned n_blocks;
    uint32_t wgs_per_pair;      // 0: the full grid
    CullPairs list{};
    CullGrid(const FrameParams& p, const uint16_t* pairs, uint32_t n_pairs) {
        const uint32_t blocks_per_tile = p.bx_count * p.by_count;
        if (pairs && n_pairs <= kMaxCullPairs && blocks_per_tile) {
            wgs_per_pair = (blocks_per_tile + 255) / 256;
            n_blocks = n_pairs * wgs_per_pair;
            memcpy(list.code, pairs, n_pairs * sizeof(uint16_t));
        } else {
            wgs_per_pair = 0;
            n_blocks = (unsigned)(((size_t)p.n_views * p.n_tiles * blocks_per_tile + 255) / 256);
        }
    }
};
}  // namespace
size_t cull_workgroups_max(uint32_t n_views, uint32_t n_tiles, uint32_t blocks_per_tile) {
    const size_t pairs = (size_t)n_views * n_tiles;
    return std::max((pairs * blocks_per_tile + 255) / 256, pairs * ((blocks_per_tile + 255) / 256));
}

void launch_clear_cull(const FrameParams& p, uint32_t* zero, hipStream_t s, hipEvent_t start, const ViewPack* pack, uint32_t n_pack_views, const uint16_t* pairs,
                       uint32_t n_pairs) {
    const CullGrid g(p, pairs, n_pairs);
    const unsigned n_clear = 2048;
    static const ViewPack none{};
    const ViewPack& pk = pack ? *pack : none;
    const uint32_t words = pack ? n_pack_views * (uint32_t)(sizeof(ViewDev) / 4) : 0u;
    launch_timed(k_clear_cull, dim3(g.n_blocks + n_clear), dim3(256), s, start, nullptr, p, g.n_blocks, n_clear, zero, pk, words, g.wgs_per_pair, g.list);
}

void launch_cull(const FrameParams& p, hipStream_t s, const uint16_t* pairs, uint32_t n_pairs) {
    const CullGrid g(p, pairs, n_pairs);
    if (g.n_blocks == 0) return;
    hipLaunchKernelGGL(k_cull, dim3(g.n_blocks), dim3(256), 0, s, p, g.wgs_per_pair, g.list);
}

void launch_raster(const FrameParams& p, int phase, hipStream_t s) {
    if (p.n_tiles == 0) return;
    const unsigned grid = resident_grid<0>(k_raster, 256 * 5);
    hipLaunchKernelGGL(k_raster, dim3(grid), dim3(256), 0, s, p, phase);
}

void launch_occlusion(const FrameParams& p, hipStream_t s) {
    if (p.n_tiles == 0) return;
    const unsigned grid = resident_grid<1>(k_occlusion, 256 * 8);
    hipLaunchKernelGGL(k_occlusion, dim3(grid), dim3(256), 0, s, p);
}

void launch_raster_rare(const FrameParams& p, const CoverParams& cover, hipStream_t s) {
    if (p.n_tiles == 0) return;
    hipLaunchKernelGGL(k_raster_rare, dim3(256), dim3(256), 0, s, p, cover);
}

void launch_raster_cover(const FrameParams& p, const CoverParams& cover, hipStream_t s) {
    if (p.n_tiles == 0 || cover.serial == 0 || cover.cap == 0) return;
    hipLaunchKernelGGL(k_raster_cover, dim3(cover.cap), dim3(256), 0, s, p, cover);      // a workgroup per region: most find theirs unclaimed and end
}

void launch_raster_big(const FrameParams& p, const CoverParams& cover, hipStream_t s) {
    if (p.n_tiles == 0) return;
    const unsigned grid = resident_grid<2>(k_raster_big, 256 * 4);
    hipLaunchKernelGGL(k_raster_big, dim3(grid), dim3(256), 0, s, p, cover);
}

void launch_resolve(const FrameParams& p, const OutputParams& o, const CoverParams& cover, hipStream_t s, hipEvent_t start, hipEvent_t stop) {
    const unsigned n_blocks = p.rblock_count;
    if (n_blocks == 0) return;
    // four times the resident workgroups: the hardware then hands out workgroups as others finish, which evens out what the
    // static stride leaves uneven (c3: 0.21 -> 0.16 ms; c4, with 128 blocks per resident workgroup, does not care)
    // (the four instantiations differ by a few instructions: one occupancy query serves them all)
    unsigned resident = 4u * resident_grid<3>(k_resolve<true, false>, 256 * TOPO_RESOLVE_WGS);
    if (const char* e = getenv("TOPO_RESOLVE_GRID")) resident = (unsigned)atoi(e) ? (unsigned)atoi(e) : n_blocks;      // experiments: 0 = one block per workgroup
    const dim3 grid(n_blocks < resident ? n_blocks : resident), block(256);
    const bool bgra = p.bgra && !p.post_off;      // (the render-target image of the pixelise path is always R G B A)
    auto launch = [&](auto kernel) { launch_timed(kernel, grid, block, s, start, stop, p, o, cover); };
    if (!p.linear_target && !bgra) launch(k_resolve<true, false>);
    else if (!p.linear_target) launch(k_resolve<true, true>);
    else if (!bgra) launch(k_resolve<false, false>);
    else launch(k_resolve<false, true>);
}

void launch_viewshed(const FrameParams& p, uint32_t* const* masks, unsigned long long* stats, hipStream_t s) {
    if (p.n_tiles == 0) return;
    const size_t groups = (((size_t)p.n_views * p.W * p.H + 63) / 64 + 63) / 64;      // 64 segments of 64 keys per wave and step
    const unsigned grid = (unsigned)((groups + 3) / 4 < kViewshedStatSlots ? (groups + 3) / 4 : kViewshedStatSlots);
    hipLaunchKernelGGL(k_viewshed, dim3(grid), dim3(256), 0, s, p, masks, stats);
}

void launch_horizon(const HorizonParams& p, hipStream_t s) {
    const uint64_t waves = (uint64_t)((p.W + 63) / 64) * p.n_views;      // one per (view, 64-column group)
    if (waves == 0) return;
    hipLaunchKernelGGL(k_horizon, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, p);
}

void launch_ground_tables(const TileDev* tiles, uint32_t n_tiles, double* trig, uint32_t w, uint32_t h, hipStream_t s) {
    if (n_tiles == 0) return;
    hipLaunchKernelGGL(k_ground_tables, dim3((w + h + 255) / 256, n_tiles), dim3(256), 0, s, tiles, trig, w, h);
}

void launch_ground(const GroundParams& p, const GroundQuery* queries, GroundPoint* out, uint32_t n, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_ground, dim3((n + 255) / 256), dim3(256), 0, s, p, queries, out, n);
}

void launch_ground_map(const GroundParams& p, float* out, size_t view_stride, size_t pitch, hipStream_t s) {
    const uint64_t view_keys = (uint64_t)p.q.W * p.q.H, k0 = p.q.first_view * view_keys, k1 = k0 + p.q.n_views * view_keys;
    if (k1 == k0) return;
    const uint64_t waves = ((k1 + 63) >> 6) - (k0 >> 6);      // one per 64-key segment the views touch; past 2^20 workgroups they stride
    const uint64_t blocks = (waves + 3) / 4;
    hipLaunchKernelGGL(k_ground_map, dim3((unsigned)(blocks < (1u << 20) ? blocks : (1u << 20))), dim3(256), 0, s, p, (uint8_t*)out, view_stride, pitch);
}

void launch_unwrap(const UnwrapParams& p, bool bilinear, hipStream_t s, hipEvent_t start, hipEvent_t stop) {
    UnwrapParams q = p;
    q.blocks_x = (p.out_w + 255) / 256;      // 256 columns x 4 rows per workgroup
    const uint64_t blocks = (uint64_t)q.blocks_x * ((p.out_h + 3) / 4);
    if (blocks == 0 || blocks > 0x7FFFFFFFull) return;      // (the host has refused such sizes)
    if (bilinear) launch_timed(k_unwrap<true>, dim3((unsigned)blocks), dim3(256), s, start, stop, q);
    else launch_timed(k_unwrap<false>, dim3((unsigned)blocks), dim3(256), s, start, stop, q);
}

// the overlay key image of a W x H target, (re-)initialised where the caller's keys are fresh
static void overlay_keys_init(uint64_t* keys, int32_t W, int32_t H, bool keys_fresh, hipStream_t s) {
    const size_t n = (size_t)W * H;
    if (keys_fresh) hipLaunchKernelGGL(k_overlay_init, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, keys, n);
}

void launch_overlay(const OverlayVertex* verts, const uint32_t* idx, uint32_t n_tris, uint32_t n_verts, float width, int32_t W, int32_t H, uint64_t* keys,
                    bool keys_fresh, uint8_t* rgba, size_t pitch, uint32_t linear_target, uint32_t bgra, hipStream_t s) {
    overlay_keys_init(keys, W, H, keys_fresh, s);
    if (n_tris == 0) return;
    hipLaunchKernelGGL(k_overlay_raster, dim3((n_tris + 63) / 64), dim3(64), 0, s, verts, idx, n_tris, n_verts, width, W, H, keys);
    hipLaunchKernelGGL(k_overlay_resolve, dim3((W + 63) / 64, (H + 3) / 4), dim3(256), 0, s, verts, idx, width, W, H, keys, rgba, pitch, linear_target, bgra);
}

void launch_overlay_glyphs(const GlyphInstance* glyphs, uint32_t n_glyphs, float depth, const uint8_t* atlas, uint32_t aw, uint32_t ah, int32_t W, int32_t H,
                           uint64_t* keys, bool keys_fresh, uint8_t* rgba, size_t pitch, uint32_t linear_target, uint32_t bgra, hipStream_t s) {
    overlay_keys_init(keys, W, H, keys_fresh, s);
    if (n_glyphs == 0) return;
    hipLaunchKernelGGL(k_glyph_raster, dim3(n_glyphs), dim3(64), 0, s, glyphs, n_glyphs, depth, W, H, keys);
    hipLaunchKernelGGL(k_glyph_resolve, dim3(n_glyphs), dim3(64), 0, s, glyphs, n_glyphs, depth, atlas, aw, ah, W, H, keys, rgba, pitch, linear_target, bgra);
}

void launch_post_pixelize(uint32_t n_views, int32_t W, int32_t H, float vw, float vh, float pixelize_n, const uint8_t* pre_rgba, const OutputParams& out,
                          const float* depth, size_t depth_view_stride, size_t depth_pitch, uint32_t linear_target, uint32_t bgra, hipStream_t s) {
    hipLaunchKernelGGL(k_post_pixelize, dim3((W + 63) / 64, (H + 3) / 4, n_views), dim3(256), 0, s, W, H, vw, vh, pixelize_n, pre_rgba, out, depth, depth_view_stride,
                       depth_pitch, linear_target, bgra);
}

void launch_visible_peaks(const float* proj16_dev, uint32_t w, uint32_t h, const float* depth, size_t depth_pitch, uint32_t n,
                          const float* peaks_xyz, uint8_t* visible, uint32_t* xy, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_visible_peaks, dim3((n + 255) / 256), dim3(256), 0, s, proj16_dev, w, h, depth, depth_pitch, n, peaks_xyz,
                       visible, xy);
}

void launch_tiff_rows(uint8_t* bytes, const TiffSegDev* segs, const uint32_t* row_seg, uint32_t n_rows, float* out, uint32_t W, uint32_t H,
                      uint32_t predictor, bool big_endian, hipStream_t s) {
    if (n_rows) hipLaunchKernelGGL(k_tiff_rows, dim3(n_rows), dim3(256), 0, s, bytes, segs, row_seg, out, W, H, predictor, big_endian ? 1 : 0);
}

void launch_probe_sincos(const float* x, float* s, float* c, size_t n, hipStream_t st) {
    hipLaunchKernelGGL(k_probe_sincos, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, s, c, n);
}

void launch_probe_div(int kind, const float* x, const float* y, float* out, size_t n, hipStream_t st) {
    hipLaunchKernelGGL(k_probe_div, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, kind, x, y, out, n);
}

}  // namespace topo
