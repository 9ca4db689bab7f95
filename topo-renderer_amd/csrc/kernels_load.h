// kernels_load.h -- load phase: what add_terrain computes once per tile (compute_normals*.wgsl and the frame phase's tables).
//
//   k_block_tables                       block min/max, the f64 cull bounds (block_bounds_store: topo_cull.h) and the per-tile sin/cos tables, reading the DEM
//   k_trig_tables, k_block_bounds<L>     the two halves of k_block_tables that do not read the DEM (the fused load path)
//   k_normals_interior<ROWS>             interior normals through an LDS tile
//   k_normals_rolling<R, WAVES, kTables> interior normals with the rows kept in registers; kTables: the block min/max as well
//   k_normals_border                     seams + corners
//
// Launch order: k_trig_tables -> k_normals_rolling<.., true> -> k_block_bounds where the tile's size allows it (normals_tables_fused():
// the DEM is read once), otherwise k_block_tables -> k_normals_interior or k_normals_rolling<.., false>; then k_normals_border.
#pragma once

#include "kernels_common.h"
#include "topo_cull.h"

namespace topo {
namespace {

__device__ __forceinline__ SinCos64 sincos64(double a) { SinCos64 r; r.s = sin(a); r.c = cos(a); return r; }

// The angles whose f64 sin/cos the bounds take: the latitude of vertex row vy / the longitude of vertex column vx (halves allowed).
__device__ __forceinline__ double block_lat64(const TileDev& t, double vy) { return ((vy - (double)t.raster_y) * -(double)t.scale_y + (double)t.model_y) * 0.017453292519943295; }
__device__ __forceinline__ double block_lon64(const TileDev& t, double vx) { return ((vx - (double)t.raster_x) * (double)t.scale_x + (double)t.model_x) * 0.017453292519943295; }
// entries [start, start + stride, ...) of a tile's sin/cos tables (TileDev::trig_lon, trig_lat)
__device__ __forceinline__ void trig_tables_fill(const TileDev& t, uint32_t w, uint32_t h, uint32_t start, uint32_t stride) {
    for (uint32_t e = start; e < w + h; e += stride) {
        float sn, cs;
        if (e < w) {
            sincos_f(vertex_lon(t, e), sn, cs);
            const_cast<float*>(t.trig_lon)[2 * e] = sn;
            const_cast<float*>(t.trig_lon)[2 * e + 1] = cs;
        } else {
            sincos_f(vertex_lat(t, e - w), sn, cs);
            const_cast<float*>(t.trig_lat)[2 * (e - w)] = sn;
            const_cast<float*>(t.trig_lat)[2 * (e - w) + 1] = cs;
        }
    }
}

// Per-tile tables of the frame phase, for a batch of tiles (blockIdx.y) in ONE launch: min/max height of the (kVX x kVY)
// vertices of every raster block, the view-independent half of the cull (f64: the block's bounding sphere, the unit directions
// of its four corners, the sagitta of its patch), and the tile's sin/cos tables (TileDev::trig_lon / trig_lat).
// One WAVE per run of four horizontally adjacent raster blocks (241 vertex columns x 16 vertex rows): lane i keeps the column
// minima / maxima of columns i, i + 64, i + 128, i + 192 while the rows stream by as coalesced 256-byte reads (the DEM is
// read once, at HBM speed; round 2 launched one 64-thread workgroup per block and tile after tile: 19 us per tile, 0.3 TB/s),
// the 61-column ranges of the four blocks are reduced through a wave-private LDS strip, the fifteen f64 sin/cos pairs the four
// blocks need (three latitudes, twelve longitudes) are evaluated by fifteen lanes at once instead of six per block one after
// the other on lane 0, and lanes 0..3 finish one block each.  Same expressions, same results as the one-block-per-wave form.
constexpr uint32_t kTblBlocks = 4;                                  // raster blocks per wave
constexpr uint32_t kTblCols = kTblBlocks * kBCX + 1;                // 241 vertex columns
static_assert(kTblCols <= 256, "four column slots per lane");
__global__ __launch_bounds__(256) void k_block_tables(const TileDev* __restrict__ tiles, uint32_t first, uint32_t w, uint32_t h, uint32_t bx_count,
                                                      uint32_t by_count) {
    __shared__ float s_mn[4][256], s_mx[4][256];
    __shared__ double s_sc[4][15][2];
    const TileDev& t = tiles[first + blockIdx.y];
    const uint32_t lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t runs_per_row = (bx_count + kTblBlocks - 1) / kTblBlocks, n_runs = runs_per_row * by_count;
    const uint32_t blocks_per_tile = bx_count * by_count;
    const auto heights = TOPO_GLOBAL_F32(t.heights);
    float* const minmax = const_cast<float*>(t.block_minmax);
    double* const bounds = const_cast<double*>(t.block_bounds);
    for (uint32_t run = blockIdx.x * 4 + wave; run < n_runs; run += gridDim.x * 4) {
        const uint32_t by = run / runs_per_row, bx0 = (run - by * runs_per_row) * kTblBlocks;
        const uint32_t nb = min(kTblBlocks, bx_count - bx0);       // blocks of this run
        const uint32_t c0 = bx0 * kBCX, y0 = by * kBCY;
        const uint32_t ncols = min(nb * kBCX + 1, w - c0), nrows = min(kVY, h - y0);
        // ---- column minima / maxima
        float mn[4], mx[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { mn[k] = INFINITY; mx[k] = -INFINITY; }
        if ((w & 3u) == 0u) {
            // rows are 16-byte aligned and c0 = 240 (run) is a multiple of four: lane i reads columns 4 i .. 4 i + 3 in ONE load
            const uint32_t cl = 4 * lane < ncols ? 4 * lane : (ncols - 1) & ~3u;      // (surplus lanes re-read the last vector: it exists, w % 4 == 0)
            for (uint32_t r = 0; r < nrows; ++r) {
                const f32x4_t v = *(const __attribute__((address_space(1))) f32x4_t*)(heights + (size_t)(y0 + r) * w + c0 + cl);
                mn[0] = fminf(mn[0], v.x); mx[0] = fmaxf(mx[0], v.x);
                mn[1] = fminf(mn[1], v.y); mx[1] = fmaxf(mx[1], v.y);
                mn[2] = fminf(mn[2], v.z); mx[2] = fmaxf(mx[2], v.z);
                mn[3] = fminf(mn[3], v.w); mx[3] = fmaxf(mx[3], v.w);
            }
            if (lane < 64) {      // (columns beyond ncols hold copies of real columns of this run or, in its last vector, of the tile's last columns: never read below)
#pragma unroll
                for (uint32_t k = 0; k < 4; ++k) { s_mn[wave][(4 * lane + k) & 255u] = mn[k]; s_mx[wave][(4 * lane + k) & 255u] = mx[k]; }
            }
        } else {
            for (uint32_t r = 0; r < nrows; ++r) {
                const auto row = heights + (size_t)(y0 + r) * w + c0;
                float v[4];
#pragma unroll
                for (uint32_t k = 0; k < 4; ++k) {
                    const uint32_t c = lane + 64 * k;
                    v[k] = row[c < ncols ? c : ncols - 1];      // (unconditional loads; the surplus lanes re-read the last column)
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) { mn[k] = fminf(mn[k], v[k]); mx[k] = fmaxf(mx[k], v[k]); }
            }
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) { s_mn[wave][lane + 64 * k] = mn[k]; s_mx[wave][lane + 64 * k] = mx[k]; }
        }
        // ---- the f64 sin/cos pairs: lanes 0..2 latitudes (y0, y1, centre), lanes 3 + 3 b .. 5 + 3 b longitudes (x0, x1, centre) of block b
        const double yy0 = (double)(by * kBCY);
        double yy1 = yy0 + (double)kBCY;
        if (yy1 > (double)(h - 1)) yy1 = (double)(h - 1);
        if (lane < 3u + 3u * nb) {
            double a;
            if (lane < 3u) {
                const double vy = lane == 0 ? yy0 : (lane == 1 ? yy1 : 0.5 * (yy0 + yy1));
                a = block_lat64(t, vy);
            } else {
                const uint32_t b = (lane - 3u) / 3u, which = (lane - 3u) - 3u * b;
                const double xx0 = (double)((bx0 + b) * kBCX);
                double xx1 = xx0 + (double)kBCX;
                if (xx1 > (double)(w - 1)) xx1 = (double)(w - 1);
                const double vx = which == 0 ? xx0 : (which == 1 ? xx1 : 0.5 * (xx0 + xx1));
                a = block_lon64(t, vx);
            }
            const SinCos64 sc = sincos64(a);
            s_sc[wave][lane][0] = sc.s;
            s_sc[wave][lane][1] = sc.c;
        }
        wave_lds_fence();
        // ---- the blocks' own 61-column ranges
        float bmn = INFINITY, bmx = -INFINITY;     // lane b ends up with block b's
        for (uint32_t b = 0; b < nb; ++b) {
            const uint32_t c = b * kBCX + lane;
            float lo = lane < kVX && c < ncols ? s_mn[wave][c] : INFINITY, hi = lane < kVX && c < ncols ? s_mx[wave][c] : -INFINITY;
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                lo = fminf(lo, __shfl_xor(lo, off));
                hi = fmaxf(hi, __shfl_xor(hi, off));
            }
            if (lane == b) { bmn = lo; bmx = hi; }
        }
        if (lane < nb) {
            const uint32_t blk = by * bx_count + bx0 + lane;
            minmax[2 * blk] = bmn;
            minmax[2 * blk + 1] = bmx;
            const double(*sc)[2] = s_sc[wave];
            const SinCos64 lo[2] = {{sc[3 + 3 * lane][0], sc[3 + 3 * lane][1]}, {sc[4 + 3 * lane][0], sc[4 + 3 * lane][1]}};
            const SinCos64 la[2] = {{sc[0][0], sc[0][1]}, {sc[1][0], sc[1][1]}};
            const SinCos64 loc = {sc[5 + 3 * lane][0], sc[5 + 3 * lane][1]}, lac = {sc[2][0], sc[2][1]};
            block_bounds_store(bounds, blocks_per_tile, blk, bmn, bmx, lo, la, loc, lac);
        }
        wave_lds_fence();      // (the next run rewrites the strips)
    }
    trig_tables_fill(t, w, h, blockIdx.x * 256 + threadIdx.x, gridDim.x * 256);
}

// The two halves of k_block_tables that do not read the DEM, for the load path whose normals pass collects the block minima /
// maxima itself (k_normals_rolling<.., true>): the sin/cos tables BEFORE that pass (it reads cos(latitude) from them), the f64
// bounds AFTER it (one lane per raster block, from the block's min/max).  Same expressions as k_block_tables, same results.
__global__ __launch_bounds__(256) void k_trig_tables(const TileDev* __restrict__ tiles, uint32_t first, uint32_t w, uint32_t h) {
    trig_tables_fill(tiles[first + blockIdx.y], w, h, blockIdx.x * 256 + threadIdx.x, gridDim.x * 256);
}
// kLanes = 8: eight lanes per raster block -- lanes 0..5 of a group evaluate one f64 sin/cos pair each (first / last / centre
// latitude, first / last / centre longitude), lane 0 collects them and finishes the block: a block's six sin/cos calls one after the
// other on one lane are the whole latency of this kernel when a single tile is added (add_terrain: 0.43 -> 0.36 ms per tile).
// kLanes = 1: one lane per block, for a batch of tiles, where the lanes are what counts (100 tiles: 0.239 against 0.251 ms for the
// whole load phase).
template <int kLanes>
__global__ __launch_bounds__(256) void k_block_bounds(const TileDev* __restrict__ tiles, uint32_t first, uint32_t w, uint32_t h, uint32_t bx_count,
                                                      uint32_t by_count) {
    static_assert(kLanes == 1 || kLanes == 8, "");
    const TileDev& t = tiles[first + blockIdx.y];
    const uint32_t sub = kLanes == 8 ? threadIdx.x & 7u : 0u, blocks_per_tile = bx_count * by_count;
    const uint32_t blk_raw = kLanes == 8 ? blockIdx.x * 32 + (threadIdx.x >> 3) : blockIdx.x * 256 + threadIdx.x;
    const uint32_t blk = blk_raw < blocks_per_tile ? blk_raw : blocks_per_tile - 1;      // (surplus lanes redo the last block and store nothing)
    const uint32_t by = blk / bx_count, bx = blk - by * bx_count;
    const double yy0 = (double)(by * kBCY), xx0 = (double)(bx * kBCX);
    double yy1 = yy0 + (double)kBCY, xx1 = xx0 + (double)kBCX;
    if (yy1 > (double)(h - 1)) yy1 = (double)(h - 1);
    if (xx1 > (double)(w - 1)) xx1 = (double)(w - 1);
    SinCos64 g[6];      // latitudes of yy0, yy1, the centre; longitudes of xx0, xx1, the centre
    if (kLanes == 8) {
        // sub 0 1 2: the latitudes; sub 3 4 5: the longitudes (6, 7: idle copies of 5)
        const double vy = sub == 0 ? yy0 : (sub == 1 ? yy1 : 0.5 * (yy0 + yy1)), vx = sub == 3 ? xx0 : (sub == 4 ? xx1 : 0.5 * (xx0 + xx1));
        const SinCos64 mine = sincos64(sub < 3 ? block_lat64(t, vy) : block_lon64(t, vx));
        const int base = (int)((threadIdx.x & 63u) & ~7u);
#pragma unroll
        for (int k = 0; k < 6; ++k) { g[k].s = shfl_f64(mine.s, base + k); g[k].c = shfl_f64(mine.c, base + k); }
    } else {
        g[0] = sincos64(block_lat64(t, yy0)); g[1] = sincos64(block_lat64(t, yy1)); g[2] = sincos64(block_lat64(t, 0.5 * (yy0 + yy1)));
        g[3] = sincos64(block_lon64(t, xx0)); g[4] = sincos64(block_lon64(t, xx1)); g[5] = sincos64(block_lon64(t, 0.5 * (xx0 + xx1)));
    }
    if (sub == 0 && blk_raw < blocks_per_tile) {
        const SinCos64 la[2] = {g[0], g[1]}, lo[2] = {g[3], g[4]};
        block_bounds_store(const_cast<double*>(t.block_bounds), blocks_per_tile, blk, t.block_minmax[2 * blk], t.block_minmax[2 * blk + 1], lo, la, g[5], g[2]);
    }
}

// Workgroups are dealt round-robin over the chip's eight XCDs (each with an L2 of its own), so the workgroups that share an L2
// are L, L + 8, L + 16, ... of the launch order -- and neighbouring pieces of a tile, which re-read each other's halo rows and
// columns, never meet in one.  (Measured on the c4 load phase: FETCH_SIZE 1.54x the DEM for the LDS form, 1.25x for the
// LDS-less one -- exactly their halo ratios: every halo line came over the fabric again.)  This hands each XCD a CONTIGUOUS
// eighth of a launch's pieces instead: piece = (L % 8) * ceil(n / 8) + L / 8.  A speed matter only (nothing depends on
// which XCD runs what); returns false for the slack pieces at the end.
__device__ __forceinline__ bool xcd_contiguous_piece(uint32_t n_pieces, uint32_t& piece) {
    const uint32_t L = blockIdx.x, per_xcd = (n_pieces + 7u) / 8u;
    piece = (L & 7u) * per_xcd + (L >> 3);
    return (L >> 3) < per_xcd && piece < n_pieces;
}

// Interior normals (compute_normals_shader.wgsl:22-51) of a batch of tiles (blockIdx.z).  128 x ROWS output texels per
// 256-thread workgroup, TWO horizontally adjacent texels per lane: the kernel issues as many instructions as it moves
// bytes (one texel per lane: ~90 instructions per 64 texels, 0.21 ms of issue slots beside 0.20 ms of HBM time at c4), and
// everything that is not the stencil's own arithmetic -- addresses, edge tests, LDS traffic, loop control, the staging
// loads -- is paid per lane, not per texel.  The (ROWS+2) x 130 height tile is staged in LDS row by row -- wave w takes
// rows w, w + 4, ...: one coalesced 512-byte read per row (a pair of columns per lane) plus a two-lane read for the halo
// columns -- each texel's four taps then come from LDS; cos(latitude) is evaluated once per row.  The border ring, which
// the shader leaves untouched (:30-33) and which is zero in a freshly created texture, is written as zero here so no
// separate clear is needed; seam/corner passes run afterwards.  ROWS is the LDS tile-size knob
// (topo_set_normals_lds_rows).
// Arithmetic: normal_texel_fast() -- a reciprocal-square-root estimate and a guard band around the 8-bit code boundaries
// -- settles 998 texels in 1000; a wave in which some lane's texel falls inside the guard band (or is not finite)
// evaluates the full chain (correctly rounded sqrt, three IEEE divisions) for those lanes.  Same bytes either way.
template <int ROWS>
__global__ __launch_bounds__(256) void k_normals_interior(const TileDev* __restrict__ tiles, uint32_t first, uint32_t n_tiles, int W, int H) {
    // column c of the tile (c = -1 .. 128) lives at index c + 2: a lane's pair (2 tx, 2 tx + 1) at the even index 2 tx + 2
    __shared__ __attribute__((aligned(16))) float tile[ROWS + 2][132];
    __shared__ float s_ys[ROWS];
    // pieces = (tile, row band, column block), column block fastest; handed out XCD by XCD (xcd_contiguous_piece)
    const uint32_t gx = ((uint32_t)W + 127u) / 128u, gy = ((uint32_t)H + ROWS - 1u) / ROWS;
    uint32_t piece;
    if (!xcd_contiguous_piece(gx * gy * n_tiles, piece)) return;      // (workgroup-uniform: before any barrier)
    const uint32_t bz = piece / (gx * gy), by_ = (piece - bz * gx * gy) / gx, bx_ = piece - bz * gx * gy - by_ * gx;
    const TileDev& t = tiles[first + bz];
    const auto heights = TOPO_GLOBAL_F32(t.heights);          // global, not flat, memory operations
    const auto normals = TOPO_GLOBAL_U32_RW(t.normals);
    const int x0 = (int)bx_ * 128, y0 = (int)by_ * ROWS;
    const int tx = threadIdx.x & 63, wy = threadIdx.x >> 6;
    const int gx0 = x0 + 2 * tx;                              // the lane's first column (the second: gx0 + 1)
    {
        // Every load is unconditional (clamped address, value discarded where it does not apply) and all of a wave's loads
        // are issued before the first LDS write: a branch around a load makes the compiler wait for it before going on, one
        // trip to memory per row.  The pair is read from columns (px, px + 1) with px clamped to W - 2, so that both exist.
        constexpr int kIter = (ROWS + 2 + 3) / 4;
        const int px = gx0 > W - 2 ? W - 2 : gx0;
        const int hx = x0 - 1 + 129 * (tx & 1);               // lanes 0 / 1: columns -1 / 128
        const int chx = hx < 0 ? 0 : (hx > W - 1 ? W - 1 : hx);
        f32x2_a4 a[kIter];
        float b[kIter];
#pragma unroll
        for (int k = 0; k < kIter; ++k) {
            const int gy = y0 + wy + 4 * k - 1;
            const int cy = gy < 0 ? 0 : (gy > H - 1 ? H - 1 : gy);
            a[k] = *(const __attribute__((address_space(1))) f32x2_a4*)(heights + ((size_t)cy * W + px));
            b[k] = heights[(size_t)cy * W + chx];
        }
#pragma unroll
        for (int k = 0; k < kIter; ++k) {
            const int ly = wy + 4 * k, gy = y0 + ly - 1;
            const bool row_in = gy >= 0 && gy < H;
            if (ly < ROWS + 2) {
                // (gx0 == W - 1: the tile's last column is the second element of the clamped pair)
                const float v0 = !row_in || gx0 > W - 1 ? 0.0f : (gx0 == W - 1 ? a[k].y : a[k].x);
                const float v1 = row_in && gx0 + 1 <= W - 1 ? a[k].y : 0.0f;
                *reinterpret_cast<float2*>(&tile[ly][2 * tx + 2]) = make_float2(v0, v1);
                if (tx < 2) tile[ly][1 + 129 * tx] = row_in && hx >= 0 && hx < W ? b[k] : 0.0f;
            }
        }
    }
    if (threadIdx.x < ROWS) {
        const float latitude = ((float)(y0 + (int)threadIdx.x) - t.raster_y) * -t.scale_y + t.model_y;
        s_ys[threadIdx.x] = deg2rad(t.scale_y) * kR0 * cos_f(deg2rad(latitude));
    }
    __syncthreads();
    const float xs = deg2rad(t.scale_x) * kR0;
    const bool col_in0 = gx0 >= 1 && gx0 < W - 1, col_in1 = gx0 + 1 < W - 1;      // (gx0 + 1 >= 1 always)
    auto out = normals + ((size_t)(y0 + wy) * W + (gx0 < W ? gx0 : 0));
    const size_t out_step = (size_t)4 * W;
#pragma unroll
    for (int r = wy; r < ROWS; r += 4, out += out_step) {
        const int gy = y0 + r;
        if (gy >= H) break;      // (wave-uniform)
        const bool row_in = gy >= 1 && gy < H - 1;
        const float2 top = *reinterpret_cast<const float2*>(&tile[r][2 * tx + 2]), bot = *reinterpret_cast<const float2*>(&tile[r + 2][2 * tx + 2]);
        const float2 mid = *reinterpret_cast<const float2*>(&tile[r + 1][2 * tx + 2]);      // the pair's own heights: each is the other's neighbour
        const float hl = tile[r + 1][2 * tx + 1], hr = tile[r + 1][2 * tx + 4], ys = s_ys[r];
        uint32_t t0 = 0, t1 = 0;
        const bool in0 = col_in0 && row_in, in1 = col_in1 && row_in;
        const bool settled0 = normal_texel_fast(xs, ys, top.x, hl, mid.y, bot.x, t0) || !in0;
        const bool settled1 = normal_texel_fast(xs, ys, top.y, mid.x, hr, bot.y, t1) || !in1;
        if (!settled0) t0 = normal_texel(xs, ys, top.x, hl, mid.y, bot.x);      // the guard band and non-finite heights: the full chain
        if (!settled1) t1 = normal_texel(xs, ys, top.y, mid.x, hr, bot.y);
        t0 = in0 ? t0 : 0u;
        t1 = in1 ? t1 : 0u;
        if (gx0 + 1 < W) {
            u32x2_a4 v;
            v.x = t0; v.y = t1;
            // (non-temporal: the texture is written once here and read much later -- 0.246 -> 0.235 ms at c4)
            __builtin_nontemporal_store(v, (__attribute__((address_space(1))) u32x2_a4*)(out));
        } else if (gx0 < W) {
            *out = t0;
        }
    }
}

// The same pass WITHOUT an LDS tile (topo_set_normals_lds_rows(0); needs a tile width that is a multiple of four): a wave owns
// a strip of 256 columns -- FOUR adjacent texels per lane, one 16-byte load and one 16-byte store per lane and row -- and
// walks kRollRows rows of it top to bottom with the rows above and below the current one kept in registers (each height is
// loaded once per strip and chunk; the chunk's first and last rows twice), the next four rows always in flight.  The texel
// left of a lane's first and right of its last come from the neighbouring lanes by DPP wave shifts; the two columns beside
// the strip by one extra two-address load per row.  No barrier, no LDS traffic, 1 KiB per wave and memory instruction.
// cos(latitude) of a row is the tile's trig_lat table entry (k_block_tables: the same function of the same input).
// kTables: the pass also collects the min / max height of every raster block (TileDev::block_minmax) -- the one thing
// k_block_tables reads the DEM for -- so that the load phase reads the DEM ONCE.  A strip is then 240 columns (four raster
// blocks of kBCX = 60 cells; lanes 60..63 only feed lane 59's right neighbour) and a workgroup's waves share one block row
// (kBCY = 15 rows: 4 + 4 + 4 + 3): a lane folds its four columns and its right neighbour's first one into one running minimum
// and maximum per row (lanes 15 b .. 15 b + 14 then hold exactly the 61 vertex columns of block b), a wave adds the row below
// its last one (the block's 16th vertex row for the last wave, a row of the same block for the others), the fifteen lanes of a
// block are folded by four shuffles (1, 2, 4, 7: the windows overlap, which a minimum does not mind), the waves' partial
// results meet in LDS.  Needs W % 240 == 0 (COP90: 1200, COP30: 3600); k_trig_tables runs before, k_block_bounds after.
template <int kRollRows, int kWaves, bool kTables, int kBatch = 4>      // kBatch: rows loaded per round
__global__ __launch_bounds__(64 * kWaves) void k_normals_rolling(const TileDev* __restrict__ tiles, uint32_t first, uint32_t n_tiles, int W, int H,
                                                                 uint32_t bx_count, uint32_t by_count) {
    constexpr int kCols = kTables ? 4 * (int)kBCX : 256;                      // columns of a strip
    constexpr int kChunkRows = kTables ? (int)kBCY : kRollRows * kWaves;      // rows of a workgroup
    static_assert(!kTables || (kRollRows * kWaves >= (int)kBCY && kRollRows * (kWaves - 1) < (int)kBCY), "the waves of a workgroup cover one block row");
    __shared__ float s_part[kTables ? kWaves : 1][4][2];
    const uint32_t gx = ((uint32_t)W + kCols - 1u) / kCols, gy = ((uint32_t)H + kChunkRows - 1u) / kChunkRows;
    uint32_t piece;
    if (!xcd_contiguous_piece(gx * gy * n_tiles, piece)) return;      // (workgroup-uniform: before any barrier)
    const uint32_t bz = piece / (gx * gy), by_ = (piece - bz * gx * gy) / gx, bx_ = piece - bz * gx * gy - by_ * gx;
    const TileDev& t = tiles[first + bz];
    const auto heights = TOPO_GLOBAL_F32(t.heights);
    const auto normals = TOPO_GLOBAL_U32_RW(t.normals);
    // (the table was written by an earlier launch and a row's entry is wave-uniform: const_space.  As a vector load it was the
    // youngest memory operation of its row, and waiting for it -- s_waitcnt vmcnt(0) -- waited for every row in flight and for the
    // previous row's store as well.)
    const auto trig_lat = const_space(t.trig_lat);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int x0 = (int)bx_ * kCols, c0 = x0 + 4 * lane;
    const int y0 = (int)by_ * kChunkRows + wave * kRollRows;
    const int y_end = ((int)by_ + 1) * kChunkRows < H ? ((int)by_ + 1) * kChunkRows : H;
    if (!kTables && y0 >= H) return;
    const int y1 = y0 + kRollRows < y_end ? y0 + kRollRows : y_end;      // rows [y0, y1)   (kTables: possibly none)
    const bool col_active = c0 < W && c0 < x0 + kCols;            // (W % 4 == 0: a lane's four columns are all inside or all outside)
    const int cc = c0 < W ? c0 : W - 4;
    // the two columns beside the strip, one load for both: lanes 0..31 the left one, lanes 32..63 the right one (clamped)
    const int ce = lane < 32 ? (x0 > 0 ? x0 - 1 : 0) : (x0 + 256 < W ? x0 + 256 : W - 1);
    auto row_ptr = [&](int y) { return heights + (size_t)(y < 0 ? 0 : (y > H - 1 ? H - 1 : y)) * W; };
    auto load4 = [&](int y) { return *(const __attribute__((address_space(1))) f32x4_t*)(row_ptr(y) + cc); };
    auto load_edge = [&](int y) { return row_ptr(y)[ce]; };
    const float xs = deg2rad(t.scale_x) * kR0, ys0 = deg2rad(t.scale_y) * kR0;
    float mn = INFINITY, mx = -INFINITY;      // kTables: the lane's columns 4 lane .. 4 lane + 4 over the wave's rows
    if (!kTables || y0 < y1) {
        // rows y - 1 and y of the first output row, then four new rows per round
        f32x4_t above = load4(y0 - 1), mid = load4(y0);
        float mid_edge = load_edge(y0);
        f32x4_t nx[kBatch];
        float ne[kBatch];
#pragma unroll
        for (int k = 0; k < kBatch; ++k) { nx[k] = load4(y0 + 1 + k); ne[k] = load_edge(y0 + 1 + k); }
        auto out = normals + ((size_t)y0 * W + cc);
        for (int y = y0; y < y1; y += kBatch) {
            f32x4_t cur[kBatch];
            float ce4[kBatch];
#pragma unroll
            for (int k = 0; k < kBatch; ++k) { cur[k] = nx[k]; ce4[k] = ne[k]; }
            if (y + kBatch < y1) {      // (wave-uniform) the next round's rows: in flight under this round's arithmetic
#pragma unroll
                for (int k = 0; k < kBatch; ++k) { nx[k] = load4(y + kBatch + 1 + k); ne[k] = load_edge(y + kBatch + 1 + k); }
            }
            float cos_lat[kBatch];      // (all of a round's scalar loads up front)
#pragma unroll
            for (int k = 0; k < kBatch; ++k) cos_lat[k] = trig_lat[2 * (y + k < H ? y + k : H - 1) + 1];
#pragma unroll
            for (int k = 0; k < kBatch; ++k) {
                const int gy = y + k;
                if (gy >= y1) break;      // (wave-uniform)
                const f32x4_t below = cur[k];
                const float ys = ys0 * cos_lat[k];
                const float left_edge = wave_lane(mid_edge, 0), right_edge = wave_lane(mid_edge, 63);
                const float hl = wave_from_left(mid.w, left_edge), hr = wave_from_right(mid.x, right_edge);
                if (kTables) {
                    mn = fminf(fminf(fminf(mn, mid.x), fminf(mid.y, mid.z)), fminf(mid.w, hr));
                    mx = fmaxf(fmaxf(fmaxf(mx, mid.x), fmaxf(mid.y, mid.z)), fmaxf(mid.w, hr));
                }
                const bool row_in = gy >= 1 && gy < H - 1;
                const float hL[4] = {hl, mid.x, mid.y, mid.z}, hR[4] = {mid.y, mid.z, mid.w, hr};
                const float hT[4] = {above.x, above.y, above.z, above.w}, hB[4] = {below.x, below.y, below.z, below.w};
                uint32_t tex[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int gx = c0 + q;
                    const bool in = row_in && gx >= 1 && gx < W - 1;
                    uint32_t v = 0;
                    const bool settled = normal_texel_fast(xs, ys, hT[q], hL[q], hR[q], hB[q], v) || !in;
                    if (!settled) v = normal_texel(xs, ys, hT[q], hL[q], hR[q], hB[q]);      // the guard band and non-finite heights: the full chain
                    tex[q] = in ? v : 0u;
                }
                if (col_active) {
                    u32x4_t o;
                    o.x = tex[0]; o.y = tex[1]; o.z = tex[2]; o.w = tex[3];
                    __builtin_nontemporal_store(o, (__attribute__((address_space(1))) u32x4_t*)(out));
                }
                out += W;
                above = mid;
                mid = below;
                mid_edge = ce4[k];
            }
        }
        if (kTables) {      // the row below the wave's last one (row H - 1 again at the tile's end: the loads clamp)
            const float hr = wave_from_right(mid.x, wave_lane(mid_edge, 63));
            mn = fminf(fminf(fminf(mn, mid.x), fminf(mid.y, mid.z)), fminf(mid.w, hr));
            mx = fmaxf(fmaxf(fmaxf(mx, mid.x), fmaxf(mid.y, mid.z)), fmaxf(mid.w, hr));
        }
    }
    if (kTables) {
        // lane 15 b: the minimum / maximum over lanes 15 b .. 15 b + 14 (the last window ends at lane 59)
#pragma unroll
        for (int sh = 1; sh <= 4; sh <<= 1) { mn = fminf(mn, __shfl_down(mn, sh)); mx = fmaxf(mx, __shfl_down(mx, sh)); }
        mn = fminf(mn, __shfl_down(mn, 7));
        mx = fmaxf(mx, __shfl_down(mx, 7));
        if (lane < 60 && lane % 15 == 0) { s_part[wave][lane / 15][0] = mn; s_part[wave][lane / 15][1] = mx; }
        __syncthreads();
        if (threadIdx.x < 4u && by_ < by_count && 4u * bx_ + threadIdx.x < bx_count) {
            float lo = s_part[0][threadIdx.x][0], hi = s_part[0][threadIdx.x][1];
#pragma unroll
            for (int w2 = 1; w2 < kWaves; ++w2) { lo = fminf(lo, s_part[w2][threadIdx.x][0]); hi = fmaxf(hi, s_part[w2][threadIdx.x][1]); }
            float* const minmax = const_cast<float*>(t.block_minmax);
            const uint32_t blk = by_ * bx_count + 4u * bx_ + threadIdx.x;
            minmax[2 * blk] = lo;
            minmax[2 * blk + 1] = hi;
        }
    }
}

// Seam normals (compute_normals_edge_shader.wgsl:25-105): 64 texels (piece `block_x`) of seam job `job_index`.
__device__ __forceinline__ void normals_edge_body(const TileDev* __restrict__ tiles, const EdgeJob* __restrict__ jobs, int W, int H, uint32_t block_x,
                                                  uint32_t job_index) {
    const EdgeJob job = jobs[job_index];
    const TileDev &lt = tiles[job.lt], &rb = tiles[job.rb], &u = tiles[job.uni];
    const auto h_lt = TOPO_GLOBAL_F32(lt.heights);
    const auto h_rb = TOPO_GLOBAL_F32(rb.heights);
    const auto n_lt = TOPO_GLOBAL_U32_RW(lt.normals);
    const auto n_rb = TOPO_GLOBAL_U32_RW(rb.normals);
    const float raster_y = u.raster_y, model_y = u.model_y, scale_x = u.scale_x, scale_y = u.scale_y;
    const int id = (int)block_x * 64 + (int)threadIdx.x;
    if (id < 1 || id >= W - 1) return;
    const float xs = deg2rad(fabsf(scale_x)) * kR0;
    const float ys0 = deg2rad(fabsf(scale_y)) * kR0;
    if (!job.top_bottom) {
        if (id >= H - 1) return;   // the guard uses dimensions.x although id runs along y; see DESIGN.md
        const float latitude = ((float)id - raster_y) * -scale_y + model_y;
        const float ys = ys0 * cos_f(deg2rad(latitude));
        const int lx = W - 1, ly = id, rx = 0, ry = id;
        const float hT = h_lt[(size_t)(ly - 1) * W + lx], hL = h_lt[(size_t)ly * W + lx - 1];
        const float hR = h_rb[(size_t)ry * W + rx + 1], hB = h_lt[(size_t)(ly + 1) * W + lx];
        const uint32_t texel = normal_texel(xs, ys, hT, hL, hR, hB);
        n_lt[(size_t)ly * W + lx] = texel;
        n_rb[(size_t)ry * W + rx] = texel;
    } else {
        const float latitude = ((float)(H - 1) - raster_y) * -scale_y + model_y;
        const float ys = ys0 * cos_f(deg2rad(latitude));
        const int tx = id, ty = H - 1, bx = id, by = 0;
        const float hT = h_lt[(size_t)(ty - 1) * W + tx], hL = h_lt[(size_t)ty * W + tx - 1];
        const float hR = h_lt[(size_t)ty * W + tx + 1], hB = h_rb[(size_t)(by + 1) * W + bx];
        const uint32_t texel = normal_texel(xs, ys, hT, hL, hR, hB);
        n_lt[(size_t)ty * W + tx] = texel;
        n_rb[(size_t)by * W + bx] = texel;
    }
}

// Shared corner of a 2x2 block (compute_normals_corner_shader.wgsl:29-63), one job per lane; `top` comes from
// the bottom-right tile at (0, H-2) exactly as the shader reads it (:49).
__device__ __forceinline__ void normals_corner_body(const TileDev* __restrict__ tiles, const CornerJob* __restrict__ jobs, uint32_t n_jobs, int W, int H,
                                                    uint32_t block) {
    const uint32_t j = block * 64 + threadIdx.x;
    if (j >= n_jobs) return;
    const CornerJob job = jobs[j];
    const TileDev &lt = tiles[job.lt], &rt = tiles[job.rt], &lb = tiles[job.lb], &rb = tiles[job.rb], &u = tiles[job.uni];
    const float latitude = ((float)(H - 1) - u.raster_y) * -u.scale_y + u.model_y;
    const float xs = deg2rad(fabsf(u.scale_x)) * kR0;
    const float ys = deg2rad(fabsf(u.scale_y)) * kR0 * cos_f(deg2rad(latitude));
    const float hT = TOPO_GLOBAL_F32(rb.heights)[(size_t)(H - 2) * W + 0];
    const float hL = TOPO_GLOBAL_F32(lt.heights)[(size_t)(H - 1) * W + (W - 2)];
    const float hR = TOPO_GLOBAL_F32(rt.heights)[(size_t)(H - 1) * W + 1];
    const float hB = TOPO_GLOBAL_F32(lb.heights)[(size_t)1 * W + (W - 1)];
    const uint32_t texel = normal_texel(xs, ys, hT, hL, hR, hB);
    TOPO_GLOBAL_U32_RW(lt.normals)[(size_t)(H - 1) * W + (W - 1)] = texel;
    TOPO_GLOBAL_U32_RW(rt.normals)[(size_t)(H - 1) * W + 0] = texel;
    TOPO_GLOBAL_U32_RW(lb.normals)[(size_t)0 * W + (W - 1)] = texel;
    TOPO_GLOBAL_U32_RW(rb.normals)[0] = texel;
}

// Both border passes in one launch (they write disjoint texels): workgroups [0, chunks * n_edges) take the seam jobs (chunks =
// 64-texel pieces of a seam), the rest the corner jobs, 64 per workgroup.
__global__ __launch_bounds__(64) void k_normals_border(const TileDev* __restrict__ tiles, const EdgeJob* __restrict__ edges, uint32_t n_edges,
                                                       uint32_t chunks, const CornerJob* __restrict__ corners, uint32_t n_corners, int W, int H) {
    const uint32_t n_edge_blocks = chunks * n_edges;
    if (blockIdx.x < n_edge_blocks) normals_edge_body(tiles, edges, W, H, blockIdx.x % chunks, blockIdx.x / chunks);
    else normals_corner_body(tiles, corners, n_corners, W, H, blockIdx.x - n_edge_blocks);
}

}  // namespace
}  // namespace topo
