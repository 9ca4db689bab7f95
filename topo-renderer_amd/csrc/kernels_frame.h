// kernels_frame.h -- frame phase up to the visibility buffer: render_shader.wgsl vs_main + the fixed-function raster / depth test.
//
//   k_clear, k_cull, k_clear_cull   re-initialise the marked segments of the visibility buffer; frustum-cull the raster blocks and
//                                   split them into near work items and far occlusion-test candidates (one launch: k_clear_cull)
//   k_occlusion                     drop the far candidates whose footprint is already covered by nearer depths
//   k_raster                        one wave per block strip: vertices, small triangles in-wave
//   k_raster_rare                   the generic exact path: near-clipped triangles and triangles >= 64 px across
//   k_raster_cover                  one workgroup per region that ONE near-field giant covers whole: plain stores, no atomics
//   k_raster_big                    one wave per (large triangle, 64 x 64 px region)
//   k_put_views                     a submission's view constants into their device slot, where k_clear_cull does not carry them
//
// Launch order: [k_put_views ->] k_clear_cull (or k_clear -> k_cull) -> [near] k_raster -> k_raster_rare -> k_raster_cover -> k_raster_big -> k_occlusion ->
// [far survivors] k_raster -> k_raster_rare -> k_raster_big -> k_resolve (kernels_resolve.h).
#pragma once

#include "kernels_common.h"

namespace topo {
namespace {

// Re-initialise the visibility buffer for a new frame: only the segments marked dirty are rewritten (and unmarked).
// A wave takes 64 segments at a time: one coalesced read of their marks, then one 512-byte store per marked segment.
// The queue counters come in two sets that alternate from frame to frame: this pass zeroes the set of the NEXT frame
// (`zero`: queue counters, status word, the far sub-lists' counters), so nothing that runs beside it -- the cull, which appends
// through this frame's set -- depends on it.  `counters`: this frame's set (the check build's status record).
__device__ __forceinline__ void clear_body(uint64_t* __restrict__ vis, uint8_t* __restrict__ dirty, size_t n, uint32_t* __restrict__ counters,
                                           uint32_t* __restrict__ zero, uint32_t block, uint32_t n_blocks) {
    if (block == 0)
        for (uint32_t i = threadIdx.x; i < kCounterWords; i += 256) zero[i] = 0;
    const uint32_t lane = threadIdx.x & 63;
    const size_t nseg = (n + 63) >> 6, wave = (size_t)block * 4 + (threadIdx.x >> 6), nwave = (size_t)n_blocks * 4;
    for (size_t g = wave * 64; g < nseg; g += nwave * 64) {
        const bool mine = g + lane < nseg && dirty[g + lane] != 0;
        uint64_t todo = __ballot(mine);
        if (mine) dirty[g + lane] = 0;
        while (todo) {
            const size_t seg = g + (size_t)__builtin_ctzll(todo);
            todo &= todo - 1;
            if (TOPO_CHK(counters, seg * 64 + lane < ((n + 63) & ~(size_t)63), 3u, seg * 64 + lane))
                vis[seg * 64 + lane] = kVisClear;      // the buffer is allocated in whole segments
        }
    }
}
__global__ __launch_bounds__(256) void k_clear(uint64_t* __restrict__ vis, uint8_t* __restrict__ dirty, size_t n, uint32_t* __restrict__ counters,
                                               uint32_t* __restrict__ zero) {
    clear_body(vis, dirty, n, counters, zero, blockIdx.x, gridDim.x);
}

// Conservative frustum test of one raster block against one view, in f64.  A block is kept unless its
// bounding sphere (inflated by 64 m for the f32 noise of the real vertex path) lies wholly outside one of
// the six clip planes of camera_proj.  Culling is result-neutral: culled blocks cannot produce fragments.

// Clip plane `pl` of a column-major view-projection matrix as (a, b, c, d, |(a, b, c)|): 0..3 = w +- x, w +- y,
// 4 = near (z_clip >= 0), 5 = w - z.
__device__ __forceinline__ void clip_plane(const float* m, int pl, double out[5]) {
    double a, b, cc, d;
    const int row = pl >> 1;            // 0: x, 1: y, 2: z
    const double sgn = (pl & 1) ? -1.0 : 1.0;
    if (pl == 4) {                      // near: z_clip >= 0
        a = m[2]; b = m[6]; cc = m[10]; d = m[14];
    } else {                            // w +- row
        a = (double)m[3] + sgn * (double)m[row];
        b = (double)m[7] + sgn * (double)m[4 + row];
        cc = (double)m[11] + sgn * (double)m[8 + row];
        d = (double)m[15] + sgn * (double)m[12 + row];
    }
    out[0] = a; out[1] = b; out[2] = cc; out[3] = d;
    out[4] = sqrt(a * a + b * b + cc * cc);
}

// One lane per (view, tile, block).  f64 throughout; everything here is a conservative, result-neutral filter:
//  * frustum: the block's bounding sphere (inflated by 72 m for the f32 noise of the real vertex path) against the
//    six clip planes of camera_proj -- culled blocks cannot produce fragments;
//  * near/far split: blocks whose nearest possible view depth exceeds P.split_m become occlusion-test candidates
//    (FarItem) instead of work items; for them the lane also projects the eight corners of the block's bounding
//    slab -- the lat/lon rectangle of its vertices x [hmin - 1 m, hmax + 2 m + sagitta]: the flat-faced hull of those
//    eight points holds the block's ideal surface radially (the load phase measures the sagitta of the patch over the flat top;
//    blocks where it exceeds 1 m -- coarse tiles -- are never candidates) but not sideways: the equator-side edge follows a
//    parallel, which bows out of the plane through the edge's ends by R (dlon^2 / 8) sin lat cos lat -- metres in the COP90 width
//    bands, whatever the sagitta -- and the f32 vertex path adds its own noise.  So the lane records the pixel box of the eight
//    corners with a margin of 2 px + (the block's bulge, a load-time table, + kFarNoiseM) in pixels at the slab's smallest w
//    (2.3 to 2.4 px at the benchmark's sectors and split; whatever it takes at a longer focal length), and a lower bound of the depths
//    (z_ndc at the smallest corner w, minus 8/w: the f32 clip-space cancellation noise is ~1 clip unit; bulge and noise move w by
//    metres, z_ndc by 50 m / w^2 each, far inside the 8/w beyond the 1000 m a candidate needs).
// kFarNoiseM: how far the real pipeline's vertex can lie from the ideal one, as a displacement.  The f32 longitude, latitude and
// sin / cos put the position up to 1.8 m off (measured on the oracle's vertex path: tests/test_cull_cpu.py), the f32 product with
// camera_proj adds four roundings of terms the size of |row| x 6.4e6, 1.5 m-equivalents in x, y and w: 3.3 m, taken as 8.
constexpr double kFarNoiseM = 8.0;
// Emit a block the raster must visit.  With the occlusion filter on, such blocks are few and heavy (large triangles),
// so each is cut into strips of P.near_strip cell rows (the host picks 1, 2 or 4 by the size of the submission) to spread them over the resident waves:
// block = id | first cell row << 24 | rows << 28 (rows 0 = the whole block).
__device__ __forceinline__ void emit_near(const FrameParams& P, uint32_t view, uint32_t rank, uint32_t blk) {
    if (P.split_m > 0.0f) {
        const uint32_t by = blk / P.bx_count;
        const uint32_t cell_rows = min(kBCY, P.tile_h - 1 - by * kBCY);
        const uint32_t strip = P.near_strip, n = (cell_rows + strip - 1) / strip;
        const uint32_t base = atomicAdd(&P.counters[kCtrWork], n);
        for (uint32_t k = 0; k < n; ++k)
            if (base + k < P.near_cap && TOPO_CHK(P.counters, blk < (1u << 24) && strip * k < 16u, 4u, blk))
                P.work[base + k] = WorkItem{(view << 16) | rank, blk | ((strip * k) << 24) | (min(strip, cell_rows - strip * k) << 28)};
        return;
    }
    const uint32_t slot = atomicAdd(&P.counters[kCtrWork], 1u);
    if (slot < P.near_cap) P.work[slot] = WorkItem{(view << 16) | rank, blk};
}

// Which (view, tile, block) a cull lane works on.  Full grid (wgs_per_pair == 0): lane g of the launch is triple g, views outermost.
// Pair list (the host's tile prefilter, host_math.hpp: tile_prefilter): workgroup b takes blocks [256 (b % wgs_per_pair), + 256) of
// kept pair b / wgs_per_pair; `pairs`: the list in the launch's argument segment, two 16-bit codes (view * n_tiles + rank) per word.
struct CullMap {
    uint32_t blocks_per_tile, wgs_per_pair;
    size_t gid0;                // full grid: the workgroup's first triple
    uint32_t view, rank, blk0;  // pair list: the workgroup's pair and first block
    __device__ __forceinline__ CullMap(const FrameParams& P, uint32_t block, const_space_ptr<uint32_t> pairs, uint32_t wgs_per_pair_)
        : blocks_per_tile(P.bx_count * P.by_count), wgs_per_pair(wgs_per_pair_), gid0((size_t)block * 256), view(0), rank(0), blk0(0) {
        if (wgs_per_pair) {
            const uint32_t pair = block / wgs_per_pair;
            const uint32_t word = TOPO_CHK(P.counters, pair < kMaxCullPairs, 18u, pair) ? pairs[pair >> 1] : 0u;
            uint32_t code = (word >> ((pair & 1u) * 16u)) & 0xFFFFu;
            if (!TOPO_CHK(P.counters, code < P.n_views * P.n_tiles, 18u, code)) code = 0u;
            view = code / P.n_tiles; rank = code % P.n_tiles;
            blk0 = (block % wgs_per_pair) * 256u;
        } else {
            view = (uint32_t)(gid0 / ((size_t)blocks_per_tile * P.n_tiles));      // the first view the workgroup can meet
        }
    }
    // lane `t` of the workgroup: its triple; false: past the end
    __device__ __forceinline__ bool locate(const FrameParams& P, uint32_t t, uint32_t& v, uint32_t& r, uint32_t& b) const {
        if (wgs_per_pair) {
            v = view; r = rank; b = blk0 + t;
            return b < blocks_per_tile;
        }
        const size_t g = gid0 + t;
        b = (uint32_t)(g % blocks_per_tile);
        r = (uint32_t)((g / blocks_per_tile) % P.n_tiles);
        v = (uint32_t)(g / ((size_t)blocks_per_tile * P.n_tiles));
        return g < (size_t)P.n_views * P.n_tiles * blocks_per_tile;
    }
};

__device__ __forceinline__ void cull_body(const FrameParams& P, uint32_t block, const_space_ptr<uint32_t> pairs, uint32_t wgs_per_pair) {
    const CullMap map(P, block, pairs, wgs_per_pair);
    const uint32_t blocks_per_tile = map.blocks_per_tile;
    // the six clip planes (and their norms) of the first two views this workgroup can meet, once per workgroup
    __shared__ double s_plane[2][6][5];
    __shared__ uint32_t s_far[256], s_nfar;      // lanes whose block is an occlusion-test candidate
    const uint32_t view0 = map.view;
    if (threadIdx.x < 12 && view0 + threadIdx.x / 6 < P.n_views) clip_plane(P.views[view0 + threadIdx.x / 6].proj, threadIdx.x % 6, s_plane[threadIdx.x / 6][threadIdx.x % 6]);
    if (threadIdx.x == 0) s_nfar = 0;
    __syncthreads();
    // ---- phase A, one lane per (view, tile, block): frustum test, then near / far classification
    uint32_t blk, rank, view;
    if (map.locate(P, threadIdx.x, view, rank, blk)) {
        const TileDev& t = P.tiles[rank];
        const double hmin = (double)t.block_minmax[2 * blk], hmax = (double)t.block_minmax[2 * blk + 1];
        const double* bs = t.block_bounds + (size_t)blk * 4;      // bounding sphere from the load phase
        const double c[3] = {bs[0], bs[1], bs[2]}, radius = bs[3];
        const float* m = P.views[view].proj;
        bool keep = true;
        for (int pl = 0; pl < 6 && keep; ++pl) {
            double own[5];
            const double* q = s_plane[view - view0 < 2 ? view - view0 : 0][pl];
            if (view - view0 >= 2) {            // tiny mosaics: more than two views per workgroup
                clip_plane(m, pl, own);
                q = own;
            }
            const double dist = q[0] * c[0] + q[1] * c[1] + q[2] * c[2] + q[3];
            if (dist < -radius * q[4]) keep = false;
        }
        const bool sane = hmin <= hmax;         // NaN heights: no filtering at all, the raster path deals with it
        if (!sane) keep = true;
        if (keep) {
            // view depth of the nearest point the block can contain
            const double wn = sqrt((double)m[3] * m[3] + (double)m[7] * m[7] + (double)m[11] * m[11]);
            const double w_near = ((double)m[3] * c[0] + (double)m[7] * c[1] + (double)m[11] * c[2] + (double)m[15]) - radius * wn;
            // (coarse tiles: a block whose curvature exceeds the slab's 1 m allowance is always rastered, never filtered)
            const double sagitta = t.block_bounds[(size_t)blocks_per_tile * 16 + blk];
            if (sane && P.split_m > 0.0f && w_near > (double)P.split_m && sagitta <= 1.0) {
                const uint32_t fslot = atomicAdd(&s_nfar, 1u);
                if (TOPO_CHK(P.counters, fslot < 256u, 5u, fslot)) s_far[fslot] = threadIdx.x;
            }
            else emit_near(P, view, rank, blk);
        }
    }
    __syncthreads();
    // ---- phase B, one lane per candidate (they are ~10 % of the lanes, scattered: handled in place, every wave would
    // pay for the f64 projection of the eight slab corners)
    for (uint32_t i = threadIdx.x; i < s_nfar; i += blockDim.x) {
        (void)map.locate(P, s_far[i], view, rank, blk);
        const TileDev& t = P.tiles[rank];
        const double hmin = (double)t.block_minmax[2 * blk], hmax = (double)t.block_minmax[2 * blk + 1];
        const double* bb = t.block_bounds + (size_t)blocks_per_tile * 4 + (size_t)blk * 12;   // corner directions
        const float* m = P.views[view].proj;
        double bxlo = 1e30, bxhi = -1e30, bylo = 1e30, byhi = -1e30, wmin = 1e30, zclip_at_wmin = 0.0;
        const double hs[2] = {hmin - 1.0, hmax + 2.0 + t.block_bounds[(size_t)blocks_per_tile * 16 + blk]};      // + the patch's sagitta (<= 1 m here)
#pragma unroll 1      // (eight corners unrolled kept 124 registers live; the loop form needs half, and the clear running beside this kernel gets the waves)
        for (int k = 0; k < 8; ++k) {
            const double R = (double)kR0 + (k < 4 ? hs[0] : hs[1]);
            const double px = R * bb[3 * (k & 3)], py = R * bb[3 * (k & 3) + 1], pz = R * bb[3 * (k & 3) + 2];
            const double cx = (double)m[0] * px + (double)m[4] * py + (double)m[8] * pz + (double)m[12];
            const double cy = (double)m[1] * px + (double)m[5] * py + (double)m[9] * pz + (double)m[13];
            const double cz = (double)m[2] * px + (double)m[6] * py + (double)m[10] * pz + (double)m[14];
            const double cw = (double)m[3] * px + (double)m[7] * py + (double)m[11] * pz + (double)m[15];
            const double icw = 1.0 / cw;      // one f64 division per corner (the +-2 px margin dwarfs the extra rounding)
            const double sx = (cx * icw * 0.5 + 0.5) * (double)P.W, sy = (0.5 - cy * icw * 0.5) * (double)P.H;
            bxlo = sx < bxlo ? sx : bxlo; bxhi = sx > bxhi ? sx : bxhi;
            bylo = sy < bylo ? sy : bylo; byhi = sy > byhi ? sy : byhi;
            if (cw < wmin) { wmin = cw; zclip_at_wmin = cz; }
        }
        // z_ndc = a + b / w (b < 0) is a function of w alone and w is linear in position, so over the slab's convex
        // hull its minimum sits at the corner with the smallest w.  The real pipeline computes z_clip and w as f32
        // fma chains over ~6.4e6-sized terms: each carries up to ~1 (metre-sized clip units) of cancellation noise,
        // i.e. z_ndc is only good to ~2 / w.  Shave 8 / w.
        const double zmin = (zclip_at_wmin - 8.0) / wmin;
        if (!(wmin > 1000.0 && zmin > 0.0 && zmin < 1.0)) {
            emit_near(P, view, rank, blk);          // no usable bound: rasterise it with the near blocks
            continue;
        }
        // The margin.  A vertex of the real pipeline lies within `off` metres of the slab's hull: the block's sideways bulge (load
        // phase) + kFarNoiseM.  A point p = q + d, q in the hull, |d| <= off, has x_clip and w within |x row| off and |w row| off of
        // q's, so wherever p is on the target (|x / w| <= 1) its x / w lies within (|x row| + |w row|) off / w(q) of q's, and
        // w(q) >= wmin; likewise y.  2 px on top, for the rounding of all this.
        const double off = t.block_bounds[(size_t)blocks_per_tile * 17 + blk] + kFarNoiseM;
        const double wrow = sqrt((double)m[3] * m[3] + (double)m[7] * m[7] + (double)m[11] * m[11]);
        const double mx = 2.0 + 0.5 * (double)P.W * (sqrt((double)m[0] * m[0] + (double)m[4] * m[4] + (double)m[8] * m[8]) + wrow) * off / wmin;
        const double my = 2.0 + 0.5 * (double)P.H * (sqrt((double)m[1] * m[1] + (double)m[5] * m[5] + (double)m[9] * m[9]) + wrow) * off / wmin;
        // (clamped as doubles: at a long focal length the margin alone can exceed what an int32 holds)
        const double fx0 = fmax(floor(bxlo - mx), 0.0), fx1 = fmin(ceil(bxhi + mx), (double)(P.W - 1));
        const double fy0 = fmax(floor(bylo - my), 0.0), fy1 = fmin(ceil(byhi + my), (double)(P.H - 1));
        if (!(fx0 <= fx1 && fy0 <= fy1)) continue;       // wholly outside the target even with the margin
        const int32_t ix0 = (int32_t)fx0, ix1 = (int32_t)fx1, iy0 = (int32_t)fy0, iy1 = (int32_t)fy1;
        float zf = (float)zmin;
        if ((double)zf > zmin) zf = bits_f(f_bits(zf) - 1u);      // round down
        // 10^5 candidates appended through ONE counter cost this kernel 12 of its 43 us (atomics on one address are served one
        // at a time, ~12 ns each, however the waves aggregate them): the list is kept as kFarLists sub-lists, workgroup b
        // appending to sub-list b % kFarLists
        const uint32_t q = block % kFarLists, slot = atomicAdd(&P.counters[far_list_counter(q)], 1u);
        if (TOPO_CHK(P.counters, slot < P.far_sub_cap, 5u, slot)) {
            FarItem fi;
            fi.view_rank = (view << 16) | rank; fi.block = blk;
            fi.x0 = (uint16_t)ix0; fi.x1 = (uint16_t)ix1; fi.y0 = (uint16_t)iy0; fi.y1 = (uint16_t)iy1;
            fi.zmin_bits = f_bits(zf);
            P.far[(size_t)q * P.far_sub_cap + slot] = fi;
        }
    }
}

// The kept (view, tile) pairs of a submission, as the launch's argument segment carries them (wgs_per_pair != 0): up to kMaxCullPairs
// 16-bit codes.  With the ViewPack beside it the segment stays well inside the 4 KB a launch may pass.
struct CullPairs { uint16_t code[kMaxCullPairs]; };
struct CullArgs {               // k_cull's parameter list as the argument segment lays it out
    FrameParams P;
    uint32_t wgs_per_pair;
    CullPairs pairs;
};
__global__ __launch_bounds__(256) void k_cull(FrameParams P, uint32_t wgs_per_pair, CullPairs pairs) {
    cull_body(P, blockIdx.x, kernarg<uint32_t>(offsetof(CullArgs, pairs)), wgs_per_pair);
}
// The clear and the cull of a frame in ONE launch: they share nothing (the clear rewrites visibility keys and zeroes the NEXT
// frame's counters, the cull reads the load-time tables and appends through this frame's counters), one is bound by its
// stores, the other by f64 arithmetic and gathers -- side by side they take what the clear takes alone (c4: 0.046 + 0.031 ->
// 0.05 ms).
// `pack_words` != 0: the submission's view constants ride in this launch's own argument segment (`pack`: up to kPackViews views, 22
// words each).  The cull reads them there -- the segment is ordinary device-visible memory behind a constant-address-space pointer --
// and the launch's first workgroup copies them into the device slot the frame's later kernels read (P.views): no upload in front of
// the frame, not even a kernel's.  n_cull_blocks may be 0 (no pair survived the prefilter): the launch is the clear alone.
struct ClearCullArgs {          // the kernel's parameter list as the argument segment lays it out (natural alignment, in order)
    FrameParams P;
    uint32_t n_cull_blocks, n_clear_blocks;
    uint32_t* zero;
    ViewPack pack;
    uint32_t pack_words;
    uint32_t wgs_per_pair;
    CullPairs pairs;
};
static_assert(sizeof(ClearCullArgs) <= 3584 && sizeof(CullArgs) <= 3584, "a launch's argument segment holds 4 KB, the hidden arguments included");
static_assert(offsetof(ClearCullArgs, pairs) % 4 == 0 && offsetof(CullArgs, pairs) % 4 == 0, "the pair list is read in words");
// (the offsets the code object's metadata gives for the two kernels' arguments: tools/kernel_resources.py leaves the object to read them from)
static_assert(offsetof(ClearCullArgs, pack) == 232 && offsetof(ClearCullArgs, pairs) == 944 && offsetof(CullArgs, pairs) == 220, "the argument segment's layout");
__global__ __launch_bounds__(256) void k_clear_cull(FrameParams P, uint32_t n_cull_blocks, uint32_t n_clear_blocks, uint32_t* __restrict__ zero, ViewPack pack,
                                                    uint32_t pack_words, uint32_t wgs_per_pair, CullPairs pairs) {
    if (pack_words) {
        const auto src = kernarg<uint32_t>(offsetof(ClearCullArgs, pack));
        if (blockIdx.x == 0 && threadIdx.x < pack_words) const_cast<uint32_t*>(reinterpret_cast<const uint32_t*>(P.views))[threadIdx.x] = src[threadIdx.x];
        P.views = (const ViewDev*)(const void*)src;
    }
    // the two kinds of workgroup interleaved evenly along the launch order (all of one kind first would run them one after the other:
    // a launch's workgroups start in order)
    const uint32_t total = n_cull_blocks + n_clear_blocks;
    const uint32_t before = (uint32_t)((uint64_t)blockIdx.x * n_clear_blocks / total), upto = (uint32_t)((uint64_t)(blockIdx.x + 1u) * n_clear_blocks / total);
    if (upto > before) clear_body(P.vis, P.dirty, (size_t)P.n_views * P.W * P.H, P.counters, zero, before, n_clear_blocks);
    else cull_body(P, blockIdx.x - before, kernarg<uint32_t>(offsetof(ClearCullArgs, pairs)), wgs_per_pair);
}

// One wave per far candidate: the block is dropped iff EVERY pixel of its footprint already holds a depth below
// the block's lower bound -- then none of its fragments could pass `Less`.  Pixels in the gaps between tiles, or
// anywhere nothing nearer has been drawn, keep the block alive, so the filter is exact by construction.
#ifndef TOPO_OCC_ROWS
#define TOPO_OCC_ROWS 4
#endif
constexpr uint32_t kOccRows = TOPO_OCC_ROWS;      // rows of a footprint whose depths are in flight before the wave votes
__global__ __launch_bounds__(256) void k_occlusion(FrameParams P) {
    // between the two raster phases: the rare/big queues keep growing, the second phase starts where the first ended
    // (nothing enqueues while this kernel runs, and the consumers of the marks are launched after it)
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        P.counters[kCtrBigStart] = P.counters[kCtrBig];
        P.counters[kCtrRareStart] = P.counters[kCtrRare];
    }
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave_global = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), wave_count = gridDim.x * 4;
    // The sub-lists are walked as one list: lane k of every wave holds the number of entries in sub-lists 0 .. k (an inclusive
    // scan of the 64 counts), entry g of the whole lies in the sub-list q with incl[q - 1] <= g < incl[q].
    static_assert(kFarLists == 64, "one sub-list per lane");
    uint32_t incl = min(P.counters[far_list_counter(lane)], P.far_sub_cap);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, o);
        if ((int)lane >= o) incl += up;
    }
    const uint32_t count = (uint32_t)__shfl((int)incl, 63);
    if (blockIdx.x == 0 && threadIdx.x == 0) P.counters[kCtrFarTested] = count;      // the candidate count, for the frame's statistics
    auto entry = [&](uint32_t g) -> const FarItem& {
        const uint32_t q = (uint32_t)__popcll(__ballot(incl <= g));      // sub-lists that end at or before g
        const uint32_t start = q ? (uint32_t)__shfl((int)incl, (int)q - 1) : 0u;
        return P.far[(size_t)q * P.far_sub_cap + (g - start)];
    };
    if (count == 0) return;
    FarItem fi_next = entry(wave_global < count ? wave_global : 0u);      // (the next candidate's record is fetched under the current one's scan)
    for (uint32_t item = wave_global; item < count; item += wave_count) {
        const FarItem fi = fi_next;
        fi_next = entry(item + wave_count < count ? item + wave_count : item);
        const uint64_t* vis = P.vis + (size_t)(fi.view_rank >> 16) * P.W * P.H;
        // footprints are wide and flat: lanes run along x, kOccRows rows per round so that as many loads are in flight
        // before the first wave-wide vote
        bool visible = false;
        for (uint32_t x = fi.x0; x <= fi.x1 && !visible; x += 64) {
            const uint32_t px = min(x + lane, (uint32_t)fi.x1);       // surplus lanes re-test the last column
            for (uint32_t y = fi.y0; y <= fi.y1; y += kOccRows) {
                uint32_t d[kOccRows];
#pragma unroll
                for (uint32_t k = 0; k < kOccRows; ++k) {
                    const size_t at = (size_t)min(y + k, (uint32_t)fi.y1) * P.W + px;
                    d[k] = TOPO_CHK(P.counters, at < (size_t)P.W * P.H && (fi.view_rank >> 16) < P.n_views, 6u, at) ? (uint32_t)(vis[at] >> 32) : 0u;
                }
                bool open = false;
#pragma unroll
                for (uint32_t k = 0; k < kOccRows; ++k) open |= d[k] >= fi.zmin_bits;
                if (__any(open)) { visible = true; break; }
            }
        }
        if (visible && lane == 0) {
            // survivors are few: cut them into strips like the near blocks, or the second raster phase runs on a
            // fraction of the resident waves
            const uint32_t blk = fi.block, by = blk / P.bx_count;
            const uint32_t cell_rows = min(kBCY, P.tile_h - 1 - by * kBCY);
            const uint32_t strip = P.near_strip, n = (cell_rows + strip - 1) / strip;
            const uint32_t base = atomicAdd(&P.counters[kCtrFarSurvived], n);
            for (uint32_t k = 0; k < n; ++k)
                if (base + k < P.near_cap)
                    P.work2[base + k] = WorkItem{fi.view_rank, blk | ((strip * k) << 24) | (min(strip, cell_rows - strip * k) << 28)};
        }
    }
}


// ---- raster ------------------------------------------------------------------------------------------

// Pixel loop of the generic (int64) path.
__device__ __forceinline__ void raster_box(const TriSetup& ts, const Vis& vis, int32_t W, uint32_t id,
                                           int32_t px0, int32_t px1, int32_t py0, int32_t py1) {
    for (int32_t py = py0; py <= py1; ++py)
        for (int32_t px = px0; px <= px1; ++px) {
            float z, b[3];
            if (triangle_pixel(ts, px, py, z, b)) vis_min(vis, (size_t)py * W + px, vis_key(z, id));
        }
}

// A region that one giant covers whole needs no atomics: nobody else's fragment can be lost if the region is written in a launch of
// its own (k_raster_cover), one lane per pixel taking min(old, mine).  k_raster_rare, in the near phase, asks every item it has room
// for in the big queue whether it covers its region (setup_covers_region, exact); such an item is flagged kBigCovered and bids for
// its (view, region): a 64-bit atomicMax of (the frame's serial << 32 | the item's queue index) into the region's owner word.  The
// atomic returns nothing -- the lane never waits for it (with a returning claim and a list appended through one counter the kernel
// took 43 instead of 19 us at c4: two trips to memory in every step of the whole-wave region loop) -- and nothing has to be reset
// between frames: a word of an older serial loses against any bid.  When the kernel is done the word names the region's one winner:
// k_raster_cover draws it, k_raster_big skips it and draws every other item, the losing bidders among them.
// The frame keeps no statistics of this: the test hook counts the flagged items and the owner words afterwards, on the host.
__device__ __forceinline__ uint32_t cover_region_index(const CoverParams& C, uint32_t view, int32_t rx, int32_t ry) {
    return (view * C.regions_y + (uint32_t)ry) * C.regions_x + (uint32_t)rx;
}
__device__ __forceinline__ uint64_t cover_bid(const CoverParams& C, uint32_t big_index) { return ((uint64_t)C.serial << 32) | big_index; }
__device__ __forceinline__ bool cover_claim(const FrameParams& P, const CoverParams& C, const TriSetup& ts, uint32_t view, int32_t rx, int32_t ry,
                                            uint32_t big_index) {
    if (!setup_covers_region(ts, P.W, P.H, rx, ry)) return false;
    const uint32_t r = cover_region_index(C, view, rx, ry);
    if (!TOPO_CHK(P.counters, view < P.n_views && (uint32_t)rx < C.regions_x && (uint32_t)ry < C.regions_y && r < C.cap, 30u, r)) return false;
    atomicMax(reinterpret_cast<unsigned long long*>(C.owner + r), (unsigned long long)cover_bid(C, big_index));
    return true;
}

// Hand a triangle whose pixel box is larger than 4x4 to k_raster_big: one BigItem per overlapped 64x64 px
// region.  Returns false when the queue is full (the caller then rasterises in-lane).  view_of(rx, ry, queue index): the word that
// goes into the item's `view` -- the view itself (k_raster), or the view flagged kBigCovered where the item has bid for its region
// (k_raster_rare: cover_claim).
template <typename ViewOf>
__device__ __forceinline__ bool enqueue_big_items(const FrameParams& P, uint32_t view, uint32_t id, const SVert& s0, const SVert& s1, const SVert& s2,
                                                  int32_t px0, int32_t px1, int32_t py0, int32_t py1, ViewOf&& view_of) {
    const int32_t rx0 = px0 >> 6, rx1 = px1 >> 6, ry0 = py0 >> 6, ry1 = py1 >> 6;
    const uint32_t n = (uint32_t)((rx1 - rx0 + 1) * (ry1 - ry0 + 1));
    const uint32_t base = atomicAdd(&P.counters[kCtrBig], n);
    BigItem it;
    it.view = view;
    it.id = id;
    it.X[0] = s0.X; it.X[1] = s1.X; it.X[2] = s2.X;
    it.Y[0] = s0.Y; it.Y[1] = s1.Y; it.Y[2] = s2.Y;
    it.z[0] = s0.z; it.z[1] = s1.z; it.z[2] = s2.z;
    if (base >= P.big_cap || n > P.big_cap - base) {
        atomicOr(&P.counters[kCtrStatus], kStatusBigOverflow);
        // neutralise whatever part of the reservation lies inside the queue
        it.id = kNoTri;
        it.region = 0;
        for (uint32_t k = base; k < P.big_cap && k - base < n; ++k) P.big[k] = it;
        return false;
    }
    uint32_t k = base;
    for (int32_t ry = ry0; ry <= ry1; ++ry)
        for (int32_t rx = rx0; rx <= rx1; ++rx) {
            it.region = ((uint32_t)ry << 16) | (uint32_t)rx;
            if (TOPO_CHK(P.counters, k < P.big_cap && rx >= 0 && ry >= 0 && rx * 64 < P.W && ry * 64 < P.H, 7u, k)) {
                it.view = view_of(rx, ry, k);
                P.big[k] = it;
            }
            ++k;
        }
    return true;
}
__device__ bool enqueue_big(const FrameParams& P, uint32_t view, uint32_t id, const SVert& s0, const SVert& s1, const SVert& s2,
                            int32_t px0, int32_t px1, int32_t py0, int32_t py1) {
    return enqueue_big_items(P, view, id, s0, s1, s2, px0, px1, py0, py1, [&](int32_t, int32_t, uint32_t) { return view; });
}
// k_raster_rare's: `ts` is the triangle's setup
__device__ bool enqueue_big_cover(const FrameParams& P, const CoverParams& C, const TriSetup& ts, uint32_t view, uint32_t id, const SVert& s0, const SVert& s1,
                                  const SVert& s2) {
    return enqueue_big_items(P, view, id, s0, s1, s2, ts.px0, ts.px1, ts.py0, ts.py1, [&](int32_t rx, int32_t ry, uint32_t k) {
        return C.serial && cover_claim(P, C, ts, view, rx, ry, k) ? view | kBigCovered : view;
    });
}

// Triangles the lean kernel does not handle go to k_raster_rare.
__device__ __forceinline__ void enqueue_rare(const FrameParams& P, uint32_t view, uint32_t draw) {
    const uint32_t slot = atomicAdd(&P.counters[kCtrRare], 1u);
    if (slot < P.rare_cap) P.rare[slot] = RareItem{view, draw};
    else atomicOr(&P.counters[kCtrStatus], kStatusRareOverflow);
}

// Fragment staging: lanes of k_raster do not touch the visibility buffer while they walk their triangles (the
// walk is divergent: a few lanes would issue one atomic each per iteration); they append (pixel, key) pairs to a
// per-wave LDS list which the wave then drains densely, one atomic per lane and instruction.
#ifndef TOPO_FRAG_CAP
#define TOPO_FRAG_CAP 128
#endif
constexpr uint32_t kFragCap = TOPO_FRAG_CAP;
struct FragList {
    uint32_t count;
    uint32_t pix[kFragCap];
    uint64_t key[kFragCap];
};

#ifndef TOPO_INLANE_ROWS
#define TOPO_INLANE_ROWS 5
#endif
#ifndef TOPO_INLANE_COLS
#define TOPO_INLANE_COLS 24
#endif
constexpr int32_t kInlaneRows = TOPO_INLANE_ROWS, kInlaneCols = TOPO_INLANE_COLS;

__device__ __forceinline__ void frag_push(FragList& fl, const Vis& vis, uint32_t pix, uint64_t key) {
    const uint32_t slot = atomicAdd(&fl.count, 1u);
    if (slot < kFragCap) {
        fl.pix[slot] = pix;
        fl.key[slot] = key;
    } else {
        vis_min(vis, pix, key);   // list full: fall back to the direct path
    }
}

// ---- in-wave triangle compaction -------------------------------------------------------------------------
// Far-field cells are sub-pixel: nine triangles in ten die in the early tests (back face, no pixel centre in the
// box).  Walking the survivors' pixels in the lane that found them would leave 58 of 64 lanes idle through every
// loop, so k_raster works in two stages: stage 1 classifies the two triangles of each lane's cell and appends the
// survivors to a per-wave LDS list (slot = running count + rank among the pushing lanes: no atomics); whenever
// the list holds a wave's worth, stage 2 pops 64 of them, one per lane, and walks their pixel rows.
constexpr uint32_t kTriCap = 128;
struct TriList {                 // structure of arrays: lane-consecutive entries hit consecutive banks
    int32_t X0[kTriCap], Y0[kTriCap], X1[kTriCap], Y1[kTriCap], X2[kTriCap], Y2[kTriCap];
    float z0[kTriCap], z1[kTriCap], z2[kTriCap];
    uint32_t id[kTriCap];
};

// Stage 1.  A triangle whose three snapped vertices span < 64 px fits int32 (|delta| < 2^14, so every product is
// < 2^28; 24-bit multiplies give the exact integers triangle_setup computes in int64).  Returns true when the
// triangle is to be walked in-wave (front-facing, its pixel box holds a centre and is at most kInlaneRows x
// kInlaneCols); larger boxes go to k_raster_big, >= 64 px spans to k_raster_rare.
__device__ __forceinline__ bool classify_small(const FrameParams& P, const SVert& s0, const SVert& s1, const SVert& s2, uint32_t view,
                                               uint32_t id) {
    const int32_t X0 = s0.X, Y0 = s0.Y, X1 = s1.X, Y1 = s1.Y, X2 = s2.X, Y2 = s2.Y;
    const int32_t mnx = min(X0, min(X1, X2)), mxx = max(X0, max(X1, X2));
    const int32_t mny = min(Y0, min(Y1, Y2)), mxy = max(Y0, max(Y1, Y2));
    if ((mxx - mnx) >= (1 << 14) || (mxy - mny) >= (1 << 14)) {
        enqueue_rare(P, view, id >> 1);
        return false;
    }
    const int32_t area2 = __mul24(X1 - X0, Y2 - Y0) - __mul24(Y1 - Y0, X2 - X0);
    if (area2 >= 0) return false;
    const int32_t px0 = max((mnx + 127) >> 8, 0), px1 = min((mxx - 128) >> 8, P.W - 1);
    const int32_t py0 = max((mny + 127) >> 8, 0), py1 = min((mxy - 128) >> 8, P.H - 1);
    if (px0 > px1 || py0 > py1) return false;
    if (py1 - py0 >= kInlaneRows || px1 - px0 >= kInlaneCols) {
        if (!enqueue_big(P, view, id, s0, s1, s2, px0, px1, py0, py1)) enqueue_rare(P, view, id >> 1);
        return false;
    }
    return true;
}

// Stage 2 = raster_rows() (topo_pipeline.h), one listed triangle per lane, fragments into the per-wave LDS list.

// Append this lane's triangle (if `push`) behind the `n` entries already listed; returns the new count.  Runs in
// wave-uniform control flow: the slot is n + the lane's rank among the pushing lanes.
__device__ __forceinline__ uint32_t tri_push(TriList& tl, uint32_t n, bool push, const SVert& s0, const SVert& s1, const SVert& s2,
                                             uint32_t id, uint32_t* vis_counters) {
    const uint64_t mask = __ballot(push);
    if (push) {
        const uint32_t slot = n + __popcll(mask & ((1ull << (threadIdx.x & 63)) - 1ull));
        if (!TOPO_CHK(vis_counters, slot < kTriCap, 8u, slot)) return n;
        tl.X0[slot] = s0.X; tl.Y0[slot] = s0.Y; tl.X1[slot] = s1.X; tl.Y1[slot] = s1.Y; tl.X2[slot] = s2.X; tl.Y2[slot] = s2.Y;
        tl.z0[slot] = s0.z; tl.z1[slot] = s1.z; tl.z2[slot] = s2.z;
        tl.id[slot] = id;
    }
    return n + (uint32_t)__popcll(mask);
}

// Pop up to 64 listed triangles (the newest ones), one per lane, walk them, then flush the fragment list if it
// holds a wave's worth (or unconditionally when `flush`).  Returns the remaining count.
__device__ __forceinline__ uint32_t tri_drain(TriList& tl, FragList& fl, const Vis& vis, int32_t W, int32_t H, uint32_t n,
                                              bool flush) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t take = min(n, 64u), base = n - take;
    if (lane < take) {
        const uint32_t e = base + lane;
        raster_rows(W, H, tl.X0[e], tl.Y0[e], tl.X1[e], tl.Y1[e], tl.X2[e], tl.Y2[e], tl.z0[e], tl.z1[e], tl.z2[e], tl.id[e],
                    [&](uint32_t pix, uint64_t key) { frag_push(fl, vis, pix, key); });
    }
    const uint32_t nfrag = min(fl.count, kFragCap);
    if (nfrag >= 64 || (flush && nfrag > 0)) {
        for (uint32_t f = lane; f < nfrag; f += 64) vis_min(vis, fl.pix[f], fl.key[f]);
        if (lane == 0) fl.count = 0;
    }
    return base;
}

__device__ __forceinline__ SVert shfl_down1(const SVert& v) {
    SVert o;
    o.X = __shfl_down(v.X, 1);
    o.Y = __shfl_down(v.Y, 1);
    o.z = __shfl_down(v.z, 1);
    o.flag = __shfl_down(v.flag, 1);
    return o;
}

// One WAVE per surviving (view, tile, block) -- no workgroup barriers, no LDS vertex staging.  Lane i owns
// vertex column x0+i of the block (61 of 64 lanes); the wave walks the block's 16 vertex rows top to bottom,
// each lane transforming one vertex per row (coalesced 244-B row reads of the DEM, the next row's heights
// prefetched while the current row is processed; sin/cos of the longitude once per lane, of the latitudes once
// per row on lanes 0..15 and broadcast).  The previous row stays in registers; lane i then owns grid cell
// (x0+i, row-1): its four corners are its own two vertices and lane i+1's two, fetched with wave shuffles.
// Fragments go to a per-wave LDS list that the wave drains densely (one fragment per lane) whenever a row left
// more than a wave's worth in it.
#ifndef TOPO_RASTER_WAVES
#define TOPO_RASTER_WAVES 5
#endif
__global__ __launch_bounds__(256, TOPO_RASTER_WAVES) void k_raster(FrameParams P, int phase) {
    __shared__ FragList s_fl[4];
    __shared__ TriList s_tl[4];
    const WorkItem* __restrict__ work = phase == 0 ? P.work : P.work2;
    uint32_t count = P.counters[phase == 0 ? kCtrWork : kCtrFarSurvived];
    const uint32_t cap = P.near_cap;      // both lists hold strips
    if (count > cap) count = cap;
    // the wave index is wave-uniform: say so (readfirstlane), or the compiler treats everything derived from the
    // work item -- the view matrix, the tile descriptor -- as per-lane data and re-loads it with vector loads.
    // Waves stride statically over the work list (pulling chunks from an atomic cursor measured 17 % slower).
    const uint32_t lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    FragList& fl = s_fl[wave];
    TriList& tl = s_tl[wave];
    uint32_t ntri = 0;           // triangles waiting in tl (wave-uniform)
    const uint32_t wave_global = blockIdx.x * 4 + wave, wave_count = gridDim.x * 4;
    for (uint32_t item = wave_global; item < count; item += wave_count) {
        // The work item, the tile's descriptor and the view matrix are wave-uniform and written by EARLIER kernels: read through
        // the constant address space (const_space) they come in two round trips -- item, then descriptor and matrix together --
        // that wait on lgkmcnt.  As vector loads they were four dependent trips behind s_waitcnt vmcnt(0), each of which also
        // waits for every visibility atomic the wave still has in flight from the strip before.
        const auto wi_c = const_space(work + item);
        const WorkItem wi = {wi_c->view_rank, wi_c->block};
        const uint32_t view_idx = wi.view_rank >> 16, rank = wi.view_rank & 0xFFFFu;
        TileDev t;      // the fields this kernel reads (the rest stay unset)
        {
            const auto tc = const_space(P.tiles + rank);
            t.heights = tc->heights;
            t.raster_x = tc->raster_x; t.raster_y = tc->raster_y;
            t.model_x = tc->model_x; t.model_y = tc->model_y;
            t.scale_x = tc->scale_x; t.scale_y = tc->scale_y;
        }
        const auto view_proj = const_space(P.views[view_idx].proj);
        const uint32_t blk_id = wi.block & 0xFFFFFFu, strip_first = (wi.block >> 24) & 15u, strip_rows = wi.block >> 28;
        const uint32_t bx = blk_id % P.bx_count, by = blk_id / P.bx_count;
        const uint32_t x0 = bx * kBCX, y0 = by * kBCY + strip_first;   // strip_rows == 0: the whole block
        const uint32_t nrows = min(strip_rows ? strip_rows + 1 : kVY, P.tile_h - y0);   // vertex rows of this item
        const uint32_t ncx = min(kBCX, P.tile_w - 1 - x0);       // cells per row
        const uint32_t vx = x0 + lane;
        const bool vcol = lane < kVX && vx < P.tile_w;
        const Vis vis = view_vis(P, view_idx);
        // the view matrix, read once per block into scalar registers: left to the compiler it is re-loaded from
        // memory every row (it cannot prove the visibility-buffer atomics do not alias it) behind an
        // s_waitcnt vmcnt(0) that also drains the height prefetch
        float proj[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) proj[q] = view_proj[q];
        if (lane == 0) fl.count = 0;
        float slo, clo, lat_s = 0.0f, lat_c = 0.0f;
        sincos_f(vertex_lon(t, vcol ? vx : x0), slo, clo);
        if (lane < nrows) sincos_f(vertex_lat(t, y0 + lane), lat_s, lat_c);
        const auto hcol = TOPO_GLOBAL_F32(t.heights) + (size_t)y0 * P.tile_w + (vcol ? vx : x0);   // global, not flat, loads
        // heights are prefetched four rows ahead (a rotating register window): one 244-B row read per wave is
        // too little to have in flight at a time
        (void)TOPO_CHK(P.counters, rank < P.n_tiles && view_idx < P.n_views && y0 + nrows <= P.tile_h && (vcol ? vx : x0) < P.tile_w && nrows >= 1u, 9u,
                       ((uint64_t)y0 << 32) | x0);
        float h0 = hcol[0];
        float h1 = nrows > 1 ? hcol[(size_t)1 * P.tile_w] : 0.0f;
        float h2 = nrows > 2 ? hcol[(size_t)2 * P.tile_w] : 0.0f;
        float h3 = nrows > 3 ? hcol[(size_t)3 * P.tile_w] : 0.0f;
        SVert prev;
        prev.X = 0; prev.Y = 0; prev.z = 0.0f; prev.flag = kVtxNear;
        for (uint32_t r = 0; r < nrows; ++r) {
            const float h = h0;
            h0 = h1; h1 = h2; h2 = h3;
            if (r + 4 < nrows) h3 = hcol[(size_t)(r + 4) * P.tile_w];
            const float sla = __shfl(lat_s, (int)r), cla = __shfl(lat_c, (int)r);
            SVert cur;
            cur.X = 0; cur.Y = 0; cur.z = 0.0f; cur.flag = kVtxNear;
            if (vcol) {
                const f3 p = world_from_sincos(h, sla, cla, slo, clo);
                float clip[4];
                mat4_point(proj, p.x, p.y, p.z, clip);
                clip_to_screen(clip, (float)P.W, (float)P.H, cur);
            }
            if (r > 0) {
                // cell (i, j) = (x0 + lane, y0 + r - 1): a = (i,j) b = (i,j+1) c = (i+1,j) d = (i+1,j+1)
                const SVert cc = shfl_down1(prev), d = shfl_down1(cur);
                // Quad-level reject (result-neutral): if all four corners are plain vertices and their common pixel
                // box holds no pixel centre, neither triangle can produce a fragment.
                bool live = lane < ncx;
                if (live && (prev.flag | cur.flag | cc.flag | d.flag) == kVtxOk) {
                    const int32_t qx0 = min(min(prev.X, cur.X), min(cc.X, d.X)), qx1 = max(max(prev.X, cur.X), max(cc.X, d.X));
                    const int32_t qy0 = min(min(prev.Y, cur.Y), min(cc.Y, d.Y)), qy1 = max(max(prev.Y, cur.Y), max(cc.Y, d.Y));
                    const int32_t bx0 = max((qx0 + 127) >> 8, 0), bx1 = min((qx1 - 128) >> 8, P.W - 1);
                    const int32_t by0 = max((qy0 + 127) >> 8, 0), by1 = min((qy1 - 128) >> 8, P.H - 1);
                    live = bx0 <= bx1 && by0 <= by1;
                }
                const SVert &a = prev, &b = cur;
                const uint32_t i = x0 + lane, j = y0 + r - 1;
                const bool even = ((i + j) & 1u) == 0;
                const uint32_t tri0 = (i * (P.tile_h - 1) + j) * 2;
#pragma unroll
                for (uint32_t k = 0; k < 2; ++k) {
                    const SVert& s0 = k == 0 ? a : d;
                    const SVert& s1 = k == 0 ? b : cc;
                    const SVert& s2 = k == 0 ? (even ? d : cc) : (even ? a : b);
                    const uint32_t draw = rank * P.tris_per_tile + tri0 + k;
                    bool push = false;
                    if (live) {
                        const int fg = s0.flag | s1.flag | s2.flag;
                        if (fg == kVtxOk) {
                            push = classify_small(P, s0, s1, s2, view_idx, draw << 1);
                        } else if (fg & kVtxNear) {
                            const int nnear = (s0.flag == kVtxNear) + (s1.flag == kVtxNear) + (s2.flag == kVtxNear);
                            if (nnear != 3) enqueue_rare(P, view_idx, draw);
                        }   // else: guard band -> primitive discarded
                    }
                    ntri = tri_push(tl, ntri, push, s0, s1, s2, draw << 1, P.counters);
                    if (ntri >= 64) ntri = tri_drain(tl, fl, vis, P.W, P.H, ntri, false);
                }
            }
            prev = cur;
        }
        // block end: the list refers to this block's view, so it is emptied before the next item
        while (ntri > 0) ntri = tri_drain(tl, fl, vis, P.W, P.H, ntri, true);
        const uint32_t nfrag = min(fl.count, kFragCap);
        for (uint32_t f = lane; f < nfrag; f += 64) vis_min(vis, fl.pix[f], fl.key[f]);
        if (lane == 0) fl.count = 0;
    }
}

// One lane per RareItem: the generic exact path (near clipping, int64 setup).  Boxes up to 4x4 px are
// rasterised in-lane, larger ones go to the big queue (or, if that is full, are rasterised here as well).
// A triangle with at least kCoopRegions regions has its BigItems written by the WHOLE wave, 64 regions at a time: a lane's own loop
// over the regions of a triangle that covers a good part of the target (the near field's largest, cut by the near plane: a thousand
// regions and more) was this kernel's duration -- ~20 instructions per region on ONE lane, while the other 15 000 triangles had long
// been done.
// `C`: the near phase's launch lets covering items bid for their regions (C.serial != 0; cover_claim), only after their queue reservation
// has succeeded; the far phase's launch and a frame with the path switched off pass serial 0.
constexpr uint32_t kCoopRegions = 24;
__global__ __launch_bounds__(256) void k_raster_rare(FrameParams P, CoverParams C) {
    uint32_t count = P.counters[kCtrRare];
    if (count > P.rare_cap) count = P.rare_cap;
    const uint32_t lane = threadIdx.x & 63;
    for (uint32_t item = P.counters[kCtrRareStart] + blockIdx.x * blockDim.x + threadIdx.x; item < count; item += gridDim.x * blockDim.x) {
        const RareItem ri = P.rare[item];
        const uint32_t rank = fastdiv(ri.draw, P.div_tris), tri = ri.draw - rank * P.tris_per_tile;
        if (!TOPO_CHK(P.counters, rank < P.n_tiles && ri.view < P.n_views, 10u, ri.draw)) continue;
        const Vis vis = view_vis(P, ri.view);
        for (uint32_t fan = 0; fan < 2; ++fan) {
            ResolvedTri r;
            const bool has = resolve_triangle(P.tiles[rank], P.tile_w, P.div_hm1, P.tile_h - 1, P.views[ri.view], P.W, P.H, tri, fan, r);
            const TriSetup& ts = r.ts;
            const uint32_t id = (ri.draw << 1) | fan;
            const int32_t nx = has ? ts.px1 - ts.px0 + 1 : 0, ny = has ? ts.py1 - ts.py0 + 1 : 0;
            const bool small = nx <= 4 && ny <= 4;
            const int32_t rx0 = has ? ts.px0 >> 6 : 0, rx1 = has ? ts.px1 >> 6 : 0, ry0 = has ? ts.py0 >> 6 : 0, ry1 = has ? ts.py1 >> 6 : 0;
            const uint32_t rw = (uint32_t)(rx1 - rx0 + 1), n_regions = rw * (uint32_t)(ry1 - ry0 + 1);
            const bool coop = has && !small && n_regions >= kCoopRegions && rw <= 256u;
            bool in_lane = has && small;      // rasterised by this lane itself: boxes up to 4 x 4 px, and whatever the queue has no room for
            if (has && !small && !coop) in_lane = !enqueue_big_cover(P, C, ts, ri.view, id, r.s[0], r.s[1], r.s[2]);
            // ---- the wave's large jobs, one after the other, every lane that is still in this loop taking part
            uint64_t jobs = __ballot(coop);
            if (jobs) {
                const uint64_t act = __ballot(true);
                const uint32_t n_act = (uint32_t)__popcll(act), mine = (uint32_t)__popcll(act & ((1ull << lane) - 1ull));
                while (jobs) {
                    const int L = __builtin_ctzll(jobs);
                    jobs &= jobs - 1ull;
                    auto from = [&](int32_t v) { return __builtin_amdgcn_readlane(v, L); };
                    BigItem it;
                    it.view = (uint32_t)from((int32_t)ri.view);
                    it.id = (uint32_t)from((int32_t)id);
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        it.X[k] = from(r.s[k].X);
                        it.Y[k] = from(r.s[k].Y);
                        it.z[k] = wave_lane(r.s[k].z, L);
                    }
                    const int32_t jx0 = from(rx0), jy0 = from(ry0);
                    const uint32_t jw = (uint32_t)from((int32_t)rw), n = (uint32_t)from((int32_t)n_regions);
                    uint32_t base = 0;
                    if ((int)lane == L) base = atomicAdd(&P.counters[kCtrBig], n);
                    base = (uint32_t)from((int32_t)base);
                    if (base >= P.big_cap || n > P.big_cap - base) {      // no room: neutralise the part of the reservation inside the queue; the owner rasterises
                        if ((int)lane == L) { atomicOr(&P.counters[kCtrStatus], kStatusBigOverflow); in_lane = true; }
                        it.id = kNoTri;
                        it.region = 0;
                        for (uint32_t k = mine; k < n && base + k < P.big_cap; k += n_act) P.big[base + k] = it;
                        continue;
                    }
                    // the job's setup again, from its wave-uniform vertices (scalar registers), for the lanes' claims
                    TriSetup jts;
                    bool jcover = false;
                    if (C.serial) {
                        SVert q[3];
#pragma unroll
                        for (int k = 0; k < 3; ++k) { q[k].X = it.X[k]; q[k].Y = it.Y[k]; q[k].z = it.z[k]; q[k].flag = kVtxOk; }
                        jcover = triangle_setup(q[0], q[1], q[2], P.W, P.H, jts);
                    }
                    const uint32_t jview = it.view;
                    const uint32_t magic = region_split_magic(jw);
                    for (uint32_t k = mine; k < n; k += n_act) {
                        const uint32_t q = region_split_row(k, jw, n, magic);
                        const int32_t ry = jy0 + (int32_t)q, rx = jx0 + (int32_t)(k - q * jw);
                        it.region = ((uint32_t)ry << 16) | (uint32_t)rx;
                        if (TOPO_CHK(P.counters, base + k < P.big_cap && rx >= 0 && ry >= 0 && rx * 64 < P.W && ry * 64 < P.H, 7u, base + k)) {
                            it.view = jcover && cover_claim(P, C, jts, jview, rx, ry, base + k) ? jview | kBigCovered : jview;
                            P.big[base + k] = it;
                        }
                    }
                }
            }
            if (in_lane) raster_box(ts, vis, P.W, id, ts.px0, ts.px1, ts.py0, ts.py1);
        }
    }
}

// One workgroup per claimed region at a time: a near-field giant that covers its 64 x 64 px region (the part inside the target) and
// has won it, so this launch -- behind k_raster and k_raster_rare, in front of k_raster_big -- has ONE writer per pixel of the region
// and needs no atomics: key = min(old, mine) with a plain load and a plain store.  Workgroup b reads region b's owner word and is done
// unless it carries this frame's serial (three regions in four at c4; with 16 regions per workgroup, drawn one after the other, the
// kernel took 50 instead of 29 us: a region is three dependent trips to memory).  A wave takes 16 rows, a lane a pixel column (512
// contiguous bytes per row and wave).  The rows' segment marks are read first: a row none of whose segments is marked has not been
// touched since the clear, its keys are kVisClear and the store alone suffices; the marked rows' keys are loaded, all of them in
// flight before the walk uses the first.  (A neighbouring region's workgroup may be marking a shared segment meanwhile: read as 0 or
// as 1, the result is the same -- the neighbour writes none of this region's pixels.)  Plain stores, not non-temporal ones: k_raster_big
// and k_resolve read the keys again soon.  The walk is big_cover_lane (topo_pipeline.h), run lane by lane on the CPU in the tests.
//
// The region's first wave also leaves k_resolve the records of the region's strips (CoverParams::recs): lane s < 8 takes the strip of
// rows 8 s .. 8 s + 7, if it starts inside the target, and evaluates resolve_setup for the owner at the strip's origin -- the function
// and the arguments of k_resolve's record pass for that strip (without its LDS table of the normal decode: normal_channel itself,
// which is what fills the table), so the 34 words are the ones that pass would compute -- and stores them with the owner's id and the
// frame's serial.  It does so in front of everything that can end the wave early; the other three waves go straight to their rows.
// (Kept here, not among k_raster_big's waves that skip a won item: DESIGN 5, "Owned strips".)
__device__ __forceinline__ void cover_strip_record(const FrameParams& P, const CoverParams& C, uint32_t id, uint32_t view, int32_t rx, int32_t ry, uint32_t strip) {
    const int32_t x = rx * 64, y = ry * 64 + (int32_t)(strip * kOwnedStripRows);
    if (strip >= kOwnedStrips || y >= P.H) return;
    const uint32_t draw = id >> 1, fan = id & 1u;
    const uint32_t rank = fastdiv(draw, P.div_tris), tri = draw - rank * P.tris_per_tile;
    const size_t at = owned_record_index(C.regions_x, C.regions_y, view, x, y);
    if (!TOPO_CHK(P.counters, rank < P.n_tiles && at < (size_t)C.cap * kOwnedStrips, 37u, at)) return;
    TriRecord rec;
    resolve_setup<false>(P.tiles[rank], P.tile_w, P.div_hm1, P.tile_h - 1, P.views[view], P.W, P.H, tri, fan, nullptr, x, y, rec);
    uint32_t w[kOwnedRecWords];
    int k = 0;
#define TOPO_X(f) w[k++] = rec.f;
    TOPO_TRIREC_WORDS(TOPO_X)
#undef TOPO_X
    static_assert(kTriRecordWords == (int)kOwnedIdWord && kOwnedSerialWord + 1 == kOwnedRecWords && kOwnedRecWords % 4 == 0, "a record is the TriRecord, the id, the serial");
    w[kOwnedIdWord] = id;
    w[kOwnedSerialWord] = C.serial;
    uint4* const dst = reinterpret_cast<uint4*>(C.recs + at * kOwnedRecWords);
#pragma unroll
    for (int q = 0; q < (int)kOwnedRecWords / 4; ++q) dst[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
}

constexpr int kCoverRows = 16;
__global__ __launch_bounds__(256) void k_raster_cover(FrameParams P, CoverParams C) {
    const uint32_t lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const size_t view_keys = (size_t)P.W * P.H, nseg = ((size_t)P.n_views * view_keys + 63) >> 6;
    (void)nseg;      // (the check build's)
    const uint32_t region = blockIdx.x;      // (the grid is C.cap workgroups)
    const uint64_t word = *const_space(C.owner + region);      // written by k_raster_rare, a launch ago: the scalar data path
    for (bool won = (uint32_t)(word >> 32) == C.serial; won; won = false) {
        const uint32_t item = (uint32_t)word;
        if (!TOPO_CHK(P.counters, region < C.cap && item < P.big_cap, 32u, item)) continue;
        BigItem bi;
        {
            const BigItem& g = P.big[item];
            bi.view = wave_first(g.view); bi.id = wave_first(g.id); bi.region = wave_first(g.region);
#pragma unroll
            for (int k = 0; k < 3; ++k) { bi.X[k] = wave_first(g.X[k]); bi.Y[k] = wave_first(g.Y[k]); bi.z[k] = wave_first(g.z[k]); }
        }
        const uint32_t view = bi.view & ~kBigCovered;
        const int32_t rx = (int32_t)(bi.region & 0xFFFFu), ry = (int32_t)(bi.region >> 16);
        if (!TOPO_CHK(P.counters, (bi.view & kBigCovered) && bi.id != kNoTri && view < P.n_views && rx * 64 < P.W && ry * 64 < P.H &&
                                      cover_region_index(C, view, rx, ry) == region, 33u, bi.region)) continue;
        if (C.recs && wave == 0u) cover_strip_record(P, C, bi.id, view, rx, ry, lane);
        SVert s[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { s[k].X = bi.X[k]; s[k].Y = bi.Y[k]; s[k].z = bi.z[k]; s[k].flag = kVtxOk; }
        TriSetup ts;
        if (!triangle_setup(s[0], s[1], s[2], P.W, P.H, ts)) continue;
        const bool narrow = giant_narrow(bi.X, bi.Y);
        const Vis vis = view_vis(P, view);
        const int32_t row0 = (int32_t)wave * kCoverRows, y0 = ry * 64 + row0, x0 = rx * 64, x1 = min(x0 + 63, P.W - 1);
        if (y0 >= P.H) continue;      // (the region is cut by the image's lower edge above this wave's rows)
        // lane j < 16: the marks of row j's segment(s) -- one, or two when W or the view origin is not a multiple of 64
        const bool row = lane < (uint32_t)kCoverRows && y0 + (int32_t)lane < P.H;
        const size_t first = (size_t)(vis.p - vis.base) + (size_t)(y0 + (int32_t)(row ? lane : 0u)) * P.W;
        const size_t s0 = (first + x0) >> 6, s1 = (first + x1) >> 6;
        const bool row_ok = row && TOPO_CHK(P.counters, s1 < nseg, 34u, s1);
        const bool marked = row_ok && (vis.dirty[s0] | vis.dirty[s1]) != 0;
        const uint32_t marked_rows = (uint32_t)__ballot(marked);      // bit j: row j holds somebody's keys
        const int32_t px = x0 + (int32_t)lane;
        uint64_t old[kCoverRows];
#pragma unroll
        for (int j = 0; j < kCoverRows; ++j) {
            old[j] = kVisClear;
            if ((marked_rows >> j & 1u) && px < P.W) {
                const size_t pix = (size_t)(y0 + j) * P.W + px;
                if (TOPO_CHK(P.counters, y0 + j < P.H && pix < view_keys, 35u, pix)) old[j] = vis.p[pix];
            }
        }
        big_cover_lane<kCoverRows>(ts, narrow, bi.id, P.W, P.H, rx, ry, row0, lane, [&](size_t pix, uint64_t key, int j) {
            if (TOPO_CHK(P.counters, pix < view_keys, 36u, pix)) vis.p[pix] = key < old[j] ? key : old[j];
        });
        if (row_ok) {
            vis.dirty[s0] = 1;
            if (s1 != s0) vis.dirty[s1] = 1;
        }
    }
}

// One wave per BigItem: the item carries the snapped vertices, so every lane re-runs the exact integer setup
// (wave-uniform: the item's fields are forced into scalar registers) and the wave sweeps the part of the triangle's
// pixel box inside the item's 64x64 px region.  Triangles spanning < 64 px (all that k_raster enqueues) take the int32
// form of the same integers (big_medium_lane), the giants that come through k_raster_rare the int64 form
// (big_giant_lane); both are in topo_pipeline.h and run lane by lane on the CPU in the tests.  Fragments are issued
// blind (no depth pre-test, see vis_min): only entries that carry a fragment (key != kVisClear) are dereferenced.
__global__ __launch_bounds__(256) void k_raster_big(FrameParams P, CoverParams C) {
    // Segment marks: an item stays inside one 64 x 64 px region, i.e. inside 64 pixel rows of one or two 64-key segments
    // each.  Instead of one mark store beside every atomic instruction (half of this kernel's memory instructions), the
    // lanes note the rows they hit in LDS and lane r marks row r's segment(s) once per item.
    __shared__ uint8_t s_rows[4][64];
    uint32_t count = P.counters[kCtrBig];
    if (count > P.big_cap) count = P.big_cap;
    const uint32_t lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    s_rows[wave][lane] = 0;
    const uint32_t wave_global = blockIdx.x * 4 + wave, wave_count = gridDim.x * 4;
    for (uint32_t item = P.counters[kCtrBigStart] + wave_global; item < count; item += wave_count) {
        // The item is the same for the whole wave, but the compiler cannot use scalar loads for it (the queue is
        // written by other kernels through the same pointer type): say so field by field, and the integer setup
        // runs on the scalar unit instead of 64 times over on the vector one.
        BigItem bi;
        {
            const BigItem& g = P.big[item];
            bi.view = wave_first(g.view); bi.id = wave_first(g.id); bi.region = wave_first(g.region);
#pragma unroll
            for (int k = 0; k < 3; ++k) { bi.X[k] = wave_first(g.X[k]); bi.Y[k] = wave_first(g.Y[k]); bi.z[k] = wave_first(g.z[k]); }
        }
        if (bi.id == kNoTri) continue;
        const int32_t rx = (int32_t)(bi.region & 0xFFFFu), ry = (int32_t)(bi.region >> 16);
        if (bi.view & kBigCovered) {      // a covering item: if its bid won the region, k_raster_cover has drawn it
            bi.view &= ~kBigCovered;
            const uint32_t r = cover_region_index(C, bi.view, rx, ry);
            if (C.serial != 0u && TOPO_CHK(P.counters, bi.view < P.n_views && rx * 64 < P.W && ry * 64 < P.H && r < C.cap, 31u, r) &&
                *const_space(C.owner + r) == cover_bid(C, item))
                continue;
        }
        const Vis vis = view_vis(P, bi.view);
        if (!TOPO_CHK(P.counters, bi.view < P.n_views && rx * 64 < P.W && ry * 64 < P.H, 11u, bi.region)) continue;
        uint8_t* const rows = s_rows[wave];
        if (spans_fit_int32(bi.X[0], bi.Y[0], bi.X[1], bi.Y[1], bi.X[2], bi.Y[2])) {
            big_medium_lane(bi.X, bi.Y, bi.z, bi.id, P.W, P.H, rx, ry, lane, [&](const uint32_t pix[4], const uint64_t key[4], const int32_t py[4]) {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (key[k] != kVisClear) {
                        vis_min_unmarked(vis, pix[k], key[k]);
                        rows[py[k] & 63] = 1;
                    }
            });
        } else {
            big_giant_lane(bi.X, bi.Y, bi.z, bi.id, P.W, P.H, rx, ry, lane, [&](size_t pix, uint64_t key, int32_t py) {
                vis_min_unmarked(vis, pix, key);
                rows[py & 63] = 1;
            });
        }
        // (LDS operations of one wave complete in order: the notes above are visible to the reads below)
        if (rows[lane]) {
            rows[lane] = 0;
            const int32_t y = ry * 64 + (int32_t)lane, x0 = rx * 64, x1 = min(rx * 64 + 63, P.W - 1);
            const size_t first = (size_t)(vis.p - vis.base) + (size_t)y * P.W;
            const size_t s0 = (first + x0) >> 6, s1 = (first + x1) >> 6;      // a region row lies in one segment, two when W or the view origin is not a multiple of 64
            if (TOPO_CHK(P.counters, y < P.H && s1 < (((size_t)P.n_views * P.W * P.H + 63) >> 6), 14u, s1)) {
                vis.dirty[s0] = 1;
                if (s1 != s0) vis.dirty[s1] = 1;
            }
        }
    }
}

}  // namespace

// The view constants of a submission, from the kernel's own argument segment into the device slot the frame's kernels read: in
// front of a frame whose k_clear_cull does not carry them.  (Outside the anonymous namespace, as it always was: inside, its symbol
// and with it the layout of the code object change.)
__global__ __launch_bounds__(256) void k_put_views(ViewPack pack, uint32_t n_words, uint32_t* __restrict__ dst) {
    static_assert(sizeof(ViewPack) % 4 == 0 && sizeof(ViewPack) / 4 <= 256, "one word per lane");
    const auto src = kernarg<uint32_t>();      // `pack` is the first argument
    if (threadIdx.x < n_words) dst[threadIdx.x] = src[threadIdx.x];
}

}  // namespace topo
