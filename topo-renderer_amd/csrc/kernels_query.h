// kernels_query.h -- queries that read a finished frame's visibility buffer.
//
//   k_viewshed   behind the frame's last k_resolve: the DEM cells that own a pixel, OR-ed into per-tile bit masks
//   k_horizon    per view and column, the topmost pixel that shows terrain, decoded to its tile and cell
//   k_ground     per queried pixel, the terrain point under it (f64: topo_ground.h); k_ground_map: the same for every pixel of whole views
// and the one query over finished IMAGES:
//   k_unwrap     a strip of perspective views resampled into one azimuth / elevation image (f64: topo_unwrap.h)
#pragma once

#include "kernels_common.h"
#include "kernels_ground.h"
#include "topo_ground.h"
#include "topo_unwrap.h"

namespace topo {
namespace {

// Viewshed (topo_viewshed_*): after the frame's last k_resolve, every DEM cell that owns at least one pixel of the visibility
// buffer gets its bit set in the mask of its tile.  A key's low word is draw << 1 | fan (the two halves of a near-clipped triangle),
// draw = rank * tris_per_tile + triangle; bit = cell = triangle >> 1 = x (h-1) + y; masks[rank] is the mask of the tile at that
// rank.  A frame whose rare-triangle queue overflowed is incomplete -- farther triangles won pixels they should not have -- and
// marks nothing.  A wave takes 64 segments at a time (one coalesced read of their marks, as k_clear); unmarked
// segments are sky.  Of each marked segment's 64 keys, a run of neighbouring lanes that hit the same mask word is combined into its
// last lane (a segmented OR over as many doubling steps as the longest run needs), and only that lane updates the word: a load,
// and the atomicOr only when it would set a bit (issued blind, the atomics cost 6x as much at c4: DESIGN.md §5,
// tools/experiments/viewshed_blind_atomics_experiment.patch).  kBatch segments are taken at once so that their key loads -- and
// then their mask loads -- are in flight together.
// stats (per workgroup, 4 words): [0] terrain keys, [1] combined updates (run tails), [2] atomics issued.
__global__ __launch_bounds__(256) void k_viewshed(FrameParams P, uint32_t* const* __restrict__ masks, unsigned long long* __restrict__ stats) {
    if (P.counters[kCtrStatus] & kStatusRareOverflow) return;
    constexpr int kBatch = 4;
    constexpr uint32_t kSky = 0xFFFFFFFFu;
    const uint32_t lane = threadIdx.x & 63;
    const size_t n = (size_t)P.n_views * P.W * P.H, nseg = (n + 63) >> 6;
    const size_t wave = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwave = (size_t)gridDim.x * 4;
    const uint32_t cells = P.tris_per_tile >> 1, words = (cells + 31) >> 5;
    uint64_t n_keys = 0, n_tails = 0, n_atomics = 0;
    for (size_t g = wave * 64; g < nseg; g += nwave * 64) {
        uint64_t todo = __ballot(g + lane < nseg && P.dirty[g + lane] != 0);
        while (todo) {
            uint32_t t[kBatch], rank[kBatch], word[kBatch], bit[kBatch], cur[kBatch];
            uint64_t heads[kBatch];
            bool tail[kBatch];
#pragma unroll
            for (int b = 0; b < kBatch; ++b) {
                t[b] = kSky;
                if (todo) {
                    const size_t at = (g + (size_t)__builtin_ctzll(todo)) * 64 + lane;
                    todo &= todo - 1;
                    if (at < n) t[b] = (uint32_t)P.vis[at];      // the key's low word: draw << 1 | fan
                }
            }
#pragma unroll
            for (int b = 0; b < kBatch; ++b) {
                rank[b] = 0; word[b] = 0; bit[b] = 0;
                if (t[b] != kSky) {
                    const uint32_t draw = t[b] >> 1;
                    rank[b] = fastdiv(draw, P.div_tris);
                    const uint32_t cell = (draw - rank[b] * P.tris_per_tile) >> 1;
                    word[b] = cell >> 5;
                    bit[b] = 1u << (cell & 31u);
                    t[b] = rank[b] * words + word[b];      // the run key: one mask word of one tile (< 2^26: ids are < 2^31)
                }
                n_keys += (uint64_t)__popcll(__ballot(t[b] != kSky));
                const uint32_t prev = __shfl_up(t[b], 1);
                heads[b] = __ballot(lane == 0 || prev != t[b]);
                // The OR takes a lane d back whenever it holds the same word, with no segment flag: a run is contiguous, so a lane of
                // ANOTHER run with the same word (A B A) only adds bits of that same word -- still right for the word the tail updates --
                // and every lane of the tail's own run is reached, because a step's source lane outside the run has nothing of the run
                // behind it either.
                uint64_t need = ~heads[b];      // lanes whose run reaches back further than the bits gathered so far
                for (uint32_t d = 1; need; d <<= 1) {
                    const uint32_t tp = __shfl_up(t[b], d), bp = __shfl_up(bit[b], d);
                    if (lane >= d && tp == t[b]) bit[b] |= bp;      // (a lane further back with the same word: its bits belong there too)
                    need &= need << d;
                }
                tail[b] = t[b] != kSky && (lane == 63 || ((heads[b] >> (lane + 1)) & 1u));
                n_tails += (uint64_t)__popcll(__ballot(tail[b]));
                // (the table index is tested in the product build too: what it reads is a pointer)
                if (tail[b] && !(TOPO_CHK(P.counters, rank[b] < P.n_tiles && word[b] < words, 16u, t[b]) && rank[b] < P.n_tiles && word[b] < words))
                    tail[b] = false;
            }
#pragma unroll
            for (int b = 0; b < kBatch; ++b) cur[b] = tail[b] ? masks[rank[b]][word[b]] : 0u;
#pragma unroll
            for (int b = 0; b < kBatch; ++b) {
                const bool issue = tail[b] && (cur[b] & bit[b]) != bit[b];
                n_atomics += (uint64_t)__popcll(__ballot(issue));
                if (issue) atomicOr(&masks[rank[b]][word[b]], bit[b]);
            }
        }
    }
    if (lane == 0 && n_keys) {      // (n_keys == 0: nothing else is either)
        unsigned long long* s = stats + (size_t)blockIdx.x * 4;
        atomicAdd(&s[0], (unsigned long long)n_keys);
        atomicAdd(&s[1], (unsigned long long)n_tails);
        atomicAdd(&s[2], (unsigned long long)n_atomics);
    }
}

// One horizon record, as two 16-byte vector stores.
__device__ __forceinline__ void horizon_store(HorizonPoint* dst, int32_t row, uint32_t depth_bits, int32_t lat, int32_t lon, uint32_t cx, uint32_t cy,
                                              uint32_t fan) {
    int4* d = reinterpret_cast<int4*>(dst);
    d[0] = make_int4(row, (int32_t)depth_bits, lat, lon);
    d[1] = make_int4((int32_t)cx, (int32_t)cy, (int32_t)fan, 0);
}

// Horizon (topo_horizon_*): for every column of every queried view of a finished submission, the topmost pixel whose key names a
// triangle (the smallest row whose low word is not kNoTri), and what it shows: the key's depth, the tile (rank -> (lat, lon) in the
// submission's tile order) and the cell (draw = rank * tris_per_tile + tri, cell = tri >> 1 = x (h-1) + y, as k_viewshed decodes it).
// Launched by the query on the submission's stream, behind it; it reads the keys, the marks and the status word and writes only
// `out` (the next k_clear trusts the marks).  A frame whose rare-triangle queue overflowed is incomplete: every record reads row -2.
// One wave per (view, 64-column group), a lane per column; no column is walked row by row from the top.  A step takes the marks of
// kWin x 64 rows at once (lane l: row y0 + 64 j + l, both segments the group's <= 64 keys of that row can touch) and ballots them into
// row masks: an unmarked segment holds only kVisClear, so a row without a mark is sky for the whole group.  The marked rows then go
// in ascending order, kBatch at a time with their key loads in flight together, until every lane has found terrain or the rows run
// out.  Linear indices are 64-bit: a submission holds up to 2^32 - 1 keys.
__global__ __launch_bounds__(256) void k_horizon(HorizonParams P) {
    constexpr int kWin = 4, kBatch = 8;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t groups = (P.W + 63) >> 6;
    const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wave >= (uint64_t)groups * P.n_views) return;      // (whole waves)
    const uint32_t v = (uint32_t)(wave / groups), x0 = (uint32_t)(wave - (uint64_t)v * groups) * 64;
    const uint32_t ncols = P.W - x0 < 64u ? P.W - x0 : 64u;
    const bool valid = lane < ncols;
    HorizonPoint* const dst = P.out + (size_t)v * P.view_stride + x0 + lane;
    if (P.counters[kCtrStatus] & kStatusRareOverflow) {
        if (valid) horizon_store(dst, -2, 0u, 0, 0, 0u, 0u, 0u);
        return;
    }
    const size_t vbase = (size_t)(P.first_view + v) * P.W * P.H + x0;      // the key of (row 0, column x0) of the view
    [[maybe_unused]] const size_t nseg = (P.n_keys + 63) >> 6;      // (the check build's bound)
    const uint64_t* const col = P.vis + vbase + lane;
    uint64_t key = kVisClear;
    int32_t row = -1;
    bool searching = valid;
    for (uint32_t y0 = 0; y0 < P.H && __ballot(searching); y0 += 64 * kWin) {
        uint64_t rows[kWin];
#pragma unroll
        for (int j = 0; j < kWin; ++j) {
            const uint32_t y = y0 + 64 * j + lane;
            bool m = false;
            if (y < P.H) {
                const size_t a = vbase + (size_t)y * P.W, sa = a >> 6, sb = (a + ncols - 1) >> 6;
                if (TOPO_CHK(P.check, sb < nseg, 17u, sb)) m = (P.dirty[sa] | P.dirty[sb]) != 0;
            }
            rows[j] = __ballot(m);
        }
#pragma unroll
        for (int j = 0; j < kWin; ++j) {
            uint64_t todo = rows[j];
            while (todo && __ballot(searching)) {
                uint32_t r[kBatch];
                uint64_t k[kBatch];
#pragma unroll
                for (int b = 0; b < kBatch; ++b) {
                    r[b] = todo ? y0 + 64 * j + (uint32_t)__builtin_ctzll(todo) : P.H;      // (P.H: no row left)
                    todo &= todo - 1;
                }
#pragma unroll
                for (int b = 0; b < kBatch; ++b) {
                    const size_t at = (size_t)r[b] * P.W;
                    k[b] = searching && r[b] < P.H && TOPO_CHK(P.check, vbase + lane + at < P.n_keys, 17u, vbase + lane + at) ? col[at] : kVisClear;
                }
#pragma unroll
                for (int b = 0; b < kBatch; ++b)
                    if (searching && (uint32_t)k[b] != kNoTri) {      // (rows ascend within the batch: the first hit is the topmost)
                        key = k[b];
                        row = (int32_t)r[b];
                        searching = false;
                    }
            }
        }
    }
    if (!valid) return;
    if (row < 0) {
        horizon_store(dst, -1, (uint32_t)(kVisClear >> 32), 0, 0, 0u, 0u, 0u);      // sky: depth 1.0
        return;
    }
    const uint32_t id = (uint32_t)key, draw = id >> 1;
    const uint32_t rank = fastdiv(draw, P.div_tris), cell = (draw - rank * P.tris_per_tile) >> 1;
    const uint32_t cx = fastdiv(cell, P.div_hm1), cy = cell - cx * P.hm1;
    int32_t lat = 0, lon = 0;
    // (the rank is tested in the product build too: what it indexes is a table)
    if (TOPO_CHK(P.check, rank < P.n_tiles, 17u, id) && rank < P.n_tiles) {
        lat = P.tile_ll[2 * (size_t)rank];
        lon = P.tile_ll[2 * (size_t)rank + 1];
    }
    horizon_store(dst, row, (uint32_t)(key >> 32), lat, lon, cx, cy, id & 1u);
}

// ---- ground (topo_ground_*) --------------------------------------------------------------------------------------------------
// The terrain point under a pixel of a finished submission.  The pixel's key names its winning triangle (decoded as k_horizon decodes
// it); the triangle's three vertex texels (triangle_vertices) get their heights from the tile's resident DEM and the sin / cos of
// their longitude and latitude from the tiles' f64 tables (k_ground_tables); ground_solve (topo_ground.h, f64 throughout) finds the
// point of the triangle's plane that the view maps to the pixel centre.  Launched by the query on the submission's stream, behind it;
// the kernels read the keys, the marks, the status word, the tile table, the DEMs and the tables and write only their output.  Both
// kernels answer a pixel through ground_answer (kernels_ground.h: device helpers, no kernel, shared with kernels_rays.h): with
// -ffp-contract=off the list and the map agree bit for bit.
// The tiles' f64 (cos, sin) tables (ground_table_doubles each, draw order): a lane per column or row, once per tile set.
__global__ __launch_bounds__(256) void k_ground_tables(const TileDev* __restrict__ tiles, double* __restrict__ trig, uint32_t w, uint32_t h) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= w + h) return;
    const TileDev& t = tiles[blockIdx.y];
    double c, s;
    if (i < w) ground_trig_lon(t, i, c, s);
    else ground_trig_lat(t, i - w, c, s);
    *reinterpret_cast<double2*>(trig + (size_t)blockIdx.y * ground_table_doubles(w, h) + 2 * (size_t)i) = make_double2(c, s);
}

// One ground record, as four 16-byte vector stores.  Only a terrain record carries a position; a degenerate one keeps what the key
// itself says (depth, tile, cell, triangle).
__device__ __forceinline__ void ground_store(GroundPoint* dst, const GroundAnswer& a, uint32_t depth_bits) {
    int4* d = reinterpret_cast<int4*>(dst);
    const bool pos = a.kind == kGroundTerrain;
    const double lon = pos ? a.r.lon_deg : 0.0, lat = pos ? a.r.lat_deg : 0.0;
    const float h = pos ? (float)a.r.height : 0.0f, rg = pos ? (float)a.r.range : 0.0f;
    const float w1 = pos ? (float)a.r.w1 : 0.0f, w2 = pos ? (float)a.r.w2 : 0.0f;
    d[0] = make_int4(__double2loint(lon), __double2hiint(lon), __double2loint(lat), __double2hiint(lat));
    d[1] = make_int4(__float_as_int(h), __float_as_int(rg), (int32_t)depth_bits, a.kind);
    d[2] = make_int4(a.lat, a.lon, (int32_t)a.t.cell_x, (int32_t)a.t.cell_y);
    d[3] = make_int4((int32_t)(a.t.tri & 1u), (int32_t)a.t.fan, __float_as_int(w1), __float_as_int(w2));
}

// The list form: one lane per query.  A query outside the submission (the host variant has refused those) reads nothing and
// answers kind -1; a submission whose rare-triangle queue overflowed is incomplete: kind -2.
__global__ __launch_bounds__(256) void k_ground(GroundParams P, const GroundQuery* __restrict__ queries, GroundPoint* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const GroundQuery q = queries[i];
    GroundAnswer a{};
    if (P.q.counters[kCtrStatus] & kStatusRareOverflow) {
        a.kind = kGroundIncomplete;
        ground_store(out + i, a, 0u);
        return;
    }
    if (q.view >= P.sub_views || q.x >= P.q.W || q.y >= P.q.H) {
        a.kind = kGroundOutside;
        ground_store(out + i, a, 0u);
        return;
    }
    const size_t at = ((size_t)q.view * P.q.H + q.y) * P.q.W + q.x;
    const uint64_t key = TOPO_CHK(P.q.check, at < P.q.n_keys, 18u, at) ? P.q.vis[at] : kVisClear;
    a = ground_answer(P, key, q.view, q.x, q.y);
    ground_store(out + i, a, (uint32_t)(key >> 32));
}

// The dense form: float4 (lon, lat, height, range) -- each the f64 value rounded once -- for every pixel of views
// [first_view, first_view + n_views), four quiet NaNs where there is no terrain point (sky, degenerate, incomplete frame).  One wave
// per 64-key segment of the visibility buffer, grid-stride; a segment without a mark holds only sky and costs no key load, only the
// 64 coalesced 16-byte stores -- non-temporal: nothing here reads them again.  Linear key indices are 64-bit (a submission holds up
// to 2^32 - 1 keys, so the index of one view's pixel fits 32 bits for the divisions).
__global__ __launch_bounds__(256) void k_ground_map(GroundParams P, uint8_t* __restrict__ out, size_t view_stride, size_t pitch) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwave = (uint64_t)gridDim.x * 4;
    const uint64_t view_keys = (uint64_t)P.q.W * P.q.H;
    const uint64_t k0 = P.q.first_view * view_keys, k1 = k0 + P.q.n_views * view_keys;
    const bool incomplete = (P.q.counters[kCtrStatus] & kStatusRareOverflow) != 0;
    [[maybe_unused]] const uint64_t nseg = ((uint64_t)P.q.n_keys + 63) >> 6;      // (the check build's bound)
    const uint32_t qnan = 0x7FC00000u;
    for (uint64_t seg = (k0 >> 6) + wave; seg * 64 < k1; seg += nwave) {
        const uint64_t k = seg * 64 + lane;
        if (k < k0 || k >= k1) continue;
        const bool marked = !incomplete && TOPO_CHK(P.q.check, seg < nseg, 18u, seg) && P.q.dirty[seg] != 0;
        const uint64_t key = marked && TOPO_CHK(P.q.check, k < P.q.n_keys, 18u, k) ? P.q.vis[k] : kVisClear;
        const uint32_t v = (uint32_t)k / (uint32_t)view_keys, rem = (uint32_t)k - v * (uint32_t)view_keys;      // (k < 2^32)
        const uint32_t y = rem / P.q.W, x = rem - y * P.q.W;
        u32x4_t val = {qnan, qnan, qnan, qnan};
        if ((uint32_t)key != kNoTri) {
            const GroundAnswer a = ground_answer(P, key, v, x, y);
            if (a.kind == kGroundTerrain) {
                val.x = __float_as_uint((float)a.r.lon_deg);
                val.y = __float_as_uint((float)a.r.lat_deg);
                val.z = __float_as_uint((float)a.r.height);
                val.w = __float_as_uint((float)a.r.range);
            }
        }
        uint8_t* const dst = out + (size_t)(v - P.q.first_view) * view_stride + (size_t)y * pitch + (size_t)x * 16;
        __builtin_nontemporal_store(val, reinterpret_cast<u32x4_t*>(dst));
    }
}

// ---- unwrap (topo_unwrap_*) ---------------------------------------------------------------------------------------------------
// Views that share an eye, resampled into one image whose columns are linear in azimuth and whose rows are linear in elevation (or
// its tangent): topo_unwrap.h has the mapping, the seam rule and the tables.  A workgroup takes 256 columns of four rows, a wave one
// of the rows, a lane four consecutive pixels of it: the row's (cos, sin), up and the views' matrices are wave-uniform and come over
// the scalar path (the tables were written by an earlier copy: constant address space), the four columns' h vectors are six 16-byte
// loads, and each output is one 16-byte non-temporal store per lane (nothing here reads them again); a ragged last group of a row
// stores its pixels one by one.  Neighbouring output pixels read neighbouring source texels, row by row of the source.
// The views' cw rows are applied to all four pixels view by view; the winner's rows 0 and 1 are then fetched once per view that
// won a pixel of the wave (one or two of them: a wave spans at most 256 columns), still as scalars.  Only a pixel its nearest-axis
// view does not contain (beyond the vertical field of view, a gap of a pitched panorama) takes unwrap_scan.
template <bool kBilinear>
__global__ __launch_bounds__(256) void k_unwrap(UnwrapParams P) {
    [[maybe_unused]] __shared__ float s_thresh[256], s_decode[256];
    if constexpr (kBilinear) {
        if (P.srgb) {
            s_thresh[threadIdx.x] = bits_f(TOPO_SRGB_THRESH_BITS[threadIdx.x]);
            s_decode[threadIdx.x] = bits_f(TOPO_SRGB_DECODE_BITS[threadIdx.x]);
            __syncthreads();
        }
    }
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t by = blockIdx.x / P.blocks_x, bx = blockIdx.x - by * P.blocks_x;
    const uint32_t r = wave_first(by * 4 + (threadIdx.x >> 6));
    const uint32_t c0 = (bx * 64 + lane) * 4;
    if (r >= P.out_h || c0 >= P.out_w) return;
    const auto tab = const_space(P.tab);
    const auto views = tab + kUnwrapViewsAt;
    const size_t row_at = unwrap_rows_at(P.n_views, P.out_w) + 2 * (size_t)r;
    const double ce = tab[row_at], se = tab[row_at + 1];
    const double up[3] = {tab[0], tab[1], tab[2]};
    // (c0 + 3 is inside the padded column table: the host sizes it to a multiple of four columns)
    const double2* const hc = reinterpret_cast<const double2*>(P.tab + unwrap_cols_at(P.n_views) + 3 * (size_t)c0);
    double2 hv[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) hv[i] = hc[i];
    const double hs[12] = {hv[0].x, hv[0].y, hv[1].x, hv[1].y, hv[2].x, hv[2].y, hv[3].x, hv[3].y, hv[4].x, hv[4].y, hv[5].x, hv[5].y};
    double d[4][3], best[4];
    uint32_t kb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        unwrap_dir(ce, se, hs + 3 * j, up, d[j]);
        best[j] = unwrap_row(views + 6, d[j]);
        kb[j] = 0;
    }
    for (uint32_t k = 1; k < P.n_views; ++k) {
        const auto m = views + (size_t)kUnwrapViewDoubles * k + 6;
        const double m0 = m[0], m1 = m[1], m2 = m[2];
        const double row[3] = {m0, m1, m2};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double cw = unwrap_row(row, d[j]);
            if (cw > best[j]) { best[j] = cw; kb[j] = k; }
        }
    }
    UnwrapSource src[4];
    bool found[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        src[j] = UnwrapSource{(int32_t)kb[j], 0.0, 0.0};
        found[j] = false;
    }
    // the winners' rows 0 and 1: once per view that won a pixel of the wave
    for (uint32_t k = 0; k < P.n_views; ++k) {
        bool mine[4];
        bool any = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            mine[j] = kb[j] == k;
            any |= mine[j];
        }
        if (!__ballot(any)) continue;
        const auto m = views + (size_t)kUnwrapViewDoubles * k;
        const double mm[6] = {m[0], m[1], m[2], m[3], m[4], m[5]};
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (mine[j]) found[j] = unwrap_project(mm, d[j], best[j], P.src_w, P.src_h, src[j].px, src[j].py);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (!found[j]) src[j] = unwrap_scan(views, P.n_views, P.src_w, P.src_h, d[j]);

    u32x4_t rgba = {0u, 0u, 0u, 0u}, depth = {kUnwrapNoDepthBits, kUnwrapNoDepthBits, kUnwrapNoDepthBits, kUnwrapNoDepthBits};
    u32x4_t smap = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (src[j].view < 0) continue;
        const uint32_t v = (uint32_t)src[j].view, sx = (uint32_t)floor(src[j].px), sy = (uint32_t)floor(src[j].py);
        // (the product build trusts unwrap_project's containment test; the check build tests what it yields)
        if (!TOPO_CHK(P.check, v < P.n_views && sx < P.src_w && sy < P.src_h, 19u, ((uint64_t)v << 48) | ((uint64_t)sy << 24) | sx)) continue;
        smap[j] = (uint32_t)unwrap_source_index(v, sx, sy, P.src_w, P.src_h);
        if (P.depth_out) depth[j] = *reinterpret_cast<const uint32_t*>(P.depth_src + (size_t)v * P.depth_view_stride + (size_t)sy * P.depth_pitch + (size_t)sx * 4);
        if (!P.rgba_out) continue;
        const uint8_t* const img = P.rgba_src + (size_t)v * P.rgba_view_stride;
        if constexpr (kBilinear) {
            const UnwrapTaps t = unwrap_taps(src[j].px, src[j].py, P.src_w, P.src_h);
            if (!TOPO_CHK(P.check, t.x[0] < P.src_w && t.x[1] < P.src_w && t.y[0] < P.src_h && t.y[1] < P.src_h && t.fx < 256u && t.fy < 256u, 19u,
                          ((uint64_t)t.y[1] << 32) | t.x[1]))
                continue;
            const uint8_t* const r0 = img + (size_t)t.y[0] * P.rgba_pitch, * const r1 = img + (size_t)t.y[1] * P.rgba_pitch;
            const uint32_t t00 = *reinterpret_cast<const uint32_t*>(r0 + (size_t)t.x[0] * 4), t10 = *reinterpret_cast<const uint32_t*>(r0 + (size_t)t.x[1] * 4);
            const uint32_t t01 = *reinterpret_cast<const uint32_t*>(r1 + (size_t)t.x[0] * 4), t11 = *reinterpret_cast<const uint32_t*>(r1 + (size_t)t.x[1] * 4);
            rgba[j] = unwrap_blend(t00, t10, t01, t11, t.fx, t.fy, P.srgb != 0u, s_thresh, s_decode);
        } else {
            rgba[j] = *reinterpret_cast<const uint32_t*>(img + (size_t)sy * P.rgba_pitch + (size_t)sx * 4);
        }
    }
    if (!TOPO_CHK(P.check, r < P.out_h && c0 < P.out_w, 19u, ((uint64_t)r << 32) | c0)) return;
    const bool whole = c0 + 4 <= P.out_w;
    auto put = [&](uint8_t* base, size_t pitch, const u32x4_t& val) {
        if (!base) return;
        uint8_t* const dst = base + (size_t)r * pitch + (size_t)c0 * 4;
        if (whole) {
            __builtin_nontemporal_store(val, reinterpret_cast<u32x4_t*>(dst));
        } else {
#pragma unroll
            for (int j = 0; j < 3; ++j)      // (a ragged group holds one to three pixels)
                if (c0 + j < P.out_w) reinterpret_cast<uint32_t*>(dst)[j] = val[j];
        }
    };
    put(P.rgba_out, P.rgba_out_pitch, rgba);
    put(P.depth_out, P.depth_out_pitch, depth);
    put(P.src_out, P.src_out_pitch, smap);
}

}  // namespace
}  // namespace topo
