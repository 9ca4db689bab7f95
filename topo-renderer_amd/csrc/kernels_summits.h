// kernels_summits.h -- the summits of the drawn mesh and the snapping of peaks to them (topo_summits.hip: a translation unit of its
// own, as topo_surface.hip, so that every other unit's code stays exactly what it was).  The rule is topo_summits.h.
//
// A band is up to band_rows vertex rows of one tile; a call works through the tiles' bands in tile order, and each band goes through
//
//   k_summit_candidates   a lane per post, a wave per 64 columns of a row: streams the DEM once.  A lane loads its column of the rows
//                         above, at and below (three coalesced row reads per wave), takes the columns left and right from its
//                         neighbour lanes (DPP shifts; lanes 0 and 63 load theirs) and drops the post iff it does not exist, lies
//                         under min_height_m or an in-tile 8-neighbour dominates it nearer than min_isolation_m
//                         (summit_neighbour_rejects' test on the staged heights).  Per wave: the ballot and its count.
//   k_summit_scan         one workgroup: the waves' counts into exclusive offsets, the total into the band's state
//   k_summit_scatter      a lane per ballot bit: the survivors' post indices into the list, at offset + rank within the ballot --
//                         ascending (row, column): tile order, with no sort and no order-bearing atomic
//   k_summit_reject       a wave per candidate: any dominator within min_isolation_m (d <)?  Any-hit, as wave_any_hit is for rays:
//                         per tile the window, its blocks 64 at a time by block_minmax, the surviving blocks' posts dealt to the
//                         lanes, the block rows nearest the centre first; the first ballot with a hit ends the candidate.  A byte
//                         per candidate.
//   k_summit_flags        a lane per candidate: the bytes into ballots and counts; k_summit_scan again
//   k_summit_append       a lane per ballot bit: the band's summits, numbered from the running offset; the first `capacity` of the
//                         call leave (tile rank, post index) in their record
// and once, behind the last band,
//   k_summit_isolation    a wave per recorded summit: the nearest dominator within radius_m.  Closest-hit: lane-private bests, a
//                         wave-min on (distance, rank, index) after every batch of blocks, and the window shrunk to the best
//                         distance so far (topo_summits.h argues why that loses nothing).  Overwrites the record with its values.
//                         (Measured on c4: launched per band -- some 95 waves a tile, each walking 18 000 posts on its own -- the
//                         100 launches took 23.7 ms one after the other; the one launch of 9493 waves takes 0.97 ms.)
//
// The candidates live in scratch sized for one band (SummitScratch); the running offset and the counts stay on the device (state[]),
// so a device call never waits.  Every index goes through TOPO_CHK (tags 40 .. 44); those into the scratch lists are checked against
// the sizes the lists were allocated with (SummitScratch::posts, ::waves), not against the launch's own shape.  Nothing depends on
// the banding: the prefilter reads the rows around a post wherever the band ends, and a summit's number is the running count.
//   k_summit_snap         a wave per point: the same window and block walk with a wave-max on (h, -distance, rank, index), blocks
//                         rejected when their max < the best height so far.
#pragma once

#include "kernels_common.h"
#include "topo_summits.h"

namespace topo {
namespace {

// The wave's best of the lanes' bests, in every lane (both lanes of a pair choose the same winner: the orders are total).
__device__ __forceinline__ void wave_summit_best(SummitBest& b, bool snap) {
#pragma unroll
    for (int s = 32; s; s >>= 1) {
        SummitBest o;
        o.d = shfl_xor_f64(b.d, s);
        o.rank = (uint32_t)__shfl_xor((int)b.rank, s);
        o.idx = (uint32_t)__shfl_xor((int)b.idx, s);
        o.h = __shfl_xor(b.h, s);
        o.found = __shfl_xor((int)b.found, s) != 0;
        summit_merge(b, o, snap);
    }
}

// Block row j of n in the order nearest `mid` first: mid, mid + 1, mid - 1, ... and, once one side is used up, the rest of the other.
__device__ __forceinline__ uint32_t summit_row_order(uint32_t j, uint32_t lo, uint32_t hi, uint32_t mid) {
    const uint32_t up = hi - mid, dn = mid - lo, m = up < dn ? up : dn;
    if (j == 0) return mid;
    if (j <= 2 * m) return (j & 1u) ? mid + (j + 1) / 2 : mid - j / 2;
    return up > dn ? mid + (j - dn) : mid - (j - up);
}

enum SummitWalk { kWalkAny, kWalkNearest, kWalkSnap };

// The walk of one wave over the resident tiles around the centre (lon, lat) with direction uc.  kWalkAny / kWalkNearest: the
// dominators of P = (hp, rank_p, idx_p) within `radius` (kWalkAny: d < radius, and any one ends the walk); kWalkSnap: the snap
// target.  Returns the wave's best in every lane.
template <SummitWalk kMode>
__device__ __forceinline__ SummitBest wave_summit_walk(const RayParams& P, float hp, uint32_t rank_p, uint32_t idx_p, const double uc[3], double lon, double lat, double radius,
                                                       uint32_t lane, uint32_t tag) {
    const LosScene& S = P.s;
    auto chk = [&](bool ok, uint64_t value) { return TOPO_CHK(P.check, ok, tag, value); };
    SummitBest best{0.0, 0u, 0u, 0.0f, false};      // the lane's own between two reductions
    double reach = radius;
    bool have = false;      // wave-uniform: `best` held a post at the last reduction
    float have_h = 0.0f;
    for (uint32_t rank = 0; rank < S.n_tiles; ++rank) {
        const TileDev& t = S.tiles[rank];
        SummitWindow w = summit_window(S, t, lon, lat, reach);
        if (!w.any || S.bx_count == 0 || S.by_count == 0) continue;
        const uint32_t bx0 = summit_block_of(w.x0, kLosBCX, S.bx_count), bx1 = summit_block_of(w.x1, kLosBCX, S.bx_count);
        const uint32_t by0 = summit_block_of(w.y0, kLosBCY, S.by_count), by1 = summit_block_of(w.y1, kLosBCY, S.by_count);
        const uint32_t nbx = bx1 - bx0 + 1, nblk = nbx * (by1 - by0 + 1), mid = summit_block_of((w.y0 + w.y1) / 2, kLosBCY, S.by_count);
        for (uint32_t base = 0; base < nblk; base += 64) {
            const uint32_t j = base + lane;
            bool take = j < nblk;
            if (take) {
                const uint32_t by = summit_row_order(j / nbx, by0, by1, mid), bx = bx0 + j % nbx;
                const uint32_t blk = by * S.bx_count + bx;
                if (kMode == kWalkSnap) take = !(have && summit_block_below(S, t, blk, have_h, chk));
                else take = !summit_block_below(S, t, blk, hp, chk);
            }
            uint64_t mask = __ballot(take);
            while (mask) {
                const uint32_t jb = base + pop_bit(mask);
                const uint32_t by = summit_row_order(jb / nbx, by0, by1, mid), bx = bx0 + jb % nbx;
                uint32_t x0, x1, y0, y1;
                summit_block_span(bx, kLosBCX, S.bx_count, S.tile_w, w.x0, w.x1, x0, x1);
                summit_block_span(by, kLosBCY, S.by_count, S.tile_h, w.y0, w.y1, y0, y1);
                if (!w.any || x0 > x1 || y0 > y1) continue;
                const uint32_t nx = x1 - x0 + 1, n = nx * (y1 - y0 + 1);
                for (uint32_t k0 = 0; k0 < n; k0 += 64) {
                    const uint32_t k = k0 + lane;
                    if (k < n) {
                        const uint32_t ry = k / nx, vx = x0 + (k - ry * nx), vy = y0 + ry;
                        if (kMode == kWalkSnap) summit_try_snap(S, t, rank, vx, vy, uc, radius, best, chk);
                        else summit_try_dominator(S, t, rank, vx, vy, hp, rank_p, idx_p, uc, radius, kMode == kWalkAny, best, chk);
                    }
                }
                if (kMode == kWalkAny && __ballot(best.found)) {
                    wave_summit_best(best, false);
                    return best;
                }
            }
            if (kMode != kWalkAny) {
                wave_summit_best(best, kMode == kWalkSnap);
                have = best.found;
                have_h = best.h;
                if (kMode == kWalkNearest && best.found && best.d < reach) {
                    reach = best.d;
                    w = summit_window_cut(w, summit_window(S, t, lon, lat, reach));
                }
            }
        }
    }
    return best;
}

// ---- stage 1: the candidates of a band ------------------------------------------------------------------------------------------

// Wave `wave` of the band is columns 64 c .. 64 c + 63 of row y0 + r with r = wave / waves_per_row, c = wave % waves_per_row.
__global__ __launch_bounds__(256) void k_summit_candidates(RayParams P, double min_isolation, float min_height, uint32_t rank, uint32_t y0, uint32_t rows,
                                                           uint32_t waves_per_row, uint64_t* __restrict__ wave_mask, uint32_t* __restrict__ wave_count, uint32_t wave_cap) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = wave_first(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (wave >= rows * waves_per_row) return;
    const LosScene& S = P.s;
    const uint32_t W = S.tile_w, H = S.tile_h;
    const uint32_t r = wave / waves_per_row, vy = y0 + r, x = (wave - r * waves_per_row) * 64u + lane;
    if (!(TOPO_CHK(P.check, rank < S.n_tiles && vy < H, 40u, ((uint64_t)rank << 32) | vy) && rank < S.n_tiles && vy < H)) return;
    const TileDev& t = S.tiles[rank];
    const auto hts = TOPO_GLOBAL_F32(t.heights);
    const bool in = x < W;
    const float nan = __builtin_nanf("");
    const size_t n_posts = (size_t)W * H;
    auto height = [&](bool want, size_t i) { return want && TOPO_CHK(P.check, i < n_posts, 40u, i) && i < n_posts ? hts[i] : nan; };
    float left[3], mine[3], right[3];      // rows vy - 1, vy, vy + 1; a quiet NaN where the tile has no post
#pragma unroll
    for (uint32_t k = 0; k < 3; ++k) {
        const uint32_t y = vy + k - 1;      // (wraps below row 0)
        const bool row = y < H;
        const size_t at = (size_t)(row ? y : vy) * W;
        mine[k] = height(in && row, at + x);
        const float first = height(lane == 0 && row && x > 0 && in, at + x - 1);
        const float last = height(lane == 63 && row && x + 1 < W, at + x + 1);
        left[k] = wave_from_left(mine[k], first);
        right[k] = wave_from_right(mine[k], last);
    }
    const float hp = mine[1];
    bool keep = in && surface_tile_ok(t) && surface_height_ok(hp) && hp >= min_height;
    if (keep && min_isolation > 0.0) {
        auto chk = [&](bool ok, uint64_t value) { return TOPO_CHK(P.check, ok, 40u, value); };
        const uint32_t idx_p = vy * W + x;
        const bool all_near = min_isolation > summit_neighbour_reach(t);      // wave-uniform: every dominating neighbour is nearer (topo_summits.h)
        double up[3] = {0.0, 0.0, 0.0};
        if (!all_near) keep = summit_direction(S, rank, x, vy, up, chk);
#pragma unroll
        for (uint32_t k = 0; k < 3; ++k)
#pragma unroll
            for (uint32_t c = 0; c < 3; ++c) {
                if (c == 1 && k == 1) continue;
                const float hq = c == 0 ? left[k] : (c == 1 ? mine[k] : right[k]);
                const uint32_t qx = x + c - 1, qy = vy + k - 1;
                if (!keep || !surface_height_ok(hq) || qx >= W || qy >= H || !summit_dominates(hq, rank, qy * W + qx, hp, rank, idx_p)) continue;
                if (all_near) {
                    keep = false;
                    continue;
                }
                double uq[3];
                if (!summit_direction(S, rank, qx, qy, uq, chk)) continue;
                if (summit_chord(up, uq) < min_isolation) keep = false;
            }
    }
    const uint64_t mask = __ballot(keep);
    if (lane == 0 && TOPO_CHK(P.check, wave < wave_cap, 40u, wave) && wave < wave_cap) {
        wave_mask[wave] = mask;
        wave_count[wave] = (uint32_t)__popcll(mask);
    }
}

// One workgroup of 1024: counts[0 .. n) into their exclusive prefix sums, in place; the total into state[slot].  n = n_waves, or the
// waves of *n_items (64 items each), and at most the cap entries counts has room for.  advance: the band is complete -- state[base] = state[total], state[total] += the band's count.
__global__ __launch_bounds__(1024) void k_summit_scan(uint32_t* __restrict__ counts, uint32_t n_waves, const uint32_t* __restrict__ n_items, uint32_t cap, uint32_t* __restrict__ state,
                                                     uint32_t slot, uint32_t advance, uint32_t* check) {
    __shared__ uint32_t part[1024];
    uint32_t n = n_items ? (*n_items + 63u) / 64u : n_waves;
    n = n < cap ? n : cap;
    const uint32_t per = (n + 1023u) / 1024u, a = threadIdx.x * per, b = a + per < n ? a + per : n;
    uint32_t sum = 0;
    for (uint32_t i = a; i < b; ++i)
        if (TOPO_CHK(check, i < cap, 41u, i) && i < cap) sum += counts[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (uint32_t off = 1; off < 1024; off <<= 1) {      // inclusive scan of the 1024 partial sums
        const uint32_t v = threadIdx.x >= off ? part[threadIdx.x - off] : 0u;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    if (threadIdx.x == 1023) {
        const uint32_t all = part[1023];
        state[slot] = all;
        if (advance) {
            state[kSummitStateBase] = state[kSummitStateTotal];
            state[kSummitStateTotal] += all;
        } else {
            state[kSummitStateSeen] += all;      // (the candidates of the call's bands: topo_debug_summit_counts)
        }
    }
    uint32_t run = part[threadIdx.x] - sum;
    for (uint32_t i = a; i < b; ++i) {
        if (!(TOPO_CHK(check, i < cap, 41u, i) && i < cap)) break;
        const uint32_t v = counts[i];
        counts[i] = run;
        run += v;
    }
}

// A lane per ballot bit: item (wave, lane) is the post of k_summit_candidates' numbering; its index goes to dst, which has room for cap.
__global__ __launch_bounds__(256) void k_summit_scatter(const uint64_t* __restrict__ wave_mask, const uint32_t* __restrict__ offsets, uint32_t n_waves, uint32_t y0,
                                                        uint32_t tile_w, uint32_t waves_per_row, uint32_t* __restrict__ dst, uint32_t cap, uint32_t wave_cap, uint32_t* check) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = wave_first(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (wave >= n_waves || !(TOPO_CHK(check, wave < wave_cap, 41u, wave) && wave < wave_cap)) return;
    const uint64_t mask = wave_mask[wave];
    if (!((mask >> lane) & 1ull)) return;
    const uint32_t pos = offsets[wave] + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    if (!(TOPO_CHK(check, pos < cap, 41u, pos) && pos < cap)) return;
    const uint32_t r = wave / waves_per_row;
    dst[pos] = (y0 + r) * tile_w + (wave - r * waves_per_row) * 64u + lane;
}

// The same for the candidates k_summit_reject kept (entry 64 wave + lane of `src`): the band's summits, appended to the call's.  Summit
// number g = state[base] + its rank within the band; while g < capacity its (tile rank, post index) go to the first two words of
// record g, where k_summit_isolation finds them once every band is through.  No list of summits is kept besides.
__global__ __launch_bounds__(256) void k_summit_append(const uint64_t* __restrict__ wave_mask, const uint32_t* __restrict__ offsets, uint32_t n_waves,
                                                       const uint32_t* __restrict__ state, const uint32_t* __restrict__ src, uint32_t cap, uint32_t rank, SummitRec* __restrict__ out,
                                                       uint32_t capacity, uint32_t wave_cap, uint32_t* check) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = wave_first(blockIdx.x * 4u + (threadIdx.x >> 6));
    uint32_t n = (state[kSummitStateCandidates] + 63u) / 64u;
    n = n < n_waves ? n : n_waves;
    if (wave >= n || !(TOPO_CHK(check, wave < wave_cap, 41u, wave) && wave < wave_cap)) return;
    const uint64_t mask = wave_mask[wave];
    if (!((mask >> lane) & 1ull)) return;
    const uint32_t i = wave * 64u + lane;
    const uint32_t g = state[kSummitStateBase] + offsets[wave] + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    if (g >= capacity || g < state[kSummitStateBase]) return;      // (counted, not recorded)
    if (!(TOPO_CHK(check, i < cap, 41u, i) && i < cap)) return;
    *reinterpret_cast<uint2*>(out + g) = make_uint2(rank, src[i]);
}

// ---- stage 2: the candidates with no dominator within min_isolation_m ---------------------------------------------------------------

__global__ __launch_bounds__(256) void k_summit_reject(RayParams P, double min_isolation, uint32_t rank, const uint32_t* __restrict__ cand, const uint32_t* __restrict__ state,
                                                       uint32_t cap, uint8_t* __restrict__ keep) {
    const uint32_t lane = threadIdx.x & 63;
    const LosScene& S = P.s;
    uint32_t n = state[kSummitStateCandidates];
    n = n < cap ? n : cap;
    if (!(TOPO_CHK(P.check, rank < S.n_tiles, 42u, rank) && rank < S.n_tiles)) return;
    const TileDev& t = S.tiles[rank];
    auto chk = [&](bool ok, uint64_t value) { return TOPO_CHK(P.check, ok, 42u, value); };
    for (uint32_t i = wave_first(blockIdx.x * 4u + (threadIdx.x >> 6)); i < n; i += gridDim.x * 4u) {
        if (!(TOPO_CHK(P.check, i < cap, 42u, i) && i < cap)) return;      // (cand and keep have room for cap)
        const uint32_t idx = wave_first(cand[i]);
        const uint32_t vy = idx / S.tile_w, vx = idx - vy * S.tile_w;
        bool hit = false;
        if (min_isolation > 0.0 && TOPO_CHK(P.check, vy < S.tile_h, 42u, idx) && vy < S.tile_h) {
            const float hp = wave_first(TOPO_GLOBAL_F32(t.heights)[idx]);
            double up[3];
            if (summit_direction(S, rank, vx, vy, up, chk))
                hit = wave_summit_walk<kWalkAny>(P, hp, rank, idx, up, summit_lon(t, vx), summit_lat(t, vy), min_isolation, lane, 42u).found;
        }
        if (lane == 0) keep[i] = hit ? 0 : 1;
    }
}

// A lane per candidate: the bytes of k_summit_reject into ballots and counts.
__global__ __launch_bounds__(256) void k_summit_flags(const uint8_t* __restrict__ keep, const uint32_t* __restrict__ state, uint32_t cap, uint64_t* __restrict__ wave_mask,
                                                      uint32_t* __restrict__ wave_count, uint32_t wave_cap, uint32_t* check) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = wave_first(blockIdx.x * 4u + (threadIdx.x >> 6));
    uint32_t n = state[kSummitStateCandidates];
    n = n < cap ? n : cap;
    if (wave * 64u >= n) return;
    const uint32_t i = wave * 64u + lane;
    const uint64_t mask = __ballot(i < n && TOPO_CHK(check, i < cap, 41u, i) && i < cap && keep[i] != 0);
    if (lane == 0 && TOPO_CHK(check, wave < wave_cap, 41u, wave) && wave < wave_cap) {
        wave_mask[wave] = mask;
        wave_count[wave] = (uint32_t)__popcll(mask);
    }
}

// ---- stage 3: the summits' records ----------------------------------------------------------------------------------------------------

__device__ __forceinline__ void summit_store(SummitRec* dst, double lon, double lat, double iso, float h, float hh, int32_t tlat, int32_t tlon, uint32_t vx, uint32_t vy,
                                             int32_t hlat, int32_t hlon, uint32_t hx, uint32_t hy) {
    int4* d = reinterpret_cast<int4*>(dst);
    d[0] = make_int4(__double2loint(lon), __double2hiint(lon), __double2loint(lat), __double2hiint(lat));
    d[1] = make_int4(__double2loint(iso), __double2hiint(iso), __float_as_int(h), __float_as_int(hh));
    d[2] = make_int4(tlat, tlon, (int32_t)vx, (int32_t)vy);
    d[3] = make_int4(hlat, hlon, (int32_t)hx, (int32_t)hy);
}

// One launch a call, behind the last band: record i < min(summits, capacity) holds its post (k_summit_append) and gets its values.
__global__ __launch_bounds__(256) void k_summit_isolation(RayParams P, double radius, const uint32_t* __restrict__ state, SummitRec* __restrict__ out, uint32_t capacity) {
    const uint32_t lane = threadIdx.x & 63;
    const LosScene& S = P.s;
    uint32_t n = state[kSummitStateTotal];
    n = n < capacity ? n : capacity;
    auto chk = [&](bool ok, uint64_t value) { return TOPO_CHK(P.check, ok, 43u, value); };
    for (uint32_t i = wave_first(blockIdx.x * 4u + (threadIdx.x >> 6)); i < n; i += gridDim.x * 4u) {
        const uint2 post = *reinterpret_cast<const uint2*>(out + i);
        const uint32_t rank = wave_first(post.x), idx = wave_first(post.y);
        const uint32_t vy = idx / S.tile_w, vx = idx - vy * S.tile_w;
        if (!(TOPO_CHK(P.check, rank < S.n_tiles && vy < S.tile_h, 43u, ((uint64_t)rank << 32) | idx) && rank < S.n_tiles && vy < S.tile_h)) continue;
        const TileDev& t = S.tiles[rank];
        const float hp = wave_first(TOPO_GLOBAL_F32(t.heights)[idx]);
        const double lon = summit_lon(t, vx), lat = summit_lat(t, vy);
        double up[3];
        SummitBest b{0.0, 0u, 0u, 0.0f, false};
        if (summit_direction(S, rank, vx, vy, up, chk)) b = wave_summit_walk<kWalkNearest>(P, hp, rank, idx, up, lon, lat, radius, lane, 43u);
        if (lane != 0) continue;
        const int32_t tlat = P.tile_ll[2 * (size_t)rank], tlon = P.tile_ll[2 * (size_t)rank + 1];
        if (b.found && TOPO_CHK(P.check, b.rank < S.n_tiles, 43u, b.rank) && b.rank < S.n_tiles) {
            const uint32_t hy = b.idx / S.tile_w;
            summit_store(out + i, lon, lat, b.d, hp, b.h, tlat, tlon, vx, vy, P.tile_ll[2 * (size_t)b.rank], P.tile_ll[2 * (size_t)b.rank + 1], b.idx - hy * S.tile_w, hy);
        } else {
            summit_store(out + i, lon, lat, __builtin_inf(), hp, 0.0f, tlat, tlon, vx, vy, 0, 0, 0u, 0u);
        }
    }
}

// ---- snap ---------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ void snap_store(SummitSnapRec* dst, double lon, double lat, double d, float h, int32_t status, int32_t tlat, int32_t tlon, uint32_t vx, uint32_t vy) {
    int4* o = reinterpret_cast<int4*>(dst);
    o[0] = make_int4(__double2loint(lon), __double2hiint(lon), __double2loint(lat), __double2hiint(lat));
    o[1] = make_int4(__double2loint(d), __double2hiint(d), __float_as_int(h), status);
    o[2] = make_int4(tlat, tlon, (int32_t)vx, (int32_t)vy);
}

// A wave per point.  The point is two doubles (one 16-byte load), the record three 16-byte stores.
__global__ __launch_bounds__(256) void k_summit_snap(RayParams P, const double2* __restrict__ lonlat, double radius, SummitSnapRec* __restrict__ out, uint32_t n) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t i = wave_first(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (i >= n) return;
    const double2 ll = lonlat[i];
    const double lon = lane_f64(ll.x, 0), lat = lane_f64(ll.y, 0);
    if (!surface_point_valid(lon, lat)) {
        if (lane == 0) snap_store(out + i, 0.0, 0.0, 0.0, 0.0f, kSnapInvalid, 0, 0, 0u, 0u);
        return;
    }
    double uc[3];
    surface_direction(lon, lat, uc);
    const SummitBest b = wave_summit_walk<kWalkSnap>(P, 0.0f, 0u, 0u, uc, lon, lat, radius, lane, 44u);
    if (lane != 0) return;
    const LosScene& S = P.s;
    if (!b.found || !(TOPO_CHK(P.check, b.rank < S.n_tiles, 44u, b.rank) && b.rank < S.n_tiles)) {
        snap_store(out + i, 0.0, 0.0, 0.0, 0.0f, kSnapNone, 0, 0, 0u, 0u);
        return;
    }
    const uint32_t vy = b.idx / S.tile_w, vx = b.idx - vy * S.tile_w;
    snap_store(out + i, summit_lon(S.tiles[b.rank], vx), summit_lat(S.tiles[b.rank], vy), b.d, b.h, kSnapFound, P.tile_ll[2 * (size_t)b.rank], P.tile_ll[2 * (size_t)b.rank + 1], vx,
               vy);
}

}  // namespace
}  // namespace topo
