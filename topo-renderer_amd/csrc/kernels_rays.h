// kernels_rays.h -- rays against the resident tiles, and their first application on a finished frame (topo_rays.hip: a translation
// unit of its own, so that the frame path's unit -- and with it every frame kernel's code -- stays exactly what it was).
//
//   k_raycast      per ray, the first terrain it meets among the resident tiles (f64: topo_los.h); k_raycast_lane: the other launch shape (-DTOPO_RAYCAST_LANE builds only)
//   k_sunlit_map   per pixel of whole views, whether its ground point is lit, faces away from the sun or lies in cast shadow
#pragma once

#include "kernels_common.h"
#include "kernels_ground.h"     // ground_triangle: the sunlit layer finds a pixel's ground point as k_ground_map does
#include "topo_los.h"

namespace topo {
namespace {

// ---- rays (topo_raycast_*) ----------------------------------------------------------------------------------------------------
// A ray from anywhere against the triangles of every resident tile: topo_los.h has the mesh, the hit rule, the winner and the
// traversal with the argument for each rejection.  The kernels read the tile table, the DEMs, the block tables, the tiles' f64
// tables and the tile spheres and write only `out`, as four 16-byte stores per record.  No frame is involved: frames in flight on
// other streams only read what this reads.  Two launch shapes were measured on the c4 mosaic: one wave per ray
// (k_raycast, kept: 4.7 times the rate on near-horizontal rays, whose cost is the cells of the blocks they graze) and one lane per
// ray (k_raycast_lane: los_cast as it stands; an experiment build, -DTOPO_RAYCAST_LANE, launches it instead: tools/README.md).
__device__ __forceinline__ void ray_store(RayHit* dst, double t, double lon, double lat, float h, int32_t kind, int32_t tlat, int32_t tlon, uint32_t cx,
                                          uint32_t cy, uint32_t tri, uint32_t front, float w1, float w2) {
    int4* d = reinterpret_cast<int4*>(dst);
    d[0] = make_int4(__double2loint(t), __double2hiint(t), __double2loint(lon), __double2hiint(lon));
    d[1] = make_int4(__double2loint(lat), __double2hiint(lat), __float_as_int(h), kind);
    d[2] = make_int4(tlat, tlon, (int32_t)cx, (int32_t)cy);
    d[3] = make_int4((int32_t)tri, (int32_t)front, __float_as_int(w1), __float_as_int(w2));
}

#ifdef TOPO_RAYCAST_LANE
__global__ __launch_bounds__(256) void k_raycast_lane(RayParams P, const LosRay* __restrict__ rays, RayHit* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const double2* const src = reinterpret_cast<const double2*>(rays + i);
    const double2 a = src[0], b = src[1], c = src[2], e = src[3];
    const LosRay r{{a.x, a.y, b.x}, {b.y, c.x, c.y}, e.x, e.y};
    if (!los_ray_valid(r)) {
        ray_store(out + i, 0.0, 0.0, 0.0, 0.0f, kRayInvalid, 0, 0, 0u, 0u, 0u, 0u, 0.0f, 0.0f);
        return;
    }
    LosHit best;
    los_cast<false>(P.s, r, kLosNoTri, kLosNoTri, best, [&](bool ok, uint64_t value) { return TOPO_CHK(P.check, ok, 20u, value); });
    // (the rank is tested in the product build too: what it indexes is a table)
    if (!best.hit || !(TOPO_CHK(P.check, best.rank < P.s.n_tiles, 20u, best.rank) && best.rank < P.s.n_tiles)) {
        ray_store(out + i, 0.0, 0.0, 0.0, 0.0f, kRayMiss, 0, 0, 0u, 0u, 0u, 0u, 0.0f, 0.0f);
        return;
    }
    double lon, lat, h;
    los_hit_point(r, best.t, lon, lat, h);
    const uint32_t cell = best.tri >> 1, hm1 = P.s.tile_h - 1, cx = cell / hm1, cy = cell - cx * hm1;
    ray_store(out + i, best.t, lon, lat, (float)h, kRayHit, P.tile_ll[2 * (size_t)best.rank], P.tile_ll[2 * (size_t)best.rank + 1], cx, cy, best.tri & 1u,
              best.front, (float)best.u, (float)best.v);
}
#endif

// One WAVE per ray.  The lanes take 64 raster blocks of a tile at a time (their spheres and heights: one coalesced read), the
// survivors are ballotted and taken one by one, a survivor's cells are dealt out to the lanes, every lane keeps its own best hit,
// and t_max shrinks to the wave's minimum after each block; at the end the wave's best under (t, rank, triangle) is found with six
// exchange steps.  The answer is los_cast's, byte for byte: the same rejections, the same triangle test, the same order.
__global__ __launch_bounds__(256) void k_raycast(RayParams P, const LosRay* __restrict__ rays, RayHit* __restrict__ out, uint32_t n) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t i = wave_first(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (i >= n) return;
    const LosScene& S = P.s;
    const double2* const src = reinterpret_cast<const double2*>(rays + i);
    const double2 a = src[0], b = src[1], c = src[2], e = src[3];
    const LosRay r{{a.x, a.y, b.x}, {b.y, c.x, c.y}, e.x, e.y};
    if (!los_ray_valid(r)) {
        if (lane == 0) ray_store(out + i, 0.0, 0.0, 0.0, 0.0f, kRayInvalid, 0, 0, 0u, 0u, 0u, 0u, 0.0f, 0.0f);
        return;
    }
    auto chk = [&](bool ok, uint64_t value) { return TOPO_CHK(P.check, ok, 20u, value); };
    const double* const o = r.o;
    const double* const d = r.d;
    const double oo = o[0] * o[0] + o[1] * o[1] + o[2] * o[2], od = o[0] * d[0] + o[1] * d[1] + o[2] * d[2], dd = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    const double origin[3] = {0.0, 0.0, 0.0};
    LosHit best{0.0, 0.0, 0.0, 0u, 0u, 0u, false};
    double tmax = r.tmax;
    const uint32_t cells_x = S.tile_w - 1, cells_y = S.tile_h - 1, nb = S.bx_count * S.by_count;
    for (uint32_t rank = 0; rank < S.n_tiles; ++rank) {
        const double* const ts = S.spheres + (size_t)kLosSphereDoubles * rank;
        {
            double ta = r.tmin, tb = tmax;
            if (ts[3] >= 0.0 && ts[4] >= 0.0 && !los_clip_sphere(o, d, dd, ts, ts[3] + ts[4], ta, tb)) continue;
        }
        const TileDev& t = S.tiles[rank];
        const double sx = (double)t.scale_x, sy = (double)t.scale_y;
        const double pad_y = 1.0 / 64.0 + fabs(0.25 * kGroundRad * sx * sx / sy);
        for (uint32_t b0 = 0; b0 < nb; b0 += 64) {
            const uint32_t blk = b0 + lane;
            double ta = r.tmin, tb = tmax;
            bool keep = blk < nb;
            if (keep) {
                const double* const bs = t.block_bounds + 4 * (size_t)blk;
                const double hmin = (double)t.block_minmax[2 * (size_t)blk], hmax = (double)t.block_minmax[2 * (size_t)blk + 1];
                if (bs[3] < kLosAbsurd && !los_clip_sphere(o, d, dd, bs, bs[3], ta, tb)) keep = false;
                if (keep && hmin <= hmax) {
                    const double r0 = fabs(kGroundR0 + hmin), r1 = fabs(kGroundR0 + hmax), top = (r0 > r1 ? r0 : r1) + kLosShellPad;
                    if (top < kLosAbsurd && !los_clip_sphere(o, d, dd, origin, top, ta, tb)) keep = false;
                }
            }
            uint64_t todo = __ballot(keep);
            while (todo) {
                const int j = (int)pop_bit(todo);
                const double ja = shfl_f64(ta, j);
                double jb = shfl_f64(tb, j);
                if (tmax < jb) jb = tmax;      // (t_max may have shrunk since the block was tested)
                if (!(ja <= jb)) continue;
                const uint32_t bj = b0 + (uint32_t)j, by = bj / S.bx_count, bx = bj - by * S.bx_count;
                const uint32_t cx0 = bx * kLosBCX, cy0 = by * kLosBCY;
                const uint32_t cx1 = cx0 + kLosBCX < cells_x ? cx0 + kLosBCX : cells_x, cy1 = cy0 + kLosBCY < cells_y ? cy0 + kLosBCY : cells_y;
                uint32_t ix0 = cx0, ix1 = cx1 - 1, iy0 = cy0, iy1 = cy1 - 1;
                if (ground_finite(ja) && ground_finite(jb)) los_cell_range(t, o, d, oo, od, dd, ja, jb, pad_y, cx0, cx1, cy0, cy1, ix0, ix1, iy0, iy1);
                if (ix0 > ix1 || iy0 > iy1 || ix1 >= cx1 || iy1 >= cy1) continue;
                const uint32_t ncy = iy1 - iy0 + 1, total = (ix1 - ix0 + 1) * ncy;
                for (uint32_t k = lane; k < total; k += 64) {
                    const uint32_t ci = k / ncy;
                    (void)los_cell<false>(S, t, rank, ix0 + ci, iy0 + (k - ci * ncy), o, d, r.tmin, tmax, kLosNoTri, best, chk);
                }
#pragma unroll
                for (int m = 32; m; m >>= 1) {      // t_max: the wave's smallest
                    const double other = shfl_xor_f64(tmax, m);
                    tmax = other < tmax ? other : tmax;
                }
            }
        }
    }
#pragma unroll
    for (int m = 32; m; m >>= 1) {      // the wave's best under (t, rank, triangle)
        LosHit other;
        other.t = shfl_xor_f64(best.t, m);
        other.u = shfl_xor_f64(best.u, m);
        other.v = shfl_xor_f64(best.v, m);
        other.rank = (uint32_t)__shfl_xor((int)best.rank, m);
        other.tri = (uint32_t)__shfl_xor((int)best.tri, m);
        other.front = (uint32_t)__shfl_xor((int)best.front, m);
        other.hit = __shfl_xor((int)best.hit, m) != 0;
        if (other.hit && los_better(other.t, other.rank, other.tri, best)) best = other;
    }
    if (lane != 0) return;
    if (!best.hit || !(TOPO_CHK(P.check, best.rank < S.n_tiles, 20u, best.rank) && best.rank < S.n_tiles)) {
        ray_store(out + i, 0.0, 0.0, 0.0, 0.0f, kRayMiss, 0, 0, 0u, 0u, 0u, 0u, 0.0f, 0.0f);
        return;
    }
    double lon, lat, h;
    los_hit_point(r, best.t, lon, lat, h);
    const uint32_t cell = best.tri >> 1, hm1 = S.tile_h - 1, cx = cell / hm1, cy = cell - cx * hm1;
    ray_store(out + i, best.t, lon, lat, (float)h, kRayHit, P.tile_ll[2 * (size_t)best.rank], P.tile_ll[2 * (size_t)best.rank + 1], cx, cy, best.tri & 1u,
              best.front, (float)best.u, (float)best.v);
}

// The sunlit layer (topo_sunlit_map_device): one byte per pixel of views [first_view, first_view + n_views) of a finished
// submission -- kSunNone where there is no terrain point (sky, degenerate, incomplete frame), else the class los_sunlit (topo_los.h)
// gives the pixel's ground point, found exactly as k_ground_map finds it; a piece of a near-clipped triangle answers with its
// original triangle.  The shadow ray stops at its first hit.  One wave per 64-key segment, grid-stride, as k_ground_map: a segment
// without a mark costs no key load, and a wave's 64 bytes are one contiguous store.
__global__ __launch_bounds__(256) void k_sunlit_map(GroundParams P, LosScene S, double sx, double sy, double sz, uint8_t* __restrict__ out, size_t view_stride,
                                                    size_t pitch) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwave = (uint64_t)gridDim.x * 4;
    const uint64_t view_keys = (uint64_t)P.q.W * P.q.H;
    const uint64_t k0 = P.q.first_view * view_keys, k1 = k0 + P.q.n_views * view_keys;
    const bool incomplete = (P.q.counters[kCtrStatus] & kStatusRareOverflow) != 0;
    [[maybe_unused]] const uint64_t nseg = ((uint64_t)P.q.n_keys + 63) >> 6;      // (the check build's bound)
    const double sun[3] = {sx, sy, sz};
    for (uint64_t seg = (k0 >> 6) + wave; seg * 64 < k1; seg += nwave) {
        const uint64_t k = seg * 64 + lane;
        if (k < k0 || k >= k1) continue;
        const bool marked = !incomplete && TOPO_CHK(P.q.check, seg < nseg, 21u, seg) && P.q.dirty[seg] != 0;
        const uint64_t key = marked && TOPO_CHK(P.q.check, k < P.q.n_keys, 21u, k) ? P.q.vis[k] : kVisClear;
        const uint32_t v = (uint32_t)k / (uint32_t)view_keys, rem = (uint32_t)k - v * (uint32_t)view_keys;      // (k < 2^32)
        const uint32_t y = rem / P.q.W, x = rem - y * P.q.W;
        uint8_t val = kSunNone;
        if ((uint32_t)key != kNoTri) {
            GroundAnswer a{};
            double p[3][3];
            if (ground_triangle(P, (uint32_t)key, a, p)) {
                a.r = ground_solve(p, P.views[v], ground_ndc_x(x, P.q.W), ground_ndc_y(y, P.q.H));
                if (a.r.ok)
                    val = los_sunlit(S, p, a.r.w1, a.r.w2, a.t.rank, a.t.tri, sun, [&](bool ok, uint64_t value) { return TOPO_CHK(P.q.check, ok, 21u, value); });
            }
        }
        out[(size_t)(v - P.q.first_view) * view_stride + (size_t)y * pitch + x] = val;
    }
}

}  // namespace
}  // namespace topo
