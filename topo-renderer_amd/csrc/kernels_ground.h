// kernels_ground.h -- device helpers of the ground queries, no kernel: a pixel's winning triangle and its ground point.  Shared by
// k_ground / k_ground_map (kernels_query.h) and k_sunlit_map (kernels_rays.h, a translation unit of its own).
#pragma once

#include "kernels_common.h"
#include "topo_ground.h"

namespace topo {
namespace {

struct GroundAnswer {
    int32_t kind;
    int32_t lat, lon;
    GroundTri t;
    GroundResult r;
};

// The per-triangle part of an answer: the key's low word decoded, the tile, and the ECEF positions of the three vertices.  false
// (a.kind = degenerate) where the id names nothing of the tile set.
__device__ __forceinline__ bool ground_triangle(const GroundParams& P, uint32_t id, GroundAnswer& a, double p[3][3]) {
    a.kind = kGroundDegenerate;
    a.t = ground_decode(id, P.q.tris_per_tile, P.q.hm1);
    // (the rank and the vertex texels are tested in the product build too: what they index are tables and the DEM)
    if (!(TOPO_CHK(P.q.check, a.t.rank < P.q.n_tiles, 18u, id) && a.t.rank < P.q.n_tiles)) return false;
    a.lat = P.q.tile_ll[2 * (size_t)a.t.rank];
    a.lon = P.q.tile_ll[2 * (size_t)a.t.rank + 1];
    const TileDev& t = P.tiles[a.t.rank];
    uint32_t vx[3], vy[3];
    triangle_vertices(a.t.tri, P.q.hm1, vx, vy);
    const size_t tab = (size_t)a.t.rank * ground_table_doubles(P.tile_w, P.tile_h);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const bool inside = vx[i] < P.tile_w && vy[i] < P.tile_h;
        if (!(TOPO_CHK(P.q.check, inside, 18u, ((uint64_t)vy[i] << 32) | vx[i]) && inside)) return false;
        const size_t lo = tab + 2 * (size_t)vx[i], la = tab + 2 * ((size_t)P.tile_w + vy[i]);
        if (!TOPO_CHK(P.q.check, la + 1 < P.trig_doubles, 18u, la)) return false;
        const double2 clo_slo = *reinterpret_cast<const double2*>(P.trig + lo), cla_sla = *reinterpret_cast<const double2*>(P.trig + la);
        ground_vertex_from(TOPO_GLOBAL_F32(t.heights)[(size_t)vy[i] * P.tile_w + vx[i]], clo_slo.x, clo_slo.y, cla_sla.x, cla_sla.y, p[i]);
    }
    return true;
}

__device__ __forceinline__ GroundAnswer ground_answer(const GroundParams& P, uint64_t key, uint32_t view, uint32_t x, uint32_t y) {
    GroundAnswer a{};
    const uint32_t id = (uint32_t)key;
    if (id == kNoTri) return a;      // kind 0: sky
    double p[3][3];
    if (!ground_triangle(P, id, a, p)) return a;
    a.r = ground_solve(p, P.views[view], ground_ndc_x(x, P.q.W), ground_ndc_y(y, P.q.H));
    if (a.r.ok) a.kind = kGroundTerrain;
    return a;
}

}  // namespace
}  // namespace topo
