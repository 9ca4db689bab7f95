// ground_emul.cpp -- TEST-ONLY g++ build of the product's ground-point arithmetic (topo-renderer_amd/csrc/topo_ground.h): the lane
// function k_ground and k_ground_map call for every pixel they answer, run here over a whole frame of winners on the CPU
// (tests/ground_emul.py, tests/test_ground_cpu.py).  The glue around it -- key, decode, vertex texels, DEM loads -- is the kernels'.
#include "../topo-renderer_amd/csrc/topo_ground.h"
#include "emul_tiles.h"

using namespace topo;

struct EmulGroundOut {     // topo_ground_point's fields, the computed ones in f64
    double lon_deg, lat_deg, height, range, w1, w2;
    float depth;
    int32_t kind, tile_lat, tile_lon;
    uint32_t cell_x, cell_y, tri, fan;
};

// depth / winners: H x W (winner = rank * tris_per_tile + triangle, kNoTri = sky); uniforms: the view's 40 floats.
extern "C" int emul_ground(const EmulGeoTile* tiles, uint32_t n_tiles, uint32_t tile_w, uint32_t tile_h, const float* uniforms, uint32_t W, uint32_t H,
                           const float* depth, const uint32_t* winners, EmulGroundOut* out) {
    GroundView view{};
    memcpy(view.proj, uniforms, sizeof view.proj);
    memcpy(view.pos, uniforms + 32, sizeof view.pos);
    const uint32_t tris_per_tile = 2u * (tile_w - 1) * (tile_h - 1), hm1 = tile_h - 1;
    for (uint32_t y = 0; y < H; ++y)
        for (uint32_t x = 0; x < W; ++x) {
            const size_t at = (size_t)y * W + x;
            EmulGroundOut o{};
            o.depth = 1.0f;
            if (winners[at] != kNoTri) {
                const uint32_t id = winners[at] << 1;      // (the oracle's winners carry no fan piece)
                const GroundTri g = ground_decode(id, tris_per_tile, hm1);
                if (g.rank >= n_tiles) return -1;
                const EmulGeoTile& et = tiles[g.rank];
                const TileDev t = make_dev(et);
                uint32_t vx[3], vy[3];
                triangle_vertices(g.tri, hm1, vx, vy);
                double p[3][3];
                for (int i = 0; i < 3; ++i) {
                    if (vx[i] >= tile_w || vy[i] >= tile_h) return -2;
                    ground_vertex(t, vx[i], vy[i], et.heights[(size_t)vy[i] * tile_w + vx[i]], p[i]);
                }
                const GroundResult r = ground_solve(p, view, ground_ndc_x(x, W), ground_ndc_y(y, H));
                o.depth = depth[at];
                o.kind = r.ok ? kGroundTerrain : kGroundDegenerate;
                o.tile_lat = et.lat; o.tile_lon = et.lon;
                o.cell_x = g.cell_x; o.cell_y = g.cell_y; o.tri = g.tri & 1u; o.fan = g.fan;
                if (r.ok) { o.lon_deg = r.lon_deg; o.lat_deg = r.lat_deg; o.height = r.height; o.range = r.range; o.w1 = r.w1; o.w2 = r.w2; }
            }
            out[at] = o;
        }
    return 0;
}
