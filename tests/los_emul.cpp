// los_emul.cpp -- TEST-ONLY g++ build of the product's ray arithmetic and traversal (topo-renderer_amd/csrc/topo_los.h): los_cast, the
// function k_raycast calls for every ray, and los_cast_all, the same triangle test and ordering over every triangle (tests/los_emul.py,
// tests/test_raycast_cpu.py).  The tables the traversal reads are built here on the host: the tiles' f64 (cos, sin) tables with the
// functions k_ground_tables calls, block minima / maxima that skip NaN, and bounding spheres of this file's own making (the mean of a
// block's finite vertices, the largest distance plus a metre) -- any spheres that hold the vertices must give the brute-force answer.
#include <cmath>
#include <vector>

#include "../topo-renderer_amd/csrc/topo_los.h"
#include "emul_tiles.h"

using namespace topo;

struct EmulLosOut {        // topo_ray_hit's fields, the computed ones in f64, plus the winner's rank and triangle
    double t, lon_deg, lat_deg, height, w1, w2;
    int32_t kind, tile_lat, tile_lon;
    uint32_t cell_x, cell_y, tri, front, rank, triangle;
};

// The tables los_cast reads, built on the host.
struct EmulScene {
    std::vector<TileDev> dev;
    std::vector<double> trig, spheres;
    std::vector<std::vector<float>> minmax;
    std::vector<std::vector<double>> bounds;
    LosScene S;
    EmulScene(const EmulGeoTile* tiles, uint32_t n_tiles, uint32_t tile_w, uint32_t tile_h) {
        const uint32_t bxc = (tile_w - 1 + kLosBCX - 1) / kLosBCX, byc = (tile_h - 1 + kLosBCY - 1) / kLosBCY, nb = bxc * byc;
        const size_t tab = ground_table_doubles(tile_w, tile_h);
        dev.resize(n_tiles);
        trig.assign(tab * n_tiles + 2, 0.0);
        spheres.assign((size_t)kLosSphereDoubles * n_tiles + 2, 0.0);
        minmax.resize(n_tiles);
        bounds.resize(n_tiles);
        for (uint32_t r = 0; r < n_tiles; ++r) {
            TileDev& t = dev[r];
            t = make_dev(tiles[r]);
            fill_trig(t, tile_w, tile_h, trig.data() + tab * r);
            minmax[r].assign(2 * (size_t)nb, 0.0f);
            bounds[r].assign(4 * (size_t)nb, 0.0);
            double tc[3] = {0.0, 0.0, 0.0}, rmax = 0.0;
            bool finite = true;
            for (uint32_t by = 0; by < byc; ++by)
                for (uint32_t bx = 0; bx < bxc; ++bx) {
                    const uint32_t blk = by * bxc + bx;
                    float mn = INFINITY, mx = -INFINITY;
                    double c[3] = {0.0, 0.0, 0.0};
                    size_t cnt = 0;
                    std::vector<double> pts;
                    for (uint32_t y = by * kLosBCY; y <= by * kLosBCY + kLosBCY && y < tile_h; ++y)
                        for (uint32_t x = bx * kLosBCX; x <= bx * kLosBCX + kLosBCX && x < tile_w; ++x) {
                            const float h = t.heights[(size_t)y * tile_w + x];
                            mn = fminf(mn, h);
                            mx = fmaxf(mx, h);
                            if (!ground_finite((double)h)) continue;
                            double p[3];
                            ground_vertex(t, x, y, h, p);
                            pts.insert(pts.end(), p, p + 3);
                            for (int k = 0; k < 3; ++k) c[k] += p[k];
                            ++cnt;
                        }
                    double rad = 0.0;
                    for (int k = 0; k < 3; ++k) c[k] = cnt ? c[k] / (double)cnt : NAN;
                    for (size_t i = 0; i < pts.size(); i += 3)
                        rad = fmax(rad, sqrt((pts[i] - c[0]) * (pts[i] - c[0]) + (pts[i + 1] - c[1]) * (pts[i + 1] - c[1]) + (pts[i + 2] - c[2]) * (pts[i + 2] - c[2])));
                    minmax[r][2 * blk] = mn;
                    minmax[r][2 * blk + 1] = mx;
                    double* bs = bounds[r].data() + 4 * (size_t)blk;
                    bs[0] = c[0]; bs[1] = c[1]; bs[2] = c[2]; bs[3] = rad + 1.0;
                    finite = finite && cnt > 0;
                    for (int k = 0; k < 3; ++k) tc[k] += c[k];
                    rmax = fmax(rmax, bs[3]);
                }
            double* ts = spheres.data() + (size_t)kLosSphereDoubles * r;
            double r2 = 0.0;
            for (int k = 0; k < 3; ++k) ts[k] = tc[k] / (double)nb;
            for (uint32_t b = 0; b < nb && finite; ++b) {
                const double* bs = bounds[r].data() + 4 * (size_t)b;
                r2 = fmax(r2, (bs[0] - ts[0]) * (bs[0] - ts[0]) + (bs[1] - ts[1]) * (bs[1] - ts[1]) + (bs[2] - ts[2]) * (bs[2] - ts[2]));
            }
            ts[3] = finite ? sqrt(r2) : -1.0;
            ts[4] = finite ? rmax : -1.0;
            t.block_minmax = minmax[r].data();
            t.block_bounds = bounds[r].data();
        }
    S = LosScene{dev.data(), trig.data(), spheres.data(), tab * n_tiles, n_tiles, tile_w, tile_h, bxc, byc};
    }
};

// mode 0: the traversal; 1: every triangle.  Returns the number of index checks that failed.
extern "C" int emul_raycast(const EmulGeoTile* tiles, uint32_t n_tiles, uint32_t tile_w, uint32_t tile_h, const LosRay* rays, uint32_t n, int mode,
                            EmulLosOut* out) {
    EmulScene scene(tiles, n_tiles, tile_w, tile_h);
    const LosScene& S = scene.S;
    int bad = 0;
    auto chk = [&](bool ok, uint64_t) { if (!ok) ++bad; return ok; };
    const uint32_t hm1 = tile_h - 1;
    for (uint32_t i = 0; i < n; ++i) {
        EmulLosOut o{};
        const LosRay& r = rays[i];
        if (!los_ray_valid(r)) {
            o.kind = kRayInvalid;
        } else {
            LosHit best;
            if (mode == 0) los_cast<false>(S, r, kLosNoTri, kLosNoTri, best, chk);
            else los_cast_all<false>(S, r, kLosNoTri, kLosNoTri, best, chk);
            if (best.hit) {
                o.kind = kRayHit;
                o.t = best.t;
                los_hit_point(r, best.t, o.lon_deg, o.lat_deg, o.height);
                o.w1 = best.u; o.w2 = best.v;
                o.tile_lat = tiles[best.rank].lat; o.tile_lon = tiles[best.rank].lon;
                const uint32_t cell = best.tri >> 1;
                o.cell_x = cell / hm1; o.cell_y = cell - o.cell_x * hm1;
                o.tri = best.tri & 1u; o.front = best.front; o.rank = best.rank; o.triangle = best.tri;
            }
        }
        out[i] = o;
    }
    return bad;
}

// The sunlit class (los_sunlit) of n ground points: triangle tri[i] of tile rank[i] with plane weights w1[i], w2[i] (ground_solve's).
// mode as emul_raycast.  Returns the number of index checks that failed.
extern "C" int emul_sunlit(const EmulGeoTile* tiles, uint32_t n_tiles, uint32_t tile_w, uint32_t tile_h, uint32_t n, const uint32_t* rank, const uint32_t* tri,
                           const double* w1, const double* w2, const double* sun, uint8_t* out) {
    EmulScene scene(tiles, n_tiles, tile_w, tile_h);
    int bad = 0;
    auto chk = [&](bool ok, uint64_t) { if (!ok) ++bad; return ok; };
    for (uint32_t i = 0; i < n; ++i) {
        out[i] = kSunNone;
        if (rank[i] >= n_tiles) continue;
        uint32_t vx[3], vy[3];
        triangle_vertices(tri[i], tile_h - 1, vx, vy);
        double p[3][3];
        const TileDev& t = scene.dev[rank[i]];
        for (int k = 0; k < 3; ++k) ground_vertex(t, vx[k], vy[k], t.heights[(size_t)vy[k] * tile_w + vx[k]], p[k]);
        out[i] = los_sunlit(scene.S, p, w1[i], w2[i], rank[i], tri[i], sun, chk);
    }
    return bad;
}
