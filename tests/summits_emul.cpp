// summits_emul.cpp -- TEST-ONLY g++ build of the product's summit rule and search (topo-renderer_amd/csrc/topo_summits.h): the
// windowed forms the kernels restate wave by wave (the prefilter, the any-hit and the closest-hit search, the snap) and the same
// answers over every post of every tile (tests/summits_emul.py, tests/test_summits_cpu.py).  The tables are built here on the host:
// the trig tables with the functions k_ground_tables calls, the blocks' min / max as the load phase leaves them.
#include <cmath>
#include <vector>

#include "../topo-renderer_amd/csrc/topo_summits.h"
#include "emul_tiles.h"

using namespace topo;

struct EmulSummit {        // a post and its nearest dominator: topo_summit's values with ranks and post indices for the tiles
    double lon_deg, lat_deg, isolation_m;
    float height_m, higher_height_m;
    uint32_t rank, idx, higher_rank, higher_idx;
    int32_t has_higher, pad_;
};

struct EmulSnap {          // topo_summit_snap's values
    double lon_deg, lat_deg, distance_m;
    float height_m;
    int32_t status;
    uint32_t rank, idx;
};

struct EmulSummitScene {
    std::vector<TileDev> dev;
    std::vector<double> trig;
    std::vector<std::vector<float>> minmax;
    LosScene S;
    EmulSummitScene(const EmulGeoTile* tiles, uint32_t n_tiles, uint32_t tile_w, uint32_t tile_h) {
        const uint32_t bxc = (tile_w - 1 + kLosBCX - 1) / kLosBCX, byc = (tile_h - 1 + kLosBCY - 1) / kLosBCY;
        const size_t tab = ground_table_doubles(tile_w, tile_h);
        dev.resize(n_tiles);
        minmax.resize(n_tiles);
        trig.assign(tab * n_tiles + 2, 0.0);
        for (uint32_t r = 0; r < n_tiles; ++r) {
            dev[r] = make_dev(tiles[r]);
            fill_trig(dev[r], tile_w, tile_h, trig.data() + tab * r);
            minmax[r].assign(2 * (size_t)bxc * byc, 0.0f);
            for (uint32_t by = 0; by < byc; ++by)
                for (uint32_t bx = 0; bx < bxc; ++bx) {
                    float mn = INFINITY, mx = -INFINITY;
                    for (uint32_t y = by * kLosBCY; y <= by * kLosBCY + kLosBCY && y < tile_h; ++y)
                        for (uint32_t x = bx * kLosBCX; x <= bx * kLosBCX + kLosBCX && x < tile_w; ++x) {
                            mn = fminf(mn, dev[r].heights[(size_t)y * tile_w + x]);
                            mx = fmaxf(mx, dev[r].heights[(size_t)y * tile_w + x]);
                        }
                    minmax[r][2 * (by * bxc + bx)] = mn;
                    minmax[r][2 * (by * bxc + bx) + 1] = mx;
                }
            dev[r].block_minmax = minmax[r].data();
        }
        S = LosScene{dev.data(), trig.data(), nullptr, tab * n_tiles, n_tiles, tile_w, tile_h, bxc, byc};
    }
};

static EmulSummit record(const LosScene& S, uint32_t rank, uint32_t idx, float h, const SummitBest& b) {
    EmulSummit o{};
    o.lon_deg = summit_lon(S.tiles[rank], idx % S.tile_w);
    o.lat_deg = summit_lat(S.tiles[rank], idx / S.tile_w);
    o.isolation_m = b.found ? b.d : INFINITY;
    o.height_m = h;
    o.rank = rank;
    o.idx = idx;
    if (b.found) {
        o.higher_height_m = b.h;
        o.higher_rank = b.rank;
        o.higher_idx = b.idx;
        o.has_higher = 1;
    }
    return o;
}

// The nearest dominator within `radius` of each of n posts (rank, idx pairs).  mode 0: over the windows; 1: every post of every tile.
// A post that does not exist gets has_higher = -1.  Returns the number of index checks that failed.
extern "C" int emul_isolation(const EmulGeoTile* tiles, uint32_t n_tiles, uint32_t tile_w, uint32_t tile_h, const uint32_t* posts, uint32_t n, double radius, int mode,
                              EmulSummit* out) {
    EmulSummitScene scene(tiles, n_tiles, tile_w, tile_h);
    const LosScene& S = scene.S;
    int bad = 0;
    auto chk = [&](bool ok, uint64_t) { if (!ok) ++bad; return ok; };
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t rank = posts[2 * (size_t)i], idx = posts[2 * (size_t)i + 1];
        const float h = S.tiles[rank].heights[idx];
        SummitBest b{0.0, 0u, 0u, 0.0f, false};
        const bool exists = surface_tile_ok(S.tiles[rank]) && surface_height_ok(h);
        if (exists) {
            if (mode == 0) summit_nearest<false>(S, rank, idx, h, radius, b, chk);
            else summits_all(S, rank, idx, h, radius, false, b, chk);
        }
        out[i] = record(S, rank, idx, h, b);
        if (!exists) out[i].has_higher = -1;
    }
    return bad;
}

// The summits of a call in tile order, the way the kernels find them: the prefilter, the any-hit search within min_isolation, the
// closest-hit search within radius.  out: the first `capacity`; count: all; stages[0], [1]: the posts left after the first two stages.
extern "C" int emul_summits(const EmulGeoTile* tiles, uint32_t n_tiles, uint32_t tile_w, uint32_t tile_h, double radius, double min_isolation, float min_height,
                            EmulSummit* out, uint32_t capacity, uint32_t* count, uint64_t* stages) {
    EmulSummitScene scene(tiles, n_tiles, tile_w, tile_h);
    const LosScene& S = scene.S;
    int bad = 0;
    auto chk = [&](bool ok, uint64_t) { if (!ok) ++bad; return ok; };
    uint32_t found = 0;
    stages[0] = stages[1] = 0;
    for (uint32_t rank = 0; rank < n_tiles; ++rank) {
        const TileDev& t = S.tiles[rank];
        if (!surface_tile_ok(t)) continue;
        for (uint32_t vy = 0; vy < tile_h; ++vy)
            for (uint32_t vx = 0; vx < tile_w; ++vx) {
                const uint32_t idx = vy * tile_w + vx;
                const float h = t.heights[idx];
                if (!surface_height_ok(h) || !(h >= min_height) || summit_neighbour_rejects(S, t, rank, vx, vy, h, min_isolation, chk)) continue;
                ++stages[0];
                SummitBest b;
                if (min_isolation > 0.0) {
                    summit_nearest<true>(S, rank, idx, h, min_isolation, b, chk);
                    if (b.found) continue;
                }
                ++stages[1];
                summit_nearest<false>(S, rank, idx, h, radius, b, chk);
                if (found < capacity) out[found] = record(S, rank, idx, h, b);
                ++found;
            }
    }
    *count = found;
    return bad;
}

// mode 0: over the windows; 1: every post of every tile.
extern "C" int emul_summit_snap(const EmulGeoTile* tiles, uint32_t n_tiles, uint32_t tile_w, uint32_t tile_h, const double* lonlat, uint32_t n, double radius, int mode,
                                EmulSnap* out) {
    EmulSummitScene scene(tiles, n_tiles, tile_w, tile_h);
    const LosScene& S = scene.S;
    int bad = 0;
    auto chk = [&](bool ok, uint64_t) { if (!ok) ++bad; return ok; };
    for (uint32_t i = 0; i < n; ++i) {
        EmulSnap o{};
        const double lon = lonlat[2 * (size_t)i], lat = lonlat[2 * (size_t)i + 1];
        if (!surface_point_valid(lon, lat)) {
            o.status = kSnapInvalid;
        } else {
            SummitBest b;
            if (mode == 0) summit_snap(S, lon, lat, radius, b, chk);
            else snap_all(S, lon, lat, radius, b, chk);
            if (b.found) {
                o.status = kSnapFound;
                o.lon_deg = summit_lon(S.tiles[b.rank], b.idx % tile_w);
                o.lat_deg = summit_lat(S.tiles[b.rank], b.idx / tile_w);
                o.distance_m = b.d;
                o.height_m = b.h;
                o.rank = b.rank;
                o.idx = b.idx;
            }
        }
        out[i] = o;
    }
    return bad;
}
