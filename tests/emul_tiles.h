// tests/emul_tiles.h -- the tile records the TEST-ONLY g++ builds take over ctypes (tests/emul_tiles.py declares the same two), and
// what turns them into the product's TileDev and its f64 trig table.
#pragma once
#include <cstdint>

#include "../topo-renderer_amd/csrc/topo_ground.h"

struct EmulTile {          // host_emul.cpp, cover_emul.cpp: a tile with its normals
    const float* heights;
    uint32_t* normals;
    float tu[24];          // TerrainUniforms, 96 B
};

inline topo::TileDev make_dev(const EmulTile& e) {
    topo::TileDev t{};
    t.heights = e.heights; t.normals = e.normals; t.block_minmax = nullptr;
    t.raster_x = e.tu[0]; t.raster_y = e.tu[1]; t.model_x = e.tu[2]; t.model_y = e.tu[3];
    t.scale_x = e.tu[4]; t.scale_y = e.tu[5];
    for (int c = 0; c < 3; ++c) for (int r = 0; r < 3; ++r) t.rot[c * 3 + r] = e.tu[8 + c * 4 + r];
    return t;
}

struct EmulGeoTile {       // ground_emul.cpp, los_emul.cpp, surface_emul.cpp: a tile of the queries, which read no normals
    const float* heights;
    float tf[6];           // raster_point, model_point, pixel_scale
    int32_t lat, lon;
};

inline topo::TileDev make_dev(const EmulGeoTile& e) {
    topo::TileDev t{};
    t.heights = e.heights;
    t.raster_x = e.tf[0]; t.raster_y = e.tf[1];
    t.model_x = e.tf[2]; t.model_y = e.tf[3];
    t.scale_x = e.tf[4]; t.scale_y = e.tf[5];
    return t;
}

// The tile's f64 (cos, sin) table, ground_table_doubles(tile_w, tile_h) doubles at tg, with the functions k_ground_tables calls.
inline void fill_trig(const topo::TileDev& t, uint32_t tile_w, uint32_t tile_h, double* tg) {
    for (uint32_t x = 0; x < tile_w; ++x) topo::ground_trig_lon(t, x, tg[2 * x], tg[2 * x + 1]);
    for (uint32_t y = 0; y < tile_h; ++y) topo::ground_trig_lat(t, y, tg[2 * (tile_w + y)], tg[2 * (tile_w + y) + 1]);
}
