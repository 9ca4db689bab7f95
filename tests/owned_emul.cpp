// tests/owned_emul.cpp -- TEST-ONLY g++ build of what the owned strips of k_resolve rest on (topo_pipeline.h): the index function
// of the strip records as k_raster_cover and k_resolve call it, and the record route over one strip -- resolve_setup at the strip's
// origin without the normal table (k_raster_cover's call), then resolve_pixel -- against resolve_varyings.  Nothing in the product
// links or loads it.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../topo-renderer_amd/csrc/topo_pipeline.h"
#include "emul_tiles.h"

using namespace topo;

extern "C" {

// k_raster_cover's side: region r of the owner words (cover_region_index's order), lane s < 8 for the strip of rows 8 s .. if it
// starts inside the target.  out: the record indices, xy: (view, x, y) of each strip's origin.  Returns their number; *cap = the
// table's records.
uint64_t emul_owned_producer(uint32_t W, uint32_t H, uint32_t n_views, uint64_t* out, uint32_t* xy, uint64_t* cap) {
    const uint32_t regions_x = (W + 63) / 64, regions_y = (H + 63) / 64;
    const uint32_t regions = n_views * regions_x * regions_y;
    *cap = (uint64_t)regions * kOwnedStrips;
    uint64_t n = 0;
    for (uint32_t r = 0; r < regions; ++r) {
        const uint32_t view = r / (regions_x * regions_y), in_view = r % (regions_x * regions_y);
        const int32_t ry = (int32_t)(in_view / regions_x), rx = (int32_t)(in_view % regions_x);
        for (uint32_t s = 0; s < kOwnedStrips; ++s) {
            const int32_t x = rx * 64, y = ry * 64 + (int32_t)(s * kOwnedStripRows);
            if (y >= (int32_t)H) continue;
            out[n] = owned_record_index(regions_x, regions_y, view, x, y);
            xy[3 * n] = view; xy[3 * n + 1] = (uint32_t)x; xy[3 * n + 2] = (uint32_t)y;
            ++n;
        }
    }
    return n;
}

// k_resolve's side: its blocks of 64 x 32 px in launch order (resolve_block), wave w's strip of rows 8 w .. of each, if it starts
// inside the target.
uint64_t emul_owned_consumer(uint32_t W, uint32_t H, uint32_t n_views, uint64_t* out, uint32_t* xy) {
    const uint32_t regions_x = (W + 63) / 64, regions_y = (H + 63) / 64;
    const uint32_t rblocks_x = (W + 63) / 64, rblocks_view = rblocks_x * ((H + 31) / 32);
    uint64_t n = 0;
    for (uint32_t b = 0; b < rblocks_view * n_views; ++b) {
        const uint32_t view = b / rblocks_view, in_view = b % rblocks_view, row = in_view / rblocks_x;
        const int32_t bx = (int32_t)(in_view - row * rblocks_x) * 64, by = (int32_t)row * 32;
        for (int32_t wave = 0; wave < 4; ++wave) {
            const int32_t y0 = by + 8 * wave;
            if (y0 >= (int32_t)H) continue;
            out[n] = owned_record_index(regions_x, regions_y, view, bx, y0);
            xy[3 * n] = view; xy[3 * n + 1] = (uint32_t)bx; xy[3 * n + 2] = (uint32_t)y0;
            ++n;
        }
    }
    return n;
}

// The record route over the strip at (ox, oy) for winner `id`: the record as k_raster_cover computes it (words36: its 34 words, then
// id and 0), every pixel of the strip inside the target finished by resolve_pixel and compared, bit for bit, with resolve_varyings
// (through k_resolve's table of the normal decode).  Returns the pixels that differ; *kind = the record's kind.  Tiles in draw order.
int emul_owned_route(const EmulTile* tiles, uint32_t n_tiles, uint32_t tile_w, uint32_t tile_h, const float* uniforms40, int W, int H, uint32_t id, int ox, int oy,
                     int* kind, uint32_t* words36) {
    ViewDev view{};
    memcpy(view.proj, uniforms40, 64);
    view.cam_x = uniforms40[32]; view.cam_y = uniforms40[33];
    const uint32_t tris_per_tile = 2u * (tile_w - 1) * (tile_h - 1);
    const FastDiv div_hm1 = fastdiv_make(tile_h - 1), div_tris = fastdiv_make(tris_per_tile);
    const uint32_t draw = id >> 1, fan = id & 1u, rank = fastdiv(draw, div_tris), tri = draw - rank * tris_per_tile;
    if (rank >= n_tiles) return -1;
    TileDev t = make_dev(tiles[rank]);
    std::vector<float> trig(2 * (size_t)(tile_w + tile_h));
    for (uint32_t x = 0; x < tile_w; ++x) sincos_f(vertex_lon(t, x), trig[2 * x], trig[2 * x + 1]);
    for (uint32_t y = 0; y < tile_h; ++y) sincos_f(vertex_lat(t, y), trig[2 * (tile_w + y)], trig[2 * (tile_w + y) + 1]);
    t.trig_lon = trig.data();
    t.trig_lat = trig.data() + 2 * (size_t)tile_w;
    float ndec[256];
    for (uint32_t c = 0; c < 256; ++c) ndec[c] = normal_channel(c);
    TriRecord rec;
    resolve_setup<false>(t, tile_w, div_hm1, tile_h - 1, view, W, H, tri, fan, nullptr, ox, oy, rec);
    memcpy(words36, &rec, sizeof rec);
    words36[kOwnedIdWord] = id;
    words36[kOwnedSerialWord] = 0;
    *kind = (int)rec.kind;
    int differ = 0;
    for (int py = oy; py < oy + (int)kOwnedStripRows && py < H; ++py)
        for (int px = ox; px < ox + 64 && px < W; ++px) {
            f3 a = {0.0f, 0.0f, 0.0f}, an = {0.0f, 0.0f, 0.0f}, b = {0.0f, 0.0f, 0.0f}, bn = {0.0f, 0.0f, 0.0f};
            const bool oka = resolve_pixel(rec, pixel_at(W, H, px, py, ox, oy), a.x, a.y, an);
            const bool okb = resolve_varyings<true>(t, tile_w, div_hm1, tile_h - 1, view, W, H, tri, fan, ndec, px, py, b, bn);
            const bool same = oka == okb && (!oka || (f_bits(a.x) == f_bits(b.x) && f_bits(a.y) == f_bits(b.y) && f_bits(an.x) == f_bits(bn.x) &&
                                                      f_bits(an.y) == f_bits(bn.y) && f_bits(an.z) == f_bits(bn.z)));
            differ += same ? 0 : 1;
        }
    return differ;
}

}  // extern "C"
