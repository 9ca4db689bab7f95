// tests/cover_emul.cpp -- TEST-ONLY g++ build of the lane bodies of the covered-region path (topo_pipeline.h: setup_covers_region /
// item_covers_region, big_cover_lane), run lane by lane under a bounds-checking sink, and of a whole near phase as the kernels
// order it (k_raster and k_raster_rare's in-lane fragments -> k_raster_cover -> k_raster_big), so that the tests can say which
// scenes exercise which branch without a GPU.  Nothing in the product links or loads it.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../topo-renderer_amd/csrc/topo_pipeline.h"
#include "emul_tiles.h"

using namespace topo;

namespace {

constexpr int kRows = 16;      // k_raster_cover: rows per wave (kernels_frame.h: kCoverRows)

bool setup_of(const int32_t* X, const int32_t* Y, const float* z, int W, int H, TriSetup& ts) {
    SVert s[3];
    for (int k = 0; k < 3; ++k) { s[k].X = X[k]; s[k].Y = Y[k]; s[k].z = z ? z[k] : 0.5f; s[k].flag = kVtxOk; }
    return triangle_setup(s[0], s[1], s[2], W, H, ts);
}

// every lane of the four waves of a k_raster_cover workgroup; sink(pix, key, row of the region)
template <typename Sink>
void cover_item_lanes(const TriSetup& ts, bool narrow, uint32_t id, int W, int H, int rx, int ry, Sink&& sink) {
    for (int wave = 0; wave < 64 / kRows; ++wave)
        for (uint32_t lane = 0; lane < 64; ++lane)
            big_cover_lane<kRows>(ts, narrow, id, W, H, rx, ry, wave * kRows, lane, [&](size_t pix, uint64_t key, int j) { sink(pix, key, wave * kRows + j); });
}

}  // namespace

extern "C" {

int emul_item_covers(const int32_t* X, const int32_t* Y, int W, int H, int rx, int ry) { return item_covers_region(X, Y, W, H, rx, ry) ? 1 : 0; }

// the definition, by brute force: triangle_pixel accepts every pixel centre of the region's box inside the target (depths 0.5: the
// far plane never clips), and that box is not empty
int emul_covers_brute(const int32_t* X, const int32_t* Y, int W, int H, int rx, int ry) {
    TriSetup ts;
    if (rx < 0 || ry < 0 || !setup_of(X, Y, nullptr, W, H, ts)) return 0;
    const int x0 = rx * 64, y0 = ry * 64, x1 = x0 + 63 < W - 1 ? x0 + 63 : W - 1, y1 = y0 + 63 < H - 1 ? y0 + 63 : H - 1;
    if (x0 > x1 || y0 > y1) return 0;
    for (int py = y0; py <= y1; ++py) for (int px = x0; px <= x1; ++px) {
        float z, b[3];
        if (px < ts.px0 || px > ts.px1 || py < ts.py0 || py > ts.py1 || !triangle_pixel(ts, px, py, z, b)) return 0;
    }
    return 1;
}

// Every lane of big_cover_lane over region (rx, ry), whatever the triangle (a covering one or not: the walk must stay inside the
// region and the target either way).  Returns the violations of the sink: an index outside the target or outside the region, a row
// number that is not the pixel's, a pixel emitted twice.  keys (W * H, caller-initialised to kVisClear) receives the keys;
// n_frag: fragments emitted; n_missing: pixels of the region inside the target that triangle_pixel accepts and the walk left out;
// n_wrong: emitted keys that are not vis_key(triangle_pixel(...)) (or whose pixel triangle_pixel rejects).
int emul_cover_item(const int32_t* X, const int32_t* Y, const float* z, uint32_t id, int W, int H, int rx, int ry, uint64_t* keys, uint32_t* n_frag,
                    uint32_t* n_missing, uint32_t* n_wrong) {
    *n_frag = *n_missing = *n_wrong = 0;
    TriSetup ts;
    if (!setup_of(X, Y, z, W, H, ts)) return 0;
    int violations = 0;
    std::vector<uint8_t> seen((size_t)W * H, 0);
    cover_item_lanes(ts, giant_narrow(X, Y), id, W, H, rx, ry, [&](size_t pix, uint64_t key, int row) {
        if (pix >= (size_t)W * H) { ++violations; return; }
        const int px = (int)(pix % W), py = (int)(pix / W);
        if (px < rx * 64 || px > rx * 64 + 63 || py < ry * 64 || py > ry * 64 + 63 || py != ry * 64 + row) ++violations;
        if (seen[pix]) ++violations;
        seen[pix] = 1;
        keys[pix] = key;
        ++*n_frag;
        float zz, b[3];
        if (!triangle_pixel(ts, px, py, zz, b) || vis_key(zz, id) != key) ++*n_wrong;
    });
    for (int py = ry * 64; py < ry * 64 + 64 && py < H; ++py) for (int px = rx * 64; px < rx * 64 + 64 && px < W; ++px) {
        float zz, b[3];
        if (px >= ts.px0 && px <= ts.px1 && py >= ts.py0 && py <= ts.py1 && triangle_pixel(ts, px, py, zz, b) && !seen[(size_t)py * W + px]) ++*n_missing;
    }
    return violations;
}

// The near phase of one view as the kernels order it, every block taken as a near block (the scenes of the tests have no far phase):
//   old     what k_raster draws in-wave (boxes under 5 rows x 24 columns) and k_raster_rare in-lane (boxes up to 4 x 4): the keys and
//           segment marks k_raster_cover finds;
//   cover   per region, the covering items of k_raster_rare's triangles (setup_covers_region): the first claims the region and is
//           written row by row as k_raster_cover does -- a row none of whose segments is marked by a plain store (it must find
//           kVisClear there), a marked row by min(old, mine);
//   rest    every other big item by min, as k_raster_big's atomics.
// key_base: index of the view's first key in the submission's buffer (segments are counted from the buffer's start).
// stats[0] covering items, [1] claims won, [2] claims lost, [3] claimed regions where an older key beats EVERY covering item's key at some
// pixel, [4] rows stored blind, [5] rows merged, [6] keys that differ from the plain minimum over all fragments (must be 0), [7] blind
// stores that found a key other than kVisClear (must be 0), [8] big items, [9] violations of the cover walk's sink.
// Tiles in draw order.  keys_out (W * H, or null): the final keys.
int emul_cover_frame(const EmulTile* tiles, uint32_t n_tiles, uint32_t tile_w, uint32_t tile_h, const float* uniforms40, int W, int H, uint64_t key_base,
                     uint64_t* stats, uint64_t* keys_out) {
    for (int i = 0; i < 10; ++i) stats[i] = 0;
    ViewDev view{};
    memcpy(view.proj, uniforms40, 64);
    struct Item { int32_t X[3], Y[3]; float z[3]; uint32_t id; int rx, ry; bool covers; };
    std::vector<Item> items;
    const size_t n_px = (size_t)W * H;
    std::vector<uint64_t> old(n_px, kVisClear), plain(n_px, kVisClear);
    std::vector<uint8_t> mark((key_base + n_px + 63) / 64 + 1, 0);
    auto draw_all = [&](const TriSetup& ts, uint32_t id, bool is_old) {
        for (int py = ts.py0; py <= ts.py1; ++py) for (int px = ts.px0; px <= ts.px1; ++px) {
            float z, b[3];
            if (!triangle_pixel(ts, px, py, z, b)) continue;
            const size_t pix = (size_t)py * W + px;
            const uint64_t key = vis_key(z, id);
            if (key < plain[pix]) plain[pix] = key;
            if (is_old) {
                if (key < old[pix]) old[pix] = key;
                mark[(key_base + pix) >> 6] = 1;
            }
        }
    };
    auto enqueue = [&](const SVert* s, const TriSetup& ts, uint32_t id, bool from_rare) {
        for (int ry = ts.py0 >> 6; ry <= ts.py1 >> 6; ++ry) for (int rx = ts.px0 >> 6; rx <= ts.px1 >> 6; ++rx) {
            Item it;
            for (int k = 0; k < 3; ++k) { it.X[k] = s[k].X; it.Y[k] = s[k].Y; it.z[k] = s[k].z; }
            it.id = id; it.rx = rx; it.ry = ry;
            it.covers = from_rare && setup_covers_region(ts, W, H, rx, ry);
            items.push_back(it);
        }
        draw_all(ts, id, false);
    };
    const FastDiv div_hm1 = fastdiv_make(tile_h - 1);
    const uint32_t tris_per_tile = 2u * (tile_w - 1) * (tile_h - 1);
    std::vector<std::vector<float>> trig(n_tiles);
    for (uint32_t rank = 0; rank < n_tiles; ++rank) {
        TileDev t = make_dev(tiles[rank]);
        trig[rank].resize(2 * (size_t)(tile_w + tile_h));
        for (uint32_t x = 0; x < tile_w; ++x) sincos_f(vertex_lon(t, x), trig[rank][2 * x], trig[rank][2 * x + 1]);
        for (uint32_t y = 0; y < tile_h; ++y) sincos_f(vertex_lat(t, y), trig[rank][2 * (tile_w + y)], trig[rank][2 * (tile_w + y) + 1]);
        t.trig_lon = trig[rank].data();
        t.trig_lat = trig[rank].data() + 2 * (size_t)tile_w;
        std::vector<SVert> sv((size_t)tile_w * tile_h);
        for (uint32_t vy = 0; vy < tile_h; ++vy) for (uint32_t vx = 0; vx < tile_w; ++vx) {
            float clip[4];
            vertex_clip(t, view, vx, vy, t.heights[(size_t)vy * tile_w + vx], clip);
            clip_to_screen(clip, (float)W, (float)H, sv[(size_t)vy * tile_w + vx]);
        }
        for (uint32_t i = 0; i + 1 < tile_w; ++i) for (uint32_t j = 0; j + 1 < tile_h; ++j) {
            const SVert a = sv[(size_t)j * tile_w + i], b = sv[(size_t)(j + 1) * tile_w + i];
            const SVert c = sv[(size_t)j * tile_w + i + 1], d = sv[(size_t)(j + 1) * tile_w + i + 1];
            const bool even = ((i + j) & 1u) == 0;
            for (uint32_t k = 0; k < 2; ++k) {
                const SVert s[3] = {k == 0 ? a : d, k == 0 ? b : c, k == 0 ? (even ? d : c) : (even ? a : b)};
                const uint32_t tri = (i * (tile_h - 1) + j) * 2 + k, draw = rank * tris_per_tile + tri;
                const int fg = s[0].flag | s[1].flag | s[2].flag;
                bool rare = false;
                if (fg == kVtxOk) {      // classify_small
                    if (!spans_fit_int32(s[0].X, s[0].Y, s[1].X, s[1].Y, s[2].X, s[2].Y)) rare = true;
                    else {
                        TriSetup ts;
                        if (!triangle_setup(s[0], s[1], s[2], W, H, ts)) continue;
                        if (ts.py1 - ts.py0 >= 5 || ts.px1 - ts.px0 >= 24) enqueue(s, ts, draw << 1, false);      // kInlaneRows, kInlaneCols
                        else draw_all(ts, draw << 1, true);
                    }
                } else if (fg & kVtxNear) {
                    rare = (s[0].flag == kVtxNear) + (s[1].flag == kVtxNear) + (s[2].flag == kVtxNear) != 3;
                }
                if (!rare) continue;
                for (uint32_t fan = 0; fan < 2; ++fan) {      // k_raster_rare
                    ResolvedTri r;
                    if (!resolve_triangle(t, tile_w, div_hm1, tile_h - 1, view, W, H, tri, fan, r)) continue;
                    const uint32_t id = (draw << 1) | fan;
                    if (r.ts.px1 - r.ts.px0 + 1 <= 4 && r.ts.py1 - r.ts.py0 + 1 <= 4) draw_all(r.ts, id, true);
                    else enqueue(r.s, r.ts, id, true);
                }
            }
        }
    }
    stats[8] = items.size();
    // claims: the first covering item of a region (any one may win on the GPU: the counts and the keys do not depend on which)
    const int regions_x = (W + 63) / 64, regions_y = (H + 63) / 64;
    std::vector<int> owner((size_t)regions_x * regions_y, -1);
    for (size_t i = 0; i < items.size(); ++i)
        if (items[i].covers) {
            ++stats[0];
            int& o = owner[(size_t)items[i].ry * regions_x + items[i].rx];
            if (o < 0) { o = (int)i; ++stats[1]; } else ++stats[2];
        }
    // k_raster_cover
    std::vector<uint64_t> vis = old;
    std::vector<uint8_t> mark_new = mark;
    for (size_t r = 0; r < owner.size(); ++r) {
        if (owner[r] < 0) continue;
        const Item& it = items[(size_t)owner[r]];
        TriSetup ts;
        if (!setup_of(it.X, it.Y, it.z, W, H, ts)) return -1;
        const int x0 = it.rx * 64, x1 = x0 + 63 < W - 1 ? x0 + 63 : W - 1;
        uint8_t row_marked[64];
        for (int row = 0; row < 64; ++row) {
            const int y = it.ry * 64 + row;
            row_marked[row] = 0;
            if (y >= H) continue;
            const size_t first = key_base + (size_t)y * W, s0 = (first + x0) >> 6, s1 = (first + x1) >> 6;
            row_marked[row] = mark[s0] | mark[s1];      // (the marks as the kernels before this launch left them)
            ++stats[row_marked[row] ? 5 : 4];
            mark_new[s0] = mark_new[s1] = 1;
        }
        cover_item_lanes(ts, giant_narrow(it.X, it.Y), it.id, W, H, it.rx, it.ry, [&](size_t pix, uint64_t key, int row) {
            if (pix >= n_px || row < 0 || row > 63 || (int)(pix / W) != it.ry * 64 + row || (int)(pix % W) < x0 || (int)(pix % W) > x1) { ++stats[9]; return; }
            if (row_marked[row]) vis[pix] = key < vis[pix] ? key : vis[pix];
            else {
                if (vis[pix] != kVisClear) ++stats[7];
                vis[pix] = key;
            }
        });
        // does an older key beat every covering item of the region somewhere?
        std::vector<uint64_t> best(64 * 64, kVisClear);
        for (const Item& c : items)
            if (c.covers && c.rx == it.rx && c.ry == it.ry) {
                TriSetup cs;
                if (!setup_of(c.X, c.Y, c.z, W, H, cs)) return -1;
                cover_item_lanes(cs, giant_narrow(c.X, c.Y), c.id, W, H, c.rx, c.ry, [&](size_t pix, uint64_t key, int row) {
                    uint64_t& q = best[(size_t)row * 64 + (pix % W - x0)];
                    q = key < q ? key : q;
                });
            }
        bool older = false;
        for (int row = 0; row < 64 && it.ry * 64 + row < H; ++row) for (int x = x0; x <= x1; ++x)
            older = older || old[(size_t)(it.ry * 64 + row) * W + x] < best[(size_t)row * 64 + (x - x0)];
        stats[3] += older ? 1 : 0;
    }
    // k_raster_big: everything that did not claim
    for (size_t i = 0; i < items.size(); ++i) {
        const Item& it = items[i];
        if (it.covers && owner[(size_t)it.ry * regions_x + it.rx] == (int)i) continue;
        TriSetup ts;
        if (!setup_of(it.X, it.Y, it.z, W, H, ts)) return -1;
        for (int py = it.ry * 64; py < it.ry * 64 + 64; ++py) for (int px = it.rx * 64; px < it.rx * 64 + 64; ++px) {
            float z, b[3];
            if (px < ts.px0 || px > ts.px1 || py < ts.py0 || py > ts.py1 || !triangle_pixel(ts, px, py, z, b)) continue;
            const uint64_t key = vis_key(z, it.id);
            uint64_t& q = vis[(size_t)py * W + px];
            q = key < q ? key : q;
        }
    }
    for (size_t p = 0; p < n_px; ++p) stats[6] += vis[p] != plain[p];
    if (keys_out) memcpy(keys_out, vis.data(), n_px * 8);
    return 0;
}

}  // extern "C"
