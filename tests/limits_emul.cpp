// tests/limits_emul.cpp -- TEST-ONLY driver: the lane bodies of k_raster (raster_rows) and k_raster_big (big_medium_lane,
// big_giant_lane) from topo-renderer_amd/csrc/topo_pipeline.h on targets at the size limits the host accepts (65536 px a
// side, up to 2^32 - 1 px in one view), with triangles up to the +-2^20 px guard band.  tests/test_emul_cpu.py builds it
// twice, optimised and under UBSan, and runs each build in a subprocess; every signed overflow in the header's index
// arithmetic ends the sanitised run.
//
// The sinks hold one 64 x 64 region (big items) or one triangle's pixel box (raster_rows), not the target: every fragment
// must lie in the target and in that window, be emitted once, and carry the key triangle_setup / triangle_pixel give.
// `limits_emul split` checks region_split_row, k_raster_rare's split of a triangle's regions, against plain division.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "../topo-renderer_amd/csrc/topo_pipeline.h"

using namespace topo;

namespace {

struct Rng {      // splitmix64
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
    double uni(double a, double b) { return a + (b - a) * (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
    int64_t below(int64_t n) { return (int64_t)(next() % (uint64_t)n); }
};

struct Stats {
    long violations = 0, mismatches = 0, items_medium = 0, items_narrow = 0, items_wide = 0, rows_tris = 0, frags = 0;
    long frags_high = 0;          // fragments at pixel index >= 2^31 of the view
    long frags_last_row = 0, frags_last_col = 0, frags_first_row = 0, frags_first_col = 0;
};

// A window [x0, x0 + w) x [y0, y0 + h) of a W x H target.  Fragments land at their view-wide pixel index.
struct Window {
    int64_t W, H, x0, y0, w, h;
    std::vector<uint64_t> keys;
    std::vector<uint8_t> seen;
    long n = 0, bad = 0;
    Window(int64_t W_, int64_t H_, int64_t x0_, int64_t y0_, int64_t x1, int64_t y1)
        : W(W_), H(H_), x0(x0_), y0(y0_), w(x1 - x0_ + 1), h(y1 - y0_ + 1), keys((size_t)(w * h), kVisClear), seen((size_t)(w * h), 0) {}
    void emit(uint64_t pix, uint64_t key, Stats& st) {
        if (pix >= (uint64_t)(W * H)) { ++bad; return; }
        const int64_t px = (int64_t)(pix % (uint64_t)W), py = (int64_t)(pix / (uint64_t)W);
        if (px < x0 || px >= x0 + w || py < y0 || py >= y0 + h) { ++bad; return; }
        const size_t i = (size_t)((py - y0) * w + (px - x0));
        if (seen[i]) ++bad;
        seen[i] = 1;
        if (key < keys[i]) keys[i] = key;
        ++n;
        st.frags += 1;
        st.frags_high += pix >= (1ull << 31);
        st.frags_last_row += py == H - 1;
        st.frags_last_col += px == W - 1;
        st.frags_first_row += py == 0;
        st.frags_first_col += px == 0;
    }
    // the same window through the generic path the oracle-parity tests pin
    bool matches_reference(const int32_t X[3], const int32_t Y[3], const float z[3], uint32_t id) const {
        std::vector<uint64_t> ref((size_t)(w * h), kVisClear);
        long nr = 0;
        SVert s[3];
        for (int k = 0; k < 3; ++k) { s[k].X = X[k]; s[k].Y = Y[k]; s[k].z = z[k]; s[k].flag = kVtxOk; }
        TriSetup ts;
        if (triangle_setup(s[0], s[1], s[2], (int32_t)W, (int32_t)H, ts))
            for (int64_t py = y0 > ts.py0 ? y0 : ts.py0; py <= ts.py1 && py < y0 + h; ++py)
                for (int64_t px = x0 > ts.px0 ? x0 : ts.px0; px <= ts.px1 && px < x0 + w; ++px) {
                    float zz, b[3];
                    if (triangle_pixel(ts, (int32_t)px, (int32_t)py, zz, b)) {
                        ref[(size_t)((py - y0) * w + (px - x0))] = vis_key(zz, id);
                        ++nr;
                    }
                }
        return nr == n && ref == keys;
    }
};

// One BigItem (triangle, region) through the 64 lanes of k_raster_big, as emul_big_item in host_emul.cpp runs it.
void run_big_item(const int32_t X[3], const int32_t Y[3], const float z[3], uint32_t id, int32_t W, int32_t H, int32_t rx, int32_t ry,
                  Stats& st) {
    const int64_t x1 = (int64_t)rx * 64 + 63 < W - 1 ? (int64_t)rx * 64 + 63 : W - 1, y1 = (int64_t)ry * 64 + 63 < H - 1 ? (int64_t)ry * 64 + 63 : H - 1;
    Window win(W, H, (int64_t)rx * 64, (int64_t)ry * 64, x1, y1);
    const bool medium = spans_fit_int32(X[0], Y[0], X[1], Y[1], X[2], Y[2]);
    for (uint32_t lane = 0; lane < 64; ++lane) {
        if (medium)
            big_medium_lane(X, Y, z, id, W, H, rx, ry, lane, [&](const uint32_t pix[4], const uint64_t key[4], const int32_t py[4]) {
                for (int k = 0; k < 4; ++k)
                    if (key[k] != kVisClear) {      // pix[k], py[k] are only meaningful with a key
                        if (py[k] < 0 || py[k] >= H || (uint64_t)py[k] != pix[k] / (uint64_t)W) ++win.bad;
                        win.emit(pix[k], key[k], st);
                    }
            });
        else
            big_giant_lane(X, Y, z, id, W, H, rx, ry, lane, [&](size_t pix, uint64_t key, int32_t py) {
                if (py < 0 || py >= H || (uint64_t)py != pix / (uint64_t)W) ++win.bad;
                win.emit(pix, key, st);
            });
    }
    if (medium) {
        ++st.items_medium;
    } else {
        const int64_t area2 = ((int64_t)X[1] - X[0]) * ((int64_t)Y[2] - Y[0]) - ((int64_t)Y[1] - Y[0]) * ((int64_t)X[2] - X[0]);
        if (area2 < 0) (-area2 < (1ll << 48) ? st.items_narrow : st.items_wide) += 1;      // big_giant_lane's `narrow`
    }
    st.violations += win.bad;
    if (!win.matches_reference(X, Y, z, id)) {
        if (st.mismatches < 5) fprintf(stderr, "big item mismatch: W=%d H=%d region (%d,%d) X=%d,%d,%d Y=%d,%d,%d\n", W, H, rx, ry, X[0], X[1], X[2], Y[0], Y[1], Y[2]);
        ++st.mismatches;
    }
}

void run_raster_rows(const int32_t X[3], const int32_t Y[3], const float z[3], uint32_t id, int32_t W, int32_t H, Stats& st) {
    if (!spans_fit_int32(X[0], Y[0], X[1], Y[1], X[2], Y[2])) return;
    const int32_t area2 = (X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0]);
    if (area2 >= 0) return;      // classify_small lists front-facing triangles only
    SVert s[3];
    for (int k = 0; k < 3; ++k) { s[k].X = X[k]; s[k].Y = Y[k]; s[k].z = z[k]; s[k].flag = kVtxOk; }
    TriSetup ts;
    if (!triangle_setup(s[0], s[1], s[2], W, H, ts)) return;      // nothing on the target: k_raster drops it
    Window win(W, H, ts.px0, ts.py0, ts.px1, ts.py1);
    raster_rows(W, H, X[0], Y[0], X[1], Y[1], X[2], Y[2], z[0], z[1], z[2], id, [&](uint32_t pix, uint64_t key) { win.emit(pix, key, st); });
    ++st.rows_tris;
    st.violations += win.bad;
    if (!win.matches_reference(X, Y, z, id)) {
        if (st.mismatches < 5) fprintf(stderr, "raster_rows mismatch: W=%d H=%d X=%d,%d,%d Y=%d,%d,%d\n", W, H, X[0], X[1], X[2], Y[0], Y[1], Y[2]);
        ++st.mismatches;
    }
}

// Triangles of every size class from sub-pixel to the guard band, anchored at the target's corners, its last row and column
// and at random, some slivers, some degenerate, both windings, depths that cross both clamps.
void run_target(int32_t W, int32_t H, int n_tris, Rng& rng, Stats& st) {
    static const double sizes[] = {0.7, 3.0, 12.0, 40.0, 63.9, 200.0, 3000.0, 65536.0, 524288.0, 1048576.0};
    for (int i = 0; i < n_tris; ++i) {
        const int kind = i % 10;
        const double size = sizes[kind];
        double ax, ay;
        switch ((i / 10) % 7) {
            case 0: ax = 0.0; ay = 0.0; break;
            case 1: ax = W - 1.0; ay = 0.0; break;
            case 2: ax = 0.0; ay = H - 1.0; break;
            case 3: ax = W - 1.0; ay = H - 1.0; break;
            case 4: ax = rng.uni(0, W); ay = H - 1.0; break;
            case 5: ax = W - 1.0; ay = rng.uni(0, H); break;
            default: ax = rng.uni(-0.1 * W, 1.1 * W); ay = rng.uni(-0.1 * H, 1.1 * H); break;
        }
        double px[3], py[3];
        for (int k = 0; k < 3; ++k) { px[k] = ax + rng.uni(-size, size); py[k] = ay + rng.uni(-size, size); }
        if (i % 3 == 0) { px[0] = ax + rng.uni(-0.6, 0.6); py[0] = ay + rng.uni(-0.6, 0.6); }      // a vertex on the anchor pixel itself
        if (i % 17 == 5) {                                                                       // sliver
            const double t = rng.uni(0, 1);
            px[2] = px[0] + t * (px[1] - px[0]) + rng.uni(-0.3, 0.3);
            py[2] = py[0] + t * (py[1] - py[0]) + rng.uni(-0.3, 0.3);
        }
        int32_t X[3], Y[3];
        float z[3];
        for (int k = 0; k < 3; ++k) {      // snapped as clip_to_screen does, inside the guard band |coord| <= 2^20 px
            const double gx = std::fmin(std::fmax(px[k], -1048576.0), 1048576.0), gy = std::fmin(std::fmax(py[k], -1048576.0), 1048576.0);
            X[k] = (int32_t)std::nearbyint(gx * 256.0);
            Y[k] = (int32_t)std::nearbyint(gy * 256.0);
            z[k] = i % 7 == 0 ? (float)rng.uni(-0.2, 1.3) : (float)rng.uni(0.0, 1.05);
        }
        if (i % 13 == 0) { X[1] = X[0]; Y[1] = Y[0]; }      // degenerate
        if (rng.next() & 1) { std::swap(X[1], X[2]); std::swap(Y[1], Y[2]); std::swap(z[1], z[2]); }      // back faces emit nothing
        const uint32_t id = 2u * (uint32_t)i;
        run_raster_rows(X, Y, z, id, W, H, st);
        // the BigItems enqueue_big / k_raster_rare cut the triangle into (one per 64 x 64 region of its pixel box): the corner
        // regions of that box, the regions of its vertices, the target's last region and a few at random
        SVert s[3];
        for (int k = 0; k < 3; ++k) { s[k].X = X[k]; s[k].Y = Y[k]; s[k].z = z[k]; s[k].flag = kVtxOk; }
        TriSetup ts;
        if (!triangle_setup(s[0], s[1], s[2], W, H, ts)) {
            run_big_item(X, Y, z, id, W, H, 0, 0, st);      // nothing on the target: no lane may emit
            run_big_item(X, Y, z, id, W, H, (W - 1) >> 6, (H - 1) >> 6, st);
            continue;
        }
        const int32_t rx0 = ts.px0 >> 6, rx1 = ts.px1 >> 6, ry0 = ts.py0 >> 6, ry1 = ts.py1 >> 6;
        std::vector<std::pair<int32_t, int32_t>> regions = {{rx0, ry0}, {rx1, ry0}, {rx0, ry1}, {rx1, ry1}, {(W - 1) >> 6, (H - 1) >> 6}};
        for (int k = 0; k < 3; ++k) regions.push_back({(int32_t)(((int64_t)X[k] >> 8) >> 6), (int32_t)(((int64_t)Y[k] >> 8) >> 6)});
        for (int k = 0; k < 4; ++k) regions.push_back({rx0 + (int32_t)rng.below(rx1 - rx0 + 1), ry0 + (int32_t)rng.below(ry1 - ry0 + 1)});
        std::vector<std::pair<int32_t, int32_t>> done;
        for (auto r : regions) {
            r.first = r.first < rx0 ? rx0 : r.first > rx1 ? rx1 : r.first;
            r.second = r.second < ry0 ? ry0 : r.second > ry1 ? ry1 : r.second;
            bool dup = false;
            for (auto& d : done) dup |= d == r;
            if (dup) continue;
            done.push_back(r);
            run_big_item(X, Y, z, id, W, H, r.first, r.second, st);
        }
    }
}

// region_split_row against k / jw for every region column count jw <= 256 and every k < 2^17, on both sides of the n < 65536
// switch (the row depends on n only through it): 0 when exact.
long check_region_split() {
    long bad = 0;
    for (uint32_t jw = 1; jw <= 256; ++jw) {
        const uint32_t magic = region_split_magic(jw);
        for (uint32_t k = 0; k < (1u << 17); ++k) {
            const uint32_t want = k / jw;
            if (k < 65535u && region_split_row(k, jw, k + 1, magic) != want) ++bad;      // smallest block holding k
            if (k < 65535u && region_split_row(k, jw, 65535u, magic) != want) ++bad;     // largest multiply-shift block
            if (region_split_row(k, jw, 65536u, magic) != want) ++bad;
            if (region_split_row(k, jw, 1u << 17, magic) != want) ++bad;
        }
    }
    return bad;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc > 1 && strcmp(argv[1], "split") == 0) {
        const long bad = check_region_split();
        printf("split_mismatches %ld\n", bad);
        return bad == 0 ? 0 : 1;
    }
    const int n_tris = argc > 1 ? atoi(argv[1]) : 420;
    static const int32_t targets[][2] = {{65536, 64}, {64, 65536}, {65536, 40000}, {46341, 46341}};
    Stats st;
    Rng rng{20261016};
    for (const auto& t : targets) run_target(t[0], t[1], n_tris, rng, st);
    printf("violations %ld\nmismatches %ld\nitems_medium %ld\nitems_narrow %ld\nitems_wide %ld\nrows_tris %ld\nfrags %ld\n"
           "frags_high %ld\nfrags_last_row %ld\nfrags_last_col %ld\nfrags_first_row %ld\nfrags_first_col %ld\n",
           st.violations, st.mismatches, st.items_medium, st.items_narrow, st.items_wide, st.rows_tris, st.frags, st.frags_high,
           st.frags_last_row, st.frags_last_col, st.frags_first_row, st.frags_first_col);
    return st.violations == 0 && st.mismatches == 0 ? 0 : 1;
}
