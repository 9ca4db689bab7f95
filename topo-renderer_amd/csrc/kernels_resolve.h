// kernels_resolve.h -- k_resolve<kSrgb, kBgra>: the frame's last kernel: fs_main for the winner of every pixel, then the post pass
// (render_shader.wgsl fs_main, postprocessing_shader.wgsl).
//
// A workgroup takes 64 x (4 kRPW) px blocks (kRPW = TOPO_RESOLVE_RPW = 8: 64 x 32); wave w shades rows kRPW w .. kRPW w + kRPW - 1
// of each (a 64 x kRPW px strip) on its own: its own halo, depth tile and record table, no barrier once the tables are staged
// (see k_resolve).
//
// The grid is PERSISTENT (four times the resident workgroups) and each workgroup walks its blocks with a static stride,
// software-pipelined: a strip's shading needs two dependent trips to memory before it can start -- the segment marks that
// say whether anything was drawn there (about half of a panorama is sky: such a strip is written out as constants without
// reading a key; with every tap at depth 1 the contour term is exactly 0 and the post pass returns the cleared texel
// unchanged), then the visibility keys -- and at ~1.5 us per trip under load those two waits were three quarters of a
// block's 12 us in a one-block-per-workgroup kernel (measured: with ALL arithmetic removed it still took 0.38 of its
// 0.50 ms).  So the marks of up to 64 strips are read in one go (lane j: strip j); a strip's keys are requested when the strip
// starts (each lane reads the keys of its own kRPW pixels, 512-byte row segments, and three depth words of the ring around the
// strip) and the stores of the untouched strips go out under that trip -- requesting the keys a strip ahead, as rounds 2 and 3
// did, cost what it hid (see the strip loop); the sRGB tables are staged into LDS once per workgroup.
//
// Winners are shared: the near field consists of triangles tens to thousands of pixels large, and two thirds of a
// pixel's arithmetic (three vs_main, the perspective divides, the doubled area: resolve_setup) depends on the winning
// triangle alone.  Each wave therefore lists the distinct winners of its 256 pixels -- a lane starts a new entry when
// its id differs from its left neighbour's -- and computes their records densely, one triangle per lane, into a
// per-wave LDS table; the pixels then finish from the record (resolve_pixel: the values of the one-step resolve_varyings,
// bit for bit).  The table holds kRecCap = 20 records (at c4 a wave's 256 pixels share 6.7 winners on average); a wave that meets
// more takes its rows in groups that fit, and a single row with more than that (far field: a triangle or less per
// pixel) is shaded in one step per pixel.
//
// Round 3: the kernel is bound by instruction issue (vector AND scalar instructions take the SIMD's one issue slot), so
// the row loop carries no per-row selects any more: what a row needs of the listing pass -- each pixel's record slot, or
// its winner id where the row is shaded in one step -- waits in LDS (s_uid, s_slot), the output pointers advance by the pitch,
// the colour format is a template parameter, a record's kind-specific part is affine in the pixel (TriRecord), the
// positions of the ring entries are lane constants, and a row none of whose pixels can have a non-zero contour factor
// (decided by one comparison per pixel that can only err towards the long route) skips the post pass's divisions.
#pragma once

#include <type_traits>

#include "kernels_common.h"

namespace topo {
namespace {

constexpr int kRPW = TOPO_RESOLVE_RPW;             // pixel rows per wave
constexpr int kResolveRows = 4 * kRPW;
static_assert(kResolveRows == (int)kResolveBlockH && kResolveBlockW == 64u, "the host sizes k_resolve's block grid from these");
static_assert(kRPW == 4 || kRPW == 8, "RowN below names the rows of a wave");
#ifndef TOPO_RESOLVE_RECS
#define TOPO_RESOLVE_RECS 20      // (20 records + 5 workgroups per CU beat 32 + 4: the table's 4.6 KB are what the fifth workgroup's LDS needs)
#endif
constexpr uint32_t kRecCap = TOPO_RESOLVE_RECS;    // triangle records per wave
#ifndef TOPO_RESOLVE_WGS
#define TOPO_RESOLVE_WGS 5
#endif
// One value per row of a wave.  Named members, not an array: an array indexed by a loop variable goes to scratch memory.
template <typename T>
struct RowN {
    T a, b, c, d, e, f, g, h;
};
#if TOPO_RESOLVE_RPW == 8
#define TOPO_ROWS(X) X(0, a) X(1, b) X(2, c) X(3, d) X(4, e) X(5, f) X(6, g) X(7, h)
#else
#define TOPO_ROWS(X) X(0, a) X(1, b) X(2, c) X(3, d)
#endif

struct ResolveBlock {          // wave-uniform description of one 64 x (4 kRPW) block
    uint32_t view;
    int32_t bx, by;            // pixel origin
};
__device__ __forceinline__ ResolveBlock resolve_block(const FrameParams& P, uint32_t b) {
    const uint32_t view = P.rblocks_view > 1u ? fastdiv(b, P.div_rblocks_view) : b, in_view = b - view * P.rblocks_view;      // (fastdiv needs a divisor >= 2)
    const uint32_t row = P.rblocks_x > 1u ? fastdiv(in_view, P.div_rblocks_x) : in_view;
    return ResolveBlock{view, (int32_t)(in_view - row * P.rblocks_x) * 64, (int32_t)row * kResolveRows};
}
// Did anything write a key of wave `wave`'s strip (rows kRPW wave .. kRPW wave + kRPW - 1 of the block) or its halo?  Every row
// of strip + halo spans at most three 64-key segments; t < kStripMarks names one (row, segment) mark.
constexpr uint32_t kStripMarks = (kRPW + 2) * 3;
__device__ __forceinline__ bool resolve_strip_marked(const FrameParams& P, const ResolveBlock& B, uint32_t wave, uint32_t t) {
    const int32_t row = (int32_t)t / 3, k = (int32_t)t - row * 3;
    int32_t y = B.by + kRPW * (int32_t)wave + row - 1;
    y = y < 0 ? 0 : (y > P.H - 1 ? P.H - 1 : y);
    const int32_t x0 = B.bx > 0 ? B.bx - 1 : 0, x1 = B.bx + 64 < P.W ? B.bx + 64 : P.W - 1;
    // (32-bit key and mark numbers -- a submission has fewer than 2^32 pixels (the host refuses more) --: each of the strip's marks
    // is loaded with one vector register of offset from the array's scalar address, all of them in flight at once)
    const uint32_t first = B.view * (uint32_t)P.W * (uint32_t)P.H + (uint32_t)y * (uint32_t)P.W;
    const uint32_t seg = ((first + (uint32_t)x0) >> 6) + (uint32_t)k;
    const uint32_t last = (first + (uint32_t)x1) >> 6;
    const uint32_t at = seg <= last ? seg : last;    // (always a load, of a mark of this row: no branch around it)
    const bool mark = TOPO_CHK(P.counters, at < (((size_t)P.n_views * P.W * P.H + 63) >> 6), 12u, at) ? P.dirty[at] != 0 : false;
    return seg <= last && mark;
}
// What a lane holds of a strip: the keys of its own kRPW pixels and up to three depths of the ring around the strip:
// ring0 = the pixel above the lane's column (row -1), ring1 = the pixel below it (row kRPW), ring2 (lanes 0 .. 2 kRPW + 3) =
// columns -1 and 64 of rows -1 .. kRPW (lane = 2 (row + 1) + side).
struct ResolveKeys {
    RowN<uint32_t> id, raw;
    uint32_t ring0, ring1, ring2;
};
constexpr uint32_t kRing2Lanes = 2 * (kRPW + 2);
__device__ __forceinline__ void resolve_load_keys(const FrameParams& P, const ResolveBlock& B, uint32_t lane, uint32_t wave, ResolveKeys& K) {
    const uint64_t* vis = P.vis + (size_t)B.view * P.W * P.H;
    const int32_t px = B.bx + (int32_t)lane, sy = B.by + kRPW * (int32_t)wave;
    // (outside the target the positions clamp to the edge -- the depth sampler is clamp-to-edge (texture.rs:113-117) --; lanes /
    // rows beyond the target only feed the contour taps' LDS tile)
    const int32_t cx = px > P.W - 1 ? P.W - 1 : px;
    const int32_t ym = sy > 0 ? sy - 1 : 0;            // the row above the strip
    auto row_of = [&](int32_t y) { return y > P.H - 1 ? P.H - 1 : y; };      // (wave-uniform)
    const uint64_t* col = vis + cx;
#define TOPO_X(r, m)                                                      \
    {                                                                     \
        const uint64_t key = col[(size_t)row_of(sy + r) * P.W];           \
        K.id.m = (uint32_t)key;                                           \
        K.raw.m = (uint32_t)(key >> 32);                                  \
    }
    TOPO_ROWS(TOPO_X)
#undef TOPO_X
    // the ring: depth words only; every lane loads three (clamped positions: no branches around the loads)
    K.ring0 = reinterpret_cast<const uint32_t*>(col + (size_t)ym * P.W)[1];
    K.ring1 = reinterpret_cast<const uint32_t*>(col + (size_t)row_of(sy + kRPW) * P.W)[1];
    {
        const int32_t e = (int32_t)(lane < kRing2Lanes ? lane : kRing2Lanes - 1u);
        int32_t x = (e & 1) ? B.bx + 64 : B.bx - 1, y = sy + (e >> 1) - 1;
        x = x < 0 ? 0 : (x > P.W - 1 ? P.W - 1 : x);
        y = y < 0 ? 0 : (y > P.H - 1 ? P.H - 1 : y);
        K.ring2 = reinterpret_cast<const uint32_t*>(vis + (size_t)y * P.W + x)[1];
    }
}
// the winner id of one pixel again (rows shaded in one step per pixel, later record groups: both rare)
__device__ __forceinline__ uint32_t resolve_reload_id(const FrameParams& P, const ResolveBlock& B, int32_t px, int32_t py) {
    const int32_t cx = px > P.W - 1 ? P.W - 1 : px, cy = py > P.H - 1 ? P.H - 1 : py;
    return (uint32_t)P.vis[(size_t)B.view * P.W * P.H + (size_t)cy * P.W + cx];
}

template <bool kBgra>
__device__ __forceinline__ uint32_t surface_order(uint32_t c) {      // Rgba -> the surface's channel order
    return kBgra ? (c & 0xFF00FF00u) | ((c >> 16) & 0xFFu) | ((c & 0xFFu) << 16) : c;
}
template <bool kBgra>
__device__ __forceinline__ void resolve_fill_sky(const FrameParams& P, const OutputParams& O, const ResolveBlock& B, uint32_t lane, uint32_t wave) {
    const int32_t px = B.bx + (int32_t)lane;
    if (px >= P.W) return;
    const int32_t y0 = B.by + kRPW * (int32_t)wave;
    uint8_t* rgba = O.rgba + (size_t)B.view * O.rgba_view_stride + (size_t)y0 * O.rgba_pitch + (size_t)px * 4;
    uint8_t* depth = O.depth ? reinterpret_cast<uint8_t*>(O.depth) + (size_t)B.view * O.depth_view_stride + (size_t)y0 * O.depth_pitch + (size_t)px * 4 : nullptr;
    const uint32_t sky = surface_order<kBgra>(P.sky_c8);
    for (int32_t r = 0; r < kRPW && y0 + r < P.H; ++r, rgba += O.rgba_pitch) {
        *reinterpret_cast<uint32_t*>(rgba) = sky;
        if (depth) { *reinterpret_cast<float*>(depth) = 1.0f; depth += O.depth_pitch; }
    }
}

// The four waves of a workgroup share the tables and the list of blocks, and nothing else: wave w takes rows kRPW w .. of every
// block (a 64 x kRPW strip) with its own halo, its own depth tile and its own record table, at its own pace -- no barrier after
// the tables are in place.  (With one depth tile per block, two barriers per block made every wave wait for the block's
// slowest: 29 % of all wave time.)
// kSrgb: the targets are *Srgb formats (encode on store, decode on sample); otherwise plain unorm8.  kBgra: channel order.
struct ResolveArgs {             // k_resolve's parameter list as the argument segment lays it out
    FrameParams P;
    OutputParams O;
    CoverParams C;
};
// A wave-uniform constant-address-space object behind a pointer the compiler cannot prove to be the same from one call to the
// next: fields read through it are loaded (s_load, scalar cache) where they are used, instead of being loaded once and held in
// scalar registers (or their addresses precomputed) across every loop around the use.
template <typename T>
__device__ __forceinline__ const T& reload_ref(const_space_ptr<T> p) {
    asm volatile("" : "+s"(p));
    return *(const T*)(const void*)p;
}
__device__ __forceinline__ const ResolveArgs& resolve_args() {
    return reload_ref(kernarg<ResolveArgs>());
}

template <bool kSrgb, bool kBgra>
__global__ __launch_bounds__(256, TOPO_RESOLVE_WGS) void k_resolve(FrameParams P, OutputParams O, CoverParams C) {
    __shared__ float s_thresh[258];    // sRGB code boundaries; [255..257] = NaN: never <= anything (srgb_encode_lut probes up to 256)
    __shared__ float s_decode[256];
    __shared__ float s_ndec[256];      // normal channel decode 2c/255 - 1
    __shared__ uint32_t s_lut[1024];   // 4096 one-byte bins of srgb_encode_lut
    __shared__ float s_lin[4][kRPW + 2][66];                 // per wave: linear depth of the strip + halo
    // per wave: the records, record-major at a stride of 36 words (16-byte aligned): a record is written and read as nine 16-byte
    // LDS operations instead of the 34 / 17 four- and eight-byte ones of the round-2 layout (word-major)
    constexpr int kRecStride = (kTriRecordWords + 3) & ~3;
    __shared__ __attribute__((aligned(16))) uint32_t s_rec[4][kRecCap][kRecStride];
    static_assert(kRecStride == (int)kOwnedRecWords && kRPW == (int)kOwnedStripRows, "a record of CoverParams::recs is a strip's record as it lies here");
    __shared__ uint32_t s_uid[4][kRecCap];                   // per wave: the distinct winner ids of a group of rows
    __shared__ uint8_t s_slot[4][kRPW][64];                  // per wave and pixel: the number of its entry among the strip's table entries (0xFF: none)
    const uint32_t lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int32_t tx = (int32_t)lane;
    // Blocks are dealt out with a static stride: workgroup g takes blocks g, g + grid, g + 2 grid, ... -- a sample of every
    // part of every view, so each workgroup gets the same mix of sky, far field and near field.  (Handing out runs of
    // consecutive blocks dynamically measured 10 % to 3.5x slower: a run is all sky or all near field, and a block takes
    // ~10 us from first mark to last store, so whoever draws the last near-field run finishes long after everyone else.)
    const uint32_t n_blocks = P.rblock_count, stride = gridDim.x;               // blocks P.rblock_first .. of the submission's rblocks_view * n_views
    const uint32_t per_wg = (n_blocks - blockIdx.x + stride - 1) / stride;      // blocks blockIdx.x + j * stride, j < per_wg (the grid is <= n_blocks)
    // once per workgroup: the tables
    s_thresh[threadIdx.x] = threadIdx.x < 255 ? bits_f(TOPO_SRGB_THRESH_BITS[threadIdx.x]) : NAN;
    if (threadIdx.x < 2) s_thresh[256 + threadIdx.x] = NAN;
    s_decode[threadIdx.x] = bits_f(TOPO_SRGB_DECODE_BITS[threadIdx.x]);
    s_ndec[threadIdx.x] = normal_channel(threadIdx.x);
#pragma unroll
    for (int k = 0; k < 4; ++k) s_lut[threadIdx.x + 256 * k] = TOPO_SRGB_LUT12_WORDS[threadIdx.x + 256 * k];
    const uint8_t* lut = reinterpret_cast<const uint8_t*>(s_lut);
    // the frame's counters (queue fills, status bits) for whoever waits for the frame: final since the last raster kernel, stored to
    // the host's pinned ring from here (a copy operation behind the frame was a blit kernel of its own: ~10 us of every frame)
    if (P.status_out && blockIdx.x == 0 && threadIdx.x < kStatusWords) P.status_out[threadIdx.x] = P.counters[threadIdx.x];
    __syncthreads();                   // the only barrier
    float (*const lin_tile)[66] = s_lin[wave];
    uint8_t (*const slot_tile)[64] = s_slot[wave];
    const int32_t sy0 = kRPW * (int32_t)wave;      // the strip's first row within its block
    // lane constants: the pixel's column as a double (TriRecord kind 1), the lane's entry of the ring's side columns
    const double lane_d = (double)tx;
    const float two_over_w = div_f(2.0f, (float)P.W), two_over_h = div_f(2.0f, (float)P.H);
    const int32_t ring2_e = (int32_t)(lane < kRing2Lanes ? lane : kRing2Lanes - 1u);
    float* const ring2_at = &lin_tile[ring2_e >> 1][(ring2_e & 1) ? 65 : 0];

    for (uint32_t j0 = 0; j0 < per_wg; j0 += 64) {
        const uint32_t nj = per_wg - j0 < 64u ? per_wg - j0 : 64u;
        // ---- which of these blocks' strips hold anything: lane j looks at block j0 + j, all its marks in one trip to memory
        uint64_t mm, mc;       // strips with / without anything drawn
        {
            const FrameParams& P = resolve_args().P;
            const ResolveBlock Bl = resolve_block(P, P.rblock_first + blockIdx.x + (j0 + (lane < nj ? lane : 0u)) * stride);
            bool any = false;
#pragma unroll
            for (uint32_t t = 0; t < kStripMarks; ++t) any |= resolve_strip_marked(P, Bl, wave, t);      // (unconditional loads, none chained to another)
            const bool exists = lane < nj && Bl.by + sy0 < P.H;
            mm = __ballot(exists && any);
            mc = __ballot(exists && !any);
        }
        const uint32_t n_marked = (uint32_t)__popcll(mm), n_clear = (uint32_t)__popcll(mc);
        auto block_of = [&](const FrameParams& P, uint32_t j) { return resolve_block(P, P.rblock_first + blockIdx.x + (j0 + j) * stride); };      // (j comes out of a wave-uniform mask)
        // the untouched strips are pure stores: spread over the marked strips' iterations, so that their bandwidth hides
        // under the shading
        const uint32_t fills_per_iter = n_marked ? (n_clear + n_marked - 1) / n_marked : n_clear;
        // The keys of strip i + 1 are requested once strip i's keys have been consumed (depths into the LDS tile and the depth
        // output, ids into entry numbers): they travel under strip i's record pass and shading -- the bulk of a strip's time --
        // in the registers strip i's keys have just left.
        ResolveKeys K;
        uint32_t j_cur = 0;
        bool have = mm != 0ull;
        // every strip's keys are requested when the strip starts, none ahead (the round-2 form requested them a strip ahead: see below)
        if (have) j_cur = pop_bit(mm);
        while (have) {
            // the parameters again for every strip, from the argument segment: held from the kernel's start, ~50 of them filled
            // the scalar register file and were spilled and restored around every strip's row loop
            const FrameParams& P = resolve_args().P;
            const OutputParams& O = resolve_args().O;
            resolve_load_keys(P, block_of(P, j_cur), lane, wave, K);
            // Owned strips.  A strip of a region that one near-field giant has claimed (k_raster_cover) has a record in the frame's
            // table (CoverParams::recs): the owner's TriRecord at this strip's origin, its id, the frame's serial.  Lanes 0 .. 8 read
            // one 16-byte chunk of it each, under the keys' trip; if it carries this frame's serial and every pixel of the strip
            // inside the target has the owner's id, the strip has ONE winner and its record is at hand: no listing, no record pass.
            // (No table or serial 0: the path is off, at the price of this wave-uniform test.)
            const bool recs_on = resolve_args().C.recs != nullptr && resolve_args().C.serial != 0u;
            uint4 own = make_uint4(0u, 0u, 0u, 0u);
            if (recs_on) {
                const CoverParams& C = resolve_args().C;
                const ResolveBlock Bo = block_of(P, j_cur);
                const size_t at = owned_record_index(C.regions_x, C.regions_y, Bo.view, Bo.bx, Bo.by + sy0);
                if (TOPO_CHK(P.counters, at < (size_t)C.cap * kOwnedStrips, 38u, at))
                    own = reinterpret_cast<const uint4*>(C.recs + at * kOwnedRecWords)[lane < kOwnedRecWords / 4 ? lane : kOwnedRecWords / 4 - 1u];
            }
            // (this strip's share of the untouched strips -- pure stores -- goes out under the keys' trip to memory)
            for (uint32_t f = 0; f < fills_per_iter && mc; ++f) resolve_fill_sky<kBgra>(P, O, block_of(P, pop_bit(mc)), lane, wave);
            const ResolveBlock B = block_of(P, j_cur);
            const int32_t px = B.bx + tx, y0 = B.by + sy0;
            const bool in_x = px < P.W;        // lanes beyond the target's right edge stay: they compute triangle records
            const int32_t n_rows = P.H - y0 < kRPW ? P.H - y0 : kRPW;      // rows of the strip inside the target (>= 1)
            bool terrain = K.ring0 != 0x3F800000u || K.ring1 != 0x3F800000u || (lane < kRing2Lanes && K.ring2 != 0x3F800000u);
#define TOPO_X(r, m) terrain |= K.raw.m != 0x3F800000u;
            TOPO_ROWS(TOPO_X)
#undef TOPO_X
            const bool any_terrain = __ballot(terrain) != 0ull;
            uint64_t n_row = 0;            // byte r: table entries of row r (<= kRecCap + 1; one word instead of kRPW registers)
            uint32_t n_all = 0;            // table entries of the strip
            bool over = false;             // a row has more entries than the table holds
            if (any_terrain) {
                wave_lds_fence();              // (the previous strip's reads of the tiles are done)
#define TOPO_X(r, m) lin_tile[r + 1][tx + 1] = linear_depth(bits_f(K.raw.m));
                TOPO_ROWS(TOPO_X)
#undef TOPO_X
                lin_tile[0][tx + 1] = linear_depth(bits_f(K.ring0));
                lin_tile[kRPW + 1][tx + 1] = linear_depth(bits_f(K.ring1));
                {
                    const float l2 = linear_depth(bits_f(K.ring2));
                    if (lane < kRing2Lanes) *ring2_at = l2;
                }
                // the depth output is the key's depth word
                if (in_x && O.depth) {
                    uint8_t* dp = reinterpret_cast<uint8_t*>(O.depth) + (size_t)B.view * O.depth_view_stride + (size_t)y0 * O.depth_pitch + (size_t)px * 4;
#define TOPO_X(r, m) if (r < n_rows) { *reinterpret_cast<uint32_t*>(dp) = K.raw.m; dp += O.depth_pitch; }
                    TOPO_ROWS(TOPO_X)
#undef TOPO_X
                }
                bool owned = false;
                if (recs_on) {       // words 34 and 35 are in lane 8's chunk
                    const uint32_t o_id = (uint32_t)__builtin_amdgcn_readlane((int)own.z, (int)kOwnedRecWords / 4 - 1);
                    const uint32_t o_serial = (uint32_t)__builtin_amdgcn_readlane((int)own.w, (int)kOwnedRecWords / 4 - 1);
                    bool other = false;
#define TOPO_X(r, m) other |= r < n_rows && K.id.m != o_id;
                    TOPO_ROWS(TOPO_X)
#undef TOPO_X
                    owned = o_serial == resolve_args().C.serial && __ballot(in_x && other) == 0ull;
                }
                if (owned) {
                    // entry 0 for every pixel, the table's record 0 = the strip's record as it came; n_all stays 0, so the group loop
                    // below takes all rows as one group from the table and finds no record to compute (cnt = 0)
                    const uint8_t sl = in_x ? (uint8_t)0u : (uint8_t)0xFFu;
#define TOPO_X(r, m) slot_tile[r][tx] = sl;
                    TOPO_ROWS(TOPO_X)
#undef TOPO_X
                    if (lane < kOwnedRecWords / 4) *reinterpret_cast<uint4*>(&s_rec[wave][0][4 * lane]) = own;
                } else {
                // ---- the distinct winners of this wave's pixels: a lane opens an entry where its id differs from its left
                // neighbour's.  Entries are numbered over the strip's rows that are shaded from the table (rows with at most kRecCap
                // entries, while the numbers fit a byte); n_row = entries of a row.  A pixel's entry number waits in LDS.
#define TOPO_X(r, m)                                                                                                            \
    {                                                                                                                           \
        const bool valid = in_x && r < n_rows && K.id.m != kNoTri;                                                              \
        const uint32_t left = (uint32_t)__shfl_up((int)K.id.m, 1);                                                              \
        const bool leader = valid && (lane == 0 || K.id.m != left);                                                             \
        const uint64_t mask = __ballot(leader);                                                                                 \
        uint32_t n = (uint32_t)__popcll(mask);                                                                                  \
        if (n_all + n > 254u) n = kRecCap + 1u; /* (entry numbers are bytes: such a row is shaded in one step per pixel) */     \
        const uint32_t slot = n_all + (uint32_t)__popcll(mask & ((2ull << lane) - 1ull)) - 1u; /* valid lanes: the last leader at or before them */ \
        slot_tile[r][tx] = (uint8_t)(valid && n <= kRecCap ? slot : 0xFFu);                                                     \
        if (leader && n <= kRecCap && slot < kRecCap) s_uid[wave][slot] = K.id.m; /* the first group's ids (later groups: below) */ \
        n_all += n <= kRecCap ? n : 0u;                                                                                         \
        n_row |= (uint64_t)n << (8 * r);                                                                                        \
        over |= n > kRecCap;                                                                                                    \
    }
                TOPO_ROWS(TOPO_X)
#undef TOPO_X
                }
                wave_lds_fence();
            }
            // ---- this strip's keys are consumed: the next strip's turn
            const bool more = mm != 0ull;
            uint32_t j_next = 0;
            // (Rounds 2 and 3 requested the NEXT strip's keys here, to travel under the record pass and the rows.  But the wait counter
            // is in order: the record pass below waits for its own loads -- cache hits -- behind that request's trip to HBM, so what
            // the request hid of the trip at the next strip's start it cost here: with no request ahead at all the kernel took the
            // same 0.371 ms -- with 106 registers instead of 125, which is what lets a fifth workgroup onto the CU (0.362 ms).
            // Requesting BEHIND the record pass would hide the trip under the rows; every form of it tried -- the request inside the
            // group loop, the first record pass peeled in front of the loop, its loads and its arithmetic as two calls with the request
            // between them -- spilled 12 to 35 registers and lost.)
            if (more) j_next = pop_bit(mm);
            if (!any_terrain) {                // marked, but every key still cleared (a mark covers 64 keys): the cleared texel and depth 1
                resolve_fill_sky<kBgra>(P, O, B, lane, wave);
                have = more;
                j_cur = j_next;
                continue;
            }
            uint8_t* rgba_p = O.rgba + (size_t)B.view * O.rgba_view_stride + (size_t)y0 * O.rgba_pitch + (size_t)px * 4;
            // what fs_main reads of the view, once per strip and wave-uniform: left to the compiler these are re-loaded in every
            // row (it cannot prove the output stores do not alias them) behind an s_waitcnt vmcnt(0) that also waits for the
            // previous row's stores to land
            // (over the scalar data path -- constant address space --: as vector loads they were waited for with s_waitcnt vmcnt(0)
            // right behind the request for the next strip's keys, i.e. every strip began by sitting out that request's trip to HBM)
            const auto view_c = const_space(P.views + B.view);
            const f3 sun = {view_c->sun[0], view_c->sun[1], view_c->sun[2]};
            const float cam_x = view_c->cam_x, cam_y = view_c->cam_y;
            const int32_t view_mode = view_c->view_mode;
            const float gx = pixel_gx(px, two_over_w);
            // Rows are taken in groups of consecutive rows whose table entries fit the table (near field: all rows in one
            // group, a handful of records); a row with more entries than the table holds is a group of its own, shaded in
            // one step per pixel (resolve_varyings), as every row was in round 1.
            int32_t r0 = 0;
            uint32_t gbase = 0;            // table entries of the groups before this one
            const bool one_group = n_all <= kRecCap && !over;
#pragma unroll 1
            while (r0 < n_rows) {
                int32_t r1;
                uint32_t cnt;
                bool table = true;
                if (one_group) {
                    r1 = n_rows;
                    cnt = n_all;
                } else {
                    r1 = r0;
                    cnt = 0;
                    // (a loop, not unrolled over the rows: unrolled, the compiler decodes every row's count ahead of the group loop
                    // and holds the results in scalar registers across it)
#pragma unroll 1
                    for (int32_t r = r0; r < n_rows; ++r) {
                        const uint32_t n = (uint32_t)(n_row >> (8 * r)) & 0xFFu;
                        if (n > kRecCap || cnt + n > kRecCap) break;
                        cnt += n;
                        r1 = r + 1;
                    }
                    if (r1 == r0) {            // the row at r0 alone exceeds the table
                        table = false;
                        r1 = r0 + 1;
                    } else if (gbase != 0u) {
                        // a later group: its ids were not listed above (their entry numbers lie beyond the table): listed now -- a
                        // lane is the leader of its entry iff its left neighbour has another one; the id is read again
                        for (int32_t r = r0; r < r1; ++r) {
                            const uint32_t e = slot_tile[r][tx], el = (uint32_t)__shfl_up((int)e, 1);
                            if (e != 0xFFu && (lane == 0 || e != el) && TOPO_CHK(P.counters, e - gbase < kRecCap, 15u, e)) s_uid[wave][e - gbase] = resolve_reload_id(P, B, px, y0 + r);
                        }
                    }
                }
                if (table && cnt) {            // one triangle per lane: everything that depends on the triangle alone
                    wave_lds_fence();
                    if (lane < cnt) {
                        const FrameParams& P = resolve_args().P;
                        const ViewDev& view = reload_ref(view_c);
                        const uint32_t id = s_uid[wave][lane];
                        const uint32_t draw = id >> 1, fan = id & 1u;
                        const uint32_t rank = fastdiv(draw, P.div_tris), tri = draw - rank * P.tris_per_tile;
                        TriRecord rec;
                        if (TOPO_CHK(P.counters, rank < P.n_tiles, 13u, id)) resolve_setup<true>(P.tiles[rank], P.tile_w, P.div_hm1, P.tile_h - 1, view, P.W, P.H, tri, fan, s_ndec, B.bx, y0, rec);
                        else rec = TriRecord{};
                        int k = 0;
#define TOPO_X(f) s_rec[wave][lane][k++] = rec.f;
                        TOPO_TRIREC_WORDS(TOPO_X)
#undef TOPO_X
                    }
                    wave_lds_fence();
                }
                // One row of the group.  The two ways a row gets its varyings -- from the wave's record table, or in one step per pixel
                // with memory loads of its own (rows with more winners than the table holds: 0.5 % at c4) -- are two INSTANCES of
                // this body, each in a loop of its own: in one loop the compiler had to assume the memory loads of the second form
                // pending in the first as well, and every table row began by waiting for the previous row's output store to land
                // (s_waitcnt vmcnt(0)).
                auto shade_row = [&](auto table_tag, int32_t r) __attribute__((always_inline)) {
                    constexpr bool kTable = decltype(table_tag)::value;
                        const int32_t py = y0 + r;
                        // the pixel's entry number (rows shaded from the table) or its winner id
                        const uint32_t sel = kTable ? (uint32_t)slot_tile[r][tx] : (in_x ? resolve_reload_id(P, B, px, py) : kNoTri);
                        // the contour taps first: they depend on nothing, so their LDS trip overlaps the record's
                        float ln[8];
                        {
                            int k = 0;
    #pragma unroll
                            for (int i = -1; i <= 1; ++i)
    #pragma unroll
                                for (int j = -1; j <= 1; ++j) {
                                    if (i == 0 && j == 0) continue;
                                    ln[k++] = lin_tile[r + 1 + j][tx + 1 + i];
                                }
                        }
                        const float lin_c = lin_tile[r + 1][tx + 1];
                        // render target texel (Rgba8UnormSrgb): the cleared value or the shaded winner
                        uint32_t c8 = P.sky_c8;
                        if (sel != (kTable ? 0xFFu : kNoTri)) {
                            float lin[4] = {0.0f, 0.71f, 0.885f, 1.0f};
                            f3 wpos = {0.0f, 0.0f, 0.0f}, wnrm;
                            bool ok;
                            if (kTable) {
                                const uint32_t sl = sel - gbase;
                                TriRecord rec;
                                int k = 0;
    #define TOPO_X(f) rec.f = s_rec[wave][sl][k++];
                                TOPO_TRIREC_WORDS(TOPO_X)
    #undef TOPO_X
                                const PixelAt at = {px, py, lane_d, (double)r, gx, pixel_gy(py, two_over_h)};
                                ok = resolve_pixel(rec, at, wpos.x, wpos.y, wnrm);
                            } else {
                                const FrameParams& P = resolve_args().P;
                                const ViewDev& view = reload_ref(view_c);
                                const uint32_t draw = sel >> 1, fan = sel & 1u;
                                const uint32_t rank = fastdiv(draw, P.div_tris), tri = draw - rank * P.tris_per_tile;
                                ok = TOPO_CHK(P.counters, rank < P.n_tiles, 13u, sel) &&
                                     resolve_varyings<true>(P.tiles[rank], P.tile_w, P.div_hm1, P.tile_h - 1, view, P.W, P.H, tri, fan, s_ndec, px, py, wpos, wnrm);
                            }
                            if (ok) shade_fragment(view_mode, sun, cam_x, cam_y, (float)px + 0.5f, (float)py + 0.5f, wpos, wnrm, lin);
                            c8 = (kSrgb ? srgb_encode_lut3(s_thresh, lut, lin[0], lin[1], lin[2]) : to_unorm8(lin[0]) | (to_unorm8(lin[1]) << 8) | (to_unorm8(lin[2]) << 16)) |
                                 (to_unorm8(lin[3]) << 24);
                        }
                        // The post pass.  Its contour factor a is 0 iff RN(contour / centre) <= 0.05f; contour <= 0.0499f * centre
                        // (centre is a linear depth: 50 .. 5e5) puts the quotient below 0.04991: such a pixel returns its texel
                        // unchanged, and a row of them skips the divisions.  (A NaN fails the comparison and takes the long route.)
                        float contour = 8.0f * lin_c;
    #pragma unroll
                        for (int k = 0; k < 8; ++k) contour -= ln[k];
                        uint32_t out = c8;
                        const bool long_post = !P.post_off && __ballot(!(contour <= 0.0499f * lin_c)) != 0ull;      // (post_off: the render-target texel itself)
                        if (long_post) out = post_pixel_t<true>(s_thresh, s_decode, c8, lin_c, ln, lut, kSrgb);
                        if (in_x) *reinterpret_cast<uint32_t*>(rgba_p) = surface_order<kBgra>(out);
                };
                if (table) {
#pragma unroll 1
                    for (int32_t r = r0; r < r1; ++r, rgba_p += O.rgba_pitch) shade_row(std::true_type{}, r);
                } else {
#pragma unroll 1
                    for (int32_t r = r0; r < r1; ++r, rgba_p += O.rgba_pitch) shade_row(std::false_type{}, r);
                }
                gbase += table ? cnt : 0u;
                r0 = r1;
            }
            have = more;
            j_cur = j_next;
        }
        while (mc) {
            const FrameParams& P = resolve_args().P;
            resolve_fill_sky<kBgra>(P, resolve_args().O, block_of(P, pop_bit(mc)), lane, wave);
        }
    }
}

}  // namespace
}  // namespace topo
