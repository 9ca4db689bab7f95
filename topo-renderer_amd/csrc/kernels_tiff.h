// kernels_tiff.h -- kernels outside the frame and the load phase.
//
//   k_tiff_rows                   GeoTIFF decode, device half: predictor, byte order, placement (geotiff.hpp)
//   k_probe_sincos, k_probe_div   unit-test probes of the arithmetic spec's device forms
#pragma once

#include "kernels_common.h"

namespace topo {
namespace {

// ---- GeoTIFF rows: predictor, byte order, placement --------------------------------------------------------
// Inclusive prefix sum over `n` elements of a row held in global memory, in place, by one 256-thread workgroup: each
// thread sums a contiguous chunk, the 256 partial sums are scanned in LDS, each thread rewrites its chunk.
template <typename T, typename Load, typename Store>
__device__ void row_prefix_sum(uint32_t n, Load load, Store store) {
    __shared__ uint32_t part[256];
    const uint32_t per = (n + 255) / 256, lo = min(threadIdx.x * per, n), hi = min(lo + per, n);
    uint32_t sum = 0;
    for (uint32_t i = lo; i < hi; ++i) sum += load(i);
    part[threadIdx.x] = sum;
    __syncthreads();
    for (uint32_t off = 1; off < 256; off <<= 1) {
        const uint32_t a = threadIdx.x >= off ? part[threadIdx.x - off] : 0;
        __syncthreads();
        part[threadIdx.x] += a;
        __syncthreads();
    }
    uint32_t run = part[threadIdx.x] - sum;      // exclusive prefix of this chunk
    for (uint32_t i = lo; i < hi; ++i) {
        run += load(i);
        store(i, (T)run);
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void k_tiff_rows(uint8_t* __restrict__ bytes, const TiffSegDev* __restrict__ segs,
                                                   const uint32_t* __restrict__ row_seg, float* __restrict__ out, uint32_t W, uint32_t H,
                                                   uint32_t predictor, int big_endian) {
    const TiffSegDev sg = segs[row_seg[blockIdx.x]];
    const uint32_t r = blockIdx.x - sg.row0, y = sg.y0 + r;
    uint8_t* row = bytes + sg.byte_off + (size_t)r * sg.w * 4;
    auto word = [&](uint32_t i) {           // sample i of the row in the file's byte order -> native
        const uint8_t* p = row + 4 * (size_t)i;
        return big_endian ? ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]
                          : ((uint32_t)p[3] << 24) | ((uint32_t)p[2] << 16) | ((uint32_t)p[1] << 8) | p[0];
    };
    if (predictor == 3) {
        // floating-point predictor: the row is stored as four byte planes, most significant first, the whole 4w-byte
        // sequence differenced byte-wise (Adobe Photoshop TIFF Technical Note 3)
        row_prefix_sum<uint8_t>(sg.w * 4, [&](uint32_t i) { return (uint32_t)row[i]; }, [&](uint32_t i, uint8_t v) { row[i] = v; });
        for (uint32_t i = threadIdx.x; i < sg.w; i += 256) {
            const uint32_t x = sg.x0 + i;
            if (x < W && y < H)
                out[(size_t)y * W + x] = __uint_as_float(((uint32_t)row[i] << 24) | ((uint32_t)row[sg.w + i] << 16) |
                                                         ((uint32_t)row[2 * sg.w + i] << 8) | row[3 * sg.w + i]);
        }
        return;
    }
    if (predictor == 2) {                   // horizontal differencing of the 32-bit words
        uint32_t* wrow = reinterpret_cast<uint32_t*>(row);      // segments start 4-byte aligned in the staging buffer
        for (uint32_t i = threadIdx.x; i < sg.w; i += 256) wrow[i] = word(i);
        __syncthreads();
        row_prefix_sum<uint32_t>(sg.w, [&](uint32_t i) { return wrow[i]; }, [&](uint32_t i, uint32_t v) { wrow[i] = v; });
        for (uint32_t i = threadIdx.x; i < sg.w; i += 256) {
            const uint32_t x = sg.x0 + i;
            if (x < W && y < H) out[(size_t)y * W + x] = __uint_as_float(wrow[i]);
        }
        return;
    }
    for (uint32_t i = threadIdx.x; i < sg.w; i += 256) {
        const uint32_t x = sg.x0 + i;
        if (x < W && y < H) out[(size_t)y * W + x] = __uint_as_float(word(i));
    }
}

__global__ void k_probe_sincos(const float* x, float* s, float* c, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) sincos_f(x[i], s[i], c[i]);
}

__global__ void k_probe_div(int kind, const float* x, const float* y, float* out, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = kind == 0   ? div_f(x[i], y[i])
             : kind == 1 ? div_const(x[i], 255.0f, 1.0f / 255.0f)
             : kind == 2 ? div_const(x[i], 0.15f - 0.05f, 1.0f / (0.15f - 0.05f))
             : kind == 4 ? __builtin_amdgcn_fractf(x[i])      // v_fract_f32, the instruction itself
             : kind == 5 ? fract_f(x[i])                       // the spec's fract as the kernels evaluate it
                         : sqrt_f(x[i]);
    if (kind >= 6 && kind <= 8) {      // fs_main's dither (mode 0) of channel kind - 6 at p = (x, y), shading 0.25: the wave-level choice of the fraction's form
        float c[4];
        shade_fragment(0, f3{0.0f, 0.0f, 0.25f / 0.7f}, 0.0f, 0.0f, x[i], y[i], f3{0.0f, 0.0f, 0.0f}, f3{0.0f, 0.0f, 1.0f}, c);
        out[i] = c[kind - 6];
    }
}

}  // namespace
}  // namespace topo
