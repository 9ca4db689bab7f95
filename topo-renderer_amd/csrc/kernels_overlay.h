// kernels_overlay.h -- what runs over a resolved frame: the pixelise form of the post pass, line and glyph overlays, peak labels.
//
//   k_post_pixelize                        the post pass with the pixelise branch on (behind a k_resolve with post_off)
//   k_overlay_raster, k_overlay_resolve    line overlays (line_shader.wgsl)
//   k_glyph_raster, k_glyph_resolve        text
//   k_overlay_init                         a fresh overlay key image
//   k_visible_peaks                        which peaks the depth image shows (the labels' visibility test)
#pragma once

#include "kernels_common.h"

namespace topo {
namespace {

// The post pass with the pixelise branch on (postprocessing_shader.wgsl:70-74; never in the reference, which pins pixelize_n to
// 100): the colour is a sample of the render target AWAY from the pixel's own texel, so the frame takes two passes -- k_resolve
// stores the render-target texels (post_off), this kernel samples them (sample_pixelized), takes the contour from the depth
// image and stores the surface texel.  One lane per pixel; nothing here is tuned.
__global__ __launch_bounds__(256) void k_post_pixelize(int32_t W, int32_t H, float vw, float vh, float n, const uint8_t* __restrict__ pre, OutputParams O,
                                                       const float* __restrict__ depth, size_t depth_view_stride, size_t depth_pitch, uint32_t linear_target,
                                                       uint32_t bgra) {
    __shared__ float s_thresh[256], s_decode[256];
    s_thresh[threadIdx.x] = bits_f(TOPO_SRGB_THRESH_BITS[threadIdx.x]);
    s_decode[threadIdx.x] = bits_f(TOPO_SRGB_DECODE_BITS[threadIdx.x]);
    __syncthreads();
    const int32_t px = blockIdx.x * 64 + (threadIdx.x & 63), py = blockIdx.y * 4 + (threadIdx.x >> 6);
    const uint32_t view = blockIdx.z;
    if (px >= W || py >= H) return;
    const uint8_t* img = pre + (size_t)view * W * H * 4;
    const uint8_t* dimg = reinterpret_cast<const uint8_t*>(depth) + (size_t)view * depth_view_stride;
    auto texel = [&](int32_t x, int32_t y, float out[4]) {
        const uint32_t c8 = *reinterpret_cast<const uint32_t*>(img + ((size_t)y * W + x) * 4);
        out[0] = linear_target ? from_unorm8(c8 & 255u) : s_decode[c8 & 255u];
        out[1] = linear_target ? from_unorm8((c8 >> 8) & 255u) : s_decode[(c8 >> 8) & 255u];
        out[2] = linear_target ? from_unorm8((c8 >> 16) & 255u) : s_decode[(c8 >> 16) & 255u];
        out[3] = from_unorm8(c8 >> 24);
    };
    float rc[4];
    sample_pixelized(px, py, vw, vh, n, W, H, texel, rc);
    auto lin_at = [&](int32_t x, int32_t y) {
        x = x < 0 ? 0 : (x > W - 1 ? W - 1 : x);
        y = y < 0 ? 0 : (y > H - 1 ? H - 1 : y);
        return linear_depth(*reinterpret_cast<const float*>(dimg + (size_t)y * depth_pitch + (size_t)x * 4));
    };
    float ln[8];
    int k = 0;
#pragma unroll
    for (int i = -1; i <= 1; ++i)
#pragma unroll
        for (int j = -1; j <= 1; ++j) {
            if (i == 0 && j == 0) continue;
            ln[k++] = lin_at(px + i, py + j);
        }
    uint32_t out = post_mix(s_thresh, rc, lin_at(px, py), ln, linear_target == 0u);
    if (bgra) out = (out & 0xFF00FF00u) | ((out >> 16) & 0xFFu) | ((out & 0xFFu) << 16);
    *reinterpret_cast<uint32_t*>(O.rgba + (size_t)view * O.rgba_view_stride + (size_t)py * O.rgba_pitch + (size_t)px * 4) = out;
}

// ---- overlay pass (line_shader.wgsl) ------------------------------------------------------------------
// Overlay geometry is a few hundred CPU-tessellated triangles: one lane per triangle walks its pixel box and raises the
// pixel's overlay key (depth bits << 32 | ~triangle index) with a 64-bit atomic MAX -- `Greater` plus "the earlier draw
// keeps an equal depth" -- over a key image that starts at the post quad's depth 1/4096; a second kernel colours the
// pixels whose key moved.
__global__ __launch_bounds__(64) void k_overlay_raster(const OverlayVertex* __restrict__ verts, const uint32_t* __restrict__ idx, uint32_t n_tris,
                                                       uint32_t n_verts, float width, int32_t W, int32_t H, uint64_t* __restrict__ keys) {
    const uint32_t t = blockIdx.x * 64 + threadIdx.x;
    if (t >= n_tris) return;
    const uint32_t i0 = idx[3 * t], i1 = idx[3 * t + 1], i2 = idx[3 * t + 2];
    if (i0 >= n_verts || i1 >= n_verts || i2 >= n_verts) return;      // (wgpu rejects such a draw; here the triangle is skipped)
    SVert s0, s1, s2;
    if (overlay_vertex(verts[i0], width, (float)W, (float)H, s0) != kVtxOk || overlay_vertex(verts[i1], width, (float)W, (float)H, s1) != kVtxOk ||
        overlay_vertex(verts[i2], width, (float)W, (float)H, s2) != kVtxOk)
        return;
    TriSetup ts;
    if (!triangle_setup(s0, s1, s2, W, H, ts)) return;
    for (int32_t py = ts.py0; py <= ts.py1; ++py)
        for (int32_t px = ts.px0; px <= ts.px1; ++px) {
            const int64_t cx = (int64_t)px * 256 + 128, cy = (int64_t)py * 256 + 128;
            int64_t F[3];
            bool in = true;
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                F[e] = ts.dy[e] * (cx - ts.ax[e]) - ts.dx[e] * (cy - ts.ay[e]);
                in = in && F[e] + ts.bias[e] >= 0;
            }
            if (!in) continue;
            const float z = fmaf((float)F[1] * ts.iA, ts.dz1, fmaf((float)F[2] * ts.iA, ts.dz2, ts.z0));
            if (!(z >= 0.0f && z <= 1.0f)) continue;      // clip volume 0 <= z <= w
            atomicMax(reinterpret_cast<unsigned long long*>(keys + (size_t)py * W + px), (unsigned long long)overlay_key(z, t));
        }
}

__global__ __launch_bounds__(256) void k_overlay_resolve(const OverlayVertex* __restrict__ verts, const uint32_t* __restrict__ idx, float width,
                                                         int32_t W, int32_t H, uint64_t* __restrict__ keys, uint8_t* __restrict__ rgba, size_t pitch,
                                                         uint32_t linear_target, uint32_t bgra) {
    const int32_t px = blockIdx.x * 64 + (threadIdx.x & 63), py = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (px >= W || py >= H) return;
    const uint64_t key = keys[(size_t)py * W + px];
    keys[(size_t)py * W + px] = kOverlayClear;      // ready for the next frame's overlay
    if (key <= kOverlayClear) return;                // nothing passed `Greater` here (an equal depth has a smaller low word)
    const uint32_t t = 0xFFFFFFFFu - (uint32_t)key;
    float rgb[3];
    if (!overlay_color(verts[idx[3 * t]], verts[idx[3 * t + 1]], verts[idx[3 * t + 2]], width, W, H, px, py, rgb)) return;
    uint32_t out;
    if (linear_target) {
        out = to_unorm8(rgb[0]) | (to_unorm8(rgb[1]) << 8) | (to_unorm8(rgb[2]) << 16);
    } else {
        float thresh[1];      // (the 8-probe search reads the table from constant memory: overlays are a few thousand pixels)
        (void)thresh;
        auto enc = [](float l) {
            uint32_t lo = 0;
#pragma unroll
            for (uint32_t step = 128; step >= 1; step >>= 1)
                if (bits_f(TOPO_SRGB_THRESH_BITS[lo + step - 1]) <= l) lo += step;
            return lo;
        };
        out = enc(rgb[0]) | (enc(rgb[1]) << 8) | (enc(rgb[2]) << 16);
    }
    out |= to_unorm8(1.0f) << 24;
    if (bgra) out = (out & 0xFF00FF00u) | ((out >> 16) & 0xFFu) | ((out & 0xFFu) << 16);
    *reinterpret_cast<uint32_t*>(rgba + (size_t)py * pitch + (size_t)px * 4) = out;
}

// Text: one 64-thread workgroup per glyph quad.  Pass 1 raises the key of every pixel the quad covers (the lines' key image:
// depth bits << 32 | ~glyph index, 64-bit atomic max = Greater + "the earlier draw keeps an equal depth"); pass 2 lets the
// glyph that owns a pixel blend into it and puts the key back to the post quad's depth.
__global__ __launch_bounds__(64) void k_glyph_raster(const GlyphInstance* __restrict__ glyphs, uint32_t n_glyphs, float depth, int32_t W, int32_t H,
                                                     uint64_t* __restrict__ keys) {
    const uint32_t g = blockIdx.x;
    if (g >= n_glyphs) return;
    const GlyphInstance gi = glyphs[g];
    const uint32_t gw = gi.dim[0], n = gw * gi.dim[1];
    const unsigned long long key = (unsigned long long)overlay_key(depth, g);
    for (uint32_t i = threadIdx.x; i < n; i += 64) {
        const int64_t px = (int64_t)gi.pos[0] + (int64_t)(i % gw), py = (int64_t)gi.pos[1] + (int64_t)(i / gw);
        if (px < 0 || py < 0 || px >= W || py >= H) continue;
        atomicMax(reinterpret_cast<unsigned long long*>(keys + (size_t)py * W + (size_t)px), key);
    }
}

__global__ __launch_bounds__(64) void k_glyph_resolve(const GlyphInstance* __restrict__ glyphs, uint32_t n_glyphs, float depth, const uint8_t* __restrict__ atlas,
                                                      uint32_t aw, uint32_t ah, int32_t W, int32_t H, uint64_t* __restrict__ keys, uint8_t* __restrict__ rgba,
                                                      size_t pitch, uint32_t linear_target, uint32_t bgra) {
    __shared__ float s_thresh[256], s_decode[256];
    for (uint32_t i = threadIdx.x; i < 256; i += 64) {
        s_thresh[i] = bits_f(TOPO_SRGB_THRESH_BITS[i]);
        s_decode[i] = bits_f(TOPO_SRGB_DECODE_BITS[i]);
    }
    __syncthreads();
    const uint32_t g = blockIdx.x;
    if (g >= n_glyphs) return;
    const GlyphInstance gi = glyphs[g];
    const uint32_t gw = gi.dim[0], n = gw * gi.dim[1];
    const uint64_t mine = overlay_key(depth, g);
    for (uint32_t i = threadIdx.x; i < n; i += 64) {
        const uint32_t dx = i % gw, dy = i / gw;
        const int64_t px = (int64_t)gi.pos[0] + dx, py = (int64_t)gi.pos[1] + dy;
        if (px < 0 || py < 0 || px >= W || py >= H) continue;
        uint64_t* k = keys + (size_t)py * W + (size_t)px;
        if (*k != mine) continue;                 // another glyph (an earlier one) owns the pixel, or the depth never passed
        *k = kOverlayClear;                        // ready for the next overlay call
        const uint32_t ax = gi.uv[0] + dx, ay = gi.uv[1] + dy;
        const uint32_t mask = ax < aw && ay < ah ? atlas[(size_t)ay * aw + ax] : 0u;      // (outside the atlas: transparent)
        uint32_t* out = reinterpret_cast<uint32_t*>(rgba + (size_t)py * pitch + (size_t)px * 4);
        *out = glyph_blend(gi, mask, *out, linear_target == 0u, bgra != 0u, s_thresh, s_decode);
    }
}

__global__ __launch_bounds__(256) void k_overlay_init(uint64_t* __restrict__ keys, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) keys[i] = kOverlayClear;
}

// One lane per peak: project, one depth lookup, one comparison (render_engine.rs:338-396).
__global__ __launch_bounds__(256) void k_visible_peaks(const float* __restrict__ proj, uint32_t w, uint32_t h,
                                                       const float* __restrict__ depth, size_t depth_pitch, uint32_t n,
                                                       const float* __restrict__ peaks, uint8_t* __restrict__ visible,
                                                       uint32_t* __restrict__ xy) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t x_pos = 0, y_pos = 0;
    float peak_dist = 0.0f;
    bool vis = false;
    if (project_peak(proj, peaks[3 * i], peaks[3 * i + 1], peaks[3 * i + 2], (float)w, (float)h, x_pos, y_pos, peak_dist) &&
        x_pos < w && y_pos < h) {       // the reference's buffer lookup would panic outside ("Failed depth buffer lookup")
        const float d = *reinterpret_cast<const float*>(reinterpret_cast<const uint8_t*>(depth) + (size_t)y_pos * depth_pitch + (size_t)x_pos * 4);
        vis = peak_dist - 10.0f < linear_depth(d);
    }
    visible[i] = vis ? 1 : 0;
    xy[2 * i] = vis ? x_pos : 0u;
    xy[2 * i + 1] = vis ? y_pos : 0u;
}

}  // namespace
}  // namespace topo
