// unwrap_emul.cpp -- TEST-ONLY g++ build of the product's unwrap arithmetic (topo-renderer_amd/csrc/topo_unwrap.h): the functions
// k_unwrap calls for every pixel, run here over a whole output image on the CPU (tests/unwrap_emul.py, tests/test_unwrap_cpu.py), over
// the tables the library's own host code builds (host_math.cpp, compiled alongside).  The glue around them -- who takes which pixels,
// loads, stores -- is the kernel's.
#include <vector>

#include "../topo-renderer_amd/csrc/host_math.hpp"
#include "../topo-renderer_amd/csrc/topo_unwrap.h"

using namespace topo;

// uniforms: n_views x 40 floats.  rgba_src [n_views][src_h][src_w][4] / depth_src [n_views][src_h][src_w], densely packed, each
// nullable with its output.  Outputs out_h x out_w, densely packed; pxy (nullable): (view's px, py) per pixel, NaN without a source.
// Returns 0, or -1 for arguments the library would refuse.
extern "C" int emul_unwrap(const topo_unwrap_params* p, uint32_t n_views, const float* uniforms, uint32_t src_w, uint32_t src_h, const uint8_t* rgba_src,
                           const float* depth_src, int srgb, uint8_t* rgba_out, float* depth_out, int32_t* src_out, double* pxy) {
    const topo_uniforms* views = reinterpret_cast<const topo_uniforms*>(uniforms);
    if (unwrap_params_error(p) || unwrap_views_error(n_views, views, src_w, src_h)) return -1;
    std::vector<double> tab;
    unwrap_tables(p, n_views, views, tab);
    float thresh[256], decode[256];
    for (int i = 0; i < 256; ++i) {
        thresh[i] = bits_f(TOPO_SRGB_THRESH_BITS[i]);
        decode[i] = bits_f(TOPO_SRGB_DECODE_BITS[i]);
    }
    const double* const vt = tab.data() + kUnwrapViewsAt;
    const double* const cols = tab.data() + unwrap_cols_at(n_views);
    const double* const rows = tab.data() + unwrap_rows_at(n_views, p->out_w);
    const uint32_t* const texels = reinterpret_cast<const uint32_t*>(rgba_src);
    for (uint32_t r = 0; r < p->out_h; ++r)
        for (uint32_t c = 0; c < p->out_w; ++c) {
            const size_t at = (size_t)r * p->out_w + c;
            double d[3];
            unwrap_dir(rows[2 * (size_t)r], rows[2 * (size_t)r + 1], cols + 3 * (size_t)c, tab.data(), d);
            const UnwrapSource s = unwrap_locate(vt, n_views, src_w, src_h, d);
            uint32_t rgba = 0, depth = kUnwrapNoDepthBits;
            int32_t smap = -1;
            double px = NAN, py = NAN;
            if (s.view >= 0) {
                const uint32_t sx = (uint32_t)floor(s.px), sy = (uint32_t)floor(s.py);
                if (sx >= src_w || sy >= src_h) return -2;
                const size_t view0 = (size_t)s.view * src_h * src_w;
                smap = unwrap_source_index((uint32_t)s.view, sx, sy, src_w, src_h);
                px = s.px;
                py = s.py;
                if (depth_src) depth = f_bits(depth_src[view0 + (size_t)sy * src_w + sx]);
                if (texels && p->filter == TOPO_UNWRAP_BILINEAR) {
                    const UnwrapTaps t = unwrap_taps(s.px, s.py, src_w, src_h);
                    if (t.x[0] >= src_w || t.x[1] >= src_w || t.y[0] >= src_h || t.y[1] >= src_h) return -3;
                    const uint32_t* const r0 = texels + view0 + (size_t)t.y[0] * src_w, * const r1 = texels + view0 + (size_t)t.y[1] * src_w;
                    rgba = unwrap_blend(r0[t.x[0]], r0[t.x[1]], r1[t.x[0]], r1[t.x[1]], t.fx, t.fy, srgb != 0, thresh, decode);
                } else if (texels) {
                    rgba = texels[view0 + (size_t)sy * src_w + sx];
                }
            }
            if (rgba_out) memcpy(rgba_out + 4 * at, &rgba, 4);
            if (depth_out) memcpy(depth_out + at, &depth, 4);
            if (src_out) src_out[at] = smap;
            if (pxy) { pxy[2 * at] = px; pxy[2 * at + 1] = py; }
        }
    return 0;
}
