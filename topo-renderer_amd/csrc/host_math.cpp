// host_math.cpp -- the reference's CPU-side math behind the C ABI, free of HIP (see host_math.hpp).
#include "host_math.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "topo_labels.h"
#include "topo_math.h"
#include "topo_unwrap.h"

namespace topo {

// =========================================================================================================
// Host-side CPU math of the reference (glam 0.31.0, Cargo.lock:1272-1273), restated in f32.
// =========================================================================================================
namespace {

inline float rs_to_radians(float d) { return d * 0.017453292519943295f; }   // f32::to_radians

struct V3 { float x, y, z; };
inline float vdot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
inline V3 vcross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
inline V3 vnormalize(V3 v) {   // Vec3::normalize: self * length_recip()
    const float r = 1.0f / sqrtf(vdot(v, v));
    return {v.x * r, v.y * r, v.z * r};
}

// Mat3::from_euler(EulerRot::XYZEx, 0, b, c) = Rz(c) * Ry(b); with a = 0 every entry is one product.
void euler_xyz_ex_a0(float b, float c, float m[9] /*column-major*/) {
    const float si = sinf(0.0f), ci = cosf(0.0f);
    const float sj = sinf(b), cj = cosf(b), sh = sinf(c), ch = cosf(c);
    const float cc = ci * ch, cs = ci * sh, sc = si * ch, ss = si * sh;
    m[0] = cj * ch;       m[1] = cj * sh;       m[2] = -sj;
    m[3] = sj * sc - cs;  m[4] = sj * ss + cc;  m[5] = cj * si;
    m[6] = sj * cc + ss;  m[7] = sj * cs - sc;  m[8] = cj * ci;
}

}  // namespace

// TerrainUniforms::new's normal_to_world_rot (render/data.rs:125-133)
void terrain_rotation(float model_lon_deg, float model_lat_deg, float rot[9]) {
    euler_xyz_ex_a0(rs_to_radians(90.0f - model_lat_deg), rs_to_radians(model_lon_deg), rot);
}

// geometry::transform (render/geometry.rs:12-20)
void geometry_transform(float h, float lon_deg, float lat_deg, float out[3]) {
    const float r = kR0 + h;
    const float lon = rs_to_radians(lon_deg), lat = rs_to_radians(lat_deg);
    out[0] = r * cosf(lat) * cosf(lon);
    out[1] = r * cosf(lat) * sinf(lon);
    out[2] = r * sinf(lat);
}

// The local frame at an eye (geometry_transform's axes: x to (0 N, 0 E), z to the north pole): up = the eye's geocentric radius,
// east = z x up normalised (at a pole: +y), north = up x east.  What topo_pixel_angles and the unwrap tables measure azimuth and
// elevation in.
void local_frame(const float eye[3], double east[3], double north[3], double up[3]) {
    const double ex = eye[0], ey = eye[1], ez = eye[2];
    const double el = std::sqrt(ex * ex + ey * ey + ez * ez);
    up[0] = ex / el; up[1] = ey / el; up[2] = ez / el;
    const double eh = std::hypot(up[0], up[1]);
    east[0] = eh > 0.0 ? -up[1] / eh : 0.0;
    east[1] = eh > 0.0 ? up[0] / eh : 1.0;
    east[2] = 0.0;
    north[0] = up[1] * east[2] - up[2] * east[1];
    north[1] = up[2] * east[0] - up[0] * east[2];
    north[2] = up[0] * east[1] - up[1] * east[0];
}

// topo_sun_direction: local_frame's axes at (lon, lat) -- up = (cos lat cos lon, cos lat sin lon, sin lat), east = (-sin lon, cos lon, 0),
// north = up x east -- and the direction cos el (sin az east + cos az north) + sin el up.
void sun_direction(double lon_deg, double lat_deg, double az_deg, double el_deg, double out[3]) {
    const double kRad = 3.14159265358979323846 / 180.0;
    const double lo = lon_deg * kRad, la = lat_deg * kRad, az = az_deg * kRad, el = el_deg * kRad;
    const double up[3] = {std::cos(la) * std::cos(lo), std::cos(la) * std::sin(lo), std::sin(la)};
    const double east[3] = {-std::sin(lo), std::cos(lo), 0.0};
    const double north[3] = {up[1] * east[2] - up[2] * east[1], up[2] * east[0] - up[0] * east[2], up[0] * east[1] - up[1] * east[0]};
    const double ce = std::cos(el), se = std::sin(el), ca = std::cos(az), sa = std::sin(az);
    for (int k = 0; k < 3; ++k) out[k] = ce * (sa * east[k] + ca * north[k]) + se * up[k];
}

// topo_pixel_angles, in f64: the ray through pixel-space point (x, y) is the line between the points the inverse of camera_proj maps
// it to on the near (NDC z 0) and the far (z 1) plane -- no f32 eye enters the direction -- seen in the local east / north / up
// frame at the eye (up = the eye's geocentric radius; geometry_transform's axes: x to (0 N, 0 E), z to the north pole).
void pixel_angles(const topo_uniforms* view, uint32_t w, uint32_t h, uint32_t n, const float* xy, double* az_el) {
    const float* f = view->camera_proj;      // column-major: element (row r, column c) at f[4 c + r]
    double m[4][4], inv[4][8];
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) m[r][c] = f[4 * c + r];
    for (int r = 0; r < 4; ++r)      // Gauss-Jordan with partial pivoting on [m | I]
        for (int c = 0; c < 8; ++c) inv[r][c] = c < 4 ? m[r][c] : (c - 4 == r ? 1.0 : 0.0);
    for (int c = 0; c < 4; ++c) {
        int piv = c;
        for (int r = c + 1; r < 4; ++r)
            if (std::fabs(inv[r][c]) > std::fabs(inv[piv][c])) piv = r;
        for (int k = 0; k < 8; ++k) std::swap(inv[c][k], inv[piv][k]);
        const double d = inv[c][c];
        for (int k = 0; k < 8; ++k) inv[c][k] /= d;
        for (int r = 0; r < 4; ++r)
            if (r != c) {
                const double s = inv[r][c];
                for (int k = 0; k < 8; ++k) inv[r][k] -= s * inv[c][k];
            }
    }
    auto unproject = [&](double nx, double ny, double nz, double out[3]) {
        double p[4];
        for (int r = 0; r < 4; ++r) p[r] = inv[r][4] * nx + inv[r][5] * ny + inv[r][6] * nz + inv[r][7];
        for (int k = 0; k < 3; ++k) out[k] = p[k] / p[3];
    };
    double east[3], north[3], up[3];
    local_frame(view->camera_pos, east, north, up);
    const double kDeg = 180.0 / 3.14159265358979323846;
    for (uint32_t i = 0; i < n; ++i) {
        const double nx = 2.0 * xy[2 * i] / w - 1.0, ny = 1.0 - 2.0 * xy[2 * i + 1] / h;
        double p0[3], p1[3];
        unproject(nx, ny, 0.0, p0);
        unproject(nx, ny, 1.0, p1);
        const double d[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
        const double de = d[0] * east[0] + d[1] * east[1] + d[2] * east[2];
        const double dn = d[0] * north[0] + d[1] * north[1] + d[2] * north[2];
        const double du = d[0] * up[0] + d[1] * up[1] + d[2] * up[2];
        double az = std::atan2(de, dn) * kDeg;
        if (az < 0.0) az += 360.0;
        az_el[2 * i] = az;
        az_el[2 * i + 1] = std::atan2(du, std::hypot(de, dn)) * kDeg;
    }
}

// ---- unwrap (topo_unwrap_*): parameter checks, the f64 tables of k_unwrap (topo_unwrap.h), the inverse mapping ----------------------
const char* unwrap_params_error(const topo_unwrap_params* p) {
    if (!p) return "null parameters";
    if (p->projection > TOPO_UNWRAP_CYLINDRICAL || p->filter > TOPO_UNWRAP_BILINEAR) return "unknown projection or filter";
    if (p->out_w == 0 || p->out_h == 0) return "output size must be non-zero";
    if (!(p->az_span_deg > 0.0 && p->az_span_deg <= 360.0) || !std::isfinite(p->az0_deg)) return "az_span_deg must be in (0, 360] and az0_deg finite";
    if (!(p->el_bottom_deg > -90.0 && p->el_bottom_deg < p->el_top_deg && p->el_top_deg < 90.0)) return "elevations must satisfy -90 < bottom < top < 90";
    return nullptr;
}

const char* unwrap_views_error(uint32_t n_views, const topo_uniforms* views, uint32_t src_w, uint32_t src_h) {
    if (!views || n_views == 0 || n_views > kUnwrapMaxViews) return "1 .. 64 views";
    if (src_w == 0 || src_h == 0) return "source size must be non-zero";
    for (uint32_t k = 1; k < n_views; ++k)
        if (memcmp(views[k].camera_pos, views[0].camera_pos, 3 * sizeof(float)) != 0) return "the views must share one eye (camera_pos bitwise equal)";
    return nullptr;
}

void unwrap_tables(const topo_unwrap_params* p, uint32_t n_views, const topo_uniforms* views, std::vector<double>& out) {
    out.assign(unwrap_table_doubles(n_views, p->out_w, p->out_h), 0.0);
    double east[3], north[3], up[3];
    local_frame(views[0].camera_pos, east, north, up);
    for (int k = 0; k < 3; ++k) out[k] = up[k];
    static const int kRows[3] = {0, 1, 3};
    for (uint32_t v = 0; v < n_views; ++v)
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) out[kUnwrapViewsAt + (size_t)kUnwrapViewDoubles * v + 3 * r + c] = (double)views[v].camera_proj[4 * c + kRows[r]];
    double* cols = out.data() + unwrap_cols_at(n_views);
    for (uint32_t c = 0; c < p->out_w; ++c) unwrap_column(p->az0_deg, p->az_span_deg, p->out_w, c, east, north, cols + 3 * (size_t)c);
    double* rows = out.data() + unwrap_rows_at(n_views, p->out_w);
    for (uint32_t r = 0; r < p->out_h; ++r)
        unwrap_row_entry(p->projection == TOPO_UNWRAP_CYLINDRICAL, p->el_top_deg, p->el_bottom_deg, p->out_h, r, rows[2 * (size_t)r], rows[2 * (size_t)r + 1]);
}

// The inverse of the tables' mapping: column c's centre has x = c + 0.5, row r's centre y = r + 0.5.
void unwrap_xy(const topo_unwrap_params* p, uint32_t n, const double* az_el, double* xy) {
    const bool cyl = p->projection == TOPO_UNWRAP_CYLINDRICAL;
    const double tt = std::tan(p->el_top_deg * kUnwrapRad), tb = std::tan(p->el_bottom_deg * kUnwrapRad);
    for (uint32_t i = 0; i < n; ++i) {
        double a = std::fmod(az_el[2 * i] - p->az0_deg, 360.0);
        if (a < 0.0) a += 360.0;
        const double el = az_el[2 * i + 1];
        xy[2 * i] = a / p->az_span_deg * (double)p->out_w;
        xy[2 * i + 1] = (cyl ? (tt - std::tan(el * kUnwrapRad)) / (tt - tb) : (p->el_top_deg - el) / (p->el_top_deg - p->el_bottom_deg)) * (double)p->out_h;
    }
}

// ---- peak labels: the layout rule on the host (topo_labels.h) ----------------------------------------------------------------------

static_assert(sizeof(LabelRec) == sizeof(topo_label) && sizeof(topo_label) == 32 && sizeof(topo_label_params) == 16, "label layouts");

const char* label_grid_error(uint64_t image_width, uint32_t max_rows, int* code) {
    *code = TOPO_ERR_INVALID;
    if (image_width == 0) return "an image without columns";
    if (max_rows == 0) return "max_rows must not be 0";
    *code = TOPO_ERR_UNSUPPORTED;
    if (max_rows > kLabelMaxRows) return "at most 64 label rows";
    if (image_width * max_rows > kLabelMaxGridBits) return "image columns x max_rows must not exceed 524288 (64 KiB of occupancy bits)";
    return nullptr;
}

int label_layout(uint32_t n, const uint32_t* x, const float* widths, uint32_t image_width, float row_height, uint32_t max_rows, int32_t* row_out, topo_label* out) {
    int code;
    if (label_grid_error(image_width, max_rows, &code)) return code;
    if (n && (!x || !widths || !row_out)) return TOPO_ERR_INVALID;
    for (uint32_t j = 0; j < n; ++j)
        if (x[j] >= image_width) return TOPO_ERR_INVALID;
    std::vector<uint32_t> grid(label_grid_words(image_width, max_rows), 0u);
    uint32_t count = 0;
    for (uint32_t j = 0; j < n; ++j) {
        const float w = widths[j];
        if (!label_width_usable(w)) {
            row_out[j] = -2;
            continue;
        }
        const int32_t k = label_place(grid.data(), image_width, max_rows, x[j], label_right(x[j], w, image_width));
        row_out[j] = k;
        if (k < 0) continue;
        if (out) {
            const LabelRec rec{j, 0u, (uint32_t)k, (float)x[j], label_y(row_height, (uint32_t)k), w, (float)x[j], 0.0f};
            memcpy(&out[count], &rec, sizeof rec);
        }
        ++count;
    }
    return (int)count;
}

// Uniforms::new (render/data.rs:44-58) over Camera::{up,direction,get_view,build_view_proj_matrix}
// (data/camera.rs:97-128) and LightAngle::to_vec3 (:44-53).
void camera_uniforms(const float eye_in[3], float yaw, float pitch, float fov_y, float width, float height,
                     float sun_theta_deg, float sun_phi_deg, int32_t view_mode, topo_uniforms* out) {
    memset(out, 0, sizeof *out);
    const V3 eye = {eye_in[0], eye_in[1], eye_in[2]};
    const V3 up = vnormalize(eye);
    // Quat::from_rotation_arc(-Y, up)
    const V3 from = {0.0f, -1.0f, 0.0f};
    float qx, qy, qz, qw;
    const float d = vdot(from, up);
    const float one_minus_eps = 1.0f - 2.0f * 1.1920929e-7f;
    if (d > one_minus_eps) {
        qx = qy = qz = 0.0f; qw = 1.0f;
    } else if (d < -one_minus_eps) {   // any_orthonormal_vector(from), half-turn
        const float sign = copysignf(1.0f, from.z);
        const float a = -1.0f / (sign + from.z);
        const float b = from.x * from.y * a;
        const V3 axis = {b, sign + from.y * from.y * a, -from.y};
        const float s = sinf(3.14159265358979323846f * 0.5f), c = cosf(3.14159265358979323846f * 0.5f);
        qx = axis.x * s; qy = axis.y * s; qz = axis.z * s; qw = c;
    } else {
        const V3 c = vcross(from, up);
        const float w = 1.0f + d;
        const float l2 = (c.x * c.x + c.z * c.z) + (c.y * c.y + w * w);   // SSE2 dot4 order
        const float r = 1.0f / sqrtf(l2);
        qx = c.x * r; qy = c.y * r; qz = c.z * r; qw = w * r;
    }
    // direction = rot * (cos yaw cos pitch, sin pitch, sin yaw cos pitch)   (Quat * Vec3)
    const V3 v = {cosf(yaw) * cosf(pitch), sinf(pitch), sinf(yaw) * cosf(pitch)};
    const V3 b = {qx, qy, qz};
    const float b2 = vdot(b, b);
    const float k0 = qw * qw - b2, k1 = vdot(v, b) * 2.0f, k2 = qw * 2.0f;
    const V3 bxv = vcross(b, v);
    const V3 f = {(v.x * k0 + b.x * k1) + bxv.x * k2, (v.y * k0 + b.y * k1) + bxv.y * k2, (v.z * k0 + b.z * k1) + bxv.z * k2};
    // Mat4::look_to_rh(eye, f, up)
    const V3 s = vnormalize(vcross(f, up));
    const V3 u = vcross(s, f);
    const float view[16] = {s.x, u.x, -f.x, 0.0f, s.y, u.y, -f.y, 0.0f, s.z, u.z, -f.z, 0.0f,
                            -vdot(eye, s), -vdot(eye, u), vdot(eye, f), 1.0f};
    // Mat4::perspective_rh(fov_y, aspect, NEAR, FAR)
    const float aspect = width / height;
    const float sf = sinf(0.5f * fov_y), cf = cosf(0.5f * fov_y);
    const float hh = cf / sf, ww = hh / aspect, r = kFar / (kNear - kFar);
    const float proj[16] = {ww, 0, 0, 0, 0, hh, 0, 0, 0, 0, r, -1.0f, 0, 0, r * kNear, 0};
    for (int c = 0; c < 4; ++c)        // proj * view, column by column: ((c0*x + c1*y) + c2*z) + c3*w
        for (int rr = 0; rr < 4; ++rr) {
            float t = proj[rr] * view[c * 4 + 0];
            t = t + proj[4 + rr] * view[c * 4 + 1];
            t = t + proj[8 + rr] * view[c * 4 + 2];
            t = t + proj[12 + rr] * view[c * 4 + 3];
            out->camera_proj[c * 4 + rr] = t;
        }
    // normal_proj = view.inverse().transpose(): no shader reads it (render_shader.wgsl:5); filled with the
    // rotation block of the view, which is what it equals for a rigid transform up to rounding.
    for (int c = 0; c < 3; ++c)
        for (int rr = 0; rr < 3; ++rr) out->normal_proj[c * 4 + rr] = view[c * 4 + rr];
    out->normal_proj[15] = 1.0f;
    out->camera_pos[0] = eye.x; out->camera_pos[1] = eye.y; out->camera_pos[2] = eye.z; out->camera_pos[3] = 0.0f;
    float m3[9];
    euler_xyz_ex_a0(rs_to_radians(90.0f - sun_phi_deg), rs_to_radians(sun_theta_deg), m3);
    out->sun_direction[0] = m3[6]; out->sun_direction[1] = m3[7]; out->sun_direction[2] = m3[8];   // * Vec3::Z
    out->view_mode = view_mode;
}

// The cameras of a 360-degree strip of n_sectors perspective sectors: sector k looks at yaw0 - k * 360/n
// degrees with the vertical field of view that makes every sector 360/n degrees wide.
void panorama_uniforms(const float eye[3], float yaw0, float pitch, uint32_t sector_w, uint32_t sector_h, float sun_theta_deg, float sun_phi_deg,
                       int32_t view_mode, uint32_t n_sectors, topo_uniforms* out) {
    const double kPi = 3.14159265358979323846;
    const double fov = 2.0 * atan(tan(kPi / (double)n_sectors) * (double)sector_h / (double)sector_w);
    for (uint32_t k = 0; k < n_sectors; ++k)
        camera_uniforms(eye, (float)((double)yaw0 - (double)k * (2.0 * kPi / (double)n_sectors)), pitch, (float)fov, (float)sector_w,
                        (float)sector_h, sun_theta_deg, sun_phi_deg, view_mode, out + k);
}

// UiController::get_locations_range (control/ui_controller.rs:61-83), f32 as in the reference.
uint32_t locations_range(float latitude, float longitude, float range_dist, int32_t* out, uint32_t cap) {
    // center.0 = (floor(lat) as i32).min(-90).max(89): always 89, as written
    int c_lat = (int)floorf(latitude);
    c_lat = c_lat < -90 ? c_lat : -90;
    c_lat = c_lat > 89 ? c_lat : 89;
    const int c_lon = ((int)(floorf(longitude) + 540.0f)) % 360 - 180;
    const float lat_cos = cosf(rs_to_radians(latitude));
    const float arc_factor = 0.5f * range_dist / kR0;
    const float arc_factor_sin = sinf(arc_factor);
    const float afs_sq = arc_factor_sin * arc_factor_sin;
    const float R2D = 57.29577951308232f;                       // f32::to_degrees: self * (180 / PI)
    const float dlon = acosf(1.0f - afs_sq / lat_cos / lat_cos) * R2D;
    const float dlat = acosf(1.0f - afs_sq) * R2D;
    int lat_start = (int)floorf(latitude - dlat);
    lat_start = lat_start > -90 ? lat_start : -90;
    int lat_end = (int)floorf(latitude + dlat);
    lat_end = lat_end < 89 ? lat_end : 89;
    const int lon_start = (int)floorf(longitude - dlon), lon_end = (int)floorf(longitude + dlon);
    struct Item { int lat, lon, k0, k1; };
    std::vector<Item> v;
    for (int la = lat_start; la <= lat_end; ++la)
        for (int lo = lon_start; lo <= lon_end; ++lo) v.push_back({la, lo, std::abs(la - c_lat), std::abs(lo - c_lon)});
    std::stable_sort(v.begin(), v.end(), [](const Item& a, const Item& b) { return a.k0 != b.k0 ? a.k0 < b.k0 : a.k1 < b.k1; });
    uint32_t n = 0;
    for (const Item& it : v) {
        if (n < cap && out) { out[2 * n] = it.lat; out[2 * n + 1] = (it.lon + 540) % 360 - 180; }
        ++n;
    }
    return n;
}

// UiController::change_location (control/ui_controller.rs:23-59) as a plan: the tiles of get_locations_range(location,
// range) that are not loaded yet are to be requested, the loaded ones outside it are to be unloaded.  The reference walks
// HashSets (order unspecified); here both lists come out in a defined order: `request` in get_locations_range's sorted
// order, `unload` in the order of `loaded`.
void change_location_plan(float latitude, float longitude, float range_dist, const int32_t* loaded, uint32_t n_loaded,
                          std::vector<std::pair<int32_t, int32_t>>& unload, std::vector<std::pair<int32_t, int32_t>>& request) {
    const uint32_t n = locations_range(latitude, longitude, range_dist, nullptr, 0);
    std::vector<int32_t> want(2 * (size_t)n);
    locations_range(latitude, longitude, range_dist, want.data(), n);
    std::vector<bool> have(n, false);
    unload.clear();
    request.clear();
    for (uint32_t i = 0; i < n_loaded; ++i) {
        bool in_new = false;
        for (uint32_t k = 0; k < n; ++k)
            if (want[2 * k] == loaded[2 * i] && want[2 * k + 1] == loaded[2 * i + 1]) { in_new = true; have[k] = true; }
        if (!in_new) unload.emplace_back(loaded[2 * i], loaded[2 * i + 1]);
    }
    for (uint32_t k = 0; k < n; ++k) {
        bool dup = false;       // (the range wraps at 180 degrees: a location can appear twice; a HashSet holds it once)
        for (uint32_t j = 0; j < k && !dup; ++j) dup = want[2 * j] == want[2 * k] && want[2 * j + 1] == want[2 * k + 1];
        if (!have[k] && !dup) request.emplace_back(want[2 * k], want[2 * k + 1]);
    }
}

// Tile prefilter (host_math.hpp).  The planes are k_cull's clip_plane, term for term: 0..3 = w +- x, w +- y, 4 = near
// (z_clip >= 0), 5 = w - z, each with the norm of its (a, b, c).
uint32_t tile_prefilter(const topo_uniforms* views, uint32_t n_views, const double* spheres, uint32_t n_tiles, uint16_t* out, uint32_t cap) {
    uint32_t kept = 0;
    for (uint32_t v = 0; v < n_views; ++v) {
        const float* m = views[v].camera_proj;
        double q[6][5];
        for (int pl = 0; pl < 6; ++pl) {
            const int row = pl >> 1;
            const double sgn = (pl & 1) ? -1.0 : 1.0;
            double a, b, c, d;
            if (pl == 4) {
                a = m[2]; b = m[6]; c = m[10]; d = m[14];
            } else {
                a = (double)m[3] + sgn * (double)m[row];
                b = (double)m[7] + sgn * (double)m[4 + row];
                c = (double)m[11] + sgn * (double)m[8 + row];
                d = (double)m[15] + sgn * (double)m[12 + row];
            }
            q[pl][0] = a; q[pl][1] = b; q[pl][2] = c; q[pl][3] = d;
            q[pl][4] = std::sqrt(a * a + b * b + c * c);
        }
        for (uint32_t t = 0; t < n_tiles; ++t) {
            const double* s = spheres + (size_t)t * kTileSphereDoubles;
            bool outside = false;
            if (s[3] >= 0.0 && s[4] >= 0.0) {      // (NaN fails both, and every comparison below)
                const double reach = s[3] + s[4] + 1.0;
                for (int pl = 0; pl < 6 && !outside; ++pl)
                    outside = q[pl][0] * s[0] + q[pl][1] * s[1] + q[pl][2] * s[2] + q[pl][3] < -reach * q[pl][4];
            }
            if (outside) continue;
            if (kept < cap) out[kept] = (uint16_t)(v * n_tiles + t);
            ++kept;
        }
    }
    return kept;
}

// Synthetic COP90-shaped heights: 5-octave value-noise fBm over global texel coordinates with an integer
// hash (same definition as topo-renderer_amd/synth.py; f32 ops in the same order).
namespace {
inline float synth_hash(int64_t ix, int64_t iy, uint32_t seed) {
    uint32_t h = ((uint32_t)ix * 0x9E3779B1u) ^ ((uint32_t)iy * 0x85EBCA77u) ^ (seed * 0xC2B2AE3Du);
    h ^= h >> 15; h *= 0x2C1B3C6Du; h ^= h >> 12; h *= 0x297A2D39u; h ^= h >> 15;
    return (float)(h >> 8) * (1.0f / 16777216.0f);
}
}  // namespace

void synth_tile(int32_t lat, int32_t lon, uint32_t w, uint32_t h, uint32_t seed, float* out) {
    static const int wl[5] = {512, 256, 128, 64, 32};
    static const float amp[5] = {1.0f, 0.5f, 0.25f, 0.125f, 0.0625f};
    const float norm = (float)(3000.0 / 1.9375);
    for (uint32_t y = 0; y < h; ++y) {
        const int64_t gy = (int64_t)(89 - lat) * h + y;
        for (uint32_t x = 0; x < w; ++x) {
            const int64_t gx = ((int64_t)lon + 180) * w + x;
            float acc = 0.0f;
            for (int o = 0; o < 5; ++o) {
                const int64_t cx = gx / wl[o], cy = gy / wl[o];
                const float fx = (float)(gx % wl[o]) / (float)wl[o], fy = (float)(gy % wl[o]) / (float)wl[o];
                const float ux = fx * fx * (3.0f - 2.0f * fx), uy = fy * fy * (3.0f - 2.0f * fy);
                const uint32_t s = seed + (uint32_t)o;
                const float v00 = synth_hash(cx, cy, s), v10 = synth_hash(cx + 1, cy, s);
                const float v01 = synth_hash(cx, cy + 1, s), v11 = synth_hash(cx + 1, cy + 1, s);
                const float a = v00 + ux * (v10 - v00), b = v01 + ux * (v11 - v01);
                const float v = a + uy * (b - a);
                acc = acc + amp[o] * v;
            }
            out[(size_t)y * w + x] = acc * norm;
        }
    }
}

}  // namespace topo