// host_math.hpp -- host-side restatements of the reference's CPU math (glam 0.31) and the other pure functions behind the
// C ABI: no HIP, so host_math.cpp builds with any C++17 compiler.
#pragma once

#include <cstdint>
#include <utility>
#include <vector>

#include "../../include/topo_hip.h"

namespace topo {

void camera_uniforms(const float eye[3], float yaw, float pitch, float fov_y, float width, float height,
                     float sun_theta_deg, float sun_phi_deg, int32_t view_mode, topo_uniforms* out);
void panorama_uniforms(const float eye[3], float yaw0, float pitch, uint32_t sector_w, uint32_t sector_h, float sun_theta_deg, float sun_phi_deg,
                       int32_t view_mode, uint32_t n_sectors, topo_uniforms* out);
void geometry_transform(float h, float lon_deg, float lat_deg, float out[3]);
void pixel_angles(const topo_uniforms* view, uint32_t w, uint32_t h, uint32_t n, const float* xy, double* az_el);
// up = eye / |eye|, east = z x up normalised (at a pole: +y), north = up x east: the frame of topo_pixel_angles and topo_unwrap_*
void local_frame(const float eye[3], double east[3], double north[3], double up[3]);
// topo_sun_direction: the unit direction at azimuth / elevation (degrees) in that frame at the point (lon, lat) (degrees), f64
void sun_direction(double lon_deg, double lat_deg, double az_deg, double el_deg, double out[3]);
// unwrap (topo_unwrap_*): why the parameters / the views cannot be unwrapped (null: they can); the f64 tables k_unwrap reads
// (topo_unwrap.h has their layout); output-pixel coordinates of azimuth / elevation pairs
const char* unwrap_params_error(const topo_unwrap_params* p);
const char* unwrap_views_error(uint32_t n_views, const topo_uniforms* views, uint32_t src_w, uint32_t src_h);
void unwrap_tables(const topo_unwrap_params* p, uint32_t n_views, const topo_uniforms* views, std::vector<double>& out);
void unwrap_xy(const topo_unwrap_params* p, uint32_t n, const double* az_el, double* xy_out);
// topo_label_layout: the label rows of positions already known (topo_labels.h: label_place); the number placed or a TOPO_ERR_* code
int label_layout(uint32_t n, const uint32_t* x, const float* widths, uint32_t image_width, float row_height, uint32_t max_rows, int32_t* row_out, topo_label* out);
// why a label grid of image_width columns and max_rows rows cannot be had (null: it can), and the code that goes with it
const char* label_grid_error(uint64_t image_width, uint32_t max_rows, int* code);
void terrain_rotation(float model_lon_deg, float model_lat_deg, float rot3x3_colmajor[9]);
uint32_t locations_range(float latitude, float longitude, float range_dist, int32_t* out_lat_lon, uint32_t cap);
void change_location_plan(float latitude, float longitude, float range_dist, const int32_t* loaded, uint32_t n_loaded,
                          std::vector<std::pair<int32_t, int32_t>>& unload, std::vector<std::pair<int32_t, int32_t>>& request);
// Tile-level frustum prefilter of the cull: which (view, tile) pairs can hold a raster block that the device's frustum test
// (k_cull: the block's bounding sphere against the six clip planes of camera_proj, f64) keeps.  `spheres`: kTileSphereDoubles
// doubles per tile, in draw order -- the centre and radius of a sphere around the centres of the tile's block spheres, then the
// largest radius among those block spheres.  A pair is dropped only when that sphere, grown by the largest block radius and 1 m
// (the device adds its terms in another order), lies wholly outside one plane: every block of the tile then fails the device's
// test against the same plane.  An unknown sphere (radius < 0) or anything not finite keeps the pair.  The kept pairs' codes,
// view * n_tiles + tile, go to out[0 .. cap) in ascending order; returns how many were kept (those beyond cap are not written).
// Needs n_views * n_tiles <= 65536.  A function of its arguments alone: no HIP, no state.
constexpr uint32_t kTileSphereDoubles = 5;
uint32_t tile_prefilter(const topo_uniforms* views, uint32_t n_views, const double* spheres, uint32_t n_tiles, uint16_t* out, uint32_t cap);
void synth_tile(int32_t lat, int32_t lon, uint32_t w, uint32_t h, uint32_t seed, float* out);

}  // namespace topo
