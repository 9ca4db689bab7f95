"""topo-renderer_amd -- MI355X-native terrain-panorama render path of krzyz/topo-renderer.

Python is only the test/bench binding here: the product is `libtopo_hip.so` (hand-written gfx950 HIP kernels
behind the C ABI of include/topo_hip.h, host orchestration in C++).  This module mirrors the reference's
`TerrainRenderer` method set (topo-renderer/src/render/terrain_renderer.rs: new / update / add_terrain /
unload_terrain / render) over ctypes.

The directory name carries a hyphen, so it is imported through the loader `topo_renderer_amd.py` at the
repository root (``import topo_renderer_amd``).

There is no CPU fallback: if the shared library is missing, or no HIP device is present, calls raise.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import subprocess

import numpy as np

from . import panorama, synth  # noqa: F401  (re-exported)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TOPO_HIP_LIB") or os.path.join(_HERE, "libtopo_hip.so")   # TOPO_HIP_LIB: A/B builds
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "topo_hip.h")
TEST_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "topo_hip_test.h")      # test hooks: not part of the boundary

TOPO_OK = 0
TOPO_ERR_INVALID, TOPO_ERR_UNSUPPORTED, TOPO_ERR_HIP, TOPO_ERR_NOT_FOUND, TOPO_ERR_CAPACITY = -1, -2, -3, -4, -5
FORMAT_RGBA8_UNORM_SRGB, FORMAT_BGRA8_UNORM_SRGB, FORMAT_RGBA8_UNORM, FORMAT_BGRA8_UNORM = 1, 2, 3, 4
TIMING_SLOTS = 9
TIMING_NAMES = ("clear", "cull", "raster", "occlusion", "raster_big", "resolve", "total", "load", "load_tables")

NEAR, FAR = 50.0, 500000.0           # data/camera.rs:6-7
N_SECTORS = 8                        # fixed panorama sector count
HORIZON_SKY, HORIZON_INCOMPLETE = -1, -2
# topo_horizon_point (include/topo_hip.h), 32 bytes
HORIZON_DTYPE = np.dtype([("row", "<i4"), ("depth", "<f4"), ("lat_deg", "<i4"), ("lon_deg", "<i4"), ("cell_x", "<u4"), ("cell_y", "<u4"),
                          ("fan", "<u4"), ("_reserved", "<u4")])
GROUND_TERRAIN, GROUND_SKY, GROUND_OUTSIDE, GROUND_INCOMPLETE, GROUND_DEGENERATE = 1, 0, -1, -2, -3
# topo_ground_point, 64 bytes, and topo_ground_query, 16 bytes
GROUND_DTYPE = np.dtype([("lon_deg", "<f8"), ("lat_deg", "<f8"), ("height_m", "<f4"), ("range_m", "<f4"), ("depth", "<f4"), ("kind", "<i4"),
                         ("tile_lat_deg", "<i4"), ("tile_lon_deg", "<i4"), ("cell_x", "<u4"), ("cell_y", "<u4"), ("tri", "<u4"), ("fan", "<u4"),
                         ("w1", "<f4"), ("w2", "<f4")])
GROUND_QUERY_DTYPE = np.dtype([("view", "<u4"), ("x", "<u4"), ("y", "<u4"), ("_reserved", "<u4")])
RAY_HIT, RAY_MISS, RAY_INVALID = 1, 0, -1
SUN_NONE, SUN_LIT, SUN_AWAY, SUN_SHADOW = 0, 1, 2, 3
# topo_ray and topo_ray_hit, 64 bytes each
RAY_DTYPE = np.dtype([("origin", "<f8", 3), ("dir", "<f8", 3), ("t_min", "<f8"), ("t_max", "<f8")])
RAY_HIT_DTYPE = np.dtype([("t", "<f8"), ("lon_deg", "<f8"), ("lat_deg", "<f8"), ("height_m", "<f4"), ("kind", "<i4"), ("tile_lat_deg", "<i4"),
                          ("tile_lon_deg", "<i4"), ("cell_x", "<u4"), ("cell_y", "<u4"), ("tri", "<u4"), ("front", "<u4"), ("w1", "<f4"), ("w2", "<f4")])
SURFACE_TERRAIN, SURFACE_NONE, SURFACE_INVALID = 1, 0, -1
PROFILE_NO_SAMPLE = 0xFFFFFFFF
# topo_surface_point, 48 bytes, and topo_profile_summary, 16 bytes
SURFACE_DTYPE = np.dtype([("height_m", "<f8"), ("slope_deg", "<f4"), ("aspect_deg", "<f4"), ("kind", "<i4"), ("tile_lat_deg", "<i4"), ("tile_lon_deg", "<i4"),
                          ("cell_x", "<u4"), ("cell_y", "<u4"), ("tri", "<u4"), ("w1", "<f4"), ("w2", "<f4")])
PROFILE_SUMMARY_DTYPE = np.dtype([("min_clearance_m", "<f4"), ("min_sample", "<u4"), ("n_terrain", "<u4"), ("kind", "<i4")])
VIS_NONE, VIS_VISIBLE, VIS_AWAY, VIS_HIDDEN, VIS_NO_OBSERVER = 0, 1, 2, 3, 4
OBSERVER_ABOVE_TERRAIN = 1
REFRACTION_STANDARD = 0.13      # TOPO_REFRACTION_STANDARD: the coefficient k of the standard atmosphere
# topo_observer, 32 bytes
OBSERVER_DTYPE = np.dtype([("lon_deg", "<f8"), ("lat_deg", "<f8"), ("height_m", "<f8"), ("flags", "<u4"), ("_reserved", "<u4")])
SKY_NONE, SKY_TERRAIN, SKY_NO_OBSERVER = 0, 1, 4
# topo_skyline_sample, 64 bytes
SKYLINE_DTYPE = np.dtype([("elevation_deg", "<f8"), ("range_m", "<f8"), ("lon_deg", "<f8"), ("lat_deg", "<f8"), ("height_m", "<f4"), ("kind", "<i4"),
                          ("tile_lat_deg", "<i4"), ("tile_lon_deg", "<i4"), ("cell_x", "<u4"), ("cell_y", "<u4"), ("tri", "<u4"), ("edge", "<u4")])
SUN_NIGHT = 4
# topo_sun, 32 bytes
SUN_DTYPE = np.dtype([("dir", "<f8", 3), ("weight", "<f8")])
LABEL_HIDDEN, LABEL_PLACED, LABEL_NO_ROW, LABEL_BAD_WIDTH = 0, 1, 2, 3      # the state bytes of topo_labels_*
# topo_label, 32 bytes, and topo_label_params, 16 bytes
LABEL_DTYPE = np.dtype([("peak", "<u4"), ("view", "<u4"), ("row", "<u4"), ("label_x", "<f4"), ("label_y", "<f4"), ("label_width", "<f4"), ("peak_x", "<f4"),
                        ("peak_y", "<f4")])
LABEL_PARAMS_DTYPE = np.dtype([("row_height", "<f4"), ("max_rows", "<u4"), ("views_per_image", "<u4"), ("cap", "<u4")])
SUMMIT_ORDER_TILE, SUMMIT_ORDER_HEIGHT, SUMMIT_ORDER_ISOLATION = 0, 1, 2
SNAP_FOUND, SNAP_NONE, SNAP_INVALID = 1, 0, -1
# topo_summit_params, 24 bytes, topo_summit, 64 bytes, and topo_summit_snap, 48 bytes
SUMMIT_PARAMS_DTYPE = np.dtype([("radius_m", "<f8"), ("min_isolation_m", "<f8"), ("min_height_m", "<f4"), ("order", "<u4")])
SUMMIT_DTYPE = np.dtype([("lon_deg", "<f8"), ("lat_deg", "<f8"), ("isolation_m", "<f8"), ("height_m", "<f4"), ("higher_height_m", "<f4"), ("tile_lat_deg", "<i4"),
                         ("tile_lon_deg", "<i4"), ("vx", "<u4"), ("vy", "<u4"), ("higher_tile_lat_deg", "<i4"), ("higher_tile_lon_deg", "<i4"), ("higher_vx", "<u4"),
                         ("higher_vy", "<u4")])
SUMMIT_SNAP_DTYPE = np.dtype([("lon_deg", "<f8"), ("lat_deg", "<f8"), ("distance_m", "<f8"), ("height_m", "<f4"), ("status", "<i4"), ("tile_lat_deg", "<i4"),
                              ("tile_lon_deg", "<i4"), ("vx", "<u4"), ("vy", "<u4")])
MAP_RELIEF, MAP_CONTOURS, MAP_SEEN = 1, 2, 4                                # topo_map_params.layers
MAP_FLAG_TERRAIN, MAP_FLAG_CONTOUR, MAP_FLAG_INDEX, MAP_FLAG_SEEN = 1, 2, 4, 8      # the flags byte of topo_map_*
# topo_map_params, 88 bytes
MAP_PARAMS_DTYPE = np.dtype([("lon0_deg", "<f8"), ("lat0_deg", "<f8"), ("dlon_deg", "<f8"), ("dlat_deg", "<f8"), ("contour_interval_m", "<f8"), ("nx", "<u4"), ("ny", "<u4"),
                             ("index_every", "<u4"), ("layers", "<u4"), ("sun_direction", "<f4", 3), ("void_rgba", "u1", 4), ("seen_rgba", "u1", 4),
                             ("contour_rgba", "u1", 4), ("index_rgba", "u1", 4), ("reserved", "<u4")])
UNWRAP_EQUIRECTANGULAR, UNWRAP_CYLINDRICAL = 0, 1
UNWRAP_NEAREST, UNWRAP_BILINEAR = 0, 1
# topo_debug_read_cull_lists (test hook): WorkItem and FarItem of csrc/topo_kernels.h
WORK_ITEM_DTYPE = np.dtype([("view_rank", "<u4"), ("block", "<u4")])      # block | first cell row << 24 | rows << 28 (rows 0: the whole block)
FAR_ITEM_DTYPE = np.dtype([("view_rank", "<u4"), ("block", "<u4"), ("x0", "<u2"), ("x1", "<u2"), ("y0", "<u2"), ("y1", "<u2"), ("zmin", "<f4")])
# topo_unwrap_params, 48 bytes
UNWRAP_PARAMS_DTYPE = np.dtype([("projection", "<u4"), ("filter", "<u4"), ("out_w", "<u4"), ("out_h", "<u4"), ("az0_deg", "<f8"), ("az_span_deg", "<f8"),
                                ("el_top_deg", "<f8"), ("el_bottom_deg", "<f8")])


class TopoError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"topo_hip error {code}: {msg}")
        self.code = code


def build(verbose: bool = False) -> str:
    """Compile libtopo_hip.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    subprocess.check_call(["make", "-C", os.path.join(_HERE, "csrc"), "all"] + ([] if verbose else ["-s"]))
    return LIB_PATH


_lib = None


def _preload_torch_hip_runtime():
    """PyTorch wheels bundle their own libamdhip64.so (same SONAME as /opt/rocm's).  Two HIP runtimes in one
    process cannot both own the GPU, so when torch is installed its runtime is loaded first and
    libtopo_hip.so binds to it; processes that never import torch are unaffected."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec and spec.submodule_search_locations:
        cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)


def lib():
    """The loaded C ABI.  Fails loudly when the HIP extension has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing -- run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(there is no Python/CPU fallback for the render path)")
        _preload_torch_hip_runtime()
        L = C.CDLL(LIB_PATH)
        vp, u32, i32, f32, sz = C.c_void_p, C.c_uint32, C.c_int32, C.c_float, C.c_size_t
        sigs = {
            "topo_create": (C.c_int, [C.POINTER(vp), C.c_int, u32, u32, u32]),
            "topo_destroy": (None, [vp]),
            "topo_last_error": (C.c_char_p, [vp]),
            "topo_add_terrain": (C.c_int, [vp, i32, i32, vp, u32, u32, vp, vp, vp]),
            "topo_add_terrain_device": (C.c_int, [vp, i32, i32, vp, u32, u32, vp, vp, vp]),
            "topo_unload_terrain": (C.c_int, [vp, i32, i32]),
            "topo_update": (C.c_int, [vp, u32, u32, vp, vp]),
            "topo_render": (C.c_int, [vp, vp, sz, vp, sz]),
            "topo_recompute_normals": (C.c_int, [vp]),
            "topo_render_views_device": (C.c_int, [vp, u32, vp, u32, u32, vp, sz, sz, vp, sz, sz]),
            "topo_set_stream": (C.c_int, [vp, vp]),
            "topo_synchronize": (C.c_int, [vp]),
            "topo_set_normals_lds_rows": (C.c_int, [vp, C.c_int]),
            "topo_debug_set_queue_caps": (C.c_int, [vp, u32, u32]),
            "topo_debug_far_phase_launched": (C.c_int, [vp, vp]),
            "topo_debug_set_tile_prefilter": (C.c_int, [vp, i32]),
            "topo_debug_cull_pairs": (C.c_int, [vp, vp]),
            "topo_debug_cover_stats": (C.c_int, [vp, vp]),
            "topo_debug_set_resolve_owned": (C.c_int, [vp, i32]),
            "topo_debug_owned_strips": (C.c_int, [vp, vp]),
            "topo_debug_read_cull_lists": (C.c_int, [vp, vp, u32, vp, u32, vp, u32, vp]),
            "topo_pin_host_buffer": (C.c_int, [vp, vp, sz]),
            "topo_unpin_host_buffer": (C.c_int, [vp, vp]),
            "topo_get_timings": (C.c_int, [vp, vp]),
            "topo_get_timing_history": (C.c_int, [vp, C.c_uint32, vp, vp]),
            "topo_get_counters": (C.c_int, [vp, vp]),
            "topo_set_occlusion_split": (C.c_int, [vp, f32]),
            "topo_set_timing_slots": (C.c_int, [vp, u32]),
            "topo_read_normals": (C.c_int, [vp, i32, i32, vp]),
            "topo_read_tile_tables": (C.c_int, [vp, i32, i32, vp, vp, vp, vp]),
            "topo_probe_sincos": (C.c_int, [vp, vp, vp, vp, sz]),
            "topo_probe_div": (C.c_int, [vp, i32, vp, vp, vp, sz]),
            "topo_set_pipeline_depth": (C.c_int, [vp, i32]),
            "topo_join": (C.c_int, [vp]),
            "topo_frame_status": (C.c_int, [vp, vp]),
            "topo_overlay_lines": (C.c_int, [vp, vp, u32, vp, u32, f32, vp, sz]),
            "topo_overlay_lines_device": (C.c_int, [vp, vp, u32, vp, u32, f32, vp, sz]),
            "topo_overlay_glyphs": (C.c_int, [vp, vp, u32, C.c_float, vp, u32, u32, vp, sz]),
            "topo_overlay_glyphs_device": (C.c_int, [vp, vp, u32, C.c_float, vp, u32, u32, vp, sz]),
            "topo_change_location_plan": (None, [f32, f32, f32, vp, u32, vp, u32, vp, vp, u32, vp]),
            "topo_change_location": (C.c_int, [vp, f32, f32, f32, vp, u32, vp, vp]),
            "topo_comm_unique_id": (C.c_int, [vp]),
            "topo_comm_init": (C.c_int, [C.POINTER(vp), C.c_int, vp, C.c_int, C.c_int]),
            "topo_comm_from_nccl": (C.c_int, [C.POINTER(vp), vp, C.c_int, C.c_int]),
            "topo_comm_destroy": (None, [vp]),
            "topo_panorama_sector_range": (None, [C.c_int, C.c_int, vp, vp]),
            "topo_panorama_slots": (u32, [C.c_int, u32, u32, vp, u32]),
            "topo_render_panorama": (C.c_int, [vp, vp, vp, f32, f32, u32, u32, f32, f32, i32, vp, vp]),
            "topo_render_batch": (C.c_int, [vp, u32, vp, vp, vp, f32, u32, u32, i32, vp, vp]),
            "topo_visible_peaks": (C.c_int, [vp, u32, vp, vp, vp]),
            "topo_visible_peaks_device": (C.c_int, [vp, vp, u32, u32, vp, sz, u32, vp, vp, vp]),
            "topo_camera_uniforms": (None, [vp, f32, f32, f32, f32, f32, f32, f32, i32, vp]),
            "topo_terrain_uniforms": (None, [vp, vp, vp, u32, u32, vp]),
            "topo_geometry_transform": (None, [f32, f32, f32, vp]),
            "topo_dist_from_depth": (f32, [f32]),
            "topo_pad_256": (u32, [u32]),
            "topo_synth_tile": (None, [i32, i32, u32, u32, u32, vp]),
            "topo_locations_range": (u32, [f32, f32, f32, vp, u32]),
            "topo_coordinate_transform": (C.c_int, [vp, u32, vp, u32, vp, vp, vp, vp]),
            "topo_geotiff_info": (C.c_int, [vp, sz, vp, vp, vp, vp, vp]),
            "topo_sector_fov_y": (f32, [u32, u32, u32]),
            "topo_panorama_uniforms": (None, [vp, f32, f32, u32, u32, f32, f32, i32, u32, vp]),
            "topo_render_device": (C.c_int, [vp, vp, sz, vp, sz]),
            "topo_geotiff_decode": (C.c_int, [vp, vp, sz, vp, sz]),
            "topo_add_terrain_geotiff": (C.c_int, [vp, i32, i32, vp, sz]),
            "topo_to_model": (None, [vp, vp, vp, f32, f32, vp]),
            "topo_to_raster": (None, [vp, vp, vp, f32, f32, vp]),
            "topo_height_value_at": (C.c_int, [vp, u32, u32, vp, vp, vp, C.c_double, C.c_double, vp]),
            "topo_viewshed_enable": (C.c_int, [vp, i32]),
            "topo_viewshed_reset": (C.c_int, [vp]),
            "topo_viewshed_read": (C.c_int, [vp, i32, i32, vp, sz, vp]),
            "topo_debug_viewshed_stats": (C.c_int, [vp, vp]),
            "topo_horizon_shape": (C.c_int, [vp, vp, vp, vp]),
            "topo_horizon_read": (C.c_int, [vp, u32, u32, vp, sz]),
            "topo_horizon_device": (C.c_int, [vp, u32, u32, vp, sz]),
            "topo_pixel_angles": (None, [vp, u32, u32, u32, vp, vp]),
            "topo_ground_read": (C.c_int, [vp, u32, vp, vp]),
            "topo_ground_device": (C.c_int, [vp, u32, vp, vp]),
            "topo_ground_map_device": (C.c_int, [vp, u32, u32, vp, sz, sz]),
            "topo_raycast_read": (C.c_int, [vp, u32, vp, vp]),
            "topo_raycast_device": (C.c_int, [vp, u32, vp, vp]),
            "topo_sunlit_map_device": (C.c_int, [vp, u32, u32, vp, vp, sz, sz]),
            "topo_sun_direction": (None, [C.c_double, C.c_double, C.c_double, C.c_double, vp]),
            "topo_surface_read": (C.c_int, [vp, u32, vp, vp]),
            "topo_surface_device": (C.c_int, [vp, u32, vp, vp]),
            "topo_surface_grid_device": (C.c_int, [vp, C.c_double, C.c_double, C.c_double, C.c_double, u32, u32, vp, sz]),
            "topo_profile_device": (C.c_int, [vp, u32, vp, u32, vp, sz, vp]),
            "topo_profile_read": (C.c_int, [vp, u32, vp, u32, vp, vp]),
            "topo_visibility_grid_device": (C.c_int, [vp, u32, vp, C.c_double, C.c_double, C.c_double, C.c_double, u32, u32, C.c_double, vp, sz, sz]),
            "topo_visibility_device": (C.c_int, [vp, u32, vp, u32, vp, C.c_double, vp, sz]),
            "topo_visibility_read": (C.c_int, [vp, u32, vp, u32, vp, C.c_double, vp]),
            "topo_skyline_device": (C.c_int, [vp, u32, vp, C.c_double, C.c_double, u32, C.c_double, C.c_double, vp, sz, vp, sz]),
            "topo_skyline_read": (C.c_int, [vp, u32, vp, C.c_double, C.c_double, u32, C.c_double, C.c_double, vp, vp]),
            "topo_sun_exposure_grid_device": (C.c_int, [vp, u32, vp, C.c_double, C.c_double, C.c_double, C.c_double, u32, u32, vp, vp, vp, sz, sz]),
            "topo_sun_exposure_device": (C.c_int, [vp, u32, vp, u32, vp, vp, vp, vp]),
            "topo_sun_exposure_read": (C.c_int, [vp, u32, vp, u32, vp, vp, vp, vp]),
            "topo_label_layout": (C.c_int, [u32, vp, vp, u32, f32, u32, vp, vp]),
            "topo_labels_device": (C.c_int, [vp, vp, u32, vp, u32, u32, vp, sz, sz, u32, vp, vp, vp, vp, vp]),
            "topo_labels_read": (C.c_int, [vp, vp, u32, vp, u32, u32, vp, sz, sz, u32, vp, vp, vp, vp, vp]),
            "topo_summits_device": (C.c_int, [vp, vp, vp, u32, vp]),
            "topo_summits_read": (C.c_int, [vp, vp, vp, u32, vp]),
            "topo_summit_snap_device": (C.c_int, [vp, u32, vp, C.c_double, vp]),
            "topo_summit_snap_read": (C.c_int, [vp, u32, vp, C.c_double, vp]),
            "topo_debug_set_summit_band_rows": (C.c_int, [vp, u32]),
            "topo_debug_summit_counts": (C.c_int, [vp, vp]),
            "topo_map_device": (C.c_int, [vp, vp, vp, sz, vp, sz]),
            "topo_map_read": (C.c_int, [vp, vp, vp, vp]),
            "topo_map_xy": (None, [vp, u32, vp, vp]),
            "topo_map_rows_per_wave": (u32, []),
            "topo_ecef_from_lonlat": (None, [C.c_double, C.c_double, C.c_double, vp]),
            "topo_visibility_refracted_grid_device": (C.c_int, [vp, u32, vp, C.c_double, C.c_double, C.c_double, C.c_double, u32, u32, C.c_double, C.c_double, vp, sz, sz]),
            "topo_visibility_refracted_device": (C.c_int, [vp, u32, vp, u32, vp, C.c_double, C.c_double, vp, sz]),
            "topo_visibility_refracted_read": (C.c_int, [vp, u32, vp, u32, vp, C.c_double, C.c_double, vp]),
            "topo_refraction_lift": (C.c_int, [vp, vp, C.c_double, vp]),
            "topo_unwrap_device": (C.c_int, [vp, vp, u32, vp, u32, u32, vp, sz, sz, vp, sz, sz, vp, sz, vp, sz, vp, sz]),
            "topo_unwrap_xy": (None, [vp, u32, vp, vp]),
        }
        for name, (res, args) in sigs.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        L._topo_symbols = tuple(sigs)
        _lib = L
    return _lib


def map_params(lon0: float, lat0: float, dlon: float, dlat: float, nx: int, ny: int, sun_direction=(0.0, 0.0, 1.0), contour_interval_m: float = 0.0,
               index_every: int = 0, layers: int = MAP_RELIEF | MAP_CONTOURS | MAP_SEEN, void_rgba=(0, 0, 0, 0), seen_rgba=(255, 208, 0, 96),
               contour_rgba=(96, 64, 32, 160), index_rgba=(64, 32, 16, 255)):
    """One MAP_PARAMS_DTYPE record (topo_map_params): pixel (c, r) at lon0 + c * dlon, lat0 + r * dlat."""
    p = np.zeros(1, MAP_PARAMS_DTYPE)
    p["lon0_deg"], p["lat0_deg"], p["dlon_deg"], p["dlat_deg"], p["nx"], p["ny"] = lon0, lat0, dlon, dlat, nx, ny
    p["contour_interval_m"], p["index_every"], p["layers"] = contour_interval_m, index_every, layers
    p["sun_direction"][0] = np.asarray(sun_direction, np.float32)
    for k, v in (("void_rgba", void_rgba), ("seen_rgba", seen_rgba), ("contour_rgba", contour_rgba), ("index_rgba", index_rgba)):
        p[k][0] = np.asarray(v, np.uint8)
    return p


def map_xy(params, lonlat) -> np.ndarray:
    """topo_map_xy: (n, 2) f64 (longitude, latitude) in degrees -> (n, 2) f64 fractional (column, row) of the map; NaN where there is
    none.  Pure: no context, no GPU."""
    p = np.ascontiguousarray(params, dtype=MAP_PARAMS_DTYPE).reshape(-1)[:1]
    ll = np.ascontiguousarray(lonlat, dtype=np.float64).reshape(-1, 2)
    out = np.zeros((len(ll), 2), np.float64)
    lib().topo_map_xy(_p(p), len(ll), _p(ll) if len(ll) else None, _p(out) if len(ll) else None)
    return out


def summit_params(radius_m: float, min_isolation_m: float = 0.0, min_height_m: float = -np.inf, order: int = SUMMIT_ORDER_TILE):
    """One SUMMIT_PARAMS_DTYPE record (topo_summit_params)."""
    p = np.zeros(1, SUMMIT_PARAMS_DTYPE)
    p["radius_m"], p["min_isolation_m"], p["min_height_m"], p["order"] = radius_m, min_isolation_m, min_height_m, order
    return p


def order_summits(records, order: int):
    """Records in tile order (any dtype with height_m and isolation_m) as topo_summits_read orders them: TILE as they are; HEIGHT by
    height descending; ISOLATION by isolation descending (+inf first), then height descending; ties stay in tile order."""
    r = np.asarray(records)
    if order == SUMMIT_ORDER_TILE:
        return r.copy()
    k = np.arange(len(r))
    if order == SUMMIT_ORDER_HEIGHT:
        return r[np.lexsort((k, -r["height_m"].astype(np.float64)))]
    if order == SUMMIT_ORDER_ISOLATION:
        return r[np.lexsort((k, -r["height_m"].astype(np.float64), -r["isolation_m"]))]
    raise ValueError("unknown order")


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- host-side helpers (reference CPU code restated in the library) ------------------------------------

def camera_uniforms(eye, yaw, pitch, fov_y, width, height, sun_theta_deg, sun_phi_deg, view_mode=0) -> np.ndarray:
    """Uniforms::new(&camera, bounds) -> 40 x f32 view of the 160-byte struct (render/data.rs:33-58)."""
    out = np.zeros(40, dtype=np.float32)
    e = np.ascontiguousarray(eye, dtype=np.float32)
    lib().topo_camera_uniforms(_p(e), yaw, pitch, fov_y, width, height, sun_theta_deg, sun_phi_deg, view_mode, _p(out))
    return out


def terrain_uniforms(raster_point, model_point, pixel_scale, w, h) -> np.ndarray:
    out = np.zeros(24, dtype=np.float32)
    rp, mp, ps = (np.ascontiguousarray(a, dtype=np.float32) for a in (raster_point, model_point, pixel_scale))
    lib().topo_terrain_uniforms(_p(rp), _p(mp), _p(ps), w, h, _p(out))
    return out


def geometry_transform(h, lon_deg, lat_deg) -> np.ndarray:
    out = np.zeros(3, dtype=np.float32)
    lib().topo_geometry_transform(h, lon_deg, lat_deg, _p(out))
    return out


def dist_from_depth(d: float) -> float:
    return float(lib().topo_dist_from_depth(d))


def pad_256(n: int) -> int:
    return int(lib().topo_pad_256(n))


def synth_tile(lat_deg, lon_deg, w=1200, h=1200, seed=synth.SEED_DEFAULT) -> np.ndarray:
    """C++ twin of synth.synth_tile (bit-identical, ~50x faster)."""
    out = np.empty((h, w), dtype=np.float32)
    lib().topo_synth_tile(lat_deg, lon_deg, w, h, seed & 0xFFFFFFFF, _p(out))
    return out


def locations_range(latitude: float, longitude: float, range_dist: float = 100_000.0):
    """UiController::get_locations_range (ui_controller.rs:61-83): [(lat_deg, lon_deg), ...] in the reference's order."""
    buf = np.zeros((4096, 2), np.int32)
    n = int(lib().topo_locations_range(latitude, longitude, range_dist, _p(buf), 4096))
    return [(int(a), int(b)) for a, b in buf[:min(n, 4096)]]


def change_location_plan(latitude: float, longitude: float, loaded, range_dist: float = 100_000.0):
    """UiController::change_location's set arithmetic (ui_controller.rs:23-59): (to_unload, to_request) for a list of loaded
    (lat_deg, lon_deg) tiles."""
    ld = np.ascontiguousarray(np.array(list(loaded), dtype=np.int32).reshape(-1, 2))
    un, rq = np.zeros((4096, 2), np.int32), np.zeros((4096, 2), np.int32)
    nu, nr = C.c_uint32(), C.c_uint32()
    lib().topo_change_location_plan(latitude, longitude, range_dist, _p(ld) if len(ld) else None, len(ld), _p(un), 4096, C.byref(nu), _p(rq), 4096, C.byref(nr))
    return [(int(a), int(b)) for a, b in un[:nu.value]], [(int(a), int(b)) for a, b in rq[:nr.value]]


class CoordinateTransform:
    """CoordinateTransform (common/coordinate_transform.rs:16-71): the six f32 a tile's GeoTIFF tags reduce to."""

    def __init__(self, raster_point, model_point, pixel_scale):
        self.raster_point = np.asarray(raster_point, np.float32)
        self.model_point = np.asarray(model_point, np.float32)
        self.pixel_scale = np.asarray(pixel_scale, np.float32)

    @classmethod
    def from_geo_tag_data(cls, pixel_scale_data, tie_points_data, model_transformation_data=None):
        """Raises TopoError(UNSUPPORTED) for IncorrectGeoTags and TopoError(INVALID) for IncorrectGeoTagData."""
        arr = lambda v: None if v is None else np.ascontiguousarray(v, dtype=np.float64)
        ps, tp, mt = arr(pixel_scale_data), arr(tie_points_data), arr(model_transformation_data)
        rp, mp, sc = (np.zeros(2, np.float32) for _ in range(3))
        ptr = lambda a: None if a is None else _p(a)
        rc = lib().topo_coordinate_transform(ptr(ps), 0 if ps is None else ps.size, ptr(tp), 0 if tp is None else tp.size, ptr(mt),
                                             _p(rp), _p(mp), _p(sc))
        if rc != 0:
            raise TopoError(rc, "IncorrectGeoTags" if rc == -2 else "IncorrectGeoTagData")
        return cls(rp, mp, sc)

    def to_model(self, x, y):
        out = np.zeros(2, np.float32)
        lib().topo_to_model(_p(self.raster_point), _p(self.model_point), _p(self.pixel_scale), x, y, _p(out))
        return float(out[0]), float(out[1])

    def to_raster(self, lon, lat):
        out = np.zeros(2, np.float32)
        lib().topo_to_raster(_p(self.raster_point), _p(self.model_point), _p(self.pixel_scale), lon, lat, _p(out))
        return float(out[0]), float(out[1])

    def height_value_at(self, heights: np.ndarray, longitude: float, latitude: float):
        """get_height_value_at (coordinate_transform.rs:73-90): the f32 height, or None where the reference yields None."""
        hts = np.ascontiguousarray(heights, dtype=np.float32)
        h, w = hts.shape
        out = np.zeros(1, np.float32)
        rc = lib().topo_height_value_at(_p(hts), w, h, _p(self.raster_point), _p(self.model_point), _p(self.pixel_scale),
                                        float(longitude), float(latitude), _p(out))
        return None if rc != 0 else float(out[0])


def geotiff_info(data: bytes):
    """(width, height, CoordinateTransform) of a GeoTIFF's first image (topo_geotiff_info); no GPU involved."""
    buf = np.frombuffer(data, np.uint8)
    w, h = C.c_uint32(), C.c_uint32()
    rp, mp, sc = (np.zeros(2, np.float32) for _ in range(3))
    rc = lib().topo_geotiff_info(_p(buf), buf.size, C.byref(w), C.byref(h), _p(rp), _p(mp), _p(sc))
    if rc != 0:
        raise TopoError(rc, "GeoTIFF container or geo tags not usable")
    return int(w.value), int(h.value), CoordinateTransform(rp, mp, sc)


def ground_queries(queries) -> np.ndarray:
    """GROUND_QUERY_DTYPE records from such records or from an (n, 3) integer array of (view, x, y)."""
    q = np.asarray(queries)
    if q.dtype == GROUND_QUERY_DTYPE:
        return np.ascontiguousarray(q).reshape(-1)
    q = q.reshape(-1, 3)
    out = np.zeros(len(q), GROUND_QUERY_DTYPE)
    out["view"], out["x"], out["y"] = q[:, 0], q[:, 1], q[:, 2]
    return out


def rays(origin, direction, t_min=0.0, t_max=np.inf) -> np.ndarray:
    """RAY_DTYPE records (topo_ray) from origins and directions (f64 ECEF metres, (3,) or (n, 3), broadcast against each other) and
    bounds on t (scalars or (n,)); dir need not be unit: dir = B - A with t in [0, 1] is the segment from A to B."""
    o, d = np.broadcast_arrays(np.atleast_2d(np.asarray(origin, np.float64)), np.atleast_2d(np.asarray(direction, np.float64)))
    out = np.zeros(len(o), RAY_DTYPE)
    out["origin"], out["dir"], out["t_min"], out["t_max"] = o, d, t_min, t_max
    return out


def ecef_from_lonlat(lon_deg: float, lat_deg: float, height_m: float = 0.0) -> np.ndarray:
    """topo_ecef_from_lonlat: the f64 ECEF point height_m above the sphere R0 at (lon_deg, lat_deg), in the frame of the rays."""
    out = np.zeros(3, dtype=np.float64)
    lib().topo_ecef_from_lonlat(lon_deg, lat_deg, height_m, _p(out))
    return out


def refraction_lift(observer, point, k: float = REFRACTION_STANDARD) -> np.ndarray:
    """topo_refraction_lift: the f64 ECEF point where `point` is seen from `observer` under refraction coefficient k along straight
    lines -- the same direction, the radius raised by k |point - observer|^2 / (2 R0); no GPU."""
    o, p = np.ascontiguousarray(observer, dtype=np.float64).reshape(3), np.ascontiguousarray(point, dtype=np.float64).reshape(3)
    out = np.zeros(3, dtype=np.float64)
    rc = lib().topo_refraction_lift(_p(o), _p(p), k, _p(out))
    if rc != TOPO_OK:
        raise TopoError(rc, "topo_refraction_lift: k must lie in 0 <= k < 1")
    return out


def observers(lon_deg, lat_deg, height_m, above_terrain=True) -> np.ndarray:
    """OBSERVER_DTYPE records (topo_observer) from arrays (or scalars) of longitude, latitude and height; above_terrain: the height is
    measured above the drawn terrain (OBSERVER_ABOVE_TERRAIN), else above the sphere R0."""
    lo, la, h, f = np.broadcast_arrays(np.atleast_1d(np.asarray(lon_deg, np.float64)), np.asarray(lat_deg, np.float64), np.asarray(height_m, np.float64),
                                       np.asarray(above_terrain, bool))
    out = np.zeros(len(lo), OBSERVER_DTYPE)
    out["lon_deg"], out["lat_deg"], out["height_m"], out["flags"] = lo, la, h, np.where(f, OBSERVER_ABOVE_TERRAIN, 0)
    return out


def suns(dirs, weights=1.0) -> np.ndarray:
    """SUN_DTYPE records (topo_sun) from directions TOWARDS the sun (f64 ECEF, (3,) or (n, 3); they need not be unit, see
    sun_direction) and weights (a scalar or (n,)): minutes per sample, say."""
    d = np.atleast_2d(np.asarray(dirs, np.float64))
    out = np.zeros(len(d), SUN_DTYPE)
    out["dir"], out["weight"] = d, weights
    return out


def sun_direction(lon_deg: float, lat_deg: float, az_deg: float, el_deg: float) -> np.ndarray:
    """topo_sun_direction: the unit f64 ECEF direction at azimuth az_deg (clockwise from true north) and elevation el_deg at the
    point (lon_deg, lat_deg), in the east / north / up frame of pixel_angles and unwrap_device.  Host only."""
    out = np.zeros(3, np.float64)
    lib().topo_sun_direction(lon_deg, lat_deg, az_deg, el_deg, _p(out))
    return out


def pixel_angles(view_uniforms, width: int, height: int, xy) -> np.ndarray:
    """topo_pixel_angles: (n, 2) f64 (azimuth degrees clockwise from true north, elevation degrees above the eye's horizontal plane)
    of the pixel-space points xy (n, 2) of a view of width x height with these uniforms (160 bytes)."""
    u = np.ascontiguousarray(view_uniforms).view(np.uint8)
    if u.nbytes != 160:
        raise ValueError("uniforms must be 160 bytes")
    pts = np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, 2)
    out = np.zeros((len(pts), 2), np.float64)
    lib().topo_pixel_angles(_p(u), width, height, len(pts), _p(pts), _p(out))
    return out


def unwrap_params(out_w: int, out_h: int, el_top_deg: float, el_bottom_deg: float, az0_deg: float = 0.0, az_span_deg: float = 360.0,
                  projection: int = UNWRAP_EQUIRECTANGULAR, filter: int = UNWRAP_NEAREST) -> np.ndarray:
    """A topo_unwrap_params record: an out_w x out_h image over [az0, az0 + span) degrees clockwise from north and
    [el_bottom, el_top] degrees of elevation, rows linear in the elevation (equirectangular) or in its tangent (cylindrical)."""
    p = np.zeros(1, UNWRAP_PARAMS_DTYPE)
    p["projection"], p["filter"], p["out_w"], p["out_h"] = projection, filter, out_w, out_h
    p["az0_deg"], p["az_span_deg"], p["el_top_deg"], p["el_bottom_deg"] = az0_deg, az_span_deg, el_top_deg, el_bottom_deg
    return p


def unwrap_xy(params, az_el) -> np.ndarray:
    """topo_unwrap_xy: (n, 2) f64 output-pixel coordinates of (n, 2) azimuth / elevation pairs in degrees (what pixel_angles
    returns); NaN for parameters the library refuses."""
    p = np.ascontiguousarray(params, dtype=UNWRAP_PARAMS_DTYPE).reshape(-1)[:1]
    a = np.ascontiguousarray(az_el, dtype=np.float64).reshape(-1, 2)
    out = np.full((len(a), 2), np.nan, np.float64)
    lib().topo_unwrap_xy(_p(p), len(a), _p(a), _p(out))
    return out


def label_params(row_height: float = 20.0, max_rows: int = 8, views_per_image: int = 1, cap: int = 0) -> np.ndarray:
    """A topo_label_params record (the reference: row_height = LINE_HEIGHT + LINE_PADDING = 20, MAX_ROWS = 8, one view per image)."""
    p = np.zeros(1, LABEL_PARAMS_DTYPE)
    p["row_height"], p["max_rows"], p["views_per_image"], p["cap"] = row_height, max_rows, views_per_image, cap
    return p


def label_layout(x, widths, image_width: int, row_height: float = 20.0, max_rows: int = 8):
    """topo_label_layout: the layout rule on the host for labels at columns x (n,) with widths (n,) f32 in an image of image_width
    columns -> ((n,) int32 rows: -1 no row free, -2 unusable width; the placed labels, LABEL_DTYPE, in order, peak = the index).  No GPU."""
    xs = np.ascontiguousarray(x, dtype=np.uint32).reshape(-1)
    ws = np.ascontiguousarray(widths, dtype=np.float32).reshape(-1)
    if len(xs) != len(ws):
        raise ValueError("x and widths differ in length")
    rows, out = np.zeros(len(xs), np.int32), np.zeros(len(xs), LABEL_DTYPE)
    ptr = lambda a: _p(a) if a.size else None
    n = lib().topo_label_layout(len(xs), ptr(xs), ptr(ws), image_width, row_height, max_rows, ptr(rows), ptr(out))
    if n < 0:
        raise TopoError(n, "topo_label_layout: bad arguments" if n == TOPO_ERR_INVALID else "topo_label_layout: grid too large (max_rows <= 64, columns x max_rows <= 524288)")
    return rows, out[:n]


def post_uniforms(width, height, pixelize_n=100.0) -> np.ndarray:
    """PostprocessingUniforms::new (render/data.rs:82-89)."""
    return np.array([width, height, pixelize_n, 0.0], dtype=np.float32)


def sector_fov_y(sector_w: int, sector_h: int, n_sectors: int = N_SECTORS) -> float:
    """Vertical FOV that gives each sector a horizontal FOV of 360/n degrees."""
    return 2.0 * math.atan(math.tan(math.pi / n_sectors) * sector_h / sector_w)


def panorama_uniforms(eye, yaw0, sector_w, sector_h, sun_theta_deg, sun_phi_deg, view_mode=0,
                      n_sectors: int = N_SECTORS, pitch: float = 0.0):
    """The n_sectors reference cameras of a 360-degree strip.  The reference's yaw grows counter-clockwise seen
    from above (Camera::direction, camera.rs:101-109), so sector k looks at yaw0 - k*(360/n) degrees: the strip then
    reads left to right, each sector's right edge meeting the next one's left edge."""
    out = np.zeros((n_sectors, 40), dtype=np.float32)
    e = np.ascontiguousarray(eye, dtype=np.float32)
    lib().topo_panorama_uniforms(_p(e), yaw0, pitch, sector_w, sector_h, sun_theta_deg, sun_phi_deg, view_mode, n_sectors, _p(out))
    return [out[k].copy() for k in range(n_sectors)]


# ---- multi-GPU communicator (topo_comm_*: RCCL behind the C ABI) ---------------------------------------

def comm_unique_id() -> np.ndarray:
    """128 bytes from rank 0 (ncclGetUniqueId) for the host to hand to the other ranks."""
    out = np.zeros(128, np.uint8)
    rc = lib().topo_comm_unique_id(_p(out))
    if rc != TOPO_OK:
        raise TopoError(rc, lib().topo_last_error(None).decode())
    return out


class Comm:
    """topo_comm: this process's place in a group of one-process-per-GPU renderers.  world == 1 needs no RCCL."""

    def __init__(self, rank: int = 0, world: int = 1, unique_id=None, device: int = 0, nccl_comm: int = 0):
        h = C.c_void_p()
        if nccl_comm:
            rc = lib().topo_comm_from_nccl(C.byref(h), C.c_void_p(nccl_comm), rank, world)
        else:
            uid = None if unique_id is None else np.ascontiguousarray(unique_id, dtype=np.uint8)
            rc = lib().topo_comm_init(C.byref(h), device, None if uid is None else _p(uid), rank, world)
        if rc != TOPO_OK:
            raise TopoError(rc, lib().topo_last_error(None).decode())
        self._h, self.rank, self.world = h, rank, world

    def close(self):
        if getattr(self, "_h", None):
            lib().topo_comm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def panorama_slots(world: int, sector_w: int, sector_h: int):
    """The resolve / exchange slots of one panorama (topo_panorama_slots): [(sector within the rank's range, row0, rows)]."""
    n = lib().topo_panorama_slots(world, sector_w, sector_h, None, 0)
    out = np.zeros((max(1, n), 3), np.uint32)
    lib().topo_panorama_slots(world, sector_w, sector_h, _p(out), n)
    return [tuple(int(v) for v in row) for row in out[:n]]


def panorama_sector_range(rank: int, world: int):
    a, b = C.c_uint32(), C.c_uint32()
    lib().topo_panorama_sector_range(rank, world, C.byref(a), C.byref(b))
    return range(a.value, a.value + b.value)


# ---- the TerrainRenderer mirror ------------------------------------------------------------------------

class TerrainRenderer:
    """Mirror of the reference's TerrainRenderer (terrain_renderer.rs) on one MI355X."""

    def __init__(self, width: int, height: int, device: int = 0, color_format: int = FORMAT_RGBA8_UNORM_SRGB):
        h = C.c_void_p()
        rc = lib().topo_create(C.byref(h), device, width, height, color_format)
        if rc != TOPO_OK:
            raise TopoError(rc, lib().topo_last_error(None).decode())
        self._h = h
        self.size = (width, height)
        self.tile_size = None

    def close(self):
        if getattr(self, "_h", None):
            lib().topo_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != TOPO_OK:
            raise TopoError(rc, lib().topo_last_error(self._h).decode())

    # add_terrain(location, height_map_data, coordinate_transform, size)   terrain_renderer.rs:173-182
    def add_terrain(self, lat_deg, lon_deg, heights, raster_point, model_point, pixel_scale):
        hts = np.ascontiguousarray(heights, dtype=np.float32)
        h, w = hts.shape
        rp, mp, ps = (np.ascontiguousarray(a, dtype=np.float32) for a in (raster_point, model_point, pixel_scale))
        self._check(lib().topo_add_terrain(self._h, lat_deg, lon_deg, _p(hts), w, h, _p(rp), _p(mp), _p(ps)))
        self.tile_size = (w, h)

    def add_terrain_device(self, lat_deg, lon_deg, heights_ptr: int, w, h, raster_point, model_point, pixel_scale):
        rp, mp, ps = (np.ascontiguousarray(a, dtype=np.float32) for a in (raster_point, model_point, pixel_scale))
        self._check(lib().topo_add_terrain_device(self._h, lat_deg, lon_deg, C.c_void_p(heights_ptr), w, h, _p(rp), _p(mp), _p(ps)))
        self.tile_size = (w, h)

    def unload_terrain(self, lat_deg, lon_deg):
        self._check(lib().topo_unload_terrain(self._h, lat_deg, lon_deg))

    # update(target_size, &uniforms, &postprocessing_uniforms)              terrain_renderer.rs:151-158
    def update(self, width, height, uniforms: np.ndarray, post: np.ndarray):
        u = np.ascontiguousarray(uniforms).view(np.uint8)
        pu = np.ascontiguousarray(post, dtype=np.float32)
        if u.nbytes != 160 or pu.nbytes != 16:
            raise ValueError("uniforms must be 160 bytes and post uniforms 16 bytes")
        self._check(lib().topo_update(self._h, width, height, _p(u), _p(pu)))
        self.size = (width, height)

    # render(...) + depth read-back with the reference's pad_256 row pitch    terrain_renderer.rs:365, render_engine.rs:219-249
    def render(self, want_depth=True, padded_depth=False):
        w, h = self.size
        rgba = np.empty((h, w, 4), np.uint8)
        if not want_depth:
            self._check(lib().topo_render(self._h, _p(rgba), w * 4, None, 0))
            return rgba, None
        pitch = pad_256(4 * w) if padded_depth else 4 * w
        depth = np.zeros((h, pitch // 4), np.float32)
        self._check(lib().topo_render(self._h, _p(rgba), w * 4, _p(depth), pitch))
        return rgba, (depth if padded_depth else depth[:, :w])

    def render_into(self, rgba: np.ndarray, depth: np.ndarray = None):
        """topo_render into caller-owned arrays (rgba (h, w, 4) u8; depth (h, pitch / 4) f32 or None) -- the arrays a caller
        reuses frame after frame and may have pinned (pin_host_buffer)."""
        self._check(lib().topo_render(self._h, _p(rgba), rgba.strides[0], _p(depth) if depth is not None else None,
                                      depth.strides[0] if depth is not None else 0))

    def pin_host_buffer(self, a: np.ndarray):
        self._check(lib().topo_pin_host_buffer(self._h, _p(a), a.nbytes))

    def unpin_host_buffer(self, a: np.ndarray):
        self._check(lib().topo_unpin_host_buffer(self._h, _p(a)))

    def decode_geotiff(self, data: bytes) -> np.ndarray:
        """The f32 raster of a GeoTIFF's first image (topo_geotiff_decode: host container work, GPU predictor/layout)."""
        w, h, _ = geotiff_info(data)
        buf = np.frombuffer(data, np.uint8)
        out = np.empty((h, w), np.float32)
        self._check(lib().topo_geotiff_decode(self._h, _p(buf), buf.size, _p(out), out.size))
        return out

    def add_terrain_geotiff(self, lat_deg: int, lon_deg: int, data: bytes):
        buf = np.frombuffer(data, np.uint8)
        self._check(lib().topo_add_terrain_geotiff(self._h, lat_deg, lon_deg, _p(buf), buf.size))
        w, h, _ = geotiff_info(data)
        self.tile_size = (w, h)

    def render_device(self, rgba_ptr: int, rgba_pitch: int, depth_ptr: int = 0, depth_pitch: int = 0):
        """topo_render_device: the frame of the last update() into device buffers."""
        self._check(lib().topo_render_device(self._h, C.c_void_p(rgba_ptr), rgba_pitch, C.c_void_p(depth_ptr) if depth_ptr else None, depth_pitch))

    def recompute_normals(self):
        self._check(lib().topo_recompute_normals(self._h))

    # LineRenderer::render (line_renderer.rs:200-212): overlay triangles over an image of this renderer's size and format
    def overlay_lines(self, vertices, indices, rgba: np.ndarray, line_width: float = 0.5) -> np.ndarray:
        """vertices: (n, 8) 4-byte words / structured array of 32-byte GpuVertex records; indices u32; rgba (h, w, 4) u8, in place."""
        v = np.ascontiguousarray(vertices)
        ix = np.ascontiguousarray(indices, dtype=np.uint32)
        assert rgba.dtype == np.uint8 and rgba.flags.c_contiguous
        self._check(lib().topo_overlay_lines(self._h, _p(v), v.nbytes // 32, _p(ix), ix.size, line_width, _p(rgba), rgba.strides[0]))
        return rgba

    def overlay_lines_device(self, vertices, indices, rgba_ptr: int, rgba_pitch: int, line_width: float = 0.5):
        v = np.ascontiguousarray(vertices)
        ix = np.ascontiguousarray(indices, dtype=np.uint32)
        self._check(lib().topo_overlay_lines_device(self._h, _p(v), v.nbytes // 32, _p(ix), ix.size, line_width, C.c_void_p(rgba_ptr), rgba_pitch))

    def overlay_glyphs(self, glyphs, atlas: np.ndarray, rgba: np.ndarray, depth: float = 100.0 / 4096.0) -> np.ndarray:
        """glyphs: structured array / (n, 7) words of 28-byte GlyphToRender records; atlas (ah, aw) u8 mask; rgba (h, w, 4) u8, in place."""
        g = np.ascontiguousarray(glyphs)
        a = np.ascontiguousarray(atlas, dtype=np.uint8)
        assert rgba.dtype == np.uint8 and rgba.flags.c_contiguous
        self._check(lib().topo_overlay_glyphs(self._h, _p(g), g.nbytes // 28, depth, _p(a), a.shape[1], a.shape[0], _p(rgba), rgba.strides[0]))
        return rgba

    def overlay_glyphs_device(self, glyphs, atlas: np.ndarray, rgba_ptr: int, rgba_pitch: int, depth: float = 100.0 / 4096.0):
        g = np.ascontiguousarray(glyphs)
        a = np.ascontiguousarray(atlas, dtype=np.uint8)
        self._check(lib().topo_overlay_glyphs_device(self._h, _p(g), g.nbytes // 28, depth, _p(a), a.shape[1], a.shape[0], C.c_void_p(rgba_ptr), rgba_pitch))

    def change_location(self, latitude: float, longitude: float, range_dist: float = 100_000.0):
        """UiController::change_location on this renderer's tile set: unloads what left the range, returns (tiles to fetch, n unloaded)."""
        rq = np.zeros((4096, 2), np.int32)
        nr, nu = C.c_uint32(), C.c_uint32()
        self._check(lib().topo_change_location(self._h, latitude, longitude, range_dist, _p(rq), 4096, C.byref(nr), C.byref(nu)))
        return [(int(a), int(b)) for a, b in rq[:nr.value]], int(nu.value)

    def render_panorama(self, comm, eye, yaw0, sector_w, sector_h, sun_theta_deg, sun_phi_deg, strip_ptr: int, depth_ptr: int = 0,
                        view_mode: int = 0, pitch: float = 0.0):
        """topo_render_panorama: this rank's sectors into the sector-major strip [8][sector_h][sector_w][4] (+ depth), then the
        in-place RCCL all-gather (comm None / world 1: all 8 sectors, no collective).  Asynchronous on the context's stream."""
        e = np.ascontiguousarray(eye, dtype=np.float32)
        self._check(lib().topo_render_panorama(self._h, comm._h if comm is not None else None, _p(e), yaw0, pitch, sector_w, sector_h,
                                               sun_theta_deg, sun_phi_deg, view_mode, C.c_void_p(strip_ptr),
                                               C.c_void_p(depth_ptr) if depth_ptr else None))

    def render_batch(self, eyes, yaw0s, suns_theta_phi_deg, sector_w, sector_h, rgba_ptr: int, depth_ptr: int = 0, view_mode: int = 0,
                     pitch: float = 0.0):
        """topo_render_batch: n independent panoramas (eyes (n,3), yaw0s (n,), suns (n,2) degrees) into rgba [n][8][h][w][4]."""
        e = np.ascontiguousarray(eyes, dtype=np.float32).reshape(-1, 3)
        y = np.ascontiguousarray(yaw0s, dtype=np.float32).reshape(-1)
        sn = np.ascontiguousarray(suns_theta_phi_deg, dtype=np.float32).reshape(-1, 2)
        assert len(e) == len(y) == len(sn)
        self._check(lib().topo_render_batch(self._h, len(e), _p(e), _p(y), _p(sn), pitch, sector_w, sector_h, view_mode,
                                            C.c_void_p(rgba_ptr), C.c_void_p(depth_ptr) if depth_ptr else None))

    def render_views_device(self, uniforms_list, width, height, rgba_ptr: int, rgba_view_stride: int, rgba_pitch: int,
                            depth_ptr: int = 0, depth_view_stride: int = 0, depth_pitch: int = 0):
        if isinstance(uniforms_list, np.ndarray) and uniforms_list.dtype == np.uint8 and uniforms_list.ndim == 2:
            us = np.ascontiguousarray(uniforms_list)           # already packed: (n_views, 160) bytes
            assert us.shape[1] == 160
        else:
            us = np.ascontiguousarray(np.stack([np.ascontiguousarray(u).view(np.uint8).reshape(160) for u in uniforms_list]))
        self._check(lib().topo_render_views_device(self._h, len(us), _p(us), width, height,
                                                   C.c_void_p(rgba_ptr), rgba_view_stride, rgba_pitch,
                                                   C.c_void_p(depth_ptr) if depth_ptr else None, depth_view_stride, depth_pitch))

    def set_stream(self, hip_stream: int):
        self._check(lib().topo_set_stream(self._h, C.c_void_p(hip_stream) if hip_stream else None))

    def set_pipeline_depth(self, depth: int):
        """Frames in flight for render_views_device (topo_set_pipeline_depth); outputs are complete after join()."""
        self._check(lib().topo_set_pipeline_depth(self._h, depth))

    def join(self):
        self._check(lib().topo_join(self._h))

    def synchronize(self):
        self._check(lib().topo_synchronize(self._h))

    def frame_status(self) -> dict:
        """Status of the last frame waited for (topo_frame_status): bits + the bounds record of the check build."""
        out = np.zeros(4, np.uint32)
        self._check(lib().topo_frame_status(self._h, _p(out)))
        return {"status": int(out[0]), "big_overflow": bool(out[0] & 1), "rare_overflow": bool(out[0] & 2), "bounds_violation": bool(out[0] & 4),
                "bounds_site": int(out[1]), "bounds_value": int(out[2]) | (int(out[3]) << 32)}

    def set_normals_lds_rows(self, rows: int):
        self._check(lib().topo_set_normals_lds_rows(self._h, rows))

    def debug_set_queue_caps(self, big_cap: int, rare_cap: int):
        self._check(lib().topo_debug_set_queue_caps(self._h, big_cap, rare_cap))

    def debug_far_phase_launched(self) -> bool:
        """Whether the last submission launched its far phase (include/topo_hip_test.h)."""
        out = np.zeros(1, np.int32)
        self._check(lib().topo_debug_far_phase_launched(self._h, _p(out)))
        return bool(out[0])

    def debug_set_tile_prefilter(self, on: bool):
        """The cull's host-side tile prefilter on / off, from the next submission on (include/topo_hip_test.h)."""
        self._check(lib().topo_debug_set_tile_prefilter(self._h, 1 if on else 0))

    def debug_cull_pairs(self) -> tuple:
        """(pairs launched, pairs in all) of the last submission's cull (include/topo_hip_test.h)."""
        out = np.zeros(2, np.uint32)
        self._check(lib().topo_debug_cull_pairs(self._h, _p(out)))
        return int(out[0]), int(out[1])

    def debug_cover_stats(self) -> dict:
        """The last frame's covered regions: covering items, claims won, claims lost (include/topo_hip_test.h)."""
        out = np.zeros(3, np.uint32)
        self._check(lib().topo_debug_cover_stats(self._h, _p(out)))
        return {"candidates": int(out[0]), "won": int(out[1]), "lost": int(out[2])}

    def debug_set_resolve_owned(self, on: bool):
        """k_resolve's owned-strip path on / off, from the next submission on (include/topo_hip_test.h)."""
        self._check(lib().topo_debug_set_resolve_owned(self._h, 1 if on else 0))

    def debug_owned_strips(self) -> dict:
        """The last frame's strips that pass k_resolve's ownership test, and its strips with a record of the frame (include/topo_hip_test.h)."""
        out = np.zeros(2, np.uint32)
        self._check(lib().topo_debug_owned_strips(self._h, _p(out)))
        return {"owned": int(out[0]), "marked": int(out[1])}

    def debug_read_cull_lists(self) -> dict:
        """What the last frame's cull and occlusion test decided (topo_debug_read_cull_lists, test hook; pipeline depth 1): the near
        work items and the far survivors as WORK_ITEM_DTYPE records, the far candidates as FAR_ITEM_DTYPE records, and the frame's
        far_tested / far_survived counters."""
        n = np.zeros(5, np.uint32)
        self._check(lib().topo_debug_read_cull_lists(self._h, None, 0, None, 0, None, 0, _p(n)))
        near, far, surv = np.zeros(int(n[0]), WORK_ITEM_DTYPE), np.zeros(int(n[1]), FAR_ITEM_DTYPE), np.zeros(int(n[2]), WORK_ITEM_DTYPE)
        self._check(lib().topo_debug_read_cull_lists(self._h, _p(near), near.size, _p(far), far.size, _p(surv), surv.size, _p(n)))
        assert (int(n[0]), int(n[1]), int(n[2])) == (near.size, far.size, surv.size)
        return {"near": near, "far": far, "survivors": surv, "far_tested": int(n[3]), "far_survived": int(n[4])}

    def timings(self) -> dict:
        out = np.zeros(TIMING_SLOTS, np.float32)
        self._check(lib().topo_get_timings(self._h, _p(out)))
        return {k: float(v) for k, v in zip(TIMING_NAMES, out) if k != "_"}

    def timing_history(self, n_frames: int) -> list:
        """Per-kernel durations of the last n_frames frames (at most 32 per frame in flight), oldest first; waits for them."""
        out, n = np.zeros((max(1, n_frames), 7), np.float32), C.c_uint32(0)
        self._check(lib().topo_get_timing_history(self._h, n_frames, _p(out), C.byref(n)))
        return [{k: float(v) for k, v in zip(TIMING_NAMES[:7], row)} for row in out[:n.value]]

    def counters(self) -> dict:
        out = np.zeros(6, np.uint32)
        self._check(lib().topo_get_counters(self._h, _p(out)))
        return {"blocks_rastered": int(out[0]) + int(out[5]), "big_items": int(out[1]), "status": int(out[2]), "rare_items": int(out[3]),
                "near_blocks": int(out[0]), "far_tested": int(out[4]), "far_survived": int(out[5])}   # near/survivors: in strips of 1 or 2 cell rows (terrain_renderer.cpp: near_strip)

    def set_timing_slots(self, names=None, total=True):
        """Measure only the named per-kernel durations (TIMING_NAMES[:6]); None = all, () = just the total; total=False: not
        even that (TOPO_TIMING_NO_TOTAL: no event in front of the frame)."""
        mask = 0x3F if names is None else sum(1 << TIMING_NAMES.index(n) for n in names)
        if not total:
            mask |= 0x80
        self._check(lib().topo_set_timing_slots(self._h, mask))

    def set_occlusion_split(self, metres: float):
        self._check(lib().topo_set_occlusion_split(self._h, metres))

    def read_tile_tables(self, lat_deg, lon_deg) -> dict:
        """The load-time tables of a tile (topo_read_tile_tables, test hook): block min/max, sin/cos tables, f64 cull bounds."""
        w, h = self.tile_size
        n = C.c_uint32(0)
        self._check(lib().topo_read_tile_tables(self._h, lat_deg, lon_deg, None, None, None, C.byref(n)))
        minmax, trig, bounds = np.empty((n.value, 2), np.float32), np.empty((w + h, 2), np.float32), np.empty(n.value * 18, np.float64)
        self._check(lib().topo_read_tile_tables(self._h, lat_deg, lon_deg, _p(minmax), _p(trig), _p(bounds), C.byref(n)))
        return {"minmax": minmax, "trig": trig, "bounds": bounds}

    def read_normals(self, lat_deg, lon_deg) -> np.ndarray:
        w, h = self.tile_size
        out = np.empty((h, w, 4), np.uint8)
        self._check(lib().topo_read_normals(self._h, lat_deg, lon_deg, _p(out)))
        return out

    # RenderEngine::get_visible_labels                                       render_engine.rs:338-396
    def visible_peaks(self, peaks_xyz: np.ndarray):
        """peaks (n,3) f32 ECEF -> (visible (n,) bool, xy (n,2) u32) against the depth of the last render()."""
        pk = np.ascontiguousarray(peaks_xyz, dtype=np.float32).reshape(-1, 3)
        n = pk.shape[0]
        vis = np.zeros(n, np.uint8)
        xy = np.zeros((n, 2), np.uint32)
        self._check(lib().topo_visible_peaks(self._h, n, _p(pk), _p(vis), _p(xy)))
        return vis.astype(bool), xy

    def visible_peaks_device(self, uniforms, width, height, depth_ptr, depth_pitch, n, peaks_ptr, visible_ptr, xy_ptr):
        u = np.ascontiguousarray(uniforms).view(np.uint8)
        self._check(lib().topo_visible_peaks_device(self._h, _p(u), width, height, C.c_void_p(depth_ptr), depth_pitch, n,
                                                    C.c_void_p(peaks_ptr), C.c_void_p(visible_ptr), C.c_void_p(xy_ptr)))

    # peak labels: the peaks depth images show, laid out in rows, per image of views_per_image views (include/topo_hip.h)
    def labels_device(self, params, uniforms_list, width: int, height: int, depth_ptr: int, n_peaks: int, peaks_ptr: int, widths_ptr: int, labels_ptr: int,
                      counts_ptr: int, state_ptr: int = 0, depth_view_stride: int = None, depth_pitch: int = None):
        """topo_labels_device: the views (uniforms_list: their 160-byte uniforms, or packed (n, 160) bytes) whose depth is at depth_ptr
        (defaults: densely packed) -> per image of params["views_per_image"] views its first params["cap"] labels (LABEL_DTYPE) at
        labels_ptr + image * cap, the number placed at counts_ptr + 4 * image and, if wanted, the state bytes at state_ptr + image *
        n_peaks + peak; everything device memory; queued on the context's stream."""
        p, us = self._label_args(params, uniforms_list)
        ptr = lambda v: C.c_void_p(v) if v else None
        dp = 4 * width if depth_pitch is None else depth_pitch
        self._check(lib().topo_labels_device(self._h, _p(p), len(us), _p(us) if len(us) else None, width, height, ptr(depth_ptr),
                                             dp * height if depth_view_stride is None else depth_view_stride, dp, n_peaks, ptr(peaks_ptr), ptr(widths_ptr),
                                             ptr(labels_ptr), ptr(counts_ptr), ptr(state_ptr)))

    def labels_read(self, params, uniforms_list, width: int, height: int, depth_ptr: int, peaks_xyz, widths, depth_view_stride: int = None, depth_pitch: int = None):
        """topo_labels_read: peaks (n, 3) f32 and widths (n,) f32 from the host against the depth at depth_ptr (device memory) ->
        ((images, cap) LABEL_DTYPE, zero behind each image's labels; (images,) uint32 counts; (images, n) uint8 states); waits."""
        p, us = self._label_args(params, uniforms_list)
        pk = np.ascontiguousarray(peaks_xyz, dtype=np.float32).reshape(-1, 3)
        ws = np.ascontiguousarray(widths, dtype=np.float32).reshape(-1)
        if len(pk) != len(ws):
            raise ValueError("peaks and widths differ in length")
        vpi, cap = int(p["views_per_image"][0]), int(p["cap"][0])
        images = len(us) // vpi if vpi else 0
        labels, counts, state = np.zeros((images, cap), LABEL_DTYPE), np.zeros(images, np.uint32), np.zeros((images, len(pk)), np.uint8)
        ptr = lambda a: _p(a) if a.size else None
        dp = 4 * width if depth_pitch is None else depth_pitch
        self._check(lib().topo_labels_read(self._h, _p(p), len(us), _p(us) if len(us) else None, width, height, C.c_void_p(depth_ptr) if depth_ptr else None,
                                           dp * height if depth_view_stride is None else depth_view_stride, dp, len(pk), ptr(pk), ptr(ws), ptr(labels),
                                           _p(counts) if images else _p(np.zeros(1, np.uint32)), ptr(state)))
        return labels, counts, state

    @staticmethod
    def _label_args(params, uniforms_list):
        p = np.ascontiguousarray(params, dtype=LABEL_PARAMS_DTYPE).reshape(-1)[:1]
        if isinstance(uniforms_list, np.ndarray) and uniforms_list.dtype == np.uint8 and uniforms_list.ndim == 2:
            us = np.ascontiguousarray(uniforms_list)
            assert us.shape[1] == 160
        elif len(uniforms_list) == 0:
            us = np.zeros((0, 160), np.uint8)
        else:
            us = np.ascontiguousarray(np.stack([np.ascontiguousarray(u).view(np.uint8).reshape(160) for u in uniforms_list]))
        return p, us

    # viewshed: the DEM cells the frames rendered while accumulation is on show (include/topo_hip.h)
    def viewshed_enable(self, on: bool = True):
        """Every later frame ORs the cells that won >= 1 pixel into per-tile masks (on), or stops doing so (the masks stay)."""
        self._check(lib().topo_viewshed_enable(self._h, 1 if on else 0))

    def viewshed_reset(self):
        self._check(lib().topo_viewshed_reset(self._h))

    def viewshed(self, lat_deg, lon_deg) -> np.ndarray:
        """The tile's mask: (h-1, w-1) bool, cell (x, y) = the quad between texels (x, y) and (x+1, y+1), row 0 north."""
        if self.tile_size is None:
            raise TopoError(TOPO_ERR_NOT_FOUND, "no tile loaded")
        w, h = self.tile_size
        out = np.zeros((h - 1, w - 1), np.uint8)
        n = C.c_uint64(0)
        self._check(lib().topo_viewshed_read(self._h, lat_deg, lon_deg, _p(out), w - 1, C.byref(n)))
        if int(out.sum()) != n.value:
            raise TopoError(TOPO_ERR_INVALID, f"viewshed count {n.value} differs from the mask's {int(out.sum())} cells")
        return out.astype(bool)

    def debug_viewshed_stats(self) -> dict:
        """What k_viewshed did since the masks were made or last reset (include/topo_hip_test.h)."""
        out = np.zeros(3, np.uint64)
        self._check(lib().topo_debug_viewshed_stats(self._h, _p(out)))
        return {"terrain_keys": int(out[0]), "updates": int(out[1]), "atomics": int(out[2])}

    # horizon: the topmost terrain pixel of every column of the latest submission (include/topo_hip.h)
    def horizon_shape(self):
        """(n_views, width, height) of the latest submission."""
        n, w, h = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._check(lib().topo_horizon_shape(self._h, C.byref(n), C.byref(w), C.byref(h)))
        return int(n.value), int(w.value), int(h.value)

    def horizon(self, first_view: int = 0, n_views: int = None) -> np.ndarray:
        """Views [first_view, first_view + n_views) of the latest submission as a structured array [n_views][width] of
        HORIZON_DTYPE; waits for the submission.  Raises TopoError(CAPACITY) if it overflowed its rare-triangle queue."""
        total, w, _ = self.horizon_shape()
        n = total - first_view if n_views is None else n_views
        out = np.zeros((max(n, 0), w), HORIZON_DTYPE)
        self._check(lib().topo_horizon_read(self._h, first_view, n, _p(out) if out.size else None, w))
        return out

    def horizon_device(self, out_ptr: int, first_view: int = 0, n_views: int = None, view_stride: int = None):
        """topo_horizon_device: records into device memory (view i at out_ptr + 32 * i * view_stride), queued behind the latest
        submission on its stream."""
        total, w, _ = self.horizon_shape()
        n = total - first_view if n_views is None else n_views
        self._check(lib().topo_horizon_device(self._h, first_view, n, C.c_void_p(out_ptr), w if view_stride is None else view_stride))

    # ground: the terrain point under pixels of the latest submission (include/topo_hip.h)
    def ground(self, queries) -> np.ndarray:
        """topo_ground_read.  queries: GROUND_QUERY_DTYPE records, or an (n, 3) integer array of (view, x, y); returns n
        GROUND_DTYPE records (f64 longitude / latitude); waits for the submission.  Raises TopoError(INVALID) for a query outside
        it, TopoError(CAPACITY) if it overflowed its rare-triangle queue."""
        q = ground_queries(queries)
        out = np.zeros(len(q), GROUND_DTYPE)
        self._check(lib().topo_ground_read(self._h, len(q), _p(q) if len(q) else None, _p(out) if len(q) else None))
        return out

    def ground_device(self, queries_ptr: int, out_ptr: int, n: int):
        """topo_ground_device: n topo_ground_query at queries_ptr -> n topo_ground_point at out_ptr (device memory, 16-byte
        aligned), queued behind the latest submission on its stream."""
        self._check(lib().topo_ground_device(self._h, n, C.c_void_p(queries_ptr), C.c_void_p(out_ptr)))

    def ground_map_device(self, out_ptr: int, first_view: int = 0, n_views: int = None, view_stride_bytes: int = None, pitch_bytes: int = None):
        """topo_ground_map_device: float4 (lon, lat, height, range) for every pixel of the views, NaN where there is no terrain
        point; view i at out_ptr + i * view_stride_bytes, rows pitch_bytes apart (defaults: densely packed)."""
        total, w, h = self.horizon_shape()
        n = total - first_view if n_views is None else n_views
        pitch = 16 * w if pitch_bytes is None else pitch_bytes
        stride = pitch * h if view_stride_bytes is None else view_stride_bytes
        self._check(lib().topo_ground_map_device(self._h, first_view, n, C.c_void_p(out_ptr), stride, pitch))

    # rays against the resident tiles (include/topo_hip.h); no submission needed
    def raycast(self, ray_records) -> np.ndarray:
        """topo_raycast_read: RAY_DTYPE records (see rays()) -> RAY_HIT_DTYPE records; waits."""
        r = np.ascontiguousarray(ray_records, dtype=RAY_DTYPE).reshape(-1)
        out = np.zeros(len(r), RAY_HIT_DTYPE)
        self._check(lib().topo_raycast_read(self._h, len(r), _p(r) if len(r) else None, _p(out) if len(r) else None))
        return out

    def raycast_device(self, rays_ptr: int, out_ptr: int, n: int):
        """topo_raycast_device: n topo_ray at rays_ptr -> n topo_ray_hit at out_ptr (device memory, 16-byte aligned), queued on
        the context's stream."""
        self._check(lib().topo_raycast_device(self._h, n, C.c_void_p(rays_ptr) if rays_ptr else None, C.c_void_p(out_ptr) if out_ptr else None))

    def sunlit_map_device(self, sun_dir, out_ptr: int, first_view: int = 0, n_views: int = None, view_stride_bytes: int = None, pitch_bytes: int = None):
        """topo_sunlit_map_device: one byte (SUN_NONE / SUN_LIT / SUN_AWAY / SUN_SHADOW) for every pixel of the views of the latest
        submission under a sun in direction sun_dir (f64, towards the sun; see sun_direction); view i at out_ptr + i *
        view_stride_bytes, rows pitch_bytes apart (defaults: densely packed)."""
        total, w, h = self.horizon_shape()
        n = total - first_view if n_views is None else n_views
        pitch = w if pitch_bytes is None else pitch_bytes
        stride = pitch * h if view_stride_bytes is None else view_stride_bytes
        sun = np.ascontiguousarray(sun_dir, dtype=np.float64).reshape(3)
        self._check(lib().topo_sunlit_map_device(self._h, first_view, n, _p(sun), C.c_void_p(out_ptr) if out_ptr else None, stride, pitch))

    # surface: the drawn terrain under a longitude and latitude (include/topo_hip.h); no submission needed
    def surface(self, lonlat) -> np.ndarray:
        """topo_surface_read: (n, 2) f64 (longitude, latitude) in degrees -> SURFACE_DTYPE records; waits."""
        p = np.ascontiguousarray(lonlat, dtype=np.float64).reshape(-1, 2)
        out = np.zeros(len(p), SURFACE_DTYPE)
        self._check(lib().topo_surface_read(self._h, len(p), _p(p) if len(p) else None, _p(out) if len(p) else None))
        return out

    def surface_device(self, lonlat_ptr: int, out_ptr: int, n: int):
        """topo_surface_device: n (lon, lat) f64 pairs at lonlat_ptr -> n topo_surface_point at out_ptr (device memory, 16-byte
        aligned), queued on the context's stream."""
        self._check(lib().topo_surface_device(self._h, n, C.c_void_p(lonlat_ptr) if lonlat_ptr else None, C.c_void_p(out_ptr) if out_ptr else None))

    def surface_grid_device(self, lon0: float, lat0: float, dlon: float, dlat: float, nx: int, ny: int, out_ptr: int, pitch_bytes: int = None):
        """topo_surface_grid_device: the f32 height at lon0 + c * dlon, lat0 + r * dlat for c < nx, r < ny at out_ptr + r * pitch_bytes +
        4 * c (device memory; default: densely packed), NaN where there is no terrain; queued on the context's stream."""
        self._check(lib().topo_surface_grid_device(self._h, lon0, lat0, dlon, dlat, nx, ny, C.c_void_p(out_ptr) if out_ptr else None,
                                                   4 * nx if pitch_bytes is None else pitch_bytes))

    # map view: relief, contours and the viewshed over a lon / lat grid (include/topo_hip.h); no submission needed
    def map(self, params, rgba: bool = True, flags: bool = True):
        """topo_map_read: MAP_PARAMS_DTYPE (see map_params) -> ((ny, nx, 4) u8 R G B A or None, (ny, nx) u8 MAP_FLAG_* or None); waits."""
        p = np.ascontiguousarray(params, dtype=MAP_PARAMS_DTYPE).reshape(-1)[:1]
        nx, ny = int(p["nx"][0]), int(p["ny"][0])
        img = np.zeros((ny, nx, 4), np.uint8) if rgba else None
        flg = np.zeros((ny, nx), np.uint8) if flags else None
        self._check(lib().topo_map_read(self._h, _p(p), _p(img) if rgba and img.size else None, _p(flg) if flags and flg.size else None))
        return img, flg

    def map_device(self, params, rgba=None, flags=None):
        """topo_map_device: rgba a (ny, >= nx, 4) and flags a (ny, >= nx) uint8 torch tensor on the device (either may be None), each with
        contiguous pixels and rows a stride apart; queued on the context's stream."""
        p = np.ascontiguousarray(params, dtype=MAP_PARAMS_DTYPE).reshape(-1)[:1]
        self.map_device_ptr(p, rgba.data_ptr() if rgba is not None else 0, rgba.stride(0) if rgba is not None else 0, flags.data_ptr() if flags is not None else 0,
                            flags.stride(0) if flags is not None else 0)

    def map_device_ptr(self, params, rgba_ptr: int, rgba_pitch: int, flags_ptr: int, flags_pitch: int):
        """topo_map_device on raw device pointers and pitches in bytes."""
        p = np.ascontiguousarray(params, dtype=MAP_PARAMS_DTYPE).reshape(-1)[:1]
        self._check(lib().topo_map_device(self._h, _p(p), C.c_void_p(rgba_ptr) if rgba_ptr else None, rgba_pitch, C.c_void_p(flags_ptr) if flags_ptr else None, flags_pitch))

    def profile(self, ray_records, m: int, samples: bool = True):
        """topo_profile_read: RAY_DTYPE segments (finite t_min, t_max) -> (PROFILE_SUMMARY_DTYPE records, (n, m, 2) f32 (terrain,
        line) samples or None); waits."""
        r = np.ascontiguousarray(ray_records, dtype=RAY_DTYPE).reshape(-1)
        summary = np.zeros(len(r), PROFILE_SUMMARY_DTYPE)
        smp = np.zeros((len(r), m, 2), np.float32) if samples else None
        self._check(lib().topo_profile_read(self._h, len(r), _p(r) if len(r) else None, m, _p(smp) if samples and len(r) else None, _p(summary) if len(r) else None))
        return summary, smp

    def profile_device(self, segs_ptr: int, n: int, m: int, summary_ptr: int, samples_ptr: int = 0, segment_stride_bytes: int = None):
        """topo_profile_device: n topo_ray at segs_ptr -> n topo_profile_summary at summary_ptr and, unless samples_ptr is 0, m
        (terrain, line) f32 pairs per segment at samples_ptr + i * segment_stride_bytes (default 8 * m); queued on the context's stream."""
        self._check(lib().topo_profile_device(self._h, n, C.c_void_p(segs_ptr) if segs_ptr else None, m, C.c_void_p(samples_ptr) if samples_ptr else None,
                                              8 * m if segment_stride_bytes is None else segment_stride_bytes, C.c_void_p(summary_ptr) if summary_ptr else None))

    # visibility: what observers see of the drawn terrain (include/topo_hip.h); no submission needed
    def visibility_grid_device(self, obs, lon0: float, lat0: float, dlon: float, dlat: float, nx: int, ny: int, out_ptr: int, target_height_m: float = 0.0,
                               layer_stride_bytes: int = None, pitch_bytes: int = None):
        """topo_visibility_grid_device: one byte (VIS_*) per (observer o, row r, column c) at out_ptr + o * layer_stride_bytes + r *
        pitch_bytes + c for the target at lon0 + c * dlon, lat0 + r * dlat (device memory; defaults: densely packed); obs:
        OBSERVER_DTYPE records (see observers()); queued on the context's stream."""
        o = np.ascontiguousarray(obs, dtype=OBSERVER_DTYPE).reshape(-1)
        pitch = nx if pitch_bytes is None else pitch_bytes
        stride = pitch * ny if layer_stride_bytes is None else layer_stride_bytes
        self._check(lib().topo_visibility_grid_device(self._h, len(o), _p(o) if len(o) else None, lon0, lat0, dlon, dlat, nx, ny, target_height_m,
                                                      C.c_void_p(out_ptr) if out_ptr else None, stride, pitch))

    def visibility_device(self, obs, lonlat_ptr: int, n: int, out_ptr: int, target_height_m: float = 0.0, list_stride_bytes: int = None):
        """topo_visibility_device: n (lon, lat) f64 pairs at lonlat_ptr (device memory, 16-byte aligned) -> one byte (VIS_*) per
        (observer o, entry i) at out_ptr + o * list_stride_bytes + i (default stride n); queued on the context's stream."""
        o = np.ascontiguousarray(obs, dtype=OBSERVER_DTYPE).reshape(-1)
        self._check(lib().topo_visibility_device(self._h, len(o), _p(o) if len(o) else None, n, C.c_void_p(lonlat_ptr) if lonlat_ptr else None, target_height_m,
                                                 C.c_void_p(out_ptr) if out_ptr else None, n if list_stride_bytes is None else list_stride_bytes))

    def visibility(self, obs, lonlat, target_height_m: float = 0.0) -> np.ndarray:
        """topo_visibility_read: OBSERVER_DTYPE records and (n, 2) f64 (longitude, latitude) in degrees -> (observers, n) uint8 classes
        (VIS_*); waits."""
        o = np.ascontiguousarray(obs, dtype=OBSERVER_DTYPE).reshape(-1)
        p = np.ascontiguousarray(lonlat, dtype=np.float64).reshape(-1, 2)
        out = np.zeros((len(o), len(p)), np.uint8)
        self._check(lib().topo_visibility_read(self._h, len(o), _p(o) if len(o) else None, len(p), _p(p) if len(p) else None, target_height_m,
                                               _p(out) if out.size else None))
        return out

    # refracted visibility: the same three calls along sight lines bent by refraction coefficient k (include/topo_hip.h)
    def visibility_refracted_grid_device(self, obs, lon0: float, lat0: float, dlon: float, dlat: float, nx: int, ny: int, out_ptr: int, target_height_m: float = 0.0,
                                         refraction_k: float = REFRACTION_STANDARD, layer_stride_bytes: int = None, pitch_bytes: int = None):
        """topo_visibility_refracted_grid_device: visibility_grid_device's bytes on the mesh lifted for each observer with
        refraction_k (0 <= k < 1; 0 gives visibility_grid_device's bytes); queued on the context's stream."""
        o = np.ascontiguousarray(obs, dtype=OBSERVER_DTYPE).reshape(-1)
        pitch = nx if pitch_bytes is None else pitch_bytes
        stride = pitch * ny if layer_stride_bytes is None else layer_stride_bytes
        self._check(lib().topo_visibility_refracted_grid_device(self._h, len(o), _p(o) if len(o) else None, lon0, lat0, dlon, dlat, nx, ny, target_height_m, refraction_k,
                                                                C.c_void_p(out_ptr) if out_ptr else None, stride, pitch))

    def visibility_refracted_device(self, obs, lonlat_ptr: int, n: int, out_ptr: int, target_height_m: float = 0.0, refraction_k: float = REFRACTION_STANDARD,
                                    list_stride_bytes: int = None):
        """topo_visibility_refracted_device: visibility_device's bytes under refraction_k; queued on the context's stream."""
        o = np.ascontiguousarray(obs, dtype=OBSERVER_DTYPE).reshape(-1)
        self._check(lib().topo_visibility_refracted_device(self._h, len(o), _p(o) if len(o) else None, n, C.c_void_p(lonlat_ptr) if lonlat_ptr else None, target_height_m,
                                                           refraction_k, C.c_void_p(out_ptr) if out_ptr else None, n if list_stride_bytes is None else list_stride_bytes))

    def visibility_refracted(self, obs, lonlat, target_height_m: float = 0.0, refraction_k: float = REFRACTION_STANDARD) -> np.ndarray:
        """topo_visibility_refracted_read: as visibility(), under refraction_k -> (observers, n) uint8 classes (VIS_*); waits."""
        o = np.ascontiguousarray(obs, dtype=OBSERVER_DTYPE).reshape(-1)
        p = np.ascontiguousarray(lonlat, dtype=np.float64).reshape(-1, 2)
        out = np.zeros((len(o), len(p)), np.uint8)
        self._check(lib().topo_visibility_refracted_read(self._h, len(o), _p(o) if len(o) else None, len(p), _p(p) if len(p) else None, target_height_m, refraction_k,
                                                         _p(out) if out.size else None))
        return out

    # skyline: the terrain horizon by azimuth from observers (include/topo_hip.h); no submission needed
    def skyline_device(self, obs, az0_deg: float, daz_deg: float, n_az: int, elevation_ptr: int = 0, samples_ptr: int = 0, min_range_m: float = 1.0,
                       max_range_m: float = 1.0e6, observer_stride_bytes: int = None, samples_stride_bytes: int = None):
        """topo_skyline_device: for azimuth az0 + k * daz (degrees, clockwise from north) of observer o, the f32 elevation at
        elevation_ptr + o * observer_stride_bytes + 4 * k and / or the SKYLINE_DTYPE record at samples_ptr + o * samples_stride_bytes +
        64 * k (device memory, 0: not wanted; defaults: densely packed); obs: OBSERVER_DTYPE records (see observers()); queued on the
        context's stream."""
        o = np.ascontiguousarray(obs, dtype=OBSERVER_DTYPE).reshape(-1)
        self._check(lib().topo_skyline_device(self._h, len(o), _p(o) if len(o) else None, az0_deg, daz_deg, n_az, min_range_m, max_range_m,
                                              C.c_void_p(elevation_ptr) if elevation_ptr else None, 4 * n_az if observer_stride_bytes is None else observer_stride_bytes,
                                              C.c_void_p(samples_ptr) if samples_ptr else None, 64 * n_az if samples_stride_bytes is None else samples_stride_bytes))

    def skyline(self, obs, az0_deg: float, daz_deg: float, n_az: int, min_range_m: float = 1.0, max_range_m: float = 1.0e6, elevation: bool = True,
                samples: bool = True):
        """topo_skyline_read: OBSERVER_DTYPE records -> ((observers, n_az) f32 elevations in degrees, NaN where there is no terrain
        in range or no observer; (observers, n_az) SKYLINE_DTYPE records), None for an output not wanted; waits."""
        o = np.ascontiguousarray(obs, dtype=OBSERVER_DTYPE).reshape(-1)
        el = np.full((len(o), n_az), np.nan, np.float32) if elevation else None
        rec = np.zeros((len(o), n_az), SKYLINE_DTYPE) if samples else None
        self._check(lib().topo_skyline_read(self._h, len(o), _p(o) if len(o) else None, az0_deg, daz_deg, n_az, min_range_m, max_range_m,
                                            _p(el) if el is not None and el.size else None, _p(rec) if rec is not None and rec.size else None))
        return el, rec

    # summits: the peaks of the drawn mesh by isolation, and snapping peaks to them (include/topo_hip.h); no submission needed
    def summits_device(self, out_ptr: int, capacity: int, count_ptr: int, radius_m: float, min_isolation_m: float = 0.0, min_height_m: float = -np.inf,
                       order: int = SUMMIT_ORDER_TILE):
        """topo_summits_device: the first min(count, capacity) SUMMIT_DTYPE records in tile order at out_ptr and the uint32 count at
        count_ptr (device memory); queued on the context's stream."""
        p = summit_params(radius_m, min_isolation_m, min_height_m, order)
        self._check(lib().topo_summits_device(self._h, _p(p), C.c_void_p(out_ptr) if out_ptr else None, capacity, C.c_void_p(count_ptr) if count_ptr else None))

    def summits(self, radius_m: float, min_isolation_m: float = 0.0, min_height_m: float = -np.inf, order: int = SUMMIT_ORDER_TILE, capacity: int = None):
        """topo_summits_read -> (SUMMIT_DTYPE records in `order`, the full count); waits.  capacity None: every summit (a second call
        sized by the first one's count when 65536 records do not hold them); else at most `capacity` records, and the count says
        whether there are more."""
        p = summit_params(radius_m, min_isolation_m, min_height_m, order)
        n = C.c_uint32(0)
        cap = 65536 if capacity is None else capacity
        out = np.zeros(cap, SUMMIT_DTYPE)
        rc = lib().topo_summits_read(self._h, _p(p), _p(out) if cap else None, cap, C.byref(n))
        if rc == TOPO_ERR_CAPACITY and capacity is None:
            cap = n.value
            out = np.zeros(cap, SUMMIT_DTYPE)
            rc = lib().topo_summits_read(self._h, _p(p), _p(out), cap, C.byref(n))
        if rc != TOPO_ERR_CAPACITY:
            self._check(rc)
        return out[:min(cap, n.value)], int(n.value)

    def summit_snap_device(self, lonlat_ptr: int, n: int, radius_m: float, out_ptr: int):
        """topo_summit_snap_device: n (lon, lat) pairs in degrees at lonlat_ptr -> n SUMMIT_SNAP_DTYPE records at out_ptr (device
        memory, 16-byte aligned); queued on the context's stream."""
        self._check(lib().topo_summit_snap_device(self._h, n, C.c_void_p(lonlat_ptr) if lonlat_ptr else None, radius_m, C.c_void_p(out_ptr) if out_ptr else None))

    def summit_snap(self, lonlat, radius_m: float):
        """topo_summit_snap_read: (n, 2) lon / lat degrees -> SUMMIT_SNAP_DTYPE records; waits."""
        p = np.ascontiguousarray(lonlat, dtype=np.float64).reshape(-1, 2)
        out = np.zeros(len(p), SUMMIT_SNAP_DTYPE)
        self._check(lib().topo_summit_snap_read(self._h, len(p), _p(p) if len(p) else None, radius_m, _p(out) if len(p) else None))
        return out

    def debug_set_summit_band_rows(self, rows: int):
        """Test hook: the band height of the summit calls in vertex rows; 0: the default."""
        self._check(lib().topo_debug_set_summit_band_rows(self._h, rows))

    def debug_summit_counts(self):
        """Test accessor: {"candidates", "summits"} of the last summit call; waits."""
        out = np.zeros(2, np.uint64)
        self._check(lib().topo_debug_summit_counts(self._h, _p(out)))
        return {"candidates": int(out[0]), "summits": int(out[1])}

    # sun exposure: a day of sun and shadow over points of the drawn terrain (include/topo_hip.h); no submission needed
    def sun_exposure_grid_device(self, suns, lon0: float, lat0: float, dlon: float, dlat: float, nx: int, ny: int, lit_ptr: int = 0, shadow_ptr: int = 0,
                                 exposure_ptr: int = 0, mask_pitch_bytes: int = None, exposure_pitch_bytes: int = None):
        """topo_sun_exposure_grid_device: for the target at lon0 + c * dlon, lat0 + r * dlat the uint64 masks (bit k: sun k LIT / in cast
        SHADOW) at lit_ptr / shadow_ptr + r * mask_pitch_bytes + 8 * c and the f32 exposure at exposure_ptr + r * exposure_pitch_bytes +
        4 * c (device memory, 0: not wanted; defaults: densely packed); suns: SUN_DTYPE records (see suns()); queued on the context's
        stream."""
        s = np.ascontiguousarray(suns, dtype=SUN_DTYPE).reshape(-1)
        ptr = lambda v: C.c_void_p(v) if v else None
        self._check(lib().topo_sun_exposure_grid_device(self._h, len(s), _p(s) if len(s) else None, lon0, lat0, dlon, dlat, nx, ny, ptr(lit_ptr), ptr(shadow_ptr),
                                                        ptr(exposure_ptr), 8 * nx if mask_pitch_bytes is None else mask_pitch_bytes,
                                                        4 * nx if exposure_pitch_bytes is None else exposure_pitch_bytes))

    def sun_exposure_device(self, suns, lonlat_ptr: int, n: int, lit_ptr: int = 0, shadow_ptr: int = 0, exposure_ptr: int = 0):
        """topo_sun_exposure_device: n (lon, lat) f64 pairs at lonlat_ptr (device memory, 16-byte aligned) -> the uint64 masks at
        lit_ptr / shadow_ptr + 8 * i and the f32 exposure at exposure_ptr + 4 * i (0: not wanted); queued on the context's stream."""
        s = np.ascontiguousarray(suns, dtype=SUN_DTYPE).reshape(-1)
        ptr = lambda v: C.c_void_p(v) if v else None
        self._check(lib().topo_sun_exposure_device(self._h, len(s), _p(s) if len(s) else None, n, ptr(lonlat_ptr), ptr(lit_ptr), ptr(shadow_ptr), ptr(exposure_ptr)))

    def sun_exposure(self, suns, lonlat):
        """topo_sun_exposure_read: SUN_DTYPE records and (n, 2) f64 (longitude, latitude) in degrees -> ((n,) uint64 lit masks, (n,) uint64
        shadow masks, (n,) f32 exposures: NaN where there is no terrain); waits."""
        s = np.ascontiguousarray(suns, dtype=SUN_DTYPE).reshape(-1)
        p = np.ascontiguousarray(lonlat, dtype=np.float64).reshape(-1, 2)
        lit, shadow, exposure = np.zeros(len(p), np.uint64), np.zeros(len(p), np.uint64), np.zeros(len(p), np.float32)
        ptr = lambda a: _p(a) if a.size else None
        self._check(lib().topo_sun_exposure_read(self._h, len(s), _p(s) if len(s) else None, len(p), ptr(p), ptr(lit), ptr(shadow), ptr(exposure)))
        return lit, shadow, exposure

    # unwrap: finished views that share an eye as one azimuth / elevation image (include/topo_hip.h)
    def unwrap_device(self, params, uniforms_list, src_w: int, src_h: int, rgba_src_ptr: int = 0, rgba_view_stride: int = None, rgba_pitch: int = None,
                      depth_src_ptr: int = 0, depth_view_stride: int = None, depth_pitch: int = None, rgba_out_ptr: int = 0, rgba_out_pitch: int = None,
                      depth_out_ptr: int = 0, depth_out_pitch: int = None, src_out_ptr: int = 0, src_out_pitch: int = None):
        """topo_unwrap_device: the views (uniforms_list: their 160-byte uniforms) at the device pointers *_src_ptr (defaults: densely
        packed, as render_views_device / render_panorama write them) resampled by `params` (unwrap_params) into the outputs given
        (0: not wanted; default pitch 4 * out_w); asynchronous on the context's stream."""
        p = np.ascontiguousarray(params, dtype=UNWRAP_PARAMS_DTYPE).reshape(-1)[:1]
        us = np.ascontiguousarray(np.stack([np.ascontiguousarray(u).view(np.uint8).reshape(160) for u in uniforms_list]))
        row, out_row = 4 * src_w, 4 * int(p["out_w"][0])
        ptr = lambda v: C.c_void_p(v) if v else None
        dflt = lambda v, d: d if v is None else v
        rp, dp = dflt(rgba_pitch, row), dflt(depth_pitch, row)
        self._check(lib().topo_unwrap_device(self._h, _p(p), len(us), _p(us), src_w, src_h,
                                             ptr(rgba_src_ptr), dflt(rgba_view_stride, rp * src_h), rp,
                                             ptr(depth_src_ptr), dflt(depth_view_stride, dp * src_h), dp,
                                             ptr(rgba_out_ptr), dflt(rgba_out_pitch, out_row), ptr(depth_out_ptr), dflt(depth_out_pitch, out_row),
                                             ptr(src_out_ptr), dflt(src_out_pitch, out_row)))

    def probe_div(self, kind: int, x: np.ndarray, y: np.ndarray) -> np.ndarray:
        x = np.ascontiguousarray(x, dtype=np.float32)
        y = np.ascontiguousarray(y, dtype=np.float32)
        out = np.empty_like(x)
        self._check(lib().topo_probe_div(self._h, kind, _p(x), _p(y), _p(out), x.size))
        return out

    def probe_sincos(self, x: np.ndarray):
        x = np.ascontiguousarray(x, dtype=np.float32)
        s, c = np.empty_like(x), np.empty_like(x)
        self._check(lib().topo_probe_sincos(self._h, _p(x), _p(s), _p(c), x.size))
        return s, c
