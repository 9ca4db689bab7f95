"""ctypes wrapper over tests/surface_emul.cpp (TEST-ONLY g++ build of the product's surface rule and lookup, topo_surface.h)."""
from __future__ import annotations

import ctypes as C

import numpy as np

import native
from emul_tiles import RAY_DTYPE, geo_tile_array, vp as _vp

_LIB = None

OUT_DTYPE = np.dtype([("height_m", "<f8"), ("slope_deg", "<f8"), ("aspect_deg", "<f8"), ("w1", "<f8"), ("w2", "<f8"), ("kind", "<i4"), ("tile_lat_deg", "<i4"),
                      ("tile_lon_deg", "<i4"), ("cell_x", "<u4"), ("cell_y", "<u4"), ("tri", "<u4"), ("rank", "<u4"), ("triangle", "<u4")])
SUMMARY_DTYPE = np.dtype([("min_clearance_m", "<f4"), ("min_sample", "<u4"), ("n_terrain", "<u4"), ("kind", "<i4")])      # = topo_profile_summary

def lib():
    global _LIB
    if _LIB is None:
        _LIB = native.load("libsurface_emul.so", ["surface_emul.cpp"], {"emul_surface": C.c_int, "emul_profile": C.c_int})
        assert OUT_DTYPE.itemsize == 72 and SUMMARY_DTYPE.itemsize == 16
    return _LIB


def surface(tiles, order, lonlat, brute=False):
    """tiles: [(heights f32 (h, w), raster_point, model_point, pixel_scale)] in draw order, order: their (lat, lon); lonlat (n, 2)
    degrees -> (OUT_DTYPE records, failed index checks).  brute: every triangle instead of the lookup."""
    arr, keep = geo_tile_array(tiles, order)
    th, tw = keep[0].shape
    p = np.ascontiguousarray(lonlat, np.float64).reshape(-1, 2)
    out = np.zeros(len(p), OUT_DTYPE)
    bad = lib().emul_surface(arr, len(tiles), tw, th, _vp(p), len(p), 1 if brute else 0, _vp(out))
    return out, int(bad)


def profile(tiles, order, segs, m):
    """RAY_DTYPE segments, m samples each -> (SUMMARY_DTYPE records, (n, m, 2) f32 (terrain, line) samples, failed index checks)."""
    arr, keep = geo_tile_array(tiles, order)
    th, tw = keep[0].shape
    r = np.ascontiguousarray(segs, dtype=RAY_DTYPE).reshape(-1)
    smp = np.zeros((len(r), m, 2), np.float32)
    summary = np.zeros(len(r), SUMMARY_DTYPE)
    bad = lib().emul_profile(arr, len(tiles), tw, th, _vp(r), len(r), m, _vp(smp), _vp(summary))
    return summary, smp, int(bad)
