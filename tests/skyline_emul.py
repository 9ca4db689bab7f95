"""ctypes wrapper over tests/skyline_emul.cpp (TEST-ONLY g++ build of the product's skyline rule, topo_skyline.h)."""
from __future__ import annotations

import ctypes as C

import numpy as np

import native
from emul_tiles import geo_tile_array, vp
from visibility_emul import OBSERVER_DTYPE

_LIB = None

OUT_DTYPE = np.dtype([("elevation_deg", "<f8"), ("range_m", "<f8"), ("lon_deg", "<f8"), ("lat_deg", "<f8"), ("height_m", "<f8"), ("s", "<f8"), ("z", "<f8"), ("ratio", "<f8"),
                      ("kind", "<i4"), ("tile_lat_deg", "<i4"), ("tile_lon_deg", "<i4"), ("cell_x", "<u4"), ("cell_y", "<u4"), ("tri", "<u4"), ("edge", "<u4"),
                      ("rank", "<u4"), ("triangle", "<u4"), ("_pad", "<u4")])      # = EmulSkyOut


def lib():
    global _LIB
    if _LIB is None:
        _LIB = native.load("libskyline_emul.so", ["skyline_emul.cpp"], {"emul_skyline": C.c_int})
        assert OUT_DTYPE.itemsize == 104
    return _LIB


def skyline(tiles, order, observers, az0, daz, n_az, min_range, max_range, brute=False):
    """tiles: [(heights f32 (h, w), raster_point, model_point, pixel_scale)] in draw order, order: their (lat, lon); observers:
    OBSERVER_DTYPE records -> ((observers, n_az) OUT_DTYPE records, failed index checks).  brute: every triangle instead of the lookup
    and the traversal."""
    arr, keep = geo_tile_array(tiles, order)
    th, tw = keep[0].shape
    ob = np.ascontiguousarray(observers, dtype=OBSERVER_DTYPE).reshape(-1)
    out = np.zeros((len(ob), n_az), OUT_DTYPE)
    bad = lib().emul_skyline(arr, len(tiles), tw, th, vp(ob), len(ob), C.c_double(az0), C.c_double(daz), n_az, C.c_double(min_range), C.c_double(max_range),
                             1 if brute else 0, vp(out))
    return out, int(bad)
