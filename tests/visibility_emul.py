"""ctypes wrapper over tests/visibility_emul.cpp (TEST-ONLY g++ build of the product's visibility rule, topo_visibility.h)."""
from __future__ import annotations

import ctypes as C

import numpy as np

import native
from emul_tiles import geo_tile_array, vp

_LIB = None

OBSERVER_DTYPE = np.dtype([("lon_deg", "<f8"), ("lat_deg", "<f8"), ("height_m", "<f8"), ("flags", "<u4"), ("_reserved", "<u4")])      # = topo_observer
EYE_DTYPE = np.dtype([("p", "<f8", 3), ("usable", "<u4"), ("_pad", "<u4")])


def lib():
    global _LIB
    if _LIB is None:
        _LIB = native.load("libvisibility_emul.so", ["visibility_emul.cpp"], {"emul_visibility": C.c_int})
        assert OBSERVER_DTYPE.itemsize == 32 and EYE_DTYPE.itemsize == 32
    return _LIB


def visibility(tiles, order, observers, lonlat, h=0.0, brute=False):
    """tiles: [(heights f32 (h, w), raster_point, model_point, pixel_scale)] in draw order, order: their (lat, lon); observers:
    OBSERVER_DTYPE records; lonlat (n, 2) degrees -> ((observers, n) uint8 classes, the resolved observers (EYE_DTYPE), failed index
    checks).  brute: every triangle instead of the lookup and the traversal."""
    arr, keep = geo_tile_array(tiles, order)
    th, tw = keep[0].shape
    ob = np.ascontiguousarray(observers, dtype=OBSERVER_DTYPE).reshape(-1)
    p = np.ascontiguousarray(lonlat, np.float64).reshape(-1, 2)
    out = np.zeros((len(ob), len(p)), np.uint8)
    eyes = np.zeros(len(ob), EYE_DTYPE)
    bad = lib().emul_visibility(arr, len(tiles), tw, th, vp(ob), len(ob), vp(p), len(p), C.c_double(h), 1 if brute else 0, vp(out), vp(eyes))
    return out, eyes, int(bad)
