"""ctypes wrapper over tests/ground_emul.cpp (TEST-ONLY g++ build of the product's ground-point lane function, topo_ground.h)."""
from __future__ import annotations

import ctypes as C

import numpy as np

import native
from emul_tiles import geo_tile_array, vp

_LIB = None

OUT_DTYPE = np.dtype([("lon_deg", "<f8"), ("lat_deg", "<f8"), ("height_m", "<f8"), ("range_m", "<f8"), ("w1", "<f8"), ("w2", "<f8"),
                      ("depth", "<f4"), ("kind", "<i4"), ("tile_lat_deg", "<i4"), ("tile_lon_deg", "<i4"),
                      ("cell_x", "<u4"), ("cell_y", "<u4"), ("tri", "<u4"), ("fan", "<u4")])


def lib():
    global _LIB
    if _LIB is None:
        _LIB = native.load("libground_emul.so", ["ground_emul.cpp"], {"emul_ground": C.c_int})
        assert OUT_DTYPE.itemsize == 80
    return _LIB


def ground(tiles, order, uniforms, depth, winners):
    """tiles: [(heights f32 (h, w), raster_point, model_point, pixel_scale)] in draw order, order: their (lat, lon); depth / winners
    (H, W) of the view with these uniforms -> (H, W) OUT_DTYPE records."""
    depth = np.ascontiguousarray(depth, np.float32)
    win = np.ascontiguousarray(winners, np.uint32)
    H, W = win.shape
    arr, keep = geo_tile_array(tiles, order)
    th, tw = keep[0].shape
    u = np.ascontiguousarray(uniforms).view(np.float32).reshape(-1).copy()
    out = np.zeros((H, W), OUT_DTYPE)
    rc = lib().emul_ground(arr, len(tiles), tw, th, vp(u), W, H, vp(depth), vp(win), vp(out))
    if rc != 0:
        raise RuntimeError(f"emul_ground: a winner names no triangle of the tile set ({rc})")
    return out
