"""ctypes wrapper over tests/los_emul.cpp (TEST-ONLY g++ build of the product's ray test and traversal, topo_los.h)."""
from __future__ import annotations

import ctypes as C

import numpy as np

import native
from emul_tiles import RAY_DTYPE, geo_tile_array, vp

_LIB = None

OUT_DTYPE = np.dtype([("t", "<f8"), ("lon_deg", "<f8"), ("lat_deg", "<f8"), ("height_m", "<f8"), ("w1", "<f8"), ("w2", "<f8"),
                      ("kind", "<i4"), ("tile_lat_deg", "<i4"), ("tile_lon_deg", "<i4"), ("cell_x", "<u4"), ("cell_y", "<u4"), ("tri", "<u4"),
                      ("front", "<u4"), ("rank", "<u4"), ("triangle", "<u4"), ("_pad", "<u4")])

def lib():
    global _LIB
    if _LIB is None:
        _LIB = native.load("liblos_emul.so", ["los_emul.cpp"], {"emul_raycast": C.c_int, "emul_sunlit": C.c_int})
        assert OUT_DTYPE.itemsize == 88
    return _LIB


def sunlit(tiles, order, rank, tri, w1, w2, sun):
    """The sunlit class (0 none, 1 lit, 2 away, 3 shadow) of the ground points (triangle tri of tile rank, plane weights w1, w2 as
    ground_solve gives them) under a sun in unit direction `sun`; rank >= len(tiles): no point.  -> (uint8 classes, failed checks)."""
    arr, keep = geo_tile_array(tiles, order)
    th, tw = keep[0].shape
    rank, tri = np.ascontiguousarray(rank, np.uint32).reshape(-1), np.ascontiguousarray(tri, np.uint32).reshape(-1)
    w1, w2 = np.ascontiguousarray(w1, np.float64).reshape(-1), np.ascontiguousarray(w2, np.float64).reshape(-1)
    s = np.ascontiguousarray(sun, np.float64).reshape(3)
    out = np.zeros(len(rank), np.uint8)
    bad = lib().emul_sunlit(arr, len(tiles), tw, th, len(rank), vp(rank), vp(tri), vp(w1), vp(w2), vp(s), vp(out))
    return out, int(bad)


def raycast(tiles, order, rays, brute=False):
    """tiles: [(heights f32 (h, w), raster_point, model_point, pixel_scale)] in draw order, order: their (lat, lon); rays: RAY_DTYPE
    records -> (OUT_DTYPE records, failed index checks).  brute: every triangle instead of the traversal."""
    arr, keep = geo_tile_array(tiles, order)
    th, tw = keep[0].shape
    r = np.ascontiguousarray(rays, dtype=RAY_DTYPE).reshape(-1)
    out = np.zeros(len(r), OUT_DTYPE)
    bad = lib().emul_raycast(arr, len(tiles), tw, th, vp(r), len(r), 1 if brute else 0, vp(out))
    return out, int(bad)
