"""The records of tests/emul_tiles.h on the Python side of ctypes, for the wrappers of the TEST-ONLY g++ builds (tests/*_emul.py)."""
from __future__ import annotations

import ctypes as C

import numpy as np

RAY_DTYPE = np.dtype([("origin", "<f8", 3), ("dir", "<f8", 3), ("t_min", "<f8"), ("t_max", "<f8")])      # = topo_ray


class EmulTile(C.Structure):
    _fields_ = [("heights", C.c_void_p), ("normals", C.c_void_p), ("tu", C.c_float * 24)]


class GeoTile(C.Structure):      # = EmulGeoTile
    _fields_ = [("heights", C.c_void_p), ("tf", C.c_float * 6), ("lat", C.c_int32), ("lon", C.c_int32)]


assert C.sizeof(GeoTile) == 40 and RAY_DTYPE.itemsize == 64


def emul_tile(heights, normals, tu):
    """heights f32 and normals u32, contiguous and kept alive by the caller; tu: the tile's 24 TerrainUniforms floats."""
    e = EmulTile()
    e.heights, e.normals = heights.ctypes.data, normals.ctypes.data
    for i in range(24):
        e.tu[i] = float(tu[i])
    return e


def geo_tile_array(tiles, order):
    """tiles: [(heights f32 (h, w), raster_point, model_point, pixel_scale)] in draw order, order: their (lat, lon) -> (GeoTile array,
    the height arrays it points into: keep them alive as long as the array)."""
    keep = [np.ascontiguousarray(t[0], np.float32) for t in tiles]
    arr = (GeoTile * len(tiles))()
    for e, hts, t, (lat, lon) in zip(arr, keep, tiles, order):
        e.heights = hts.ctypes.data
        for i, v in enumerate(list(np.asarray(t[1], np.float32)) + list(np.asarray(t[2], np.float32)) + list(np.asarray(t[3], np.float32))):
            e.tf[i] = float(v)
        e.lat, e.lon = int(lat), int(lon)
    return arr, keep


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)
