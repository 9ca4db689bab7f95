"""ctypes wrapper over tests/ground_emul.cpp (TEST-ONLY g++ build of the product's ground-point lane function, topo_ground.h)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "_build", "libground_emul.so")
_LIB = None

OUT_DTYPE = np.dtype([("lon_deg", "<f8"), ("lat_deg", "<f8"), ("height_m", "<f8"), ("range_m", "<f8"), ("w1", "<f8"), ("w2", "<f8"),
                      ("depth", "<f4"), ("kind", "<i4"), ("tile_lat_deg", "<i4"), ("tile_lon_deg", "<i4"),
                      ("cell_x", "<u4"), ("cell_y", "<u4"), ("tri", "<u4"), ("fan", "<u4")])


class EmulGroundTile(C.Structure):
    _fields_ = [("heights", C.c_void_p), ("tf", C.c_float * 6), ("lat", C.c_int32), ("lon", C.c_int32)]


def lib():
    global _LIB
    if _LIB is None:
        src = os.path.join(_HERE, "ground_emul.cpp")
        hdrs = [os.path.join(_HERE, "..", "topo-renderer_amd", "csrc", f) for f in ("topo_math.h", "topo_pipeline.h", "topo_ground.h", "srgb_tables.h")]
        os.makedirs(os.path.dirname(_SO), exist_ok=True)
        if not os.path.exists(_SO) or any(os.path.getmtime(f) > os.path.getmtime(_SO) for f in [src] + hdrs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-shared", "-o", _SO, src])
        _LIB = C.CDLL(_SO)
        _LIB.emul_ground.restype = C.c_int
        assert C.sizeof(EmulGroundTile) == 40 and OUT_DTYPE.itemsize == 80
    return _LIB


def ground(tiles, order, uniforms, depth, winners):
    """tiles: [(heights f32 (h, w), raster_point, model_point, pixel_scale)] in draw order, order: their (lat, lon); depth / winners
    (H, W) of the view with these uniforms -> (H, W) OUT_DTYPE records."""
    depth = np.ascontiguousarray(depth, np.float32)
    win = np.ascontiguousarray(winners, np.uint32)
    H, W = win.shape
    keep = [np.ascontiguousarray(t[0], np.float32) for t in tiles]
    arr = (EmulGroundTile * len(tiles))()
    for e, hts, t, (lat, lon) in zip(arr, keep, tiles, order):
        e.heights = hts.ctypes.data
        for i, v in enumerate(list(np.asarray(t[1], np.float32)) + list(np.asarray(t[2], np.float32)) + list(np.asarray(t[3], np.float32))):
            e.tf[i] = float(v)
        e.lat, e.lon = int(lat), int(lon)
    th, tw = keep[0].shape
    u = np.ascontiguousarray(uniforms).view(np.float32).reshape(-1).copy()
    out = np.zeros((H, W), OUT_DTYPE)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = lib().emul_ground(arr, len(tiles), tw, th, vp(u), W, H, vp(depth), vp(win), vp(out))
    if rc != 0:
        raise RuntimeError(f"emul_ground: a winner names no triangle of the tile set ({rc})")
    return out
