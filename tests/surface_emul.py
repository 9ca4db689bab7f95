"""ctypes wrapper over tests/surface_emul.cpp (TEST-ONLY g++ build of the product's surface rule and lookup, topo_surface.h)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "_build", "libsurface_emul.so")
_LIB = None

OUT_DTYPE = np.dtype([("height_m", "<f8"), ("slope_deg", "<f8"), ("aspect_deg", "<f8"), ("w1", "<f8"), ("w2", "<f8"), ("kind", "<i4"), ("tile_lat_deg", "<i4"),
                      ("tile_lon_deg", "<i4"), ("cell_x", "<u4"), ("cell_y", "<u4"), ("tri", "<u4"), ("rank", "<u4"), ("triangle", "<u4")])
SUMMARY_DTYPE = np.dtype([("min_clearance_m", "<f4"), ("min_sample", "<u4"), ("n_terrain", "<u4"), ("kind", "<i4")])      # = topo_profile_summary
RAY_DTYPE = np.dtype([("origin", "<f8", 3), ("dir", "<f8", 3), ("t_min", "<f8"), ("t_max", "<f8")])      # = topo_ray


class EmulSurfaceTile(C.Structure):
    _fields_ = [("heights", C.c_void_p), ("tf", C.c_float * 6), ("lat", C.c_int32), ("lon", C.c_int32)]


def lib():
    global _LIB
    if _LIB is None:
        src = os.path.join(_HERE, "surface_emul.cpp")
        hdrs = [os.path.join(_HERE, "..", "topo-renderer_amd", "csrc", f) for f in ("topo_math.h", "topo_pipeline.h", "topo_ground.h", "topo_los.h", "topo_surface.h")]
        os.makedirs(os.path.dirname(_SO), exist_ok=True)
        if not os.path.exists(_SO) or any(os.path.getmtime(f) > os.path.getmtime(_SO) for f in [src] + hdrs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-shared", "-o", _SO, src])
        _LIB = C.CDLL(_SO)
        _LIB.emul_surface.restype = C.c_int
        _LIB.emul_profile.restype = C.c_int
        assert C.sizeof(EmulSurfaceTile) == 40 and OUT_DTYPE.itemsize == 72 and SUMMARY_DTYPE.itemsize == 16 and RAY_DTYPE.itemsize == 64
    return _LIB


def _tile_array(tiles, order):
    keep = [np.ascontiguousarray(t[0], np.float32) for t in tiles]
    arr = (EmulSurfaceTile * len(tiles))()
    for e, hts, t, (lat, lon) in zip(arr, keep, tiles, order):
        e.heights = hts.ctypes.data
        for i, v in enumerate(list(np.asarray(t[1], np.float32)) + list(np.asarray(t[2], np.float32)) + list(np.asarray(t[3], np.float32))):
            e.tf[i] = float(v)
        e.lat, e.lon = int(lat), int(lon)
    return arr, keep


_vp = lambda a: a.ctypes.data_as(C.c_void_p)


def surface(tiles, order, lonlat, brute=False):
    """tiles: [(heights f32 (h, w), raster_point, model_point, pixel_scale)] in draw order, order: their (lat, lon); lonlat (n, 2)
    degrees -> (OUT_DTYPE records, failed index checks).  brute: every triangle instead of the lookup."""
    arr, keep = _tile_array(tiles, order)
    th, tw = keep[0].shape
    p = np.ascontiguousarray(lonlat, np.float64).reshape(-1, 2)
    out = np.zeros(len(p), OUT_DTYPE)
    bad = lib().emul_surface(arr, len(tiles), tw, th, _vp(p), len(p), 1 if brute else 0, _vp(out))
    return out, int(bad)


def profile(tiles, order, segs, m):
    """RAY_DTYPE segments, m samples each -> (SUMMARY_DTYPE records, (n, m, 2) f32 (terrain, line) samples, failed index checks)."""
    arr, keep = _tile_array(tiles, order)
    th, tw = keep[0].shape
    r = np.ascontiguousarray(segs, dtype=RAY_DTYPE).reshape(-1)
    smp = np.zeros((len(r), m, 2), np.float32)
    summary = np.zeros(len(r), SUMMARY_DTYPE)
    bad = lib().emul_profile(arr, len(tiles), tw, th, _vp(r), len(r), m, _vp(smp), _vp(summary))
    return summary, smp, int(bad)
