"""ctypes wrapper over tests/sun_emul.cpp (TEST-ONLY g++ build of the product's sun exposure rule, topo_sun.h)."""
from __future__ import annotations

import ctypes as C

import numpy as np

import native
from emul_tiles import geo_tile_array, vp

_LIB = None

SUN_DTYPE = np.dtype([("dir", "<f8", 3), ("weight", "<f8")])      # = topo_sun


def lib():
    global _LIB
    if _LIB is None:
        _LIB = native.load("libsun_emul.so", ["sun_emul.cpp"], {"emul_sun_exposure": C.c_int, "emul_sun_constants": None})
        assert SUN_DTYPE.itemsize == 32
    return _LIB


def unit(suns):
    """SUN_DTYPE records with their directions normalised as the host entry points normalise them: len = sqrt(x x + y y + z z), d / len."""
    s = np.ascontiguousarray(suns, dtype=SUN_DTYPE).reshape(-1).copy()
    d = s["dir"]
    s["dir"] = d / np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])[:, None]
    return s


def sun_exposure(tiles, order, suns, lonlat, brute=False):
    """tiles: [(heights f32 (h, w), raster_point, model_point, pixel_scale)] in draw order, order: their (lat, lon); suns: SUN_DTYPE
    records (normalised here); lonlat (n, 2) degrees -> ((suns, n) uint8 classes, (n) uint64 lit, (n) uint64 shadow, (n) f32
    exposure, failed index checks).  brute: every triangle instead of the lookup and the traversal."""
    arr, keep = geo_tile_array(tiles, order)
    th, tw = keep[0].shape
    s = unit(suns)
    p = np.ascontiguousarray(lonlat, np.float64).reshape(-1, 2)
    cls = np.zeros((len(s), len(p)), np.uint8)
    lit, shadow, exposure = np.zeros(len(p), np.uint64), np.zeros(len(p), np.uint64), np.zeros(len(p), np.float32)
    bad = lib().emul_sun_exposure(arr, len(tiles), tw, th, vp(s), len(s), vp(p), len(p), 1 if brute else 0, vp(cls), vp(lit), vp(shadow), vp(exposure))
    return cls, lit, shadow, exposure, int(bad)


def constants():
    out = np.zeros(8, np.uint32)
    lib().emul_sun_constants(vp(out))
    return dict(NONE=int(out[0]), LIT=int(out[1]), AWAY=int(out[2]), SHADOW=int(out[3]), NIGHT=int(out[4]), MAX_SUNS=int(out[5]), SUN_BYTES=int(out[6]))
