"""ctypes wrapper over tests/refraction_emul.cpp (TEST-ONLY g++ build of the product's refracted visibility rule, topo_refraction.h)."""
from __future__ import annotations

import ctypes as C

import numpy as np

import native
from emul_tiles import geo_tile_array, vp
from visibility_emul import EYE_DTYPE, OBSERVER_DTYPE

_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        _LIB = native.load("librefraction_emul.so", ["refraction_emul.cpp"], {"emul_refraction": C.c_int, "emul_refraction_lift": None})
    return _LIB


def visibility(tiles, order, observers, lonlat, h=0.0, k=0.0, brute=False):
    """As visibility_emul.visibility, under refraction coefficient k: ((observers, n) uint8 classes, the resolved observers
    (EYE_DTYPE), failed index checks).  brute: every triangle instead of the lookup and the traversal."""
    arr, keep = geo_tile_array(tiles, order)
    th, tw = keep[0].shape
    ob = np.ascontiguousarray(observers, dtype=OBSERVER_DTYPE).reshape(-1)
    p = np.ascontiguousarray(lonlat, np.float64).reshape(-1, 2)
    out = np.zeros((len(ob), len(p)), np.uint8)
    eyes = np.zeros(len(ob), EYE_DTYPE)
    bad = lib().emul_refraction(arr, len(tiles), tw, th, vp(ob), len(ob), vp(p), len(p), C.c_double(h), C.c_double(k), 1 if brute else 0, vp(out), vp(eyes))
    return out, eyes, int(bad)


def lift(observer, point, k):
    o, p, out = np.ascontiguousarray(observer, np.float64), np.ascontiguousarray(point, np.float64), np.zeros(3)
    lib().emul_refraction_lift(vp(o), vp(p), C.c_double(k), vp(out))
    return out
