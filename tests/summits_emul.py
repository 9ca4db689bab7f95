"""ctypes wrapper over tests/summits_emul.cpp (TEST-ONLY g++ build of the product's summit rule and search, topo_summits.h)."""
from __future__ import annotations

import ctypes as C

import numpy as np

import native
from emul_tiles import geo_tile_array, vp as _vp

_LIB = None

OUT_DTYPE = np.dtype([("lon_deg", "<f8"), ("lat_deg", "<f8"), ("isolation_m", "<f8"), ("height_m", "<f4"), ("higher_height_m", "<f4"), ("rank", "<u4"), ("idx", "<u4"),
                      ("higher_rank", "<u4"), ("higher_idx", "<u4"), ("has_higher", "<i4"), ("pad_", "<i4")])
SNAP_DTYPE = np.dtype([("lon_deg", "<f8"), ("lat_deg", "<f8"), ("distance_m", "<f8"), ("height_m", "<f4"), ("status", "<i4"), ("rank", "<u4"), ("idx", "<u4")])
FOUND, NONE, INVALID = 1, 0, -1


def lib():
    global _LIB
    if _LIB is None:
        _LIB = native.load("libsummits_emul.so", ["summits_emul.cpp"], {"emul_isolation": C.c_int, "emul_summits": C.c_int, "emul_summit_snap": C.c_int})
        assert OUT_DTYPE.itemsize == 56 and SNAP_DTYPE.itemsize == 40
    return _LIB


def isolation(tiles, order, posts, radius, brute=False):
    """posts (n, 2) u32 (rank, index) -> (OUT_DTYPE records of their nearest dominators within radius -- has_higher -1: the post does not
    exist --, failed index checks).  brute: every post of every tile instead of the windows."""
    arr, keep = geo_tile_array(tiles, order)
    th, tw = keep[0].shape
    p = np.ascontiguousarray(posts, np.uint32).reshape(-1, 2)
    out = np.zeros(len(p), OUT_DTYPE)
    bad = lib().emul_isolation(arr, len(tiles), tw, th, _vp(p), len(p), C.c_double(radius), 1 if brute else 0, _vp(out))
    return out, int(bad)


def summits(tiles, order, radius, min_isolation, min_height, capacity=None):
    """The call the way the kernels run it -> (OUT_DTYPE records in tile order, the first `capacity`; the full count; the posts left
    after the prefilter and after the any-hit stage; failed index checks)."""
    arr, keep = geo_tile_array(tiles, order)
    th, tw = keep[0].shape
    cap = len(tiles) * th * tw if capacity is None else capacity
    out = np.zeros(cap, OUT_DTYPE)
    count, stages = C.c_uint32(0), (C.c_uint64 * 2)()
    bad = lib().emul_summits(arr, len(tiles), tw, th, C.c_double(radius), C.c_double(min_isolation), C.c_float(min_height), _vp(out), cap, C.byref(count), stages)
    return out[:min(cap, count.value)], int(count.value), (int(stages[0]), int(stages[1])), int(bad)


def snap(tiles, order, lonlat, radius, brute=False):
    arr, keep = geo_tile_array(tiles, order)
    th, tw = keep[0].shape
    p = np.ascontiguousarray(lonlat, np.float64).reshape(-1, 2)
    out = np.zeros(len(p), SNAP_DTYPE)
    bad = lib().emul_summit_snap(arr, len(tiles), tw, th, _vp(p), len(p), C.c_double(radius), 1 if brute else 0, _vp(out))
    return out, int(bad)
