"""ctypes wrapper over tests/cull_emul.cpp (TEST-ONLY g++ build of the load phase's block bounds, topo_cull.h)."""
from __future__ import annotations

import ctypes as C

import numpy as np

import native

_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        _LIB = native.load("libcull_emul.so", ["cull_emul.cpp"], {"emul_block_bounds": C.c_uint32})
    return _LIB


def tile_tables(heights, transform, minmax):
    """The tables read_tile_tables hands out for one tile, from the host build: {"minmax": the (n, 2) f32 given (the kernels' own
    reductions are not emulated), "bounds": 18 n f64}."""
    th, tw = heights.shape
    rp, mp, ps = (np.asarray(a, np.float32) for a in transform)
    tr = np.float32([rp[0], rp[1], mp[0], mp[1], ps[0], ps[1]])
    mm = np.ascontiguousarray(minmax, np.float32)
    bounds = np.full(18 * len(mm), np.nan, np.float64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    n = lib().emul_block_bounds(vp(tr), C.c_uint32(tw), C.c_uint32(th), vp(mm), vp(bounds))
    assert n == len(mm)
    return {"minmax": mm, "bounds": bounds}
