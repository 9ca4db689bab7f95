"""ctypes wrapper over tests/unwrap_emul.cpp (TEST-ONLY g++ build of the product's unwrap arithmetic, topo_unwrap.h, over the tables
of host_math.cpp)."""
from __future__ import annotations

import ctypes as C

import numpy as np

import native
from emul_tiles import vp

_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        _LIB = native.load("libunwrap_emul.so", ["unwrap_emul.cpp", native.HOST_MATH],
                           {"emul_unwrap": C.c_int})
    return _LIB


def unwrap(params, uniforms_list, src_w, src_h, rgba_src=None, depth_src=None, srgb=True):
    """params: a topo_unwrap_params record (topo_renderer_amd.unwrap_params); rgba_src (n, src_h, src_w, 4) u8 and depth_src
    (n, src_h, src_w) f32, each optional -> dict(src (H, W) i32, pxy (H, W, 2) f64, rgba (H, W, 4) u8 | None, depth (H, W) f32 | None)."""
    p = np.ascontiguousarray(params).reshape(-1)[:1]
    us = np.ascontiguousarray(np.stack([np.ascontiguousarray(u).view(np.float32).reshape(40) for u in uniforms_list]))
    W, H = int(p["out_w"][0]), int(p["out_h"][0])
    rs = None if rgba_src is None else np.ascontiguousarray(rgba_src, np.uint8)
    ds = None if depth_src is None else np.ascontiguousarray(depth_src, np.float32)
    for a, shape in ((rs, (len(us), src_h, src_w, 4)), (ds, (len(us), src_h, src_w))):
        assert a is None or a.shape == shape, (a.shape, shape)
    out = {"src": np.zeros((H, W), np.int32), "pxy": np.zeros((H, W, 2), np.float64),
           "rgba": None if rs is None else np.zeros((H, W, 4), np.uint8), "depth": None if ds is None else np.zeros((H, W), np.float32)}
    rc = lib().emul_unwrap(vp(p), len(us), vp(us), src_w, src_h, vp(rs), vp(ds), 1 if srgb else 0, vp(out["rgba"]), vp(out["depth"]), vp(out["src"]), vp(out["pxy"]))
    if rc != 0:
        raise RuntimeError(f"emul_unwrap: {rc}")
    return out
