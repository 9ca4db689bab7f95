"""ctypes wrapper over tests/cover_emul.cpp (TEST-ONLY g++ build of the covered-region lane bodies of topo_pipeline.h), and the
scenes the CPU and the GPU tests of that path share."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "_build", "libcover_emul.so")
_LIB = None

VIS_CLEAR = 0x3F800000FFFFFFFF


class EmulTile(C.Structure):
    _fields_ = [("heights", C.c_void_p), ("normals", C.c_void_p), ("tu", C.c_float * 24)]


def lib():
    global _LIB
    if _LIB is None:
        src = os.path.join(_HERE, "cover_emul.cpp")
        hdrs = [os.path.join(_HERE, "..", "topo-renderer_amd", "csrc", f) for f in ("topo_math.h", "topo_pipeline.h")]
        os.makedirs(os.path.dirname(_SO), exist_ok=True)
        if not os.path.exists(_SO) or any(os.path.getmtime(f) > os.path.getmtime(_SO) for f in [src] + hdrs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-shared", "-o", _SO, src])
        _LIB = C.CDLL(_SO)
        for f in ("emul_item_covers", "emul_covers_brute", "emul_cover_item", "emul_cover_frame"):
            getattr(_LIB, f).restype = C.c_int
    return _LIB


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _xy(X, Y):
    return np.ascontiguousarray(X, np.int32), np.ascontiguousarray(Y, np.int32)


def covers(X, Y, W, H, rx, ry) -> bool:
    """item_covers_region of the triangle with snapped vertices (X, Y) (1/256 px)."""
    X, Y = _xy(X, Y)
    return bool(lib().emul_item_covers(_p(X), _p(Y), W, H, rx, ry))


def covers_brute(X, Y, W, H, rx, ry) -> bool:
    """The same by brute force: triangle_pixel accepts every pixel centre of the region inside the target."""
    X, Y = _xy(X, Y)
    return bool(lib().emul_covers_brute(_p(X), _p(Y), W, H, rx, ry))


def cover_item(X, Y, z, tri_id, W, H, rx, ry) -> dict:
    """Every lane of big_cover_lane over the region under the bounds-checking sink."""
    X, Y = _xy(X, Y)
    z = np.ascontiguousarray(z, np.float32)
    keys = np.full((H, W), VIS_CLEAR, np.uint64)
    n = [C.c_uint32(0) for _ in range(3)]
    v = lib().emul_cover_item(_p(X), _p(Y), _p(z), C.c_uint32(tri_id), W, H, rx, ry, _p(keys), *[C.byref(c) for c in n])
    return {"violations": v, "fragments": n[0].value, "missing": n[1].value, "wrong": n[2].value, "keys": keys}


STAT_NAMES = ("candidates", "won", "lost", "older_wins", "rows_blind", "rows_merged", "differ", "blind_dirty", "big_items", "violations")


def cover_frame(T, sc, W, H, uniforms, key_base=0, want_keys=False) -> dict:
    """The near phase of one view of scene `sc` as the kernels order it (cover_emul.cpp: emul_cover_frame)."""
    order = sorted(sc.locs, key=lambda l: (abs(l[0]), 1 if l[0] > 0 else 0, abs(l[1]), 1 if l[1] > 0 else 0))      # draw order
    keep, tiles = [], []
    for loc in order:
        h = np.ascontiguousarray(sc.heights[loc], np.float32)
        nrm = np.zeros(h.shape, np.uint32)
        tu = T.terrain_uniforms(*sc.transform(loc), h.shape[1], h.shape[0])
        e = EmulTile()
        e.heights, e.normals = h.ctypes.data, nrm.ctypes.data
        for i in range(24):
            e.tu[i] = float(tu[i])
        keep += [h, nrm]
        tiles.append(e)
    arr = (EmulTile * len(tiles))(*tiles)
    u = np.ascontiguousarray(uniforms).view(np.float32).copy()
    stats = np.zeros(10, np.uint64)
    keys = np.zeros((H, W), np.uint64) if want_keys else None
    rc = lib().emul_cover_frame(arr, len(tiles), sc.tile, sc.tile, _p(u), W, H, C.c_uint64(key_base), _p(stats), _p(keys) if want_keys else None)
    if rc != 0:
        raise RuntimeError(f"emul_cover_frame: {rc}")
    out = {k: int(v) for k, v in zip(STAT_NAMES, stats)}
    if want_keys:
        out["keys"] = keys
    return out


# ---- the scenes of tests/test_cover_cpu.py and tests/test_cover_gpu.py ----------------------------------------------------------
# (yaw, pitch, fov) per view, positive pitch looks down.  A case is a scene, a target size and a list of submissions, a submission a
# list of views.
#   coarse   the coarse mesh seen from close up (every triangle large, many cut by the near plane), with the views of
#            test_gpu_parity.py::test_big_triangle_queue_and_clipping_paths_are_exercised and one more pitched 80 degrees down.  Its
#            giants are cut by the near plane so close to the eye that the guard band discards them (0.7 % of a frame is terrain), so
#            NO triangle of it covers a region: the scene holds the path's "nothing to claim" side.
#   mesa     a table mountain 3 km high under the eye, seen from 1 km above it: the table's triangles cover regions, and so do
#            triangles of the plain behind its rim that the table hides -- two covering triangles on one region, a lost claim.  In
#            the last view at 333 x 200 a large triangle in front reaches no more than 4 x 4 px into the target, so k_raster_rare
#            draws it itself, into a region that a triangle behind it covers and claims: an older key wins there.
POSES_COARSE = ((10, 35, 110), (200, 80, 110), (100, 5, 110), (320, 80, 110))
POSES_MESA = ((155.19, 63.47, 90), (59.14, 20.86, 60), (98.62, 62.81, 40), (129.31, 47.32, 60), (27.33, 19.98, 110))


def _mesa(lat, lon):
    d = np.hypot((lat - 45.5123) * 111.2, (lon - 15.5217) * 78.6)      # km from the viewpoint
    return np.where(d < 3.0, 3000.0, 0.0) + 0.0 * lat + 0.0 * lon


SCENES = {"coarse": dict(tile=12, n_lat=2, n_lon=2, eye_dh=60.0), "mesa": dict(tile=64, n_lat=1, n_lon=1, eye_dh=1000.0, height_fn=_mesa)}
CASES = {      # (the second view of a 333 x 200 submission starts at key 66 600 = 1 040 * 64 + 40: not on a segment boundary)
    "coarse_640x480": ("coarse", 640, 480, [[p] for p in POSES_COARSE]),
    "coarse_333x200": ("coarse", 333, 200, [[p] for p in POSES_COARSE]),
    "coarse_333x200_two_views": ("coarse", 333, 200, [[POSES_COARSE[0], POSES_COARSE[1]], [POSES_COARSE[3], POSES_COARSE[2]]]),
    "mesa_640x480": ("mesa", 640, 480, [[p] for p in POSES_MESA]),
    "mesa_333x200": ("mesa", 333, 200, [[p] for p in POSES_MESA]),
    "mesa_333x200_two_views": ("mesa", 333, 200, [[POSES_MESA[0], POSES_MESA[3]], [POSES_MESA[1], POSES_MESA[2]], [POSES_MESA[2], POSES_MESA[4]]]),
}
SMALL_BIG_CAP = 96      # big-queue entries of the overflow case: room for most of its view's 107 items (16 of them covering), not for all
_SCENE_CACHE = {}


def case_scene(name):
    from scenes import Scene
    if name not in _SCENE_CACHE:
        _SCENE_CACHE[name] = Scene(**SCENES[name])
    return _SCENE_CACHE[name]
