"""ctypes wrapper over tests/cover_emul.cpp (TEST-ONLY g++ build of the covered-region lane bodies of topo_pipeline.h).  The scenes the
CPU and the GPU tests of that path share are tests/cover_cases.py's, which this module hands on under their names."""
from __future__ import annotations

import ctypes as C

import numpy as np

import native
from cover_cases import CASES, POSES_COARSE, POSES_MESA, SCENES, SMALL_BIG_CAP, case_scene  # noqa: F401
from emul_tiles import EmulTile, emul_tile, vp as _p

_LIB = None

VIS_CLEAR = 0x3F800000FFFFFFFF


def lib():
    global _LIB
    if _LIB is None:
        _LIB = native.load("libcover_emul.so", ["cover_emul.cpp"],
                           dict.fromkeys(("emul_item_covers", "emul_covers_brute", "emul_cover_item", "emul_cover_frame"), C.c_int))
    return _LIB


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
        keep += [h, nrm]
        tiles.append(emul_tile(h, nrm, tu))
    arr = (EmulTile * len(tiles))(*tiles)
    u = np.ascontiguousarray(uniforms).view(np.float32).copy()
    stats = np.zeros(10, np.uint64)
    keys = np.zeros((H, W), np.uint64) if want_keys else None
    rc = lib().emul_cover_frame(arr, len(tiles), sc.tile, sc.tile, _p(u), W, H, C.c_uint64(key_base), _p(stats), _p(keys))
    if rc != 0:
        raise RuntimeError(f"emul_cover_frame: {rc}")
    out = {k: int(v) for k, v in zip(STAT_NAMES, stats)}
    if want_keys:
        out["keys"] = keys
    return out
