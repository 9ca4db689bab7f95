"""ctypes wrapper over tests/owned_emul.cpp (TEST-ONLY g++ build of the owned strips' index function and record route), and the
cases the CPU and the GPU tests of k_resolve's owned strips share (tests/test_owned_strips_cpu.py, tests/test_owned_strips_gpu.py,
tests/owned_worker.py)."""
from __future__ import annotations

import ctypes as C

import numpy as np

import cover_emul as CE
import native
from emul_tiles import EmulTile, emul_tile, vp as _p

_LIB = None

M = CE.POSES_MESA
# A case is a scene of SCENES (below), a target size and a list of submissions, a submission a list of views (yaw, pitch, fov).
#   the sizes the owned strips are asked for: 128 x 72 (a whole region row and one of 8 px: a claimed region of a single strip) and two views of 200 x 150 (regions cut by both edges; the second view's first key is 30 000, not a
#   multiple of 64), with the table mountain's viewpoints;
#   and cover_cases' own 333 x 200 cases, at which those viewpoints lose a bid and, in the last one, meet a row in which an older,
#   nearer key wins inside a claimed region.
CASES = {
    "mesa_128x72": ("mesa", 128, 72, [[p] for p in M]),
    "mesa_200x150_two_views": ("mesa", 200, 150, [[M[0], M[2]], [M[2], M[4]], [M[1], M[3]], [M[3], M[2]]]),
    "mesa_333x200": CE.CASES["mesa_333x200"],
    "mesa_333x200_two_views": CE.CASES["mesa_333x200_two_views"],
}
#   and a plain of 3 x 3 cells a quarter of a degree wide seen straight down through a 5 degree lens from 100 m: triangles hundreds of
#   thousands of pixels across (doubled area beyond 2^52 in 1/256 px units: record kind 2), none cut by the near plane at 50 m.
SCENES = {"mesa": CE.SCENES["mesa"], "giant": dict(tile=4, n_lat=1, n_lon=1, eye_dh=100.0, height_fn=lambda lat, lon: 0.0 * lat + 0.0 * lon)}
CASES["giant_200x150"] = ("giant", 200, 150, [[(33.0, 90.0, 5.0)]])
_SCENE_CACHE = {}


def case_scene(name):
    from scenes import Scene
    if name not in _SCENE_CACHE:
        _SCENE_CACHE[name] = Scene(**SCENES[name])
    return _SCENE_CACHE[name]


def lib():
    global _LIB
    if _LIB is None:
        _LIB = native.load("libowned_emul.so", ["owned_emul.cpp"], {"emul_owned_producer": C.c_uint64, "emul_owned_consumer": C.c_uint64, "emul_owned_route": C.c_int})
    return _LIB


def _strips(fn, W, H, n_views, with_cap):
    room = n_views * ((W + 63) // 64) * ((H + 7) // 8 + 8)
    out, xy, cap = np.zeros(room, np.uint64), np.zeros((room, 3), np.uint32), C.c_uint64(0)
    n = fn(C.c_uint32(W), C.c_uint32(H), C.c_uint32(n_views), _p(out), _p(xy), *([C.byref(cap)] if with_cap else []))
    assert n <= room
    return out[:n], xy[:n], cap.value


def producer_strips(W, H, n_views):
    """(record indices, (view, x, y) of the strips' origins, records of the table) as k_raster_cover names them."""
    return _strips(lib().emul_owned_producer, W, H, n_views, True)


def consumer_strips(W, H, n_views):
    """(record indices, (view, x, y)) as k_resolve names them."""
    return _strips(lib().emul_owned_consumer, W, H, n_views, False)[:2]


def scene_tiles(T, sc):
    """(the EmulTile array of scene `sc` in draw order, what keeps its memory alive)."""
    order = sorted(sc.locs, key=lambda l: (abs(l[0]), 1 if l[0] > 0 else 0, abs(l[1]), 1 if l[1] > 0 else 0))
    keep, tiles = [], []
    for loc in order:
        h = np.ascontiguousarray(sc.heights[loc], np.float32)
        nrm = (np.arange(h.size, dtype=np.uint32).reshape(h.shape) * np.uint32(2654435761)) | np.uint32(0xFF000000)      # any normals: the routes must agree on them
        keep += [h, nrm]
        tiles.append(emul_tile(h, nrm, T.terrain_uniforms(*sc.transform(loc), h.shape[1], h.shape[0])))
    return (EmulTile * len(tiles))(*tiles), keep


def route(T, sc, W, H, uniforms, tri_id, ox, oy) -> dict:
    """emul_owned_route: the record route over the strip at (ox, oy) for winner tri_id."""
    arr, keep = scene_tiles(T, sc)
    u = np.ascontiguousarray(uniforms).view(np.float32).copy()
    kind, words = C.c_int(0), np.zeros(36, np.uint32)
    differ = lib().emul_owned_route(arr, len(arr), sc.tile, sc.tile, _p(u), W, H, C.c_uint32(tri_id), ox, oy, C.byref(kind), _p(words))
    return {"differ": differ, "kind": kind.value, "words": words}


def one_winner_strips(keys):
    """The strips of 64 x 8 px of a view's keys (H x W, uint64) all of whose pixels inside the target carry one triangle's id:
    [(x, y, id)]."""
    H, W = keys.shape
    ids = (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    out = []
    for y in range(0, H, 8):
        for x in range(0, W, 64):
            s = ids[y:y + 8, x:x + 64]
            if s[0, 0] != 0xFFFFFFFF and (s == s[0, 0]).all():
                out.append((x, y, int(s[0, 0])))
    return out
