"""The scenes and cases the CPU and the GPU tests of the covered-region path share (tests/test_cover_cpu.py, tests/test_cover_gpu.py,
tests/cover_worker.py)."""
from __future__ import annotations

import numpy as np

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
