"""Named placements off the 45N 15E quadrant, shared by tests/test_ground_cpu.py and tests/test_geo_gpu.py: mosaics across the
equator and the prime meridian, across the antimeridian, and poleward of 80 degrees on either side.  Each placement is a tile set
(a Scene), a frame size and a list of poses (eye, yaw, pitch, fov); every one uses 24-vertex tiles of the relief of
tests/test_ray_check_cpu.py with the eye 4000 m over the ground, 96 x 64 frames, pitch 25 and a field of view of 60 degrees."""
from __future__ import annotations

import math

import numpy as np

import topo_renderer_amd as T
from scenes import Scene, relief

TILE, EYE_DH, W, H, PITCH, FOV = 24, 4000.0, 96, 64, 25.0, 60.0


class PlacedScene(Scene):
    """A Scene from an explicit list of tile locations and an explicit eye (Scene derives both from lat0 / lon0, and so cannot name
    the tile -180 east of tile 179).  The eye's own tile is (floor(lat), floor(lon)); the tiles come in the order given."""

    def __init__(self, locs, vlat, vlon, tile=64, eye_dh=50.0, seed=T.synth.SEED_DEFAULT, height_fn=None, heights=None):
        self.tile = tile
        self.locs = [tuple(l) for l in locs]
        if heights is not None:
            self.heights = heights
        elif height_fn is None:
            self.heights = {loc: T.synth_tile(loc[0], loc[1], tile, tile, seed) for loc in self.locs}
        else:
            x = np.arange(tile, dtype=np.float64) / tile
            self.heights = {loc: np.ascontiguousarray(height_fn((loc[0] + 1 - x)[:, None], (loc[1] + x)[None, :]), dtype=np.float32)
                            for loc in self.locs}
        self.vlat, self.vlon = float(vlat), float(vlon)
        tl, to = int(math.floor(self.vlat)), int(math.floor(self.vlon))
        self.ground = T.synth.height_at(self.heights[(tl, to)], tl, to, self.vlon, self.vlat)
        self.eye = T.geometry_transform(self.ground + eye_dh, self.vlon, self.vlat)

    def at(self, vlat, vlon, eye_dh):
        """The same tiles (the same height arrays) seen from another eye."""
        return PlacedScene(self.locs, vlat, vlon, self.tile, eye_dh, heights=self.heights)


class Placement:
    """scene: the tile set (and the first eye); poses: [(scene of the pose's eye, yaw, pitch, fov)]."""

    def __init__(self, name, scene, poses):
        self.name, self.scene, self.poses, self.W, self.H = name, scene, poses, W, H

    def uniforms(self, mode=0):
        return [eye.uniforms(W, H, yaw, pitch, fov, mode) for eye, yaw, pitch, fov in self.poses]


_ANTIMERIDIAN = [(10, 179), (10, -180), (9, 179), (9, -180)]
_DONE = {}


def _build(name, height_fn):
    kw = dict(tile=TILE, eye_dh=EYE_DH, height_fn=height_fn)
    if name == "origin":
        sc = Scene(n_lat=2, n_lon=2, lat0=-1, lon0=-1, **kw)
        return Placement(name, sc, [(sc, 30.0, PITCH, FOV), (sc, 215.0, PITCH, FOV)])
    if name == "antimeridian":
        east = PlacedScene(_ANTIMERIDIAN, 10.02, 179.97, **kw)
        west = east.at(10.02, -179.97, EYE_DH)
        return Placement(name, east, [(east, 70.0, PITCH, FOV), (west, 250.0, PITCH, FOV)])
    if name == "north84":
        sc = Scene(n_lat=2, n_lon=2, lat0=83, lon0=20, **kw)
        return Placement(name, sc, [(sc, 30.0, PITCH, FOV)])
    if name == "south86":
        sc = Scene(n_lat=2, n_lon=2, lat0=-86, lon0=-40, **kw)
        return Placement(name, sc, [(sc, 200.0, PITCH, FOV)])
    raise KeyError(name)


NAMES = ("origin", "antimeridian", "north84", "south86")


def placement(name, height_fn=relief):
    key = (name, height_fn)
    if key not in _DONE:
        _DONE[key] = _build(name, height_fn)
    return _DONE[key]


def tile_set(name, tile, vfrac, eye_dh):
    """The placement's tile locations at another tile size (the benchmark's fBm heights) with a corner eye: vfrac (lat, lon) of the
    way from the mosaic's south-west corner, as Scene's argument."""
    locs = placement(name).scene.locs
    lats, lons = [l[0] for l in locs], [l[1] for l in locs]
    lat0 = min(lats)
    west = min(lons) if max(lons) - min(lons) < 180 else max(lons)      # across the antimeridian the western column is the positive one
    n_lat, n_lon = len(set(lats)), len(set(lons))
    vlon = west + n_lon * vfrac[1]
    vlon = vlon - 360.0 if vlon >= 180.0 else vlon
    return PlacedScene(locs, lat0 + n_lat * vfrac[0], vlon, tile, eye_dh)
