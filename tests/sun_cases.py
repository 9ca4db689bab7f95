"""Cases of the sun exposure tests (tests/test_sun_cpu.py, tests/test_sun_gpu.py), on the tile sets and grids of visibility_cases.  A
case is a tile set, suns and targets -- a regular grid lon0 + c dlon, lat0 + r dlat, as topo_sun_exposure_grid_device forms it; its
reference (sun_ref) and its emulation (sun_emul: traversal and every-triangle loop) are computed once and shared.

The standard suns are 13 directions along a day's arc, made with los_ref.sun_direction at the centre of the tile set's degree box:
two below the horizontal plane (night everywhere near the centre), low ones either side, a noon of 42 degrees.  Every weight is 15
(minutes per sample)."""
from __future__ import annotations

import numpy as np

import los_ref as LR
import sun_emul as SE
import sun_ref as SNR
import visibility_cases as VC

SUN_DTYPE = SE.SUN_DTYPE
MAX_AMBIGUOUS = VC.MAX_AMBIGUOUS      # los_ref's cap
ARC = ((75, -3), (90, 1), (100, 4), (115, 12), (135, 25), (160, 38), (180, 42), (200, 38), (225, 25), (245, 12), (260, 4), (270, 1), (285, -3))
WEIGHT = 15.0
EL4, EL1, NIGHT_SUNS = (2, 10), (1, 11), (0, 12)      # the suns at elevation 4, 1 and -3 degrees
GRIDS = {"ridges_ne": (40, 36, False), "blocks": (48, 30, False), "long": (60, 20, False), "void_nan": (40, 36, False), "polar": (24, 20, True),
         "antimeridian": (24, 20, False), "north84": (24, 20, False)}
BALANCED = ("ridges_ne", "blocks", "long")
_CASES, _REF, _EMU = {}, {}, {}


def sun_records(dirs, weights=WEIGHT):
    d = np.atleast_2d(np.asarray(dirs, np.float64))
    out = np.zeros(len(d), SUN_DTYPE)
    out["dir"], out["weight"] = d, weights
    return out


def arc_suns(box, arc=ARC, weights=WEIGHT):
    """The suns at the (azimuth, elevation) pairs of `arc` seen from the centre of the degree box."""
    lon, lat = 0.5 * (box[0] + box[1]), 0.5 * (box[2] + box[3])
    return sun_records([LR.sun_direction(lon, lat, az, el) for az, el in arc], weights)


def standard_suns(ts):
    return arc_suns(VC.tileset(ts)[2])


def grid_case(ts, nx, ny, suns=None, south_to_north=False):
    tiles, order, box = VC.tileset(ts)
    grid = VC.box_grid(box, nx, ny, south_to_north)
    return dict(tileset=ts, tiles=tiles, order=order, suns=standard_suns(ts) if suns is None else suns, grid=grid, lonlat=VC.grid_points(grid))


def case(name):
    if name not in _CASES:
        nx, ny, s2n = GRIDS[name]
        _CASES[name] = grid_case(name, nx, ny, south_to_north=s2n)
    return _CASES[name]


def reference(name):
    """(classes, lit, shadow, exposure, ambiguous) of the case by sun_ref; computed once."""
    if name not in _REF:
        c = case(name)
        _REF[name] = SNR.sun_exposure(VC.meshes(c["tileset"]), c["suns"], c["lonlat"])
    return _REF[name]


def emulate(c, brute=False):
    """(classes, lit, shadow, exposure) of a case dict by the g++ build, the traversal or (brute) every triangle; computed once."""
    key = (c["tileset"], c["suns"].tobytes(), c["lonlat"].tobytes(), brute)
    if key not in _EMU:
        cls, lit, shadow, exposure, bad = SE.sun_exposure(c["tiles"], c["order"], c["suns"], c["lonlat"], brute)
        assert bad == 0, f"{c['tileset']}: {bad} index checks failed in the emulation"
        _EMU[key] = (cls, lit, shadow, exposure)
    return _EMU[key]


def emulation(name, brute=False):
    return emulate(case(name), brute)


def counts(cls):
    return tuple(int((cls == k).sum()) for k in range(5))


def ulp_distance_f32(a, b):
    """The distance in f32 ulps between finite values of like sign (or zeros)."""
    ia, ib = np.asarray(a, np.float32).view(np.int32).astype(np.int64), np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)
