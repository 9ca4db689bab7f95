"""Cases of the refracted visibility tests (tests/test_refraction_cpu.py, tests/test_refraction_gpu.py).  A case is a tile set,
observers, targets -- a regular grid as topo_visibility_refracted_grid_device forms it, or a list --, a target height and a
coefficient k; its reference (refraction_ref), its emulation (refraction_emul: traversal and every-triangle loop) are computed once
and shared.  The tile sets, grids and observer records are visibility_cases'.

  flat        three 64-post tiles of constant height 0 at (44 N, 5-7 E); an observer 100 m up at (5.2, 44.5); 20 m masts every 0.005
              degrees along the parallel: the hand-known case (the geometric horizon of a sphere, and of a sphere of radius R0 / (1 - k))
  gentle      the same three locations at 48 posts, heights 300 + 60 sin(700 lon) cos(500 lat) (arguments in degrees), a 60 x 20 grid,
              observers 30 m and 100 m above the terrain at (5.413, 44.517): sight lines that graze gentle relief for tens of kilometres
  ridges_ne   visibility_cases' 2 x 2 mosaic under 40 x 36 (several tiles, a wave with a tail), from 4000 m and 2500 m over the sphere
  long        visibility_cases' 1 x 3 mosaic of 700 m relief under 60 x 20, from 4000 m and 1200 m above the terrain: sight lines of
              up to 200 km, where the lift reaches hundreds of metres
  blocks130   the 130 x 34 `blocks` tile under a 130 x 7 grid with three observers, the middle one unusable
  grid        the `grid` tile (85 blocks: two batches of 64) under 24 x 12
  observers   visibility_cases' list of observers of every kind"""
from __future__ import annotations

import numpy as np

import los_cases as LC
import refraction_emul as RE
import refraction_ref as RR
import visibility_cases as VC
import visibility_ref as VR
from scenes import Scene

K = RR.STANDARD
BOX3 = (5.0, 8.0, 44.0, 45.0)
MAST_STEP = 0.005
_CASES, _REF, _EMU = {}, {}, {}


def _flat_tiles():
    sc = Scene(64, 1, 3, lat0=44, lon0=5, height_fn=lambda la, lo: 0.0 * (la + lo))
    return LC.scene_tiles(sc) + (BOX3,)


def _gentle_tiles():
    sc = Scene(48, 1, 3, lat0=44, lon0=5, height_fn=lambda la, lo: 300.0 + 60.0 * np.sin(np.radians(700.0 * lo)) * np.cos(np.radians(500.0 * la)))
    return LC.scene_tiles(sc) + (BOX3,)


VC.TILESETS.setdefault("refraction_flat", _flat_tiles)
VC.TILESETS.setdefault("refraction_gentle", _gentle_tiles)


def _case(ts, obs, grid=None, lonlat=None, h=0.0, k=K, **more):
    tiles, order, box = VC.tileset(ts)
    return dict(tileset=ts, tiles=tiles, order=order, obs=obs, grid=grid, lonlat=VC.grid_points(grid) if lonlat is None else lonlat, h=h, k=k, **more)


def _flat():
    lon = 5.2 + MAST_STEP * np.arange(1, 500)
    return _case("refraction_flat", VC.observer_records(5.2, 44.5, 100.0), lonlat=np.stack([lon, np.full(len(lon), 44.5)], axis=1), h=20.0, H=100.0)


def _gentle():
    return _case("refraction_gentle", np.concatenate([VC.observer_records(5.413, 44.517, 30.0), VC.observer_records(5.413, 44.517, 100.0)]), VC.box_grid(BOX3, 60, 20))


def _ridges():
    box = VC.tileset("ridges_ne")[2]
    return _case("ridges_ne", np.concatenate([VC.centre_observer(box, 4000.0, False), VC.centre_observer(box, 2500.0, False)]), VC.box_grid(box, 40, 36))


def _long():
    box = VC.tileset("long")[2]
    return _case("long", np.concatenate([VC.centre_observer(box, 4000.0), VC.centre_observer(box, 1200.0)]), VC.box_grid(box, 60, 20))


def _blocks130():
    box = VC.tileset("blocks")[2]
    obs = np.concatenate([VC.centre_observer(box, 300.0), VC.observer_records(2.0, 3.0, 50.0), VC.observer_records(7.113, 46.871, 9000.0, False)])
    return _case("blocks", obs, VC.box_grid(box, 130, 7))


def _grid():
    box = VC.tileset("grid")[2]
    return _case("grid", VC.centre_observer(box, 250.0), VC.box_grid(box, 24, 12))


def _observers():
    c = VC.case("observers")
    return _case("ridges_ne", c["obs"], lonlat=c["lonlat"], unusable=c["unusable"], extra=c["extra"], at=c["at"])


CASES = {"flat": _flat, "gentle": _gentle, "ridges_ne": _ridges, "long": _long, "blocks130": _blocks130, "grid": _grid, "observers": _observers}


def case(name):
    if name not in _CASES:
        _CASES[name] = CASES[name]()
    return _CASES[name]


def reference(name, k=None):
    """(classes, ambiguous) of the case by refraction_ref at the case's coefficient or at k; computed once."""
    c = case(name)
    k = c["k"] if k is None else k
    if (name, k) not in _REF:
        _REF[name, k] = RR.visibility(VC.meshes(c["tileset"]), c["obs"], c["lonlat"], c["h"], k)
    return _REF[name, k]


def emulation(name, k=None, brute=False):
    """(classes, resolved observers) of the case by the g++ build, the traversal or (brute) every triangle; computed once."""
    c = case(name)
    k = c["k"] if k is None else k
    if (name, k, brute) not in _EMU:
        cls, eyes, bad = RE.visibility(c["tiles"], c["order"], c["obs"], c["lonlat"], c["h"], k, brute)
        assert bad == 0, f"{name}: {bad} index checks failed in the emulation"
        _EMU[name, k, brute] = (cls, eyes)
    return _EMU[name, k, brute]


def horizon_range(H, h, k):
    """How far a mast of height h is seen from height H over a smooth sphere under coefficient k (metres)."""
    return np.sqrt(2.0 * VR.R0 * H / (1.0 - k)) + np.sqrt(2.0 * VR.R0 * h / (1.0 - k))


def visible_run(c, cls):
    """The masts of the flat case that have terrain: (their distances from the observer's foot in metres along the sphere, their
    classes), in order of distance."""
    keep = cls != VR.NONE
    u0 = VR.SR.direction(c["obs"]["lon_deg"][0], c["obs"]["lat_deg"][0])
    u = VR.SR.direction(c["lonlat"][:, 0], c["lonlat"][:, 1])
    dist = VR.R0 * 2.0 * np.arcsin(0.5 * np.linalg.norm(u - u0[None, :], axis=1))
    return dist[keep], cls[keep]
