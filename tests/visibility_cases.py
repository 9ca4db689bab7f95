"""Cases of the visibility tests (tests/test_visibility_cpu.py, tests/test_visibility_gpu.py), on the tile sets of los_cases.CASES
(built with los_cases' own helpers, without the rays and their references).  A case is a tile set, observers, targets -- a regular
grid lon0 + c dlon, lat0 + r dlat, as topo_visibility_grid_device forms it, or a list -- and a target height; its reference
(visibility_ref) and its emulation (visibility_emul: traversal and every-triangle loop) are computed once and shared.

The grids are offset from the DEM lattice: column centre (c + 0.37) / nx and row centre (r + 0.41) / ny, rows from the north, of the
mosaic's degree box plus 0.05 degrees each side.  The standard observer stands 4000 m above the terrain near the box's centre
(+0.013, +0.017 degrees).  On the 2 x 2 mosaics that point lies in the gap between the tile rows (a tile's last row stops one post
short of its neighbour), where an observer above TERRAIN is unusable: there the standard observer stands 4000 m above the sphere."""
from __future__ import annotations

import numpy as np

import los_cases as LC
import visibility_emul as VE
import visibility_ref as VR
from scenes import Scene

OBSERVER_DTYPE = VE.OBSERVER_DTYPE
MARGIN = 0.05
MAX_AMBIGUOUS = 0.005      # los_ref's cap


def observer_records(lon, lat, height, above_terrain=True):
    lo, la, h, f = np.broadcast_arrays(np.atleast_1d(np.asarray(lon, np.float64)), np.asarray(lat, np.float64), np.asarray(height, np.float64),
                                       np.asarray(above_terrain, bool))
    out = np.zeros(len(lo), OBSERVER_DTYPE)
    out["lon_deg"], out["lat_deg"], out["height_m"], out["flags"] = lo, la, h, np.where(f, VR.ABOVE_TERRAIN, 0)
    return out


# ---- tile sets: (tiles in draw order, their (lat, lon), the degree box (lon_min, lon_max, lat_min, lat_max)) ---------------------------
def _ridges_ne():
    sc = Scene(height_fn=LC.ridges, **LC.RIDGES["ridges_ne"][0])
    return LC.scene_tiles(sc) + ((15.0, 17.0, 45.0, 47.0),)


def _single(w, h):
    lat, lon = 46, 7
    return [(LC.blocks_heights(lat, lon, w, h),) + tuple(LC.T.synth.tile_transform(lat, lon, w, h))], [(lat, lon)], (7.0, 8.0, 46.0, 47.0)


def _long():
    sc = Scene(48, 1, 3, lat0=44, lon0=5, height_fn=lambda la, lo: 900.0 + 700.0 * np.sin(np.radians(2100.0 * lo)) * np.cos(np.radians(1300.0 * la)) + 0.0 * (la + lo))
    return LC.scene_tiles(sc) + ((5.0, 8.0, 44.0, 45.0),)


def _void_nan():
    import void_scenes as VS
    _, void, _, _, _ = VS.relief_case("ne_2x2", "nan")
    return LC.scene_tiles(void) + ((15.0, 17.0, 45.0, 47.0),)


TILESETS = {"ridges_ne": _ridges_ne, "blocks": lambda: _single(130, 34), "grid": lambda: _single(*LC.BATCH_TILES["grid"]), "long": _long, "void_nan": _void_nan,
            "antimeridian": lambda: LC.placed_tiles([(10, 179), (10, -180)], 48) + ((179.0, 181.0, 10.0, 11.0),),
            "north84": lambda: LC.placed_tiles([(84, 20), (84, 21)], 48) + ((20.0, 22.0, 84.0, 85.0),),
            "polar": lambda: LC.placed_tiles([(89, 20), (89, 21), (89, -160), (89, -159)], 32) + ((20.0, 22.0, 89.0, 90.0),)}
_TILES, _MESHES, _CASES, _REF, _EMU = {}, {}, {}, {}, {}


def tileset(name):
    if name not in _TILES:
        _TILES[name] = TILESETS[name]()
    return _TILES[name]


def meshes(name):
    if name not in _MESHES:
        _MESHES[name] = VR.Meshes(tileset(name)[0])
    return _MESHES[name]


def box_grid(box, nx, ny, south_to_north=False):
    """(lon0, lat0, dlon, dlat, nx, ny) of the offset grid over the box and its margin."""
    lon_a, lon_b, lat_a, lat_b = box[0] - MARGIN, box[1] + MARGIN, box[2] - MARGIN, box[3] + MARGIN
    dlon, dlat = (lon_b - lon_a) / nx, (lat_b - lat_a) / ny
    if south_to_north:
        return lon_a + 0.37 * dlon, lat_a + 0.41 * dlat, dlon, dlat, nx, ny
    return lon_a + 0.37 * dlon, lat_b - 0.41 * dlat, dlon, -dlat, nx, ny


def grid_points(grid):
    """The targets of a grid, row by row: one rounded product and one rounded sum each, as the kernel forms them."""
    lon0, lat0, dlon, dlat, nx, ny = grid
    lon = np.float64(lon0) + np.arange(nx, dtype=np.float64) * np.float64(dlon)
    lat = np.float64(lat0) + np.arange(ny, dtype=np.float64) * np.float64(dlat)
    return np.stack(np.broadcast_arrays(lon[None, :], lat[:, None]), axis=-1).reshape(-1, 2)


def centre_observer(box, height=4000.0, above_terrain=True):
    return observer_records(0.5 * (box[0] + box[1]) + 0.013, 0.5 * (box[2] + box[3]) + 0.017, height, above_terrain)


LOW = {"antimeridian": 150.0, "north84": 250.0, "polar": 150.0}


def _placement(ts, south_to_north=False):
    """A 24 x 20 grid over tiles off the 45N 15E quadrant, from low above the ground (ground that faces away, hidden ground; lower
    still, the sight lines graze the smooth relief and the reference calls more than 0.5 % of the targets ambiguous) and from 4000 m."""
    box = tileset(ts)[2]
    return _grid_case(ts, 24, 20, obs=np.concatenate([centre_observer(box, LOW[ts]), centre_observer(box, 4000.0)]), south_to_north=south_to_north)


def _grid_case(ts, nx, ny, obs=None, h=0.0, south_to_north=False):
    tiles, order, box = tileset(ts)
    grid = box_grid(box, nx, ny, south_to_north)
    return dict(tileset=ts, tiles=tiles, order=order, obs=centre_observer(box) if obs is None else obs, grid=grid, lonlat=grid_points(grid), h=h)


def _summit(h):
    """ridges_ne's grid seen from 2 m over its highest target."""
    base = case("ridges_ne")
    rec = VR.SR.surface(meshes("ridges_ne").surface, base["lonlat"])
    top = np.argmax(np.where(rec["kind"] == VR.SR.TERRAIN, rec["height_m"], -np.inf))
    return dict(base, obs=observer_records(base["lonlat"][top, 0], base["lonlat"][top, 1], 2.0), h=h, summit=int(top))


def _void():
    """The NaN-patterned relief from high above (no sight line is blocked: every terrain target VISIBLE, every void NONE) and from a low
    observer, whose sight lines pass over -- and through -- the voids."""
    tiles, order, box = tileset("void_nan")
    pts = grid_points(box_grid(box, 40, 36))
    rec = VR.SR.surface(meshes("void_nan").surface, pts)
    far = np.where(rec["kind"] == VR.SR.TERRAIN, np.hypot(pts[:, 0] - 16.31, pts[:, 1] - 45.79), np.inf)
    at = pts[np.argmin(far)]      # the terrain target nearest to (16.31, 45.79)
    return _grid_case("void_nan", 40, 36, obs=np.concatenate([centre_observer(box, 4000.0, False), observer_records(at[0], at[1], 800.0)]))


def _observers():
    """ridges_ne from observers of every kind over a list: every seventh grid target, invalid targets and targets without terrain, and
    the points two observers stand on."""
    base = case("ridges_ne")
    at = base["lonlat"][[411, 702]]
    tiles, order, box = tileset("ridges_ne")
    good = centre_observer(box, 4000.0, False)
    obs = np.concatenate([
        good,
        observer_records(np.nan, 46.0, 10.0),                          # 1: invalid point
        observer_records(16.0, 95.0, 10.0),                            # 2: latitude out of range
        observer_records(16.2, 46.2, np.nan),                          # 3: no height
        observer_records(16.2, 46.2, np.inf, above_terrain=False),     # 4: infinite height
        observer_records(3.0, 2.0, 10.0),                              # 5: above terrain, but none there
        observer_records(3.0, 2.0, 300000.0, above_terrain=False),     # 6: over the sphere, far away: usable
        observer_records(16.013, 46.017, 9000.0, above_terrain=False), # 7: over the sphere, above the mosaic
        observer_records(at[0, 0], at[0, 1], 0.0),                     # 8: on the ground at target `at0`
        observer_records(at[1, 0], at[1, 1], 1.0e-3),                  # 9: a millimetre over target `at1`
        observer_records(16.4, 46.3, -50.0),                           # 10: underground
    ])
    extra = np.array([[np.nan, 46.0], [16.0, np.inf], [16.0, 90.5], [16.0, -91.0], [3.0, 2.0], [-164.0, -46.0], [15.5, 90.0]])
    lonlat = np.concatenate([base["lonlat"][::7], extra, at])
    n = len(lonlat)
    return dict(tileset="ridges_ne", tiles=tiles, order=order, obs=obs, grid=None, lonlat=lonlat, h=0.0, unusable=[1, 2, 3, 4, 5], extra=slice(n - 9, n - 2),
                at=(n - 2, n - 1))


def _posts():
    """Targets on exact DEM posts and on tile borders of ridges_ne: a sight line that starts on an edge or a vertex.  Compared only
    between the emulation and its every-triangle loop."""
    tiles, order, box = tileset("ridges_ne")
    k = np.arange(0, 32, 3, dtype=np.float64)
    P = []
    for lat, lon in order:
        glon, glat = np.meshgrid(lon + k / 32.0, lat + 1 - k / 32.0)
        P.append(np.stack([glon.reshape(-1), glat.reshape(-1)], axis=1))
    s = 15.0 + 2.0 * (np.arange(25) + 0.29) / 25
    for v in (15.0, 16.0, 16.0 - 1.0 / 32.0, 17.0 - 1.0 / 32.0):      # the first and last column of a tile
        P.append(np.stack([np.full(25, v), s + 30.0], axis=1))
    for v in (47.0, 46.0, 46.0 + 1.0 / 32.0, 45.0 + 1.0 / 32.0):      # the first and last row of a tile
        P.append(np.stack([s, np.full(25, v)], axis=1))
    return dict(tileset="ridges_ne", tiles=tiles, order=order, obs=centre_observer(box, 4000.0, False), grid=None, lonlat=np.concatenate(P), h=0.0)


BALANCED = ("ridges_ne", "blocks", "long")
RIDGE_SCENES = ("ridges_ne", "summit_h0")
CASES = {"ridges_ne": lambda: _grid_case("ridges_ne", 40, 36, obs=centre_observer((15.0, 17.0, 45.0, 47.0), 4000.0, False)), "blocks": lambda: _grid_case("blocks", 48, 30), "long": lambda: _grid_case("long", 60, 20),
         "summit_h0": lambda: _summit(0.0), "summit_h30": lambda: _summit(30.0), "void_nan": _void,
         "antimeridian": lambda: _placement("antimeridian"), "north84": lambda: _placement("north84"), "polar": lambda: _placement("polar", south_to_north=True),
         "observers": _observers}
NO_REFERENCE = {"posts": _posts}


def case(name):
    if name not in _CASES:
        _CASES[name] = (CASES.get(name) or NO_REFERENCE[name])()
    return _CASES[name]


def reference(name, h=None):
    """(classes, ambiguous) of the case by visibility_ref, at the case's target height or at h; computed once."""
    c = case(name)
    h = c["h"] if h is None else h
    key = (c["tileset"], c["obs"].tobytes(), c["lonlat"].tobytes(), h)      # (the summit cases share their runs)
    if key not in _REF:
        _REF[key] = VR.visibility(meshes(c["tileset"]), c["obs"], c["lonlat"], h)
    return _REF[key]


def emulation(name, brute=False, h=None):
    """(classes, resolved observers) of the case by the g++ build, the traversal or (brute) every triangle; computed once."""
    c = case(name)
    h = c["h"] if h is None else h
    key = (c["tileset"], c["obs"].tobytes(), c["lonlat"].tobytes(), h, brute)
    if key not in _EMU:
        cls, eyes, bad = VE.visibility(c["tiles"], c["order"], c["obs"], c["lonlat"], h, brute)
        assert bad == 0, f"{name}: {bad} index checks failed in the emulation"
        _EMU[key] = (cls, eyes)
    return _EMU[key]


def counts(cls):
    return tuple(int((cls == k).sum()) for k in range(5))
