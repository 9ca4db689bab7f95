"""Scenes, grids and contour parameters of the map-view tests (tests/test_map_cpu.py, tests/test_map_gpu.py): the smallest at which
the rule and the wave form of topo_map.h can go wrong.  The tile sets are those of tests/surface_cases.py; the normals are the
oracle's (OracleRenderer.read_normals); the masks are seeded random bits, all zero or all one.  A case's emulations and its
reference are computed once and shared.

Grids are small because the emulation's plain loop looks up every pixel and both neighbours over every triangle of every tile.  They
are 66 to 70 columns wide (a full wave, a wave edge and a tail with its east halo across the waves) and R + 2 rows high (a full band,
its south halo, a short band), with steps that are no fraction of a DEM post, so that no pixel lies on a mesh edge."""
from __future__ import annotations

import numpy as np

import map_emul as ME
import map_ref as MR
import surface_cases as SC
import topo_renderer_amd as T
from oracle import oracle as O

R = ME.rows_per_wave()
ALL = T.MAP_RELIEF | T.MAP_CONTOURS | T.MAP_SEEN
_TILES, _NORMALS, _RUN, _REF = {}, {}, {}, {}


def tile_set(name):
    """(tiles in draw order, their (lat, lon)) of surface case `name`."""
    if name not in _TILES:
        tiles, order, _, _ = SC.case(name)
        _TILES[name] = (tiles, order)
    return _TILES[name]


def oracle_normals(tiles, order):
    o = O.OracleRenderer(64, 48)
    for (lat, lon), t in zip(order, tiles):
        o.add_terrain(lat, lon, *t)
    h, w = tiles[0][0].shape
    return [o.read_normals(lat, lon, w, h).copy() for lat, lon in order]


def normals(name):
    if name not in _NORMALS:
        _NORMALS[name] = oracle_normals(*tile_set(name))
    return _NORMALS[name]


def masks(name, kind="random", seed=7):
    """A (h - 1, w - 1) bool mask per tile: seeded random bits, or None ("none"), all zero, all one."""
    tiles, _ = tile_set(name)
    h, w = tiles[0][0].shape
    if kind == "none":
        return None
    if kind in ("zero", "one"):
        return [np.full((h - 1, w - 1), kind == "one") for _ in tiles]
    rng = np.random.default_rng(seed)
    return [rng.random((h - 1, w - 1)) < 0.5 for _ in tiles]


def sun(lon, lat):
    """The conventional north-west light at (lon, lat), as the f32 triple of topo_map_params."""
    return T.sun_direction(lon, lat, 315.0, 45.0).astype(np.float32)


def grid(lon_a, lon_b, lat_a, lat_b, nx, ny):
    """Pixel (0, 0) at (lon_a, lat_a), pixel (nx - 1, ny - 1) at (lon_b, lat_b)."""
    return dict(lon0=lon_a, lat0=lat_a, dlon=(lon_b - lon_a) / max(nx - 1, 1), dlat=(lat_b - lat_a) / max(ny - 1, 1), nx=nx, ny=ny)


# name -> (tile set, grid, contour interval, index_every, layers, masks)
CASES = {
    # the 130 x 34 ragged tile (7E .. 7.992E, 46.03N .. 47N): a grid coarser than the DEM that starts outside the mosaic, rows going south
    "blocks_coarse": ("blocks", grid(6.9713, 8.0231, 47.0117, 46.0021, 70, R + 2), 50.0, 5, ALL, "random"),
    # finer than the DEM: many pixels share a triangle
    "blocks_fine": ("blocks", grid(7.40013, 7.43021, 46.50017, 46.49211, 68, R + 2), 5.0, 5, ALL, "random"),
    # negative dlon and positive dlat: columns go west, rows north
    "blocks_reversed": ("blocks", grid(7.9013, 7.0231, 46.1117, 46.9021, 66, R + 2), 50.0, 1, ALL, "random"),
    # dlon = 0: every column the same longitude, no east contours
    "blocks_dlon0": ("blocks", dict(lon0=7.41317, lat0=46.9313, dlon=0.0, dlat=-0.0113, nx=66, ny=R + 2), 25.0, 0, ALL, "random"),
    # the 1 x 3 mosaic with a one-cell gap between neighbours; waves straddle a seam and a gap
    "long_gap": ("long", grid(5.9013, 6.1131, 44.9713, 44.5321, 70, R + 2), 100.0, 5, ALL, "random"),
    "overlap_higher": ("overlap_higher", grid(15.3113, 15.8931, 45.9713, 45.4321, 70, R + 2), 20.0, 5, ALL, "random"),
    "overlap_equal": ("overlap_equal", grid(15.3113, 15.8931, 45.9713, 45.4321, 68, R + 2), 20.0, 5, ALL, "random"),
    "void_nan": ("void_nan", grid(15.0113, 16.9931, 46.9713, 45.0321, 66, R + 2), 100.0, 5, ALL, "random"),
    "sentinels": ("sentinels", grid(15.1113, 15.8931, 45.9313, 45.1321, 66, 3 * R + 2), 1000.0, 5, ALL, "random"),      # the -32768 pit: negative heights and levels; rows close enough to cross it
    "antimeridian": ("antimeridian", grid(179.5113, 180.4931, 10.9713, 10.0321, 70, R + 2), 100.0, 5, ALL, "random"),      # longitudes beyond 180
    "antimeridian_wrapped": ("antimeridian", grid(-180.4887, -179.5069, 10.9713, 10.0321, 70, R + 2), 100.0, 5, ALL, "random"),
    "north84": ("north84", grid(19.9713, 22.0231, 84.9917, 84.0121, 66, R + 2), 100.0, 5, ALL, "random"),
    "polar": ("polar", grid(19.9113, 22.0931, 89.9913, 89.0121, 66, R + 2), 100.0, 5, ALL, "random"),
    "polar_far_side": ("polar", grid(-160.0887, -157.9069, 89.0121, 89.9987, 66, R + 2), 100.0, 5, ALL, "random"),      # rows going north, to 150 m from the pole
    # contour parameters and layers on the small overlap tiles
    "steep_small_interval": ("overlap_higher", grid(15.0313, 16.1931, 45.9813, 45.3121, 66, R + 2), 4.0, 5, ALL, "random"),      # levels differ by more than one
    "huge_interval": ("overlap_higher", grid(15.3113, 15.8931, 45.9713, 45.4321, 66, R + 2), 1.0e6, 5, ALL, "random"),      # no contour exists
    "index_0": ("overlap_higher", grid(15.3113, 15.8931, 45.9713, 45.4321, 66, R + 2), 20.0, 0, ALL, "random"),
    "index_1": ("overlap_higher", grid(15.3113, 15.8931, 45.9713, 45.4321, 66, R + 2), 20.0, 1, ALL, "random"),
    "relief_only": ("overlap_higher", grid(15.3113, 15.8931, 45.9713, 45.4321, 66, R + 2), 20.0, 5, T.MAP_RELIEF, "random"),
    "contours_only": ("overlap_higher", grid(15.3113, 15.8931, 45.9713, 45.4321, 66, R + 2), 20.0, 5, T.MAP_CONTOURS, "random"),
    "seen_only": ("overlap_higher", grid(15.3113, 15.8931, 45.9713, 45.4321, 66, R + 2), 20.0, 5, T.MAP_SEEN, "random"),
    "no_layer": ("overlap_higher", grid(15.3113, 15.8931, 45.9713, 45.4321, 66, R + 2), 20.0, 5, 0, "random"),
    "masks_zero": ("overlap_higher", grid(15.3113, 15.8931, 45.9713, 45.4321, 66, R + 2), 20.0, 5, ALL, "zero"),
    "masks_one": ("overlap_higher", grid(15.3113, 15.8931, 45.9713, 45.4321, 66, R + 2), 20.0, 5, ALL, "one"),
    "masks_none": ("overlap_higher", grid(15.3113, 15.8931, 45.9713, 45.4321, 66, R + 2), 20.0, 5, ALL, "none"),
}


def params(name):
    ts, g, interval, every, layers, _ = CASES[name]
    lon_c, lat_c = g["lon0"] + 0.5 * (g["nx"] - 1) * g["dlon"], g["lat0"] + 0.5 * (g["ny"] - 1) * g["dlat"]
    return T.map_params(g["lon0"], g["lat0"], g["dlon"], g["dlat"], g["nx"], g["ny"], sun_direction=sun(lon_c, min(lat_c, 90.0)), contour_interval_m=interval,
                        index_every=every, layers=layers, void_rgba=(10, 20, 30, 40), seen_rgba=(255, 208, 0, 96), contour_rgba=(96, 64, 32, 160),
                        index_rgba=(64, 32, 16, 255))


def run(name, mode):
    """The emulation of case `name` in `mode` (ME.WAVES, ME.ALL_TILES, ME.BRUTE): (rgba, flags, failed checks, stats), computed once."""
    if (name, mode) not in _RUN:
        ts = CASES[name][0]
        tiles, _ = tile_set(ts)
        _RUN[(name, mode)] = ME.run(tiles, normals(ts), params(name), masks(ts, CASES[name][5]), mode)
    return _RUN[(name, mode)]


def reference(name):
    if name not in _REF:
        ts = CASES[name][0]
        tiles, _ = tile_set(ts)
        _REF[name] = MR.reference(tiles, normals(ts), params(name), masks(ts, CASES[name][5]))
    return _REF[name]


# ---- hand-known tiles ------------------------------------------------------------------------------------------------------------
POST = 1.0 / 512.0      # degrees between the posts of a hand-known tile: exact in f32, and 217 m, so that a cell's flat triangles sag a millimetre under the sphere
UP_TEXEL = (128, 128, 255, 0)      # a normal along the tile's own up axis


def small_tile(heights, lat=45, lon=15.0):
    """One tile of the given heights, post (0, 0) at (lon, lat + 1), POST degrees between posts -> (tiles, order)."""
    hts = np.ascontiguousarray(heights, np.float32)
    return [(hts, np.float32([0.0, 0.0]), np.float32([lon, lat + 1.0]), np.float32([POST, POST]))], [(lat, int(np.floor(lon)))]


def flat_normals(tiles):
    return [np.broadcast_to(np.uint8(UP_TEXEL), t[0].shape + (4,)).copy() for t in tiles]


def cell_grid(tile, x_a, x_b, y_a, y_b, nx, ny):
    """A grid whose pixel (0, 0) lies at (x_a, y_a) and pixel (nx - 1, ny - 1) at (x_b, y_b) in the tile's cell coordinates."""
    _, rp, mp, ps = tile
    lon = lambda x: float(mp[0]) + x * float(ps[0])
    lat = lambda y: float(mp[1]) - y * float(ps[1])
    return grid(lon(x_a), lon(x_b), lat(y_a), lat(y_b), nx, ny)
