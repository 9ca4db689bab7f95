"""Scenes and rays of the ray-query tests (tests/test_raycast_cpu.py, tests/test_raycast_gpu.py): the smallest at which the traversal
of topo_los.h can go wrong.  A case is (tiles in draw order, their (lat, lon), rays); its reference answer (los_ref.cast) is computed
once and shared."""
from __future__ import annotations

import math

import numpy as np

import los_ref as LR
import topo_renderer_amd as T
from oracle import ray_check as RC
from scenes import Scene, relief

R0 = LR.R0
RAY_DTYPE = np.dtype([("origin", "<f8", 3), ("dir", "<f8", 3), ("t_min", "<f8"), ("t_max", "<f8")])
SUN_AZ, SUN_EL = 120.0, 8.0


def make_rays(origin, direction, t_min=0.0, t_max=1.0e6):
    o, d = np.broadcast_arrays(np.atleast_2d(np.asarray(origin, np.float64)), np.atleast_2d(np.asarray(direction, np.float64)))
    out = np.zeros(len(o), RAY_DTYPE)
    out["origin"], out["dir"], out["t_min"], out["t_max"] = o, d, t_min, t_max
    return out


def ecef(lon_deg, lat_deg, height):
    lo, la = np.radians(lon_deg), np.radians(lat_deg)
    r = R0 + np.asarray(height, np.float64)
    return np.stack(np.broadcast_arrays(r * np.cos(la) * np.cos(lo), r * np.cos(la) * np.sin(lo), r * np.sin(la)), axis=-1)


def up_at(lon_deg, lat_deg):
    return ecef(lon_deg, lat_deg, 1.0 - R0)


def ridges(lat, lon):
    return 2000.0 + 1800.0 * np.sin(np.radians(1400.0 * lon)) * np.cos(np.radians(900.0 * lat)) + 0.0 * (lat + lon)


def scene_tiles(sc):
    """(tiles in draw order, their (lat, lon)) of a scenes.Scene."""
    order = LR.geo_order(sc.locs)
    return [(sc.heights[loc],) + tuple(sc.transform(loc)) for loc in order], order


def eye_rays(sc, W, H, yaw_deg, pitch_deg, fov_deg):
    """The pixel-centre rays of the view, from the eye (the camera of oracle/ray_check.py; dir not normalised: t = view depth)."""
    eye = np.asarray(sc.eye, np.float64)
    f, s, u = RC.camera_basis(eye, math.radians(yaw_deg), math.radians(pitch_deg))
    th = math.tan(0.5 * math.radians(fov_deg))
    gx, gy = np.meshgrid((np.arange(W) + 0.5) / W * 2.0 - 1.0, 1.0 - (np.arange(H) + 0.5) / H * 2.0)
    D = f[None, :] + (gx.reshape(-1, 1) * th * W / H) * s[None, :] + (gy.reshape(-1, 1) * th) * u[None, :]
    return make_rays(eye, D)


RIDGES = {
    "ridges_ne": (dict(tile=32, n_lat=2, n_lon=2, eye_dh=6000.0), 96, 64, (30.0, 25.0, 60.0)),
    "ridges_sw": (dict(tile=24, n_lat=2, n_lon=2, lat0=-34, lon0=-71, eye_dh=8000.0), 64, 48, (200.0, 35.0, 79.28)),
}
_CACHE = {}


def _ridges_case(name):
    kw, W, H, pose = RIDGES[name]
    sc = Scene(height_fn=ridges, **kw)
    tiles, order = scene_tiles(sc)
    eye = eye_rays(sc, W, H, *pose)
    mesh = LR.Mesh(tiles)
    first = LR.cast(mesh, eye)
    hit = first["kind"] == LR.HIT
    pts = eye["origin"][hit] + first["t"][hit, None] * eye["dir"][hit]
    sun = make_rays(pts, LR.sun_direction(sc.vlon, sc.vlat, SUN_AZ, SUN_EL), 1.0e-3, 1.0e6)      # from each hit point towards the sun
    rays = np.concatenate([eye, sun])
    return tiles, order, rays, np.concatenate([first, LR.cast(mesh, sun)])


def _blocks_case():
    """One tile of 130 x 34 vertices: 3 block columns (60 + 60 + 9 cells) and 3 block rows (15 + 15 + 3)."""
    lat, lon, w, h = 46, 7, 130, 34
    x, y = np.arange(w) / w, np.arange(h) / h
    la, lo = (lat + 1 - y)[:, None], (lon + x)[None, :]
    hts = (1500.0 + 1200.0 * np.sin(np.radians(2300.0 * lo)) * np.cos(np.radians(1700.0 * la)) + 400.0 * np.sin(np.radians(7000.0 * (lo + la)))).astype(np.float32)
    tiles, order = [(hts,) + tuple(T.synth.tile_transform(lat, lon, w, h))], [(lat, lon)]
    rng = np.random.default_rng(11)
    R = []
    glon, glat = np.meshgrid(lon + (np.arange(24) + 0.37) / 24.5, lat + (np.arange(20) + 0.41) / 20.5)
    glon, glat = glon.reshape(-1), glat.reshape(-1)
    n = len(glon)
    top = ecef(glon, glat, 9000.0)
    aim = ecef(glon + rng.uniform(-0.2, 0.2, n), glat + rng.uniform(-0.2, 0.2, n), 0.0)
    R.append(make_rays(top, aim - top, 0.0, 4.0))                                     # grid rays from above, slanted, non-unit
    for hgt in (400.0, 1500.0, 2600.0, 3400.0):                                       # along a meridian and a parallel, between hmin and hmax of the blocks
        k = 30
        a = ecef(lon + (np.arange(k) + 0.5) / k, lat + 1.05, hgt)
        b = ecef(lon + (np.arange(k) + 0.5) / k + 0.013, lat - 0.05, hgt)
        R.append(make_rays(a, b - a, 0.0, 1.0))
        a = ecef(lon - 0.05, lat + (np.arange(k) + 0.5) / k, hgt)
        b = ecef(lon + 1.05, lat + (np.arange(k) + 0.5) / k + 0.007, hgt)
        R.append(make_rays(a, b - a, 0.0, 1.0))
        R.append(make_rays(b, a - b, 0.0, 1.0))
    nad = ecef(glon[::3], glat[::3], 12000.0)
    upv = up_at(glon[::3], glat[::3])
    R.append(make_rays(nad, -upv, 0.0, 1.0e6))                                        # nadir
    R.append(make_rays(nad, upv, 0.0, 1.0e6))                                         # zenith: miss
    under = ecef(glon[1::3], glat[1::3], -3000.0)
    R.append(make_rays(under, up_at(glon[1::3], glat[1::3]) + 0.05 * rng.standard_normal((len(under), 3)), 0.0, 1.0e6))      # from underground: back faces
    rays = np.concatenate(R)
    mesh = LR.Mesh(tiles)
    first = LR.cast(mesh, rays)
    # a t_max short of the first hit (miss) and a t_min beyond it (the second hit, if any)
    hit = np.nonzero(first["kind"] == LR.HIT)[0][::5]
    short, beyond = rays[hit].copy(), rays[hit].copy()
    short["t_max"] = first["t"][hit] * 0.999
    beyond["t_min"] = first["t"][hit] * 1.001
    extra = np.concatenate([short, beyond])
    return tiles, order, np.concatenate([rays, extra]), np.concatenate([first, LR.cast(mesh, extra)])


def _long_case():
    """A 1 x 3 mosaic of 48-vertex tiles; low rays from end to end across the tiles and the gaps between them (a tile's last column
    stops 1/48 degree short of its neighbour: a ray through a gap must pass)."""
    sc = Scene(48, 1, 3, lat0=44, lon0=5, height_fn=lambda la, lo: 900.0 + 700.0 * np.sin(np.radians(2100.0 * lo)) * np.cos(np.radians(1300.0 * la)) + 0.0 * (la + lo))
    tiles, order = scene_tiles(sc)
    k = 40
    lats = 44.0 + (np.arange(k) + 0.5) / k
    R = []
    for h0, h1 in ((1500.0, 1200.0), (2500.0, 300.0), (800.0, 800.0), (5000.0, -2000.0)):
        a, b = ecef(4.9, lats, h0), ecef(8.1, lats + 0.011, h1)
        R.append(make_rays(a, b - a, 0.0, 1.0))
        R.append(make_rays(b, a - b, 0.0, 1.0))
    gap = ecef(5.0 + 47.5 / 48.0 + np.array([0.0, 1.0])[:, None], lats[None, ::4], 9000.0).reshape(-1, 3)      # straight down the two gaps
    R.append(make_rays(gap, -gap / np.linalg.norm(gap, axis=1)[:, None], 0.0, 1.0e6))
    rays = np.concatenate(R)
    return tiles, order, rays, LR.cast(LR.Mesh(tiles), rays)


def _void_case():
    """void_scenes' ne_2x2 relief with the NaN pattern: eye rays (those aimed at a void pass through it and report what lies behind)."""
    import void_scenes as VS
    sc, void, W, H, pose = VS.relief_case("ne_2x2", "nan")
    tiles, order = scene_tiles(void)
    k = 24
    lats = 45.0 + 2.0 * (np.arange(k) + 0.5) / k
    low = []
    for h0, h1 in ((2600.0, 400.0), (1800.0, 1700.0), (3200.0, -500.0)):      # low across the ridges: behind a void lies the next slope
        a, b = ecef(14.9, lats, h0), ecef(17.1, lats + 0.017, h1)
        low += [make_rays(a, b - a, 0.0, 1.0), make_rays(b, a - b, 0.0, 1.0)]
    rays = np.concatenate([eye_rays(sc, W, H, *pose[:3])] + low)
    return tiles, order, rays, LR.cast(LR.Mesh(tiles), rays)


def _void_inf_case():
    import void_scenes as VS
    sc, void, W, H, pose = VS.relief_case("ne_2x2", "pinf")
    tiles, order = scene_tiles(void)
    rays = eye_rays(sc, W, H, *pose[:3])[::3]
    return tiles, order, rays, LR.cast(LR.Mesh(tiles), rays)


CASES = {"ridges_ne": lambda: _ridges_case("ridges_ne"), "ridges_sw": lambda: _ridges_case("ridges_sw"), "blocks": _blocks_case, "long": _long_case,
         "void_nan": _void_case, "void_pinf": _void_inf_case}


# ---- off the 45N 15E quadrant: across the equator, the prime meridian, the antimeridian and the pole -----------------------------------
geo_relief = relief


def placed_tiles(locs, n, height_fn=geo_relief):
    """(tiles in draw order, their (lat, lon)) of square n-vertex tiles at explicit locations (Scene cannot name tile -180)."""
    x = np.arange(n, dtype=np.float64) / n
    order = LR.geo_order(locs)
    return [(np.ascontiguousarray(height_fn((la + 1 - x)[:, None], (lo + x)[None, :]), dtype=np.float32),) + tuple(T.synth.tile_transform(la, lo, n, n))
            for la, lo in order], order


def _geo_rays(lat0, lat1, lon0, lon1, seed, meridians=None, k=14):
    """The standard set over the box [lat0, lat1] x [lon0, lon1] (longitudes may run past 180: ecef takes them as they come): low rays
    both ways along parallels and along meridians between the relief's lowest (100 m) and highest (2900 m) point, slanted rays from
    above, zenith rays (misses) and rays whose t_max ends above the ground (misses)."""
    rng = np.random.default_rng(seed)
    R = []
    lats = lat0 + (lat1 - lat0) * (np.arange(k) + 0.5) / k
    lons = lon0 + (lon1 - lon0) * (np.arange(k) + 0.5) / k if meridians is None else np.asarray(meridians, np.float64)
    dlat = 0.05 if lat1 + 0.05 < 90.0 and lat0 - 0.05 > -90.0 else 0.0
    for hgt in (600.0, 1500.0, 2400.0):
        a, b = ecef(lon0 - 0.1, lats, hgt), ecef(lon1 + 0.1, lats + 0.007, hgt)
        R += [make_rays(a, b - a, 0.0, 1.0), make_rays(b, a - b, 0.0, 1.0)]
        a, b = ecef(lons, lat1 + dlat, hgt), ecef(lons + 0.013, lat0 - dlat, hgt)
        R += [make_rays(a, b - a, 0.0, 1.0), make_rays(b, a - b, 0.0, 1.0)]
    return np.concatenate(R + _overhead_rays(lat0, lat1, lon0, lon1, rng))


def _overhead_rays(lat0, lat1, lon0, lon1, rng):
    glon, glat = np.meshgrid(lon0 + (lon1 - lon0) * (np.arange(9) + 0.37) / 9.5, lat0 + (lat1 - lat0) * (np.arange(8) + 0.41) / 8.5)
    glon, glat = glon.reshape(-1), glat.reshape(-1)
    n = len(glon)
    top = ecef(glon, glat, 9000.0)
    aim = ecef(glon + rng.uniform(-0.2, 0.2, n), np.clip(glat + rng.uniform(-0.2, 0.2, n), -89.99, 89.99), 0.0)
    return [make_rays(top, aim - top, 0.0, 4.0),                               # slanted from above, non-unit
            make_rays(top[::2], up_at(glon[::2], glat[::2]), 0.0, 1.0e6),      # zenith: miss
            make_rays(top[1::2], aim[1::2] - top[1::2], 0.0, 0.4)]             # ends 5000 m up: miss


def _antimeridian_case(lat):
    """Two 48-vertex tiles either side of the antimeridian: parallels from 178.9E to 178.9W and back, meridians from 179.5E to 179.5W
    (none on the meridian itself: a hit there may report +180 or -180)."""
    tiles, order = placed_tiles([(lat, 179), (lat, -180)], 48)
    meridians = np.concatenate([179.53 + 0.1 * np.arange(5), 180.03 + 0.1 * np.arange(5)])
    rays = _geo_rays(float(lat), lat + 1.0, 179.0, 181.0, 21 + abs(lat), meridians)
    return tiles, order, rays, LR.cast(LR.Mesh(tiles), rays)


def _origin_case():
    tiles, order = placed_tiles([(0, 0), (-1, 0), (0, -1), (-1, -1)], 32)
    rays = _geo_rays(-1.0, 1.0, -1.0, 1.0, 23)
    return tiles, order, rays, LR.cast(LR.Mesh(tiles), rays)


def _high_latitude_case(lat, lon):
    tiles, order = placed_tiles([(lat, lon), (lat, lon + 1)], 48)
    rays = _geo_rays(float(lat), lat + 1.0, float(lon), lon + 2.0, 25 + abs(lat))
    return tiles, order, rays, LR.cast(LR.Mesh(tiles), rays)


def _polar_case():
    """Four 32-vertex tiles whose row 0 is the north pole, two on either side of it: rays from 88.9N over the pole to 88.9N on the
    opposite longitude and back (2.5 to 4 km up at their ends: the chord dips 1.2 km towards the pole), rays along parallels between
    89N and 89.98N, rays past the pole whose latitude peaks over the tiles (the t_e term of los_cell_range), and the slanted, zenith and short rays of the standard set over either pair."""
    tiles, order = placed_tiles([(89, 20), (89, 21), (89, -160), (89, -159)], 32)
    k = 16
    lons = 20.0 + 2.0 * (np.arange(k) + 0.5) / k
    R = []
    for hgt in (2500.0, 3000.0, 3500.0, 4000.0):
        a, b = ecef(lons, 88.9, hgt), ecef(lons - 180.0 + 0.013, 88.9, hgt)
        R += [make_rays(a, b - a, 0.0, 1.0), make_rays(b, a - b, 0.0, 1.0)]
    lats = 89.0 + 0.98 * (np.arange(k) + 0.5) / k
    for west in (20.0, -160.0):
        for hgt in (900.0, 1500.0, 2100.0):
            a, b = ecef(west - 0.1, lats, hgt), ecef(west + 2.1, lats + 0.003, hgt)
            R += [make_rays(a, b - a, 0.0, 1.0), make_rays(b, a - b, 0.0, 1.0)]
    # past the pole, 9 to 100 km from it, square to the meridian of the closest point C: the latitude peaks inside every interval
    colat = np.repeat(0.08 + 0.82 * (np.arange(8) + 0.5) / 8, 4)
    lonc = np.tile([20.5, 21.5, -159.5, -158.5], 8)
    east = np.stack([-np.sin(np.radians(lonc)), np.cos(np.radians(lonc)), 0.0 * lonc], axis=-1)
    for hgt in (1100.0, 1700.0):
        c, up = ecef(lonc, 90.0 - colat, hgt), up_at(lonc, 90.0 - colat)
        a, b = c - 60000.0 * east + 900.0 * up, c + 60000.0 * east - 700.0 * up
        R += [make_rays(a, b - a, 0.0, 1.0), make_rays(b, a - b, 0.0, 1.0)]
    for west, seed in ((20.0, 31), (-160.0, 32)):
        R += _overhead_rays(89.0, 89.98, west, west + 2.0, np.random.default_rng(seed))
    rays = np.concatenate(R)
    return tiles, order, rays, LR.cast(LR.Mesh(tiles), rays)


# ---- tiles of more than 64 raster blocks: the wave-per-ray kernel takes the blocks of a tile 64 at a time ----------------------------------
BATCH = 64      # blocks per batch of k_raycast
BLOCK_CX, BLOCK_CY = 60, 15      # cells of a raster block
BATCH_TILES = {"tall": (61, 964), "grid": (301, 250)}      # (w, h) vertices: 1 x 65 blocks (the 65th of 3 cell rows); 5 x 17 blocks (the last row partial)
_BLOCKS_BASE = 1320      # the rays of _blocks_case before its short / beyond copies


def blocks_heights(lat, lon, w, h):
    """The relief of _blocks_case sampled at w x h vertices of the tile (lat, lon)."""
    la, lo = (lat + 1 - np.arange(h) / h)[:, None], (lon + np.arange(w) / w)[None, :]
    return (1500.0 + 1200.0 * np.sin(np.radians(2300.0 * lo)) * np.cos(np.radians(1700.0 * la)) + 400.0 * np.sin(np.radians(7000.0 * (lo + la)))).astype(np.float32)


def block_of(cell_x, cell_y, w):
    """The raster block of a cell, numbered as k_raycast numbers them."""
    return (np.asarray(cell_y, np.int64) // BLOCK_CY) * (-(-(w - 1) // BLOCK_CX)) + np.asarray(cell_x, np.int64) // BLOCK_CX


def _surface(hts, lat, lon, la, lo):
    """The height of the nearest vertex of the tile at (la, lo)."""
    h, w = hts.shape
    j = np.clip(np.rint((lat + 1 - np.asarray(la)) * h), 0, h - 1).astype(int)
    i = np.clip(np.rint((np.asarray(lo) - lon) * w), 0, w - 1).astype(int)
    return hts[j, i].astype(np.float64)


def aimed_rays(hts, lat, lon, k, seed):
    """Rays into the last block row of the tile: slanted from above, and along the meridian from the south (from 0.01 degrees outside
    the tile, descending 300 to 900 m to a point 40 m under the surface of the row, and on across the whole tile) and from the north
    (from 0.15 degrees inside the tile, descending 1500 m).  -> (rays, the indices of the meridional ones)."""
    rng = np.random.default_rng(seed)
    h, w = hts.shape
    rows = ((h - 2) // BLOCK_CY) * BLOCK_CY                                  # the first cell row of the last block row
    la = lat + 1 - rng.uniform(rows + 0.3, h - 1.3, 3 * k) / h
    lo = lon + rng.uniform(0.02, (w - 1.5) / w, 3 * k)
    tgt = ecef(lo, la, _surface(hts, lat, lon, la, lo) - 40.0)
    top = ecef(lo[:k] + rng.uniform(-0.05, 0.05, k), la[:k] + rng.uniform(0.0, 0.05, k), 9000.0)
    south = ecef(lo[k:2 * k] - 0.001, lat - 0.01, _surface(hts, lat, lon, la[k:2 * k], lo[k:2 * k]) + rng.uniform(300.0, 900.0, k))
    north = ecef(lo[2 * k:] - 0.004, la[2 * k:] + 0.15, _surface(hts, lat, lon, la[2 * k:], lo[2 * k:]) + 1500.0)
    span = 1.1 / (la[k:2 * k] - (lat - 0.01))                                # t at which the ray from the south leaves the tile in the north
    rays = np.concatenate([make_rays(top, tgt[:k] - top, 0.0, 2.0), make_rays(south, tgt[k:2 * k] - south, 0.0, span),
                           make_rays(north, tgt[2 * k:] - north, 0.0, 3.0)])
    return rays, np.arange(k, 3 * k)


def batch_rays(hts, lat, lon, stride, k, seed):
    """The rays of _blocks_case (the same degree), every stride-th and its 30 meridional rays at 2600 m, the full-length meridional
    ones among them; then the aimed rays.  -> (rays, the indices of the meridional ones)."""
    base = case("blocks")[2]
    assert len(base) > _BLOCKS_BASE
    idx = np.union1d(np.arange(0, _BLOCKS_BASE, stride), np.arange(660, 690))
    first = 480                                                                 # per height: 30 meridional, 30 + 30 along the parallel
    merid = np.nonzero((idx >= first) & (idx < first + 360) & ((idx - first) % 90 < 30))[0]
    aimed, am = aimed_rays(hts, lat, lon, k, seed)
    return np.concatenate([base[idx], aimed]), np.concatenate([merid, len(idx) + am])


_MERIDIONAL = {}


def batch_scene(name):
    """(tiles, order, rays, the indices of the meridional rays) of a batch case, before any reference is computed."""
    lat, lon = 46, 7
    w, h = BATCH_TILES[name]
    hts = blocks_heights(lat, lon, w, h)
    tiles, order = [(hts,) + tuple(T.synth.tile_transform(lat, lon, w, h))], [(lat, lon)]
    rays, merid = batch_rays(hts, lat, lon, *{"tall": (15, 35, 41), "grid": (15, 30, 42)}[name])
    return tiles, order, rays, merid


def _batch_case(name):
    tiles, order, rays, merid = batch_scene(name)
    mesh = LR.Mesh(tiles)
    first = LR.cast(mesh, rays)
    hit = np.nonzero(first["kind"] == LR.HIT)[0][::10]                       # _blocks_case's short and beyond copies
    short, beyond = rays[hit].copy(), rays[hit].copy()
    short["t_max"] = first["t"][hit] * 0.999
    beyond["t_min"] = first["t"][hit] * 1.001
    extra = np.concatenate([short, beyond])
    _MERIDIONAL[name] = merid
    return tiles, order, np.concatenate([rays, extra]), np.concatenate([first, LR.cast(mesh, extra)])


def meridional(name):
    """The indices of the meridional rays of a batch case."""
    case(name)
    return _MERIDIONAL[name]


def blocks_under(rays, lat, lon, w, h, samples=4000):
    """Per ray, whether its ground track over [t_min, t_max] passes over a block of index < 64, and over one of index >= 64."""
    t = rays["t_min"][:, None] + (rays["t_max"] - rays["t_min"])[:, None] * (np.arange(samples) + 0.5)[None, :] / samples
    p = rays["origin"][:, None, :] + t[..., None] * rays["dir"][:, None, :]
    la = np.degrees(np.arcsin(p[..., 2] / np.linalg.norm(p, axis=-1)))
    lo = np.degrees(np.arctan2(p[..., 1], p[..., 0]))
    cx, cy = np.floor((lo - lon) * w), np.floor((lat + 1 - la) * h)
    inside = (cx >= 0) & (cx < w - 1) & (cy >= 0) & (cy < h - 1)
    blk = block_of(np.clip(cx, 0, w - 2), np.clip(cy, 0, h - 2), w)
    return (inside & (blk < BATCH)).any(axis=1), (inside & (blk >= BATCH)).any(axis=1)


CASES.update({"antimeridian": lambda: _antimeridian_case(10), "antimeridian_south": lambda: _antimeridian_case(-11), "origin": _origin_case,
              "north84": lambda: _high_latitude_case(84, 20), "south85": lambda: _high_latitude_case(-85, -40), "polar": _polar_case,
              "tall": lambda: _batch_case("tall"), "grid": lambda: _batch_case("grid")})


def case(name):
    """(tiles, order, rays, reference records), computed once."""
    if name not in _CACHE:
        _CACHE[name] = CASES[name]()
    return _CACHE[name]


def with_invalid(rays):
    """A copy of `rays` with a NaN origin, a NaN direction, a zero direction, t_min > t_max and a NaN bound planted; their indices."""
    r = rays.copy()
    idx = np.array([3, 17, 40, 41, 77])
    r["origin"][3, 1] = np.nan
    r["dir"][17, 2] = np.inf
    r["dir"][40] = 0.0
    r["t_min"][41], r["t_max"][41] = 2.0, 1.0
    r["t_max"][77] = np.nan
    return r, idx


# ---- the sunlit layer ----------------------------------------------------------------------------------------------------------
_SUNLIT = {}


def sun_of(sc):
    return LR.sun_direction(sc.vlon, sc.vlat, SUN_AZ, SUN_EL)


def sunlit_case(name, orc):
    """A ridges scene's view, from the oracle's winners: (scene, W, H, uniforms, tiles, order, sun, reference classes (H, W), its
    ambiguous pixels, the classes composed from the g++ builds of topo_ground.h and topo_los.h).  Computed once."""
    if name not in _SUNLIT:
        import ground_emul as GE
        import ground_ref as GR
        import los_emul as LE
        kw, W, H, pose = RIDGES[name]
        sc = Scene(height_fn=ridges, **kw)
        tiles, order = GR.scene_tiles(sc), LR.geo_order(sc.locs)
        u = sc.uniforms(W, H, *pose, 0)
        o = orc.OracleRenderer(W, H)
        sc.load(o)
        o.update(W, H, u, T.post_uniforms(W, H))
        d, w = o.render_winners()
        o.close()
        sun = sun_of(sc)
        mesh = LR.Mesh(tiles)
        ref, amb = LR.sunlit(mesh, tiles, order, GR.ground(d, w, tiles, sc.locs, u), sun)
        rec = GE.ground(tiles, order, u, d, w)
        _SUNLIT[name] = (sc, W, H, u, tiles, order, sun, ref, amb, compose_sunlit(tiles, order, rec, sun))
    return _SUNLIT[name]


def compose_sunlit(tiles, order, rec, sun):
    """The sunlit classes of (H, W) ground records (kind, tile, cell, tri, w1, w2) through the g++ build of los_sunlit."""
    import los_emul as LE
    hm1 = tiles[0][0].shape[0] - 1
    rank_of = {tuple(o): r for r, o in enumerate(order)}
    ok = rec["kind"] == 1
    rank = np.array([rank_of.get((int(a), int(b)), len(order)) for a, b in zip(rec["tile_lat_deg"].ravel(), rec["tile_lon_deg"].ravel())]).reshape(ok.shape)
    rank = np.where(ok, rank, len(order))
    tri = 2 * (rec["cell_x"].astype(np.int64) * hm1 + rec["cell_y"]) + rec["tri"]
    cls, bad = LE.sunlit(tiles, order, rank, tri, rec["w1"].astype(np.float64), rec["w2"].astype(np.float64), sun)
    assert bad == 0
    return cls.reshape(ok.shape)


def against_emulation(got, emu, rays, what, keep):
    """Every ray: kind, tile, cell, triangle and face identical.  The rays the reference does not mark ambiguous (keep): t * |dir|
    within 1e-4 m (device and host sin / cos differ by an ulp or two: about 1.5e-9 m of vertex position, which 1 / |n . d| <= 1e3
    turns into 1.5e-6 m at most) -- a grazing ray has no such bound."""
    for f in ("kind", "tile_lat_deg", "tile_lon_deg", "cell_x", "cell_y", "tri", "front"):
        bad = np.nonzero(got[f] != emu[f])[0]
        assert len(bad) == 0, f"{what}: {f} differs from the emulation for {len(bad)} rays, first {bad[0]}: {got[bad[0]]} vs {emu[bad[0]]}"
    err = (np.abs(got["t"] - emu["t"]) * np.linalg.norm(rays["dir"], axis=1))[keep]
    print(f"{what}: largest |t| difference to the emulation {err.max():.3e} m")
    assert err.max() <= 1e-4, f"{what}: {err.max():.3e} m"
    hit = got["kind"] == LR.HIT
    if hit.any():
        assert np.abs(got["lon_deg"][hit] - emu["lon_deg"][hit]).max() < 1e-9 and np.abs(got["lat_deg"][hit] - emu["lat_deg"][hit]).max() < 1e-9
        assert np.abs(got["height_m"][hit] - emu["height_m"][hit].astype(np.float32)).max() <= 1e-3
        assert np.abs(got["w1"][hit] - emu["w1"][hit]).max() < 1e-5 and np.abs(got["w2"][hit] - emu["w2"][hit]).max() < 1e-5
    z = got[~hit]
    assert not z["t"].any() and not z["lon_deg"].any() and not z["cell_x"].any() and not z["w1"].any(), "every other field of a non-hit is 0"
    return float(err.max())
