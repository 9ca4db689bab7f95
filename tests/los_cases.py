"""Scenes and rays of the ray-query tests (tests/test_raycast_cpu.py, tests/test_raycast_gpu.py): the smallest at which the traversal
of topo_los.h can go wrong.  A case is (tiles in draw order, their (lat, lon), rays); its reference answer (los_ref.cast) is computed
once and shared."""
from __future__ import annotations

import math

import numpy as np

import los_ref as LR
import topo_renderer_amd as T
from oracle import ray_check as RC
from scenes import Scene

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
