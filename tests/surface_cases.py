"""Scenes and points of the surface-query tests (tests/test_surface_cpu.py, tests/test_surface_gpu.py): the smallest at which the
lookup of topo_surface.h can go wrong.  A case is (tiles in draw order, their (lat, lon), points (n, 2) lon / lat degrees, a label
per point); its reference answer (surface_ref) and its emulation (surface_emul) are computed once and shared.

Labels: RANDOM points are held to the cap on ambiguous points; VERTEX, EDGE and DIAGONAL points lie on mesh edges on purpose (which
of the triangles around them wins is rounding) and are exempt from it; GAP points must have no terrain."""
from __future__ import annotations

import numpy as np

import los_cases as LC
import surface_emul as SE
import surface_ref as SR
import topo_renderer_amd as T
from oracle import ray_check as RC
from scenes import Scene

RANDOM, VERTEX, EDGE, DIAGONAL, GAP = 0, 1, 2, 3, 4
MAX_AMBIGUOUS = 0.005      # los_ref's cap
_CACHE, _REF, _EMU = {}, {}, {}


def lonlat_of(p):
    """Longitude / latitude (degrees) of ECEF positions (n, 3)."""
    p = np.asarray(p, np.float64)
    return np.stack([np.degrees(np.arctan2(p[:, 1], p[:, 0])), np.degrees(np.arcsin(p[:, 2] / np.linalg.norm(p, axis=1)))], axis=-1)


def vertex_lonlat(tile, vx, vy):
    """Where the mesh puts vertex (vx, vy): the f32 transform widened, f64 from there on."""
    _, rp, mp, ps = tile
    rp, mp, ps = (np.asarray(a, np.float32).astype(np.float64) for a in (rp, mp, ps))
    return np.stack(np.broadcast_arrays((np.asarray(vx, np.float64) - rp[0]) * ps[0] + mp[0], (np.asarray(vy, np.float64) - rp[1]) * -ps[1] + mp[1]), axis=-1)


def random_points(lon0, lon1, lat0, lat1, n, seed, margin=0.02):
    """n points over the box and a margin of `margin` of its size around it."""
    rng = np.random.default_rng(seed)
    dx, dy = (lon1 - lon0) * margin, (lat1 - lat0) * margin
    return np.stack([rng.uniform(lon0 - dx, lon1 + dx, n), np.clip(rng.uniform(lat0 - dy, lat1 + dy, n), -90.0, 90.0)], axis=-1)


def _labelled(parts):
    pts = np.concatenate([p for p, _ in parts])
    return pts, np.concatenate([np.full(len(p), l, np.int32) for p, l in parts])


def blocks_tile():
    lat, lon, w, h = 46, 7, 130, 34
    return (LC.blocks_heights(lat, lon, w, h),) + tuple(T.synth.tile_transform(lat, lon, w, h))


def blocks_vertices():
    """Every vertex of the blocks tile: ((n, 2) lon / lat, (n,) f32 heights), column-major as the cells are numbered."""
    tile = blocks_tile()
    h, w = tile[0].shape
    vx, vy = np.meshgrid(np.arange(w), np.arange(h), indexing="ij")
    return vertex_lonlat(tile, vx.ravel(), vy.ravel()), tile[0][vy.ravel(), vx.ravel()]


def _blocks_case():
    """One tile of 130 x 34 vertices (ragged raster blocks): random points with a 2 % margin outside the tile, every third exact
    vertex, and the 3-D midpoints of every third cell edge and cell diagonal, which lie on those edges exactly."""
    tile = blocks_tile()
    h, w = tile[0].shape
    tiles, order = [tile], [(46, 7)]
    P = RC.tile_vertices(*tile)      # [j, i]
    allv, _ = blocks_vertices()
    i, j = np.meshgrid(np.arange(w - 1), np.arange(h), indexing="ij")
    horiz = 0.5 * (P[j.ravel(), i.ravel()] + P[j.ravel(), i.ravel() + 1])
    i, j = np.meshgrid(np.arange(w), np.arange(h - 1), indexing="ij")
    vert = 0.5 * (P[j.ravel(), i.ravel()] + P[j.ravel() + 1, i.ravel()])
    i, j = np.meshgrid(np.arange(w - 1), np.arange(h - 1), indexing="ij")
    i, j = i.ravel(), j.ravel()
    even = (i + j) % 2 == 0      # the diagonal of an even cell joins (i, j) and (i + 1, j + 1), of an odd one (i, j + 1) and (i + 1, j)
    diag = 0.5 * (np.where(even[:, None], P[j, i], P[j + 1, i]) + np.where(even[:, None], P[j + 1, i + 1], P[j, i + 1]))
    pts, label = _labelled([(random_points(7.0, 7.0 + (w - 1) / w, 47.0 - (h - 1) / h, 47.0, 3000, 3), RANDOM), (allv[::3], VERTEX),
                            (lonlat_of(np.concatenate([horiz, vert])[::3]), EDGE), (lonlat_of(diag[::3]), DIAGONAL)])
    return tiles, order, pts, label


def _long_case():
    """los_cases' 1 x 3 mosaic of 48-vertex tiles: a tile's last column stops 1/48 degree short of its neighbour, and points in the
    two gaps have no terrain."""
    sc = Scene(48, 1, 3, lat0=44, lon0=5, height_fn=lambda la, lo: 900.0 + 700.0 * np.sin(np.radians(2100.0 * lo)) * np.cos(np.radians(1300.0 * la)) + 0.0 * (la + lo))
    tiles, order = LC.scene_tiles(sc)
    lats = 44.0 + 1.0 / 48.0 + (47.0 / 48.0) * (np.arange(40) + 0.5) / 40
    gap = np.stack(np.broadcast_arrays((5.0 + 47.5 / 48.0 + np.array([0.0, 1.0]))[:, None], lats[None, :]), axis=-1).reshape(-1, 2)
    pts, label = _labelled([(random_points(5.0, 8.0, 44.0, 45.0, 1500, 5), RANDOM), (gap, GAP)])
    return tiles, order, pts, label


def overlap_tiles(second_fn):
    """Two 24-vertex tiles with 1/32-degree posts (exact in f32, so that shifted vertices coincide bit for bit), the second's
    model_point half a degree (16 posts) east of the first's: columns 16 .. 23 of the first are columns 0 .. 7 of the second."""
    n, s = 24, 1.0 / 32.0
    x = np.arange(n, dtype=np.float64) * s
    out = []
    for lon0, fn in ((15.0, LC.geo_relief), (15.5, second_fn)):
        hts = np.ascontiguousarray(fn((46.0 - x)[:, None], (lon0 + x)[None, :]), dtype=np.float32)
        out.append((hts, np.float32([0.0, 0.0]), np.float32([lon0, 46.0]), np.float32([s, s])))
    return out, [(45, 15), (45, 16)]


def _overlap_case(second_fn, seed):
    tiles, order = overlap_tiles(second_fn)
    s = 1.0 / 32.0
    pts, label = _labelled([(random_points(15.0, 15.5 + 23 * s, 46.0 - 23 * s, 46.0, 1500, seed), RANDOM)])
    return tiles, order, pts, label


def higher_relief(lat, lon):
    """geo_relief with a swell that changes sign across the overlap: either tile is the higher one somewhere."""
    return LC.geo_relief(lat, lon) + 400.0 * np.sin(np.radians(3000.0 * lon)) * np.cos(np.radians(2500.0 * lat))


def _void_case(value_name):
    import void_scenes as VS
    _, void, _, _, _ = VS.relief_case("ne_2x2", value_name)
    tiles, order = LC.scene_tiles(void)
    pts, label = _labelled([(random_points(15.0, 17.0, 45.0, 47.0, 2000, 9), RANDOM)])
    return tiles, order, pts, label


def _sentinel_case():
    """One 24-vertex tile with a -3.4e38 vertex (below -R0: the triangles around it do not exist) and a -32768 vertex (geometry: a pit)."""
    tiles, order = LC.placed_tiles([(45, 15)], 24)
    hts = tiles[0][0].copy()
    hts[5, 7] = np.float32(-3.4e38)
    hts[15, 12] = np.float32(-32768.0)
    tiles = [(hts,) + tuple(tiles[0][1:])]
    off = np.array([-0.3, -0.15, -0.05, 0.1, 0.25])
    grid = np.stack(np.meshgrid(off, off), axis=-1).reshape(-1, 2) / 24.0      # 25 points within 0.3 cells of a vertex, none on an edge
    near = np.concatenate([vertex_lonlat(tiles[0], 7, 5) + grid, vertex_lonlat(tiles[0], 12, 15) + grid,
                           vertex_lonlat(tiles[0], 7, 5) + np.random.default_rng(1).uniform(-1.2, 1.2, (100, 2)) / 24.0,
                           vertex_lonlat(tiles[0], 12, 15) + np.random.default_rng(2).uniform(-1.2, 1.2, (100, 2)) / 24.0])
    pts, label = _labelled([(random_points(15.0, 16.0, 45.0, 46.0, 1200, 13), RANDOM), (near, RANDOM)])
    return tiles, order, pts, label


def _antimeridian_case(lat):
    """los_cases' tiles either side of the antimeridian; the longitudes of every other point are given as 180.3, the others as -179.7."""
    tiles, order = LC.placed_tiles([(lat, 179), (lat, -180)], 48)
    pts = random_points(179.0, 181.0, float(lat), lat + 1.0, 1500, 21 + abs(lat))
    pts[1::2, 0] -= 360.0
    return tiles, order, pts, np.full(len(pts), RANDOM, np.int32)


def _origin_case():
    tiles, order = LC.placed_tiles([(0, 0), (-1, 0), (0, -1), (-1, -1)], 32)
    pts = random_points(-1.0, 1.0, -1.0, 1.0, 1500, 23)
    return tiles, order, pts, np.full(len(pts), RANDOM, np.int32)


def _high_latitude_case(lat, lon):
    tiles, order = LC.placed_tiles([(lat, lon), (lat, lon + 1)], 48)
    pts = random_points(float(lon), lon + 2.0, float(lat), lat + 1.0, 1500, 25 + abs(lat))
    return tiles, order, pts, np.full(len(pts), RANDOM, np.int32)


def _polar_case():
    """los_cases' four 32-vertex tiles whose row 0 is the north pole, points up to 89.99N."""
    tiles, order = LC.placed_tiles([(89, 20), (89, 21), (89, -160), (89, -159)], 32)
    a, b = random_points(20.0, 22.0, 89.0, 89.99, 800, 31, margin=0.0), random_points(-160.0, -158.0, 89.0, 89.99, 800, 32, margin=0.0)
    pts = np.concatenate([a, b])
    return tiles, order, pts, np.full(len(pts), RANDOM, np.int32)


CASES = {"blocks": _blocks_case, "long": _long_case, "overlap_higher": lambda: _overlap_case(higher_relief, 41), "overlap_equal": lambda: _overlap_case(LC.geo_relief, 42),
         "void_nan": lambda: _void_case("nan"), "void_pinf": lambda: _void_case("pinf"), "sentinels": _sentinel_case,
         "antimeridian": lambda: _antimeridian_case(10), "antimeridian_south": lambda: _antimeridian_case(-11), "origin": _origin_case,
         "north84": lambda: _high_latitude_case(84, 20), "south85": lambda: _high_latitude_case(-85, -40), "polar": _polar_case}


def case(name):
    """(tiles, order, points, labels), computed once."""
    if name not in _CACHE:
        _CACHE[name] = CASES[name]()
    return _CACHE[name]


def reference(name):
    if name not in _REF:
        tiles, order, pts, _ = case(name)
        _REF[name] = SR.surface(SR.Mesh(tiles), pts)
    return _REF[name]


def emulation(name):
    """(records of the lookup, failed index checks)."""
    if name not in _EMU:
        tiles, order, pts, _ = case(name)
        _EMU[name] = SE.surface(tiles, order, pts)
    return _EMU[name]


def big_tile():
    """One 1200 x 1200 tile and 20 000 random points over it and a margin."""
    lat, lon = 46, 7
    tiles, order = [(T.synth.synth_tile(lat, lon, 1200, 1200),) + tuple(T.synth.tile_transform(lat, lon, 1200, 1200))], [(lat, lon)]
    return tiles, order, random_points(float(lon), lon + 1.0, float(lat), lat + 1.0, 20000, 51)


def with_invalid(pts):
    """A copy of the points with a NaN longitude, an infinite latitude, latitudes of 90.5 and -91 and an infinite longitude
    planted; their indices."""
    p = np.array(pts, np.float64, copy=True)
    idx = np.array([3, 17, 40, 41, 77])
    p[3, 0] = np.nan
    p[17, 1] = np.inf
    p[40, 1] = 90.5
    p[41, 1] = -91.0
    p[77, 0] = -np.inf
    return p, idx


# ---- profiles ----------------------------------------------------------------------------------------------------------------
def profile_segments():
    """Segments over the long mosaic: across the tiles and the gaps 100 m to 3 km up, one that leaves the mosaic, one steep, one of
    zero length (every sample the same point: a tie), and invalid ones (a NaN origin, an infinite bound, a zero direction)."""
    k = 6
    lats = 44.2 + 0.6 * (np.arange(k) + 0.5) / k
    a, b = LC.ecef(5.1, lats, 1000.0 + 400.0 * np.arange(k)), LC.ecef(7.9, lats + 0.05, 3000.0 - 500.0 * np.arange(k))
    segs = [LC.make_rays(a, b - a, 0.0, 1.0)]
    a, b = LC.ecef(7.5, 44.5, 2500.0), LC.ecef(9.5, 44.7, 2500.0)
    segs.append(LC.make_rays(a, b - a, 0.0, 1.0))                     # leaves the mosaic at 8E
    a, b = LC.ecef(6.3, 44.4, 6000.0), LC.ecef(6.32, 44.41, -500.0)
    segs.append(LC.make_rays(a, b - a, -0.1, 1.2))                    # steep, ends under the ground
    segs.append(LC.make_rays(LC.ecef(6.4, 44.6, 2000.0), [1.0, 2.0, 3.0], 0.5, 0.5))      # zero length
    a = LC.ecef(3.0, 44.5, 2000.0)
    segs.append(LC.make_rays(a, LC.ecef(4.0, 44.5, 2000.0) - a, 0.0, 1.0))                # never over the mosaic
    bad = LC.make_rays(np.tile(LC.ecef(6.0, 44.5, 2000.0), (3, 1)), [1.0, 0.0, 0.0], 0.0, 1.0)
    bad["origin"][0, 1] = np.nan
    bad["t_max"][1] = np.inf
    bad["dir"][2] = 0.0
    segs.append(bad)
    segs = np.concatenate(segs)
    return segs, np.arange(len(segs) - 3, len(segs))


def check_summaries(summary, samples, invalid, what):
    """The summaries against the numpy reduction of the samples they came with, exactly."""
    valid = np.ones(len(summary), bool)
    valid[invalid] = False
    least, first, count = SR.reduce_samples(samples[valid])
    s = summary[valid]
    assert np.array_equal(s["n_terrain"], count), what
    assert np.array_equal(s["min_sample"], first), what
    assert np.array_equal(s["min_clearance_m"].view(np.uint32)[count > 0], least.view(np.uint32)[count > 0]), what
    assert np.isnan(s["min_clearance_m"][count == 0]).all() and (s["min_sample"][count == 0] == 0xFFFFFFFF).all(), what
    assert np.array_equal(s["kind"], np.where(count > 0, SR.TERRAIN, SR.NONE)), what
    bad = summary[invalid]
    assert (bad["kind"] == SR.INVALID).all() and not bad["min_clearance_m"].any() and not bad["min_sample"].any() and not bad["n_terrain"].any(), what
    assert np.isnan(samples[invalid]).all(), what


def aspect_difference(a, b):
    """|a - b| on the circle of 360 degrees."""
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) % 360.0
    return np.minimum(d, 360.0 - d)


def check_slope_aspect(got_slope, got_aspect, want_slope, want_aspect, f32_record, what):
    """Slope within 1e-6 degrees and, where the slope is > 1 degree, aspect within 1e-4 degrees of the f64 values wanted.  f32_record:
    `got` holds the record's f32 fields, which the ABI defines as the f64 value rounded once -- an f32 cannot lie within 1e-6 of an
    arbitrary f64 beyond 16 degrees (its steps are 1.9e-6 there, 3.8e-6 from 32) -- so the slope wanted is rounded to f32 in the
    same way before the same 1e-6 is asked: the two f32 are equal unless the two f64 straddle a rounding boundary, which then shows
    as a whole step and fails.  The aspect's 1e-4 holds an f32 step (3.1e-5 at most) and is asked of the f32 as it is."""
    want_slope, want_aspect = np.asarray(want_slope, np.float64), np.asarray(want_aspect, np.float64)
    target = want_slope.astype(np.float32).astype(np.float64) if f32_record else want_slope
    es = np.abs(np.asarray(got_slope).astype(np.float64) - target)
    assert (es <= 1e-6).all(), f"{what}: slope differs by {es.max():.3e} degrees"
    steep = want_slope > 1.0
    if steep.any():
        ea = aspect_difference(np.asarray(got_aspect)[steep], want_aspect[steep])
        assert (ea <= 1e-4).all(), f"{what}: aspect differs by {ea.max():.3e} degrees"


def compare_reference(ref, got, order, tile_h, label, what, f32_record):
    """The comparison rule against surface_ref: kind outside kind-ambiguous points; tile, cell and triangle outside triangle-ambiguous
    points; the height of every point both sides call TERRAIN within 1e-3 m (the project's bound for ground points and rays); slope
    within 1e-6 degrees and, where the slope is > 1 degree, aspect within 1e-4 degrees, outside triangle-ambiguous points (the
    neighbour's slope is another number): check_slope_aspect, which says what f32_record means.  At
    most MAX_AMBIGUOUS of the RANDOM points may be ambiguous in either sense.  Returns the largest height difference."""
    rnd = label == RANDOM
    amb = ref["tri_ambiguous"] | ref["kind_ambiguous"]
    share = float(amb[rnd].mean()) if rnd.any() else 0.0
    print(f"{what}: {len(ref)} points, {int((ref['kind'] == SR.TERRAIN).sum())} over terrain, ambiguous among the {int(rnd.sum())} random ones {share:.4%}")
    assert share <= MAX_AMBIGUOUS, f"{what}: {share:.4%} of the random points are ambiguous"
    keep = ~ref["kind_ambiguous"]
    bad = np.nonzero(keep & (ref["kind"] != got["kind"]))[0]
    assert len(bad) == 0, f"{what}: kind differs for {len(bad)} points, first {bad[0]}: ref {ref[bad[0]]} got {got[bad[0]]}"
    both = (ref["kind"] == SR.TERRAIN) & (got["kind"] == SR.TERRAIN)
    if not both.any():
        return 0.0
    err = np.abs(got["height_m"][both] - ref["height_m"][both])
    print(f"{what}: largest height difference {err.max():.3e} m")
    assert err.max() <= 1e-3, f"{what}: height differs by {err.max():.3e} m"
    t = both & ~ref["tri_ambiguous"] & keep
    hm1 = tile_h - 1
    lat = np.array([order[r][0] for r in ref["rank"][t]])
    lon = np.array([order[r][1] for r in ref["rank"][t]])
    cell = ref["tri"][t] >> 1
    g = got[t]
    same = (g["tile_lat_deg"] == lat) & (g["tile_lon_deg"] == lon) & (g["cell_x"] == cell // hm1) & (g["cell_y"] == cell % hm1) & (g["tri"] == (ref["tri"][t] & 1))
    assert same.all(), f"{what}: {int((~same).sum())} points name another triangle, first {np.nonzero(t)[0][np.nonzero(~same)[0][0]]}"
    rs, ra = ref["slope_deg"][t], ref["aspect_deg"][t]
    check_slope_aspect(g["slope_deg"], g["aspect_deg"], rs, ra, f32_record, what)
    return float(err.max())
