"""Scenes whose DEM tiles carry voids, shared by tests/test_voids_cpu.py and tests/test_voids_gpu.py.

Real DEM tiles have holes: NaN from GDAL, the -32767 and -9999 sentinels, GDAL's float nodata -3.4028235e38, now and then an
infinity.  The loaders hand those bits to the kernels unchanged, so a void vertex is an ordinary vertex with an absurd (or
non-finite) height: the triangles that touch it fall to the guard band of the raster spec ("Void heights") and do
not exist; their neighbours do.  Every void scene here is a clean scene plus a pattern, built after the eye has been placed
on the clean surface, so that a void frame and its clean twin are seen from the same point."""
from __future__ import annotations

import copy

import numpy as np

from scenes import Scene

F32_MAX = 3.4028235e38
VALUES = {
    "nan": np.nan, "pinf": np.inf, "ninf": -np.inf,
    "m32767": -32767.0, "m9999": -9999.0,           # integer DEM sentinels
    "fmin": -F32_MAX, "fmax": F32_MAX,              # GDAL's float nodata and its mirror image
    "m1e10": -1e10, "p1e7": 1e7,                    # finite, but beyond the guard band from anywhere near
}
NORMALS_VALUES = ("nan", "ninf", "m32767", "fmin")
RAY_VALUES = ("nan", "pinf", "ninf", "m32767")      # what the f64 ray caster models (no binary32 overflow after the transform)
PATTERN_SEED = 7      # with it both relief scenes show the pattern of every value in more than one pixel in twenty


def relief(lat, lon):
    """tests/test_ray_check_cpu.py's relief: kilometre-high ridges a tenth of a degree apart."""
    return 1500.0 + 900.0 * np.sin(np.radians(37.0 * lon + 11.0 * lat)) * np.cos(np.radians(53.0 * lat)) \
        + 500.0 * np.sin(np.radians(140.0 * lon)) + 0.0 * lat


def void_pattern(h, value, rng, patch=None):
    """A copy of `h` with 2 % random specks, one interior 4 x 5 patch (at row, column `patch`, or anywhere), a run on the north
    border row and one on the east border column (the seams of a mosaic then see voids from both of their tiles) and the
    south-east corner texel void."""
    out = np.array(h, dtype=np.float32, copy=True)
    th, tw = out.shape
    v = np.float32(value)
    out[rng.random(out.shape) < 0.02] = v
    y0, x0 = int(rng.integers(2, max(3, th - 6))), int(rng.integers(2, max(3, tw - 7)))
    if patch is not None:
        y0, x0 = patch
    out[y0:y0 + 4, x0:x0 + 5] = v
    out[0, tw // 4:tw // 4 + max(3, tw // 6)] = v
    out[th // 3:th // 3 + max(3, th // 6), tw - 1] = v
    out[th - 1, tw - 1] = v
    return out


def void_tile(h, value):
    """The second pattern: the whole tile void."""
    return np.full_like(np.asarray(h, np.float32), np.float32(value))


def specks(h, value, seed, frac=0.01):
    """`frac` of the texels void, nothing else (the close-up scenes: a void next to the eye)."""
    out = np.array(h, dtype=np.float32, copy=True)
    out[np.random.default_rng(seed).random(out.shape) < frac] = np.float32(value)
    return out


def with_heights(sc, heights):
    """`sc` with other heights and the same eye."""
    v = copy.copy(sc)
    v.heights = dict(heights)
    return v


def patterned(sc, value, seed=PATTERN_SEED, only=None, patches=None):
    """`sc` with void_pattern applied to every tile (or to the tiles in `only`), one generator over the tiles in order;
    patches: {loc: (row, column)} of the tiles whose patch is to lie at a given place."""
    rng = np.random.default_rng(seed)
    return with_heights(sc, {loc: void_pattern(h, value, rng, (patches or {}).get(loc)) if only is None or loc in only else h
                             for loc, h in sc.heights.items()})


# name: Scene arguments, W, H, (yaw, pitch, fov, mode).  The synthetic fBm tiles barely show a void; these relief scenes do.
RELIEF = {
    "ne_2x2": (dict(tile=24, n_lat=2, n_lon=2, eye_dh=4000.0), 96, 64, (30.0, 25.0, 60.0, 0)),
    "down_1x1": (dict(tile=32, n_lat=1, n_lon=1, eye_dh=6000.0), 80, 80, (250.0, 60.0, 90.0, 1)),
}
# steep close-ups whose near triangles are cut by the near plane
CLOSE = {
    "close_1x1": (dict(tile=32, n_lat=1, n_lon=1, eye_dh=8.0), 64, 64, (120.0, 75.0, 110.0, 1)),
    "close_2x2": (dict(tile=24, n_lat=2, n_lon=2, eye_dh=400.0), 80, 48, (200.0, 45.0, 100.0, 2)),
}
CLOSE_VALUES = ("m1e10", "m32767", "fmin")
CLOSE_SEEDS = (1, 2, 3)
_CLEAN = {}


def clean_scene(name):
    if name not in _CLEAN:
        kw = (RELIEF.get(name) or CLOSE[name])[0]
        _CLEAN[name] = Scene(height_fn=relief, **kw) if name in RELIEF else Scene(**kw)
    return _CLEAN[name]


def eye_tile(sc):
    return next(loc for loc in sc.locs if loc[0] <= sc.vlat < loc[0] + 1 and loc[1] <= sc.vlon < loc[1] + 1)


def relief_case(name, value_name, whole_tile=False):
    """(clean scene, void twin, W, H, pose) of a relief scene; whole_tile: the tile under the eye (the one of ne_2x2 whose absence
    shows in enough of the frame) is void all over instead of the pattern."""
    _, W, H, pose = RELIEF[name]
    sc = clean_scene(name)
    if whole_tile:
        victim = eye_tile(sc)
        void = with_heights(sc, {loc: void_tile(h, VALUES[value_name]) if loc == victim else h for loc, h in sc.heights.items()})
    else:
        void = patterned(sc, VALUES[value_name])
    return sc, void, W, H, pose


def close_case(name, value_name, seed):
    _, W, H, pose = CLOSE[name]
    sc = clean_scene(name)
    return sc, with_heights(sc, {loc: specks(h, VALUES[value_name], seed + 100 * i) for i, (loc, h) in enumerate(sc.heights.items())}), W, H, pose


def assert_void_in_view(void_depth, clean_depth, what=""):
    """The condition on every compared void frame (both arrays from the oracle): terrain in at least a quarter of the pixels, and
    at least one pixel in twenty differing in depth from the clean twin's frame -- no test passes on a frame without a void in view."""
    vd, cd = np.asarray(void_depth, np.float32), np.asarray(clean_depth, np.float32)
    terrain = float((vd < 1.0).mean())
    changed = float((vd.view(np.uint32) != cd.view(np.uint32)).mean())
    print(f"{what}: terrain {terrain:.3f} changed {changed:.3f}")
    assert terrain >= 0.25, f"{what}: terrain in {terrain:.3f} of the pixels"
    assert changed >= 0.05, f"{what}: {changed:.3f} of the pixels differ from the clean twin"
    return terrain, changed


def assert_cut_void_in_view(sc, void, u, void_depth, clean_depth, what=""):
    """The close-ups' own condition (they are small by nature: from a few metres up most of the frame is nearer than the near
    plane): the void changes the oracle's frame, and at least one primitive with a void vertex is cut by the near plane (f64)."""
    from limits_scenes import _cell_triangles, _clip_coords
    vd, cd = np.asarray(void_depth, np.float32), np.asarray(clean_depth, np.float32)
    changed = int((vd.view(np.uint32) != cd.view(np.uint32)).sum())
    n_cut = 0
    for loc in void.locs:
        with np.errstate(all="ignore"):
            front = _clip_coords(void, loc, u)[..., 2] >= 0
        is_void = void.heights[loc].view(np.uint32) != sc.heights[loc].view(np.uint32)
        tag = np.stack([front, is_void], axis=-1)
        th, tw = front.shape
        for j in range(th - 1):
            for i in range(tw - 1):
                for tri in _cell_triangles(tag, i, j):
                    nin = sum(bool(v[0]) for v in tri)
                    n_cut += 0 < nin < 3 and any(bool(v[1]) for v in tri)
    print(f"{what}: terrain {float((vd < 1.0).mean()):.3f} changed px {changed} cut primitives with a void vertex {n_cut}")
    assert changed > 0 and n_cut > 0, f"{what}: {changed} px differ from the clean twin, {n_cut} cut primitives have a void vertex"


_ORACLE = {}


def oracle_frames(orc, key, sc, void, W, H, pose, post):
    """The oracle's (void frame, clean frame), computed once per case and shared by the tests that need it."""
    if key not in _ORACLE:
        out = []
        for s in (void, sc):
            o = orc.OracleRenderer(W, H)
            s.load(o)
            o.update(W, H, sc.uniforms(W, H, *pose), post)
            out.append(o.render())
            o.close()
        _ORACLE[key] = tuple(out)
    return _ORACLE[key]
