"""The cull's host-side tile prefilter (host_math.cpp: tile_prefilter) never drops a (view, tile) pair that holds a raster block the
device's frustum test keeps: 1 000 seeded random views over a 3 x 3 mosaic, the device's f64 sphere-versus-plane test restated in
numpy.  A containment check: no tolerance."""
import ctypes as C
import math

import numpy as np
import pytest

import native
import topo_renderer_amd as T

R0 = 6371000.0
BCX, BCY = 60, 15          # cells per raster block (topo_kernels.h)


@pytest.fixture(scope="module")
def shim():
    L = native.load("libprefilter_shim.so", ["prefilter_shim.cpp", native.HOST_MATH], {"shim_tile_prefilter": C.c_uint32, "shim_tile_sphere_doubles": C.c_uint32})
    L.shim_tile_prefilter.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    assert L.shim_tile_sphere_doubles() == 5
    return L


def block_spheres(heights, rp, mp, ps):
    """kernels_load.h block_bounds_store, the sphere part: (n_blocks, 4) f64 = centre, radius, blocks row-major (by, bx)."""
    h, w = heights.shape
    rad = 0.017453292519943295
    lat = lambda vy: ((vy - float(rp[1])) * -float(ps[1]) + float(mp[1])) * rad
    lon = lambda vx: ((vx - float(rp[0])) * float(ps[0]) + float(mp[0])) * rad
    out = []
    for by in range((h - 1 + BCY - 1) // BCY):
        for bx in range((w - 1 + BCX - 1) // BCX):
            y0, x0 = by * BCY, bx * BCX
            y1, x1 = min(y0 + BCY, h - 1), min(x0 + BCX, w - 1)
            patch = heights[y0:y1 + 1, x0:x1 + 1].astype(np.float64)
            hmin, hmax = patch.min(), patch.max()
            rm = R0 + 0.5 * (hmin + hmax)
            unit = lambda la, lo: np.array([math.cos(la) * math.cos(lo), math.cos(la) * math.sin(lo), math.sin(la)])
            c = rm * unit(lat(0.5 * (y0 + y1)), lon(0.5 * (x0 + x1)))
            r2 = max(float(((rm * unit(lat(y), lon(x)) - c) ** 2).sum()) for y in (y0, y1) for x in (x0, x1))
            out.append([c[0], c[1], c[2], math.sqrt(r2) + 0.5 * (hmax - hmin) + 8.0 + 64.0])
    return np.array(out)


def tile_sphere(bs):
    """add_terrain's read-back: the sphere around the block spheres' centres, then the largest block radius."""
    c = bs[:, :3].mean(axis=0)
    return np.array([c[0], c[1], c[2], math.sqrt(((bs[:, :3] - c) ** 2).sum(axis=1).max()), bs[:, 3].max()])


def clip_planes(m):
    """k_cull's clip_plane over a column-major view-projection matrix: (6, 5) f64 = a, b, c, d, |(a, b, c)|."""
    m = m.astype(np.float64)
    q = np.empty((6, 5))
    for pl in range(6):
        row, sgn = pl >> 1, (-1.0 if pl & 1 else 1.0)
        if pl == 4:
            q[pl, :4] = m[2], m[6], m[10], m[14]
        else:
            q[pl, :4] = m[3] + sgn * m[row], m[7] + sgn * m[4 + row], m[11] + sgn * m[8 + row], m[15] + sgn * m[12 + row]
        q[pl, 4] = math.sqrt((q[pl, :3] ** 2).sum())
    return q


def device_keeps(q, bs):
    """The device's test, per block: kept unless the sphere is wholly outside one plane."""
    dist = bs[:, :3] @ q[:, :3].T + q[:, 3]
    return ~(dist < -bs[:, 3:4] * q[:, 4]).any(axis=1)


def test_prefilter_contains_the_device_cull(shim):
    tile, lat0, lon0 = 64, 45, 15
    locs = sorted(T.synth.mosaic_locations(lat0, lon0, 3, 3), key=lambda l: (abs(l[0]), l[0] > 0, abs(l[1]), l[1] > 0))      # draw order
    spheres_b = [block_spheres(T.synth.synth_tile(la, lo, tile, tile), *T.synth.tile_transform(la, lo, tile, tile)) for la, lo in locs]
    spheres_t = np.ascontiguousarray([tile_sphere(bs) for bs in spheres_b])
    rng = np.random.default_rng(20240521)
    n = 1000
    views = np.zeros((n, 40), np.float32)
    for i in range(n):
        # eyes inside, at the edge of and well outside the mosaic, from just above the ground to 30 km; any yaw, steep pitches, narrow and wide fields of view
        vlat, vlon = rng.uniform(lat0 - 2.0, lat0 + 5.0), rng.uniform(lon0 - 2.0, lon0 + 5.0)
        eye = T.geometry_transform(float(rng.choice([60.0, 900.0, 5000.0, 30000.0])), vlon, vlat)
        W, H = ((128, 64), (64, 128), (256, 32))[i % 3]
        views[i] = T.camera_uniforms(eye, rng.uniform(-math.pi, math.pi), math.radians(rng.uniform(-80.0, 80.0)), math.radians(rng.uniform(5.0, 120.0)), W, H,
                                     vlon, vlat, 0)
    out = np.zeros(n * len(locs), np.uint16)
    kept = shim.shim_tile_prefilter(views.ctypes.data, n, spheres_t.ctypes.data, len(locs), out.ctypes.data, out.size)
    assert kept <= out.size and np.all(np.diff(out[:kept].astype(np.int64)) > 0)
    in_list = np.zeros(n * len(locs), bool)
    in_list[out[:kept]] = True
    dropped_pairs = blocks_kept = 0
    for i in range(n):
        q = clip_planes(views[i, :16])
        for t, bs in enumerate(spheres_b):
            k = int(device_keeps(q, bs).sum())
            blocks_kept += k
            dropped_pairs += not in_list[i * len(locs) + t]
            assert k == 0 or in_list[i * len(locs) + t], f"view {i} tile {t}: the device keeps {k} blocks of a pair the prefilter dropped"
    # the views exercise both outcomes
    assert dropped_pairs > n and blocks_kept > n, (dropped_pairs, blocks_kept)


def test_prefilter_keeps_unknown_and_nan(shim):
    eye = T.geometry_transform(500.0, 16.5, 46.5)
    view = T.camera_uniforms(eye, 0.0, 0.0, math.radians(20.0), 128, 64, 16.5, 46.5, 0).reshape(1, 40)
    behind = np.array(T.geometry_transform(0.0, 100.0, -30.0), np.float64)      # a quarter of the globe away: outside the far plane
    out = np.zeros(8, np.uint16)
    spheres = np.array([[*behind, 1000.0, 100.0],                  # dropped
                        [*behind, -1.0, 100.0],                    # unknown sphere
                        [*behind, 1000.0, -1.0],                   # unknown block radius
                        [*behind, float("nan"), 100.0],
                        [float("nan"), behind[1], behind[2], 1000.0, 100.0],
                        [*behind, float("inf"), 100.0]])
    kept = shim.shim_tile_prefilter(view.ctypes.data, 1, spheres.ctypes.data, len(spheres), out.ctypes.data, out.size)
    assert kept == 5 and list(out[:5]) == [1, 2, 3, 4, 5]
    # a NaN matrix keeps everything; a short output still counts every kept pair
    bad = view.copy()
    bad[0, 3] = np.nan
    assert shim.shim_tile_prefilter(bad.ctypes.data, 1, spheres.ctypes.data, len(spheres), out.ctypes.data, 2) == 6 and list(out[:2]) == [0, 1]
