"""Horizon (topo_horizon_*, topo_pixel_angles) without a GPU: the C ABI and its bindings, the expected-horizon helper the GPU
tests compare against (tests/horizon_ref.py), and the pixel-angle helper against an f64 restatement of its own."""
import ctypes as C
import math
import re
import subprocess

import numpy as np

from horizon_ref import horizon
from viewshed_ref import NO_TRI, geo_order

SYMBOLS = ("topo_horizon_shape", "topo_horizon_read", "topo_horizon_device")


def test_horizon_symbols_are_declared_exported_and_bound(topo):
    header = open(topo.HEADER_PATH).read()
    for s in SYMBOLS:
        assert re.search(r"\bint\s+" + s + r"\s*\(", header), s
    assert re.search(r"\bvoid\s+topo_pixel_angles\s*\(", header)
    assert "TOPO_HORIZON_SKY (-1)" in header and "TOPO_HORIZON_INCOMPLETE (-2)" in header
    nm = subprocess.run(["nm", "-D", "--defined-only", topo.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (topo_[a-z0-9_]+)", nm))
    L = topo.lib()
    for s in SYMBOLS + ("topo_pixel_angles",):
        assert s in exported and s in L._topo_symbols, s
        assert getattr(L, s).argtypes is not None
    for m in ("horizon", "horizon_device", "horizon_shape"):
        assert callable(getattr(topo.TerrainRenderer, m, None)), m
    assert callable(topo.pixel_angles)


def test_horizon_calls_reject_null_arguments(topo):
    L = topo.lib()
    n = C.c_uint32()
    buf = np.zeros(64, topo.HORIZON_DTYPE)
    assert L.topo_horizon_shape(None, C.byref(n), C.byref(n), C.byref(n)) == topo.TOPO_ERR_INVALID
    assert L.topo_horizon_read(None, 0, 1, buf.ctypes.data_as(C.c_void_p), 64) == topo.TOPO_ERR_INVALID
    assert L.topo_horizon_device(None, 0, 1, buf.ctypes.data_as(C.c_void_p), 64) == topo.TOPO_ERR_INVALID
    L.topo_pixel_angles(None, 64, 64, 1, None, None)      # a void helper: null arguments are ignored, nothing is written


def test_record_is_32_bytes(topo):
    class Point(C.Structure):
        _fields_ = [("row", C.c_int32), ("depth", C.c_float), ("lat_deg", C.c_int32), ("lon_deg", C.c_int32),
                    ("cell_x", C.c_uint32), ("cell_y", C.c_uint32), ("fan", C.c_uint32), ("_reserved", C.c_uint32)]
    assert C.sizeof(Point) == 32 and topo.HORIZON_DTYPE.itemsize == 32
    assert [topo.HORIZON_DTYPE.fields[f][1] for f in topo.HORIZON_DTYPE.names] == [getattr(Point, f).offset for f, _ in Point._fields_]


def test_rust_wrapper_has_horizon():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "rust", "topo-hip", "src", "lib.rs")).read()
    assert re.search(r"pub fn horizon\(&mut self\)", src)
    sys_src = open(os.path.join(root, "rust", "topo-hip-sys", "src", "lib.rs")).read()
    assert "pub struct topo_horizon_point" in sys_src


def _loop_horizon(depth, win, locs, tw, th):
    """A plain per-column scan: the reference the vectorised helper is checked against."""
    H, W = win.shape
    order = geo_order(locs)
    tris = 2 * (tw - 1) * (th - 1)
    out = []
    for x in range(W):
        rec = (-1, np.float32(1.0), 0, 0, 0, 0)
        for y in range(H):
            v = int(win[y, x])
            if v != NO_TRI:
                rank, tri = divmod(v, tris)
                cell = tri // 2
                rec = (y, depth[y, x], order[rank][0], order[rank][1], cell // (th - 1), cell % (th - 1))
                break
        out.append(rec)
    return out


def _check(depth, win, locs, tw, th):
    got = horizon(depth, win, locs, tw, th)
    want = _loop_horizon(depth, win, locs, tw, th)
    for x, rec in enumerate(want):
        g = tuple(got[f][x] for f in ("row", "depth", "lat_deg", "lon_deg", "cell_x", "cell_y"))
        assert g[0] == rec[0] and np.float32(g[1]).view(np.uint32) == np.float32(rec[1]).view(np.uint32) and g[2:] == rec[2:], (x, g, rec)
    return got


def test_helper_against_a_per_column_loop():
    locs = [(45, 15), (-3, -71), (45, -2)]
    tw, th = 7, 5
    tris = 2 * (tw - 1) * (th - 1)
    rng = np.random.default_rng(3)
    # all sky, at several widths that are not multiples of 64
    for W in (1, 63, 65, 130):
        win = np.full((9, W), NO_TRI, np.uint32)
        got = _check(np.ones((9, W), np.float32), win, locs, tw, th)
        assert (got["row"] == -1).all() and (got["depth"] == 1.0).all()
    # terrain from row 0 in some columns, deeper in others, sky in the rest
    for W in (1, 63, 65, 130, 200):
        H = 37
        win = np.full((H, W), NO_TRI, np.uint32)
        depth = np.ones((H, W), np.float32)
        for x in range(W):
            top = int(rng.integers(-1, H))      # -1: an all-sky column
            if top < 0:
                continue
            for y in range(top, H):
                if rng.random() < 0.8 or y == top:
                    win[y, x] = int(rng.integers(0, 3 * tris))
                    depth[y, x] = np.float32(rng.random())
        win[:, 0] = 2 * tris + 5      # row 0 in column 0
        depth[:, 0] = np.float32(0.25)
        got = _check(depth, win, locs, tw, th)
        assert got["row"][0] == 0 and (W < 63 or ((got["row"] == -1).any() and (got["row"] > 0).any()))


def _enu(eye):
    up = eye / np.linalg.norm(eye)
    east = np.array([-up[1], up[0], 0.0])
    east /= np.linalg.norm(east)
    return east, np.cross(up, east), up


def _angles_f64(u, W, H, xy):
    """Independent restatement: numpy's inverse of camera_proj, the near / far plane points of each pixel, azimuth and elevation
    in the local east / north / up frame of the eye."""
    M = np.asarray(u[:16], np.float64).reshape(4, 4).T      # column-major
    inv = np.linalg.inv(M)
    east, north, up = _enu(np.asarray(u[32:35], np.float64))
    out = []
    for x, y in xy:
        nx, ny = 2.0 * x / W - 1.0, 1.0 - 2.0 * y / H
        p = [inv @ np.array([nx, ny, z, 1.0]) for z in (0.0, 1.0)]
        d = p[1][:3] / p[1][3] - p[0][:3] / p[0][3]
        az = math.degrees(math.atan2(d @ east, d @ north)) % 360.0
        out.append((az, math.degrees(math.atan2(d @ up, math.hypot(d @ east, d @ north)))))
    return np.array(out)


def _panorama(topo, W=256, H=128, yaw0=20.0, pitch=0.0):
    eye = topo.geometry_transform(1500.0, 15.5, 45.5)
    return eye, topo.panorama_uniforms(eye, math.radians(yaw0), W, H, 15.0, 45.0, 0, pitch=pitch)


def test_pixel_angles_match_an_f64_restatement(topo):
    W, H = 256, 128
    rng = np.random.default_rng(8)
    for pitch in (0.0, 0.3, -0.2):
        _, us = _panorama(topo, W, H, 20.0, pitch)
        for u in us:
            xy = np.column_stack([rng.uniform(0, W, 40), rng.uniform(0, H, 40)])
            got = topo.pixel_angles(u, W, H, xy)
            want = _angles_f64(u, W, H, xy.astype(np.float32).astype(np.float64))
            daz = (got[:, 0] - want[:, 0] + 180.0) % 360.0 - 180.0
            assert np.abs(daz).max() < 1e-6 and np.abs(got[:, 1] - want[:, 1]).max() < 1e-6
            assert ((got[:, 0] >= 0.0) & (got[:, 0] < 360.0)).all()


def test_pixel_angles_see_projected_points(topo):
    """Points projected into a view through camera_proj come back at the azimuth / elevation of (point - eye): the direction of
    the ray, not only its line."""
    W, H = 320, 200
    eye, us = _panorama(topo, W, H, 75.0, 0.1)
    east, north, up = _enu(eye.astype(np.float64))
    rng = np.random.default_rng(2)
    n_in = 0
    for u in us:
        M = np.asarray(u[:16], np.float64).reshape(4, 4).T
        for _ in range(200):
            d = rng.normal(size=3)
            P = eye.astype(np.float64) + 80000.0 * d / np.linalg.norm(d)
            c = M @ np.append(P, 1.0)
            if c[3] <= 0:
                continue
            x, y = 0.5 * (c[0] / c[3] + 1.0) * W, 0.5 * (1.0 - c[1] / c[3]) * H
            if not (0 <= x < W and 0 <= y < H):
                continue
            n_in += 1
            az, el = topo.pixel_angles(u, W, H, [(x, y)])[0]
            v = P - eye.astype(np.float64)
            waz = math.degrees(math.atan2(v @ east, v @ north)) % 360.0
            wel = math.degrees(math.atan2(v @ up, math.hypot(v @ east, v @ north)))
            assert abs((az - waz + 180.0) % 360.0 - 180.0) < 5e-3 and abs(el - wel) < 5e-3, (az, el, waz, wel)
    assert n_in > 20


def test_panorama_sector_azimuths_and_level_row(topo):
    """Sector s covers [a0 + 45 s, a0 + 45 (s + 1)] (a0: sector 0's left edge), its column azimuths increase monotonically, and the
    centre row of a pitch-0 view lies in the eye's horizontal plane."""
    W, H = 256, 128
    _, us = _panorama(topo, W, H, 33.0, 0.0)
    cols = np.column_stack([np.arange(W + 1, dtype=np.float64), np.full(W + 1, H / 2.0)])
    a0 = topo.pixel_angles(us[0], W, H, cols[:1])[0, 0]
    for s, u in enumerate(us):
        ang = topo.pixel_angles(u, W, H, cols)
        rel = (ang[:, 0] - a0 - 45.0 * s + 180.0) % 360.0 - 180.0      # relative to the sector's expected left edge
        assert abs(rel[0]) < 1e-4 and abs(rel[-1] - 45.0) < 1e-4, (s, rel[0], rel[-1])
        assert (np.diff(rel) > 0).all() and (rel >= -1e-4).all() and (rel <= 45.0 + 1e-4).all()
        assert np.abs(ang[:, 1]).max() < 1e-3, np.abs(ang[:, 1]).max()
