"""The unwrap test cases shared by tests/test_unwrap_cpu.py and tests/test_unwrap_gpu.py: source views and output windows."""
from __future__ import annotations

import math

import numpy as np

import topo_renderer_amd as T
from scenes import Scene

_SCENE = None


def scene():
    global _SCENE
    if _SCENE is None:
        _SCENE = Scene(96, 2, 2, eye_dh=120.0)
    return _SCENE


def _pano(sw, sh, yaw0_deg, pitch_deg=0.0):
    sc = scene()
    return T.panorama_uniforms(sc.eye, math.radians(yaw0_deg), sw, sh, sc.vlon, sc.vlat, 0, pitch=math.radians(pitch_deg))


def _three_views():
    sc = scene()
    return [sc.uniforms(150, 90, yaw, 0.0, 70.0, 0) for yaw in (0.0, 40.0, 80.0)]


def case(name):
    """-> (views (list of 160-byte uniforms), src_w, src_h, params, how) of case `name`; how: ("panorama", yaw0_deg, pitch_deg), the
    arguments render_panorama reproduces the views from, or ("views",)."""
    P = T.unwrap_params
    if name == "a":      # the base case
        return _pano(96, 160, 25.0), 96, 160, P(768, 160, 30.0, -30.0), ("panorama", 25.0, 0.0)
    if name == "b":      # a width that is no multiple of 4, cylindrical
        return _pano(96, 160, 25.0), 96, 160, P(777, 131, 25.0, -25.0, projection=T.UNWRAP_CYLINDRICAL), ("panorama", 25.0, 0.0)
    if name == "c":      # rows beyond the sectors' vertical field of view (+-29.6 degrees): whole fill rows
        return _pano(70, 96, 3.0), 70, 96, P(500, 200, 40.0, -40.0), ("panorama", 3.0, 0.0)
    if name == "d":      # a pitched panorama: gaps, and overlaps the nearest-axis rule decides
        return _pano(96, 160, 25.0, 10.0), 96, 160, P(768, 160, 35.0, -25.0), ("panorama", 25.0, 10.0)
    if name == "e":      # a partial span
        return _pano(96, 160, 25.0), 96, 160, P(333, 97, 30.0, -30.0, az0_deg=100.0, az_span_deg=90.0), ("panorama", 25.0, 0.0)
    if name == "f":      # three overlapping generic views: a window of 200 degrees around the middle one, cylindrical, odd sizes
        views = _three_views()
        az_mid = float(T.pixel_angles(views[1], 150, 90, [(75.0, 45.0)])[0, 0])
        return views, 150, 90, P(403, 101, 45.0, -40.0, az0_deg=az_mid - 100.0, az_span_deg=200.0, projection=T.UNWRAP_CYLINDRICAL), ("views",)
    if name == "g":      # bilinear magnification of case a's source
        return _pano(96, 160, 25.0), 96, 160, P(1536, 320, 30.0, -30.0, filter=T.UNWRAP_BILINEAR), ("panorama", 25.0, 0.0)
    raise KeyError(name)


NEAREST_CASES = ("a", "b", "c", "d", "e", "f")


def synthetic_sources(n, src_w, src_h, seed=11):
    """Source images without a renderer: smooth gradients plus noise in every channel (all 256 values occur), and a depth ramp."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:src_h, 0:src_w]
    rgba = np.zeros((n, src_h, src_w, 4), np.uint8)
    for k in range(n):
        for ch in range(4):
            smooth = 127.5 + 127.5 * np.sin(0.05 * (ch + 1) * xx + 0.07 * (k + 1) * yy + ch)
            rgba[k, ..., ch] = np.clip(smooth + rng.integers(-40, 41, (src_h, src_w)), 0, 255).astype(np.uint8)
    depth = (rng.random((n, src_h, src_w)) * 0.5 + 0.5).astype(np.float32)
    return rgba, depth
