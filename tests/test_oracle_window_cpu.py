"""The oracle's windowed render (oracle_render_window) against crops of its full render, byte for byte.

The GPU limit tests (test_limits_gpu.py) compare targets of up to 2^31 px against windows of the oracle, which could not
render such a target whole; this pins the windows to the full frame on every kind of frame the parity tests use."""
import math

import numpy as np
import pytest

from scenes import FRAMES, Scene, assert_same_frame


def _windows(rng, W, H, n):
    """1 x 1 windows, windows touching each edge and each corner, the whole target, and random ones."""
    out = [(0, 0, 1, 1), (W - 1, H - 1, 1, 1), (W - 1, 0, 1, 1), (0, H - 1, 1, 1), (0, 0, W, H),
           (0, 0, W, 1), (0, H - 1, W, 1), (0, 0, 1, H), (W - 1, 0, 1, H), (1, 1, W - 2, H - 2)]
    for _ in range(n):
        w, h = int(rng.integers(1, W + 1)), int(rng.integers(1, H + 1))
        out.append((int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), w, h))
    return [r for r in out if r[2] > 0 and r[3] > 0]


def _check_windows(o, W, H, rng, n, what):
    full = o.render()
    for x0, y0, w, h in _windows(rng, W, H, n):
        got = o.render_window(x0, y0, w, h)
        assert_same_frame(got, (full[0][y0:y0 + h, x0:x0 + w], full[1][y0:y0 + h, x0:x0 + w]), f"{what} window ({x0},{y0}) {w}x{h}")


@pytest.mark.parametrize("cfg", FRAMES, ids=[f"f{i}" for i in range(len(FRAMES))])
def test_window_equals_crop_of_frame(topo, orc, cfg):
    tile, n_lat, n_lon, W, H, yaw, pitch, fov, mode, dh = cfg
    sc = Scene(tile, n_lat, n_lon, eye_dh=dh)
    fmt = 1 + FRAMES.index(cfg) % 4
    o = orc.OracleRenderer(W, H, color_format=fmt)
    sc.load(o)
    o.update(W, H, sc.uniforms(W, H, yaw, pitch, fov, mode), topo.post_uniforms(W, H))
    _check_windows(o, W, H, np.random.default_rng(FRAMES.index(cfg)), 12, f"{cfg} format {fmt}")


def test_window_equals_crop_random_frames(topo, orc):
    """About 100 seeded random frames: target sizes from 1 px to a few hundred, all view modes and formats, eyes from
    a few metres (near-plane clipping, giants) to high above the terrain."""
    rng = np.random.default_rng(2026)
    scenes = {}
    for i in range(100):
        tile, n = [(24, 1), (33, 2), (48, 1)][i % 3]
        dh = float(rng.choice([5.0, 60.0, 400.0, 2000.0]))
        key = (tile, n, dh)
        if key not in scenes:
            scenes[key] = Scene(tile, n, n, eye_dh=dh)
        sc = scenes[key]
        W, H = int(rng.integers(1, 97)), int(rng.integers(1, 65))
        if i % 10 == 0:
            W, H = int(rng.integers(150, 260)), int(rng.integers(1, 4))
        fmt, mode = 1 + i % 4, (i // 4) % 3
        o = orc.OracleRenderer(W, H, color_format=fmt)
        sc.load(o)
        u = sc.uniforms(W, H, float(rng.uniform(0, 360)), float(rng.uniform(-20, 85)), float(rng.uniform(30, 120)), mode)
        o.update(W, H, u, topo.post_uniforms(W, H))
        _check_windows(o, W, H, rng, 4, f"random frame {i} {W}x{H} format {fmt} mode {mode}")


def test_window_refuses_pixelise_and_bad_windows(topo, orc):
    sc = Scene(24, 1, 1)
    o = orc.OracleRenderer(16, 8)
    sc.load(o)
    o.update(16, 8, sc.uniforms(16, 8), topo.post_uniforms(16, 8, pixelize_n=20.0))
    with pytest.raises(RuntimeError, match="pixelise"):
        o.render_window(0, 0, 4, 4)
    o.update(16, 8, sc.uniforms(16, 8), topo.post_uniforms(16, 8))
    for bad in [(0, 0, 0, 1), (0, 0, 17, 1), (16, 0, 1, 1), (0, 7, 1, 2), (15, 0, 2, 1)]:
        with pytest.raises(RuntimeError, match="outside"):
            o.render_window(*bad)
    o.render_window(15, 7, 1, 1)
    # a window does not disturb the frame that oracle_visible_peaks reads back
    o.render()
    o.render_window(3, 3, 2, 2)
    assert o.visible_peaks(np.zeros((1, 3), np.float32))[0].shape == (1,)
