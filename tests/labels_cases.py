"""The cases the peak-label tests share (tests/test_labels_cpu.py, tests/test_labels_gpu.py): the reference's ten layout cases
(tests/golden/label_layout_cases.json), seeded random layouts, and the panorama scene of test_visible_peaks_device_entry_point with
its peaks and widths."""
from __future__ import annotations

import functools
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

IMAGE_WIDTHS = (8, 33, 64, 200, 4097)
MAX_ROWS = (1, 2, 8, 64)
N_LAYOUTS = 2000
LAYOUT_SEED = 20240611
BAD_WIDTHS = (np.float32(np.nan), np.float32(np.inf), np.float32(-1.0))

SW, SH, YAW0, N_PEAKS = 200, 120, 33.0, 1500
ROW_HEIGHT = 20.0      # the reference's LINE_HEIGHT + LINE_PADDING


def golden_cases():
    """[(positions, widths, [(x, row), ...])]: the ten cases of the reference's test_layout."""
    with open(os.path.join(HERE, "golden", "label_layout_cases.json")) as f:
        doc = json.load(f)
    return [(c["positions"], c["widths"], [tuple(e) for e in c["expected"]]) for c in doc["cases"]]


@functools.lru_cache(maxsize=None)
def random_layouts():
    """N_LAYOUTS seeded layouts: [(Wi, max_rows, x (n,) uint32, widths (n,) f32)].  Widths: 0, 0.25, integral ones (their right edge
    is a column another label may start at: touching), fractional ones, ones past the edge, bad ones (NaN, inf, -1); layout 0 of every
    image width holds one width larger than the image, and layout 0 of the widest image one that spans more than 64 words."""
    rng = np.random.default_rng(LAYOUT_SEED)
    out = []
    for i in range(N_LAYOUTS):
        Wi = IMAGE_WIDTHS[i % len(IMAGE_WIDTHS)]
        rows = MAX_ROWS[(i // len(IMAGE_WIDTHS)) % len(MAX_ROWS)]
        n = int(rng.integers(3, 48))
        scale = max(2.0, Wi / float(rng.choice([3, 8, 20])))
        x = rng.integers(0, Wi, n).astype(np.uint32)
        w = np.zeros(n, np.float32)
        for j in range(n):
            kind = rng.integers(0, 10)
            if kind == 0:
                w[j] = 0.0
            elif kind == 1:
                w[j] = 0.25
            elif kind <= 4:
                w[j] = float(rng.integers(1, int(scale) + 1))
            elif kind <= 7:
                w[j] = rng.uniform(0.0, scale)
            elif kind == 8:
                w[j] = float(Wi - int(x[j])) + rng.uniform(0.0, 50.0)      # past the edge
            else:
                w[j] = BAD_WIDTHS[int(rng.integers(0, 3))]
        # touching on purpose: a label that starts where an earlier integral one ends
        for j in range(1, n):
            if rng.random() < 0.2 and np.isfinite(w[j - 1]) and w[j - 1] >= 0 and float(w[j - 1]) == int(w[j - 1]) and int(x[j - 1]) + int(w[j - 1]) < Wi:
                x[j] = int(x[j - 1]) + int(w[j - 1])
        if i < len(IMAGE_WIDTHS):
            w[1] = float(Wi) + 3.5
        if i == IMAGE_WIDTHS.index(4097):
            x[2], w[2] = 17, 2100.25
        out.append((Wi, rows, x, w))
    return out


def spans(Wi, x, w):
    """The closed column ranges of the usable labels, by the rule's own words (f32 sum and ceil, saturating, clamped): (index, l, r)."""
    out = []
    for j in range(len(x)):
        if np.isfinite(w[j]) and w[j] >= 0:
            r = float(np.ceil(np.float32(x[j]) + np.float32(w[j])))
            out.append((j, int(x[j]), int(min(r, Wi - 1))))
    return out


def touching_pairs(Wi, x, w):
    s = spans(Wi, x, w)
    return sum(1 for a in range(len(s)) for b in range(a + 1, len(s)) if s[a][2] == s[b][1] or s[b][2] == s[a][1])


# ---- the panorama scene ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def scene():
    from scenes import Scene
    return Scene(96, 2, 2, eye_dh=300.0)


@functools.lru_cache(maxsize=None)
def views(yaw0=YAW0):
    """The panorama's eight views (40 x f32 uniforms each)."""
    return [np.ascontiguousarray(u) for u in scene().panorama(SW, SH, yaw0_deg=yaw0)]


def projs(view_list):
    return np.stack([np.ascontiguousarray(u).view(np.float32).reshape(-1)[:16] for u in view_list])


@functools.lru_cache(maxsize=None)
def peaks():
    from scenes import random_peaks
    return random_peaks(scene(), N_PEAKS)


@functools.lru_cache(maxsize=None)
def widths(n=N_PEAKS, seed=77):
    """Seeded widths in [20, 90], a few of 0, a few of 2000 and a few bad ones."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(20.0, 90.0, n).astype(np.float32)
    pick = rng.permutation(n)
    w[pick[:25]] = 0.0
    w[pick[25:40]] = 2000.0
    w[pick[40:50]] = np.nan
    w[pick[50:60]] = np.inf
    w[pick[60:70]] = -1.0
    return w


@functools.lru_cache(maxsize=None)
def oracle_strip(yaw0=YAW0):
    """The panorama rendered view by view with the oracle: (depth (8, SH, SW) f32, [(visible, xy)] per view from oracle.visible_peaks)."""
    import topo_renderer_amd as T
    from oracle import oracle as O
    o = O.OracleRenderer(SW, SH)
    scene().load(o)
    depth, seen = [], []
    for u in views(yaw0):
        o.update(SW, SH, u, T.post_uniforms(SW, SH))
        depth.append(o.render()[1].copy())
        seen.append(o.visible_peaks(peaks()))
    o.close()
    return np.stack(depth), seen
