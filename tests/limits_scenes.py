"""Frames at the size limits the host accepts, shared by tests/test_limits_gpu.py and its bounds-checked child run.

Run as a script (with TOPO_HIP_LIB pointing at libtopo_hip_check.so) it renders every case once and prints, per case, the
status bits and the bounds record of the frame; tests/test_limits_gpu.py requires all of them clean before it renders the
same cases with the product build and compares them with the oracle."""
from __future__ import annotations

import json
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from scenes import Scene  # noqa: E402

R0 = 6371000.0


def _clip_coords(sc, loc, u):
    """Clip-space positions (h, w, 4) of a tile's vertices in float64 (vs_main without its f32 roundings)."""
    import topo_renderer_amd as T
    hts = sc.heights[loc].astype(np.float64)
    h, w = hts.shape
    rp, mp, ps = (np.asarray(a, np.float64) for a in T.synth.tile_transform(loc[0], loc[1], w, h))
    lon = np.radians((np.arange(w) - rp[0]) * ps[0] + mp[0])
    lat = np.radians((np.arange(h) - rp[1]) * -ps[1] + mp[1])
    r = R0 + hts
    p = np.stack([r * (np.cos(lat)[:, None] * np.cos(lon)[None, :]), r * (np.cos(lat)[:, None] * np.sin(lon)[None, :]),
                  r * np.sin(lat)[:, None] * np.ones((1, w)), np.ones((h, w))], axis=-1)
    M = np.asarray(u, np.float32)[:16].astype(np.float64).reshape(4, 4)      # column-major: row c is column c
    return p @ M


def _regions(x0, x1, y0, y1, W, H):
    """64 x 64 px regions of the pixel box [x0, x1] x [y0, y1] clamped to the target (0 where it misses the target)."""
    x0, y0 = np.maximum(np.floor(x0), 0), np.maximum(np.floor(y0), 0)
    x1, y1 = np.minimum(np.ceil(x1), W - 1), np.minimum(np.ceil(y1), H - 1)
    ok = (x0 <= x1) & (y0 <= y1)
    n = (np.floor(x1 / 64) - np.floor(x0 / 64) + 1) * (np.floor(y1 / 64) - np.floor(y0 / 64) + 1)
    return np.where(ok, n, 0)


def _cell_triangles(c, i, j):
    """The two triangles of cell (i, j) in clip space, as triangle_vertices orders them."""
    a, b, cc, d = c[j, i], c[j + 1, i], c[j, i + 1], c[j + 1, i + 1]
    return ((a, b, d), (d, cc, a)) if (i + j) % 2 == 0 else ((a, b, cc), (d, cc, b))


def _clipped_box(tri, W, H, pad, front_only=False):
    """Pixel box (x0, x1, y0, y1) of a triangle clipped to the near plane, None if nothing is left, the guard band drops it or
    (front_only) it faces away."""
    poly = []
    for k in range(3):
        p, q = tri[k], tri[(k + 1) % 3]
        if p[2] >= 0:
            poly.append(p)
        if (p[2] >= 0) != (q[2] >= 0):
            I, O = (p, q) if p[2] >= 0 else (q, p)
            poly.append(I + I[2] / (I[2] - O[2]) * (O - I))
    if len(poly) < 3:
        return None
    P = np.array(poly)
    x = (P[:, 0] / P[:, 3] * 0.5 + 0.5) * W
    y = (0.5 - P[:, 1] / P[:, 3] * 0.5) * H
    if np.abs(x).max() > 1.001 * 2 ** 20 or np.abs(y).max() > 1.001 * 2 ** 20:
        return None
    if front_only and (x * np.roll(y, -1) - np.roll(x, -1) * y).sum() >= 0:      # counter-clockwise on screen: negative area
        return None
    return x.min() - pad, x.max() + pad, y.min() - pad, y.max() + pad


def queue_bound(sc, views, W, H):
    """An upper bound on the BigItems (one per triangle and overlapped 64 x 64 region) a submission can reserve, from the
    vertices projected in float64: a cell whose corners are all in front of the near plane gives each of its two triangles at
    most the regions of the corners' pixel box (+1 px); a cell that crosses the plane, each of its triangles' two fan pieces
    the regions of the clipped triangle's box (+2 px), or of the whole target when there are too many such cells to walk."""
    whole = math.ceil(W / 64) * math.ceil(H / 64)
    total = 0
    for u in views:
        for loc in sc.locs:
            c = _clip_coords(sc, loc, u)
            front = c[..., 2] >= 0
            with np.errstate(all="ignore"):
                sx = (c[..., 0] / c[..., 3] * 0.5 + 0.5) * W
                sy = (0.5 - c[..., 1] / c[..., 3] * 0.5) * H
            q = [(slice(0, -1), slice(0, -1)), (slice(1, None), slice(0, -1)), (slice(0, -1), slice(1, None)), (slice(1, None), slice(1, None))]
            xs, ys, fr = [sx[a] for a in q], [sy[a] for a in q], [front[a] for a in q]
            all_front, any_front = fr[0] & fr[1] & fr[2] & fr[3], fr[0] | fr[1] | fr[2] | fr[3]
            with np.errstate(all="ignore"):
                n = _regions(np.minimum.reduce(xs) - 1, np.maximum.reduce(xs) + 1, np.minimum.reduce(ys) - 1, np.maximum.reduce(ys) + 1, W, H)
            n = np.where(np.isfinite(n), n, whole)
            total += int(2 * np.where(all_front, n, 0).sum())
            crossing = np.argwhere(any_front & ~all_front)
            if len(crossing) > 4000:
                total += 4 * whole * len(crossing)
                continue
            for j, i in crossing:
                for tri in _cell_triangles(c, i, j):
                    box = _clipped_box(tri, W, H, 2.0)
                    total += 0 if box is None else 2 * int(_regions(*box, W, H))
    return total


def largest_triangle_regions(sc, u, W, H):
    """The most 64 x 64 regions any one front-facing triangle (or near-plane fan piece) of the frame covers, in float64."""
    best = 0
    for loc in sc.locs:
        c = _clip_coords(sc, loc, u)
        h, w = c.shape[:2]
        for i in range(w - 1):
            for j in range(h - 1):
                for tri in _cell_triangles(c, i, j):
                    box = _clipped_box(tri, W, H, 0.0, front_only=True)
                    if box is not None:
                        best = max(best, int(_regions(*box, W, H)))
    return best


NEAR = dict(tile=64, n_lat=2, n_lon=2, eye_dh=100.0)                          # 1.7 km cells seen from 100 m: giants, near-plane cuts
MOSAIC = dict(tile=720, n_lat=2, n_lon=2, vfrac=(0.08, 0.07), eye_dh=900.0)      # far blocks behind the occlusion split
POSES = [(10, 35, 110, 0), (77, 60, 100, 1), (200, 45, 90, 2), (300, 20, 90, 0)]
# name: scene, W, H, views (yaw, pitch, fov, mode), colour format, occlusion split (None: the default)
CASES = {
    "wide": ("near", 65536, 256, [(10, 35, 110, 0)], 1, None),
    "tall": ("near", 256, 65536, [(77, 60, 100, 1)], 2, None),
    "column": ("near", 1, 65536, [(10, 35, 110, 2)], 3, None),
    "row": ("near", 65536, 1, [(10, 35, 110, 0)], 4, None),
    "mosaic_wide": ("mosaic", 65536, 256, [(45, 4, 50, 0)], 3, 20000.0),
    "giant": ("near", 16384, 16448, [(77, 60, 100, 2)], 4, None),      # 256 region columns x 257 rows, one giant covers all
    "view_2g": ("near", 65536, 32800, [(10, 35, 110, 0)], 1, None),   # one view of 2^31 + 2^22 px
    "views_4g": ("near", 8191, 8191, POSES * 16, 2, None),           # 64 views, 2^32 - 1 048 512 px
}
_SCENES = {}


def scene(kind):
    if kind not in _SCENES:
        _SCENES[kind] = Scene(**(NEAR if kind == "near" else MOSAIC))
    return _SCENES[kind]


def case_views(name):
    kind, W, H, poses, fmt, split = CASES[name]
    sc = scene(kind)
    return sc, W, H, [sc.uniforms(W, H, *p) for p in poses], fmt, split


def new_renderer(T, name):
    """A renderer for the case with its scene loaded and its big queue sized above queue_bound (no giant may fall back to
    the owner lane's raster_box: on these targets that is a walk of up to 10^9 px by one lane)."""
    sc, W, H, views, fmt, split = case_views(name)
    r = T.TerrainRenderer(W, H, color_format=fmt)
    sc.load(r)
    per_pose = {}
    for p, u in zip(CASES[name][3], views):
        if p not in per_pose:
            per_pose[p] = queue_bound(sc, [u], W, H)
    bound = sum(per_pose[p] for p in CASES[name][3])
    r.debug_set_queue_caps(max(1 << 22, bound + bound // 4 + 4096), 0)
    if split is not None:
        r.set_occlusion_split(split)
    r.update(W, H, views[0], T.post_uniforms(W, H))
    return r, views


def render_device(r, views, W, H, want_depth=True):
    """All views in one submission into fresh device tensors (n, H, W, 4) / (n, H, W); waits for the frame."""
    import torch
    n = len(views)
    rgba = torch.empty((n, H, W, 4), dtype=torch.uint8, device="cuda")
    depth = torch.empty((n, H, W), dtype=torch.float32, device="cuda") if want_depth else None
    r.render_views_device(views, W, H, rgba.data_ptr(), H * W * 4, W * 4, depth.data_ptr() if want_depth else 0, H * W * 4, W * 4)
    r.synchronize()
    return rgba, depth


def run(T, names):
    import torch
    out = {}
    for name in names:
        _, W, H, _, _, _ = case_views(name)
        r, views = new_renderer(T, name)
        rgba, depth = render_device(r, views, W, H)
        st = r.frame_status()
        out[name] = {"status": st["status"] & 3, "bounds_violation": st["bounds_violation"], "bounds_site": st["bounds_site"],
                     "bounds_value": st["bounds_value"]}
        del rgba, depth
        r.close()
        torch.cuda.empty_cache()
    return {"lib": T.LIB_PATH, "cases": out}


if __name__ == "__main__":
    import topo_renderer_amd as T
    print(json.dumps(run(T, sys.argv[1:] or list(CASES))))
