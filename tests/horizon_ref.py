"""Expected horizons from per-pixel winners and depths (the oracle's render_winners()): per column, the topmost pixel a triangle
won, its depth, and the tile and cell of that triangle in the viewshed's numbering (tests/viewshed_ref.py)."""
from __future__ import annotations

import numpy as np

from viewshed_ref import NO_TRI, geo_order

FIELDS = ("row", "depth", "lat_deg", "lon_deg", "cell_x", "cell_y")      # what the winners determine (the fan piece is not in them)


def horizon(depth, winners, locs, tile_w, tile_h):
    """One view: depth (H, W) f32 and winners (H, W) u32 (rank * 2(w-1)(h-1) + triangle, NO_TRI = sky) -> {field: (W,) array}.
    row -1 and depth 1.0 for an all-sky column; ranks follow geo_order(locs), the tile set the frame was rendered with."""
    depth = np.asarray(depth, np.float32)
    win = np.asarray(winners, np.uint32)
    H, W = win.shape
    terrain = win != NO_TRI
    has = terrain.any(axis=0)
    top = np.where(has, terrain.argmax(axis=0), 0)
    cols = np.arange(W)
    ids = np.where(has, win[top, cols], 0).astype(np.int64)
    tris = 2 * (tile_w - 1) * (tile_h - 1)
    rank, tri = ids // tris, ids % tris
    cell = tri >> 1
    order = geo_order(locs)
    assert not has.any() or rank[has].max() < len(order)
    lat = np.array([order[int(r)][0] if h else 0 for r, h in zip(rank, has)], np.int32)
    lon = np.array([order[int(r)][1] if h else 0 for r, h in zip(rank, has)], np.int32)
    return {"row": np.where(has, top, -1).astype(np.int32),
            "depth": np.where(has, depth[top, cols], np.float32(1.0)).astype(np.float32),
            "lat_deg": lat, "lon_deg": lon,
            "cell_x": np.where(has, cell // (tile_h - 1), 0).astype(np.uint32),
            "cell_y": np.where(has, cell % (tile_h - 1), 0).astype(np.uint32)}


def mismatches(got, want, field):
    """Columns where the record field differs (depth compared as bits)."""
    g, w = np.asarray(got[field]), np.asarray(want[field])
    if field == "depth":
        g, w = g.astype(np.float32).view(np.uint32), w.astype(np.float32).view(np.uint32)
    return np.nonzero(g != w)[0]


def assert_view(got, want, what, frame_depth=None):
    """got: (W,) records of one view; want: horizon_ref dict; frame_depth: (H, W) depth output of the same view."""
    for f in FIELDS:
        bad = mismatches(got, want, f)
        assert len(bad) == 0, f"{what}: {f} differs in {len(bad)} columns (first {bad[0]}: got {got[f][bad[0]]}, want {want[f][bad[0]]})"
    assert np.isin(got["fan"], (0, 1)).all() and (got["_reserved"] == 0).all(), what
    if frame_depth is not None:
        fd = np.asarray(frame_depth, np.float32)
        rows = got["row"]
        at = np.where(rows >= 0, fd[np.clip(rows, 0, None), np.arange(len(rows))], np.float32(1.0))
        assert np.array_equal(at.view(np.uint32), got["depth"].view(np.uint32)), f"{what}: depth differs from the frame's depth output"
        top = np.where(rows >= 0, rows, fd.shape[0])
        sky_above = np.arange(fd.shape[0])[:, None] < top[None, :]
        assert (fd[sky_above] == 1.0).all(), f"{what}: terrain depth above the reported row"


FRAMES = [
    # tile, n_lat, n_lon, eye_dh, W, H, [(yaw, pitch, fov)]  -- test_viewshed_gpu.py's frames, then an odd width and the mosaic's edge
    (96, 2, 2, 50.0, 256, 128, [(40, 10, 70), (250, 0, 60)]),
    (96, 2, 2, 100.0, 200, 150, [(120, 60, 90)]),                  # near clip / big triangles
    (64, 1, 1, 400.0, 160, 160, [(10, 85, 100), (300, 70, 80)]),   # pitch 85: terrain up to row 0
    (12, 2, 2, 60.0, 640, 480, [(10, 35, 110), (200, 80, 110), (100, 5, 110)]),   # the coarse mesh: every triangle large
    (96, 2, 2, 80.0, 333, 97, [(70, 3, 75)]),                      # a width that is no multiple of 64
    (64, 1, 1, 50.0, 190, 100, [(0, -27, 60), (90, -27, 60), (180, -27, 60), (270, -27, 60)]),   # out past the mosaic: sky columns
]
