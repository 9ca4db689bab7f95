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
