"""Expected viewshed masks from per-pixel winners (the oracle's render_winners()): the cells whose triangles won a pixel."""
from __future__ import annotations

import numpy as np

NO_TRI = 0xFFFFFFFF


def geo_order(locs):
    """Draw order of the tiles: BTreeMap<GeoLocation> order, (|lat|, lat > 0, |lon|, lon > 0)."""
    return sorted(locs, key=lambda l: (abs(l[0]), 1 if l[0] > 0 else 0, abs(l[1]), 1 if l[1] > 0 else 0))


def empty_masks(locs, tile_w, tile_h):
    return {loc: np.zeros((tile_h - 1, tile_w - 1), bool) for loc in locs}


def mark(masks, winners, locs, tile_w, tile_h):
    """OR the cells of one frame's winners (draw id = rank * 2(w-1)(h-1) + triangle, NO_TRI = sky) into masks
    ({loc: (h-1, w-1) bool}); ranks follow geo_order(locs), the tile set the frame was rendered with."""
    order = geo_order(locs)
    tris = 2 * (tile_w - 1) * (tile_h - 1)
    ids = np.unique(np.asarray(winners, np.uint32).ravel())
    ids = ids[ids != NO_TRI].astype(np.int64)
    rank, tri = ids // tris, ids % tris
    assert rank.size == 0 or rank.max() < len(order)
    cell = tri >> 1
    x, y = cell // (tile_h - 1), cell % (tile_h - 1)          # triangle_vertices: i = cell / (h-1) is x, j = cell % (h-1) is y
    for r in np.unique(rank):
        sel = rank == r
        masks[order[int(r)]][y[sel], x[sel]] = True
    return masks


def expected_masks(frames_winners, locs, tile_w, tile_h):
    """OR over several frames rendered with the same tiles."""
    masks = empty_masks(locs, tile_w, tile_h)
    for w in frames_winners:
        mark(masks, w, locs, tile_w, tile_h)
    return masks


def assert_masks(g, want, what):
    for loc, m in want.items():
        got = g.viewshed(*loc)
        assert got.shape == m.shape
        bad = np.argwhere(got != m)
        assert len(bad) == 0, f"{what}: tile {loc}: {len(bad)} cells differ (first (y, x) {tuple(bad[0])}: got {got[tuple(bad[0])]}); " \
                              f"{int(m.sum())} expected marked"
