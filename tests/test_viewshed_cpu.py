"""Viewshed (topo_viewshed_*) without a GPU: the C ABI and its bindings, and the expected-mask helper the GPU tests compare
against (tests/viewshed_ref.py), checked against computations of its own."""
import math
import re
import subprocess

import numpy as np

from viewshed_ref import NO_TRI, expected_masks, geo_order

SYMBOLS = ("topo_viewshed_enable", "topo_viewshed_reset", "topo_viewshed_read")


def test_viewshed_symbols_are_declared_exported_and_bound(topo):
    header = open(topo.HEADER_PATH).read()
    for s in SYMBOLS:
        assert re.search(r"\bint\s+" + s + r"\s*\(", header), s
    assert "topo_debug_viewshed_stats" in open(topo.TEST_HEADER_PATH).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", topo.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (topo_[a-z0-9_]+)", nm))
    L = topo.lib()
    for s in SYMBOLS + ("topo_debug_viewshed_stats",):
        assert s in exported and s in L._topo_symbols, s
        assert getattr(L, s).argtypes is not None


def test_viewshed_calls_reject_a_null_context(topo):
    L = topo.lib()
    assert L.topo_viewshed_enable(None, 1) == topo.TOPO_ERR_INVALID
    assert L.topo_viewshed_reset(None) == topo.TOPO_ERR_INVALID
    assert L.topo_viewshed_read(None, 45, 15, None, 0, None) == topo.TOPO_ERR_INVALID
    assert L.topo_debug_viewshed_stats(None, None) == topo.TOPO_ERR_INVALID


def test_python_methods_exist(topo):
    for m in ("viewshed_enable", "viewshed_reset", "viewshed", "debug_viewshed_stats"):
        assert callable(getattr(topo.TerrainRenderer, m, None)), m


def test_rust_wrapper_has_viewshed_methods():
    import os
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rust", "topo-hip", "src", "lib.rs")).read()
    for m in ("viewshed_enable", "viewshed_reset", "viewshed"):
        assert re.search(r"pub fn " + m + r"\(", src), m
    # the safe read sizes its buffer from the tile size the wrapper recorded, not from an argument
    assert re.search(r"pub fn viewshed\(&mut self, location: \(i32, i32\)\)", src)
    assert "self.tile_size = Some(" in src


def _cell_by_vertices(tri, w, h):
    """The cell of a triangle from its vertices (oracle/ray_check.py's own index-buffer restatement): the quad's corner (i, j)
    is the smallest vertex of the triangle."""
    from oracle import ray_check as RC
    t = RC.tile_triangles(w, h)[tri]          # (3, 2) vertex ids (i = x, j = y)
    return int(t[:, 0].min()), int(t[:, 1].min())


def test_expected_mask_helper_on_known_winners():
    """Hand-built winners over three tiles given in a scrambled order, both hemispheres: each id is placed by a computation
    that shares nothing with the helper (the triangle's vertices, the draw order written out by hand)."""
    w, h = 7, 5
    locs = [(45, 15), (-3, -71), (45, -2)]
    # BTreeMap<GeoLocation> order written out: |lat| 3 before 45; at lat 45 N, |lon| 2 (W) before 15 (E)
    order = [(-3, -71), (45, -2), (45, 15)]
    assert geo_order(locs) == order
    tris = 2 * (w - 1) * (h - 1)
    rng = np.random.default_rng(11)
    frames, want = [], {loc: np.zeros((h - 1, w - 1), bool) for loc in locs}
    for f in range(3):
        win = np.full((6, 9), NO_TRI, np.uint32)
        for k in range(int(rng.integers(5, 30))):
            rank, tri = int(rng.integers(0, 3)), int(rng.integers(0, tris))
            win[rng.integers(0, 6), rng.integers(0, 9)] = rank * tris + tri
        for v in win.ravel():
            if v != NO_TRI:
                x, y = _cell_by_vertices(int(v) % tris, w, h)
                want[order[int(v) // tris]][y, x] = True
        frames.append(win)
    got = expected_masks(frames, locs, w, h)
    assert set(got) == set(locs)
    for loc in locs:
        assert np.array_equal(got[loc], want[loc]), loc
    assert sum(int(m.sum()) for m in want.values()) > 10
    # both triangles of a cell mark the same cell; the last cell of the last tile is bottom right
    two = expected_masks([np.array([2 * 7, 2 * 7 + 1], np.uint32)], locs, w, h)
    assert int(two[order[0]].sum()) == 1 and two[order[0]][7 % (h - 1), 7 // (h - 1)]
    last = expected_masks([np.array([3 * tris - 1], np.uint32)], locs, w, h)
    assert last[order[2]][h - 2, w - 2] and int(last[order[2]].sum()) == 1


def test_expected_masks_agree_with_f64_ray_cast(orc):
    """On an oracle frame over a 2x2 mosaic, the helper's masks hold the cells an independent f64 ray cast
    (oracle/ray_check.py) hits well inside a triangle, and nearly nothing it does not see at all."""
    import topo_renderer_amd as T
    from oracle import ray_check as RC
    from scenes import Scene
    from scenes import relief
    tile, W, H, yaw, pitch, fov = 24, 96, 64, 30.0, 25.0, 60.0
    sc = Scene(tile, 2, 2, eye_dh=4000.0, height_fn=relief)
    o = orc.OracleRenderer(W, H)
    sc.load(o)
    o.update(W, H, sc.uniforms(W, H, yaw, pitch, fov, 1), np.array([W, H, 100.0, 0.0], np.float32))
    _, ow = o.render_winners()
    got = expected_masks([ow], sc.locs, tile, tile)
    order = geo_order(sc.locs)
    tiles = [(sc.heights[l],) + tuple(T.synth.tile_transform(l[0], l[1], tile, tile)) for l in order]
    rd, rw, mb, _ = RC.ray_cast(tiles, sc.eye, math.radians(yaw), math.radians(pitch), math.radians(fov), W, H)
    tris = 2 * (tile - 1) ** 2
    inner, hit = set(), set()
    for v, b in zip(rw.ravel(), mb.ravel()):
        if v < 0:
            continue
        x, y = _cell_by_vertices(int(v) % tris, tile, tile)
        cell = (order[int(v) // tris], y, x)
        hit.add(cell)
        if b >= 0.03:
            inner.add(cell)
    marked = {(loc, int(y), int(x)) for loc, m in got.items() for y, x in zip(*np.nonzero(m))}
    assert len(inner) > 100 and len(marked) > 100
    assert len(inner - marked) <= 0.01 * len(inner), (len(inner - marked), len(inner))
    assert len(marked - hit) <= 0.01 * len(marked), (len(marked - hit), len(marked))
