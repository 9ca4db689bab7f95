"""The map view on the GPU (topo_map_*): k_map against the g++ build of the same header run the same way (tests/map_emul.py), fed
the product's own normals (read_normals) and the masks topo_viewshed_read reports -- byte for byte -- on grids sized by the rows a
wave owns (R) and the 64 columns of a wave; the calls' contract; the seen layer behind frames; and their side effects (none)."""
import hashlib

import numpy as np
import pytest

import los_cases as LC
import map_cases as MC
import map_emul as ME
import map_ref as MR
import surface_cases as SC
from gpu_support import checked_run, renderer, strip

pytestmark = pytest.mark.gpu

R = MC.R
SENTINEL = 0xAB
COLOURS = dict(void_rgba=(10, 20, 30, 40), seen_rgba=(255, 208, 0, 96), contour_rgba=(96, 64, 32, 160), index_rgba=(64, 32, 16, 255))


def _mosaic_96():
    """2 x 2 synthetic tiles of 96 posts at 45N 15E: a tile's last column stops a post short of its neighbour (a one-cell gap)."""
    from scenes import Scene
    sc = Scene(96, 2, 2, eye_dh=100.0)
    return (sc,) + LC.scene_tiles(sc)


def _ragged_2x2():
    """2 x 2 tiles of 130 x 34 posts (ragged raster blocks) at 46N 7E."""
    import topo_renderer_amd as T
    order = [(la, lo) for la, lo in LC.LR.geo_order([(46, 7), (46, 8), (47, 7), (47, 8)])]
    return [(LC.blocks_heights(la, lo, 130, 34),) + tuple(T.synth.tile_transform(la, lo, 130, 34)) for la, lo in order], order


def _params(topo, lon_a, lon_b, lat_a, lat_b, nx, ny, interval=40.0, every=5, layers=None, **kw):
    g = MC.grid(lon_a, lon_b, lat_a, lat_b, nx, ny)
    return topo.map_params(g["lon0"], g["lat0"], g["dlon"], g["dlat"], nx, ny, sun_direction=MC.sun(0.5 * (lon_a + lon_b), min(0.5 * (lat_a + lat_b), 90.0)),
                           contour_interval_m=interval, index_every=every, layers=topo.MAP_RELIEF | topo.MAP_CONTOURS if layers is None else layers, **{**COLOURS, **kw})


def _alloc(p, rgba=True, flags=True, pad_px=3, pad_rows=2):
    """0xAB-filled output tensors whose rows are pad_px pixels and which are pad_rows rows longer than the grid (None for an output
    not wanted), complete on the device when this returns."""
    import torch
    nx, ny = int(p["nx"][0]), int(p["ny"][0])
    img = torch.full((ny + pad_rows, nx + pad_px, 4), SENTINEL, dtype=torch.uint8, device="cuda") if rgba else None
    flg = torch.full((ny + pad_rows, nx + pad_px), SENTINEL, dtype=torch.uint8, device="cuda") if flags else None
    torch.cuda.synchronize()
    return img, flg


def _collect(g, p, img, flg):
    """The outputs of a finished call -> (rgba or None, flags or None); the bytes between nx and the pitch and behind the last row
    must be untouched."""
    nx, ny = int(p["nx"][0]), int(p["ny"][0])
    g.synchronize()
    out = []
    for t in (img, flg):
        if t is None:
            out.append(None)
            continue
        a = t.cpu().numpy()
        assert (a[:ny, nx:] == SENTINEL).all() and (a[ny:] == SENTINEL).all(), "bytes beyond a row's end or behind the last row were written"
        out.append(np.ascontiguousarray(a[:ny, :nx]))
    return out


def _device(g, p, rgba=True, flags=True, pad_px=3, pad_rows=2):
    """topo_map_device into padded 0xAB-filled tensors -> (rgba or None, flags or None)."""
    img, flg = _alloc(p, rgba, flags, pad_px, pad_rows)
    g.map_device(p, img, flg)
    return _collect(g, p, img, flg)


def _emulate(g, tiles, order, p, seen=False):
    nrm = [g.read_normals(la, lo) for la, lo in order]
    masks = [g.viewshed(la, lo) for la, lo in order] if seen else None
    rgba, flags, bad, _ = ME.run(tiles, nrm, p, masks, ME.WAVES, rows=int(MC.T.lib().topo_map_rows_per_wave()))
    assert bad == 0
    return rgba, flags


def _same(got, want, what):
    for a, b, name in zip(got, want, ("rgba", "flags")):
        if a is None:
            continue
        diff = np.argwhere(a != b)
        assert len(diff) == 0, f"{what}: {name} differs from the emulation in {len(diff)} bytes, first at {diff[0].tolist()}: {a[tuple(diff[0])]} vs {b[tuple(diff[0])]}"


def test_grid_shapes_around_a_wave_and_a_band(topo):
    """nx in {1, 63, 64, 65, 130} x ny in {1, 2, R, R + 1} over the 2 x 2 mosaic: a lone lane, both sides of a wave edge, a wave with
    a tail, the east halo inside and across waves, the south halo.  The widest grids straddle the seam and the gap between the tiles."""
    sc, tiles, order = _mosaic_96()
    g = renderer(topo, tiles, order)
    for nx in (1, 63, 64, 65, 130):
        for ny in (1, 2, R, R + 1):
            p = _params(topo, 15.7113, 15.7113 + 0.0047 * nx, 46.0731, 46.0731 - 0.0171 * ny, nx, ny, interval=10.0, every=2)
            want = _emulate(g, tiles, order, p)
            got = _device(g, p)
            _same(got, want, f"{nx} x {ny}")
            rd = g.map(p)
            assert np.array_equal(rd[0], got[0]) and np.array_equal(rd[1], got[1]), f"{nx} x {ny}: topo_map_read differs from topo_map_device"
            if nx >= 65 and ny >= R:
                f = got[1]
                assert (f & MR.F_TERRAIN).any() and ((f & MR.F_TERRAIN) == 0).any() and (f & MR.F_CONTOUR).any() and (f & MR.F_INDEX).any(), "terrain, the gap, contours"
                # each output alone; a repeat; both null
                assert np.array_equal(_device(g, p, flags=False)[0], got[0]) and np.array_equal(_device(g, p, rgba=False)[1], got[1])
                again = _device(g, p, pad_px=0, pad_rows=0)
                assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1])
                g.map_device(p, None, None)
                assert g.map(p, rgba=False)[0] is None and g.map(p, flags=False)[1] is None
    g.close()


TILE_SETS = ["ragged", "overlap_higher", "antimeridian", "polar", "long_gap"]


def _tile_set(T, name):
    """(tiles, order, the grids asked of them): 130 columns (two full waves and a tail) by R + 1 rows."""
    if name == "ragged":
        tiles, order = _ragged_2x2()
        return tiles, order, [_params(T, 7.6013, 8.4731, 47.2117, 46.7321, 130, R + 1, interval=25.0),
                              _params(T, 8.4731, 7.6013, 46.7321, 47.2117, 130, R + 1, interval=25.0, every=1),      # columns going west, rows north
                              _params(T, 7.9713, 7.9713, 47.2117, 46.7321, 66, R + 1, interval=25.0, every=0),      # dlon = 0
                              _params(T, 7.6013, 8.4731, 47.2117, 46.7321, 130, R + 1, layers=T.MAP_RELIEF), _params(T, 7.6013, 8.4731, 47.2117, 46.7321, 130, R + 1, layers=0)]
    tiles, order = MC.tile_set(MC.CASES[name][0])
    g0 = MC.CASES[name][1]
    lon_b, lat_b = g0["lon0"] + g0["dlon"] * (g0["nx"] - 1), g0["lat0"] + g0["dlat"] * (g0["ny"] - 1)
    return tiles, order, [_params(T, g0["lon0"], lon_b, g0["lat0"], lat_b, 130, R + 1, interval=MC.CASES[name][2])]


@pytest.mark.parametrize("name", TILE_SETS)
def test_tile_sets(topo, name):
    """The 130 x 34 ragged 2 x 2 set with all layers off and on, an overlap, the antimeridian, the pole, a gap."""
    tiles, order, ps = _tile_set(topo, name)
    g = renderer(topo, tiles, order)
    for i, p in enumerate(ps):
        got = _device(g, p)
        _same(got, _emulate(g, tiles, order, p), f"{name} {i}")
        if int(p["layers"][0]) & topo.MAP_CONTOURS and float(p["dlon_deg"][0]) != 0.0:
            assert (got[1] & MR.F_TERRAIN).mean() > 0.3 and (got[1] & MR.F_CONTOUR).any()
    g.close()


def _behind_a_frame(g, sc, p, W, H):
    """With two frame contexts: a frame queued on its context's own stream and topo_map_device right behind it, nothing waiting in
    between (the outputs were allocated and filled before the frame was queued) -> the map's outputs."""
    import torch
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    g.set_pipeline_depth(2)
    img, flg = _alloc(p)
    keep = strip(g, [sc.uniforms(W, H, 220.0, -25.0, 80.0, 0)], W, H)
    g.map_device(p, img, flg)
    g.join()
    out = _collect(g, p, img, flg)
    assert keep[0].shape[0] == 1
    return out


def test_seen_layer_behind_frames(topo):
    """One small frame with accumulation on, then the map: the seen pixels are exactly those whose (tile, cell) the read-back mask
    marks (the emulation, fed topo_viewshed_read's masks, says which); none after a reset; TOPO_ERR_INVALID without accumulation;
    and with two frame contexts a frame queued and the map right behind it, which must see that frame's marks."""
    sc, tiles, order = _mosaic_96()
    W, H = 96, 64
    g = topo.TerrainRenderer(W, H)
    sc.load(g)
    layers = topo.MAP_RELIEF | topo.MAP_CONTOURS | topo.MAP_SEEN
    p = _params(topo, sc.vlon - 0.21, sc.vlon + 0.23, sc.vlat + 0.17, sc.vlat - 0.19, 130, 2 * R + 1, layers=layers)
    with pytest.raises(topo.TopoError) as e:
        g.map(p)
    assert e.value.code == topo.TOPO_ERR_INVALID
    with pytest.raises(topo.TopoError) as e:
        g.map_device(p, None, None)
    assert e.value.code == topo.TOPO_ERR_INVALID, "refused before anything else, outputs or not"
    g.viewshed_enable(True)
    none = g.map(p)[1]
    assert not (none & MR.F_SEEN).any() and (none & MR.F_TERRAIN).any()
    g.update(W, H, sc.uniforms(W, H, 40.0, -20.0, 70.0, 0), topo.post_uniforms(W, H))
    g.render()
    got = _device(g, p)
    _same(got, _emulate(g, tiles, order, p, seen=True), "seen, one frame")
    seen = (got[1] & MR.F_SEEN) != 0
    assert 10 <= seen.sum() < seen.size and ((got[1] & MR.F_TERRAIN) != 0)[seen].all()
    g.viewshed_reset()
    assert not (g.map(p)[1] & MR.F_SEEN).any()
    # a frame in flight on a context's own stream, the map queued right behind it
    behind = _behind_a_frame(g, sc, p, W, H)
    _same(behind, _emulate(g, tiles, order, p, seen=True), "seen, behind a frame in flight")
    assert ((behind[1] & MR.F_SEEN) != 0).sum() >= 5
    g.close()


def test_no_side_effects_and_tile_set_changes(topo):
    from scenes import assert_same_frame
    sc, tiles, order = _mosaic_96()
    W, H = 128, 80
    g = topo.TerrainRenderer(W, H)
    p = _params(topo, 15.2113, 16.7931, 46.8713, 45.1321, 130, R + 1)
    rgba, flags = g.map(p)
    assert not flags.any() and (rgba == np.uint8(COLOURS["void_rgba"])).all(), "no tiles: every pixel is void"
    sc.load(g)
    g.update(W, H, sc.uniforms(W, H, 40.0, 5.0, 70.0, 0), topo.post_uniforms(W, H))
    before = g.render()
    full = _device(g, p)
    after = g.render()
    assert_same_frame(before, after, "a frame before and after a map call")
    assert (full[1] & MR.F_TERRAIN).mean() > 0.7
    # unload one tile: its pixels turn void, the rest stays (a contour against a pixel of the tile goes with it)
    gone = order[1]
    g.unload_terrain(*gone)
    rest_tiles = [t for t, o in zip(tiles, order) if o != gone]
    rest_order = [o for o in order if o != gone]
    less = _device(g, p)
    _same(less, _emulate(g, rest_tiles, rest_order, p), "after an unload")
    pos = MR.positions(p)
    inside = (pos[..., 0] > gone[1] + 0.001) & (pos[..., 0] < gone[1] + 95.0 / 96.0 - 0.001) & (pos[..., 1] > gone[0] + 1.0 / 96.0 + 0.001) & (pos[..., 1] < gone[0] + 0.999)
    assert inside.any() and not less[1][inside].any() and (full[1][inside] & MR.F_TERRAIN).all()
    far = ~inside & (np.abs(pos[..., 0] - (gone[1] + 0.5)) > 0.55) | ~inside & (np.abs(pos[..., 1] - (gone[0] + 0.5)) > 0.55)
    assert np.array_equal(less[1][far] & MR.F_TERRAIN, full[1][far] & MR.F_TERRAIN)
    g.close()


def test_argument_errors_and_the_size_bound(topo):
    import torch
    sc, tiles, order = _mosaic_96()
    g = renderer(topo, tiles, order)
    p = _params(topo, 15.2, 15.9, 46.8, 46.1, 66, 4)
    img = torch.full((4, 70, 4), SENTINEL, dtype=torch.uint8, device="cuda")
    flg = torch.full((4, 70), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    L = topo.lib()
    vp = lambda a: a.ctypes.data_as(topo.C.c_void_p)
    call = lambda q, rp=img.data_ptr(), rpitch=280, fp=flg.data_ptr(), fpitch=70: L.topo_map_device(g._h, vp(q) if q is not None else None, rp, rpitch, fp, fpitch)
    assert call(p) == topo.TOPO_OK
    bad = [call(None), call(p, rp=img.data_ptr() + 2), call(p, rpitch=282), call(p, rpitch=4 * 65), call(p, fpitch=65)]
    for field, value in (("nx", 0), ("ny", 0), ("lon0_deg", np.nan), ("lat0_deg", np.inf), ("dlon_deg", np.nan), ("dlat_deg", -np.inf), ("contour_interval_m", -1.0),
                         ("contour_interval_m", np.nan), ("contour_interval_m", np.inf), ("layers", 8), ("layers", 0x80000001)):
        q = p.copy()
        q[field] = value
        bad.append(call(q))
    q = p.copy()
    q["sun_direction"][0, 1] = np.nan
    bad.append(call(q))
    assert all(rc == topo.TOPO_ERR_INVALID for rc in bad), bad
    # the surface grid's size bound: ceil(nx / 64) * ny < 2^32, refused with outputs or without
    q = p.copy()
    q["nx"], q["ny"] = 64 * 65536 + 1, 65536
    assert L.topo_map_device(g._h, vp(q), None, 0, None, 0) == topo.TOPO_ERR_INVALID and L.topo_map_read(g._h, vp(q), None, None) == topo.TOPO_ERR_INVALID
    q["nx"] = 64 * 65535
    assert L.topo_map_device(g._h, vp(q), None, 0, None, 0) == topo.TOPO_OK, "just under the bound, and nothing to write"
    # a zero interval switches the contour layer off; a zero index_every the index contours
    q = p.copy()
    q["contour_interval_m"] = 0.0
    assert not (g.map(q)[1] & (MR.F_CONTOUR | MR.F_INDEX)).any()
    g.synchronize()
    a, b = img.cpu().numpy(), flg.cpu().numpy()
    assert (a[:, 66:] == SENTINEL).all() and (b[:, 66:] == SENTINEL).all() and (b[:, :66] != SENTINEL).all()
    g.close()


def _checked_run(T):
    """Every case of this module once: the grid shapes with each output alone, the tile sets' grids, the seen layer behind a frame,
    after a reset and behind a frame in flight, no tiles, a frame beside the call, an unloaded tile, the argument test's grids -> hash
    of every output, status."""
    import torch
    h = hashlib.sha256()
    status = 0

    def take(arrays):
        for a in arrays:
            if a is not None:
                h.update(a.tobytes())

    sc, tiles, order = _mosaic_96()
    g = renderer(T, tiles, order)
    for nx in (1, 63, 64, 65, 130):
        for ny in (1, 2, R, R + 1):
            p = _params(T, 15.7113, 15.7113 + 0.0047 * nx, 46.0731, 46.0731 - 0.0171 * ny, nx, ny, interval=10.0, every=2)
            take(_device(g, p) + list(g.map(p)))
            if nx >= 65 and ny >= R:
                take(_device(g, p, flags=False) + _device(g, p, rgba=False) + _device(g, p, pad_px=0, pad_rows=0) + list(g.map(p, rgba=False)) + list(g.map(p, flags=False)))
                g.map_device(p, None, None)
    p = _params(T, 15.2, 15.9, 46.8, 46.1, 66, 4)      # the argument test's grids
    take(_device(g, p))
    p["contour_interval_m"] = 0.0
    take(g.map(p))
    status |= g.frame_status()["status"]
    g.close()
    for name in TILE_SETS:
        tiles, order, ps = _tile_set(T, name)
        g = renderer(T, tiles, order)
        for p in ps:
            take(_device(g, p) + list(g.map(p)))
        status |= g.frame_status()["status"]
        g.close()
    # the seen layer
    sc, tiles, order = _mosaic_96()
    W, H = 96, 64
    g = T.TerrainRenderer(W, H)
    sc.load(g)
    g.viewshed_enable(True)
    p = _params(T, sc.vlon - 0.21, sc.vlon + 0.23, sc.vlat + 0.17, sc.vlat - 0.19, 130, 2 * R + 1, layers=T.MAP_RELIEF | T.MAP_CONTOURS | T.MAP_SEEN)
    take(g.map(p))
    g.update(W, H, sc.uniforms(W, H, 40.0, -20.0, 70.0, 0), T.post_uniforms(W, H))
    g.render()
    take(_device(g, p))
    g.viewshed_reset()
    take(g.map(p))
    take(_behind_a_frame(g, sc, p, W, H))
    take(g.map(p))      # (a read folds the device call's record into the status)
    status |= g.frame_status()["status"]
    g.close()
    # no tiles, a frame beside the call, an unloaded tile
    W, H = 128, 80
    g = T.TerrainRenderer(W, H)
    p = _params(T, 15.2113, 16.7931, 46.8713, 45.1321, 130, R + 1)
    take(g.map(p))
    sc.load(g)
    g.update(W, H, sc.uniforms(W, H, 40.0, 5.0, 70.0, 0), T.post_uniforms(W, H))
    g.render()
    take(_device(g, p))
    g.render()
    g.unload_terrain(*order[1])
    take(_device(g, p) + list(g.map(p)))
    status |= g.frame_status()["status"]
    g.close()
    torch.cuda.synchronize()
    return {"sha": h.hexdigest()[:24], "status": status}


def test_bounds_checked_build_records_no_out_of_range_index(topo):
    got = checked_run("test_map_gpu")      # kStatusBounds: an index k_map formed was out of range
    assert got["sha"] == _checked_run(topo)["sha"], "the bounds-checked build answers as the product build"
