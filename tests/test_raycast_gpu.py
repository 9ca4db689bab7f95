"""Ray queries on the GPU (topo_raycast_*, topo_sunlit_map_device): k_raycast and k_sunlit_map against the numpy reference (tests/los_ref.py) and the g++ build of the same
traversal (tests/los_emul.py) on the cases of tests/los_cases.py, the calls' contract, and their side effects (none)."""
import hashlib

import numpy as np
import pytest

import los_cases as LC
import los_emul as LE
import los_ref as LR
from gpu_support import checked_run, renderer, strip, sunlit_map

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(LC.CASES))
def test_cases(topo, name):
    tiles, order, rays, ref = LC.case(name)
    g = renderer(topo, tiles, order)
    got = g.raycast(rays)
    LR.compare(ref, got, rays, order, tiles[0][0].shape[0], 1e-3, name)
    emu, _ = LE.raycast(tiles, order, rays)
    LC.against_emulation(got, emu, rays, name, ~ref["ambiguous"])
    g.close()


def test_invalid_rays_and_the_calls_contract(topo):
    import torch
    tiles, order, rays, ref = LC.case("blocks")
    g = renderer(topo, tiles, order)
    planted, idx = LC.with_invalid(rays)
    clean, got = g.raycast(rays), g.raycast(planted)
    assert (got["kind"][idx] == topo.RAY_INVALID).all()
    assert not got["t"][idx].any() and not got["cell_x"][idx].any()
    rest = np.ones(len(rays), bool)
    rest[idx] = False
    assert got[rest].tobytes() == clean[rest].tobytes(), "the neighbours of an invalid ray are untouched"
    # the device variant: the same bytes; an odd count; bytes behind the records left alone
    n = len(planted) - 3
    r_dev = torch.from_numpy(planted.view(np.uint8).reshape(-1, 64).copy()).cuda()
    out = torch.full((n + 2, 64), 0xAB, dtype=torch.uint8, device="cuda")
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    g.raycast_device(r_dev.data_ptr(), out.data_ptr(), n)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert o[:n].tobytes() == got[:n].tobytes() and (o[n:] == 0xAB).all()
    # n = 0 is a no-op; null and misaligned pointers are refused
    g.raycast_device(0, 0, 0)
    assert len(g.raycast(rays[:0])) == 0
    L = topo.lib()
    vp = lambda a: a.ctypes.data_as(topo.C.c_void_p)
    one = np.zeros(1, topo.RAY_HIT_DTYPE)
    assert L.topo_raycast_read(g._h, 1, None, vp(one)) == topo.TOPO_ERR_INVALID
    assert L.topo_raycast_read(g._h, 1, vp(rays), None) == topo.TOPO_ERR_INVALID
    for a, b in ((0, out.data_ptr()), (r_dev.data_ptr(), 0), (r_dev.data_ptr() + 8, out.data_ptr()), (r_dev.data_ptr(), out.data_ptr() + 8)):
        with pytest.raises(topo.TopoError) as e:
            g.raycast_device(a, b, 4)
        assert e.value.code == topo.TOPO_ERR_INVALID
    g.close()


def test_no_tiles_and_tile_set_changes(topo):
    tiles, order, rays, ref = LC.case("long")
    g = topo.TerrainRenderer(64, 48)
    planted, idx = LC.with_invalid(rays)
    got = g.raycast(planted)
    want = np.zeros(len(rays), np.int32)
    want[idx] = topo.RAY_INVALID
    assert (got["kind"] == want).all(), "with no tiles every valid ray misses"
    for (lat, lon), t in zip(order, tiles):
        g.add_terrain(lat, lon, *t)
    LR.compare(ref, g.raycast(rays), rays, order, tiles[0][0].shape[0], 1e-3, "long")
    # the middle tile unloaded: the tables follow the tile set
    g.unload_terrain(*order[1])
    rest_t, rest_o = [tiles[0], tiles[2]], [order[0], order[2]]
    ref2 = LR.cast(LR.Mesh(rest_t), rays)
    assert (ref2["kind"] != ref["kind"]).any() or (ref2["t"] != ref["t"]).any()
    LR.compare(ref2, g.raycast(rays), rays, rest_o, tiles[0][0].shape[0], 1e-3, "long without its middle tile")
    g.add_terrain(order[1][0], order[1][1], *tiles[1])
    LR.compare(ref, g.raycast(rays), rays, order, tiles[0][0].shape[0], 1e-3, "long again")
    g.close()


def test_consistent_with_the_ground_queries(topo):
    """tests/test_ray_check_cpu.py's ne_2x2 scene: the ray from camera_pos towards a pixel's ground point hits the triangle the ground
    record names for at least 0.999 of the pixels at least 0.03 barycentric inside their triangle (the statistic and threshold the
    oracle is held to there), at the record's range to 1e-2 m (both rounded to f32)."""
    from scenes import Scene, relief
    sc = Scene(24, 2, 2, lat0=45, lon0=15, eye_dh=4000.0, height_fn=relief)
    W, H = 96, 64
    g = topo.TerrainRenderer(W, H)
    sc.load(g)
    u = sc.uniforms(W, H, 30.0, 25.0, 60.0, 1)
    g.update(W, H, u, topo.post_uniforms(W, H))
    g.render()
    ys, xs = np.mgrid[0:H, 0:W]
    rec = g.ground(np.stack([np.zeros(W * H, np.int64), xs.reshape(-1), ys.reshape(-1)], axis=1))
    t = rec["kind"] == topo.GROUND_TERRAIN
    assert t.sum() > 0.25 * W * H
    rec = rec[t]
    eye = np.asarray(np.ascontiguousarray(u).view(np.float32)[32:35], np.float64)      # camera_pos
    pts = LC.ecef(rec["lon_deg"], rec["lat_deg"], 0.0)
    pts *= ((LC.R0 + rec["height_m"].astype(np.float64)) / LC.R0)[:, None]
    hit = g.raycast(topo.rays(eye, pts - eye, 0.0, 2.0))
    w0 = 1.0 - rec["w1"] - rec["w2"]
    inner = np.minimum(np.minimum(rec["w1"], rec["w2"]), w0) >= 0.03
    assert inner.sum() > 0.15 * W * H
    same = (hit["kind"] == topo.RAY_HIT) & (hit["tile_lat_deg"] == rec["tile_lat_deg"]) & (hit["tile_lon_deg"] == rec["tile_lon_deg"]) \
        & (hit["cell_x"] == rec["cell_x"]) & (hit["cell_y"] == rec["cell_y"]) & (hit["tri"] == rec["tri"])
    share = float(same[inner].mean())
    print(f"ground consistency: {int(inner.sum())} interior pixels, same triangle {share:.5f}")
    assert share >= 0.999
    k = inner & same
    rng = hit["t"][k] * np.linalg.norm(pts[k] - eye, axis=1)
    err = np.abs(rng - rec["range_m"][k].astype(np.float64))
    print(f"ground consistency: largest range difference {err.max():.3e} m")
    # height_m is an f32 (0.25 mm steps at 3 km) and so is range_m (2 mm steps at 20 km): 1e-2 m holds both
    assert err.max() <= 1e-2
    assert (hit["front"][k] == 1).all()
    g.close()


def test_ray_calls_change_no_frame_and_no_mask(topo):
    from scenes import Scene, assert_same_frame
    sc = Scene(96, 2, 2, eye_dh=100.0)
    W, H = 256, 160
    a, b = topo.TerrainRenderer(W, H), topo.TerrainRenderer(W, H)
    sc.load(a)
    sc.load(b)
    a.viewshed_enable(True)
    b.viewshed_enable(True)
    pu = topo.post_uniforms(W, H)
    tiles, order = LC.scene_tiles(sc)
    rays = LC.eye_rays(sc, 40, 24, 40.0, 10.0, 70.0)
    sun = LC.sun_of(sc)
    import torch
    layer = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    first = None
    for yaw, pitch, fov in ((40, 10, 70), (120, 60, 90), (300, 2, 50)):
        u = sc.uniforms(W, H, yaw, pitch, fov, 0)
        a.update(W, H, u, pu)
        b.update(W, H, u, pu)
        got = b.raycast(rays)
        assert first is None or got.tobytes() == first.tobytes()
        first = got
        ra, rb = a.render(), b.render()
        b.raycast(rays[::3])
        b.sunlit_map_device(sun, layer.data_ptr())
        assert_same_frame(ra, rb, f"rays vs none, yaw {yaw}")
        assert a.counters() == b.counters() and a.frame_status() == b.frame_status()
        assert np.array_equal(a.horizon(), b.horizon())
    assert (first["kind"] == topo.RAY_HIT).sum() > 100
    b.synchronize()
    assert (layer.cpu().numpy() != topo.SUN_NONE).any()
    masks = [(a.viewshed(*loc), b.viewshed(*loc)) for loc in sc.locs]
    assert any(ma.any() for ma, _ in masks) and all(np.array_equal(ma, mb) for ma, mb in masks)
    a.close()
    b.close()


# ---- the sunlit layer (topo_sunlit_map_device) -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(LC.RIDGES))
def test_sunlit_map(topo, orc, name):
    sc, W, H, u, tiles, order, sun, ref, amb, emu = LC.sunlit_case(name, orc)
    g = topo.TerrainRenderer(W, H)
    sc.load(g)
    g.update(W, H, u, topo.post_uniforms(W, H))
    g.render()
    got, pad = sunlit_map(g, sun, 1, W, H, pad_px=5, pad_rows=2)
    assert (pad == 0xAB).all(), "bytes between the width and the pitch, and between the views, are left alone"
    got = got[0]
    terrain = ref != LR.NONE
    counts = {c: int((ref == c).sum()) for c in (LR.LIT, LR.AWAY, LR.SHADOW)}
    print(f"{name}: terrain {int(terrain.sum())}, classes {counts}, ambiguous {int(amb.sum())}")
    for c, k in counts.items():
        assert k >= 0.1 * terrain.sum(), counts
    assert amb.sum() <= 0.005 * W * H
    bad = np.argwhere((got != ref) & ~amb)
    assert len(bad) == 0, f"{len(bad)} pixels differ from the reference, first {tuple(bad[0])}: {got[tuple(bad[0])]} vs {ref[tuple(bad[0])]}"
    bad = np.argwhere((got != emu) & ~amb)
    assert len(bad) == 0, f"{len(bad)} pixels differ from the emulation, first {tuple(bad[0])}"
    dense, _ = sunlit_map(g, 3.0 * sun, 1, W, H)
    assert np.array_equal(dense[0], got), "sun_dir is normalised"
    g.close()


def test_sunlit_sub_range_and_frames_in_flight(topo):
    """A sub-range of the views of an 8-sector submission, and the map queued with pipeline depth 2 before topo_join."""
    import torch
    from scenes import Scene
    sc = Scene(32, 2, 2, eye_dh=6000.0, height_fn=LC.ridges)
    sw, sh = 48, 40
    sun = LC.sun_of(sc)
    tiles, order = LC.scene_tiles(sc)
    g = topo.TerrainRenderer(sw, sh)
    sc.load(g)
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    us = sc.panorama(sw, sh, yaw0_deg=25.0)
    keep = strip(g, us, sw, sh)
    full, _ = sunlit_map(g, sun, 8, sw, sh)
    part, pad = sunlit_map(g, sun, 4, sw, sh, first=3, pad_px=3, pad_rows=1)
    assert np.array_equal(part, full[3:7]) and (pad == 0xAB).all()
    assert all((full == c).sum() > 50 for c in (topo.SUN_NONE, topo.SUN_LIT, topo.SUN_AWAY, topo.SUN_SHADOW)), np.bincount(full.ravel(), minlength=4)
    # ... and it is the class of each pixel's own ground record (f32 weights: a pixel may differ where its point sits on an edge)
    ys, xs, vs = np.meshgrid(np.arange(sh), np.arange(sw), np.arange(8), indexing="ij")
    rec = g.ground(np.stack([vs.ravel(), xs.ravel(), ys.ravel()], axis=1)).reshape(sh, sw, 8).transpose(2, 0, 1)
    assert np.array_equal(rec["kind"] == topo.GROUND_TERRAIN, full != topo.SUN_NONE)
    composed = LC.compose_sunlit(tiles, order, rec, sun)
    assert (composed != full).mean() <= 0.005, float((composed != full).mean())
    # two submissions in flight, the map queued behind the second before the join
    g.set_pipeline_depth(2)
    keep2 = [strip(g, us[:2], sw, sh), strip(g, us[2:7], sw, sh)]
    buf = torch.full((5 * sh * sw,), 0xAB, dtype=torch.uint8, device="cuda")
    g.sunlit_map_device(sun, buf.data_ptr())
    g.join()
    assert np.array_equal(buf.cpu().numpy().reshape(5, sh, sw), full[2:7])
    del keep, keep2
    torch.cuda.synchronize()
    g.close()


def test_sunlit_errors(topo):
    """tests/test_ground_gpu.py::test_errors' cases, plus a zero and a NaN sun."""
    import torch
    from scenes import Scene
    from viewshed_ref import geo_order
    sc = Scene(64, 2, 2, eye_dh=150.0)
    W, H = 128, 64
    g = topo.TerrainRenderer(W, H)
    sc.load(g)
    sun = LC.sun_of(sc)
    buf = torch.zeros((W * H,), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def invalid(call, what):
        with pytest.raises(topo.TopoError) as e:
            call()
        assert e.value.code == topo.TOPO_ERR_INVALID, what

    L = topo.lib()
    raw = lambda first, n, s, ptr, stride, pitch: L.topo_sunlit_map_device(g._h, first, n, s.ctypes.data_as(topo.C.c_void_p) if s is not None else None, ptr, stride, pitch)
    call = lambda: g.sunlit_map_device(sun, buf.data_ptr(), 0, 1, W * H, W)
    assert raw(0, 1, sun, buf.data_ptr(), W * H, W) == topo.TOPO_ERR_INVALID, "before any frame"
    g.update(W, H, sc.uniforms(W, H, 30, 12, 80, 0), topo.post_uniforms(W, H))
    g.render()
    call()
    invalid(lambda: g.sunlit_map_device(sun, buf.data_ptr(), 1, 1, W * H, W), "view 1")
    invalid(lambda: g.sunlit_map_device(sun, buf.data_ptr(), 0, 2, W * H, W), "two views")
    invalid(lambda: g.sunlit_map_device(sun, buf.data_ptr(), 0, 0, W * H, W), "no views")
    invalid(lambda: g.sunlit_map_device(sun, buf.data_ptr(), 0, 1, W * H, W - 1), "pitch smaller than a row")
    invalid(lambda: g.sunlit_map_device(sun, 0, 0, 1, W * H, W), "null output")
    assert raw(0, 1, None, buf.data_ptr(), W * H, W) == topo.TOPO_ERR_INVALID
    for bad in (np.zeros(3), np.array([np.nan, 0.0, 1.0]), np.array([0.0, np.inf, 0.0])):
        invalid(lambda: g.sunlit_map_device(bad, buf.data_ptr(), 0, 1, W * H, W), f"sun {bad}")
    order = geo_order(sc.locs)
    hts = sc.heights[order[1]] * np.float32(0.7) + np.float32(30.0)
    g.add_terrain(order[1][0], order[1][1], hts, *sc.transform(order[1]))
    invalid(call, "after add_terrain")
    g.render()
    call()
    g.unload_terrain(*order[0])
    invalid(call, "after unload_terrain")
    g.render()
    call()
    g.synchronize()
    assert (buf.cpu().numpy() != topo.SUN_NONE).any()
    g.close()


def _checked_run(T):
    """The blocks and ridges cases (and a void case), the tall and polar cases, then a sunlit map of an odd-sized frame -> hash of
    every output, status."""
    h = hashlib.sha256()
    status = 0
    for name in ("blocks", "ridges_sw", "void_pinf"):
        tiles, order, rays, _ = LC.case(name)
        g = renderer(T, tiles, order)
        h.update(g.raycast(LC.with_invalid(rays)[0]).tobytes())
        status |= g.frame_status()["status"]
        g.close()
    for tiles, order, rays in (LC.batch_scene("tall")[:3], LC.case("polar")[:3]):      # the second batch of 64 blocks; tiles whose row 0 is the pole
        g = renderer(T, tiles, order)
        h.update(g.raycast(rays).tobytes())
        status |= g.frame_status()["status"]
        g.close()
    import torch
    from scenes import Scene
    sc = Scene(24, 2, 2, lat0=-34, lon0=-71, eye_dh=8000.0, height_fn=LC.ridges)
    W, H = 67, 45
    g = T.TerrainRenderer(W, H)
    sc.load(g)
    g.update(W, H, sc.uniforms(W, H, 200.0, 35.0, 79.28, 0), T.post_uniforms(W, H))
    g.render()
    h.update(sunlit_map(g, LC.sun_of(sc), 1, W, H, pad_px=1)[0].tobytes())
    status |= g.frame_status()["status"]
    g.close()
    torch.cuda.synchronize()
    return {"sha": h.hexdigest()[:24], "status": status}


def test_bounds_checked_build_records_no_out_of_range_index(topo):
    got = checked_run("test_raycast_gpu")      # kStatusBounds: an index k_raycast formed was out of range
    assert got["sha"] == _checked_run(topo)["sha"], "the bounds-checked build answers as the product build"
