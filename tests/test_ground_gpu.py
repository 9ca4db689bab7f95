"""Ground points on the GPU (topo_ground_*): the exact fields of every pixel equal what the oracle's per-pixel winners and depths
give, and the positions lie within 1e-3 m of the numpy f64 reference (tests/ground_ref.py, itself checked against the f64 ray caster
and the product's lane function on the CPU by tests/test_ground_cpu.py); the dense map equals the list bit for bit."""
import hashlib
import math

import numpy as np
import pytest

import ground_ref as GR
from gpu_support import checked_run, ground_map, pair, strip
from horizon_ref import FRAMES
from scenes import Scene
from viewshed_ref import geo_order

pytestmark = pytest.mark.gpu

FRAME = dict(zip(["2x2_dh50", "2x2_dh100_p60", "1x1_dh400_p85", "coarse12", "odd_width", "past_edge"], FRAMES))


def _scene(cfg):
    tile, nla, nlo, dh, W, H, views = cfg
    return Scene(tile, nla, nlo, eye_dh=dh, vfrac=(0.5, 0.97) if W == 190 else (0.5123, 0.5217))


def _expect(o, sc, W, H, views, pu):
    out = []
    tiles = GR.scene_tiles(sc)
    for u in views:
        o.update(W, H, u, pu)
        d, w = o.render_winners()
        out.append(GR.ground(d, w, tiles, sc.locs, u))
    return out


@pytest.mark.parametrize("name", ["2x2_dh50", "2x2_dh100_p60", "odd_width", "past_edge"])
def test_every_pixel_by_list(topo, orc, name):
    cfg = FRAME[name]
    tile, nla, nlo, dh, W, H, views = cfg
    sc = _scene(cfg)
    g, o = pair(topo, orc, sc, W, H)
    pu = topo.post_uniforms(W, H)
    q = GR.all_pixels(topo, [0], W, H)
    kinds = []
    for yaw, pitch, fov in views:
        u = sc.uniforms(W, H, yaw, pitch, fov, 0)
        g.update(W, H, u, pu)
        frame = g.render()
        got = g.ground(q).reshape(H, W)
        want = _expect(o, sc, W, H, [u], pu)[0]
        what = f"{name} yaw {yaw} pitch {pitch}"
        GR.compare(got, want, what)
        assert np.array_equal(got["depth"].view(np.uint32), np.asarray(frame[1], np.float32).view(np.uint32)), f"{what}: depth differs from the frame's depth output"
        assert (got["kind"] != -3).all(), what
        GR.assert_sky(got, what)
        kinds.append(got["kind"])
    kinds = np.concatenate([k.ravel() for k in kinds])
    assert (kinds == 1).any()
    if name == "past_edge":
        assert (kinds == 0).mean() > 0.2      # sky
    if name == "2x2_dh100_p60":
        assert (kinds == 1).all()             # looking down: the near-clipped giants fill the frame


@pytest.mark.parametrize("name", ["2x2_dh100_p60", "odd_width", "past_edge"])
def test_dense_map_equals_the_list(topo, name):
    cfg = FRAME[name]
    tile, nla, nlo, dh, W, H, views = cfg
    sc = _scene(cfg)
    g = topo.TerrainRenderer(W, H)
    sc.load(g)
    yaw, pitch, fov = views[0]
    g.update(W, H, sc.uniforms(W, H, yaw, pitch, fov, 0), topo.post_uniforms(W, H))
    g.render()
    rec = g.ground(GR.all_pixels(topo, [0], W, H)).reshape(1, H, W)
    vals, pad = ground_map(g, 1, W, H)
    assert len(pad) == 0
    GR.assert_map_is_list(vals, rec, name)
    vals, pad = ground_map(g, 1, W, H, pad_px=5, pad_rows=2)      # a pitch and a view stride larger than a row / a view
    GR.assert_map_is_list(vals, rec, name + " padded")
    assert len(pad) and (pad == 0xAB).all(), "the map wrote between rows or behind the view"
    assert np.isnan(vals[rec["kind"] != 1]).all()
    if name == "past_edge":
        assert (rec["kind"] == 0).any()


def test_submissions_of_several_views(topo, orc):
    """An 8-sector submission (list over every view, map with a first_view offset), then topo_render_batch of nine viewpoints = two
    submissions, of which only the last one answers -- with the views the batch generated itself."""
    import torch
    sc = Scene(96, 2, 2, eye_dh=120.0)
    sw, sh = 64, 48
    g, o = pair(topo, orc, sc, sw, sh)
    pu = topo.post_uniforms(sw, sh)
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    us = sc.panorama(sw, sh, yaw0_deg=25.0)
    keep = strip(g, us, sw, sh)
    got = g.ground(GR.all_pixels(topo, range(8), sw, sh)).reshape(8, sh, sw)
    wants = _expect(o, sc, sw, sh, us, pu)
    for v in range(8):
        GR.compare(got[v], wants[v], f"sector {v}")
    assert np.array_equal(got["depth"], keep[1].cpu().numpy())
    vals, pad = ground_map(g, 4, sw, sh, first=3, pad_px=3, pad_rows=1)
    GR.assert_map_is_list(vals, got[3:7], "sectors 3..6")
    assert (pad == 0xAB).all()
    assert np.array_equal(g.ground([(5, 7, 9)]), got[5, 9, 7].reshape(1))      # (view, x, y)
    # the batch: viewpoints 0..7 are the first submission, viewpoint 8 the second and latest
    rng = np.random.default_rng(4)
    eyes, yaws, suns = [], [], []
    for _ in range(9):
        lat, lon = 45.1 + 1.8 * rng.random(), 15.1 + 1.8 * rng.random()
        key = (int(math.floor(lat)), int(math.floor(lon)))
        ground = topo.synth.height_at(sc.heights[key], key[0], key[1], lon, lat)
        eyes.append(topo.geometry_transform(ground + 80.0, lon, lat)); yaws.append(2 * math.pi * rng.random()); suns.append((lon, lat))
    out = torch.zeros((9, 8, sh, sw, 4), dtype=torch.uint8, device="cuda")
    g.render_batch(eyes, yaws, suns, sw, sh, out.data_ptr(), None)
    assert g.horizon_shape() == (8, sw, sh)
    got = g.ground(GR.all_pixels(topo, range(8), sw, sh)).reshape(8, sh, sw)
    last = list(topo.panorama_uniforms(eyes[8], yaws[8], sw, sh, suns[8][0], suns[8][1], 0))
    wants = _expect(o, sc, sw, sh, last, pu)
    for v in range(8):
        GR.compare(got[v], wants[v], f"batch, last viewpoint, sector {v}")
    assert (got["kind"] == 1).any()
    with pytest.raises(topo.TopoError) as e:
        g.ground([(8, 0, 0)])
    assert e.value.code == topo.TOPO_ERR_INVALID
    g.join()
    torch.cuda.synchronize()


def test_pipeline_depth_2_device_list_before_join(topo, orc):
    import torch
    sc = Scene(96, 2, 2, eye_dh=120.0)
    W, H = 150, 90
    g, o = pair(topo, orc, sc, W, H)
    pu = topo.post_uniforms(W, H)
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    g.set_pipeline_depth(2)
    first = [sc.uniforms(W, H, yaw, 4, 70, 0) for yaw in (0, 60)]
    us = [sc.uniforms(W, H, yaw, 6, 70, 0) for yaw in (130, 200, 290)]
    q = GR.all_pixels(topo, range(3), W, H)
    q_dev = torch.from_numpy(q.view(np.uint32).reshape(-1, 4).copy()).cuda()
    out = torch.full((len(q) * 64,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    keep = [strip(g, first, W, H), strip(g, us, W, H)]      # two submissions in flight
    g.ground_device(q_dev.data_ptr(), out.data_ptr(), len(q))
    g.join()
    got = out.cpu().numpy().view(topo.GROUND_DTYPE).reshape(3, H, W)
    wants = _expect(o, sc, W, H, us, pu)
    for v in range(3):
        GR.compare(got[v], wants[v], f"view {v} in flight")
    assert np.array_equal(got.view(np.uint8), g.ground(q).reshape(3, H, W).view(np.uint8))      # the host read: the same bytes
    # a query outside the submission cannot be refused by a call whose queries live on the device: it reads nothing and says so
    bad = torch.from_numpy(topo.ground_queries([(3, 0, 0), (0, W, 0), (0, 0, H), (2, W - 1, H - 1)]).view(np.uint32).reshape(-1, 4).copy()).cuda()
    out4 = torch.zeros((4 * 64,), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    g.ground_device(bad.data_ptr(), out4.data_ptr(), 4)
    g.join()
    r = out4.cpu().numpy().view(topo.GROUND_DTYPE)
    assert list(r["kind"][:3]) == [topo.GROUND_OUTSIDE] * 3 and r[3] == got[2, H - 1, W - 1]
    del keep
    torch.cuda.synchronize()


def test_errors(topo):
    import torch
    sc = Scene(64, 2, 2, eye_dh=150.0)
    W, H = 128, 64
    g = topo.TerrainRenderer(W, H)
    sc.load(g)
    buf = torch.zeros((W * H * 16,), dtype=torch.uint8, device="cuda")
    qd = torch.zeros((4,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def invalid(call, what):
        with pytest.raises(topo.TopoError) as e:
            call()
        assert e.value.code == topo.TOPO_ERR_INVALID, what

    calls = {"host list": lambda: g.ground([(0, 0, 0)]), "device list": lambda: g.ground_device(qd.data_ptr(), buf.data_ptr(), 1),
             "map": lambda: g.ground_map_device(buf.data_ptr(), 0, 1, W * H * 16, W * 16)}
    for what, call in calls.items():
        invalid(call, what + " before any frame")
    g.update(W, H, sc.uniforms(W, H, 30, 12, 80, 0), topo.post_uniforms(W, H))
    g.render()
    assert g.ground([(0, W - 1, H - 1)]).shape == (1,)
    for q in ((1, 0, 0), (0, W, 0), (0, 0, H), (0xFFFFFFFF, 0, 0)):
        invalid(lambda: g.ground([(0, 0, 0), q]), f"query {q}")
    invalid(lambda: g.ground_map_device(buf.data_ptr(), 1, 1, W * H * 16, W * 16), "map of view 1")
    invalid(lambda: g.ground_map_device(buf.data_ptr(), 0, 2, W * H * 16, W * 16), "map of two views")
    invalid(lambda: g.ground_map_device(buf.data_ptr(), 0, 1, W * H * 16, W * 16 - 16), "pitch smaller than a row")
    invalid(lambda: g.ground_map_device(buf.data_ptr() + 4, 0, 1, W * H * 16, W * 16), "misaligned map")
    order = geo_order(sc.locs)
    hts = sc.heights[order[1]] * np.float32(0.7) + np.float32(30.0)
    g.add_terrain(order[1][0], order[1][1], hts, *sc.transform(order[1]))
    for what, call in calls.items():
        invalid(call, what + " after add_terrain")
    g.render()
    assert (g.ground(GR.all_pixels(topo, [0], W, H))["kind"] == 1).any()
    g.unload_terrain(*order[0])
    for what, call in calls.items():
        invalid(call, what + " after unload_terrain")
    g.render()
    assert g.ground([(0, 0, H - 1)]).shape == (1,)


def test_overflowed_rare_queue(topo, orc):
    import torch
    sc = Scene(12, 2, 2, eye_dh=60.0)
    W, H = 640, 480
    g, o = pair(topo, orc, sc, W, H)
    u, pu = sc.uniforms(W, H, 10, 35, 110, 0), topo.post_uniforms(W, H)
    g.update(W, H, u, pu)
    q = np.ascontiguousarray(GR.all_pixels(topo, [0], W, H)[::97])
    q_dev = torch.from_numpy(q.view(np.uint32).reshape(-1, 4).copy()).cuda()
    out = torch.zeros((len(q) * 64,), dtype=torch.uint8, device="cuda")
    dense = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    rgba = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    g.debug_set_queue_caps(0, 2 | 0x80000000)
    g.render_device(rgba.data_ptr(), W * 4)
    g.ground_device(q_dev.data_ptr(), out.data_ptr(), len(q))
    g.ground_map_device(dense.data_ptr())
    with pytest.raises(topo.TopoError) as e:
        g.ground(q)
    assert e.value.code == topo.TOPO_ERR_CAPACITY
    g.join()      # reported once, by the ground read
    rec = out.cpu().numpy().view(topo.GROUND_DTYPE)
    assert (rec["kind"] == topo.GROUND_INCOMPLETE).all()
    blank = rec.copy()
    blank["kind"] = 0
    assert not blank.view(np.uint8).any()
    assert (dense.cpu().numpy().view(np.uint32) == GR.NAN_BITS).all()
    with pytest.raises(topo.TopoError) as e:
        g.ground(q)      # still the latest submission: still incomplete
    assert e.value.code == topo.TOPO_ERR_CAPACITY
    g.join()
    # topo_render grows the queue and renders again: the latest submission is the complete frame
    g.render()
    assert g.counters()["rare_items"] > 2
    full = GR.all_pixels(topo, [0], W, H)
    GR.compare(g.ground(full).reshape(H, W), _expect(o, sc, W, H, [u], pu)[0], "grow-and-retry")
    g.join()


def test_void_scene(topo):
    """A mosaic whose tiles carry NaN voids: every record is a terrain point with finite values, sky or degenerate."""
    import void_scenes as VS
    sc, void, W, H, pose = VS.relief_case("ne_2x2", "nan")
    g = topo.TerrainRenderer(W, H)
    void.load(g)
    g.update(W, H, sc.uniforms(W, H, *pose), topo.post_uniforms(W, H))
    frame = g.render()
    got = g.ground(GR.all_pixels(topo, [0], W, H)).reshape(H, W)
    assert np.isin(got["kind"], (1, 0, -3)).all()
    t = got["kind"] == 1
    assert t.mean() > 0.25
    for f in ("lon_deg", "lat_deg", "height_m", "range_m", "w1", "w2"):
        assert np.isfinite(got[f]).all(), f
    assert np.array_equal(got["depth"].view(np.uint32), np.asarray(frame[1], np.float32).view(np.uint32))
    assert np.array_equal(got["kind"] == 0, np.asarray(frame[1]) == 1.0)
    vals, _ = ground_map(g, 1, W, H)
    GR.assert_map_is_list(vals, got.reshape(1, H, W), "void scene")
    # the points lie on the mosaic, at the relief's heights (a void vertex would put them thousands of kilometres off)
    assert (got["lon_deg"][t] > 14.99).all() and (got["lon_deg"][t] < 17.01).all() and (got["lat_deg"][t] > 44.99).all() and (got["lat_deg"][t] < 47.01).all()
    assert (got["height_m"][t] > -100.0).all() and (got["height_m"][t] < 3100.0).all()


def test_queries_change_no_frame(topo):
    import torch
    from scenes import assert_same_frame
    sc = Scene(96, 2, 2, eye_dh=100.0)
    W, H = 256, 160
    a, b = topo.TerrainRenderer(W, H), topo.TerrainRenderer(W, H)
    sc.load(a)
    sc.load(b)
    pu = topo.post_uniforms(W, H)
    q = np.ascontiguousarray(GR.all_pixels(topo, [0], W, H)[::7])
    q_dev = torch.from_numpy(q.view(np.uint32).reshape(-1, 4).copy()).cuda()
    out = torch.zeros((len(q) * 64,), dtype=torch.uint8, device="cuda")
    dense = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for yaw, pitch, fov in ((40, 10, 70), (120, 60, 90), (300, 2, 50), (10, 85, 100)):
        u = sc.uniforms(W, H, yaw, pitch, fov, 0)
        a.update(W, H, u, pu)
        b.update(W, H, u, pu)
        ra, rb = a.render(), b.render()
        assert_same_frame(ra, rb, f"queries vs none, yaw {yaw}")
        assert a.counters() == b.counters() and a.frame_status() == b.frame_status()
        before = b.horizon()
        first = b.ground(q)
        b.ground_device(q_dev.data_ptr(), out.data_ptr(), len(q))
        b.ground_map_device(dense.data_ptr())
        assert np.array_equal(b.ground(q).view(np.uint8), first.view(np.uint8))
        assert np.array_equal(b.horizon(), before) and np.array_equal(a.horizon(), before)
    # frames in flight, queried between submissions
    a.set_pipeline_depth(2)
    b.set_pipeline_depth(2)
    sw, sh = 64, 96
    dense8 = torch.zeros((8, sh, sw, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    keep = []
    for k in range(4):
        us = sc.panorama(sw, sh, yaw0_deg=9.0 * k)
        keep.append((strip(a, us, sw, sh), strip(b, us, sw, sh)))
        if k % 2:
            b.ground([(k, 3, 5), (7, sw - 1, sh - 1)])
        else:
            b.ground_map_device(dense8.data_ptr())
    a.join()
    b.join()
    for (ra, da), (rb, db) in keep:
        assert torch.equal(ra, rb) and torch.equal(da, db)
    torch.cuda.synchronize()


def _checked_run(T):
    """Ground queries of the kinds above (single frames of the coarse mesh at an odd width, views in flight, a tile unloaded) ->
    hash of every output, status."""
    import torch
    h = hashlib.sha256()
    status = 0
    sc = Scene(12, 2, 2, eye_dh=60.0)
    W, H = 333, 97
    g = T.TerrainRenderer(W, H)
    sc.load(g)
    pu = T.post_uniforms(W, H)
    q = GR.all_pixels(T, [0], W, H)
    for yaw, pitch in ((10, 35), (200, 80), (100, -20)):
        g.update(W, H, sc.uniforms(W, H, yaw, pitch, 110, 0), pu)
        g.render()
        h.update(g.ground(q).tobytes())
        h.update(ground_map(g, 1, W, H, pad_px=1)[0].tobytes())
        status |= g.frame_status()["status"]
    sc2 = Scene(96, 2, 2, eye_dh=120.0)
    sw, sh = 70, 48
    p = T.TerrainRenderer(sw, sh)
    sc2.load(p)
    p.set_stream(torch.cuda.current_stream().cuda_stream)
    p.set_pipeline_depth(2)
    keep = strip(p, sc2.panorama(sw, sh, yaw0_deg=3.0), sw, sh)
    h.update(p.ground(GR.all_pixels(T, range(1, 7), sw, sh)).tobytes())
    h.update(ground_map(p, 5, sw, sh, first=3)[0].tobytes())
    p.unload_terrain(*geo_order(sc2.locs)[0])
    keep = (keep, strip(p, sc2.panorama(sw, sh, yaw0_deg=30.0), sw, sh))
    h.update(p.ground(GR.all_pixels(T, range(8), sw, sh)).tobytes())
    p.synchronize()
    status |= p.frame_status()["status"]
    torch.cuda.synchronize()
    return {"sha": h.hexdigest()[:24], "status": status}


def test_bounds_checked_build_records_no_out_of_range_index(topo):
    got = checked_run("test_ground_gpu")      # kStatusBounds: an index k_ground / k_ground_map (or any kernel) formed was out of range
    want = _checked_run(topo)
    assert got["sha"] == want["sha"] and got["status"] == want["status"]
