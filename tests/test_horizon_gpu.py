"""Horizon on the GPU (topo_horizon_*): every column's topmost terrain pixel, depth, tile and cell equal, bit for bit, what the
oracle's per-pixel winners and depths give (render_winners(), tests/horizon_ref.py), and the depth also equals the frame's own
depth output.  (The fan piece of a near-clipped triangle is not part of the oracle's winners: it is checked to be 0 or 1.)"""
import hashlib
import math
import os

import numpy as np
import pytest

from gpu_support import checked_run, padded_device_output, pair, strip
from horizon_ref import FRAMES, assert_view, horizon
from scenes import Scene, assert_same_frame
from viewshed_ref import geo_order

pytestmark = pytest.mark.gpu


def _expect(o, W, H, views, pu, locs, tile):
    out = []
    for u in views:
        o.update(W, H, u, pu)
        d, w = o.render_winners()
        out.append(horizon(d, w, locs, tile, tile))
    return out


def _assert_all(got, wants, what, frame_depths=None):
    assert got.shape[0] == len(wants), (got.shape, len(wants))
    for v, want in enumerate(wants):
        assert_view(got[v], want, f"{what} view {v}", None if frame_depths is None else frame_depths[v])


@pytest.mark.parametrize("cfg", FRAMES, ids=["2x2_dh50", "2x2_dh100_p60", "1x1_dh400_p85", "coarse12", "odd_width", "past_edge"])
def test_single_frames_match_oracle(topo, orc, cfg):
    tile, nla, nlo, dh, W, H, views = cfg
    sc = Scene(tile, nla, nlo, eye_dh=dh, vfrac=(0.5, 0.97) if W == 190 else (0.5123, 0.5217))
    g, o = pair(topo, orc, sc, W, H)
    pu = topo.post_uniforms(W, H)
    rows = []
    for yaw, pitch, fov in views:
        u = sc.uniforms(W, H, yaw, pitch, fov, 0)
        g.update(W, H, u, pu)
        frame = g.render()
        o.update(W, H, u, pu)
        assert_same_frame(frame, o.render(), f"yaw {yaw} pitch {pitch}")
        assert g.horizon_shape() == (1, W, H)
        got = g.horizon()
        assert got.shape == (1, W)
        assert_view(got[0], _expect(o, W, H, [u], pu, sc.locs, tile)[0], f"{cfg[:6]} yaw {yaw} pitch {pitch}", frame[1])
        rows.append(got[0]["row"])
    rows = np.concatenate(rows)
    assert (rows >= 0).any()
    if views[0][1] == 85:
        assert (rows == 0).any()      # terrain reaching the top edge
    if W == 190:
        assert (rows == -1).any()     # all-sky columns


def _device_horizon(g, n, W, first=0, stride=None):
    import topo_renderer_amd as T
    stride = W if stride is None else stride
    rec, _ = padded_device_output(g, n, 1, stride, 32, lambda p, *_: g.horizon_device(p, first, n, stride))
    return rec.view(T.HORIZON_DTYPE).reshape(n, stride)


def test_panorama_world_of_one_and_slot_path(topo, orc):
    import torch
    sc = Scene(96, 2, 2, eye_dh=120.0)
    sw, sh = 96, 160
    g, o = pair(topo, orc, sc, sw, sh)
    pu = topo.post_uniforms(sw, sh)
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    strip = torch.zeros((8, sh, sw, 4), dtype=torch.uint8, device="cuda")
    depth = torch.zeros((8, sh, sw), dtype=torch.float32, device="cuda")
    want = _expect(o, sw, sh, sc.panorama(sw, sh, yaw0_deg=25.0), pu, sc.locs, 96)
    g.render_panorama(None, sc.eye, math.radians(25.0), sw, sh, sc.vlon, sc.vlat, strip.data_ptr(), depth.data_ptr())
    got = g.horizon()
    g.synchronize()
    _assert_all(got, want, "panorama, world of one", depth.cpu().numpy())
    assert (got["row"] >= 0).any()
    os.environ["TOPO_PANORAMA_FORCE_SLOTS"] = "1"
    os.environ["TOPO_PANORAMA_BAND_BYTES"] = str(sw * 4 * 50)
    try:
        assert len(topo.panorama_slots(1, sw, sh)) == 8       # a world of one: k_resolve sector by sector, the query behind the last
        for yaw0 in (25.0, 70.0):
            want = _expect(o, sw, sh, sc.panorama(sw, sh, yaw0_deg=yaw0), pu, sc.locs, 96)
            g.render_panorama(topo.Comm(0, 1), sc.eye, math.radians(yaw0), sw, sh, sc.vlon, sc.vlat, strip.data_ptr(), depth.data_ptr())
            got = g.horizon()
            g.synchronize()
            _assert_all(got, want, f"slot-by-slot panorama yaw0 {yaw0}", depth.cpu().numpy())
            assert np.array_equal(_device_horizon(g, 8, sw), got)
    finally:
        del os.environ["TOPO_PANORAMA_FORCE_SLOTS"], os.environ["TOPO_PANORAMA_BAND_BYTES"]
    torch.cuda.synchronize()


def test_batch_and_views_device(topo, orc):
    """topo_render_batch (3 viewpoints = one submission of 24 views, pipeline depth 2) and topo_render_views_device with several
    views, through horizon() and horizon_device() (into a torch tensor, with a view range and a wider stride)."""
    import torch
    sc = Scene(96, 2, 2, eye_dh=120.0)
    sw, sh = 96, 130
    g, o = pair(topo, orc, sc, sw, sh)
    pu = topo.post_uniforms(sw, sh)
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(4)
    eyes, yaws, suns = [], [], []
    for _ in range(3):
        lat, lon = 45.1 + 1.8 * rng.random(), 15.1 + 1.8 * rng.random()
        key = (int(math.floor(lat)), int(math.floor(lon)))
        ground = topo.synth.height_at(sc.heights[key], key[0], key[1], lon, lat)
        eyes.append(topo.geometry_transform(ground + 80.0, lon, lat)); yaws.append(2 * math.pi * rng.random()); suns.append((lon, lat))
    out = torch.zeros((3, 8, sh, sw, 4), dtype=torch.uint8, device="cuda")
    dout = torch.zeros((3, 8, sh, sw), dtype=torch.float32, device="cuda")
    g.set_pipeline_depth(2)
    g.render_batch(eyes, yaws, suns, sw, sh, out.data_ptr(), dout.data_ptr())
    assert g.horizon_shape() == (24, sw, sh)
    got = g.horizon()
    g.join()
    views = []
    for v in range(3):
        views += list(topo.panorama_uniforms(eyes[v], yaws[v], sw, sh, suns[v][0], suns[v][1], 0))
    _assert_all(got, _expect(o, sw, sh, views, pu, sc.locs, 96), "batch of three viewpoints", dout.reshape(24, sh, sw).cpu().numpy())
    assert np.array_equal(_device_horizon(g, 24, sw), got)
    # five views of an odd width, one submission
    W, H = 150, 90
    us = [sc.uniforms(W, H, yaw, 4, 70, 0) for yaw in (0, 60, 130, 200, 290)]
    rgba, depth = strip(g, us, W, H)
    sub = _device_horizon(g, 2, W, first=2, stride=W + 13)
    got = g.horizon()
    g.join()
    _assert_all(got, _expect(o, W, H, us, pu, sc.locs, 96), "five views", depth.cpu().numpy())
    assert np.array_equal(sub[:, :W], got[2:4]) and (sub[:, W:].view(np.uint8) == 0xAB).all()
    assert np.array_equal(g.horizon(3, 1), got[3:4])
    for first, n in ((5, 1), (4, 2), (0, 6)):
        with pytest.raises(topo.TopoError) as e:
            g.horizon(first, n)
        assert e.value.code == topo.TOPO_ERR_INVALID, (first, n)
    torch.cuda.synchronize()


def test_queue_overflow(topo, orc):
    import torch
    sc = Scene(12, 2, 2, eye_dh=60.0)
    W, H = 640, 480
    g, o = pair(topo, orc, sc, W, H)
    u, pu = sc.uniforms(W, H, 10, 35, 110, 0), topo.post_uniforms(W, H)
    g.update(W, H, u, pu)
    want = _expect(o, W, H, [u], pu, sc.locs, 12)
    # an asynchronous frame that overflows: the host read says so, the device variant writes -2, the next join() is clean
    g.debug_set_queue_caps(0, 2 | 0x80000000)
    rgba = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    g.render_device(rgba.data_ptr(), W * 4)
    buf = torch.zeros((W * 32,), dtype=torch.uint8, device="cuda")
    g.horizon_device(buf.data_ptr())
    with pytest.raises(topo.TopoError) as e:
        g.horizon()
    assert e.value.code == topo.TOPO_ERR_CAPACITY
    g.join()      # reported once, by the horizon read
    assert (buf.cpu().numpy().view(topo.HORIZON_DTYPE)["row"] == topo.HORIZON_INCOMPLETE).all()
    with pytest.raises(topo.TopoError) as e:
        g.horizon()      # still the latest submission: still incomplete
    assert e.value.code == topo.TOPO_ERR_CAPACITY
    g.join()
    # topo_render grows the queue and renders again: the latest submission is the complete frame
    frame = g.render()
    assert g.counters()["rare_items"] > 2
    assert_view(g.horizon()[0], want[0], "grow-and-retry", frame[1])
    g.join()


def test_tile_lifecycle(topo, orc):
    sc = Scene(64, 2, 2, eye_dh=150.0)
    W, H = 256, 128
    g, o = pair(topo, orc, sc, W, H)
    pu = topo.post_uniforms(W, H)
    with pytest.raises(topo.TopoError) as e:
        g.horizon()      # nothing rendered yet
    assert e.value.code == topo.TOPO_ERR_INVALID
    u = sc.uniforms(W, H, 30, 12, 80, 0)
    g.update(W, H, u, pu)
    frame = g.render()
    assert_view(g.horizon()[0], _expect(o, W, H, [u], pu, sc.locs, 64)[0], "before", frame[1])
    order = geo_order(sc.locs)
    replaced, gone = order[1], order[0]
    hts = sc.heights[replaced] * np.float32(0.7) + np.float32(30.0)
    g.add_terrain(replaced[0], replaced[1], hts, *sc.transform(replaced))
    o.add_terrain(replaced[0], replaced[1], hts, *sc.transform(replaced))
    for call in (lambda: g.horizon(), lambda: _device_horizon(g, 1, W)):
        with pytest.raises(topo.TopoError) as e:
            call()
        assert e.value.code == topo.TOPO_ERR_INVALID
    frame = g.render()
    assert_view(g.horizon()[0], _expect(o, W, H, [u], pu, sc.locs, 64)[0], "after replacing a tile", frame[1])
    g.unload_terrain(*gone)
    o.unload_terrain(*gone)
    with pytest.raises(topo.TopoError) as e:
        g.horizon()
    assert e.value.code == topo.TOPO_ERR_INVALID
    left = [l for l in sc.locs if l != gone]
    for yaw in (30, 200):
        u = sc.uniforms(W, H, yaw, 12, 80, 0)
        g.update(W, H, u, pu)
        frame = g.render()
        assert_view(g.horizon()[0], _expect(o, W, H, [u], pu, left, 64)[0], f"after unloading a tile (ranks shifted), yaw {yaw}", frame[1])


def test_queries_change_no_frame(topo):
    import torch
    sc = Scene(96, 2, 2, eye_dh=100.0)
    W, H = 256, 160
    a, b = topo.TerrainRenderer(W, H), topo.TerrainRenderer(W, H)
    sc.load(a)
    sc.load(b)
    pu = topo.post_uniforms(W, H)
    buf = torch.zeros((W * 32,), dtype=torch.uint8, device="cuda")
    for yaw, pitch, fov in ((40, 10, 70), (120, 60, 90), (300, 2, 50), (10, 85, 100)):
        u = sc.uniforms(W, H, yaw, pitch, fov, 0)
        a.update(W, H, u, pu)
        b.update(W, H, u, pu)
        ra, rb = a.render(), b.render()
        assert_same_frame(ra, rb, f"queries vs none, yaw {yaw}")
        assert a.counters() == b.counters() and a.frame_status() == b.frame_status()
        b.horizon()
        b.horizon_device(buf.data_ptr())
        b.horizon()
    # frames in flight, queried between submissions
    a.set_pipeline_depth(2)
    b.set_pipeline_depth(2)
    keep = []
    for k in range(4):
        us = sc.panorama(64, 96, yaw0_deg=9.0 * k)
        keep.append((strip(a, us, 64, 96), strip(b, us, 64, 96)))
        if k % 2:
            b.horizon()
        else:
            b.horizon_device(buf.data_ptr(), 0, 1)
    a.join()
    b.join()
    for (ra, da), (rb, db) in keep:
        assert torch.equal(ra, rb) and torch.equal(da, db)
    torch.cuda.synchronize()


def test_full_size_tiles(topo, orc):
    """1200 x 1200 tiles, a 2 x 2 mosaic, the panorama of 8 x 1024 x 512: cells past 2^20."""
    import torch
    sc = Scene(1200, 2, 2, eye_dh=300.0)
    sw, sh = 1024, 512
    g, o = pair(topo, orc, sc, sw, sh)
    pu = topo.post_uniforms(sw, sh)
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    strip = torch.zeros((8, sh, sw, 4), dtype=torch.uint8, device="cuda")
    depth = torch.zeros((8, sh, sw), dtype=torch.float32, device="cuda")
    g.render_panorama(None, sc.eye, math.radians(15.0), sw, sh, sc.vlon, sc.vlat, strip.data_ptr(), depth.data_ptr())
    got = g.horizon()
    g.synchronize()
    _assert_all(got, _expect(o, sw, sh, sc.panorama(sw, sh, yaw0_deg=15.0), pu, sc.locs, 1200), "1200 x 1200 panorama", depth.cpu().numpy())
    t = got[got["row"] >= 0]
    assert len(t) > 0 and ((t["cell_x"].astype(np.int64) * 1199 + t["cell_y"]) >= (1 << 20)).any()
    torch.cuda.synchronize()


def test_size_limits(topo, orc):
    """65536 x 256 against the oracle's winners, and the submission of 64 views of 8191 x 8191 (keys past 2^31): every view's horizon
    equals its pose's, and oracle windows of whole columns agree on row and depth (tests/test_limits_gpu.py's cases)."""
    import torch
    import limits_scenes as LS
    free, _ = torch.cuda.mem_get_info()
    if free < 90 * 2 ** 30:
        pytest.fail(f"the limit cases need about 80 GB of device memory; {free / 2 ** 30:.1f} GB free")
    sc, W, H, _, fmt, _ = LS.case_views("wide")
    r, views = LS.new_renderer(topo, "wide")
    rgba, depth = LS.render_device(r, views, W, H)
    got = r.horizon()
    o = orc.OracleRenderer(W, H, color_format=fmt)
    sc.load(o)
    _assert_all(got, _expect(o, W, H, views, topo.post_uniforms(W, H), sc.locs, sc.tile), "65536 x 256", depth.cpu().numpy())
    del rgba, depth
    r.close()
    o.close()
    torch.cuda.empty_cache()
    sc, W, H, _, fmt, _ = LS.case_views("views_4g")
    r, views = LS.new_renderer(topo, "views_4g")
    rgba, depth = LS.render_device(r, views, W, H, want_depth=True)
    del rgba
    got = r.horizon()
    assert got.shape == (64, W) and (got["row"] >= 0).any()
    for v in range(4, 64):
        assert np.array_equal(got[v], got[v % 4]), f"view {v} differs from pose {v % 4}"
    dev = _device_horizon(r, 4, W, first=60)
    assert np.array_equal(dev, got[60:64])
    for v in (0, 1, 2, 3, 63):
        for x0 in (0, 4096, W - 64):
            o = orc.OracleRenderer(W, H, color_format=fmt)
            sc.load(o)
            o.update(W, H, views[v], topo.post_uniforms(W, H))
            _, od = o.render_window(x0, 0, 64, H)
            o.close()
            rec = got[v][x0:x0 + 64]
            terrain = od < 1.0
            has = terrain.any(axis=0)
            want_row = np.where(has, terrain.argmax(axis=0), -1)
            assert np.array_equal(rec["row"], want_row), f"view {v} columns {x0}.."
            want_d = np.where(has, od[np.clip(want_row, 0, None), np.arange(64)], np.float32(1.0)).astype(np.float32)
            assert np.array_equal(rec["depth"].view(np.uint32), want_d.view(np.uint32)), f"view {v} columns {x0}.. depth"
            fd = depth[v, :, x0:x0 + 64].cpu().numpy()
            assert np.array_equal(fd, od), f"view {v} columns {x0}.. frame depth"
    del depth
    r.close()
    torch.cuda.empty_cache()


def _checked_run(T):
    """Horizon queries of the kinds above (single frames, odd width, panorama, views in flight, a replaced tile) -> hashes, status."""
    import torch
    h = hashlib.sha256()
    status = 0
    sc = Scene(12, 2, 2, eye_dh=60.0)
    W, H = 333, 240
    g = T.TerrainRenderer(W, H)
    sc.load(g)
    pu = T.post_uniforms(W, H)
    for yaw, pitch in ((10, 35), (200, 80), (100, -20)):
        g.update(W, H, sc.uniforms(W, H, yaw, pitch, 110, 0), pu)
        g.render()
        h.update(g.horizon().tobytes())
        status |= g.frame_status()["status"]
    sc2 = Scene(96, 2, 2, eye_dh=120.0)
    sw, sh = 70, 96
    p = T.TerrainRenderer(sw, sh)
    sc2.load(p)
    p.set_stream(torch.cuda.current_stream().cuda_stream)
    p.set_pipeline_depth(2)
    keep = strip(p, sc2.panorama(sw, sh, yaw0_deg=3.0), sw, sh)
    h.update(p.horizon(1, 6).tobytes())
    h.update(_device_horizon(p, 8, sw).tobytes())
    p.unload_terrain(*geo_order(sc2.locs)[0])
    keep = (keep, strip(p, sc2.panorama(sw, sh, yaw0_deg=30.0), sw, sh))
    h.update(p.horizon().tobytes())
    p.synchronize()
    status |= p.frame_status()["status"]
    torch.cuda.synchronize()
    return {"sha": h.hexdigest()[:24], "status": status}


def test_bounds_checked_build_records_no_out_of_range_index(topo):
    got = checked_run("test_horizon_gpu")      # kStatusBounds: an index k_horizon (or any kernel) formed was out of range
    want = _checked_run(topo)
    assert got["sha"] == want["sha"] and got["status"] == want["status"]
