"""Viewshed on the GPU (topo_viewshed_*): every tile's mask equals, bit for bit, the cells of the oracle's per-pixel winners
(render_winners()) OR-ed over the same frames."""
import hashlib
import os

import numpy as np
import pytest

from gpu_support import checked_run, pair, strip
from scenes import Scene, assert_same_frame
from viewshed_ref import assert_masks, expected_masks, geo_order, mark

pytestmark = pytest.mark.gpu


def _oracle_winners(o, W, H, views, pu):
    out = []
    for u in views:
        o.update(W, H, u, pu)
        out.append(o.render_winners()[1])
    return out


FRAMES = [
    # tile, n_lat, n_lon, eye_dh, W, H, [(yaw, pitch, fov)]
    (96, 2, 2, 50.0, 256, 128, [(40, 10, 70), (250, 0, 60)]),
    (96, 2, 2, 100.0, 200, 150, [(120, 60, 90)]),                  # near clip / big triangles
    (64, 1, 1, 400.0, 160, 160, [(10, 85, 100), (300, 70, 80)]),
    (12, 2, 2, 60.0, 640, 480, [(10, 35, 110), (200, 80, 110), (100, 5, 110)]),   # the coarse mesh: every triangle large
]


@pytest.mark.parametrize("cfg", FRAMES, ids=["2x2_dh50", "2x2_dh100_p60", "1x1_dh400_p85", "coarse12"])
def test_single_frames_match_oracle_winners(topo, orc, cfg):
    tile, nla, nlo, dh, W, H, views = cfg
    sc = Scene(tile, nla, nlo, eye_dh=dh)
    g, o = pair(topo, orc, sc, W, H)
    g.viewshed_enable(True)
    pu = topo.post_uniforms(W, H)
    marked = 0
    for yaw, pitch, fov in views:
        g.viewshed_reset()
        u = sc.uniforms(W, H, yaw, pitch, fov, 0)
        g.update(W, H, u, pu)
        o.update(W, H, u, pu)
        frame = g.render()
        assert_same_frame(frame, o.render(), f"yaw {yaw} pitch {pitch}")
        want = expected_masks([o.render_winners()[1]], sc.locs, tile, tile)
        marked += sum(int(m.sum()) for m in want.values())
        assert_masks(g, want, f"{cfg[:4]} yaw {yaw} pitch {pitch}")
    assert marked > 0


def test_accumulation_over_frames_and_reset(topo, orc):
    sc = Scene(96, 2, 2, eye_dh=80.0)
    W, H = 192, 96
    g, o = pair(topo, orc, sc, W, H)
    pu = topo.post_uniforms(W, H)
    views = [sc.uniforms(W, H, yaw, 8, 70, 0) for yaw in (0, 90, 180, 270)]
    with pytest.raises(topo.TopoError) as e:
        topo.TerrainRenderer(W, H).viewshed(*sc.locs[0])      # no tile loaded
    assert e.value.code == topo.TOPO_ERR_NOT_FOUND
    with pytest.raises(topo.TopoError) as e:
        g.viewshed(*sc.locs[0])                       # never enabled
    assert e.value.code == topo.TOPO_ERR_INVALID
    g.viewshed_enable(True)
    for u in views:
        g.update(W, H, u, pu)
        g.render()
    want = expected_masks(_oracle_winners(o, W, H, views, pu), sc.locs, 96, 96)
    assert_masks(g, want, "four yaws")
    single = expected_masks(_oracle_winners(o, W, H, views[:1], pu), sc.locs, 96, 96)
    assert sum(int(m.sum()) for m in want.values()) > sum(int(m.sum()) for m in single.values())
    st = g.debug_viewshed_stats()
    assert st["terrain_keys"] >= st["updates"] >= st["atomics"] > 0
    # off: frames no longer mark, the masks stay
    g.viewshed_enable(False)
    g.update(W, H, sc.uniforms(W, H, 45, 30, 70, 0), pu)
    g.render()
    assert_masks(g, want, "after accumulation off")
    g.viewshed_reset()
    for loc in sc.locs:
        assert not g.viewshed(*loc).any()
    assert g.debug_viewshed_stats() == {"terrain_keys": 0, "updates": 0, "atomics": 0}
    with pytest.raises(topo.TopoError) as e:
        g.viewshed(3, 3)
    assert e.value.code == topo.TOPO_ERR_NOT_FOUND


def test_panorama_submission_and_pipelined_burst(topo, orc):
    import torch
    sc = Scene(96, 2, 2, eye_dh=120.0)
    sw, sh = 96, 128
    g, o = pair(topo, orc, sc, sw, sh)
    pu = topo.post_uniforms(sw, sh)
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    g.viewshed_enable(True)
    us = sc.panorama(sw, sh, yaw0_deg=11.0)
    keep = strip(g, us, sw, sh)
    g.synchronize()
    want = expected_masks(_oracle_winners(o, sw, sh, us, pu), sc.locs, 96, 96)
    assert_masks(g, want, "8-sector submission")
    # frames in flight on two contexts, several submissions
    g.viewshed_reset()
    g.set_pipeline_depth(2)
    views = []
    for k in range(5):
        us = sc.panorama(sw, sh, yaw0_deg=7.0 * k)
        keep = (keep, strip(g, us, sw, sh))
        views += list(us)
    g.join()
    want = expected_masks(_oracle_winners(o, sw, sh, views, pu), sc.locs, 96, 96)
    assert_masks(g, want, "pipeline depth 2 burst")
    torch.cuda.synchronize()


def test_panorama_slot_path_and_batch(topo, orc):
    """topo_render_panorama (world of one, and its slot-by-slot resolve: k_viewshed behind the last slot) and topo_render_batch
    (several viewpoints, two submissions in flight) accumulate like any other frame."""
    import math
    import torch
    sc = Scene(96, 2, 2, eye_dh=120.0)
    sw, sh = 96, 160
    g, o = pair(topo, orc, sc, sw, sh)
    pu = topo.post_uniforms(sw, sh)
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    g.viewshed_enable(True)
    strip = torch.zeros((8, sh, sw, 4), dtype=torch.uint8, device="cuda")
    depth = torch.zeros((8, sh, sw), dtype=torch.float32, device="cuda")
    want = expected_masks(_oracle_winners(o, sw, sh, sc.panorama(sw, sh, yaw0_deg=25.0), pu), sc.locs, 96, 96)
    g.render_panorama(None, sc.eye, math.radians(25.0), sw, sh, sc.vlon, sc.vlat, strip.data_ptr(), depth.data_ptr())
    g.synchronize()
    assert_masks(g, want, "panorama, world of one")
    os.environ["TOPO_PANORAMA_FORCE_SLOTS"] = "1"
    os.environ["TOPO_PANORAMA_BAND_BYTES"] = str(sw * 4 * 50)
    try:
        assert len(topo.panorama_slots(2, sw, sh)) == 4 * 3       # several slots per sector: the launch must follow the last one
        for yaw0 in (25.0, 70.0):
            g.viewshed_reset()
            want = expected_masks(_oracle_winners(o, sw, sh, sc.panorama(sw, sh, yaw0_deg=yaw0), pu), sc.locs, 96, 96)
            g.render_panorama(topo.Comm(0, 1), sc.eye, math.radians(yaw0), sw, sh, sc.vlon, sc.vlat, strip.data_ptr(), depth.data_ptr())
            g.synchronize()
            assert_masks(g, want, f"slot-by-slot panorama yaw0 {yaw0}")
    finally:
        del os.environ["TOPO_PANORAMA_FORCE_SLOTS"], os.environ["TOPO_PANORAMA_BAND_BYTES"]
    rng = np.random.default_rng(4)
    eyes, yaws, suns = [], [], []
    for _ in range(3):
        lat, lon = 45.1 + 1.8 * rng.random(), 15.1 + 1.8 * rng.random()
        key = (int(math.floor(lat)), int(math.floor(lon)))
        ground = topo.synth.height_at(sc.heights[key], key[0], key[1], lon, lat)
        eyes.append(topo.geometry_transform(ground + 80.0, lon, lat)); yaws.append(2 * math.pi * rng.random()); suns.append((lon, lat))
    g.viewshed_reset()
    out = torch.zeros((3, 8, sh, sw, 4), dtype=torch.uint8, device="cuda")
    dout = torch.zeros((3, 8, sh, sw), dtype=torch.float32, device="cuda")
    g.set_pipeline_depth(2)
    g.render_batch(eyes, yaws, suns, sw, sh, out.data_ptr(), dout.data_ptr())
    g.join()
    views = []
    for v in range(3):
        views += list(topo.panorama_uniforms(eyes[v], yaws[v], sw, sh, suns[v][0], suns[v][1], 0))
    want = expected_masks(_oracle_winners(o, sw, sh, views, pu), sc.locs, 96, 96)
    assert sum(int(m.sum()) for m in want.values()) > 0
    assert_masks(g, want, "batch of three viewpoints")
    torch.cuda.synchronize()


def test_tile_lifecycle_replace_and_unload(topo, orc):
    sc = Scene(64, 2, 2, eye_dh=150.0)
    W, H = 256, 128
    g, o = pair(topo, orc, sc, W, H)
    pu = topo.post_uniforms(W, H)
    g.viewshed_enable(True)
    va = [sc.uniforms(W, H, yaw, 12, 80, 0) for yaw in (30, 150, 260)]
    for u in va:
        g.update(W, H, u, pu)
        g.render()
    masks = expected_masks(_oracle_winners(o, W, H, va, pu), sc.locs, 64, 64)
    assert_masks(g, masks, "before")
    order = geo_order(sc.locs)
    replaced, gone = order[1], order[0]          # unloading rank 0 shifts every other rank
    assert masks[replaced].any() and masks[gone].any()
    hts = sc.heights[replaced] * np.float32(0.7) + np.float32(30.0)
    g.add_terrain(replaced[0], replaced[1], hts, *sc.transform(replaced))
    o.add_terrain(replaced[0], replaced[1], hts, *sc.transform(replaced))
    assert not g.viewshed(*replaced).any()
    masks[replaced][:] = False
    assert_masks(g, masks, "after replacing a tile")
    g.unload_terrain(*gone)
    o.unload_terrain(*gone)
    with pytest.raises(topo.TopoError) as e:
        g.viewshed(*gone)
    assert e.value.code == topo.TOPO_ERR_NOT_FOUND
    left = [l for l in sc.locs if l != gone]
    masks.pop(gone)
    vb = [sc.uniforms(W, H, yaw, 12, 80, 0) for yaw in (60, 200)]
    for u in vb:
        g.update(W, H, u, pu)
        g.render()
    for w in _oracle_winners(o, W, H, vb, pu):
        mark(masks, w, left, 64, 64)
    assert_masks(g, masks, "after unloading a tile (ranks shifted)")


def test_queue_overflow_frames_mark_only_when_complete(topo, orc):
    sc = Scene(12, 2, 2, eye_dh=60.0)
    W, H = 640, 480
    g, o = pair(topo, orc, sc, W, H)
    u, pu = sc.uniforms(W, H, 10, 35, 110, 0), topo.post_uniforms(W, H)
    g.update(W, H, u, pu)
    o.update(W, H, u, pu)
    want = expected_masks([o.render_winners()[1]], sc.locs, 12, 12)
    g.viewshed_enable(True)
    # topo_render's grow-and-retry: the overflowed attempts mark nothing, the complete re-render marks exactly the oracle's cells
    g.debug_set_queue_caps(0, 2 | 0x80000000)
    assert_same_frame(g.render(), o.render(), "rare queue grown on demand")
    assert g.counters()["rare_items"] > 2
    assert_masks(g, want, "grow-and-retry")
    # an explicit small rare cap on the asynchronous path: the frame is incomplete, join() says so, the masks are untouched
    import torch
    g.viewshed_reset()
    g.debug_set_queue_caps(0, 2)
    rgba = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    g.render_device(rgba.data_ptr(), W * 4)
    with pytest.raises(topo.TopoError) as e:
        g.join()
    assert e.value.code == topo.TOPO_ERR_CAPACITY
    for loc in sc.locs:
        assert not g.viewshed(*loc).any(), loc
    g.debug_set_queue_caps(0, 0)
    g.render_device(rgba.data_ptr(), W * 4)
    g.join()
    assert_masks(g, want, "defaults restored")


def test_accumulation_changes_no_output(topo):
    sc = Scene(96, 2, 2, eye_dh=100.0)
    W, H = 256, 160
    a, b = topo.TerrainRenderer(W, H), topo.TerrainRenderer(W, H)
    sc.load(a)
    sc.load(b)
    b.viewshed_enable(True)
    pu = topo.post_uniforms(W, H)
    for yaw, pitch, fov in ((40, 10, 70), (120, 60, 90), (300, 2, 50)):
        u = sc.uniforms(W, H, yaw, pitch, fov, 0)
        a.update(W, H, u, pu)
        b.update(W, H, u, pu)
        ra, rb = a.render(), b.render()
        assert_same_frame(ra, rb, f"accumulation on vs off, yaw {yaw}")
        assert a.counters() == b.counters()
        assert a.frame_status() == b.frame_status()
    assert any(b.viewshed(*loc).any() for loc in sc.locs)


def test_full_size_tiles(topo, orc):
    """1200 x 1200 tiles: 1.44 M cells, so bit indices run past 2^20."""
    sc = Scene(1200, 1, 1, eye_dh=300.0)
    W, H = 256, 96
    g, o = pair(topo, orc, sc, W, H)
    g.viewshed_enable(True)
    pu = topo.post_uniforms(W, H)
    views = [sc.uniforms(W, H, yaw, 3, 70, 0) for yaw in (0, 120, 240)]
    for u in views:
        g.update(W, H, u, pu)
        g.render()
    want = expected_masks(_oracle_winners(o, W, H, views, pu), sc.locs, 1200, 1200)
    assert_masks(g, want, "1200 x 1200 tiles")
    high = 0
    for m in want.values():
        y, x = np.nonzero(m)
        high += int(((x.astype(np.int64) * 1199 + y) >= (1 << 20)).sum())
    assert high > 0


def _checked_run(T):
    """A few viewshed frames (coarse mesh, panorama submission, lifecycle) -> {mask hashes, frame status}."""
    import torch
    out = {}
    sc = Scene(12, 2, 2, eye_dh=60.0)
    W, H = 320, 240
    g = T.TerrainRenderer(W, H)
    sc.load(g)
    g.viewshed_enable(True)
    pu = T.post_uniforms(W, H)
    status = 0
    for yaw, pitch in ((10, 35), (200, 80)):
        g.update(W, H, sc.uniforms(W, H, yaw, pitch, 110, 0), pu)
        g.render()
        status |= g.frame_status()["status"]
    sc2 = Scene(96, 2, 2, eye_dh=120.0)
    sw, sh = 64, 96
    p = T.TerrainRenderer(sw, sh)
    sc2.load(p)
    p.viewshed_enable(True)
    p.set_stream(torch.cuda.current_stream().cuda_stream)
    keep = strip(p, sc2.panorama(sw, sh, yaw0_deg=3.0), sw, sh)
    p.synchronize()
    p.unload_terrain(*geo_order(sc2.locs)[0])
    keep = (keep, strip(p, sc2.panorama(sw, sh, yaw0_deg=30.0), sw, sh))
    p.synchronize()
    status |= p.frame_status()["status"]
    h = hashlib.sha256()
    for r, s in ((g, sc), (p, sc2)):
        for loc in s.locs:
            if r is p and loc == geo_order(sc2.locs)[0]:
                continue
            h.update(np.packbits(r.viewshed(*loc)).tobytes())
    out["sha"] = h.hexdigest()[:24]
    out["status"] = status
    torch.cuda.synchronize()
    return out


def test_bounds_checked_build_marks_no_out_of_range_index(topo):
    got = checked_run("test_viewshed_gpu")      # kStatusBounds: an index k_viewshed (or any kernel) formed was out of range
    want = _checked_run(topo)
    assert got["sha"] == want["sha"] and got["status"] == want["status"]
