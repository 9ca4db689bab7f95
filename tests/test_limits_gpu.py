"""Frames at the size limits the host accepts, on the device, against the oracle bit for bit (DESIGN.md "Size limits").

Targets of 65536 px a side, one view past 2^31 px, a submission just under 2^32 px: regions wider than 256 columns, a giant
whose 65792 regions take k_raster_rare's dividing split, FarItem boxes near x = 65535, view offsets and pixel indices past 2^31.
Frames too large for the whole oracle are compared through oracle windows (OracleRenderer.render_window).  Every case first
runs in the bounds-checked build in a child process; the product cases run only if that is clean."""
import numpy as np
import pytest

import limits_scenes as LS
from gpu_support import checked_script
from scenes import Scene, assert_same_frame

pytestmark = pytest.mark.gpu

_PEAK = {"device_used": 0}


def _note_memory():
    import torch
    free, total = torch.cuda.mem_get_info()
    _PEAK["device_used"] = max(_PEAK["device_used"], total - free)


@pytest.fixture(scope="module")
def checked(topo):
    """Every case through the bounds-checked build in a child process: no out-of-range index, no queue overflow.  Fails (never
    skips) the product cases below when it is not clean."""
    import torch
    free, total = torch.cuda.mem_get_info()
    if free < 90 * 2 ** 30:
        pytest.fail(f"the limit cases need about 80 GB of device memory; {free / 2 ** 30:.1f} GB free")
    got = checked_script("limits_scenes.py", 600)      # (a child that does not exit cleanly fails the fixture)
    assert set(got["cases"]) == set(LS.CASES)
    bad = {k: c for k, c in got["cases"].items() if c["bounds_violation"] or c["status"]}
    if bad:
        pytest.fail(f"bounds-checked limit run not clean: {bad}")
    return got


def _render(topo, name):
    _, W, H, views, fmt, split = LS.case_views(name)
    r, views = LS.new_renderer(topo, name)
    rgba, depth = LS.render_device(r, views, W, H)
    _note_memory()
    st = r.frame_status()
    assert st["status"] & 3 == 0, f"{name}: queue overflow {st}"
    assert bool((depth[0] < 1).any()), f"{name}: no terrain in the frame"
    return r, views, rgba, depth


def _oracle(orc, name, u):
    sc, W, H, _, fmt, _ = LS.case_views(name)
    o = orc.OracleRenderer(W, H, color_format=fmt)
    sc.load(o)
    import topo_renderer_amd as T
    o.update(W, H, u, T.post_uniforms(W, H))
    return o


def _window(rgba, depth, v, x0, y0, w, h):
    return rgba[v, y0:y0 + h, x0:x0 + w].cpu().numpy(), depth[v, y0:y0 + h, x0:x0 + w].cpu().numpy()


def _free(*objs):
    import torch
    for o in objs:
        if hasattr(o, "close"):
            o.close()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("name", ["wide", "tall", "column", "row", "mosaic_wide"])
def test_extreme_shape_matches_oracle(topo, orc, checked, name):
    """65536 x 256, 256 x 65536, 1 x 65536, 65536 x 1 and a mosaic under the occlusion split on 65536 x 256: the whole frame."""
    r, views, rgba, depth = _render(topo, name)
    if name == "mosaic_wide":      # far blocks tested against the occluders, their FarItem boxes reaching x = 65535
        assert r.debug_far_phase_launched() and r.counters()["far_tested"] > 0
    got = (rgba[0].cpu().numpy(), depth[0].cpu().numpy())
    del rgba, depth
    o = _oracle(orc, name, views[0])
    assert_same_frame(got, o.render(), name)
    _free(r, o)


def test_giant_over_65536_regions_matches_oracle(topo, orc, checked):
    """16384 x 16448: 256 region columns, 257 rows; one near-plane giant covers all 65792 regions, so k_raster_rare's
    cooperative split divides (n >= 65536) instead of multiply-shifting."""
    sc, W, H, views, _, _ = LS.case_views("giant")
    assert LS.largest_triangle_regions(sc, views[0], W, H) >= 65536
    r, views, rgba, depth = _render(topo, "giant")
    o = _oracle(orc, "giant", views[0])
    rng = np.random.default_rng(5)
    wins = [(0, H - 64, W, 64), (0, 0, W, 3), (W - 64, 0, 64, H), (0, 0, 64, H)]
    wins += [(int(rng.integers(0, W - 256)), int(rng.integers(0, H - 256)), 256, 256) for _ in range(16)]
    for x0, y0, w, h in wins:
        assert_same_frame(_window(rgba, depth, 0, x0, y0, w, h), o.render_window(x0, y0, w, h), f"giant window ({x0},{y0}) {w}x{h}")
    del rgba, depth
    _free(r, o)


def test_view_past_2_31_pixels_matches_oracle(topo, orc, checked):
    """65536 x 32800 = 2^31 + 2^22 px in one view: pixel indices cross 2^31 at row 32768."""
    _, W, H, _, _, _ = LS.case_views("view_2g")
    r, views, rgba, depth = _render(topo, "view_2g")
    o = _oracle(orc, "view_2g", views[0])
    rng = np.random.default_rng(31)
    wins = [(0, 32766, W, 4), (0, 0, W, 3), (0, H - 3, W, 3), (W - 64, 0, 64, H)]
    wins += [(int(rng.integers(0, W - 256)), int(rng.integers(0, H - 64)), 256, 64) for _ in range(16)]
    for x0, y0, w, h in wins:
        assert_same_frame(_window(rgba, depth, 0, x0, y0, w, h), o.render_window(x0, y0, w, h), f"view_2g window ({x0},{y0}) {w}x{h}")
    del rgba, depth
    _free(r, o)


def test_submission_just_under_2_32_pixels(topo, orc, checked):
    """64 views of 8191 x 8191 (4 293 918 784 px), cycling 4 poses: every view equals its pose rendered alone, oracle windows
    around view 32's global key 2^31 and in the last rows of view 63 agree, the viewshed equals the single renders'; one
    pixel more per view (64 x 8192 x 8192 = 2^32) is refused, and the context still renders afterwards."""
    import torch
    import topo_renderer_amd as T
    sc, W, H, _, _, _ = LS.case_views("views_4g")
    r, views = LS.new_renderer(topo, "views_4g")
    r.viewshed_enable(True)
    rgba, depth = LS.render_device(r, views, W, H)
    _note_memory()
    assert r.frame_status()["status"] & 3 == 0
    assert all(bool((depth[v] < 1).any()) for v in range(4)), "a pose without terrain"
    masks = {loc: r.viewshed(*loc) for loc in sc.locs}
    assert sum(int(m.sum()) for m in masks.values()) > 0
    # windows against the oracle: view 0, view 32 around global key 2^31 (row 64, column 32), view 63's last rows
    assert 32 * W * H + 64 * W + 32 == 2 ** 31
    for v, (x0, y0, w, h) in ((0, (0, 0, 512, 64)), (0, (W - 300, H - 40, 300, 40)), (32, (0, 60, W, 8)), (63, (0, H - 3, W, 3))):
        o = _oracle(orc, "views_4g", views[v])
        assert_same_frame(_window(rgba, depth, v, x0, y0, w, h), o.render_window(x0, y0, w, h), f"views_4g view {v} window ({x0},{y0})")
        o.close()
    # each pose alone, on the same context, equals every view of the submission that carries it
    r.viewshed_reset()
    for p in range(4):
        one, one_d = LS.render_device(r, views[p:p + 1], W, H)
        for v in range(p, 64, 4):
            assert torch.equal(rgba[v], one[0]) and torch.equal(depth[v], one_d[0]), f"view {v} differs from pose {p} alone"
        del one, one_d
    for loc in sc.locs:
        assert np.array_equal(r.viewshed(*loc), masks[loc]), f"viewshed of {loc}"
    # 2^32 px: refused on the host before anything is queued; the next frame is whole
    with pytest.raises(T.TopoError) as e:
        r.render_views_device(views, 8192, 8192, rgba.data_ptr(), 8192 * 8192 * 4, 8192 * 4)
    assert e.value.code == T.TOPO_ERR_CAPACITY
    del rgba, depth
    torch.cuda.empty_cache()
    small = Scene(24, 1, 1)
    r2 = topo.TerrainRenderer(96, 64)
    small.load(r2)
    r.close()
    u = small.uniforms(96, 64, 40, 10, 70)
    r2.update(96, 64, u, T.post_uniforms(96, 64))
    o = orc.OracleRenderer(96, 64)
    small.load(o)
    o.update(96, 64, u, T.post_uniforms(96, 64))
    assert_same_frame(r2.render(), o.render(), "small frame after the refused submission")
    _free(r2, o)
    print(f"limit tests: peak device memory in use {_PEAK['device_used'] / 2 ** 30:.1f} GB")


def test_slot_path_refuses_oversized_sector(topo, monkeypatch):
    """The slot-by-slot panorama path (TOPO_PANORAMA_FORCE_SLOTS at world 1) checks the target size as render_views_device
    does: a 65537 px wide sector would truncate the 16-bit footprints."""
    import torch
    import topo_renderer_amd as T
    sc = Scene(24, 1, 1)
    r = topo.TerrainRenderer(64, 8)
    sc.load(r)
    strip = torch.zeros((8, 8, 65537, 4), dtype=torch.uint8, device="cuda")
    monkeypatch.setenv("TOPO_PANORAMA_FORCE_SLOTS", "1")
    for sw, sh in ((65537, 8), (8, 65537)):
        with pytest.raises(T.TopoError) as e:
            r.render_panorama(None, sc.eye, 0.0, sw, sh, sc.vlon, sc.vlat, strip.data_ptr())
        assert e.value.code == T.TOPO_ERR_INVALID, (sw, sh)
    r.close()
