"""The host query layer (csrc/terrain_queries.cpp): the tile-set tables are built lazily, by whichever query needs them first and only
as far as it needs them, and a device variant queued on a frame context's own stream keeps that context's next frame behind it.
Neither may show in what a query answers: every kind in every order gives the same bytes, and a query in flight at pipeline depth 2
the same as at depth 1."""
import numpy as np
import pytest

import los_cases as LC
from gpu_support import padded_device_output, strip
from scenes import Scene, relief

pytestmark = pytest.mark.gpu

W, H = 96, 64
KINDS = ("horizon", "ground", "ground_map", "sunlit", "raycast")      # the baseline's order
BOUND = KINDS[:4]                                                      # ... of which these need a submission
_MEMO = {}


def _scene():
    """tests/test_raycast_gpu.py::test_consistent_with_the_ground_queries' scene: four 24 x 24 tiles, every query kind has terrain."""
    if "scene" not in _MEMO:
        sc = Scene(24, 2, 2, lat0=45, lon0=15, eye_dh=4000.0, height_fn=relief)
        ys, xs = np.mgrid[0:H:7, 0:W:5]
        queries = np.stack([np.zeros(xs.size, np.int64), xs.ravel(), ys.ravel()], axis=1)
        _MEMO["scene"] = sc, sc.uniforms(W, H, 30.0, 25.0, 60.0, 1), queries, LC.eye_rays(sc, 8, 6, 30.0, 25.0, 60.0), LC.sun_of(sc)
    return _MEMO["scene"]


def _renderer(topo):
    sc, u = _scene()[:2]
    g = topo.TerrainRenderer(W, H)
    sc.load(g)
    g.update(W, H, u, topo.post_uniforms(W, H))
    g.render()
    return g


def _device(g, fill_bytes, call):
    """A device variant's output: a dense tensor of fill_bytes handed to call(pointer), read back after the renderer's streams."""
    return padded_device_output(g, 1, 1, fill_bytes, 1, lambda p, *_: call(p))[0].tobytes()


def _ask(g, kind):
    _, _, queries, rays, sun = _scene()
    if kind == "horizon":
        return g.horizon().tobytes()
    if kind == "ground":
        return g.ground(queries).tobytes()
    if kind == "ground_map":
        return _device(g, W * H * 16, lambda p: g.ground_map_device(p))
    if kind == "sunlit":
        return _device(g, W * H, lambda p: g.sunlit_map_device(sun, p))
    return g.raycast(rays).tobytes()


def _ask_all(g, first):
    return {k: _ask(g, k) for k in (first,) + tuple(k for k in KINDS if k != first)}


def _session(topo, first, first_again):
    """A renderer's life: every kind with `first` first; a tile unloaded and added back, when the rays answer at once and nothing else
    does before the next render; every kind again with `first_again` first.  (answers, the rays' in between, answers again)."""
    sc = _scene()[0]
    g = _renderer(topo)
    before = _ask_all(g, first)
    loc = sc.locs[1]
    g.unload_terrain(*loc)
    g.add_terrain(loc[0], loc[1], sc.heights[loc], *sc.transform(loc))
    between = _ask(g, "raycast")
    for k in BOUND:
        with pytest.raises(topo.TopoError) as e:
            _ask(g, k)
        assert e.value.code == topo.TOPO_ERR_INVALID, k
    g.render()
    after = _ask_all(g, first_again)
    g.close()
    return before, between, after


def _baseline(topo):
    if "baseline" not in _MEMO:
        _MEMO["baseline"] = _session(topo, KINDS[0], KINDS[0])
    return _MEMO["baseline"]


def test_the_baseline_answers_with_terrain(topo):
    """What the order tests compare is not empty: every kind sees terrain, before and after the tile set changed."""
    before, between, after = _baseline(topo)
    for got in (before, after):
        assert (np.frombuffer(got["horizon"], topo.HORIZON_DTYPE)["row"] >= 0).sum() > W // 2
        assert (np.frombuffer(got["ground"], topo.GROUND_DTYPE)["kind"] == topo.GROUND_TERRAIN).sum() > 20
        assert np.isfinite(np.frombuffer(got["ground_map"], np.float32)).sum() > W * H
        assert all((np.frombuffer(got["sunlit"], np.uint8) == c).any() for c in (topo.SUN_NONE, topo.SUN_LIT))
        assert (np.frombuffer(got["raycast"], topo.RAY_HIT_DTYPE)["kind"] == topo.RAY_HIT).sum() > 10
    assert between == before["raycast"] == after["raycast"], "the rays see the same tiles whenever they are asked"


@pytest.mark.parametrize("first", KINDS)
def test_any_kind_may_build_the_tables(topo, first):
    """A fresh renderer that asks `first` before the other kinds, and after a tile was unloaded and added back another kind first,
    answers every kind with the baseline's bytes."""
    again = KINDS[(KINDS.index(first) + 2) % len(KINDS)]
    base = _baseline(topo)
    before, between, after = _session(topo, first, again)
    for k in KINDS:
        assert before[k] == base[0][k], f"{k}, asked after {first}"
        assert after[k] == base[2][k], f"{k} after the tile set changed, asked after {again}"
    assert between == base[1], "raycast between the tile set's change and the next render"


@pytest.mark.parametrize("variant", ["horizon_device", "ground_map_device"])
def test_device_variant_in_flight_at_depth_2(topo, variant):
    """The variant queued behind a two-view frame on a context's own stream, then two frames of other views (the second reuses that
    context) before the join: what it wrote is what it writes at depth 1.  (ground_device and sunlit_map_device:
    tests/test_ground_gpu.py::test_pipeline_depth_2_device_list_before_join, tests/test_raycast_gpu.py::
    test_sunlit_sub_range_and_frames_in_flight.)"""
    import torch
    sc = _scene()[0]
    g = topo.TerrainRenderer(W, H)
    sc.load(g)
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    views = [sc.uniforms(W, H, yaw, 25.0, 60.0, 1) for yaw in (30.0, 75.0)]
    others = [sc.uniforms(W, H, yaw, 10.0, 60.0, 1) for yaw in (200.0, 290.0)]
    size = 2 * W * 32 if variant == "horizon_device" else 2 * W * H * 16
    keep = [strip(g, views, W, H)]
    want = torch.full((size,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    getattr(g, variant)(want.data_ptr())
    g.synchronize()
    want = want.cpu().numpy()
    assert (want != 0xAB).any()
    g.set_pipeline_depth(2)
    got = torch.full((size,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    keep.append(strip(g, views, W, H))
    getattr(g, variant)(got.data_ptr())
    keep += [strip(g, others, W, H), strip(g, others[::-1], W, H)]
    g.join()
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), want)
    if variant == "horizon_device":
        rows = want.view(topo.HORIZON_DTYPE)["row"]
        assert (rows >= 0).sum() > W // 2 and not (rows == topo.HORIZON_INCOMPLETE).any()
    else:
        assert np.isfinite(want.view(np.float32)).sum() > W * H
    del keep
    g.close()
