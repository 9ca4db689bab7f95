"""The cull's host-side tile prefilter on the GPU: the cull launched over the kept (view, tile) pairs alone gives the frames and the
counters of the full grid, and a submission with no pair left still clears its visibility buffer."""
import math

import numpy as np
import pytest

from scenes import Scene, assert_same_frame

pytestmark = pytest.mark.gpu


def test_prefilter_launches_fewer_pairs_same_frame_and_counters(topo, orc):
    # 3 x 3 mosaic of 64-px tiles, the eye in the middle tile, a 20-degree field of view: most tiles lie beside or behind the frustum
    sc = Scene(64, 3, 3)
    W, H = 128, 64
    g, o = topo.TerrainRenderer(W, H), orc.OracleRenderer(W, H)
    sc.load(g)
    sc.load(o)
    pu = topo.post_uniforms(W, H)
    for yaw in (0, 45, 180, 270):
        u = sc.uniforms(W, H, yaw, -2.0, 20.0, 0)
        g.update(W, H, u, pu)
        o.update(W, H, u, pu)
        ref = o.render()
        g.debug_set_tile_prefilter(True)
        on = g.render()
        launched, pairs = g.debug_cull_pairs()
        c_on = g.counters()
        g.debug_set_tile_prefilter(False)
        off = g.render()
        assert g.debug_cull_pairs() == (9, 9)
        c_off = g.counters()
        print(f"yaw {yaw}: pairs launched {launched} of {pairs}; counters {c_on}")
        assert pairs == 9 and 0 < launched < pairs, (yaw, launched, pairs)
        assert_same_frame(on, ref, f"prefilter on, yaw {yaw}")
        assert_same_frame(off, ref, f"prefilter off, yaw {yaw}")
        assert c_on == c_off, (yaw, c_on, c_off)
        st = g.frame_status()
        assert c_on["blocks_rastered"] > 0 and not st["bounds_violation"] and not st["rare_overflow"], st


def test_no_pair_left_still_clears(topo, orc):
    # the eye a degree west of the mosaic, 3 km up: looking east the whole mosaic is in view, looking west none of it
    locs = topo.synth.mosaic_locations(45, 15, 3, 3)
    W, H, tile = 128, 64, 64
    g, o = topo.TerrainRenderer(W, H), orc.OracleRenderer(W, H)
    for r in (g, o):
        for la, lo in locs:
            r.add_terrain(la, lo, topo.synth_tile(la, lo, tile, tile), *topo.synth.tile_transform(la, lo, tile, tile))
    vlon, vlat = 14.0, 46.5
    eye = topo.geometry_transform(3000.0, vlon, vlat)
    pu = topo.post_uniforms(W, H)
    view = lambda yaw: topo.camera_uniforms(eye, math.radians(yaw), 0.0, math.radians(20.0), W, H, vlon, vlat, 0)
    frames = {}
    for step, yaw in enumerate((90, 270, 90)):      # at the mosaic (marks the buffer), away from it, back at it
        u = view(yaw)
        g.update(W, H, u, pu)
        rgba, depth = g.render()
        launched, pairs = g.debug_cull_pairs()
        print(f"step {step} yaw {yaw}: pairs launched {launched} of {pairs}; terrain pixels {int((depth < 1).sum())}")
        if yaw not in frames:
            o.update(W, H, u, pu)
            frames[yaw] = o.render()
        assert_same_frame((rgba, depth), frames[yaw], f"step {step} yaw {yaw}")
        if yaw == 270:
            assert (launched, pairs) == (0, 9)
            assert (depth == 1.0).all(), "a frame with nothing to cull must be all sky"
            assert g.counters()["blocks_rastered"] == 0
        else:
            assert launched > 0 and (depth < 1).any()
        st = g.frame_status()
        assert not st["bounds_violation"] and not st["rare_overflow"], st
