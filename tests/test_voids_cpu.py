"""Void and non-finite DEM heights without a GPU (tests/void_scenes.py): the product's pipeline headers (tests/emul.py) against the
oracle on tiles with holes in them, a directed sweep across the guard band of a primitive cut by the near plane, and the
oracle's own void semantics -- a triangle with a void vertex does not exist, its neighbours do -- against the independent f64
ray caster.  (The expected-mask and expected-horizon helpers are already checked on arbitrary winners by
test_viewshed_cpu.py and test_horizon_cpu.py; nothing about them depends on the heights.)"""
import math

import numpy as np
import pytest

import emul
import void_scenes as VS
from limits_scenes import _clip_coords
from oracle import ray_check as RC
from scenes import Scene, assert_same_frame

NO_TRI = 0xFFFFFFFF


def _emul_equals_oracle(topo, orc, key, sc, void, W, H, pose, close_up=False):
    """Normals byte for byte, then the frame; the oracle's frame first has to show the void (assert_void_in_view, or the
    close-ups' own condition)."""
    pu = topo.post_uniforms(W, H)
    ref, clean = VS.oracle_frames(orc, key, sc, void, W, H, pose, pu)
    if close_up:
        VS.assert_cut_void_in_view(sc, void, sc.uniforms(W, H, *pose), ref[1], clean[1], str(key))
    else:
        VS.assert_void_in_view(ref[1], clean[1], str(key))
    e, o = emul.EmulRenderer(W, H, topo.terrain_uniforms), orc.OracleRenderer(W, H)
    void.load(e)
    void.load(o)
    for loc in void.locs:
        a, b = e.read_normals(*loc), o.read_normals(loc[0], loc[1], void.tile, void.tile)
        assert np.array_equal(a, b), f"{key} normals of tile {loc}: {np.argwhere((a != b).any(axis=-1))[:4]}"
    e.update(W, H, sc.uniforms(W, H, *pose), pu)
    assert_same_frame(e.render(), ref, f"emul {key}")


@pytest.mark.parametrize("value", list(VS.VALUES))
@pytest.mark.parametrize("name", list(VS.RELIEF))
def test_header_pipeline_matches_oracle_on_void_tiles(topo, orc, name, value):
    _emul_equals_oracle(topo, orc, (name, value), *VS.relief_case(name, value))


@pytest.mark.parametrize("value", VS.NORMALS_VALUES)
def test_header_pipeline_matches_oracle_with_a_whole_tile_void(topo, orc, value):
    _emul_equals_oracle(topo, orc, ("ne_2x2", value, "whole"), *VS.relief_case("ne_2x2", value, whole_tile=True))


@pytest.mark.parametrize("seed", VS.CLOSE_SEEDS)
@pytest.mark.parametrize("value", VS.CLOSE_VALUES)
@pytest.mark.parametrize("name", list(VS.CLOSE))
def test_header_pipeline_matches_oracle_on_cut_primitives_beside_voids(topo, orc, name, value, seed):
    """Steep close-ups: the triangles under the eye are cut by the near plane, and a void among their vertices puts a vertex of
    the clipped polygon beyond the guard band.  close_1x1 / m1e10 / seed 1 is the frame on which resolve_vertices<false>, which
    tested only the three vertices of the requested fan piece, drew the other piece of a discarded quad: 12 depth and 14 colour
    pixels differed, depth 0.99634385 against sky at pixel (0, 37)."""
    _emul_equals_oracle(topo, orc, (name, value, seed), *VS.close_case(name, value, seed), close_up=True)


# dh, yaw, pitch, fov, the void vertex (i, j): the 3 x 3 tile's cells are 55 km wide, the eye sits in the last one
GUARD = [(5.0, 40.0, 60.0, 100.0, (2, 2)), (20.0, 200.0, 45.0, 100.0, (1, 1))]


@pytest.mark.parametrize("cfg", GUARD, ids=["corner_22", "centre_11"])
def test_guard_band_sweep_of_a_cut_primitive(topo, orc, cfg):
    """One corner of the cell under the eye sinks from -1e3 m to -1e12 m in decades.  Every step equals the oracle, and the sweep
    holds both outcomes (from the oracle alone): the void triangle that covers most of the frame at the shallow end is cut by the
    near plane and drawn there, and wins no pixel at the deep end, where a vertex of its clipped polygon has left the guard band."""
    dh, yaw, pitch, fov, (vi, vj) = cfg
    W = H = 64
    tris = RC.tile_triangles(3, 3)
    touching = [t for t in range(len(tris)) if any(tuple(tris[t][k]) == (vi, vj) for k in range(3))]
    pu = topo.post_uniforms(W, H)
    won = {}
    for e10 in range(3, 13):
        sc = Scene(3, 1, 1)
        h = np.full((3, 3), 1000.0, np.float32)
        h[vj, vi] = -(10.0 ** e10)
        sc.heights = {loc: h for loc in sc.locs}
        sc.eye = topo.geometry_transform(1000.0 + dh, sc.vlon, sc.vlat)
        u = sc.uniforms(W, H, yaw, pitch, fov, 0)
        r, o = emul.EmulRenderer(W, H, topo.terrain_uniforms), orc.OracleRenderer(W, H)
        sc.load(r)
        sc.load(o)
        r.update(W, H, u, pu)
        o.update(W, H, u, pu)
        assert_same_frame(r.render(), o.render(), f"void vertex ({vi}, {vj}) at -1e{e10}")
        win = o.render_winners()[1]
        won[e10] = {t: int((win == t).sum()) for t in touching}
        if e10 == 3:
            z = _clip_coords(sc, sc.locs[0], u)[..., 2]
            cut = {t: 0 < sum(bool(z[j, i] >= 0) for i, j in tris[t]) < 3 for t in touching}
    print(won)
    main = max(touching, key=lambda t: won[3][t])
    assert cut[main] and won[3][main] > 0.25 * W * H, (main, cut, won[3])
    assert won[12][main] == 0, (main, won[12])


@pytest.mark.parametrize("value", VS.RAY_VALUES)
@pytest.mark.parametrize("name", list(VS.RELIEF))
def test_oracle_void_semantics_agree_with_f64_ray_cast(topo, orc, name, value):
    """The ray caster drops every triangle with a non-finite vertex (its np.isfinite(t)) and intersects the others as they are;
    thresholds as in test_ray_check_cpu.py::test_oracle_agrees_with_f64_ray_cast.  (+-3.4e38 and -1e10 overflow binary32 after the
    transform, which the f64 ray caster does not model: they are not part of this check.)"""
    sc, void, W, H, (yaw, pitch, fov, _) = VS.relief_case(name, value)
    pu = np.array([W, H, 100.0, 0.0], np.float32)
    frames = []
    for s in (void, sc):
        o = orc.OracleRenderer(W, H)
        s.load(o)
        o.update(W, H, sc.uniforms(W, H, yaw, pitch, fov, 1), pu)
        frames.append(o.render_winners())
    (od, ow), (cd, _) = frames
    VS.assert_void_in_view(od, cd, f"{name} {value}")
    order = sorted(void.locs, key=lambda l: (abs(l[0]), 1 if l[0] > 0 else 0, abs(l[1]), 1 if l[1] > 0 else 0))
    tiles = [(void.heights[l],) + tuple(topo.synth.tile_transform(l[0], l[1], void.tile, void.tile)) for l in order]
    with np.errstate(all="ignore"):
        rd, rw, mb, _ = RC.ray_cast(tiles, sc.eye, math.radians(yaw), math.radians(pitch), math.radians(fov), W, H)
        st = RC.compare(od, ow, rd, rw, mb)
    print(st)
    assert st["terrain_pixels_ray"] > 0.25 * W * H and st["interior_pixels"] > 0.15 * W * H, st
    assert st["interior_winner_agree"] >= 0.999, st
    assert st["interior_depth_within_tol"] >= 0.999, st
    assert st["sky_agree"] >= 0.99, st
    assert st["all_winner_agree"] >= 0.97, st
    # no triangle with a void vertex wins a pixel when the void is not a number
    if not np.isfinite(VS.VALUES[value]):
        tpt = 2 * (void.tile - 1) ** 2
        tris = RC.tile_triangles(void.tile, void.tile)
        for t in np.unique(ow[ow != NO_TRI]):
            hts = void.heights[order[int(t) // tpt]]
            assert all(np.isfinite(hts[j, i]) for i, j in tris[int(t) % tpt]), int(t)
