"""The queries off the 45N 15E quadrant and rays on tiles of many raster blocks, on the GPU.

The placements of tests/geo_scenes.py -- across the equator and the prime meridian, across the antimeridian, at 84N and at 86S --
through the frame, ground points, horizon, viewshed, sunlit layer and unwrap, each against the reference its own test module uses
(the oracle's frames and winners, tests/ground_ref.py, horizon_ref.py, viewshed_ref.py, los_ref.py, unwrap_ref.py) with that
module's tolerances; the occlusion filter's block bounds at those longitudes and latitudes; and k_raycast on one full-size tile,
whose 1600 raster blocks it takes in 25 batches of 64."""
import math
import time

import numpy as np
import pytest

import geo_scenes as GS
import ground_ref as GR
import los_cases as LC
import los_emul as LE
import los_ref as LR
import topo_renderer_amd as T
import unwrap_cases as UC
import unwrap_ref as UR
from gpu_support import ground_map, renderer, sunlit_map, unwrap_run
from horizon_ref import assert_view, horizon
from scenes import assert_same_frame
from viewshed_ref import assert_masks, expected_masks

pytestmark = pytest.mark.gpu

_PAIRS = {}
_WINNERS = {}
SEEN = {"origin": {(0, 0), (0, -1), (-1, 0), (-1, -1)}, "antimeridian": {(10, 179), (10, -180)}}      # tiles the poses see between them, at least


def winners(orc, name, height_fn=GS.relief):
    """[(uniforms, oracle depth, oracle winners)] of the placement's poses, computed once (no device involved)."""
    key = (name, height_fn)
    if key not in _WINNERS:
        p = GS.placement(name, height_fn)
        o = orc.OracleRenderer(p.W, p.H)
        p.scene.load(o)
        out = []
        for u in p.uniforms():
            o.update(p.W, p.H, u, np.array([p.W, p.H, 100.0, 0.0], np.float32))
            out.append((u,) + tuple(o.render_winners()))
        o.close()
        _WINNERS[key] = out
    return _WINNERS[key]


def pair(topo, orc, name):
    """One renderer / oracle pair per placement, shared by the tests below."""
    if name not in _PAIRS:
        p = GS.placement(name)
        g, o = topo.TerrainRenderer(p.W, p.H), orc.OracleRenderer(p.W, p.H)
        p.scene.load(g)
        p.scene.load(o)
        _PAIRS[name] = (p, g, o)
    return _PAIRS[name]


def _render(topo, p, g, u):
    g.update(p.W, p.H, u, topo.post_uniforms(p.W, p.H))
    return g.render()


@pytest.mark.parametrize("name", GS.NAMES)
def test_frame_and_normals(topo, orc, name):
    p, g, o = pair(topo, orc, name)
    for loc in p.scene.locs:
        assert np.array_equal(g.read_normals(*loc), o.read_normals(loc[0], loc[1], GS.TILE, GS.TILE)), f"{name}: normals of tile {loc}"
    for k, u in enumerate(p.uniforms()):
        o.update(p.W, p.H, u, topo.post_uniforms(p.W, p.H))
        frame = _render(topo, p, g, u)
        assert_same_frame(frame, o.render(), f"{name} pose {k}")
        share = float((frame[1] < 1).mean())
        print(f"{name} pose {k}: terrain covers {100 * share:.1f} % of the frame")
        assert 0.3 < share < 0.8


@pytest.mark.parametrize("name", GS.NAMES)
def test_ground(topo, orc, name):
    p, g, o = pair(topo, orc, name)
    tiles = GR.scene_tiles(p.scene)
    q = GR.all_pixels(topo, [0], p.W, p.H)
    named = set()
    for k, (u, d, w) in enumerate(winners(orc, name)):
        what = f"{name} pose {k}"
        frame = _render(topo, p, g, u)
        got = g.ground(q).reshape(p.H, p.W)
        want = GR.ground(d, w, tiles, p.scene.locs, u)
        GR.compare(got, want, what)
        assert np.array_equal(got["depth"].view(np.uint32), np.asarray(frame[1], np.float32).view(np.uint32)), f"{what}: depth differs from the frame's depth output"
        assert (got["kind"] != -3).all(), what
        GR.assert_sky(got, what)
        vals, pad = ground_map(g, 1, p.W, p.H, pad_px=3, pad_rows=1)
        GR.assert_map_is_list(vals, got.reshape(1, p.H, p.W), what)
        assert (pad == 0xAB).all()
        t = got["kind"] == 1
        mine = set(zip(got["tile_lat_deg"][t].tolist(), got["tile_lon_deg"][t].tolist()))
        t = want["kind"] == 1
        theirs = set(zip(want["tile_lat_deg"][t].tolist(), want["tile_lon_deg"][t].tolist()))
        assert theirs and theirs <= mine and mine <= set(p.scene.locs), (what, mine, theirs)
        if name == "antimeridian":
            assert {lo for _, lo in mine} == {179, -180}, f"{what} sees tiles on both sides of the meridian: {mine}"
        named |= mine
    assert SEEN.get(name, set()) <= named, (name, named)


@pytest.mark.parametrize("name", GS.NAMES)
def test_horizon(topo, orc, name):
    p, g, o = pair(topo, orc, name)
    for k, (u, d, w) in enumerate(winners(orc, name)):
        frame = _render(topo, p, g, u)
        assert g.horizon_shape() == (1, p.W, p.H)
        got = g.horizon()
        assert_view(got[0], horizon(d, w, p.scene.locs, GS.TILE, GS.TILE), f"{name} pose {k}", frame[1])
        assert (got[0]["row"] >= 0).any()


@pytest.mark.parametrize("name", GS.NAMES)
def test_viewshed(topo, orc, name):
    p, g, o = pair(topo, orc, name)
    g.viewshed_enable(True)
    g.viewshed_reset()
    for u in p.uniforms():
        _render(topo, p, g, u)
    g.viewshed_enable(False)
    want = expected_masks([w for _, _, w in winners(orc, name)], p.scene.locs, GS.TILE, GS.TILE)
    assert set(want) == set(p.scene.locs)
    assert_masks(g, want, name)
    seen = {loc for loc, m in want.items() if m.any()}
    assert SEEN.get(name, set()) <= seen and seen
    for loc in set(p.scene.locs) - seen:
        assert not g.viewshed(*loc).any(), f"{name}: tile {loc} is in no frame"
    absent = [(p.scene.locs[0][0] + 5, p.scene.locs[0][1]), (-p.scene.locs[0][0] - 40, p.scene.locs[0][1]), (p.scene.locs[0][0], 180), (3, 3)]
    for loc in absent:
        assert loc not in p.scene.locs
        with pytest.raises(topo.TopoError) as e:
            g.viewshed(*loc)
        assert e.value.code == topo.TOPO_ERR_NOT_FOUND, loc
    g.viewshed_reset()


def sunlit_expected(orc, name, height_fn=GS.relief):
    """Per pose: (uniforms, sun, reference classes, its ambiguous pixels, the classes composed from the g++ builds of topo_ground.h and
    topo_los.h), from the oracle's winners.  No device involved."""
    import ground_emul as GE
    p = GS.placement(name, height_fn)
    tiles, order = GR.scene_tiles(p.scene), LR.geo_order(p.scene.locs)
    mesh = LR.Mesh(tiles)
    out = []
    for (eye, _, _, _), (u, d, w) in zip(p.poses, winners(orc, name, height_fn)):
        sun = LR.sun_direction(eye.vlon, eye.vlat, LC.SUN_AZ, LC.SUN_EL)
        ref, amb = LR.sunlit(mesh, tiles, order, GR.ground(d, w, tiles, p.scene.locs, u), sun)
        emu = LC.compose_sunlit(tiles, order, GE.ground(tiles, order, u, d, w), sun)
        out.append((u, sun, ref, amb, emu))
    return p, out


@pytest.mark.parametrize("name", ["origin", "antimeridian"])
def test_sunlit(topo, orc, name):
    """The sunlit layer of every pose under a sun at azimuth 120, elevation 8 at the pose's eye: the reference outside its ambiguous
    pixels (at most 0.5 % of the frame), and the composition of the two g++ builds; lit, away and shadow each hold at least 5 % of
    the terrain pixels.  The tiles carry los_cases.ridges, not the placements' relief, which this sun lights everywhere."""
    p, poses = sunlit_expected(orc, name, LC.ridges)
    g = topo.TerrainRenderer(p.W, p.H)
    p.scene.load(g)
    for k, (u, sun, ref, amb, emu) in enumerate(poses):
        _render(topo, p, g, u)
        got, pad = sunlit_map(g, sun, 1, p.W, p.H, pad_px=5, pad_rows=2)
        assert (pad == 0xAB).all()
        got = got[0]
        terrain = ref != LR.NONE
        counts = {c: int((ref == c).sum()) for c in (LR.LIT, LR.AWAY, LR.SHADOW)}
        print(f"{name} pose {k}: terrain {int(terrain.sum())}, classes {counts}, ambiguous {int(amb.sum())}")
        assert terrain.sum() > 0.25 * p.W * p.H
        for c, n in counts.items():
            assert n >= 0.05 * terrain.sum(), counts
        assert amb.sum() <= 0.005 * p.W * p.H
        bad = np.argwhere((got != ref) & ~amb)
        assert len(bad) == 0, f"{name} pose {k}: {len(bad)} pixels differ from the reference, first {tuple(bad[0])}: {got[tuple(bad[0])]} vs {ref[tuple(bad[0])]}"
        bad = np.argwhere((got != emu) & ~amb)
        assert len(bad) == 0, f"{name} pose {k}: {len(bad)} pixels differ from the emulation, first {tuple(bad[0])}"
    g.close()


UNWRAP = {"south86": 0, "antimeridian": 1}      # placement: the pose whose eye the panorama is taken from (the western eye at the antimeridian)
UNWRAP_SW, UNWRAP_SH = 96, 160


def unwrap_expected(name):
    """(views, params, the reference's locate) of the placement's 8-sector panorama.  No device involved."""
    eye = GS.placement(name).poses[UNWRAP[name]][0]
    views = eye.panorama(UNWRAP_SW, UNWRAP_SH, yaw0_deg=25.0)
    params = T.unwrap_params(768, 160, 30.0, -30.0)
    return views, params, UR.locate(params, views, UNWRAP_SW, UNWRAP_SH)


@pytest.mark.parametrize("name", sorted(UNWRAP))
def test_unwrap(topo, orc, name):
    """The east / north frame of a southern and of a western eye through k_unwrap: every output pixel names the source texel
    unwrap_ref.locate names (its guard against ties excludes nothing here, as on the cases of tests/test_unwrap_cpu.py), and the
    one the g++ build of topo_unwrap.h names."""
    import torch
    import unwrap_emul
    views, params, ref = unwrap_expected(name)
    assert not ref["fragile"].any(), int(ref["fragile"].sum())
    _, g, _ = pair(topo, orc, name)
    rgba, depth = UC.synthetic_sources(len(views), UNWRAP_SW, UNWRAP_SH)
    r_dev, d_dev = torch.from_numpy(rgba).cuda(), torch.from_numpy(depth).cuda()
    torch.cuda.synchronize()
    got = unwrap_run(topo, g, params, views, UNWRAP_SW, UNWRAP_SH, r_dev, d_dev)
    bad = np.argwhere(got["s"] != ref["src"])
    assert len(bad) == 0, f"{name}: {len(bad)} source-map entries differ from the reference, first {tuple(bad[0])}: {got['s'][tuple(bad[0])]} vs {ref['src'][tuple(bad[0])]}"
    emu = unwrap_emul.unwrap(params, views, UNWRAP_SW, UNWRAP_SH)
    assert np.array_equal(got["s"], emu["src"])
    assert np.array_equal(got["r"], UR.gather(got["s"], rgba, 0))
    assert np.array_equal(got["d"], UR.gather(got["s"], depth.view(np.uint32), 0x7FC00000))
    assert set(np.unique(ref["view"])) == set(range(8)) and (ref["n_containing"] == 1).all()


# ---- the occlusion filter's block bounds (block_bounds_store) off the quadrant --------------------------------------------------------------
def block_sagitta(tile, lat_deg):
    """The sagitta (metres) block_bounds_store finds for a full 60 x 15 cell block of a tile-vertex tile whose centre lies at lat_deg:
    R (1 - cos theta) with theta the angle between the block's centre and a corner (heights left out: + 0.05 % at 3000 m)."""
    dlon, dlat = math.radians(30.0 / tile), math.radians(7.5 / tile)
    la = math.radians(lat_deg)
    cos_t = math.sin(la) * math.sin(la + dlat) + math.cos(la) * math.cos(la + dlat) * math.cos(dlon)
    return 6371000.0 * (1.0 - cos_t)


@pytest.mark.parametrize("name,tile", [("origin", 720), ("antimeridian", 720), ("south86", 720), ("origin", 1000), ("antimeridian", 1000)])
def test_occlusion_filter_off_the_quadrant(topo, orc, name, tile):
    """test_occlusion_filter_is_conservative_on_coarse_tiles' (720, 2, 20000.0) row on the tile sets of three placements, from a corner
    eye 900 m up: filter on == filter off == oracle.  The filter takes a block only where its patch bulges at most 1 m out of the
    flat-faced slab; a 60 x 15 cell block of a 720-vertex tile bulges 0.95 m at 45 degrees and 0.01 m at 85, but 1.79 m on the equator
    and 1.73 m at 10N, where 720-vertex tiles are never filtered (far_tested == 0): 1000-vertex tiles (0.93 m on the equator) put
    the corner directions and the sagitta to use there."""
    sc = GS.tile_set(name, tile, (0.08, 0.07), 900.0)
    W, H = 256, 128
    g, o = topo.TerrainRenderer(W, H), orc.OracleRenderer(W, H)
    sc.load(g)
    sc.load(o)
    pu = topo.post_uniforms(W, H)
    u = sc.uniforms(W, H, 45.0, 4.0, 50.0, 0)
    g.update(W, H, u, pu)
    o.update(W, H, u, pu)
    ref = o.render()
    g.set_occlusion_split(20000.0)
    assert_same_frame(g.render(), ref, f"{name} tile {tile} filter on")
    tested = g.counters()["far_tested"]
    g.set_occlusion_split(0.0)
    assert_same_frame(g.render(), ref, f"{name} tile {tile} filter off")
    assert (ref[1] < 1).mean() > 0.2
    worst = max(block_sagitta(tile, abs(la) + f) for la, _ in sc.locs for f in (0.0, 1.0))      # the most equatorward block of the mosaic ...
    best = min(block_sagitta(tile, abs(la) + f) for la, _ in sc.locs for f in (0.0, 1.0))        # ... and the most poleward one
    print(f"{name} tile {tile}: far_tested {tested}, block sagitta {best:.2f} .. {worst:.2f} m")
    assert worst <= 0.98 or best >= 1.02, "the case must not sit on the allowance"
    if worst <= 1.0:
        assert tested > 0
    else:
        assert tested == 0
    g.close()
    o.close()


# ---- k_raycast on a full-size tile: 1600 raster blocks, 25 batches of 64 ----------------------------------------------------------------
def full_size_case():
    """(tiles, order, rays) of one 1200 x 1200 tile at (46, 7) of _blocks_case's relief: every other ray of that case (the same degree)
    and the rays aimed into the last block row, as the tall and grid cases."""
    lat, lon, n = 46, 7, 1200
    hts = LC.blocks_heights(lat, lon, n, n)
    tiles, order = [(hts,) + tuple(T.synth.tile_transform(lat, lon, n, n))], [(lat, lon)]
    rays, _ = LC.batch_rays(hts, lat, lon, 2, 50, 43)
    return tiles, order, rays


def test_full_size_tile_rays(topo):
    """One 1200 x 1200 tile, about 800 rays: k_raycast against the g++ build of the traversal on every ray, and against the g++ loop
    over every triangle on every eighth (the numpy reference is not run at this size: 2.9 million triangles a ray need gigabytes per
    chunk).  The traversal is not the wave's code, the loop over every triangle is neither's.  The hits fall in at least 20 of the 25
    batches of 64 blocks."""
    tiles, order, rays = full_size_case()
    t0 = time.time()
    emu, bad = LE.raycast(tiles, order, rays)
    brute, bad_b = LE.raycast(tiles, order, rays[::8], brute=True)
    t1 = time.time()
    assert bad == 0 and bad_b == 0
    g = renderer(topo, tiles, order)
    got = g.raycast(rays)
    g.close()
    print(f"full-size tile: {len(rays)} rays, {int((got['kind'] == 1).sum())} hits; the g++ builds took {t1 - t0:.1f} s")
    everyone = np.ones(len(rays), bool)
    LC.against_emulation(got, emu, rays, "full-size tile", everyone)
    LC.against_emulation(got[::8], brute, rays[::8], "full-size tile, every triangle", everyone[::8])
    hit = got["kind"] == topo.RAY_HIT
    assert hit.mean() > 0.4 and (got["kind"] == topo.RAY_MISS).mean() > 0.15
    blk = LC.block_of(got["cell_x"][hit], got["cell_y"][hit], 1200)
    assert blk.max() < 1600
    batches = np.unique(blk // LC.BATCH)
    print(f"full-size tile: hits in {len(batches)} of 25 batches, {int((blk // LC.BATCH == 24).sum())} in the last")
    assert len(batches) >= 20 and (blk // LC.BATCH == 24).sum() >= 20
