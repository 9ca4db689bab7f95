"""Void and non-finite DEM heights on the GPU (tests/void_scenes.py): normals through every load path, frames through every raster
path, the host's keep / drop decisions, the viewshed and horizon queries and the GeoTIFF entry point, all bit for bit against
the oracle.  Every void frame that is compared with the oracle first has to show the void: terrain in a quarter of the
oracle's pixels and one pixel in twenty differing from the clean twin (void_scenes.assert_void_in_view), or, for the
close-ups under the near plane, their own condition (assert_cut_void_in_view)."""

import numpy as np
import pytest

import void_scenes as VS
from horizon_ref import FIELDS, horizon, mismatches
from oracle import ray_check as RC
from scenes import Scene, assert_same_frame
from viewshed_ref import expected_masks, geo_order

pytestmark = pytest.mark.gpu

NO_TRI = 0xFFFFFFFF


def _clean_status(g, what):
    st = g.frame_status()
    assert not st["bounds_violation"] and not st["big_overflow"] and not st["rare_overflow"], (what, st)


# ---- normals -------------------------------------------------------------------------------------------------------------

def _mosaic(topo, tw, th, value):
    """A 2 x 2 mosaic of tw x th tiles with the void pattern: {loc: (heights, transform)}."""
    rng = np.random.default_rng(VS.PATTERN_SEED)
    out = {}
    for (la, lo) in topo.synth.mosaic_locations(45, 15, 2, 2):
        h = topo.synth_tile(la, lo, max(tw, th), max(tw, th))[:th, :tw].copy()
        out[(la, lo)] = (VS.void_pattern(h, VS.VALUES[value], rng), (np.float32([0, 0]), np.float32([lo, la + 1]), np.float32([1.0 / tw, 1.0 / th])))
    return out


# name: tile width, height, topo_set_normals_lds_rows (None: the default), insertion order reversed
LOADS = {
    "rolling48": (48, 48, None, False),        # the default route of a small tile; edge and corner seams
    "rolling48_reversed": (48, 48, None, True),
    "lds8_48": (48, 48, 8, False),             # k_normals_interior<8>
    "lds32_46": (46, 46, None, False),         # a width that is no multiple of four: the LDS form with its default 32 rows
    "one_pass_240x47": (240, 47, None, False),  # k_normals_rolling<4, 4, true>: normals and block minima / maxima in one pass
    "one_pass_480x31": (480, 31, None, False),
    "no_lds_152": (152, 152, 0, False),        # the no-LDS switch as test_normals_without_lds_byte_exact sets it
}


@pytest.mark.parametrize("value", VS.NORMALS_VALUES)
@pytest.mark.parametrize("load", list(LOADS))
def test_normals_of_void_tiles_byte_exact(topo, orc, load, value):
    tw, th, rows, rev = LOADS[load]
    tiles = _mosaic(topo, tw, th, value)
    order = list(tiles)[::-1] if rev else list(tiles)
    g, o = topo.TerrainRenderer(16, 16), orc.OracleRenderer(16, 16)
    if rows is not None:
        g.set_normals_lds_rows(rows)
    for loc in order:
        g.add_terrain(loc[0], loc[1], tiles[loc][0], *tiles[loc][1])
        o.add_terrain(loc[0], loc[1], tiles[loc][0], *tiles[loc][1])
    ref = {loc: o.read_normals(loc[0], loc[1], tw, th) for loc in tiles}
    n_void = sum(int((~np.isfinite(h) | (np.abs(h) > 9000.0)).sum()) for h, _ in tiles.values())
    assert n_void > 0.01 * 4 * tw * th
    for loc in tiles:
        a = g.read_normals(*loc)
        assert np.array_equal(a, ref[loc]), f"{load} {value} add_terrain tile {loc}: {np.argwhere((a != ref[loc]).any(axis=-1))[:4]}"
    g.recompute_normals()      # the batched launches
    for loc in tiles:
        assert np.array_equal(g.read_normals(*loc), ref[loc]), f"{load} {value} recompute tile {loc}"
    if load.startswith("one_pass"):
        # the block minima / maxima of the one-pass route are fminf / fmaxf reductions: a partly void block is an ordinary
        # block, and the separate kernels leave the same tables
        sep = topo.TerrainRenderer(16, 16)
        sep.set_normals_lds_rows(8)
        for loc in order:
            sep.add_terrain(loc[0], loc[1], tiles[loc][0], *tiles[loc][1])
        bxc = (tw - 1 + 59) // 60
        for loc in tiles:
            assert np.array_equal(sep.read_normals(*loc), ref[loc]), loc
            a, b = g.read_tile_tables(*loc), sep.read_tile_tables(*loc)
            for k in ("minmax", "trig", "bounds"):
                assert np.array_equal(a[k], b[k], equal_nan=True), (loc, k, np.argwhere(a[k] != b[k])[:4])
            for blk, (lo_, hi_) in enumerate(a["minmax"]):
                by, bx = divmod(blk, bxc)
                v = tiles[loc][0][15 * by:min(15 * by + 16, th), 60 * bx:min(60 * bx + 61, tw)]
                want = (np.fmin.reduce(v, axis=None), np.fmax.reduce(v, axis=None))
                assert np.array_equal(np.float32([lo_, hi_]), np.float32(want), equal_nan=True), (loc, blk, lo_, hi_, want)


# ---- frames --------------------------------------------------------------------------------------------------------------

def _gpu_equals_oracle(topo, orc, key, sc, void, W, H, pose, close_up=False):
    pu = topo.post_uniforms(W, H)
    ref, clean = VS.oracle_frames(orc, key, sc, void, W, H, pose, pu)
    if close_up:
        VS.assert_cut_void_in_view(sc, void, sc.uniforms(W, H, *pose), ref[1], clean[1], str(key))
    else:
        VS.assert_void_in_view(ref[1], clean[1], str(key))
    g = topo.TerrainRenderer(W, H)
    void.load(g)
    g.update(W, H, sc.uniforms(W, H, *pose), pu)
    frame = g.render()
    assert_same_frame(frame, ref, f"gpu {key}")
    _clean_status(g, key)
    return g


@pytest.mark.parametrize("value", list(VS.VALUES))
@pytest.mark.parametrize("name", list(VS.RELIEF))
def test_frames_of_void_tiles_bit_exact(topo, orc, name, value):
    sc, void, W, H, pose = VS.relief_case(name, value)
    g = _gpu_equals_oracle(topo, orc, (name, value), sc, void, W, H, pose)
    o = orc.OracleRenderer(W, H)
    void.load(o)
    for loc in void.locs:
        assert np.array_equal(g.read_normals(*loc), o.read_normals(loc[0], loc[1], void.tile, void.tile)), loc


@pytest.mark.parametrize("value", VS.NORMALS_VALUES)
def test_frame_with_a_whole_tile_void(topo, orc, value):
    _gpu_equals_oracle(topo, orc, ("ne_2x2", value, "whole"), *VS.relief_case("ne_2x2", value, whole_tile=True))


@pytest.mark.parametrize("name", list(VS.CLOSE))
def test_cut_primitives_beside_voids(topo, orc, name):
    """The rare path (k_raster_rare -> the big queue): primitives cut by the near plane with a void among their vertices are
    discarded as a whole when any vertex of the clipped polygon leaves the guard band."""
    big = rare = 0
    for value in VS.CLOSE_VALUES:
        for seed in VS.CLOSE_SEEDS:
            g = _gpu_equals_oracle(topo, orc, (name, value, seed), *VS.close_case(name, value, seed), close_up=True)
            big += g.counters()["big_items"]
            rare += g.counters()["rare_items"]
    print(f"{name}: big_items {big} rare_items {rare}")
    assert rare > 0
    if name == "close_1x1":
        assert big > 0


FAR = dict(tile=720, n_lat=2, n_lon=2, vfrac=(0.08, 0.07), eye_dh=900.0)      # test_occlusion_filter_is_conservative_on_coarse_tiles
_FAR = {}


def _far_case(value):
    if "clean" not in _FAR:
        _FAR["clean"] = Scene(**FAR)
    sc = _FAR["clean"]
    # 2 % specks are sub-pixel out there: the eye tile's 4 x 5 patch is put 1.5 km in front of the eye, where it fills a few
    # hundred pixels (the eye stands at row 604, column 100 of tile (45, 15))
    return sc, VS.patterned(sc, VS.VALUES[value], patches={(45, 15): (610, 110)}), 256, 128, (45.0, 10.0, 50.0, 0)


@pytest.mark.parametrize("value", ["nan", "m32767"])
def test_far_phase_on_void_tiles(topo, orc, value):
    """720-px tiles: blocks behind the occlusion split are tested against the near field's depth (k_occlusion) from block bounds
    that fminf / fmaxf reduced over partly void blocks.  Filter on == filter off == oracle."""
    sc, void, W, H, pose = _far_case(value)
    pu = topo.post_uniforms(W, H)
    ref, clean = VS.oracle_frames(orc, ("far", value), sc, void, W, H, pose, pu)
    VS.assert_void_in_view(ref[1], clean[1], f"far {value}")
    g = topo.TerrainRenderer(W, H)
    void.load(g)
    g.update(W, H, sc.uniforms(W, H, *pose), pu)
    g.set_occlusion_split(20000.0)
    assert_same_frame(g.render(), ref, f"far {value}, split 20 km")
    assert g.counters()["far_tested"] > 0, g.counters()
    _clean_status(g, value)
    g.set_occlusion_split(0.0)
    assert_same_frame(g.render(), ref, f"far {value}, filter off")
    _clean_status(g, value)


def _views_case(orc, topo, key, poses):
    """The down_1x1 relief scene with the NaN pattern seen from `poses`: (scene, void twin, W, H, uniforms, oracle frames); every
    view has to show the void."""
    sc, void, W, H, _ = VS.relief_case("down_1x1", "nan")
    pu = topo.post_uniforms(W, H)
    us, refs = [], []
    for k, pose in enumerate(poses):
        ref, clean = VS.oracle_frames(orc, (key, k), sc, void, W, H, pose, pu)
        VS.assert_void_in_view(ref[1], clean[1], f"{key} view {k}")
        us.append(sc.uniforms(W, H, *pose))
        refs.append(ref)
    return sc, void, W, H, us, refs


def _submit(g, us, W, H):
    import torch
    n = len(us)
    rgba = torch.zeros((n, H, W, 4), dtype=torch.uint8, device="cuda")
    depth = torch.zeros((n, H, W), dtype=torch.float32, device="cuda")
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    g.render_views_device(us, W, H, rgba.data_ptr(), H * W * 4, W * 4, depth.data_ptr(), H * W * 4, W * 4)
    torch.cuda.synchronize()
    return rgba.cpu().numpy(), depth.cpu().numpy()


@pytest.mark.parametrize("n", [8, 9], ids=["eight_views_packed", "nine_views_by_copy"])
def test_void_scene_in_multi_view_submissions(topo, orc, n):
    """One submission of eight views (the panorama's shape: the views travel packed in the launch arguments) and one of nine (the
    view block is copied), looking down at the void tile all round the compass."""
    poses = [(360.0 * k / n + 10.0, 75.0, 90.0, k % 3) for k in range(n)]
    sc, void, W, H, us, refs = _views_case(orc, topo, f"views{n}", poses)
    g = topo.TerrainRenderer(W, H)
    void.load(g)
    rgba, depth = _submit(g, us, W, H)
    for k in range(n):
        assert_same_frame((rgba[k], depth[k]), refs[k], f"{n}-view submission, view {k}")
    _clean_status(g, n)


# ---- host decisions ------------------------------------------------------------------------------------------------------

HOST = dict(tile=32, n_lat=3, n_lon=3, eye_dh=5000.0, vfrac=(0.643, 0.643))      # the eye in the centre tile's north-east corner
HOST_SIZE = (96, 64)
HOST_POSES = [(yaw, 30.0, 60.0, 0) for yaw in (45.0, 135.0, 225.0, 315.0)]      # east, north, west, south
HOST_ALL_NAN, HOST_PATTERN = (47, 16), (46, 17)      # the tile north of the eye's, the tile east of it


def _host_scene():
    sc = Scene(height_fn=VS.relief, **HOST)
    rng = np.random.default_rng(VS.PATTERN_SEED)
    hts = dict(sc.heights)
    hts[HOST_ALL_NAN] = VS.void_tile(hts[HOST_ALL_NAN], np.nan)
    hts[HOST_PATTERN] = VS.void_pattern(hts[HOST_PATTERN], np.nan, rng)
    return sc, VS.with_heights(sc, hts)


def test_prefilter_keeps_a_tile_whose_sphere_is_unknown(topo, orc):
    """A tile that is NaN all over has no finite block sphere: add_terrain marks its sphere unknown and the prefilter keeps its
    pair in every view, also in those that look away from it, while the tiles beside it are still dropped.  A tile with NaN
    specks has a finite sphere (fminf / fmaxf skip the NaN) and is filtered like any other.  Prefilter on == off."""
    sc, void = _host_scene()
    W, H = HOST_SIZE
    pu = topo.post_uniforms(W, H)
    g, without = topo.TerrainRenderer(W, H), topo.TerrainRenderer(W, H)
    void.load(g)
    void.load(without, [loc for loc in void.locs if loc != HOST_ALL_NAN])      # the same spheres, minus the all-NaN tile
    o = orc.OracleRenderer(W, H)
    sc.load(o)
    rank_nan = geo_order(sc.locs).index(HOST_ALL_NAN)
    tpt = 2 * (sc.tile - 1) ** 2
    away = compared = 0
    for k, pose in enumerate(HOST_POSES):
        u = sc.uniforms(W, H, *pose)
        for r in (g, without):
            r.update(W, H, u, pu)
            r.debug_set_tile_prefilter(True)
        on = g.render()
        launched, pairs = g.debug_cull_pairs()
        c_on = g.counters()
        without.render()
        launched_without, pairs_without = without.debug_cull_pairs()
        print(f"yaw {pose[0]}: pairs launched {launched} of {pairs}; without the all-NaN tile {launched_without} of {pairs_without}")
        assert (pairs, pairs_without) == (9, 8)
        assert launched == launched_without + 1, "the all-NaN tile's pair was dropped"
        assert launched < pairs, "no tile was dropped"
        g.debug_set_tile_prefilter(False)
        off = g.render()
        assert g.debug_cull_pairs() == (9, 9)
        assert_same_frame(on, off, f"prefilter on vs off, yaw {pose[0]}")
        assert c_on == g.counters()
        _clean_status(g, pose)
        # a view that looks away from the all-NaN tile: the clean twin shows none of it
        o.update(W, H, u, pu)
        win = o.render_winners()[1]
        away += not ((win != NO_TRI) & (win // tpt == rank_nan)).any()
        ref, clean = VS.oracle_frames(orc, ("host", k), sc, void, W, H, pose, pu)
        changed = float((ref[1].view(np.uint32) != clean[1].view(np.uint32)).mean())
        if float((ref[1] < 1.0).mean()) >= 0.25 and changed >= 0.05:      # the views that show the voids are compared with the oracle
            VS.assert_void_in_view(ref[1], clean[1], f"host yaw {pose[0]}")
            assert_same_frame(on, ref, f"host yaw {pose[0]}")
            compared += 1
    assert away > 0 and compared > 0, (away, compared)


def test_prefilter_drops_a_sentinel_tile_only_when_out_of_view(topo, orc):
    """-32767 specks leave the tile's sphere finite (and large): its pair may be dropped only when the oracle's frame has none of
    that tile's pixels."""
    sc = Scene(height_fn=VS.relief, **HOST)
    victim = HOST_PATTERN
    void = VS.patterned(sc, -32767.0, only=(victim,))
    W, H = HOST_SIZE
    pu = topo.post_uniforms(W, H)
    g, without = topo.TerrainRenderer(W, H), topo.TerrainRenderer(W, H)
    void.load(g)
    void.load(without, [loc for loc in void.locs if loc != victim])
    o = orc.OracleRenderer(W, H)
    void.load(o)
    rank = geo_order(sc.locs).index(victim)
    tpt = 2 * (sc.tile - 1) ** 2
    shown = 0
    for k, pose in enumerate(HOST_POSES):
        u = sc.uniforms(W, H, *pose)
        for r in (g, without, o):
            r.update(W, H, u, pu)
        g.render()
        without.render()
        kept = g.debug_cull_pairs()[0] - without.debug_cull_pairs()[0]
        assert kept in (0, 1)
        win = o.render_winners()[1]
        in_view = bool(((win != NO_TRI) & (win // tpt == rank)).any())
        print(f"yaw {pose[0]}: pair kept {kept}, tile in the oracle's frame {in_view}")
        assert kept or not in_view, f"yaw {pose[0]}: the pair of a tile the oracle shows was dropped"
        shown += in_view
        _clean_status(g, pose)
    assert shown > 0


# ---- queries -------------------------------------------------------------------------------------------------------------

def test_viewshed_and_horizon_of_a_void_scene(topo, orc):
    sc, void, W, H, pose = VS.relief_case("ne_2x2", "nan")
    pu = topo.post_uniforms(W, H)
    ref, clean = VS.oracle_frames(orc, ("ne_2x2", "nan"), sc, void, W, H, pose, pu)
    VS.assert_void_in_view(ref[1], clean[1], "queries")
    g, o = topo.TerrainRenderer(W, H), orc.OracleRenderer(W, H)
    void.load(g)
    void.load(o)
    g.viewshed_enable(True)
    u = sc.uniforms(W, H, *pose)
    g.update(W, H, u, pu)
    o.update(W, H, u, pu)
    frame = g.render()
    assert_same_frame(frame, ref, "queries frame")
    od, ow = o.render_winners()
    tile = void.tile
    want = expected_masks([ow], void.locs, tile, tile)
    tris = RC.tile_triangles(tile, tile)
    dead_cells = marked = 0
    for loc, m in want.items():
        got = g.viewshed(*loc)
        bad = np.argwhere(got != m)
        assert len(bad) == 0, f"tile {loc}: {len(bad)} cells differ (first (y, x) {tuple(bad[0])})"
        # a cell both of whose triangles have a void vertex is never marked
        fin = np.isfinite(void.heights[loc])
        dead_tri = np.array([not all(fin[j, i] for i, j in t) for t in tris])
        dead = (dead_tri[0::2] & dead_tri[1::2]).reshape(tile - 1, tile - 1).T      # cell = i * (h - 1) + j -> [y = j, x = i]
        assert not (got & dead).any(), loc
        dead_cells += int(dead.sum())
        marked += int(got.sum())
    assert dead_cells > 0 and marked > 0
    hw = horizon(od, ow, void.locs, tile, tile)
    got = g.horizon()[0]
    for f in FIELDS:
        bad = mismatches(got, hw, f)
        assert len(bad) == 0, f"horizon {f} differs in {len(bad)} columns (first {bad[0]}: got {got[f][bad[0]]}, want {hw[f][bad[0]]})"
    assert (got["row"] >= 0).any()


# ---- GeoTIFF -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("value", ["nan", "fmin"])
def test_add_terrain_geotiff_of_a_void_tile(topo, orc, value):
    """The void tile written as a GeoTIFF (floating-point predictor, Deflate) renders the frame add_terrain of the same array
    renders: the decode hands the void bits on unchanged."""
    from tiff_writer import write_geotiff
    sc, void, W, H, pose = VS.relief_case("down_1x1", value)
    pu = topo.post_uniforms(W, H)
    ref, clean = VS.oracle_frames(orc, ("down_1x1", value), sc, void, W, H, pose, pu)
    VS.assert_void_in_view(ref[1], clean[1], f"geotiff {value}")
    a, b = topo.TerrainRenderer(W, H), topo.TerrainRenderer(W, H)
    for loc in void.locs:
        rp, mp, ps = void.transform(loc)
        data = write_geotiff(void.heights[loc], tile=(16, 16), pixel_scale=(float(ps[0]), float(ps[1]), 0.0),
                             tie_points=(float(rp[0]), float(rp[1]), 0.0, float(mp[0]), float(mp[1]), 0.0))
        assert np.array_equal(a.decode_geotiff(data).view(np.uint32), void.heights[loc].view(np.uint32))
        a.add_terrain_geotiff(loc[0], loc[1], data)
    void.load(b)
    u = sc.uniforms(W, H, *pose)
    a.update(W, H, u, pu)
    b.update(W, H, u, pu)
    fa = a.render()
    assert_same_frame(fa, b.render(), f"GeoTIFF bytes vs add_terrain, {value}")
    assert_same_frame(fa, ref, f"GeoTIFF bytes vs oracle, {value}")
    for loc in void.locs:
        assert np.array_equal(a.read_normals(*loc), b.read_normals(*loc))
