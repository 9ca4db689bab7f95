"""The map view without a GPU (topo_map_*): the g++ build of csrc/topo_map.h run as k_map runs it -- waves of 64 columns x R rows over
the tile lists of their box test -- against the same waves over every tile and against a plain loop over every triangle, byte for
byte (tests/map_emul.cpp); against the independent numpy reference (tests/map_ref.py); on tiles whose answer can be named on paper;
topo_map_xy; and the calls' argument checks that need no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import map_cases as MC
import map_emul as ME
import map_ref as MR
import surface_cases as SC

HERE = os.path.dirname(os.path.abspath(__file__))
R = MC.R


@pytest.mark.parametrize("name", sorted(MC.CASES))
def test_wave_form_equals_every_tile_and_the_plain_loop(name):
    rgba, flags, bad, stats = MC.run(name, ME.WAVES)
    tiles, _ = MC.tile_set(MC.CASES[name][0])
    assert bad == 0 and stats[2] == 0 and stats[0] <= len(tiles) * stats[1]
    for mode in (ME.ALL_TILES, ME.BRUTE):
        rgba2, flags2, bad2, _ = MC.run(name, mode)
        assert bad2 == 0
        assert np.array_equal(flags, flags2), f"{name}: flags differ from mode {mode} at {np.argwhere(flags != flags2)[:5].tolist()}"
        assert np.array_equal(rgba, rgba2), f"{name}: rgba differs from mode {mode}"
    layers = MC.CASES[name][4]
    assert ((flags & MR.F_INDEX) == 0)[(flags & MR.F_CONTOUR) == 0].all(), "index implies contour"
    assert not (flags[(flags & MR.F_TERRAIN) == 0]).any(), "a void pixel is 0"
    if not layers & MR.CONTOURS:
        assert not (flags & (MR.F_CONTOUR | MR.F_INDEX)).any()
    if not layers & MR.SEEN or MC.CASES[name][5] in ("zero", "none"):
        assert not (flags & MR.F_SEEN).any()
    void = (flags & MR.F_TERRAIN) == 0
    assert (rgba[void] == np.uint8([10, 20, 30, 40])).all() and (rgba[~void][:, 3] == 255).all()


def test_the_box_test_shortens_the_lists():
    """Three tiles in a row, a grid over the first: every wave lists one tile or two, never the far one."""
    _, _, _, stats = MC.run("long_gap", ME.WAVES)
    assert stats[0] < 3 * stats[1]


@pytest.mark.parametrize("name", sorted(MC.CASES))
def test_against_the_reference(name):
    """The reference alone must call at most SC.MAX_AMBIGUOUS of the pixels ambiguous; outside those the flags are equal and the grey
    code lies within 1 of the reference's: an f32 shading error of about 1e-6 against code widths of at least 3e-4 in linear light
    can move a value across one threshold, never two."""
    ref = MC.reference(name)
    share = float(ref["ambiguous"].mean())
    print(f"{name}: {ref['flags'].size} pixels, {int(ref['terrain'].sum())} terrain, ambiguous {share:.4%}")
    assert share <= SC.MAX_AMBIGUOUS, f"{name}: the reference calls {share:.4%} of the pixels ambiguous"
    rgba, flags, bad, _ = MC.run(name, ME.WAVES)
    keep = ~ref["ambiguous"]
    diff = np.argwhere(keep & (flags != ref["flags"]))
    assert len(diff) == 0, f"{name}: flags differ at {diff[:5].tolist()}: {flags[tuple(diff[0])]} vs {ref['flags'][tuple(diff[0])]}"
    # the grey: the relief layer alone puts the code into R, G and B
    ts, layers = MC.CASES[name][0], MC.CASES[name][4]
    tiles, _ = MC.tile_set(ts)
    p = MC.params(name).copy()
    p["layers"] = layers & MR.RELIEF
    grey_rgba, _, bad, _ = ME.run(tiles, MC.normals(ts), p, None, ME.WAVES)
    assert bad == 0
    t = keep & ref["terrain"]
    grey = grey_rgba[..., 0].astype(np.int64)
    assert (grey_rgba[t][:, 0] == grey_rgba[t][:, 1]).all() and (grey_rgba[t][:, 1] == grey_rgba[t][:, 2]).all()
    err = np.abs(grey - ref["grey"])[t]
    if t.any():
        print(f"{name}: grey codes {grey[t].min()} .. {grey[t].max()}, {int((err == 1).sum())} of {int(t.sum())} one off the reference")
        assert err.max() <= 1, f"{name}: grey differs by {err.max()}"
    # the composition: where the grey is the reference's, so is the pixel
    same = keep & ((grey == ref["grey"]) | ~ref["terrain"])
    assert np.array_equal(rgba[same], ref["rgba"][same]), f"{name}: rgba differs from the reference's composition"


def test_cases_cover_what_they_are_meant_to():
    f = {n: MC.run(n, ME.WAVES)[1] for n in ("blocks_coarse", "blocks_dlon0", "huge_interval", "steep_small_interval", "sentinels", "long_gap", "index_0", "index_1")}
    assert (f["blocks_coarse"][:, 0] == 0).all() and (f["blocks_coarse"][0] == 0).all(), "the grid starts outside the mosaic"
    assert not (f["huge_interval"] & MR.F_CONTOUR).any() and (f["steep_small_interval"] & MR.F_CONTOUR).mean() > 0.9
    assert not (f["index_0"] & MR.F_INDEX).any() and np.array_equal((f["index_1"] & MR.F_INDEX) != 0, (f["index_1"] & MR.F_CONTOUR) != 0)
    assert (f["sentinels"] & MR.F_CONTOUR).any(), "the pit's rim is a contour of negative levels"
    gap = f["long_gap"]
    assert ((gap & MR.F_TERRAIN) == 0).any(axis=0).sum() >= 1 and (gap & MR.F_TERRAIN).any(), "a column of the grid falls into the gap"
    # dlon = 0: one longitude, so no pixel differs from its east neighbour -- the contours are the south neighbours' alone
    d0 = f["blocks_dlon0"]
    assert (d0 == d0[:, :1]).all()


def test_more_tiles_than_a_list_holds():
    """70 copies of one small tile: every wave's box keeps them all, the list overflows and the wave walks the table."""
    tiles, _ = MC.small_tile(100.0 + 40.0 * np.add.outer(np.arange(5.0), np.arange(5.0)))
    tiles = tiles * 70
    nrm = MC.flat_normals(tiles)
    g = MC.cell_grid(tiles[0], -0.31, 3.87, -0.23, 3.79, 66, R + 1)
    p = MC.T.map_params(g["lon0"], g["lat0"], g["dlon"], g["dlat"], g["nx"], g["ny"], sun_direction=MC.sun(15.0, 46.0), contour_interval_m=10.0, index_every=5)
    rgba, flags, bad, stats = ME.run(tiles, nrm, p, None, ME.WAVES)
    assert bad == 0 and stats[2] == stats[1] > 0
    rgba2, flags2, bad2, _ = ME.run(tiles, nrm, p, None, ME.BRUTE)
    assert bad2 == 0 and np.array_equal(rgba, rgba2) and np.array_equal(flags, flags2) and (flags & MR.F_TERRAIN).any()


def test_a_tile_across_the_antimeridian():
    """A tile whose columns run from 179.99 E to 179.99 W: grids given east and west of 180 find it, and their lists hold it."""
    tiles, _ = MC.small_tile(300.0 + 25.0 * np.add.outer(np.arange(9.0), np.arange(11.0)), lat=10, lon=180.0 - 5 * MC.POST)
    nrm = MC.flat_normals(tiles)
    out = []
    for lon_a in (180.0 - 5.3 * MC.POST, -180.0 - 5.3 * MC.POST, 180.0 - 5.3 * MC.POST + 720.0):
        p = MC.T.map_params(lon_a, 11.0 + 0.4 * MC.POST, 0.161 * MC.POST, -0.97 * MC.POST, 68, R + 1, sun_direction=MC.sun(180.0, 11.0), contour_interval_m=10.0, index_every=5)
        res = [ME.run(tiles, nrm, p, None, mode) for mode in (ME.WAVES, ME.BRUTE)]
        assert res[0][2] == 0 and np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
        assert (res[0][1][1:, 2:64] & MR.F_TERRAIN).all() and not (res[0][1][:, 0] & MR.F_TERRAIN).any()      # column c lies 0.161 c - 0.3 posts into the tile's ten
        out.append(res[0][1] & MR.F_TERRAIN)
    assert np.array_equal(out[0], out[1]) and np.array_equal(out[0], out[2])


def test_box_test_limits():
    """The box keeps the tile under it and drops one far away; a box beyond 1e6 degrees and a full turn keep every tile; a zero
    pixel scale has no surface."""
    tiles, _ = MC.small_tile(np.zeros((9, 9)))
    nrm = MC.flat_normals(tiles)
    mp = lambda lon0, lat0, dlon, dlat: MC.T.map_params(lon0, lat0, dlon, dlat, 64, 8)
    assert ME.box_keeps(tiles, nrm, 0, mp(15.001, 45.999, 1e-4, -1e-4), 0, 63, 0, 7)
    assert not ME.box_keeps(tiles, nrm, 0, mp(16.001, 45.999, 1e-4, -1e-4), 0, 63, 0, 7)
    assert not ME.box_keeps(tiles, nrm, 0, mp(15.001, 44.9, 1e-4, -1e-4), 0, 63, 0, 7)
    assert ME.box_keeps(tiles, nrm, 0, mp(15.001 - 3600.0, 45.999, 1e-4, 0.0), 0, 63, 0, 7), "longitudes wrap"
    assert ME.box_keeps(tiles, nrm, 0, mp(100.0, 45.999, 6.0, 0.0), 0, 63, 0, 7), "a box of a full turn"
    assert ME.box_keeps(tiles, nrm, 0, mp(1.0e7, 45.999, 1e-4, 0.0), 0, 63, 0, 7), "beyond 1e6 degrees every longitude"
    assert ME.box_keeps(tiles, nrm, 0, mp(15.02, 45.999, -1e-4, 0.0), 0, 63, 0, 7), "negative steps"
    flat = [(tiles[0][0], tiles[0][1], tiles[0][2], np.float32([0.0, MC.POST]))]
    assert not ME.box_keeps(flat, nrm, 0, mp(15.001, 45.999, 1e-4, -1e-4), 0, 63, 0, 7)


# ---- hand-known tiles ------------------------------------------------------------------------------------------------------------
def test_plane_tilted_east():
    """3 x 3 posts, height 25 + 100 x: with a 50 m interval the level of column c is floor((25 + 100 x_c) / 50), rows are equal, so the
    contour columns are those whose right neighbour has another level, and with index_every = 2 the index columns those that cross a
    multiple of 100 m."""
    tiles, _ = MC.small_tile(25.0 + 100.0 * np.tile(np.arange(3.0), (3, 1)))
    nx, ny = 16, 4
    g = MC.cell_grid(tiles[0], 0.03, 1.97, 0.21, 1.83, nx, ny)
    p = MC.T.map_params(g["lon0"], g["lat0"], g["dlon"], g["dlat"], nx, ny, sun_direction=MC.sun(15.0, 46.0), contour_interval_m=50.0, index_every=2)
    rgba, flags, bad, _ = ME.run(tiles, MC.flat_normals(tiles), p, None, ME.WAVES)
    x = 0.03 + (1.97 - 0.03) * np.arange(nx) / (nx - 1)
    height = 25.0 + 100.0 * x
    assert (np.abs(height / 50.0 - np.round(height / 50.0)) > 0.02).all(), "no column within a metre of a level"
    level = np.floor(height / 50.0)
    contour = np.append(level[:-1] != level[1:], False)
    index = np.append(np.floor(level[1:] / 2.0) > np.floor(level[:-1] / 2.0), False)
    assert contour.sum() == 4 and index.sum() == 2
    want = MR.F_TERRAIN | np.where(contour, MR.F_CONTOUR, 0) | np.where(index, MR.F_INDEX, 0)
    assert bad == 0 and (flags == want[None, :]).all(), flags
    assert (rgba[:, index] == np.uint8([64, 32, 16, 255])).all(), "an opaque index colour replaces the grey"


def test_flat_tile():
    tiles, _ = MC.small_tile(np.full((4, 5), 123.4))
    g = MC.cell_grid(tiles[0], 0.07, 3.91, 0.13, 2.89, 40, 12)
    p = MC.T.map_params(g["lon0"], g["lat0"], g["dlon"], g["dlat"], 40, 12, sun_direction=MC.sun(15.0, 46.0), contour_interval_m=50.0, index_every=2)
    rgba, flags, bad, _ = ME.run(tiles, MC.flat_normals(tiles), p, None, ME.WAVES)
    assert bad == 0 and (flags == MR.F_TERRAIN).all(), "no contour"
    assert (rgba == rgba[0, 0]).all() and rgba[0, 0, 3] == 255 and 100 < rgba[0, 0, 0] < 255, "one grey"
    # the light from straight above: 0.01 + 0.7 cos(angle between the texel's normal and the sun)
    up = MC.T.sun_direction(15.0, 46.0, 0.0, 90.0).astype(np.float32)
    p["sun_direction"][0] = up
    p["layers"] = MR.RELIEF
    rgba, _, _, _ = ME.run(tiles, MC.flat_normals(tiles), p, None, ME.WAVES)
    assert abs(int(rgba[0, 0, 0]) - int(MR.srgb_code(0.71))) <= 1


def test_one_marked_cell():
    """Cell (1, 0) of a 3 x 3 tile marked: exactly the pixels inside it are seen, in both its triangles."""
    tiles, _ = MC.small_tile(500.0 + 30.0 * np.add.outer(np.arange(3.0), np.arange(3.0)))
    mask = np.zeros((2, 2), bool)
    mask[0, 1] = True      # [y, x]
    nx = ny = 41
    g = MC.cell_grid(tiles[0], -0.13, 2.11, -0.17, 2.09, nx, ny)
    p = MC.T.map_params(g["lon0"], g["lat0"], g["dlon"], g["dlat"], nx, ny, layers=MR.SEEN, seen_rgba=(255, 0, 0, 255))
    rgba, flags, bad, _ = ME.run(tiles, MC.flat_normals(tiles), p, [mask], ME.WAVES)
    x = -0.13 + (2.11 + 0.13) * np.arange(nx) / (nx - 1)
    y = -0.17 + (2.09 + 0.17) * np.arange(ny) / (ny - 1)
    inside = ((x > 1) & (x < 2))[None, :] & ((y > 0) & (y < 1))[:, None]
    terrain = ((x > 0) & (x < 2))[None, :] & ((y > 0) & (y < 2))[:, None]
    assert bad == 0 and np.array_equal((flags & MR.F_SEEN) != 0, inside) and np.array_equal((flags & MR.F_TERRAIN) != 0, terrain)
    assert inside.sum() > 200 and (rgba[inside] == np.uint8([255, 0, 0, 255])).all() and (rgba[terrain & ~inside] == 255).all()
    # both triangles of the cell: pixels either side of its diagonal
    sub = inside[:, ((x > 1) & (x < 2))][((y > 0) & (y < 1))]
    assert sub.all() and sub.shape[0] >= 15 and sub.shape[1] >= 15


def test_helpers_blend_and_floor_division():
    L = ME.lib()
    for a, n in ((7, 5), (-7, 5), (-10, 5), (0, 5), (-1, 1), (10, 5), (-(1 << 62), 3), ((1 << 62), 7)):
        assert L.emul_map_floor_div(a, n) == a // n
    rng = np.random.default_rng(5)
    for c, s in rng.integers(0, 1 << 32, (200, 2), dtype=np.uint64):
        got = L.emul_map_blend(int(c), int(s))
        a = int(s) >> 24
        want = int(c) & 0xFF000000
        for k in (0, 8, 16):
            want |= ((((int(c) >> k) & 255) * (255 - a) + ((int(s) >> k) & 255) * a + 127) // 255) << k
        assert got == want
    assert L.emul_map_blend(0xFF123456, 0x00FFFFFF) == 0xFF123456 and L.emul_map_blend(0xFF123456, 0xFFABCDEF) == 0xFFABCDEF


# ---- topo_map_xy -----------------------------------------------------------------------------------------------------------------
def test_map_xy(topo):
    p = topo.map_params(179.2, 47.0, 0.0125, -0.0075, 130, 40)
    c, r = np.meshgrid(np.arange(130.0), np.arange(40.0))
    pos = MR.positions(p)
    xy = topo.map_xy(p, pos.reshape(-1, 2)).reshape(40, 130, 2)
    assert np.abs(xy[..., 0] - c).max() < 1e-9 and np.abs(xy[..., 1] - r).max() < 1e-9, "the round trip of the pixel positions"
    # the grid crosses 180: a longitude given west of it lands on the same column, and so does one a turn away
    east, west, turn = topo.map_xy(p, [[180.45, 46.9], [-179.55, 46.9], [180.45 - 720.0, 46.9]])
    assert abs(east[0] - 100.0) < 1e-9 and np.allclose(east, west, atol=1e-9) and np.allclose(east, turn, atol=1e-9)
    # fractional and outside values are reported as they are
    assert np.allclose(topo.map_xy(p, [[179.2 - 0.025, 47.0075]]), [[-2.0, -1.0]], atol=1e-9)
    # NaN: invalid points, a zero step in the direction asked, null or non-finite parameters
    bad = topo.map_xy(p, [[np.nan, 46.0], [179.0, 91.0], [np.inf, 0.0], [179.0, np.nan]])
    assert np.isnan(bad).all()
    p0 = topo.map_params(10.0, 47.0, 0.0, -0.01, 8, 8)
    got = topo.map_xy(p0, [[10.0, 46.95]])
    assert np.isnan(got[0, 0]) and abs(got[0, 1] - 5.0) < 1e-9
    p0 = topo.map_params(10.0, 47.0, 0.01, 0.0, 8, 8)
    got = topo.map_xy(p0, [[10.03, 46.95]])
    assert abs(got[0, 0] - 3.0) < 1e-9 and np.isnan(got[0, 1])
    out = np.zeros((1, 2))
    ll = np.array([[10.0, 46.0]])
    topo.lib().topo_map_xy(None, 1, ll.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    assert np.isnan(out).all()
    assert np.isnan(topo.map_xy(topo.map_params(np.nan, 47.0, 0.01, 0.01, 8, 8), ll)).all()
    topo.lib().topo_map_xy(p.ctypes.data_as(C.c_void_p), 0, None, None)      # n = 0: nothing is touched


# ---- what needs no device --------------------------------------------------------------------------------------------------------
def test_argument_errors_without_a_context(topo):
    L = topo.lib()
    p = topo.map_params(10.0, 47.0, 0.01, -0.01, 8, 8)
    buf = np.zeros(8 * 8 * 4, np.uint8)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.topo_map_device(None, vp(p), vp(buf), 32, vp(buf), 8) == topo.TOPO_ERR_INVALID
    assert L.topo_map_read(None, vp(p), vp(buf), vp(buf)) == topo.TOPO_ERR_INVALID
    assert not buf.any()
    assert topo.MAP_PARAMS_DTYPE.itemsize == 88 and L.topo_map_rows_per_wave() == ME.rows_per_wave() and 1 <= R <= 64


def test_abi_harness_compiles_links_and_runs(topo, tmp_path):
    exe = str(tmp_path / "map_abi_harness")
    libdir = os.path.dirname(topo.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(os.path.dirname(HERE), "include"), os.path.join(HERE, "map_abi_harness.c"), "-o", exe,
                           "-L", libdir, "-ltopo_hip", "-Wl,-rpath," + libdir, "-lm"])
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(os.path.dirname(__import__("torch").__file__), "lib") + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    out = subprocess.run([exe], env=env, capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    lines = out.stdout.strip().split("\n")
    d = topo.MAP_PARAMS_DTYPE
    assert lines[0].split() == [str(v) for v in (d.itemsize, d.fields["nx"][1], d.fields["sun_direction"][1], d.fields["void_rgba"][1], d.fields["reserved"][1])]
    assert lines[1].split() == [str(v) for v in (topo.MAP_RELIEF, topo.MAP_CONTOURS, topo.MAP_SEEN, topo.MAP_FLAG_TERRAIN, topo.MAP_FLAG_CONTOUR, topo.MAP_FLAG_INDEX,
                                                  topo.MAP_FLAG_SEEN)]
    assert lines[2].split() == ["2", "3", "1", "1"] and lines[3].split() == [str(topo.TOPO_ERR_INVALID)] * 2
