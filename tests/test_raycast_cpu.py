"""Ray queries without a GPU: the g++ build of topo_los.h (tests/los_emul.py: the traversal k_raycast runs, and the same triangle test
over every triangle) against the independent numpy reference (tests/los_ref.py) on the cases of tests/los_cases.py; the host helper
topo_sun_direction; the record layouts."""
import ctypes as C

import numpy as np
import pytest

import los_cases as LC
import los_emul as LE
import los_ref as LR


@pytest.mark.parametrize("name", sorted(LC.CASES))
def test_emulation_against_reference(name):
    tiles, order, rays, ref = LC.case(name)
    got, bad = LE.raycast(tiles, order, rays)
    assert bad == 0, f"{bad} index checks of the traversal failed"
    assert (ref["kind"] == LR.HIT).sum() >= 0.1 * len(rays) and (ref["kind"] == LR.MISS).sum() >= 0.1 * len(rays), "the case needs hits and misses"
    LR.compare(ref, got, rays, order, tiles[0][0].shape[0], 1e-3, name)


@pytest.mark.parametrize("name", sorted(LC.CASES))
def test_traversal_equals_every_triangle(name):
    """The pruning is conservative: block by block and cell by cell it finds, bit for bit, what the loop over every triangle finds."""
    tiles, order, rays, _ = LC.case(name)
    got, bad = LE.raycast(tiles, order, rays)
    brute, bad_b = LE.raycast(tiles, order, rays, brute=True)
    assert bad == 0 and bad_b == 0
    assert got.tobytes() == brute.tobytes(), f"{int((got != brute).sum())} rays differ, first {np.nonzero(got != brute)[0][:1]}"


def test_blocks_case_covers_its_kinds():
    """The blocks case holds what it is there for: back-face hits, a t_max short of the first hit, a t_min beyond it."""
    _, _, rays, ref = LC.case("blocks")
    hit = ref["kind"] == LR.HIT
    assert (ref["front"][hit] == 0).sum() >= 50 and (ref["front"][hit] == 1).sum() >= 50
    assert ((rays["t_min"] > 0) & hit).sum() >= 5, "some rays find a second hit"
    d = np.linalg.norm(rays["dir"], axis=1)
    assert (np.abs(d - 1.0) > 0.1).sum() >= 100, "non-unit directions"


@pytest.mark.parametrize("name", sorted(LC.BATCH_TILES))
def test_batch_cases_cross_the_batch_boundary(name):
    """k_raycast takes the raster blocks of a tile 64 at a time.  The reference's hits of the tall and grid cases lie on both sides of
    block 64, and meridional rays cross from one batch into the other before and after their first hit: a t_max that shrank in one
    batch is applied in the next."""
    tiles, order, rays, ref = LC.case(name)
    w, h = LC.BATCH_TILES[name]
    assert tiles[0][0].shape == (h, w)
    hit = ref["kind"] == LR.HIT
    cell = ref["tri"] >> 1
    blk = LC.block_of(cell // (h - 1), cell % (h - 1), w)
    n_blocks = -(-(w - 1) // LC.BLOCK_CX) * -(-(h - 1) // LC.BLOCK_CY)
    assert LC.BATCH < n_blocks <= 2 * LC.BATCH and blk[hit].max() < n_blocks
    high, low = int((hit & (blk >= LC.BATCH)).sum()), int((hit & (blk < LC.BATCH)).sum())
    m = LC.meridional(name)
    over_first, over_second = LC.blocks_under(rays[m], order[0][0], order[0][1], w, h)
    second_then_first = int((hit[m] & (blk[m] >= LC.BATCH) & over_first).sum())
    first_then_second = int((hit[m] & (blk[m] < LC.BATCH) & over_second).sum())
    print(f"{name}: {high} hits in blocks >= 64, {low} below; of {len(m)} meridional rays {second_then_first} hit first in the second batch and "
          f"cross the first, {first_then_second} the reverse; {int((hit & (blk == n_blocks - 1)).sum())} hits in the last block")
    assert high >= 20 and low >= 20
    assert second_then_first >= 10 and first_then_second >= 10
    assert ((rays["t_min"] > 0) & hit).sum() >= 5 and (np.abs(np.linalg.norm(rays["dir"], axis=1) - 1.0) > 0.1).sum() >= 100


def test_geographic_cases_hit_every_tile():
    """The cases across the equator and the prime meridian, the antimeridian and the pole have hits in each of their tiles, at
    least 15 % hits and 15 % misses, and the rays over the pole hit on either side of it."""
    for name in ("antimeridian", "antimeridian_south", "origin", "north84", "south85", "polar"):
        tiles, order, rays, ref = LC.case(name)
        hit = ref["kind"] == LR.HIT
        assert hit.mean() >= 0.15 and (ref["kind"] == LR.MISS).mean() >= 0.15, (name, float(hit.mean()))
        assert {int(r) for r in ref["rank"][hit]} == set(range(len(order))), name
    tiles, order, rays, ref = LC.case("polar")
    over = ref[:128]      # the rays over the pole come first
    east = np.array([order[r][1] > 0 for r in over["rank"]]) & (over["kind"] == LR.HIT)
    west = np.array([order[r][1] < 0 for r in over["rank"]]) & (over["kind"] == LR.HIT)
    assert east.sum() >= 20 and west.sum() >= 20, (int(east.sum()), int(west.sum()))


def test_long_case_passes_through_the_gaps():
    tiles, order, rays, ref = LC.case("long")
    assert (ref["kind"][-20:] == LR.MISS).all(), "a ray straight down a gap between two tiles passes"
    assert len({int(r) for r in ref["rank"][ref["kind"] == LR.HIT]}) == 3, "hits in all three tiles"


def test_void_case_reports_what_lies_behind():
    """Rays that hit the clean scene inside a void of the void twin go on to whatever lies behind (or miss)."""
    import void_scenes as VS
    tiles, order, rays, ref = LC.case("void_nan")
    sc = VS.clean_scene("ne_2x2")
    clean = LR.cast(LR.Mesh(LC.scene_tiles(sc)[0]), rays)
    moved = (clean["kind"] == LR.HIT) & ((ref["kind"] != LR.HIT) | (ref["tri"] != clean["tri"]) | (ref["rank"] != clean["rank"]))
    assert moved.sum() >= 0.02 * len(rays), int(moved.sum())
    behind = moved & (ref["kind"] == LR.HIT)
    assert behind.any() and (ref["t"][behind] > clean["t"][behind]).all()
    got, bad = LE.raycast(tiles, order, rays)
    assert bad == 0 and (got["kind"][moved] == ref["kind"][moved]).all()


def test_invalid_rays_leave_their_neighbours_alone():
    tiles, order, rays, ref = LC.case("blocks")
    planted, idx = LC.with_invalid(rays)
    got, _ = LE.raycast(tiles, order, planted)
    clean, _ = LE.raycast(tiles, order, rays)
    assert (got["kind"][idx] == LR.INVALID).all()
    assert (LR.cast(LR.Mesh(tiles), planted[:100])["kind"][idx[idx < 100]] == LR.INVALID).all()
    rest = np.ones(len(rays), bool)
    rest[idx] = False
    assert got[rest].tobytes() == clean[rest].tobytes()
    z = got[idx]
    assert not z["t"].any() and not z["cell_x"].any() and not z["front"].any()


def test_reference_marks_rays_through_vertices_and_edges_ambiguous():
    """The exclusion rule has teeth: a ray aimed exactly at a vertex or along a triangle's plane is marked."""
    tiles, order, _, _ = LC.case("blocks")
    mesh = LR.Mesh(tiles)
    o = LC.ecef(7.5, 46.5, 20000.0)
    at_vertices = LC.make_rays(o, mesh.v0[100:140] - o, 0.0, 2.0)
    r = LR.cast(mesh, at_vertices)
    seen = np.abs(r["t"] - 1.0) < 1e-9      # (some of the vertices lie behind other terrain)
    assert seen.sum() >= 20 and r["ambiguous"][seen].all()
    edge_on = LC.make_rays(mesh.v0[500] - 3.0 * (mesh.v1[500] - mesh.v0[500]), mesh.v1[500] - mesh.v0[500], 0.0, 10.0)
    assert LR.cast(mesh, edge_on)["ambiguous"].all()


def test_sun_direction_against_numpy(topo):
    rng = np.random.default_rng(3)
    for lon, lat, az, el in zip(rng.uniform(-180, 180, 40), rng.uniform(-89, 89, 40), rng.uniform(0, 360, 40), rng.uniform(-20, 90, 40)):
        got = topo.sun_direction(lon, lat, az, el)
        assert np.abs(got - LR.sun_direction(lon, lat, az, el)).max() < 1e-15
        assert abs(np.linalg.norm(got) - 1.0) < 1e-15
    # the frame is that of pixel_angles: straight up, due north, due east at (lon 15, lat 45)
    up = LC.up_at(15.0, 45.0)
    assert np.abs(topo.sun_direction(15.0, 45.0, 0.0, 90.0) - up).max() < 1e-15
    north = topo.sun_direction(15.0, 45.0, 0.0, 0.0)
    east = topo.sun_direction(15.0, 45.0, 90.0, 0.0)
    assert north[2] > 0 and abs(north @ up) < 1e-15 and abs(east[2]) < 1e-15 and np.abs(np.cross(up, east) - north).max() < 1e-15
    # ... and the azimuth / elevation pixel_angles reports for a pixel is the direction through it
    import scenes
    sc = scenes.Scene(24, 1, 1)
    W, H = 64, 48
    u = sc.uniforms(W, H, 70.0, 12.0, 60.0, 0)
    az, el = topo.pixel_angles(u, W, H, [(W / 2.0, H / 2.0)])[0]
    eye = np.asarray(sc.eye, np.float64)
    lon, lat = np.degrees(np.arctan2(eye[1], eye[0])), np.degrees(np.arcsin(eye[2] / np.linalg.norm(eye)))
    fwd = LC.RC.camera_basis(eye, np.radians(70.0), np.radians(12.0))[0]
    assert np.abs(topo.sun_direction(lon, lat, az, el) - fwd).max() < 1e-5      # (the f32 matrix of the uniforms)


def test_record_layouts(topo):
    class Ray(C.Structure):
        _fields_ = [("origin", C.c_double * 3), ("dir", C.c_double * 3), ("t_min", C.c_double), ("t_max", C.c_double)]

    class RayHit(C.Structure):
        _fields_ = [("t", C.c_double), ("lon_deg", C.c_double), ("lat_deg", C.c_double), ("height_m", C.c_float), ("kind", C.c_int32),
                    ("tile_lat_deg", C.c_int32), ("tile_lon_deg", C.c_int32), ("cell_x", C.c_uint32), ("cell_y", C.c_uint32), ("tri", C.c_uint32),
                    ("front", C.c_uint32), ("w1", C.c_float), ("w2", C.c_float)]

    assert C.sizeof(Ray) == 64 == topo.RAY_DTYPE.itemsize and C.sizeof(RayHit) == 64 == topo.RAY_HIT_DTYPE.itemsize
    for name, _ in RayHit._fields_:
        assert getattr(RayHit, name).offset == topo.RAY_HIT_DTYPE.fields[name][1], name
    for name, _ in Ray._fields_:
        assert getattr(Ray, name).offset == topo.RAY_DTYPE.fields[name][1], name
    header = open(topo.HEADER_PATH).read()
    assert "} topo_ray_hit;" in header and "int topo_raycast_device(" in header
    r = topo.rays([1.0, 2.0, 3.0], [[0.0, 0.0, 1.0], [0.0, 1.0, 0.0]], 0.5, [1.0, 2.0])
    assert r.dtype == topo.RAY_DTYPE and len(r) == 2 and r["origin"][1, 2] == 3.0 and r["t_max"][1] == 2.0 and r["t_min"][0] == 0.5


@pytest.mark.parametrize("name", sorted(LC.RIDGES))
def test_sunlit_emulation_against_reference(orc, name):
    """The sunlit layer composed from the g++ builds of topo_ground.h and topo_los.h against the numpy reference, on frames of the
    oracle.  Each class holds at least a tenth of the terrain pixels: the test has teeth."""
    sc, W, H, u, tiles, order, sun, ref, amb, emu = LC.sunlit_case(name, orc)
    terrain = ref != LR.NONE
    counts = {c: int((ref == c).sum()) for c in (LR.LIT, LR.AWAY, LR.SHADOW)}
    print(f"{name}: terrain {int(terrain.sum())} of {W * H}, lit {counts[LR.LIT]}, away {counts[LR.AWAY]}, shadow {counts[LR.SHADOW]}, ambiguous {int(amb.sum())}")
    assert terrain.sum() > 0.25 * W * H
    for c, k in counts.items():
        assert k >= 0.1 * terrain.sum(), (c, counts)
    assert amb.sum() <= 0.005 * W * H
    bad = np.argwhere((emu != ref) & ~amb)
    assert len(bad) == 0, f"{len(bad)} pixels differ, first {tuple(bad[0])}: {emu[tuple(bad[0])]} vs {ref[tuple(bad[0])]}"
