"""Surface queries on the GPU (topo_surface_*, topo_profile_*): k_surface, k_surface_grid and k_profile against the numpy reference
(tests/surface_ref.py) and the g++ build of the same lookup (tests/surface_emul.py) on the cases of tests/surface_cases.py, the
calls' contract, their agreement with the ray and ground queries, and their side effects (none)."""
import hashlib

import numpy as np
import pytest

import los_cases as LC
import surface_cases as SC
import surface_emul as SE
import surface_ref as SR
from gpu_support import checked_run, padded_device_output, renderer, strip

pytestmark = pytest.mark.gpu


def _against_emulation(got, emu, what, tri_ambiguous, kind_ambiguous):
    """The comparison rule against the g++ build: kind outside kind-ambiguous points; tile, cell and triangle outside
    triangle-ambiguous points; the height of every point both call TERRAIN within 1e-4 m (the bound test_raycast_gpu.py derives for
    device against host sin / cos); slope within 1e-6 degrees and aspect within 1e-4 degrees where the slope is > 1 degree, the
    record's f32 against the emulation's f64 as SC.check_slope_aspect says."""
    keep = ~kind_ambiguous
    bad = np.nonzero(keep & (got["kind"] != emu["kind"]))[0]
    assert len(bad) == 0, f"{what}: kind differs from the emulation for {len(bad)} points, first {bad[0]}: {got[bad[0]]} vs {emu[bad[0]]}"
    both = (got["kind"] == SR.TERRAIN) & (emu["kind"] == SR.TERRAIN)
    err = np.abs(got["height_m"] - emu["height_m"])[both]
    print(f"{what}: largest height difference to the emulation {err.max():.3e} m")
    assert err.max() <= 1e-4, f"{what}: {err.max():.3e} m"
    t = both & keep & ~tri_ambiguous
    for f in ("tile_lat_deg", "tile_lon_deg", "cell_x", "cell_y", "tri"):
        bad = np.nonzero(t & (got[f] != emu[f]))[0]
        assert len(bad) == 0, f"{what}: {f} differs from the emulation for {len(bad)} points, first {bad[0]}: {got[bad[0]]} vs {emu[bad[0]]}"
    SC.check_slope_aspect(got["slope_deg"][t], got["aspect_deg"][t], emu["slope_deg"][t], emu["aspect_deg"][t], True, what)
    assert np.abs(got["w1"][t] - emu["w1"][t]).max() < 1e-5 and np.abs(got["w2"][t] - emu["w2"][t]).max() < 1e-5
    z = got[got["kind"] != SR.TERRAIN]
    assert not z["height_m"].any() and not z["slope_deg"].any() and not z["cell_x"].any() and not z["w1"].any() and not z["tile_lat_deg"].any(), \
        "every other field of a record that is not TERRAIN is 0"


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_cases(topo, name):
    tiles, order, pts, label = SC.case(name)
    g = renderer(topo, tiles, order)
    got = g.surface(pts)
    g.close()
    ref = SC.reference(name)
    SC.compare_reference(ref, got, order, tiles[0][0].shape[0], label, name, f32_record=True)
    emu, bad = SC.emulation(name)
    assert bad == 0
    _against_emulation(got, emu, name, ref["tri_ambiguous"], ref["kind_ambiguous"])
    assert (got["kind"][label == SC.GAP] == topo.SURFACE_NONE).all(), "points in a gap have no terrain"
    if name == "blocks":      # exact DEM posts, the border's included, have terrain
        assert (got["kind"][label == SC.VERTEX] == topo.SURFACE_TERRAIN).all()


def test_full_size_tile_against_the_emulation(topo):
    """One 1200 x 1200 tile, 20 000 random points, against the g++ build only.  Without a reference the ambiguous points are
    taken from the emulation's own weights (within 1e-6 of an edge of the winning triangle) and from the tile's border (within
    1e-5 of a cell)."""
    tiles, order, pts = SC.big_tile()
    emu, bad = SE.surface(tiles, order, pts)
    assert bad == 0
    g = renderer(topo, tiles, order)
    got = g.surface(pts)
    g.close()
    w0 = 1.0 - emu["w1"] - emu["w2"]
    tri_amb = (emu["kind"] == SR.TERRAIN) & (np.minimum(np.minimum(emu["w1"], emu["w2"]), w0) < 1e-6)
    fx, fy = (pts[:, 0] - 7.0) * 1200.0, (47.0 - pts[:, 1]) * 1200.0
    kind_amb = (np.minimum(np.abs(fx), np.abs(fx - 1199.0)) < 1e-5) | (np.minimum(np.abs(fy), np.abs(fy - 1199.0)) < 1e-5)
    assert (tri_amb | kind_amb).mean() <= SC.MAX_AMBIGUOUS
    assert 0.85 * len(pts) < (emu["kind"] == SR.TERRAIN).sum() < len(pts)
    _against_emulation(got, emu, "one 1200 x 1200 tile", tri_amb, kind_amb)


def test_invalid_points_and_the_device_variant(topo):
    import torch
    tiles, order, pts, label = SC.case("blocks")
    pts = pts[label == SC.RANDOM]
    g = renderer(topo, tiles, order)
    planted, idx = SC.with_invalid(pts)
    clean, got = g.surface(pts), g.surface(planted)
    assert (got["kind"][idx] == topo.SURFACE_INVALID).all()
    bad = got[idx]
    assert not bad["height_m"].any() and not bad["slope_deg"].any() and not bad["aspect_deg"].any() and not bad["tile_lat_deg"].any() \
        and not bad["cell_x"].any() and not bad["cell_y"].any() and not bad["tri"].any() and not bad["w1"].any() and not bad["w2"].any()
    rest = np.ones(len(pts), bool)
    rest[idx] = False
    assert got[rest].tobytes() == clean[rest].tobytes(), "the neighbours of an invalid point are untouched"
    # latitude +-90 is valid, and any finite longitude wraps
    poles = g.surface([[12.0, 90.0], [12.0, -90.0], [7.5 + 720.0, 46.5], [7.5, 46.5]])
    assert (poles["kind"][:2] == topo.SURFACE_NONE).all() and poles["kind"][2] == topo.SURFACE_TERRAIN
    assert abs(poles["height_m"][2] - poles["height_m"][3]) < 1e-4 and poles["cell_x"][2] == poles["cell_x"][3]
    # the device variant: the same bytes; an odd count; bytes behind the records left alone
    n = len(planted) - 3
    p_dev = torch.from_numpy(planted.copy()).cuda()
    out = torch.full((n + 2, 48), 0xAB, dtype=torch.uint8, device="cuda")
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    g.surface_device(p_dev.data_ptr(), out.data_ptr(), n)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert o[:n].tobytes() == got[:n].tobytes() and (o[n:] == 0xAB).all()
    # n = 0 is a no-op; null and misaligned pointers are refused
    g.surface_device(0, 0, 0)
    assert len(g.surface(pts[:0])) == 0
    L = topo.lib()
    vp = lambda a: a.ctypes.data_as(topo.C.c_void_p)
    one = np.zeros(1, topo.SURFACE_DTYPE)
    assert L.topo_surface_read(g._h, 1, None, vp(one)) == topo.TOPO_ERR_INVALID
    assert L.topo_surface_read(g._h, 1, vp(pts), None) == topo.TOPO_ERR_INVALID
    for a, b in ((0, out.data_ptr()), (p_dev.data_ptr(), 0), (p_dev.data_ptr() + 8, out.data_ptr()), (p_dev.data_ptr(), out.data_ptr() + 8)):
        with pytest.raises(topo.TopoError) as e:
            g.surface_device(a, b, 4)
        assert e.value.code == topo.TOPO_ERR_INVALID
    g.close()


def test_no_tiles_and_tile_set_changes(topo):
    tiles, order, pts, label = SC.case("long")
    ref = SC.reference("long")
    g = topo.TerrainRenderer(64, 48)
    planted, idx = SC.with_invalid(pts)
    got = g.surface(planted)
    want = np.zeros(len(pts), np.int32)
    want[idx] = topo.SURFACE_INVALID
    assert (got["kind"] == want).all(), "with no tiles every valid point is NONE"
    for (lat, lon), t in zip(order, tiles):
        g.add_terrain(lat, lon, *t)
    th = tiles[0][0].shape[0]
    SC.compare_reference(ref, g.surface(pts), order, th, label, "long", f32_record=True)
    # the middle tile unloaded: the tables follow the tile set
    g.unload_terrain(*order[1])
    rest_t, rest_o = [tiles[0], tiles[2]], [order[0], order[2]]
    sub = slice(0, 600)
    ref2 = SR.surface(SR.Mesh(rest_t), pts[sub])
    assert (ref2["kind"] != ref["kind"][sub]).sum() > 100
    got2 = g.surface(pts)
    SC.compare_reference(ref2, got2[sub], rest_o, th, label[sub], "long without its middle tile", f32_record=True)
    assert not (got2["tile_lon_deg"][got2["kind"] == topo.SURFACE_TERRAIN] == order[1][1]).any()
    g.add_terrain(order[1][0], order[1][1], *tiles[1])
    SC.compare_reference(ref, g.surface(pts), order, th, label, "long again", f32_record=True)
    g.close()


@pytest.mark.parametrize("name", ["blocks", "antimeridian", "polar"])
def test_consistent_with_the_ray_calls(topo, name):
    """For the points the reference does not call ambiguous, the nadir ray from 20 km names the same tile, cell and triangle, and
    |20000 - t - height| <= 1e-4 m."""
    tiles, order, pts, label = SC.case(name)
    ref = SC.reference(name)
    keep = ~ref["tri_ambiguous"] & ~ref["kind_ambiguous"] & (label == SC.RANDOM)
    pts = pts[keep]
    g = renderer(topo, tiles, order)
    got = g.surface(pts)
    up = SR.direction(pts[:, 0], pts[:, 1])
    hit = g.raycast(topo.rays((SR.R0 + 20000.0) * up, -up, 0.0, 1.0e6))
    g.close()
    t = got["kind"] == topo.SURFACE_TERRAIN
    assert t.sum() > 0.5 * len(pts)
    assert np.array_equal(hit["kind"] == topo.RAY_HIT, t)
    for f in ("tile_lat_deg", "tile_lon_deg", "cell_x", "cell_y", "tri"):
        assert np.array_equal(hit[f][t], got[f][t]), f
    err = np.abs(20000.0 - hit["t"][t] - got["height_m"][t])
    print(f"{name}: largest |20000 - t - height| {err.max():.3e} m")
    assert err.max() <= 1e-4


def test_consistent_with_the_ground_queries(topo):
    """tests/test_ray_check_cpu.py's ne_2x2 scene: for the TERRAIN records of a rendered frame whose three weights are >= 0, the
    surface under the record's longitude and latitude is the record's tile, cell and triangle, at the record's height to 1e-3 m
    (the record's height is an f32)."""
    from scenes import Scene, relief
    sc = Scene(24, 2, 2, lat0=45, lon0=15, eye_dh=4000.0, height_fn=relief)
    W, H = 96, 64
    g = topo.TerrainRenderer(W, H)
    sc.load(g)
    g.update(W, H, sc.uniforms(W, H, 30.0, 25.0, 60.0, 1), topo.post_uniforms(W, H))
    g.render()
    ys, xs = np.mgrid[0:H, 0:W]
    rec = g.ground(np.stack([np.zeros(W * H, np.int64), xs.reshape(-1), ys.reshape(-1)], axis=1))
    w0 = 1.0 - rec["w1"].astype(np.float64) - rec["w2"]
    rec = rec[(rec["kind"] == topo.GROUND_TERRAIN) & (rec["w1"] >= 0) & (rec["w2"] >= 0) & (w0 >= 0)]
    assert len(rec) > 0.2 * W * H
    got = g.surface(np.stack([rec["lon_deg"], rec["lat_deg"]], axis=1))
    g.close()
    assert (got["kind"] == topo.SURFACE_TERRAIN).all()
    for f in ("tile_lat_deg", "tile_lon_deg", "cell_x", "cell_y", "tri"):
        bad = np.nonzero(got[f] != rec[f])[0]
        assert len(bad) == 0, f"{f} differs for {len(bad)} of {len(rec)} records, first {rec[bad[0]]} vs {got[bad[0]]}"
    err = np.abs(got["height_m"] - rec["height_m"].astype(np.float64))
    print(f"ground consistency: {len(rec)} records, largest height difference {err.max():.3e} m")
    assert err.max() <= 1e-3


def _grid(g, lon0, lat0, dlon, dlat, nx, ny, pad_px=0):
    """surface_grid_device into a tensor whose rows are pad_px floats longer than needed: ((ny, nx) f32, the padding bytes)."""
    vals, pad = padded_device_output(g, 1, ny, nx, 4, lambda p, stride, pitch: g.surface_grid_device(lon0, lat0, dlon, dlat, nx, ny, p, pitch), pad_px)
    return vals.view(np.float32).reshape(ny, nx), pad


def _grid_expected(g, T, lon0, lat0, dlon, dlat, nx, ny):
    """float32(list height) on the same lon0 + c * dlon, lat0 + r * dlat computed in numpy; NaN where the list has no terrain."""
    lon = np.float64(lon0) + np.arange(nx, dtype=np.float64) * np.float64(dlon)
    lat = np.float64(lat0) + np.arange(ny, dtype=np.float64) * np.float64(dlat)
    rec = g.surface(np.stack(np.broadcast_arrays(lon[None, :], lat[:, None]), axis=-1).reshape(-1, 2)).reshape(ny, nx)
    return np.where(rec["kind"] == T.SURFACE_TERRAIN, rec["height_m"].astype(np.float32), np.float32(np.nan)), rec


def test_grid(topo):
    import torch
    tiles, order, _, _ = SC.case("blocks")
    g = renderer(topo, tiles, order)
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    # 150 x 37 (nx no multiple of 64) over the tile and a margin, north to south (negative dlat), rows padded by 5 floats
    nx, ny = 150, 37
    lon0, lat0, dlon, dlat = 6.99, 47.012, 1.013 / nx, -1.021 / ny
    got, pad = _grid(g, lon0, lat0, dlon, dlat, nx, ny, pad_px=5)
    want, rec = _grid_expected(g, topo, lon0, lat0, dlon, dlat, nx, ny)
    assert (pad == 0xAB).all(), "bytes between nx and the pitch are left alone"
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "the grid is float32(list height), NaN elsewhere, bit for bit"
    terrain = rec["kind"] == topo.SURFACE_TERRAIN
    assert 0.5 < terrain.mean() < 0.99 and np.isnan(got[~terrain]).all()
    # rows beyond the pole are invalid points: NaN
    polar, _ = _grid(g, 7.5, 89.0, 0.0, 0.5, 3, 5)
    assert np.isnan(polar).all()
    # a sub-rectangle of a larger image: only it changes
    W, H, c0, r0, sx, sy = 200, 50, 23, 7, 70, 20
    img = torch.full((H, W * 4), 0xCD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    g.surface_grid_device(7.2, 46.9, 0.004, -0.01, sx, sy, img.data_ptr() + r0 * W * 4 + c0 * 4, W * 4)
    g.synchronize()
    raw = img.cpu().numpy().view(np.float32)
    sub_want, _ = _grid_expected(g, topo, 7.2, 46.9, 0.004, -0.01, sx, sy)
    assert np.array_equal(raw[r0:r0 + sy, c0:c0 + sx].view(np.uint32), sub_want.view(np.uint32)) and not np.isnan(sub_want).any()
    outside = np.ones((H, W), bool)
    outside[r0:r0 + sy, c0:c0 + sx] = False
    assert (raw.view(np.uint32)[outside] == 0xCDCDCDCD).all()
    # errors
    buf = torch.zeros((64,), dtype=torch.float32, device="cuda")
    for args in ((7.0, 46.0, 0.1, 0.1, 0, 4, buf.data_ptr(), 16), (7.0, 46.0, 0.1, 0.1, 4, 0, buf.data_ptr(), 16), (7.0, 46.0, 0.1, 0.1, 4, 4, 0, 16),
                 (np.nan, 46.0, 0.1, 0.1, 4, 4, buf.data_ptr(), 16), (7.0, 46.0, np.inf, 0.1, 4, 4, buf.data_ptr(), 16), (7.0, 46.0, 0.1, 0.1, 4, 4, buf.data_ptr() + 2, 16),
                 (7.0, 46.0, 0.1, 0.1, 4, 4, buf.data_ptr(), 12), (7.0, 46.0, 0.1, 0.1, 4, 4, buf.data_ptr(), 18)):
        with pytest.raises(topo.TopoError) as e:
            g.surface_grid_device(*args)
        assert e.value.code == topo.TOPO_ERR_INVALID, args
    g.close()


@pytest.mark.parametrize("m", [2, 100, 257])
def test_profile(topo, m):
    """Heights over the `long` mosaic stay below 2048 m, where an f32 sample is within 6.1e-5 m of its f64 value: the samples'
    terrain is held to 1e-4 m of the list answer.  The lines reach 7 km (4.9e-4 m steps) and are held to 1e-3 m."""
    import torch
    tiles, order, _, _ = SC.case("long")
    segs, invalid = SC.profile_segments()
    n = len(segs)
    valid = np.ones(n, bool)
    valid[invalid] = False
    g = renderer(topo, tiles, order)
    summary, samples = g.profile(segs, m)
    # the summary is the reduction of the device's own samples, exactly; ties go to the first sample
    SC.check_summaries(summary, samples, invalid, f"m = {m}")
    assert summary["n_terrain"][n - 4] == 0 and summary["min_sample"][n - 5] == 0 and summary["n_terrain"][n - 5] == m
    if m >= 100:
        assert 0 < summary["n_terrain"][6] < m, "samples beyond the mosaic are counted out"
        assert summary["min_clearance_m"][7] < -100.0
    # a null samples pointer: the same summaries
    only, none = g.profile(segs, m, samples=False)
    assert none is None and only.tobytes() == summary.tobytes()
    # the emulation: the same kinds; the same samples have terrain (and so the same counts) unless the reference calls a sample
    # ambiguous; terrain within 1e-4 m and line within 1e-3 m of the emulation's f32 samples
    esum, esmp, bad = SE.profile(tiles, order, segs, m)
    assert bad == 0 and np.array_equal(esum["kind"], summary["kind"])
    terrain, _, amb = SR.profile(SR.Mesh(tiles), segs[valid], m)
    g_has, e_has = ~np.isnan(samples[valid][..., 0]), ~np.isnan(esmp[valid][..., 0])
    assert ((g_has == e_has) | amb).all()
    clear = ~amb.any(axis=1)
    assert np.array_equal(esum["n_terrain"][valid][clear], summary["n_terrain"][valid][clear])
    d = np.abs(samples[valid].astype(np.float64) - esmp[valid].astype(np.float64))
    assert d[..., 0][g_has & e_has].max() <= 1e-4 and d[..., 1].max() <= 1e-3
    # the samples against the list answers at the samples' longitude and latitude
    p, line = SR.sample_points(segs[valid], m)
    lst = g.surface(SC.lonlat_of(p.reshape(-1, 3))).reshape(p.shape[:2])
    got = samples[valid].astype(np.float64)
    has = ~np.isnan(got[..., 0])
    assert ((has == (lst["kind"] == topo.SURFACE_TERRAIN)) | amb).all()
    both = has & (lst["kind"] == topo.SURFACE_TERRAIN)
    err = np.abs(got[..., 0] - lst["height_m"])[both]
    print(f"m = {m}: largest |sample - list height| {err.max():.3e} m")
    assert err.max() <= 1e-4
    assert np.abs(got[..., 1] - line).max() <= 1e-3
    # clearances against the reference
    ref_c = line - terrain
    got_c = (samples[valid][..., 1] - samples[valid][..., 0]).astype(np.float64)
    k = has & ~np.isnan(terrain)
    assert ((has == ~np.isnan(terrain)) | amb).all()
    cerr = np.abs(got_c - ref_c)[k]
    print(f"m = {m}: largest clearance difference to the reference {cerr.max():.3e} m")
    assert cerr.max() <= 1e-3
    # a segment that starts above ground and dips under it at a sample is a ray hit no later than that sample
    s = summary[valid]
    start_above = ~np.isnan(samples[valid][:, 0, 0]) & (got_c[:, 0] > 0)
    under = start_above & (s["min_clearance_m"] < -1e-3)
    hit = g.raycast(segs[valid][under])
    sv = segs[valid][under]
    t_k = sv["t_min"] + (sv["t_max"] - sv["t_min"]) * (s["min_sample"][under].astype(np.float64) / (m - 1))
    assert (hit["kind"] == topo.RAY_HIT).all() and (hit["t"] <= t_k).all()
    if m >= 100:
        assert under.sum() >= 1
    # the device variant with a padded stride: the same bytes, the bytes behind a segment's samples left alone
    stride = 8 * m + 24
    s_dev = torch.from_numpy(segs.view(np.uint8).reshape(-1, 64).copy()).cuda()
    smp_dev = torch.full((n, stride), 0xAB, dtype=torch.uint8, device="cuda")
    sum_dev = torch.full((n + 1, 16), 0xAB, dtype=torch.uint8, device="cuda")
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    g.profile_device(s_dev.data_ptr(), n, m, sum_dev.data_ptr(), smp_dev.data_ptr(), stride)
    torch.cuda.synchronize()
    raw = smp_dev.cpu().numpy()
    assert raw[:, :8 * m].tobytes() == samples.tobytes() and (raw[:, 8 * m:] == 0xAB).all()
    so = sum_dev.cpu().numpy()
    assert so[:n].tobytes() == summary.tobytes() and (so[n:] == 0xAB).all()
    g.close()


def test_profile_errors(topo):
    import torch
    tiles, order, _, _ = SC.case("long")
    segs, _ = SC.profile_segments()
    g = renderer(topo, tiles, order)
    s_dev = torch.from_numpy(segs.view(np.uint8).reshape(-1, 64).copy()).cuda()
    smp = torch.zeros((len(segs), 8 * 16 + 8), dtype=torch.uint8, device="cuda")
    out = torch.zeros((len(segs), 16), dtype=torch.uint8, device="cuda")
    sp, mp, op = s_dev.data_ptr(), smp.data_ptr(), out.data_ptr()
    g.profile_device(sp, 4, 16, op, mp, 8 * 16)
    g.profile_device(0, 0, 16, 0)      # n = 0 is a no-op
    for args in ((sp, 4, 1, op, mp, 128), (sp, 4, 65537, op, 0, 0), (sp, 40000, 65536, op, 0, 0), (0, 4, 16, op, mp, 128), (sp, 4, 16, 0, mp, 128),
                 (sp + 8, 4, 16, op, mp, 128), (sp, 4, 16, op + 8, mp, 128), (sp, 4, 16, op, mp + 4, 128), (sp, 4, 16, op, mp, 120), (sp, 4, 16, op, mp, 132)):
        with pytest.raises(topo.TopoError) as e:
            g.profile_device(*args)
        assert e.value.code == topo.TOPO_ERR_INVALID, args
    L = topo.lib()
    vp = lambda a: a.ctypes.data_as(topo.C.c_void_p)
    one = np.zeros(1, topo.PROFILE_SUMMARY_DTYPE)
    assert L.topo_profile_read(g._h, 1, None, 4, None, vp(one)) == topo.TOPO_ERR_INVALID
    assert L.topo_profile_read(g._h, 1, vp(segs), 4, None, None) == topo.TOPO_ERR_INVALID
    assert L.topo_profile_read(g._h, 1, vp(segs), 1, None, vp(one)) == topo.TOPO_ERR_INVALID
    g.synchronize()
    g.close()


def test_surface_calls_change_no_frame_and_no_mask(topo):
    import torch
    from scenes import Scene, assert_same_frame
    sc = Scene(96, 2, 2, eye_dh=100.0)
    W, H = 256, 160
    a, b = topo.TerrainRenderer(W, H), topo.TerrainRenderer(W, H)
    sc.load(a)
    sc.load(b)
    a.viewshed_enable(True)
    b.viewshed_enable(True)
    pu = topo.post_uniforms(W, H)
    pts = SC.random_points(15.0, 17.0, 45.0, 47.0, 700, 61)
    eye = np.asarray(sc.eye, np.float64)
    far = LC.ecef(sc.vlon + 0.6 * np.cos(np.arange(12.0)), sc.vlat + 0.6 * np.sin(np.arange(12.0)), 1500.0)
    segs = topo.rays(eye, far - eye, 0.0, 1.0)
    grid = torch.zeros((40, 64), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    first = None
    for yaw, pitch, fov in ((40, 10, 70), (120, 60, 90), (300, 2, 50)):
        u = sc.uniforms(W, H, yaw, pitch, fov, 0)
        a.update(W, H, u, pu)
        b.update(W, H, u, pu)
        got = b.surface(pts)
        assert first is None or got.tobytes() == first.tobytes()
        first = got
        ra, rb = a.render(), b.render()
        b.surface(pts[::3])
        b.surface_grid_device(15.0, 47.0, 2.0 / 64, -2.0 / 40, 64, 40, grid.data_ptr())
        b.profile(segs, 50)
        assert_same_frame(ra, rb, f"surface calls vs none, yaw {yaw}")
        assert a.counters() == b.counters() and a.frame_status() == b.frame_status()
        assert np.array_equal(a.horizon(), b.horizon())
    assert (first["kind"] == topo.SURFACE_TERRAIN).sum() > 500
    b.synchronize()
    assert not np.isnan(grid.cpu().numpy()).all()
    masks = [(a.viewshed(*loc), b.viewshed(*loc)) for loc in sc.locs]
    assert any(ma.any() for ma, _ in masks) and all(np.array_equal(ma, mb) for ma, mb in masks)
    # two submissions in flight, the calls queued before the join: the frames are those of a renderer that made none
    sw, sh = 48, 40
    us = sc.panorama(sw, sh, yaw0_deg=25.0)
    p_dev = torch.from_numpy(pts.copy()).cuda()
    rec_dev = torch.zeros((len(pts), 48), dtype=torch.uint8, device="cuda")
    s_dev = torch.from_numpy(segs.view(np.uint8).reshape(-1, 64).copy()).cuda()
    sum_dev = torch.zeros((len(segs), 16), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    frames = []
    for r, ask in ((a, False), (b, True)):
        r.set_stream(torch.cuda.current_stream().cuda_stream)
        r.set_pipeline_depth(2)
        keep = [strip(r, us[:2], sw, sh), strip(r, us[2:7], sw, sh)]
        if ask:
            r.surface_device(p_dev.data_ptr(), rec_dev.data_ptr(), len(pts))
            r.profile_device(s_dev.data_ptr(), len(segs), 50, sum_dev.data_ptr())
            r.surface_grid_device(15.0, 47.0, 2.0 / 64, -2.0 / 40, 64, 40, grid.data_ptr())
        r.join()
        r.synchronize()
        frames.append([(c.cpu().numpy(), d.cpu().numpy()) for c, d in keep])
    for (ca, da), (cb, db) in zip(frames[0], frames[1]):
        assert np.array_equal(ca, cb) and np.array_equal(da.view(np.uint32), db.view(np.uint32))
    assert rec_dev.cpu().numpy().tobytes() == first.tobytes(), "the records queued beside frames in flight are the list call's"
    a.close()
    b.close()


def _checked_run(T):
    """The list on the blocks case (invalid points planted), the polar case and part of the full-size tile, a grid and the profiles
    -> hash of every output, status."""
    import torch
    h = hashlib.sha256()
    status = 0
    for name in ("blocks", "polar", "void_pinf"):
        tiles, order, pts, _ = SC.case(name)
        g = renderer(T, tiles, order)
        h.update(g.surface(SC.with_invalid(pts)[0]).tobytes())
        if name == "blocks":
            h.update(_grid(g, 6.99, 47.012, 1.013 / 150, -1.021 / 37, 150, 37, pad_px=1)[0].tobytes())
        status |= g.frame_status()["status"]
        g.close()
    tiles, order, pts = SC.big_tile()
    g = renderer(T, tiles, order)
    h.update(g.surface(pts[::10]).tobytes())
    status |= g.frame_status()["status"]
    g.close()
    tiles, order, _, _ = SC.case("long")
    g = renderer(T, tiles, order)
    for m in (2, 257):
        summary, samples = g.profile(SC.profile_segments()[0], m)
        h.update(summary.tobytes())
        h.update(samples.tobytes())
    status |= g.frame_status()["status"]
    g.close()
    torch.cuda.synchronize()
    return {"sha": h.hexdigest()[:24], "status": status}


def test_bounds_checked_build_records_no_out_of_range_index(topo):
    got = checked_run("test_surface_gpu")      # kStatusBounds: an index a surface kernel formed was out of range
    assert got["sha"] == _checked_run(topo)["sha"], "the bounds-checked build answers as the product build"
