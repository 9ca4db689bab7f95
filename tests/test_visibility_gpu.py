"""Visibility queries on the GPU (topo_visibility_*): k_visibility_observers, k_visibility_grid and k_visibility_list against the
g++ build of the same rule (tests/visibility_emul.py: the traversal and the every-triangle loop) and the numpy reference
(tests/visibility_ref.py) on the cases of tests/visibility_cases.py, the calls' contract, and their side effects (none).

Comparison rule: the classes equal the emulation's and the reference's on every target the reference does not mark ambiguous; the
device and the emulation may differ only on ambiguous targets (device and host sin / cos differ by an ulp)."""
import hashlib

import numpy as np
import pytest

import visibility_cases as VC
import visibility_emul as VE
import visibility_ref as VR
from gpu_support import checked_run, padded_device_output, renderer, strip

pytestmark = pytest.mark.gpu

GRID_CASES = [n for n in sorted(VC.CASES) if n != "observers"]


def _grid(g, obs, grid, h=0.0, pad_cols=0, pad_rows=0):
    """visibility_grid_device into a 0xAB-filled tensor whose rows are pad_cols bytes and whose layers pad_rows rows longer than
    needed: ((observers, ny, nx) classes, the padding bytes)."""
    lon0, lat0, dlon, dlat, nx, ny = grid
    vals, pad = padded_device_output(g, len(obs), ny, nx, 1, lambda p, stride, pitch: g.visibility_grid_device(obs, lon0, lat0, dlon, dlat, nx, ny, p, h, stride, pitch),
                                     pad_cols, pad_rows)
    return vals.reshape(len(obs), ny, nx), pad


def _list_device(g, obs, lonlat, h=0.0, pad=0):
    """visibility_device into a 0xAB-filled tensor whose lists are `pad` bytes longer than needed: ((observers, n) classes, padding)."""
    import torch
    n = len(lonlat)
    p_dev = torch.from_numpy(np.ascontiguousarray(lonlat, np.float64)).cuda()
    out = torch.full((len(obs), n + pad), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    g.visibility_device(obs, p_dev.data_ptr(), n, out.data_ptr(), h, n + pad)
    g.synchronize()
    raw = out.cpu().numpy()
    return np.ascontiguousarray(raw[:, :n]), raw[:, n:]


def _compare(got, emu, ref, amb, what):
    """The comparison rule (module docstring) -> the number of device / emulation differences, all on ambiguous targets."""
    got = got.reshape(emu.shape)
    for o in range(len(emu)):
        bad = np.nonzero((got[o] != emu[o]) & ~amb[o])[0]
        assert len(bad) == 0, f"{what} observer {o}: {len(bad)} unambiguous targets differ from the emulation, first {bad[0]}: {got[o][bad[0]]} vs {emu[o][bad[0]]}"
        bad = np.nonzero((got[o] != ref[o]) & ~amb[o])[0]
        assert len(bad) == 0, f"{what} observer {o}: {len(bad)} unambiguous targets differ from the reference, first {bad[0]}: {got[o][bad[0]]} vs {ref[o][bad[0]]}"
    n = int((got != emu).sum())
    print(f"{what}: {got.size} targets, {int(amb.sum())} ambiguous, {n} device / emulation differences; observer 0 {VC.counts(got[0])}")
    return n


@pytest.mark.parametrize("name", GRID_CASES)
def test_grid_cases(topo, name):
    """Every grid case (nx = 40: a wave with a tail; negative and positive dlat): the grid call, the list call on the same numbers and
    the host read give the same bytes, and those are the emulation's and the reference's."""
    c = VC.case(name)
    ref, amb = VC.reference(name)
    emu, _ = VC.emulation(name)
    g = renderer(topo, c["tiles"], c["order"])
    got, pad = _grid(g, c["obs"], c["grid"], c["h"], pad_cols=3)
    assert (pad == 0xAB).all()
    lst, _ = _list_device(g, c["obs"], c["lonlat"], c["h"])
    read = g.visibility(c["obs"], c["lonlat"], c["h"])
    g.close()
    assert got.reshape(len(c["obs"]), -1).tobytes() == lst.tobytes(), "the list form on the same targets gives the grid's bytes"
    assert read.tobytes() == lst.tobytes(), "topo_visibility_read equals the device call"
    _compare(got, emu, ref, amb, name)


def test_observers_over_a_list(topo):
    c = VC.case("observers")
    ref, amb = VC.reference("observers")
    emu, _ = VC.emulation("observers")
    g = renderer(topo, c["tiles"], c["order"])
    read = g.visibility(c["obs"], c["lonlat"])
    lst, pad = _list_device(g, c["obs"], c["lonlat"], pad=5)
    assert (pad == 0xAB).all(), "the bytes behind a list are left alone"
    assert read.tobytes() == lst.tobytes()
    _compare(read, emu, ref, amb, "observers")
    for o in c["unusable"]:
        assert (read[o] == topo.VIS_NO_OBSERVER).all()
    assert read[8][c["at"][0]] == topo.VIS_VISIBLE and read[9][c["at"][1]] == topo.VIS_VISIBLE
    assert (read[0][c["extra"]] == topo.VIS_NONE).all()
    # no observers and no targets are no-ops; with no tiles an observer above terrain is unusable and one over the sphere sees nothing
    assert g.visibility(c["obs"][:0], c["lonlat"]).shape == (0, len(c["lonlat"])) and g.visibility(c["obs"], c["lonlat"][:0]).shape == (len(c["obs"]), 0)
    g.visibility_device(c["obs"], 0, 0, 0)
    g.visibility_grid_device(c["obs"][:0], 7.0, 46.0, 0.1, 0.1, 4, 4, 0)
    g.close()
    e = topo.TerrainRenderer(64, 48)
    none = e.visibility(c["obs"][[0, 8]], c["lonlat"][:70])
    assert (none[0] == topo.VIS_NONE).all() and (none[1] == topo.VIS_NO_OBSERVER).all()
    e.close()


def test_three_waves_per_row_and_three_observers(topo):
    """The 130 x 34 tile of 3 x 3 ragged blocks under a 130 x 7 grid: a row takes three waves, the last partial, and the waves (21,
    63 with three observers) are no multiple of a workgroup's four.  Three observers in one call, the middle one unusable; layer
    stride and pitch padded, and the padding's sentinel bytes survive."""
    tiles, order, box = VC.tileset("blocks")
    grid = VC.box_grid(box, 130, 7)
    pts = VC.grid_points(grid)
    obs = np.concatenate([VC.centre_observer(box, 300.0), VC.observer_records(2.0, 3.0, 50.0), VC.observer_records(7.113, 46.871, 9000.0, False)])
    ref, amb = VR.visibility(VC.meshes("blocks"), obs, pts)
    emu, eyes, bad = VE.visibility(tiles, order, obs, pts)
    brute, _, bad2 = VE.visibility(tiles, order, obs, pts, brute=True)
    assert bad == 0 and bad2 == 0 and emu.tobytes() == brute.tobytes() and list(eyes["usable"]) == [1, 0, 1]
    assert amb.mean() <= VC.MAX_AMBIGUOUS
    g = renderer(topo, tiles, order)
    got, pad = _grid(g, obs, grid, pad_cols=7, pad_rows=2)
    assert (pad == 0xAB).all(), "bytes between nx and the pitch and between the layers are left alone"
    _compare(got, emu, ref, amb, "130 x 7, three observers")
    assert (got[1] == topo.VIS_NO_OBSERVER).all()
    for k in (topo.VIS_VISIBLE, topo.VIS_AWAY, topo.VIS_HIDDEN):
        assert (got[0] == k).sum() >= 10, VC.counts(got[0])
    one, _ = _grid(g, obs[:1], grid)
    assert one[0].tobytes() == got[0].tobytes(), "an observer's layer does not depend on its company"
    # masts: nothing is AWAY, and the list form agrees
    up, _ = _grid(g, obs, grid, h=25.0)
    emu_up, _, _ = VE.visibility(tiles, order, obs, pts, 25.0)
    ref_up, amb_up = VR.visibility(VC.meshes("blocks"), obs, pts, 25.0)
    g.close()
    assert not (up == topo.VIS_AWAY).any() and amb_up.mean() <= VC.MAX_AMBIGUOUS
    _compare(up, emu_up, ref_up, amb_up, "130 x 7, h = 25")


def test_tile_of_more_than_64_blocks(topo):
    """The `grid` tile, 301 x 250 vertices in 85 raster blocks: the wave takes a tile's blocks in two batches of 64.  A small target
    grid against the emulation's every-triangle loop, and against the reference on every fifth target."""
    tiles, order, box = VC.tileset("grid")
    grid = VC.box_grid(box, 24, 12)
    pts = VC.grid_points(grid)
    obs = VC.centre_observer(box, 250.0)
    brute, _, bad = VE.visibility(tiles, order, obs, pts, brute=True)
    emu, _, bad2 = VE.visibility(tiles, order, obs, pts)
    assert bad == 0 and bad2 == 0 and emu.tobytes() == brute.tobytes()
    sub = np.arange(0, len(pts), 5)
    ref, amb = VR.visibility(VC.meshes("grid"), obs, pts[sub])
    assert not ((ref != brute[:, sub]) & ~amb).any()
    g = renderer(topo, tiles, order)
    got, _ = _grid(g, obs, grid)
    g.close()
    got = got.reshape(1, -1)
    _compare(got[:, sub], brute[:, sub], ref, amb, "grid tile, every fifth target")
    differ = got != brute
    print(f"grid tile: {int(differ.sum())} of {got.size} targets differ from the every-triangle loop")
    assert differ.sum() <= 0.005 * got.size and not (differ[:, sub] & ~amb).any()
    for k in (topo.VIS_VISIBLE, topo.VIS_AWAY, topo.VIS_HIDDEN):
        assert (got[0] == k).sum() >= 2, VC.counts(got[0])


def test_sub_rectangle_of_a_larger_image(topo):
    import torch
    c = VC.case("blocks")
    g = renderer(topo, c["tiles"], c["order"])
    emu, _ = VC.emulation("blocks")
    lon0, lat0, dlon, dlat, nx, ny = c["grid"]
    W, H, c0, r0 = 100, 40, 13, 5
    img = torch.full((H, W), 0xCD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    g.visibility_grid_device(c["obs"], lon0, lat0, dlon, dlat, nx, ny, img.data_ptr() + r0 * W + c0, 0.0, W * H, W)
    g.synchronize()
    raw = img.cpu().numpy()
    full, _ = _grid(g, c["obs"], c["grid"])
    g.close()
    assert raw[r0:r0 + ny, c0:c0 + nx].tobytes() == full[0].tobytes()
    outside = np.ones((H, W), bool)
    outside[r0:r0 + ny, c0:c0 + nx] = False
    assert (raw[outside] == 0xCD).all()
    assert ((full[0].reshape(-1) != emu[0]).sum()) <= int(VC.reference("blocks")[1].sum())


def test_errors(topo):
    import torch
    c = VC.case("blocks")
    g = renderer(topo, c["tiles"], c["order"])
    obs = c["obs"]
    buf = torch.zeros((4096,), dtype=torch.uint8, device="cuda")
    pts = torch.from_numpy(c["lonlat"][:64].copy()).cuda()
    b, p = buf.data_ptr(), pts.data_ptr()
    ok = dict(lon0=7.0, lat0=46.0, dlon=0.1, dlat=0.1, nx=8, ny=4, out_ptr=b, target_height_m=0.0, layer_stride_bytes=32, pitch_bytes=8)
    g.visibility_grid_device(obs, **ok)
    many = np.concatenate([obs] * 65)
    for change in (dict(nx=0), dict(ny=0), dict(out_ptr=0), dict(lon0=np.nan), dict(lat0=np.inf), dict(dlon=-np.inf), dict(dlat=np.nan), dict(pitch_bytes=7),
                   dict(layer_stride_bytes=31), dict(target_height_m=-1.0), dict(target_height_m=1.0e5 + 1.0), dict(target_height_m=np.nan),
                   dict(target_height_m=np.inf), dict(nx=1 << 31, ny=1 << 31, pitch_bytes=1 << 31, layer_stride_bytes=1 << 62),
                   dict(nx=64 * 65536, ny=65536, pitch_bytes=64 * 65536, layer_stride_bytes=64 * 65536 * 65536)):
        with pytest.raises(topo.TopoError) as e:
            g.visibility_grid_device(obs, **dict(ok, **change))
        assert e.value.code == topo.TOPO_ERR_INVALID, change
    with pytest.raises(topo.TopoError) as e:
        g.visibility_grid_device(many, **ok)
    assert e.value.code == topo.TOPO_ERR_INVALID, "more than 64 observers"
    g.visibility_device(obs, p, 64, b)
    for args in ((obs, 0, 64, b), (obs, p, 64, 0), (obs, p + 8, 63, b), (obs, p, 64, b, 0.0, 63), (obs, p, 64, b, -0.5), (obs, p, 64, b, np.nan), (many, p, 64, b)):
        with pytest.raises(topo.TopoError) as e:
            g.visibility_device(*args)
        assert e.value.code == topo.TOPO_ERR_INVALID, args[1:]
    L = topo.lib()
    vp = lambda a: a.ctypes.data_as(topo.C.c_void_p)
    out = np.zeros(64, np.uint8)
    host = c["lonlat"][:64].copy()
    assert L.topo_visibility_read(g._h, 1, None, 64, vp(host), 0.0, vp(out)) == topo.TOPO_ERR_INVALID
    assert L.topo_visibility_read(g._h, 1, vp(obs), 64, None, 0.0, vp(out)) == topo.TOPO_ERR_INVALID
    assert L.topo_visibility_read(g._h, 1, vp(obs), 64, vp(host), 0.0, None) == topo.TOPO_ERR_INVALID
    assert L.topo_visibility_read(g._h, 65, vp(many), 64, vp(host), 0.0, vp(out)) == topo.TOPO_ERR_INVALID
    assert L.topo_visibility_read(g._h, 1, vp(obs), 64, vp(host), 2.0e5, vp(out)) == topo.TOPO_ERR_INVALID
    assert L.topo_visibility_grid_device(g._h, 1, None, 7.0, 46.0, 0.1, 0.1, 8, 4, 0.0, topo.C.c_void_p(b), 32, 8) == topo.TOPO_ERR_INVALID
    g.synchronize()
    g.close()


def test_visibility_calls_change_no_frame_and_no_mask(topo):
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
    obs = np.concatenate([topo.observers(sc.vlon, sc.vlat, 30.0), topo.observers(15.7, 46.4, 3000.0)])
    grid = (15.0, 47.0, 2.0 / 70, -2.0 / 40, 70, 40)
    pts = VC.grid_points(grid)
    out = torch.zeros((2, 40, 70), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    first = None
    for yaw, pitch, fov in ((40, 10, 70), (120, 60, 90), (300, 2, 50)):
        u = sc.uniforms(W, H, yaw, pitch, fov, 0)
        a.update(W, H, u, pu)
        b.update(W, H, u, pu)
        got = b.visibility(obs, pts)
        assert first is None or got.tobytes() == first.tobytes()
        first = got
        ra, rb = a.render(), b.render()
        b.visibility(obs, pts[::3], 12.0)
        b.visibility_grid_device(obs, *grid, out.data_ptr())
        assert_same_frame(ra, rb, f"visibility calls vs none, yaw {yaw}")
        assert a.counters() == b.counters() and a.frame_status() == b.frame_status()
        assert np.array_equal(a.horizon(), b.horizon())
    assert (first[0] == topo.VIS_VISIBLE).sum() > 50 and (first[0] == topo.VIS_AWAY).sum() > 50, VC.counts(first[0])      # (smooth relief: little is hidden)
    b.synchronize()
    assert out.cpu().numpy().reshape(2, -1).tobytes() == first.tobytes()
    masks = [(a.viewshed(*loc), b.viewshed(*loc)) for loc in sc.locs]
    assert any(ma.any() for ma, _ in masks) and all(np.array_equal(ma, mb) for ma, mb in masks)
    # two submissions in flight, the calls queued before the join: the frames are those of a renderer that made none
    sw, sh = 48, 40
    us = sc.panorama(sw, sh, yaw0_deg=25.0)
    p_dev = torch.from_numpy(pts.copy()).cuda()
    lst = torch.zeros((2, len(pts)), dtype=torch.uint8, device="cuda")
    out.zero_()
    torch.cuda.synchronize()
    frames = []
    for r, ask in ((a, False), (b, True)):
        r.set_stream(torch.cuda.current_stream().cuda_stream)
        r.set_pipeline_depth(2)
        keep = [strip(r, us[:2], sw, sh), strip(r, us[2:7], sw, sh)]
        if ask:
            r.visibility_device(obs, p_dev.data_ptr(), len(pts), lst.data_ptr())
            r.visibility_grid_device(obs, *grid, out.data_ptr())
        r.join()
        r.synchronize()
        frames.append([(c.cpu().numpy(), d.cpu().numpy()) for c, d in keep])
    for (ca, da), (cb, db) in zip(frames[0], frames[1]):
        assert np.array_equal(ca, cb) and np.array_equal(da.view(np.uint32), db.view(np.uint32))
    assert lst.cpu().numpy().tobytes() == first.tobytes() and out.cpu().numpy().reshape(2, -1).tobytes() == first.tobytes(), \
        "the classes queued beside frames in flight are the host read's"
    a.close()
    b.close()


def _checked_run(T):
    """The grid on the ridges, blocks, void and polar cases, the 130-wide grid with three observers, the list of the observers case
    and part of the many-block tile -> hash of every output, status."""
    import torch
    h = hashlib.sha256()
    status = 0
    for name in ("ridges_ne", "blocks", "void_nan", "polar", "summit_h30"):
        c = VC.case(name)
        g = renderer(T, c["tiles"], c["order"])
        h.update(_grid(g, c["obs"], c["grid"], c["h"], pad_cols=1)[0].tobytes())
        if name == "blocks":
            box = VC.tileset("blocks")[2]
            obs = np.concatenate([VC.centre_observer(box, 300.0), VC.observer_records(2.0, 3.0, 50.0), VC.observer_records(7.113, 46.871, 9000.0, False)])
            h.update(_grid(g, obs, VC.box_grid(box, 130, 7), pad_cols=2, pad_rows=1)[0].tobytes())
        status |= g.frame_status()["status"]
        g.close()
    c = VC.case("observers")
    g = renderer(T, c["tiles"], c["order"])
    h.update(g.visibility(c["obs"], c["lonlat"]).tobytes())
    status |= g.frame_status()["status"]
    g.close()
    tiles, order, box = VC.tileset("grid")
    g = renderer(T, tiles, order)
    h.update(_grid(g, VC.centre_observer(box, 250.0), VC.box_grid(box, 30, 16))[0].tobytes())
    status |= g.frame_status()["status"]
    g.close()
    torch.cuda.synchronize()
    return {"sha": h.hexdigest()[:24], "status": status}


def test_bounds_checked_build_records_no_out_of_range_index(topo):
    got = checked_run("test_visibility_gpu")      # kStatusBounds: an index a visibility kernel formed was out of range
    assert got["sha"] == _checked_run(topo)["sha"], "the bounds-checked build answers as the product build"
