"""Sun exposure queries on the GPU (topo_sun_exposure_*): k_sun_exposure_grid and k_sun_exposure_list against the g++ build of the
same rule (tests/sun_emul.py: the traversal and the every-triangle loop) and the numpy reference (tests/sun_ref.py) on the cases of
tests/sun_cases.py, the calls' contract, and their side effects (none).

Comparison rule: the device reports two bits per (target, sun) -- LIT, cast SHADOW, or neither (NONE, AWAY, NIGHT).  They equal the
emulation's and the reference's on every pair the reference does not mark ambiguous; the device and the emulation may differ only on
ambiguous pairs (device and host sin / cos differ by an ulp).  The exposure is a quiet NaN exactly where the reference has no terrain
(on targets whose lookup is not ambiguous) and within 1 f32 ulp of the reference on terrain targets with no ambiguous pair: the sum has
non-negative f64 terms that are each good to a few f64 ulps, and it is rounded once."""
import hashlib

import numpy as np
import pytest

import sun_cases as SC
import sun_emul as SE
import sun_ref as SNR
import visibility_cases as VC
from gpu_support import checked_run, renderer, strip

pytestmark = pytest.mark.gpu

FILL = 0xAB


def _states(lit, shadow, n_suns):
    """(n) masks -> (suns, n) uint8: 1 LIT, 3 SHADOW, 0 neither (the classes with AWAY, NIGHT and NONE folded into 0)."""
    k = np.arange(n_suns, dtype=np.uint64)[:, None]
    one = np.uint64(1)
    return (((lit.reshape(-1)[None, :] >> k) & one) * SNR.LIT + ((shadow.reshape(-1)[None, :] >> k) & one) * SNR.SHADOW).astype(np.uint8)


def _fold(cls):
    return np.where((cls == SNR.LIT) | (cls == SNR.SHADOW), cls, 0).astype(np.uint8)


def _grid(g, suns, grid, pad_cols=0, want="lse"):
    """sun_exposure_grid_device into 0xAB-filled tensors whose rows are pad_cols entries longer than needed -> (lit (ny, nx) u64 or
    None, shadow, exposure (ny, nx) f32 or None, the padding bytes of all three)."""
    import torch
    lon0, lat0, dlon, dlat, nx, ny = grid
    bufs = {k: torch.full((ny, (nx + pad_cols) * (4 if k == "e" else 8)), FILL, dtype=torch.uint8, device="cuda") for k in want}
    ptr = lambda k: bufs[k].data_ptr() if k in bufs else 0
    torch.cuda.synchronize()
    g.sun_exposure_grid_device(suns, lon0, lat0, dlon, dlat, nx, ny, ptr("l"), ptr("s"), ptr("e"), 8 * (nx + pad_cols), 4 * (nx + pad_cols))
    g.synchronize()
    out, pads = {}, []
    for k, b in bufs.items():
        raw = b.cpu().numpy()
        item = 4 if k == "e" else 8
        out[k] = np.ascontiguousarray(raw[:, :nx * item]).view(np.float32 if k == "e" else np.uint64)
        pads.append(raw[:, nx * item:].ravel())
    return out.get("l"), out.get("s"), out.get("e"), np.concatenate(pads)


def _list_device(g, suns, lonlat, want="lse", pad=3):
    """sun_exposure_device into 0xAB-filled tensors `pad` entries longer than the list -> (lit, shadow, exposure, padding bytes)."""
    import torch
    n = len(lonlat)
    p_dev = torch.from_numpy(np.ascontiguousarray(lonlat, np.float64)).cuda()
    bufs = {k: torch.full(((n + pad) * (4 if k == "e" else 8),), FILL, dtype=torch.uint8, device="cuda") for k in want}
    ptr = lambda k: bufs[k].data_ptr() if k in bufs else 0
    torch.cuda.synchronize()
    g.sun_exposure_device(suns, p_dev.data_ptr(), n, ptr("l"), ptr("s"), ptr("e"))
    g.synchronize()
    out, pads = {}, []
    for k, b in bufs.items():
        raw = b.cpu().numpy()
        item = 4 if k == "e" else 8
        out[k] = raw[:n * item].copy().view(np.float32 if k == "e" else np.uint64)
        pads.append(raw[n * item:])
    return out.get("l"), out.get("s"), out.get("e"), np.concatenate(pads)


def _compare(lit, shadow, exposure, emu, ref, amb, what, ref_exposure=None):
    """The comparison rule (module docstring); emu, ref: (suns, n) classes; -> the number of device / emulation differences."""
    got = _states(lit, shadow, len(emu))
    assert not (lit.reshape(-1) & shadow.reshape(-1)).any(), "no sun is LIT and SHADOW"
    for other, name in ((_fold(emu), "emulation"), (_fold(ref), "reference")):
        bad = np.argwhere((got != other) & ~amb)
        assert len(bad) == 0, f"{what}: {len(bad)} unambiguous pairs differ from the {name}, first (sun, target) {tuple(bad[0])}: {got[tuple(bad[0])]} vs {other[tuple(bad[0])]}"
    n = int((got != _fold(emu)).sum())
    print(f"{what}: {got.size} pairs, {int(amb.sum())} ambiguous, {n} device / emulation differences; lit {int((got == 1).sum())}, shadow {int((got == 3).sum())}")
    if exposure is not None and ref_exposure is not None:
        e = exposure.reshape(-1)
        clear = ~amb.any(axis=0)
        none = ref[0] == SNR.NONE
        assert np.array_equal(np.isnan(e)[clear], none[clear]), f"{what}: the exposure is NaN exactly where there is no terrain"
        at = clear & ~none
        ulps = SC.ulp_distance_f32(e[at], ref_exposure[at])
        print(f"{what}: exposure on {int(at.sum())} clear terrain targets: max {int(ulps.max())} f32 ulps from the reference, {int((ulps > 0).sum())} differ")
        assert ulps.max() <= 1
    return n


@pytest.mark.parametrize("name", sorted(SC.GRIDS))
def test_grid_cases(topo, name):
    """Every grid case (nx = 40: a wave with a tail; negative and positive dlat): the grid call, the list call on the same numbers and
    the host read give the same bytes, and those are the emulation's and the reference's."""
    c = SC.case(name)
    ref, _, _, ref_exp, amb = SC.reference(name)
    emu = SC.emulation(name)[0]
    assert amb.mean() <= SC.MAX_AMBIGUOUS
    g = renderer(topo, c["tiles"], c["order"])
    lit, shadow, exposure, pad = _grid(g, c["suns"], c["grid"], pad_cols=3)
    assert (pad == FILL).all(), "bytes between nx and a pitch are left alone"
    l_lit, l_shadow, l_exp, pad = _list_device(g, c["suns"], c["lonlat"])
    assert (pad == FILL).all(), "the bytes behind a list are left alone"
    r_lit, r_shadow, r_exp = g.sun_exposure(c["suns"], c["lonlat"])
    g.close()
    for what, a, b, d in (("lit", lit, l_lit, r_lit), ("shadow", shadow, l_shadow, r_shadow), ("exposure", exposure, l_exp, r_exp)):
        assert a.tobytes() == b.tobytes(), f"{what}: the list form on the same targets gives the grid's bytes"
        assert d.tobytes() == b.tobytes(), f"{what}: topo_sun_exposure_read equals the device call"
    _compare(lit, shadow, exposure, emu, ref, amb, name, ref_exp)


def test_three_waves_per_row(topo):
    """The 130 x 34 tile of 3 x 3 ragged blocks under a 130 x 7 grid: a row takes three waves, the last partial, and the 21 waves are
    no multiple of a workgroup's four.  The pitches are padded, and the padding's sentinel bytes survive."""
    tiles, order, box = VC.tileset("blocks")
    c = SC.grid_case("blocks", 130, 7)
    ref, _, _, ref_exp, amb = SNR.sun_exposure(VC.meshes("blocks"), c["suns"], c["lonlat"])
    emu, brute = SC.emulate(c)[0], SC.emulate(c, brute=True)[0]
    assert emu.tobytes() == brute.tobytes() and amb.mean() <= SC.MAX_AMBIGUOUS
    g = renderer(topo, tiles, order)
    lit, shadow, exposure, pad = _grid(g, c["suns"], c["grid"], pad_cols=7)
    g.close()
    assert (pad == FILL).all(), "bytes between nx and a pitch are left alone"
    _compare(lit, shadow, exposure, emu, ref, amb, "130 x 7", ref_exp)
    got = _states(lit, shadow, 13)
    for k in SC.EL4:
        assert (got[k] == SNR.LIT).sum() >= 10 and (got[k] == SNR.SHADOW).sum() >= 10, k


def test_64_and_33_suns_bit_by_bit(topo):
    """64 suns repeat the arc and use bit 63; 33 suns use bit 32.  Bit k of each equals the bit of sun k alone."""
    c = SC.case("blocks")
    suns64 = np.concatenate([c["suns"]] * 5)[:64]
    suns64["weight"] = 1.0 + np.arange(64)
    g = renderer(topo, c["tiles"], c["order"])
    alone = [g.sun_exposure(c["suns"][k:k + 1], c["lonlat"])[:2] for k in range(13)]
    emu = SC.emulation("blocks")[0]
    amb = SC.reference("blocks")[4]
    for n in (64, 33):
        lit, shadow, exposure = g.sun_exposure(suns64[:n], c["lonlat"])
        if n < 64:
            assert not ((lit | shadow) >> np.uint64(n)).any(), "no bit beyond the suns of the call"
        for k in range(n):
            one = np.uint64(1)
            assert np.array_equal((lit >> np.uint64(k)) & one, alone[k % 13][0]) and np.array_equal((shadow >> np.uint64(k)) & one, alone[k % 13][1]), (n, k)
        got = _states(lit, shadow, n)
        want = _fold(emu)[np.arange(n) % 13]
        assert not ((got != want) & ~amb[np.arange(n) % 13]).any()
        # the exposure is the weighted sum over the lit suns: against the emulation on the same 64 suns, where the bits agree
        e_cls, e_lit, e_shadow, e_exp, bad = SE.sun_exposure(c["tiles"], c["order"], suns64[:n], c["lonlat"])
        same = (e_lit == lit) & ~np.isnan(e_exp)
        assert bad == 0 and same.sum() > 0.9 * (~np.isnan(e_exp)).sum() and SC.ulp_distance_f32(exposure[same], e_exp[same]).max() <= 1
    assert ((lit >> np.uint64(32)) & np.uint64(1)).any(), "bit 32 is in use"
    lit64 = g.sun_exposure(suns64, c["lonlat"])[0]
    g.close()
    assert (lit64 >> np.uint64(63)).any(), "bit 63 is in use"


def test_tile_of_more_than_64_blocks(topo):
    """The `grid` tile, 301 x 250 vertices in 85 raster blocks: the wave takes a tile's blocks in two batches of 64.  A 24 x 12 grid
    under the three eastern low suns against the emulation's every-triangle loop, and against the reference on every fifth target."""
    tiles, order, box = VC.tileset("grid")
    c = SC.grid_case("grid", 24, 12, suns=SC.standard_suns("grid")[1:4])
    brute, emu = SC.emulate(c, brute=True)[0], SC.emulate(c)[0]
    assert emu.tobytes() == brute.tobytes()
    sub = np.arange(0, len(c["lonlat"]), 5)
    ref, _, _, _, amb = SNR.sun_exposure(VC.meshes("grid"), c["suns"], c["lonlat"][sub])
    assert not ((ref != brute[:, sub]) & ~amb).any()
    g = renderer(topo, tiles, order)
    lit, shadow, exposure, _ = _grid(g, c["suns"], c["grid"])
    g.close()
    lit, shadow = lit.reshape(-1), shadow.reshape(-1)
    _compare(lit[sub], shadow[sub], None, brute[:, sub], ref, amb, "grid tile, every fifth target")
    got = _states(lit, shadow, 3)
    differ = got != _fold(brute)
    print(f"grid tile: {int(differ.sum())} of {got.size} pairs differ from the every-triangle loop")
    assert differ.sum() <= 0.005 * got.size and not (differ[:, sub] & ~amb).any()
    assert (got == SNR.LIT).sum() >= 2 and (got == SNR.SHADOW).sum() >= 2


def test_each_output_alone_gives_the_bytes_it_gives_with_the_others(topo):
    c = SC.case("ridges_ne")
    g = renderer(topo, c["tiles"], c["order"])
    lit, shadow, exposure, _ = _grid(g, c["suns"], c["grid"])
    l_all = _list_device(g, c["suns"], c["lonlat"])
    for want in ("l", "s", "e", "ls", "le"):
        a = _grid(g, c["suns"], c["grid"], pad_cols=1, want=want)
        b = _list_device(g, c["suns"], c["lonlat"], want=want)
        assert (a[3] == FILL).all() and (b[3] == FILL).all()
        for k, full, l_full, x, y in zip("lse", (lit, shadow, exposure), l_all[:3], a[:3], b[:3]):
            assert (x is None) == (k not in want) and (y is None) == (k not in want)
            if k in want:
                assert x.tobytes() == full.tobytes() and y.tobytes() == l_full.tobytes(), (want, k)
    # the host read: an output not asked for is not touched
    L = topo.lib()
    vp = lambda a: a.ctypes.data_as(topo.C.c_void_p)
    s, p = np.ascontiguousarray(c["suns"]), np.ascontiguousarray(c["lonlat"])
    only = np.zeros(len(p), np.float32)
    assert L.topo_sun_exposure_read(g._h, len(s), vp(s), len(p), vp(p), None, None, vp(only)) == 0
    assert only.tobytes() == exposure.tobytes()
    only = np.zeros(len(p), np.uint64)
    assert L.topo_sun_exposure_read(g._h, len(s), vp(s), len(p), vp(p), None, vp(only), None) == 0
    assert only.tobytes() == shadow.tobytes()
    g.close()


def test_sub_rectangle_of_a_larger_image(topo):
    import torch
    c = SC.case("blocks")
    g = renderer(topo, c["tiles"], c["order"])
    lon0, lat0, dlon, dlat, nx, ny = c["grid"]
    W, H, c0, r0 = 100, 40, 13, 5
    masks = torch.full((2, H, W), -0x3232323232323233, dtype=torch.int64, device="cuda")      # 0xCD bytes
    img = torch.full((H, W), 0xCD, dtype=torch.uint8, device="cuda").repeat(1, 4).contiguous()
    torch.cuda.synchronize()
    at = (r0 * W + c0)
    g.sun_exposure_grid_device(c["suns"], lon0, lat0, dlon, dlat, nx, ny, masks[0].data_ptr() + 8 * at, masks[1].data_ptr() + 8 * at, img.data_ptr() + 4 * at, 8 * W, 4 * W)
    g.synchronize()
    raw_m = masks.cpu().numpy().view(np.uint64)
    raw_e = img.cpu().numpy().view(np.uint8).reshape(H, W, 4)
    lit, shadow, exposure, _ = _grid(g, c["suns"], c["grid"])
    g.close()
    assert raw_m[0, r0:r0 + ny, c0:c0 + nx].tobytes() == lit.tobytes() and raw_m[1, r0:r0 + ny, c0:c0 + nx].tobytes() == shadow.tobytes()
    assert raw_e[r0:r0 + ny, c0:c0 + nx].tobytes() == exposure.tobytes()
    outside = np.ones((H, W), bool)
    outside[r0:r0 + ny, c0:c0 + nx] = False
    assert (raw_m[:, outside] == 0xCDCDCDCDCDCDCDCD).all() and (raw_e[outside] == 0xCD).all()


def test_errors(topo):
    import torch
    c = SC.case("blocks")
    g = renderer(topo, c["tiles"], c["order"])
    suns = c["suns"]
    buf = torch.zeros((4096,), dtype=torch.uint8, device="cuda")
    pts = torch.from_numpy(c["lonlat"][:64].copy()).cuda()
    b, p = buf.data_ptr(), pts.data_ptr()
    ok = dict(lon0=7.0, lat0=46.0, dlon=0.1, dlat=0.1, nx=8, ny=4, lit_ptr=b, shadow_ptr=b + 1024, exposure_ptr=b + 2048, mask_pitch_bytes=64, exposure_pitch_bytes=32)
    g.sun_exposure_grid_device(suns, **ok)
    many = np.concatenate([suns] * 5)[:65]

    def sun(d, w=15.0):
        return SC.sun_records(d, w)

    bad_suns = (many, sun([0.0, 0.0, 0.0]), sun([np.nan, 0.0, 1.0]), sun([np.inf, 0.0, 1.0]), sun([0.0, 1.0, 0.0], np.nan), sun([0.0, 1.0, 0.0], np.inf),
                sun([0.0, 1.0, 0.0], -1.0), np.concatenate([suns, sun([0.0, 0.0, 0.0])]))
    for change in (dict(nx=0), dict(ny=0), dict(lit_ptr=0, shadow_ptr=0, exposure_ptr=0), dict(lon0=np.nan), dict(lat0=np.inf), dict(dlon=-np.inf), dict(dlat=np.nan),
                   dict(mask_pitch_bytes=56), dict(mask_pitch_bytes=68), dict(exposure_pitch_bytes=28), dict(exposure_pitch_bytes=34), dict(lit_ptr=b + 4),
                   dict(shadow_ptr=b + 1028), dict(exposure_ptr=b + 2050), dict(nx=1 << 31, ny=1 << 31, mask_pitch_bytes=1 << 34, exposure_pitch_bytes=1 << 33),
                   dict(nx=64 * 65536, ny=65536, mask_pitch_bytes=8 * 64 * 65536, exposure_pitch_bytes=4 * 64 * 65536)):
        with pytest.raises(topo.TopoError) as e:
            g.sun_exposure_grid_device(suns, **dict(ok, **change))
        assert e.value.code == topo.TOPO_ERR_INVALID, change
    # a pitch is checked only for the outputs given
    g.sun_exposure_grid_device(suns, **dict(ok, lit_ptr=0, shadow_ptr=0, mask_pitch_bytes=3))
    g.sun_exposure_grid_device(suns, **dict(ok, exposure_ptr=0, exposure_pitch_bytes=1))
    for s in bad_suns:
        with pytest.raises(topo.TopoError) as e:
            g.sun_exposure_grid_device(s, **ok)
        assert e.value.code == topo.TOPO_ERR_INVALID
        with pytest.raises(topo.TopoError) as e:
            g.sun_exposure_device(s, p, 64, b, b + 1024, b + 2048)
        assert e.value.code == topo.TOPO_ERR_INVALID
        with pytest.raises(topo.TopoError) as e:
            g.sun_exposure(s, c["lonlat"][:64])
        assert e.value.code == topo.TOPO_ERR_INVALID
    g.sun_exposure_device(suns, p, 64, b, b + 1024, b + 2048)
    for args in ((suns, 0, 64, b, 0, 0), (suns, p + 8, 63, b, 0, 0), (suns, p, 64, 0, 0, 0), (suns, p, 64, b + 4, 0, 0), (suns, p, 64, 0, b + 12, 0), (suns, p, 64, 0, 0, b + 2)):
        with pytest.raises(topo.TopoError) as e:
            g.sun_exposure_device(*args)
        assert e.value.code == topo.TOPO_ERR_INVALID, args[1:]
    L = topo.lib()
    vp = lambda a: a.ctypes.data_as(topo.C.c_void_p)
    out = np.zeros(64, np.uint64)
    host = c["lonlat"][:64].copy()
    s = np.ascontiguousarray(suns)
    assert L.topo_sun_exposure_read(g._h, 13, None, 64, vp(host), vp(out), None, None) == topo.TOPO_ERR_INVALID
    assert L.topo_sun_exposure_read(g._h, 13, vp(s), 64, None, vp(out), None, None) == topo.TOPO_ERR_INVALID
    assert L.topo_sun_exposure_read(g._h, 13, vp(s), 64, vp(host), None, None, None) == topo.TOPO_ERR_INVALID
    assert L.topo_sun_exposure_read(g._h, 65, vp(many), 64, vp(host), vp(out), None, None) == topo.TOPO_ERR_INVALID
    assert L.topo_sun_exposure_grid_device(g._h, 13, None, 7.0, 46.0, 0.1, 0.1, 8, 4, topo.C.c_void_p(b), None, None, 64, 32) == topo.TOPO_ERR_INVALID
    assert L.topo_sun_exposure_device(g._h, 13, None, 64, topo.C.c_void_p(p), topo.C.c_void_p(b), None, None) == topo.TOPO_ERR_INVALID
    # no suns and no targets are no-ops, whatever else is given
    before = buf.cpu().numpy().copy()
    g.sun_exposure_grid_device(suns[:0], **ok)
    g.sun_exposure_device(suns[:0], p, 64, b)
    g.sun_exposure_device(suns, 0, 0, 0)
    assert L.topo_sun_exposure_read(g._h, 0, None, 64, vp(host), None, None, None) == 0 and L.topo_sun_exposure_read(g._h, 13, vp(s), 0, None, None, None, None) == 0
    g.synchronize()
    assert np.array_equal(buf.cpu().numpy(), before)
    g.close()
    # with no tiles every point is NONE
    e = topo.TerrainRenderer(64, 48)
    lit, shadow, exposure = e.sun_exposure(suns, c["lonlat"][:70])
    assert not lit.any() and not shadow.any() and np.isnan(exposure).all()
    e.close()


def test_sun_calls_change_no_frame_and_no_mask(topo):
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
    suns = topo.suns([topo.sun_direction(16.0, 46.0, az, el) for az, el in SC.ARC], SC.WEIGHT)
    grid = (15.0, 47.0, 2.0 / 70, -2.0 / 40, 70, 40)
    pts = VC.grid_points(grid)
    out_l, out_s = torch.zeros((40, 70), dtype=torch.int64, device="cuda"), torch.zeros((40, 70), dtype=torch.int64, device="cuda")
    out_e = torch.zeros((40, 70), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    first = None
    for yaw, pitch, fov in ((40, 10, 70), (120, 60, 90), (300, 2, 50)):
        u = sc.uniforms(W, H, yaw, pitch, fov, 0)
        a.update(W, H, u, pu)
        b.update(W, H, u, pu)
        got = b.sun_exposure(suns, pts)
        assert first is None or all(x.tobytes() == y.tobytes() for x, y in zip(got, first))
        first = got
        ra, rb = a.render(), b.render()
        b.sun_exposure(suns[3:9], pts[::3])
        b.sun_exposure_grid_device(suns, *grid, out_l.data_ptr(), out_s.data_ptr(), out_e.data_ptr())
        assert_same_frame(ra, rb, f"sun exposure calls vs none, yaw {yaw}")
        assert a.counters() == b.counters() and a.frame_status() == b.frame_status()
        assert np.array_equal(a.horizon(), b.horizon())
    assert (first[0] != 0).sum() > 50 and not np.isnan(first[2]).all()
    b.synchronize()
    dev = (out_l.cpu().numpy().view(np.uint64).reshape(-1), out_s.cpu().numpy().view(np.uint64).reshape(-1), out_e.cpu().numpy().reshape(-1))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(dev, first))
    masks = [(a.viewshed(*loc), b.viewshed(*loc)) for loc in sc.locs]
    assert any(ma.any() for ma, _ in masks) and all(np.array_equal(ma, mb) for ma, mb in masks)
    # two submissions in flight, the calls queued before the join: the frames are those of a renderer that made none
    sw, sh = 48, 40
    us = sc.panorama(sw, sh, yaw0_deg=25.0)
    p_dev = torch.from_numpy(pts.copy()).cuda()
    lst_l, lst_e = torch.zeros((len(pts),), dtype=torch.int64, device="cuda"), torch.zeros((len(pts),), dtype=torch.float32, device="cuda")
    out_l.zero_()
    out_s.zero_()
    out_e.zero_()
    torch.cuda.synchronize()
    frames = []
    for r, ask in ((a, False), (b, True)):
        r.set_stream(torch.cuda.current_stream().cuda_stream)
        r.set_pipeline_depth(2)
        keep = [strip(r, us[:2], sw, sh), strip(r, us[2:7], sw, sh)]
        if ask:
            r.sun_exposure_device(suns, p_dev.data_ptr(), len(pts), lst_l.data_ptr(), 0, lst_e.data_ptr())
            r.sun_exposure_grid_device(suns, *grid, out_l.data_ptr(), out_s.data_ptr(), out_e.data_ptr())
        r.join()
        r.synchronize()
        frames.append([(c.cpu().numpy(), d.cpu().numpy()) for c, d in keep])
    for (ca, da), (cb, db) in zip(frames[0], frames[1]):
        assert np.array_equal(ca, cb) and np.array_equal(da.view(np.uint32), db.view(np.uint32))
    assert lst_l.cpu().numpy().tobytes() == first[0].tobytes() and lst_e.cpu().numpy().tobytes() == first[2].tobytes()
    assert out_l.cpu().numpy().tobytes() == first[0].tobytes() and out_s.cpu().numpy().tobytes() == first[1].tobytes() and out_e.cpu().numpy().tobytes() == first[2].tobytes(), \
        "the answers queued beside frames in flight are the host read's"
    a.close()
    b.close()


def _checked_run(T):
    """The grid on the ridges, blocks, void and polar cases, the 130-wide grid, 64 suns over a list and part of the many-block tile
    -> hash of every output, status."""
    import torch
    h = hashlib.sha256()
    status = 0
    for name in ("ridges_ne", "blocks", "void_nan", "polar"):
        c = SC.case(name)
        g = renderer(T, c["tiles"], c["order"])
        for x in _grid(g, c["suns"], c["grid"], pad_cols=1)[:3]:
            h.update(x.tobytes())
        if name == "blocks":
            for x in _grid(g, c["suns"], VC.box_grid(VC.tileset("blocks")[2], 130, 7), pad_cols=2)[:3]:
                h.update(x.tobytes())
            for x in g.sun_exposure(np.concatenate([c["suns"]] * 5)[:64], c["lonlat"]):
                h.update(x.tobytes())
        status |= g.frame_status()["status"]
        g.close()
    tiles, order, box = VC.tileset("grid")
    g = renderer(T, tiles, order)
    for x in _grid(g, SC.standard_suns("grid")[1:4], VC.box_grid(box, 30, 16))[:3]:
        h.update(x.tobytes())
    status |= g.frame_status()["status"]
    g.close()
    torch.cuda.synchronize()
    return {"sha": h.hexdigest()[:24], "status": status}


def test_bounds_checked_build_records_no_out_of_range_index(topo):
    got = checked_run("test_sun_gpu")      # kStatusBounds: an index a sun exposure kernel formed was out of range
    assert got["sha"] == _checked_run(topo)["sha"], "the bounds-checked build answers as the product build"
