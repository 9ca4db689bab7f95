"""Skyline queries on the GPU (topo_skyline_*): k_skyline against the g++ build of the same rule (tests/skyline_emul.py: the traversal
and the every-triangle loop) and the numpy reference (tests/skyline_ref.py) on the cases of tests/skyline_cases.py, the calls'
contract, and their side effects (none).

Comparison rule: on every azimuth the reference does not mark ambiguous the device names the emulation's edge with the crossing
point within 1e-4 m, and the reference's with the point within 1e-3 m; the device and the emulation may differ only on ambiguous
azimuths (device and host sin / cos differ by an ulp)."""
import hashlib

import numpy as np
import pytest

import skyline_cases as SC
import skyline_ref as SR
from gpu_support import checked_run, padded_device_output, renderer, strip

pytestmark = pytest.mark.gpu

IDENTITY = ("kind", "tile_lat_deg", "tile_lon_deg", "cell_x", "cell_y", "tri", "edge")


def _call(g, c, n_az=None, obs=None):
    obs = c["obs"] if obs is None else obs
    return obs, c["az0"], c["daz"], c["n_az"] if n_az is None else n_az


def _device(g, c, elevation=True, samples=True, pad_el=0, pad_rec=0, obs=None):
    """skyline_device into 0xAB-filled tensors whose observer rows are pad_el floats / pad_rec records longer than needed:
    ((observers, n_az) f32 elevations or None, (observers, n_az) records or None, the padding bytes of both)."""
    import topo_renderer_amd as T
    obs, az0, daz, n_az = _call(g, c, obs=obs)
    n = len(obs)
    got = {}

    def run(el_ptr, el_stride, rec_ptr, rec_stride):
        g.skyline_device(obs, az0, daz, n_az, el_ptr, rec_ptr, c["min_range"], c["max_range"], el_stride, rec_stride)

    if elevation and samples:      # the records' tensor is filled inside the elevations' call
        def both(p, stride, pitch):
            got["rec"] = padded_device_output(g, n, 1, n_az, 64, lambda q, s2, p2: run(p, pitch, q, p2), pad_rec)
        el = padded_device_output(g, n, 1, n_az, 4, both, pad_el)
        rec = got["rec"]
    else:
        el = padded_device_output(g, n, 1, n_az, 4, lambda p, stride, pitch: run(p, pitch, 0, 0), pad_el) if elevation else None
        rec = padded_device_output(g, n, 1, n_az, 64, lambda p, stride, pitch: run(0, 0, p, pitch), pad_rec) if samples else None
    pads = np.concatenate([x[1] for x in (el, rec) if x is not None])
    return (None if el is None else el[0].view(np.float32).reshape(n, n_az), None if rec is None else rec[0].view(T.SKYLINE_DTYPE).reshape(n, n_az), pads)


def _against_emulation(got, name, what):
    """The comparison rule (module docstring) against the emulation -> the number of device / emulation differences, all ambiguous."""
    emu = SC.emulation(name)
    ref, _ = SC.reference(name)
    keep = ~ref["ambiguous"]
    differ = np.zeros(got.shape, bool)
    for f in IDENTITY:
        differ |= got[f] != emu[f]
    bad = np.argwhere(differ & keep)
    assert len(bad) == 0, f"{what}: {len(bad)} unambiguous azimuths differ from the emulation, first {tuple(bad[0])}: {got[tuple(bad[0])]} vs {emu[tuple(bad[0])]}"
    t = keep & (emu["kind"] == SR.TERRAIN)
    gs, gz = SC.plane_point(got[t])
    err = np.hypot(gs - emu["s"][t], gz - emu["z"][t])
    print(f"{what}: {got.size} azimuths, {int((~keep).sum())} ambiguous, {int(differ.sum())} device / emulation differences, crossing point within {err.max():.3e} m of the emulation's")
    assert err.max() <= 1e-4
    assert np.abs(got["lon_deg"][t] - emu["lon_deg"][t]).max() < 1e-9 and np.abs(got["lat_deg"][t] - emu["lat_deg"][t]).max() < 1e-9
    assert np.abs(got["height_m"][t] - emu["height_m"][t].astype(np.float32)).max() <= 1e-3
    z = got[got["kind"] != SR.TERRAIN]
    assert np.isnan(z["elevation_deg"]).all() and not z["range_m"].any() and not z["lon_deg"].any() and not z["height_m"].any() and not z["cell_x"].any() \
        and not z["edge"].any(), "no terrain: a NaN elevation, every other field 0"
    return int(differ.sum())


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_cases(topo, name):
    """Every case: 90 azimuths an observer (the last workgroup has a tail of two waves, or none with four observers).  The device
    call into padded outputs, the host read and the single-output calls give the same bytes, and those are the emulation's and the
    reference's."""
    c = SC.case(name)
    g = renderer(topo, c["tiles"], c["order"])
    el, rec, pad = _device(g, c, pad_el=3, pad_rec=2)
    assert (pad == 0xAB).all(), "the bytes between n_az and a stride are left alone"
    el_read, rec_read = g.skyline(c["obs"], c["az0"], c["daz"], c["n_az"], c["min_range"], c["max_range"])
    el_only, _, pad1 = _device(g, c, samples=False, pad_el=1)
    _, rec_only, pad2 = _device(g, c, elevation=False, pad_rec=1)
    g.close()
    assert (pad1 == 0xAB).all() and (pad2 == 0xAB).all()
    assert rec_read.tobytes() == rec.tobytes() and el_read.tobytes() == el.tobytes(), "topo_skyline_read equals the device call"
    assert el_only.tobytes() == el.tobytes() and rec_only.tobytes() == rec.tobytes(), "a single-output call gives the two-output call's bytes"
    assert el.tobytes() == rec["elevation_deg"].astype(np.float32).tobytes(), "the f32 plane is (float) of the records' elevation, bit for bit"
    for o in c["unusable"]:
        assert (rec[o]["kind"] == topo.SKY_NO_OBSERVER).all()
    _against_emulation(rec, name, name)
    SC.against_reference(rec, name, f"{name} (device)")


def test_an_observers_row_does_not_depend_on_its_company(topo):
    c = SC.case("ridges_ne")
    g = renderer(topo, c["tiles"], c["order"])
    _, rec, _ = _device(g, c, elevation=False)
    _, alone, _ = _device(g, c, elevation=False, obs=c["obs"][4:5])
    _, pair, _ = _device(g, c, elevation=False, obs=c["obs"][[3, 0]])
    g.close()
    assert alone[0].tobytes() == rec[4].tobytes() and pair[1].tobytes() == rec[0].tobytes() and pair[0].tobytes() == rec[3].tobytes()


def test_errors_and_no_ops(topo):
    import torch
    c = SC.case("blocks")
    g = renderer(topo, c["tiles"], c["order"])
    obs = c["obs"][:2]
    n_az = 8
    el = torch.full((2, n_az + 2), 7.0, dtype=torch.float32, device="cuda")
    rec = torch.full((2 * (n_az + 1) * 64,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    e, r = el.data_ptr(), rec.data_ptr()
    assert r % 16 == 0
    ok = dict(az0_deg=1.0, daz_deg=45.0, n_az=n_az, elevation_ptr=e, samples_ptr=r, min_range_m=10.0, max_range_m=1.0e6, observer_stride_bytes=4 * (n_az + 2),
              samples_stride_bytes=64 * (n_az + 1))
    g.skyline_device(obs, **ok)
    many = np.concatenate([c["obs"][:1]] * 65)
    for change in (dict(elevation_ptr=0, samples_ptr=0), dict(elevation_ptr=e + 2), dict(samples_ptr=r + 8), dict(observer_stride_bytes=4 * n_az - 4),
                   dict(observer_stride_bytes=4 * n_az + 2), dict(samples_stride_bytes=64 * n_az - 64), dict(samples_stride_bytes=64 * n_az + 8),
                   dict(az0_deg=np.nan), dict(az0_deg=np.inf), dict(daz_deg=np.nan), dict(daz_deg=-np.inf), dict(min_range_m=np.nan), dict(max_range_m=np.nan),
                   dict(max_range_m=np.inf), dict(min_range_m=0.0), dict(min_range_m=-1.0), dict(min_range_m=2.0e3, max_range_m=1.0e3), dict(max_range_m=1.0e6 + 1.0),
                   dict(n_az=1 << 31, observer_stride_bytes=1 << 33, samples_stride_bytes=1 << 37)):
        with pytest.raises(topo.TopoError) as err:
            g.skyline_device(obs, **dict(ok, **change))
        assert err.value.code == topo.TOPO_ERR_INVALID, change
    with pytest.raises(topo.TopoError) as err:
        g.skyline_device(many, **ok)
    assert err.value.code == topo.TOPO_ERR_INVALID, "more than 64 observers"
    L = topo.lib()
    vp = lambda a: a.ctypes.data_as(topo.C.c_void_p)
    host_el, host_rec = np.zeros((2, n_az), np.float32), np.zeros((2, n_az), topo.SKYLINE_DTYPE)
    assert L.topo_skyline_device(g._h, 2, None, 1.0, 45.0, n_az, 10.0, 1.0e6, topo.C.c_void_p(e), 4 * n_az, None, 0) == topo.TOPO_ERR_INVALID
    assert L.topo_skyline_read(g._h, 2, None, 1.0, 45.0, n_az, 10.0, 1.0e6, vp(host_el), vp(host_rec)) == topo.TOPO_ERR_INVALID
    assert L.topo_skyline_read(g._h, 2, vp(obs), 1.0, 45.0, n_az, 10.0, 1.0e6, None, None) == topo.TOPO_ERR_INVALID
    assert L.topo_skyline_read(g._h, 65, vp(many), 1.0, 45.0, n_az, 10.0, 1.0e6, vp(host_el), None) == topo.TOPO_ERR_INVALID
    assert L.topo_skyline_read(g._h, 2, vp(obs), 1.0, 45.0, n_az, 0.0, 1.0e6, vp(host_el), None) == topo.TOPO_ERR_INVALID
    assert L.topo_skyline_read(g._h, 2, vp(obs), np.nan, 45.0, n_az, 10.0, 1.0e6, vp(host_el), None) == topo.TOPO_ERR_INVALID
    # equal limits are allowed; the limits themselves are inside
    assert L.topo_skyline_read(g._h, 2, vp(obs), 1.0, 45.0, n_az, 1.0e6, 1.0e6, vp(host_el), vp(host_rec)) == topo.TOPO_OK
    assert (host_rec["kind"] == topo.SKY_NONE).all() and np.isnan(host_el).all()
    # the no-ops write nothing, and are no-ops before anything else is looked at
    g.synchronize()
    before = (el.cpu().numpy().tobytes(), rec.cpu().numpy().tobytes())
    g.skyline_device(obs[:0], **ok)
    g.skyline_device(obs, **dict(ok, n_az=0))
    assert L.topo_skyline_device(g._h, 0, None, np.nan, 45.0, n_az, 10.0, 1.0e6, None, 0, None, 0) == topo.TOPO_OK
    assert L.topo_skyline_read(g._h, 2, vp(obs), 1.0, 45.0, 0, 10.0, 1.0e6, None, None) == topo.TOPO_OK
    el0, rec0 = g.skyline(obs[:0], 1.0, 45.0, n_az)
    assert el0.shape == (0, n_az) and rec0.shape == (0, n_az)
    g.synchronize()
    assert (el.cpu().numpy().tobytes(), rec.cpu().numpy().tobytes()) == before
    got = el.cpu().numpy()
    assert (got[:, n_az:] == 7.0).all() and not (got[:, :n_az] == 7.0).any()
    g.close()
    # with no tiles an observer above terrain is unusable and one over the sphere has no skyline
    empty = topo.TerrainRenderer(64, 48)
    el, rec = empty.skyline(c["obs"][[0, 2]], 1.0, 45.0, n_az)
    assert (rec[0]["kind"] == topo.SKY_NO_OBSERVER).all() and (rec[1]["kind"] == topo.SKY_NONE).all() and np.isnan(el).all()
    empty.close()


def test_skyline_calls_change_no_frame(topo):
    """A rendered frame's outputs hash the same before and after a skyline call, frames rendered beside skyline calls are those of a
    renderer that made none, and the skyline's bytes are the same with and without a frame in between."""
    import torch
    from scenes import Scene, assert_same_frame
    sc = Scene(96, 2, 2, eye_dh=100.0)
    W, H = 256, 160
    a, b = topo.TerrainRenderer(W, H), topo.TerrainRenderer(W, H)
    sc.load(a)
    sc.load(b)
    pu = topo.post_uniforms(W, H)
    obs = np.concatenate([topo.observers(sc.vlon, sc.vlat, 30.0), topo.observers(15.7, 46.4, 3000.0)])
    args = (obs, 1.48, 4.0, 90, 5.0, 4.0e5)
    first = b.skyline(*args)
    assert (first[1]["kind"] == topo.SKY_TERRAIN).sum() > 150
    for yaw, pitch, fov in ((40, 10, 70), (300, 2, 50)):
        u = sc.uniforms(W, H, yaw, pitch, fov, 0)
        a.update(W, H, u, pu)
        b.update(W, H, u, pu)
        ra, rb = a.render(), b.render()
        assert_same_frame(ra, rb, f"skyline calls vs none, yaw {yaw}")
        sha = hashlib.sha256(np.ascontiguousarray(rb[0]).tobytes() + np.ascontiguousarray(rb[1]).tobytes()).hexdigest()
        got = b.skyline(*args)
        assert got[0].tobytes() == first[0].tobytes() and got[1].tobytes() == first[1].tobytes(), "the skyline does not depend on the frames around it"
        assert a.counters() == b.counters() and a.frame_status() == b.frame_status()
        assert np.array_equal(a.horizon(), b.horizon())
        rb2 = b.render()
        assert hashlib.sha256(np.ascontiguousarray(rb2[0]).tobytes() + np.ascontiguousarray(rb2[1]).tobytes()).hexdigest() == sha, "the same frame after a skyline call"
        a.render()
    # two submissions in flight, the call queued before the join: the frames are those of a renderer that made none
    sw, sh = 48, 40
    us = sc.panorama(sw, sh, yaw0_deg=25.0)
    el = torch.zeros((2, 90), dtype=torch.float32, device="cuda")
    rec = torch.zeros((2 * 90 * 64,), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    frames = []
    for r, ask in ((a, False), (b, True)):
        r.set_stream(torch.cuda.current_stream().cuda_stream)
        r.set_pipeline_depth(2)
        keep = [strip(r, us[:2], sw, sh), strip(r, us[2:7], sw, sh)]
        if ask:
            r.skyline_device(obs, 1.48, 4.0, 90, el.data_ptr(), rec.data_ptr(), 5.0, 4.0e5)
        r.join()
        r.synchronize()
        frames.append([(c.cpu().numpy(), d.cpu().numpy()) for c, d in keep])
    for (ca, da), (cb, db) in zip(frames[0], frames[1]):
        assert np.array_equal(ca, cb) and np.array_equal(da.view(np.uint32), db.view(np.uint32))
    assert el.cpu().numpy().tobytes() == first[0].tobytes() and rec.cpu().numpy().tobytes() == first[1].tobytes(), \
        "the skyline queued beside frames in flight is the host read's"
    a.close()
    b.close()


def _checked_run(T):
    """The ridges (five observers, the gap's among them), blocks, void, polar and range-limited cases and the many-block tile -> hash of
    every output, status."""
    import torch
    h = hashlib.sha256()
    status = 0
    for name in ("ridges_ne", "blocks", "void_nan", "polar", "ridges_ne_min", "grid"):
        c = SC.case(name)
        g = renderer(T, c["tiles"], c["order"])
        el, rec, _ = _device(g, c, pad_el=1, pad_rec=1)
        h.update(el.tobytes() + rec.tobytes())
        status |= g.frame_status()["status"]
        g.close()
    torch.cuda.synchronize()
    return {"sha": h.hexdigest()[:24], "status": status}


def test_bounds_checked_build_records_no_out_of_range_index(topo):
    got = checked_run("test_skyline_gpu")      # kStatusBounds: an index k_skyline formed was out of range
    assert got["sha"] == _checked_run(topo)["sha"], "the bounds-checked build answers as the product build"
