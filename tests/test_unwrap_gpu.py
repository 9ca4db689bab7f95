"""Unwrap (topo_unwrap_device) on the GPU: k_unwrap against the g++ build of the same per-pixel functions (tests/unwrap_emul.py), whose
agreement with the independent reference tests/test_unwrap_cpu.py establishes; the outputs against the rendered sources gathered
through the source map; pitches, partial outputs, errors, and that an unwrap changes no frame."""
import ctypes as C
import hashlib
import math

import numpy as np
import pytest

import unwrap_cases as UC
import unwrap_ref as UR
from gpu_support import checked_run, unwrap_run

pytestmark = pytest.mark.gpu
_SOURCES = {}


def rendered(T, name, fmt=None):
    """(renderer, rgba (n, sh, sw, 4) u8 tensor, depth (n, sh, sw) f32 tensor) of a case's source views, rendered once per distinct source."""
    import torch
    fmt = T.FORMAT_RGBA8_UNORM_SRGB if fmt is None else fmt
    views, sw, sh, _, how = UC.case(name)
    key = (how, sw, sh, fmt, id(T))
    if key not in _SOURCES:
        sc = UC.scene()
        g = T.TerrainRenderer(sw, sh, color_format=fmt)
        sc.load(g)
        g.set_stream(torch.cuda.current_stream().cuda_stream)
        n = len(views)
        rgba = torch.zeros((n, sh, sw, 4), dtype=torch.uint8, device="cuda")
        depth = torch.zeros((n, sh, sw), dtype=torch.float32, device="cuda")
        if how[0] == "panorama":      # a world of one
            g.render_panorama(None, sc.eye, math.radians(how[1]), sw, sh, sc.vlon, sc.vlat, rgba.data_ptr(), depth.data_ptr(), pitch=math.radians(how[2]))
        else:
            g.render_views_device(views, sw, sh, rgba.data_ptr(), sh * sw * 4, sw * 4, depth.data_ptr(), sh * sw * 4, sw * 4)
        g.synchronize()
        assert (depth < 1).any() and (depth == 1).any()      # terrain and sky
        _SOURCES[key] = (g, rgba, depth)
    return _SOURCES[key]


@pytest.mark.parametrize("name", UC.NEAREST_CASES)
def test_nearest_cases(topo, name):
    import unwrap_emul
    views, sw, sh, params, _ = UC.case(name)
    g, rgba, depth = rendered(topo, name)
    got = unwrap_run(topo, g, params, views, sw, sh, rgba, depth)
    emu = unwrap_emul.unwrap(params, views, sw, sh)
    assert np.array_equal(got["s"], emu["src"]), f"{int((got['s'] != emu['src']).sum())} source-map entries differ from the emulation"
    r, d = rgba.cpu().numpy(), depth.cpu().numpy().view(np.uint32)
    assert np.array_equal(got["r"], UR.gather(got["s"], r, 0))
    assert np.array_equal(got["d"], UR.gather(got["s"], d, 0x7FC00000))
    none = got["s"] < 0
    assert (got["r"][none] == 0).all() and (got["d"][none] == 0x7FC00000).all()
    assert (~none).any() and ((got["d"][~none].view(np.float32) < 1).any())      # terrain came across


@pytest.mark.parametrize("fmt", ["FORMAT_RGBA8_UNORM_SRGB", "FORMAT_BGRA8_UNORM"])
def test_bilinear_equals_the_emulation(topo, fmt):
    import unwrap_emul
    fmt = getattr(topo, fmt)
    views, sw, sh, params, _ = UC.case("g")
    g, rgba, depth = rendered(topo, "g", fmt)
    got = unwrap_run(topo, g, params, views, sw, sh, rgba, depth)
    emu = unwrap_emul.unwrap(params, views, sw, sh, rgba.cpu().numpy(), depth.cpu().numpy(), srgb=fmt == topo.FORMAT_RGBA8_UNORM_SRGB)
    assert np.array_equal(got["s"], emu["src"])
    assert np.array_equal(got["r"], emu["rgba"]), f"{int((got['r'] != emu['rgba']).sum())} channels differ from the emulation"
    assert np.array_equal(got["d"], emu["depth"].view(np.uint32))      # depth stays nearest
    assert (got["r"] != UR.gather(got["s"], rgba.cpu().numpy(), 0)).any()      # (a blend, not a gather)


def test_partial_outputs(topo):
    views, sw, sh, params, _ = UC.case("b")
    g, rgba, depth = rendered(topo, "b")
    full = unwrap_run(topo, g, params, views, sw, sh, rgba, depth)
    for want in ("r", "d", "s", "rd", "ds"):
        part = unwrap_run(topo, g, params, views, sw, sh, rgba, depth, want=want, slack=0)
        for k in want:
            assert np.array_equal(part[k], full[k]), (want, k)


def test_errors(topo):
    import torch
    views, sw, sh, params, _ = UC.case("a")
    g, rgba, depth = rendered(topo, "a")
    L = topo.lib()
    W, H = int(params["out_w"][0]), int(params["out_h"][0])
    out = torch.zeros((3, H, W * 4 + 16), dtype=torch.uint8, device="cuda")
    us = np.ascontiguousarray(np.stack([np.ascontiguousarray(u).view(np.uint8).reshape(160) for u in views]))
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    pitch = W * 4 + 16
    base = dict(params=vp(params), n=8, views=vp(us), sw=sw, sh=sh, rs=rgba.data_ptr(), rvs=sw * sh * 4, rp=sw * 4, ds=depth.data_ptr(), dvs=sw * sh * 4, dp=sw * 4,
                ro=out[0].data_ptr(), rop=pitch, do=out[1].data_ptr(), dop=pitch, so=out[2].data_ptr(), sop=pitch)

    def call(**kw):
        a = dict(base, **kw)
        return L.topo_unwrap_device(g._h, a["params"], a["n"], a["views"], a["sw"], a["sh"], a["rs"] or None, a["rvs"], a["rp"], a["ds"] or None, a["dvs"], a["dp"],
                                    a["ro"] or None, a["rop"], a["do"] or None, a["dop"], a["so"] or None, a["sop"])

    def with_params(**kw):
        q = params.copy()
        for k, v in kw.items():
            q[k] = v
        return call(params=vp(q))

    assert call() == topo.TOPO_OK
    bad = {"null params": call(params=None), "null views": call(views=None), "no views": call(n=0), "65 views": call(n=65),
           "zero src_w": call(sw=0), "zero src_h": call(sh=0), "zero out_w": with_params(out_w=0), "zero out_h": with_params(out_h=0),
           "projection": with_params(projection=2), "filter": with_params(filter=7), "span 0": with_params(az_span_deg=0.0),
           "span > 360": with_params(az_span_deg=361.0), "top 90": with_params(el_top_deg=90.0), "bottom >= top": with_params(el_bottom_deg=30.0),
           "no output": call(ro=0, do=0, so=0), "rgba without source": call(rs=0), "depth without source": call(ds=0),
           "misaligned pointer": call(ro=out[0].data_ptr() + 4), "misaligned pitch": call(dop=pitch + 4), "pitch below a row": call(sop=W * 4 - 16),
           "source pitch below a row": call(rp=sw * 4 - 4),
           "source map beyond 2^31": call(n=64, sw=8192, sh=4096, views=vp(np.ascontiguousarray(np.repeat(us[:1], 64, axis=0))), ro=0, do=0)}
    eyes = us.copy()
    eyes[3].view(np.float32)[32] += 1.0
    bad["differing eyes"] = call(views=vp(eyes))
    for what, rc in bad.items():
        assert rc == topo.TOPO_ERR_INVALID, (what, rc)
    assert b"eye" in L.topo_last_error(g._h)
    g.synchronize()
    assert g.frame_status()["status"] == 0


def test_unwrap_changes_no_frame(topo):
    """A frame rendered after an unwrap equals the one of a renderer that never unwrapped; counters and frame status too."""
    import torch
    from scenes import assert_same_frame
    sc = UC.scene()
    W, H = 256, 160
    a, b = topo.TerrainRenderer(W, H), topo.TerrainRenderer(W, H)
    sc.load(a)
    sc.load(b)
    pu = topo.post_uniforms(W, H)
    views, sw, sh, params, _ = UC.case("d")
    rgba, rgba_a = (torch.zeros((8, sh, sw, 4), dtype=torch.uint8, device="cuda") for _ in range(2))
    depth, depth_a = (torch.zeros((8, sh, sw), dtype=torch.float32, device="cuda") for _ in range(2))
    for yaw, pitch, fov in ((40, 10, 70), (120, 60, 90), (300, 2, 50)):
        b.render_views_device(views, sw, sh, rgba.data_ptr(), sh * sw * 4, sw * 4, depth.data_ptr(), sh * sw * 4, sw * 4)
        a.render_views_device(views, sw, sh, rgba_a.data_ptr(), sh * sw * 4, sw * 4, depth_a.data_ptr(), sh * sw * 4, sw * 4)
        unwrap_run(topo, b, params, views, sw, sh, rgba, depth)
        a.synchronize()
        assert torch.equal(rgba, rgba_a) and torch.equal(depth, depth_a)
        u = sc.uniforms(W, H, yaw, pitch, fov, 0)
        a.update(W, H, u, pu)
        b.update(W, H, u, pu)
        assert_same_frame(a.render(), b.render(), f"unwrap vs none, yaw {yaw}")
        assert a.counters() == b.counters() and a.frame_status() == b.frame_status()
    torch.cuda.synchronize()


def _checked_run(T):
    """Unwraps of the kinds above (ragged width, fill rows, a pitched panorama, generic views, bilinear) -> hash of the outputs, status."""
    import torch
    h = hashlib.sha256()
    status = 0
    for name in ("b", "c", "d", "f", "g"):
        views, sw, sh, params, _ = UC.case(name)
        g, rgba, depth = rendered(T, name)
        got = unwrap_run(T, g, params, views, sw, sh, rgba, depth)
        for k in "rds":
            h.update(got[k].tobytes())
        status |= g.frame_status()["status"]
    torch.cuda.synchronize()
    return {"sha": h.hexdigest()[:24], "status": status}


def test_bounds_checked_build_records_no_out_of_range_index(topo):
    got = checked_run("test_unwrap_gpu")      # kStatusBounds: an index k_unwrap (or any kernel) formed was out of range
    want = _checked_run(topo)
    assert got["sha"] == want["sha"] and got["status"] == want["status"]
