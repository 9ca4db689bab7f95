"""Refracted visibility queries on the GPU (topo_visibility_refracted_*): k_visibility_refracted_grid and
k_visibility_refracted_list against the g++ build of the same rule (tests/refraction_emul.py) and the numpy reference
(tests/refraction_ref.py) on the cases of tests/refraction_cases.py; k = 0 against topo_visibility_*; the calls' contract and their
side effects (none).

Comparison rule (that of tests/test_visibility_gpu.py): the classes equal the emulation's and the reference's on every target the
reference does not mark ambiguous; the device and the emulation may differ only on ambiguous targets (device and host sin / cos
differ by an ulp)."""
import hashlib
import subprocess

import numpy as np
import pytest

import refraction_cases as RCS
import visibility_cases as VC
from gpu_support import checked_run, padded_device_output, renderer, strip
from test_refraction_cpu import build_harness
from test_visibility_gpu import _compare

pytestmark = pytest.mark.gpu

GRID_CASES = ["gentle", "ridges_ne", "long", "grid"]


def _grid(g, obs, grid, h, k, pad_cols=0, pad_rows=0):
    """visibility_refracted_grid_device (k None: visibility_grid_device) into a 0xAB-filled tensor whose rows are pad_cols bytes and
    whose layers pad_rows rows longer than needed: ((observers, ny, nx) classes, the padding bytes)."""
    lon0, lat0, dlon, dlat, nx, ny = grid
    if k is None:
        call = lambda p, stride, pitch: g.visibility_grid_device(obs, lon0, lat0, dlon, dlat, nx, ny, p, h, stride, pitch)
    else:
        call = lambda p, stride, pitch: g.visibility_refracted_grid_device(obs, lon0, lat0, dlon, dlat, nx, ny, p, h, k, stride, pitch)
    vals, pad = padded_device_output(g, len(obs), ny, nx, 1, call, pad_cols, pad_rows)
    return vals.reshape(len(obs), ny, nx), pad


def _list_device(g, obs, lonlat, h, k, pad=0):
    """visibility_refracted_device (k None: visibility_device) into a 0xAB-filled tensor whose lists are `pad` bytes longer than
    needed: ((observers, n) classes, padding)."""
    import torch
    n = len(lonlat)
    p_dev = torch.from_numpy(np.ascontiguousarray(lonlat, np.float64)).cuda()
    out = torch.full((len(obs), n + pad), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    if k is None:
        g.visibility_device(obs, p_dev.data_ptr(), n, out.data_ptr(), h, n + pad)
    else:
        g.visibility_refracted_device(obs, p_dev.data_ptr(), n, out.data_ptr(), h, k, n + pad)
    g.synchronize()
    raw = out.cpu().numpy()
    return np.ascontiguousarray(raw[:, :n]), raw[:, n:]


def _three_ways(g, c, pad_cols=0, pad_rows=0):
    """The case by the grid call (if it has a grid), the list call and the host read: equal bytes, untouched padding -> (observers, n)."""
    lst, pad = _list_device(g, c["obs"], c["lonlat"], c["h"], c["k"], pad=5)
    assert (pad == 0xAB).all(), "the bytes behind a list are left alone"
    read = g.visibility_refracted(c["obs"], c["lonlat"], c["h"], c["k"])
    assert read.tobytes() == lst.tobytes(), "topo_visibility_refracted_read equals the device call"
    if c["grid"] is not None:
        got, pad = _grid(g, c["obs"], c["grid"], c["h"], c["k"], pad_cols, pad_rows)
        assert (pad == 0xAB).all(), "bytes between nx and the pitch and between the layers are left alone"
        assert got.reshape(len(c["obs"]), -1).tobytes() == lst.tobytes(), "the list form on the same targets gives the grid's bytes"
    return lst


def _k_zero_is_plain(g, c):
    """k = 0 against topo_visibility_* on the same calls, byte for byte."""
    a, _ = _list_device(g, c["obs"], c["lonlat"], c["h"], 0.0)
    b, _ = _list_device(g, c["obs"], c["lonlat"], c["h"], None)
    assert a.tobytes() == b.tobytes(), f"{int((a != b).sum())} bytes of the list call differ at k = 0"
    assert g.visibility_refracted(c["obs"], c["lonlat"], c["h"], 0.0).tobytes() == g.visibility(c["obs"], c["lonlat"], c["h"]).tobytes()
    if c["grid"] is not None:
        assert _grid(g, c["obs"], c["grid"], c["h"], 0.0, 3)[0].tobytes() == _grid(g, c["obs"], c["grid"], c["h"], None, 3)[0].tobytes()


@pytest.mark.parametrize("name", GRID_CASES)
def test_grid_cases(topo, name):
    c = RCS.case(name)
    ref, amb = RCS.reference(name)
    emu, _ = RCS.emulation(name)
    g = renderer(topo, c["tiles"], c["order"])
    got = _three_ways(g, c, pad_cols=3)
    _k_zero_is_plain(g, c)
    g.close()
    _compare(got, emu, ref, amb, name)


def test_three_waves_per_row_and_three_observers(topo):
    """The `blocks` tile under 130 x 7: a row takes three waves, the last partial; three observers, the middle one unusable; layer
    stride and pitch padded, and the padding's 0xAB bytes survive."""
    c = RCS.case("blocks130")
    ref, amb = RCS.reference("blocks130")
    emu, eyes = RCS.emulation("blocks130")
    assert list(eyes["usable"]) == [1, 0, 1] and amb.mean() <= VC.MAX_AMBIGUOUS
    g = renderer(topo, c["tiles"], c["order"])
    got = _three_ways(g, c, pad_cols=7, pad_rows=2)
    _k_zero_is_plain(g, c)
    one, _ = _grid(g, c["obs"][:1], c["grid"], c["h"], c["k"])
    g.close()
    _compare(got, emu, ref, amb, "130 x 7, three observers")
    assert (got[1] == topo.VIS_NO_OBSERVER).all()
    assert one.reshape(-1).tobytes() == got[0].tobytes(), "an observer's layer does not depend on its company"


def test_observers_over_a_list(topo):
    c = RCS.case("observers")
    ref, amb = RCS.reference("observers")
    emu, _ = RCS.emulation("observers")
    g = renderer(topo, c["tiles"], c["order"])
    got = _three_ways(g, c)
    _k_zero_is_plain(g, c)
    _compare(got, emu, ref, amb, "observers")
    for o in c["unusable"]:
        assert (got[o] == topo.VIS_NO_OBSERVER).all()
    # observers 8 and 9 stand on the UNLIFTED ground, on 3 km cells centimetres beneath the lifted one (topo_refraction.h): they do not
    # sit at their targets as under the plain rule, and the answer is the emulation's
    assert got[8][c["at"][0]] == emu[8][c["at"][0]] and got[9][c["at"][1]] == emu[9][c["at"][1]]
    assert (got[0][c["extra"]] == topo.VIS_NONE).all()
    # no observers and no targets are no-ops
    assert g.visibility_refracted(c["obs"][:0], c["lonlat"]).shape == (0, len(c["lonlat"])) and g.visibility_refracted(c["obs"], c["lonlat"][:0]).shape == (len(c["obs"]), 0)
    g.visibility_refracted_device(c["obs"], 0, 0, 0)
    g.visibility_refracted_grid_device(c["obs"][:0], 7.0, 46.0, 0.1, 0.1, 4, 4, 0)
    g.close()


def test_masts_end_at_the_refracted_horizon(topo):
    """The hand-known case on the device: the run of visible masts is the emulation's, at k = 0 and at k = 0.13."""
    c = RCS.case("flat")
    g = renderer(topo, c["tiles"], c["order"])
    runs = []
    for k in (0.0, RCS.K):
        got = g.visibility_refracted(c["obs"], c["lonlat"], c["h"], k)
        emu, _ = RCS.emulation("flat", k)
        differ = int((got != emu).sum())
        print(f"flat k = {k}: {differ} device / emulation differences, visible {int((got == topo.VIS_VISIBLE).sum())}")
        # (device and host sin / cos differ by an ulp, nanometres: only the one mast that stands AT the horizon could fall either way)
        assert differ <= 1, "more than the mast at the horizon differs between the device and the emulation"
        runs.append(int((got == topo.VIS_VISIBLE).sum()))
    g.close()
    assert runs[1] >= runs[0] + 5


def test_errors(topo, tmp_path):
    import torch
    c = RCS.case("blocks130")
    g = renderer(topo, c["tiles"], c["order"])
    obs = c["obs"][:1]
    buf = torch.zeros((4096,), dtype=torch.uint8, device="cuda")
    pts = torch.from_numpy(c["lonlat"][:64].copy()).cuda()
    b, p = buf.data_ptr(), pts.data_ptr()
    ok = dict(lon0=7.0, lat0=46.0, dlon=0.1, dlat=0.1, nx=8, ny=4, out_ptr=b, target_height_m=0.0, refraction_k=0.13, layer_stride_bytes=32, pitch_bytes=8)
    g.visibility_refracted_grid_device(obs, **ok)
    g.visibility_refracted_grid_device(obs, **dict(ok, refraction_k=0.999))
    many = np.concatenate([obs] * 65)
    for change in (dict(refraction_k=np.nan), dict(refraction_k=-0.01), dict(refraction_k=1.0), dict(refraction_k=np.inf), dict(nx=0), dict(out_ptr=0), dict(lon0=np.nan),
                   dict(pitch_bytes=7), dict(layer_stride_bytes=31), dict(target_height_m=-1.0), dict(target_height_m=np.nan)):
        with pytest.raises(topo.TopoError) as e:
            g.visibility_refracted_grid_device(obs, **dict(ok, **change))
        assert e.value.code == topo.TOPO_ERR_INVALID, change
    with pytest.raises(topo.TopoError) as e:
        g.visibility_refracted_grid_device(many, **ok)
    assert e.value.code == topo.TOPO_ERR_INVALID, "more than 64 observers"
    g.visibility_refracted_device(obs, p, 64, b)
    for args in ((obs, 0, 64, b), (obs, p, 64, 0), (obs, p + 8, 63, b), (obs, p, 64, b, 0.0, 0.13, 63), (obs, p, 64, b, 0.0, np.nan), (obs, p, 64, b, 0.0, 1.0),
                 (obs, p, 64, b, 0.0, -0.01), (many, p, 64, b)):
        with pytest.raises(topo.TopoError) as e:
            g.visibility_refracted_device(*args)
        assert e.value.code == topo.TOPO_ERR_INVALID, args[1:]
    for k in (np.nan, -0.01, 1.0):
        with pytest.raises(topo.TopoError) as e:
            g.visibility_refracted(obs, c["lonlat"][:8], 0.0, k)
        assert e.value.code == topo.TOPO_ERR_INVALID, k
    g.synchronize()
    g.close()
    # the same contract through the C ABI: k = NaN, -0.01, 1.0 and 65 observers are refused, k = 0 and the standard k are not
    exe, env = build_harness(topo, tmp_path)
    out = subprocess.run([exe, "gpu"], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert out.stdout.strip().split("\n")[3].split() == [str(topo.TOPO_ERR_INVALID)] * 4 + ["0", "0", str(topo.VIS_NONE)], out.stdout


def test_refracted_calls_change_no_frame(topo):
    """The calls leave a frame queued before them unchanged: two submissions in flight, the calls queued before the join."""
    import torch
    from scenes import Scene
    sc = Scene(96, 2, 2, eye_dh=100.0)
    W, H = 256, 160
    a, b = topo.TerrainRenderer(W, H), topo.TerrainRenderer(W, H)
    sc.load(a)
    sc.load(b)
    obs = np.concatenate([topo.observers(sc.vlon, sc.vlat, 30.0), topo.observers(15.7, 46.4, 3000.0)])
    grid = (15.0, 47.0, 2.0 / 70, -2.0 / 40, 70, 40)
    pts = VC.grid_points(grid)
    first = b.visibility_refracted(obs, pts)
    sw, sh = 48, 40
    us = sc.panorama(sw, sh, yaw0_deg=25.0)
    p_dev = torch.from_numpy(pts.copy()).cuda()
    lst = torch.zeros((2, len(pts)), dtype=torch.uint8, device="cuda")
    out = torch.zeros((2, 40, 70), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    frames = []
    for r, ask in ((a, False), (b, True)):
        r.set_stream(torch.cuda.current_stream().cuda_stream)
        r.set_pipeline_depth(2)
        keep = [strip(r, us[:2], sw, sh), strip(r, us[2:7], sw, sh)]
        if ask:
            r.visibility_refracted_device(obs, p_dev.data_ptr(), len(pts), lst.data_ptr())
            r.visibility_refracted_grid_device(obs, *grid, out.data_ptr())
        r.join()
        r.synchronize()
        frames.append([(c.cpu().numpy(), d.cpu().numpy()) for c, d in keep])
    for (ca, da), (cb, db) in zip(frames[0], frames[1]):
        assert np.array_equal(ca, cb) and np.array_equal(da.view(np.uint32), db.view(np.uint32))
    assert a.counters() == b.counters() and a.frame_status() == b.frame_status()
    assert lst.cpu().numpy().tobytes() == first.tobytes() and out.cpu().numpy().reshape(2, -1).tobytes() == first.tobytes(), \
        "the classes queued beside frames in flight are the host read's"
    assert (first[0] == topo.VIS_VISIBLE).sum() > 50, VC.counts(first[0])
    a.close()
    b.close()


def _checked_run(T):
    """The gentle case (grid, two observers), the 130-wide grid with three observers and part of the many-block tile -> hash of
    every output, status."""
    import torch
    h = hashlib.sha256()
    status = 0
    for name in ("gentle", "blocks130", "grid"):
        c = RCS.case(name)
        g = renderer(T, c["tiles"], c["order"])
        h.update(_grid(g, c["obs"], c["grid"], c["h"], c["k"], pad_cols=1)[0].tobytes())
        status |= g.frame_status()["status"]
        g.close()
    torch.cuda.synchronize()
    return {"sha": h.hexdigest()[:24], "status": status}


def test_bounds_checked_build_records_no_out_of_range_index(topo):
    got = checked_run("test_refraction_gpu")      # kStatusBounds: an index a refracted visibility kernel formed was out of range
    assert got["sha"] == _checked_run(topo)["sha"], "the bounds-checked build answers as the product build"
