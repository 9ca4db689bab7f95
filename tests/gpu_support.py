"""What the GPU tests share: renderers over a scene, strips of views, device variants into padded 0xAB-filled tensors, and the run of
a test module's scenes through the bounds-checked build in a child process.  torch is imported inside the functions: the CPU suite
imports modules that import this one."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def pair(topo, orc, sc, W, H):
    g, o = topo.TerrainRenderer(W, H), orc.OracleRenderer(W, H)
    sc.load(g)
    sc.load(o)
    return g, o


def renderer(T, tiles, order, W=64, H=48):
    g = T.TerrainRenderer(W, H)
    for (lat, lon), t in zip(order, tiles):
        g.add_terrain(lat, lon, *t)
    return g


def strip(r, views, sw, sh):
    import torch
    n = len(views)
    rgba = torch.zeros((n, sh, sw, 4), dtype=torch.uint8, device="cuda")
    depth = torch.zeros((n, sh, sw), dtype=torch.float32, device="cuda")
    r.render_views_device(views, sw, sh, rgba.data_ptr(), sh * sw * 4, sw * 4, depth.data_ptr(), sh * sw * 4, sw * 4)
    return rgba, depth


def strip_host(r, views, sw, sh):
    """strip() on torch's current stream, waited for and copied to the host: (rgba, depth) numpy arrays."""
    import torch
    r.set_stream(torch.cuda.current_stream().cuda_stream)
    rgba, depth = strip(r, views, sw, sh)
    torch.cuda.synchronize()
    return rgba.cpu().numpy(), depth.cpu().numpy()


# ---- device variants into padded tensors ---------------------------------------------------------------------------------------------
def padded_device_output(g, n, rows, cols, item, call, pad_cols=0, pad_rows=0):
    """A device variant's output: n views of rows x cols items of `item` bytes in a 0xAB-filled tensor whose rows are pad_cols items
    and whose views pad_rows rows longer than needed, handed to call(pointer, view stride, pitch) (bytes), read back after the
    renderer's streams -> ((n, rows, cols, item) u8 payload, the padding bytes)."""
    import torch
    pitch = (cols + pad_cols) * item
    stride = pitch * (rows + pad_rows)
    buf = torch.full((n * stride,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    call(buf.data_ptr(), stride, pitch)
    g.synchronize()
    raw = buf.cpu().numpy().reshape(n, rows + pad_rows, cols + pad_cols, item)
    return np.ascontiguousarray(raw[:, :rows, :cols]), np.concatenate([raw[:, :rows, cols:].ravel(), raw[:, rows:].ravel()])


def ground_map(g, n, W, H, first=0, pad_px=0, pad_rows=0):
    """ground_map_device of views [first, first + n) into a torch tensor whose rows are pad_px pixels and whose views are pad_rows
    rows longer than needed: ((n, H, W, 4) f32 values, the padding bytes)."""
    vals, pad = padded_device_output(g, n, H, W, 16, lambda p, stride, pitch: g.ground_map_device(p, first, n, stride, pitch), pad_px, pad_rows)
    return vals.view(np.float32).reshape(n, H, W, 4), pad


def sunlit_map(g, sun, n, W, H, first=0, pad_px=0, pad_rows=0):
    """sunlit_map_device of views [first, first + n) into a tensor whose rows are pad_px bytes and whose views pad_rows rows longer
    than needed: ((n, H, W) classes, the padding bytes)."""
    vals, pad = padded_device_output(g, n, H, W, 1, lambda p, stride, pitch: g.sunlit_map_device(sun, p, first, n, stride, pitch), pad_px, pad_rows)
    return vals.reshape(n, H, W), pad


def unwrap_run(T, g, params, views, sw, sh, rgba_src, depth_src, want="rds", slack=48):
    """topo_unwrap_device into 0xAB-filled outputs whose pitch is `slack` bytes (rounded up to 16) more than a row; -> dict of numpy
    arrays (rgba (H, W, 4) u8, depth (H, W) u32 bits, src (H, W) i32) for the outputs in `want`; the bytes beyond out_w must be untouched."""
    import torch
    W, H = int(params["out_w"][0]), int(params["out_h"][0])
    pitch = (W * 4 + slack + 15) // 16 * 16
    bufs = {k: torch.full((H, pitch), 0xAB, dtype=torch.uint8, device="cuda") for k in want}
    ptr = lambda k: bufs[k].data_ptr() if k in bufs else 0
    g.unwrap_device(params, views, sw, sh, rgba_src_ptr=rgba_src.data_ptr() if "r" in want else 0, depth_src_ptr=depth_src.data_ptr() if "d" in want else 0,
                    rgba_out_ptr=ptr("r"), rgba_out_pitch=pitch, depth_out_ptr=ptr("d"), depth_out_pitch=pitch, src_out_ptr=ptr("s"), src_out_pitch=pitch)
    g.synchronize()
    out = {}
    for k, b in bufs.items():
        a = b.cpu().numpy()
        assert (a[:, W * 4:] == 0xAB).all(), f"output {k}: bytes between out_w and the pitch were written"
        body = np.ascontiguousarray(a[:, :W * 4])
        out[k] = body.reshape(H, W, 4) if k == "r" else body.view(np.uint32 if k == "d" else np.int32).reshape(H, W)
    return out


# ---- the bounds-checked build in a child process -------------------------------------------------------------------------------------
def _checked_child(argv, timeout):
    """One fresh python child with TOPO_HIP_LIB = libtopo_hip_check.so; its last line of output is JSON that names the library it
    loaded.  Fails on any other exit status than 0, with the end of the child's stderr."""
    import pytest
    import topo_renderer_amd as T
    check = os.path.join(os.path.dirname(T.LIB_PATH), "libtopo_hip_check.so")
    assert os.path.exists(check), "run __graft_entry__.build()"
    res = subprocess.run([sys.executable, *argv], env=dict(os.environ, TOPO_HIP_LIB=check), capture_output=True, text=True, timeout=timeout)
    if res.returncode != 0:
        pytest.fail(f"bounds-checked run of {argv[-1][-200:]} failed ({res.returncode}): {res.stderr[-3000:]}")
    got = json.loads(res.stdout.strip().split("\n")[-1])
    assert got["lib"].endswith("libtopo_hip_check.so")
    return got


def checked_run(module_name, timeout=600):
    """The test module's _checked_run(T) in the bounds-checked build -> its dict.  No index any kernel formed may have been out of
    range (kStatusBounds, status bit 4).  The caller runs its own _checked_run(topo) only after this returned: nothing more is
    started on the device behind a child that did not exit cleanly."""
    code = f"import sys, json; sys.path[:0] = [{os.path.dirname(HERE)!r}, {HERE!r}]; import topo_renderer_amd as T; " \
           f"import {module_name} as m; print(json.dumps(dict(m._checked_run(T), lib=T.LIB_PATH)))"
    got = _checked_child(["-c", code], timeout)
    assert not (got["status"] & 4), got
    return got


def checked_script(path, timeout):
    """A scene script of tests/ (bounds_scenes.py, limits_scenes.py) in the bounds-checked build -> the dict it prints."""
    return _checked_child([os.path.join(HERE, path)], timeout)
