"""Independent numpy f64 reference of the unwrap (topo_unwrap_*), written from the definition in include/topo_hip.h: the mapping, the
seam rule, the fill values, the nearest gather and the bilinear filter with its 8-bit weights.  It shares no code with the product
(topo_unwrap.h is not read): the tables are numpy's sin / cos, the blend is f64 and the sRGB curve is the analytic one."""
from __future__ import annotations

import numpy as np

EQUIRECTANGULAR, CYLINDRICAL = 0, 1


def local_frame(eye):
    e = np.asarray(eye, np.float32)[:3].astype(np.float64)
    up = e / np.linalg.norm(e)
    eh = np.hypot(up[0], up[1])
    east = np.array([-up[1] / eh, up[0] / eh, 0.0]) if eh > 0 else np.array([0.0, 1.0, 0.0])
    return east, np.cross(up, east), up


def angles(params):
    """(az (W,), el (H,)) in degrees of the output pixel centres."""
    p = np.asarray(params).reshape(-1)[0]
    W, H = int(p["out_w"]), int(p["out_h"])
    az = float(p["az0_deg"]) + (np.arange(W) + 0.5) * float(p["az_span_deg"]) / W
    f = (np.arange(H) + 0.5) / H
    top, bot = float(p["el_top_deg"]), float(p["el_bottom_deg"])
    if int(p["projection"]) == CYLINDRICAL:
        tt, tb = np.tan(np.radians(top)), np.tan(np.radians(bot))
        el = np.degrees(np.arctan(tt - f * (tt - tb)))
    else:
        el = top - f * (top - bot)
    return az, el


def locate(params, uniforms_list, src_w, src_h):
    """dict: view (H, W) int (-1: none), px, py (H, W) f64 of that view, src (H, W) i32 source map, n_containing (H, W), and the guard
    of the comparison with an f64 implementation: `fragile` (H, W) bool -- px or py of the source within 1e-9 px of an integer, any
    view with cw > 0 whose px or py lies within 1e-9 px of an edge of that view (the other coordinate inside), or the two best cw
    among the containing views within 1e-12 relative -- and `closest`, the smallest such distance met in px."""
    us = [np.ascontiguousarray(u).view(np.float32).reshape(40) for u in uniforms_list]
    east, north, up = local_frame(us[0][32:35])
    az, el = angles(params)
    a, e = np.radians(az)[None, :, None], np.radians(el)[:, None, None]
    d = np.cos(e) * (np.sin(a) * east + np.cos(a) * north) + np.sin(e) * up      # (H, W, 3)
    H, W = d.shape[:2]
    n = len(us)
    cw_all, px_all, py_all = (np.zeros((n, H, W)) for _ in range(3))
    inside = np.zeros((n, H, W), bool)
    fragile = np.zeros((H, W), bool)
    closest = np.inf
    with np.errstate(all="ignore"):
        for k, u in enumerate(us):
            m = u[:16].astype(np.float64).reshape(4, 4).T      # m[row, col]
            cx, cy, cw = d @ m[0, :3], d @ m[1, :3], d @ m[3, :3]
            px, py = (cx / cw + 1.0) * src_w / 2.0, (1.0 - cy / cw) * src_h / 2.0
            cw_all[k], px_all[k], py_all[k] = cw, px, py
            inside[k] = (cw > 0) & (px >= 0) & (px < src_w) & (py >= 0) & (py < src_h)
            ex = np.minimum(np.abs(px), np.abs(px - src_w))
            ey = np.minimum(np.abs(py), np.abs(py - src_h))
            near_x = (cw > 0) & (py > -1e-9) & (py < src_h + 1e-9)
            near_y = (cw > 0) & (px > -1e-9) & (px < src_w + 1e-9)
            fragile |= (near_x & (ex < 1e-9)) | (near_y & (ey < 1e-9))
            for mask, dist in ((near_x, ex), (near_y, ey)):
                if mask.any():
                    closest = min(closest, float(dist[mask].min()))
    score = np.where(inside, cw_all, -np.inf)
    view = np.argmax(score, axis=0)                              # the first maximum: the lowest index on a tie
    has = inside.any(axis=0)
    yy, xx = np.mgrid[0:H, 0:W]
    px, py = px_all[view, yy, xx], py_all[view, yy, xx]
    top2 = np.sort(score, axis=0)[-2:] if n > 1 else None
    if top2 is not None:
        with np.errstate(all="ignore"):
            both = np.isfinite(top2[0])
            fragile |= both & (np.abs(top2[1] - top2[0]) <= 1e-12 * np.abs(top2[1]))
    fx, fy = np.abs(px - np.round(px)), np.abs(py - np.round(py))
    fragile |= has & ((fx < 1e-9) | (fy < 1e-9))
    if has.any():
        closest = min(closest, float(fx[has].min()), float(fy[has].min()))
    view = np.where(has, view, -1)
    sx, sy = np.floor(px).astype(np.int64), np.floor(py).astype(np.int64)
    src = np.where(has, (view.astype(np.int64) * src_h + sy) * src_w + sx, -1).astype(np.int32)
    return {"view": view, "px": np.where(has, px, np.nan), "py": np.where(has, py, np.nan), "src": src, "n_containing": inside.sum(axis=0),
            "fragile": fragile, "closest": closest, "az": az, "el": el}


def gather(src_map, layer, fill):
    """A per-texel layer of the views (n, src_h, src_w[, c]) carried across through the source map; `fill` where it is -1."""
    flat = layer.reshape((-1,) + layer.shape[3:])
    out = flat[np.clip(src_map, 0, None)]
    out[src_map < 0] = fill
    return out


def srgb_decode(c8):
    c = np.asarray(c8, np.float64) / 255.0
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)


def srgb_encode(lin):
    l = np.clip(lin, 0.0, 1.0)
    s = np.where(l <= 0.0031308, 12.92 * l, 1.055 * l ** (1.0 / 2.4) - 0.055)
    return np.floor(s * 255.0 + 0.5).astype(np.uint8)


def bilinear(loc, rgba_src, srgb):
    """The bilinear colour of every pixel `loc` (locate's result) has a source for; 0 0 0 0 elsewhere.  rgba_src (n, h, w, 4) u8."""
    n, h, w, _ = rgba_src.shape
    has = loc["view"] >= 0
    v = np.where(has, loc["view"], 0)
    u_, v_ = np.where(has, loc["px"], 0.5) - 0.5, np.where(has, loc["py"], 0.5) - 0.5
    x0, y0 = np.floor(u_), np.floor(v_)
    wx, wy = np.floor((u_ - x0) * 256.0) / 256.0, np.floor((v_ - y0) * 256.0) / 256.0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    xa, xb = np.clip(x0, 0, w - 1), np.clip(x0 + 1, 0, w - 1)
    ya, yb = np.clip(y0, 0, h - 1), np.clip(y0 + 1, 0, h - 1)
    out = np.zeros(has.shape + (4,), np.uint8)
    for ch in range(4):
        lin = not srgb or ch == 3
        dec = (lambda c: c.astype(np.float64) / 255.0) if lin else srgb_decode
        t00, t10, t01, t11 = (dec(rgba_src[v, y, x, ch]) for y, x in ((ya, xa), (ya, xb), (yb, xa), (yb, xb)))
        val = (t00 * (1 - wx) + t10 * wx) * (1 - wy) + (t01 * (1 - wx) + t11 * wx) * wy
        out[..., ch] = np.floor(np.clip(val, 0, 1) * 255.0 + 0.5).astype(np.uint8) if lin else srgb_encode(val)
    out[~has] = 0
    return out
