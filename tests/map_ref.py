"""An independent numpy f64 reference of the map view (topo_map_*).  It shares no code with csrc/topo_map.h.

The surface under a pixel and its winning (tile, triangle, weights) come from tests/surface_ref.py (every point against every
triangle).  The relief is restated here: the three vertex normals of the winning triangle, 2 c / 255 - 1 per channel, rotated by the
tile's normal_to_world rotation Rz(model_lon) Ry(90 - model_lat) in f64 (the f32 model point widened), interpolated with
(1 - u - v, u, v), normalised; linear = 0.01 + 0.7 max(n . sun, 0); the code is the closed sRGB formula, round(255 s).  Levels are
numpy.floor(height / interval); a pixel is on a contour iff its level differs from that of its east or south neighbour, void and
outside neighbours taking no part; on an index contour iff floor(max / n) > floor(min / n) for one differing pair.  Seen: the mask
bit of (winning tile, winning cell).

A pixel is AMBIGUOUS iff its own f64 height or that of a neighbour it is compared with lies within 1e-3 m of a multiple of the
interval, or surface_ref calls it or such a neighbour triangle- or kind-ambiguous: another implementation's rounding may decide it
the other way."""
from __future__ import annotations

import numpy as np

import surface_ref as SR
from oracle import ray_check as RC

RELIEF, CONTOURS, SEEN = 1, 2, 4
F_TERRAIN, F_CONTOUR, F_INDEX, F_SEEN = 1, 2, 4, 8
NEAR_LEVEL = 1e-3      # metres


def positions(p):
    """(ny, nx, 2) lon / lat of the pixels: one rounded product and one rounded sum each."""
    lon = np.float64(p["lon0_deg"][0]) + np.arange(int(p["nx"][0]), dtype=np.float64) * np.float64(p["dlon_deg"][0])
    lat = np.float64(p["lat0_deg"][0]) + np.arange(int(p["ny"][0]), dtype=np.float64) * np.float64(p["dlat_deg"][0])
    return np.stack(np.broadcast_arrays(lon[None, :], lat[:, None]), axis=-1)


def rotation(model_point):
    lon, lat = (np.radians(np.float64(np.float32(v))) for v in (model_point[0], np.float32(90.0) - np.float32(model_point[1])))
    rz = np.array([[np.cos(lon), -np.sin(lon), 0.0], [np.sin(lon), np.cos(lon), 0.0], [0.0, 0.0, 1.0]])
    ry = np.array([[np.cos(lat), 0.0, np.sin(lat)], [0.0, 1.0, 0.0], [-np.sin(lat), 0.0, np.cos(lat)]])
    return rz @ ry


def srgb_code(lin):
    lin = np.asarray(lin, np.float64)
    s = np.where(lin <= 0.0031308, 12.92 * lin, 1.055 * np.power(np.maximum(lin, 1e-30), 1.0 / 2.4) - 0.055)
    return np.floor(255.0 * np.clip(s, 0.0, 1.0) + 0.5).astype(np.int64)


def blend(c, s):
    """(..., 3) colour c blended with the R G B A quadruple s by its alpha, in integers."""
    a = int(s[3])
    return (c.astype(np.int64) * (255 - a) + np.asarray(s[:3], np.int64) * a + 127) // 255


def reference(tiles, normals, params, masks=None):
    """-> dict: flags (ny, nx) u8, grey (ny, nx) i64 (the relief code; 255 with the layer off), rgba (ny, nx, 4) u8 from the
    reference's own flags and grey, ambiguous (ny, nx) bool, terrain (ny, nx) bool."""
    p = params
    nx, ny, layers = int(p["nx"][0]), int(p["ny"][0]), int(p["layers"][0])
    interval, every = float(p["contour_interval_m"][0]), int(p["index_every"][0])
    pts = positions(p).reshape(-1, 2)
    if len(tiles):
        rec = SR.surface(SR.Mesh(tiles), pts).reshape(ny, nx)
    else:
        rec = np.zeros((ny, nx), SR.OUT_DTYPE)
    terrain = rec["kind"] == SR.TERRAIN
    amb = rec["tri_ambiguous"] | rec["kind_ambiguous"]
    flags = np.where(terrain, F_TERRAIN, 0).astype(np.uint8)
    grey = np.full((ny, nx), 255, np.int64)
    if layers & RELIEF and terrain.any():
        sun = np.asarray(p["sun_direction"][0], np.float32).astype(np.float64)
        for r, (hts, rp, mp, ps) in enumerate(tiles):
            sel = terrain & (rec["rank"] == r)
            if not sel.any():
                continue
            h, w = hts.shape
            tri = RC.tile_triangles(w, h)[rec["tri"][sel]]      # (n, 3, 2): x, y of the three vertices
            tex = np.asarray(normals[r], np.uint8).reshape(h, w, 4)[..., :3].astype(np.float64)
            nv = 2.0 * tex[tri[:, :, 1], tri[:, :, 0]] / 255.0 - 1.0      # (n, 3 vertices, 3)
            nv = nv @ rotation(np.asarray(mp, np.float32)).T
            u, v = rec["u"][sel], rec["v"][sel]
            n = nv[:, 0] * (1.0 - u - v)[:, None] + nv[:, 1] * u[:, None] + nv[:, 2] * v[:, None]
            n /= np.linalg.norm(n, axis=1)[:, None]
            grey[sel] = srgb_code(0.01 + 0.7 * np.maximum(n @ sun, 0.0))
    if layers & SEEN and masks is not None and terrain.any():
        for r, (hts, *_) in enumerate(tiles):
            sel = terrain & (rec["rank"] == r)
            if not sel.any():
                continue
            hm1 = hts.shape[0] - 1
            cell = rec["tri"][sel] >> 1
            seen = np.asarray(masks[r], bool)[cell % hm1, cell // hm1]
            f = flags[sel]
            f[seen] |= F_SEEN
            flags[sel] = f
    if layers & CONTOURS and interval > 0.0:
        with np.errstate(invalid="ignore"):
            level = np.floor(rec["height_m"] / interval)
            near = terrain & (np.abs(rec["height_m"] - np.round(rec["height_m"] / interval) * interval) <= NEAR_LEVEL)
        shaky = amb | near
        for dy, dx in ((0, 1), (1, 0)):
            a, b = level[:ny - dy, :nx - dx], level[dy:, dx:]
            both = terrain[:ny - dy, :nx - dx] & terrain[dy:, dx:]
            differ = both & (a != b)
            index = differ & (np.floor(np.maximum(a, b) / every) > np.floor(np.minimum(a, b) / every)) if every else np.zeros_like(differ)
            flags[:ny - dy, :nx - dx] |= np.where(differ, F_CONTOUR, 0).astype(np.uint8) | np.where(index, F_INDEX, 0).astype(np.uint8)
            amb[:ny - dy, :nx - dx] |= shaky[dy:, dx:]
        amb |= shaky
    rgba = np.zeros((ny, nx, 4), np.uint8)
    rgba[...] = np.asarray(p["void_rgba"][0], np.uint8)
    col = np.repeat(grey[..., None], 3, axis=-1)
    seen = (flags & F_SEEN) != 0
    col[seen] = blend(col[seen], p["seen_rgba"][0])
    on = (flags & F_CONTOUR) != 0
    idx = (flags & F_INDEX) != 0
    col[on & ~idx] = blend(col[on & ~idx], p["contour_rgba"][0])
    col[idx] = blend(col[idx], p["index_rgba"][0])
    rgba[terrain, :3] = col[terrain].astype(np.uint8)
    rgba[terrain, 3] = 255
    return {"flags": flags, "grey": grey, "rgba": rgba, "ambiguous": amb, "terrain": terrain}
