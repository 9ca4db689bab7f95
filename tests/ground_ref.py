"""Expected ground points (topo_ground_*) from per-pixel winners (the oracle's render_winners()), the tiles and camera_proj: a
vectorised numpy f64 reference of the definition in include/topo_hip.h, written the OTHER way round from the product's
topo_ground.h -- the pixel centre's ray is unprojected from the matrix (eye: where clip x, y, w vanish; direction: what maps to
(gx, gy, . , 1)) and intersected with the winning triangle's plane, where the product solves for clip-space adjugate weights.
Vertices and topology come from oracle/ray_check.py (tile_vertices, tile_triangles), not from the product."""
from __future__ import annotations

import numpy as np

from oracle import ray_check as RC
from viewshed_ref import NO_TRI, geo_order

R0 = RC.R0
NAN_BITS = 0x7FC00000
EXACT = ("kind", "tile_lat_deg", "tile_lon_deg", "cell_x", "cell_y", "tri", "depth")      # what the winners and depths determine


def scene_tiles(sc):
    """[(heights, raster_point, model_point, pixel_scale)] of a scenes.Scene in draw order, the six tile values as f32."""
    return [(sc.heights[l],) + tuple(np.asarray(a, np.float32) for a in sc.transform(l)) for l in geo_order(sc.locs)]


def ground(depth, winners, tiles, locs, uniforms):
    """One view.  depth (H, W) f32, winners (H, W) u32 (rank * 2(w-1)(h-1) + triangle, NO_TRI = sky), tiles in draw order
    (scene_tiles), locs the tile set, uniforms the view's 160-byte block -> {field: (H, W) array}: the exact fields, lon_deg /
    lat_deg / height_m / range_m / w1 / w2 in f64, the ECEF point `p` (H, W, 3), and `finite`."""
    depth = np.asarray(depth, np.float32)
    win = np.asarray(winners, np.uint32)
    H, W = win.shape
    u = np.ascontiguousarray(uniforms).view(np.float32).reshape(-1)
    M = u[:16].astype(np.float64).reshape(4, 4).T          # column-major -> [row, col]
    cam = u[32:35].astype(np.float64)
    terrain = win != NO_TRI
    th, tw = tiles[0][0].shape
    tris = 2 * (tw - 1) * (th - 1)
    ids = np.where(terrain, win, 0).astype(np.int64)
    rank, tri = ids // tris, ids % tris
    cell = tri >> 1
    order = geo_order(locs)
    T = RC.tile_triangles(tw, th)
    v = np.zeros((3, H, W, 3))
    for r, (hts, rp, mp, ps) in enumerate(tiles):
        sel = terrain & (rank == r)
        if not sel.any():
            continue
        with np.errstate(all="ignore"):
            P = RC.tile_vertices(np.asarray(hts, np.float32), rp, mp, ps)
        t = T[tri[sel]]                                     # (n, 3, 2) (i, j) vertex ids
        for k in range(3):
            v[k][sel] = P[t[:, k, 1], t[:, k, 0]]
    # the ray of every pixel centre, from the matrix alone
    R = M[[0, 1, 3], :3]
    eye = np.linalg.solve(R, -M[[0, 1, 3], 3])
    gx = (np.arange(W) + 0.5) * 2.0 / W - 1.0
    gy = 1.0 - (np.arange(H) + 0.5) * 2.0 / H
    rhs = np.stack(np.broadcast_arrays(gx[None, :], gy[:, None], np.ones((H, W))), axis=-1)
    d = np.linalg.solve(R, rhs.reshape(-1, 3).T).T.reshape(H, W, 3)
    e1, e2 = v[1] - v[0], v[2] - v[0]
    nrm = np.cross(e1, e2)
    with np.errstate(all="ignore"):
        s = np.einsum("hwk,hwk->hw", nrm, v[0] - eye) / np.einsum("hwk,hwk->hw", nrm, d)
        p = eye + s[..., None] * d
        # barycentric weights in the triangle's plane
        r = p - v[0]
        a11, a12, a22 = (e1 * e1).sum(-1), (e1 * e2).sum(-1), (e2 * e2).sum(-1)
        b1, b2 = (r * e1).sum(-1), (r * e2).sum(-1)
        det = a11 * a22 - a12 * a12
        w1, w2 = (b1 * a22 - b2 * a12) / det, (b2 * a11 - b1 * a12) / det
        norm = np.linalg.norm(p, axis=-1)
        lon, lat = np.degrees(np.arctan2(p[..., 1], p[..., 0])), np.degrees(np.arcsin(p[..., 2] / norm))
        height, rng = norm - R0, np.linalg.norm(p - cam, axis=-1)
    finite = terrain & np.isfinite(lon) & np.isfinite(lat) & np.isfinite(height) & np.isfinite(rng) & np.isfinite(w1) & np.isfinite(w2)
    lats = np.array([o[0] for o in order], np.int32)
    lons = np.array([o[1] for o in order], np.int32)
    z = lambda a, dt=np.float64: np.where(finite, a, 0).astype(dt)
    return {"kind": np.where(terrain, np.where(finite, 1, -3), 0).astype(np.int32),
            "depth": np.where(terrain, depth, np.float32(1.0)).astype(np.float32),
            "tile_lat_deg": np.where(terrain, lats[np.minimum(rank, len(order) - 1)], 0).astype(np.int32),
            "tile_lon_deg": np.where(terrain, lons[np.minimum(rank, len(order) - 1)], 0).astype(np.int32),
            "cell_x": np.where(terrain, cell // (th - 1), 0).astype(np.uint32),
            "cell_y": np.where(terrain, cell % (th - 1), 0).astype(np.uint32),
            "tri": np.where(terrain, tri & 1, 0).astype(np.uint32),
            "lon_deg": z(lon), "lat_deg": z(lat), "height_m": z(height), "range_m": z(rng), "w1": z(w1), "w2": z(w2),
            "p": np.where(finite[..., None], p, 0.0), "finite": finite, "terrain": terrain}


def ecef(lon_deg, lat_deg, height):
    """The ECEF point of (lon, lat, height): what a record's three values say, for comparison in metres."""
    lo, la = np.radians(np.asarray(lon_deg, np.float64)), np.radians(np.asarray(lat_deg, np.float64))
    r = R0 + np.asarray(height, np.float64)
    return np.stack([r * np.cos(la) * np.cos(lo), r * np.cos(la) * np.sin(lo), r * np.sin(la)], axis=-1)


def compare(got, want, what, f64=None, tol_m=1e-3, tol_w=1e-6):
    """got: (H, W) GROUND_DTYPE records (or a dict of such arrays); want: ground()'s dict.  Asserts the exact fields, the ECEF point
    rebuilt from (lon, lat, height), the height and the range within tol_m and the weights within tol_w; returns the maxima measured.
    f64: {"height_m", "range_m", "w1", "w2"} in f64 where the caller has them (the CPU emulation returns the lane function's own
    values); then nothing is added to the tolerances.  A record holds range and weights as f32: half an f32 ulp of the expected
    value -- the record format's rounding, 3.9e-3 m at 100 km, 3e-8 for a weight near 1 -- is then allowed on top for those two;
    the point and the height stay at tol_m (an f32 height below 4096 m is within 1.3e-4 m of the f64 one)."""
    for f in EXACT:
        g, w = np.asarray(got[f]), want[f]
        if f == "depth":
            g, w = g.astype(np.float32).view(np.uint32), w.view(np.uint32)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, f"{what}: {f} differs in {len(bad)} pixels (first {tuple(bad[0])}: got {got[f][tuple(bad[0])]}, want {want[f][tuple(bad[0])]})"
    assert np.isin(np.asarray(got["fan"]), (0, 1)).all(), what
    t = want["kind"] == 1
    out = {"pixels": int(t.size), "terrain": int(t.sum())}
    for f in ("lon_deg", "lat_deg", "height_m", "range_m", "w1", "w2"):
        assert (np.asarray(got[f])[~t] == 0).all(), f"{what}: {f} is not 0 where there is no terrain point"
    if not t.any():
        return out
    val = lambda f: np.asarray((got if f64 is None else f64)[f], np.float64)
    half_ulp = (lambda a: 0.0 * a) if f64 is not None else (lambda a: 0.5 * np.spacing(np.abs(a).astype(np.float32)).astype(np.float64))
    dp = np.linalg.norm(ecef(got["lon_deg"], got["lat_deg"], val("height_m")) - want["p"], axis=-1)
    dh = np.abs(val("height_m") - want["height_m"])
    dr = np.abs(val("range_m") - want["range_m"]) - half_ulp(want["range_m"])
    dw = np.maximum(np.abs(val("w1") - want["w1"]) - half_ulp(want["w1"]), np.abs(val("w2") - want["w2"]) - half_ulp(want["w2"]))
    out.update(point_m=float(dp[t].max()), height_m=float(dh[t].max()), range_m=float(dr[t].max()), w=float(dw[t].max()),
               point_over_range=float((dp / want["range_m"].clip(1.0))[t].max()),
               min_bary=float(np.minimum(np.minimum(want["w1"], want["w2"]), 1.0 - want["w1"] - want["w2"])[t].min()))
    print(f"{what}: {out}")
    assert out["point_m"] <= tol_m and out["height_m"] <= tol_m and out["range_m"] <= tol_m, f"{what}: {out}"
    assert out["w"] <= tol_w, f"{what}: {out}"
    return out


def all_pixels(topo, views, W, H):
    """Queries for every pixel of the given view indices, view-major then row-major."""
    v, y, x = np.meshgrid(np.asarray(views), np.arange(H), np.arange(W), indexing="ij")
    return topo.ground_queries(np.stack([v.ravel(), x.ravel(), y.ravel()], axis=-1))


def assert_sky(got, what):
    sky = got[got["kind"] == 0]
    assert (sky["depth"] == 1.0).all(), what
    blank = sky.copy()
    blank["depth"] = 0
    assert not blank.view(np.uint8).any(), f"{what}: a sky record carries something besides depth 1.0"


def assert_map_is_list(vals, rec, what):
    """vals (..., 4) f32 of the map, rec (...) list records of the same pixels: np.float32 of the record bit for bit, NaN elsewhere."""
    t = rec["kind"] == 1
    want = np.stack([rec["lon_deg"].astype(np.float32), rec["lat_deg"].astype(np.float32), rec["height_m"], rec["range_m"]], axis=-1).view(np.uint32)
    want = np.where(t[..., None], want, np.uint32(NAN_BITS))
    bad = np.argwhere(vals.view(np.uint32) != want)
    assert len(bad) == 0, f"{what}: the map differs from the list in {len(bad)} values (first {tuple(bad[0])}: {vals[tuple(bad[0])]!r} vs record {rec[tuple(bad[0][:-1])]})"
