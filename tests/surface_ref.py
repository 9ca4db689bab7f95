"""An independent numpy f64 brute-force reference of the surface queries (topo_surface_*, topo_profile_*): every point against
every triangle.

Vertices and topology come from oracle/ray_check.py (tile_vertices, tile_triangles), as los_ref.Mesh; the rule is the one
include/topo_hip.h states: a triangle exists iff its three vertex heights are finite, < 1e9 and > -R0; the line under the unit
direction u of (lon, lat) has origin R0 u and direction u; Moeller-Trumbore on vertices translated by the origin; hit iff u >= -e,
v >= -e, u + v <= 1 + e with e = 2^-30, t finite and -R0 < t < 1e9; the LARGEST t wins, then the earlier tile in draw order, then the
lower triangle index; a tile whose pixel scale is zero or not finite in x or y has no surface.  slope = acos(n^ . u) with n turned to
the side of u; aspect = the azimuth of the horizontal part of n^.

Every point is evaluated three times, with the barycentric bounds at e, loosened to 1e-6 and tightened to -1e-6: a point whose
winner (tile, triangle) differs between those is TRIANGLE-AMBIGUOUS, one for which they differ on hit or no hit KIND-AMBIGUOUS --
the f64 rounding of another implementation may legitimately decide it the other way."""
from __future__ import annotations

import numpy as np

from oracle import ray_check as RC

R0 = RC.R0
TERRAIN, NONE, INVALID = 1, 0, -1
EDGE = 2.0 ** -30
EPS_BARY = 1e-6
ABSURD = 1.0e9
OUT_DTYPE = np.dtype([("kind", "<i4"), ("height_m", "<f8"), ("rank", "<i8"), ("tri", "<i8"), ("u", "<f8"), ("v", "<f8"), ("slope_deg", "<f8"), ("aspect_deg", "<f8"),
                      ("tri_ambiguous", "?"), ("kind_ambiguous", "?")])


class Mesh:
    """tiles: [(heights f32 (h, w), raster_point, model_point, pixel_scale)] in draw order."""

    def __init__(self, tiles):
        v0, v1, v2, rank, tri = [], [], [], [], []
        for r, (hts, rp, mp, ps) in enumerate(tiles):
            h, w = hts.shape
            scale = np.asarray(ps, np.float32).astype(np.float64)
            if not (np.isfinite(scale).all() and (scale != 0).all()):      # a tile with a zero or non-finite pixel scale has no surface
                continue
            with np.errstate(all="ignore"):
                P = RC.tile_vertices(hts, rp, mp, ps)
                h64 = hts.astype(np.float64)
                ok = np.isfinite(h64) & (h64 < ABSURD) & (h64 > -R0)
            T = RC.tile_triangles(w, h)
            exists = ok[T[:, 0, 1], T[:, 0, 0]] & ok[T[:, 1, 1], T[:, 1, 0]] & ok[T[:, 2, 1], T[:, 2, 0]]
            idx = np.nonzero(exists)[0]
            v0.append(P[T[idx, 0, 1], T[idx, 0, 0]])
            v1.append(P[T[idx, 1, 1], T[idx, 1, 0]])
            v2.append(P[T[idx, 2, 1], T[idx, 2, 0]])
            rank.append(np.full(len(idx), r, np.int64))
            tri.append(idx.astype(np.int64))
        self.v0, self.v1, self.v2 = np.concatenate(v0), np.concatenate(v1), np.concatenate(v2)
        self.rank, self.tri = np.concatenate(rank), np.concatenate(tri)      # ascending (rank, tri): argmax's first maximum is the tie rule
        self.tile_h, self.tile_w = tiles[0][0].shape


def direction(lon_deg, lat_deg):
    lo, la = np.radians(np.asarray(lon_deg, np.float64)), np.radians(np.asarray(lat_deg, np.float64))
    return np.stack([np.cos(la) * np.cos(lo), np.cos(la) * np.sin(lo), np.sin(la)], axis=-1)


def under(mesh, u_all, chunk=96):
    """The terrain under unit directions u_all (n, 3) -> OUT_DTYPE records (kind TERRAIN or NONE)."""
    n = len(u_all)
    out = np.zeros(n, OUT_DTYPE)
    E1, E2 = mesh.v1 - mesh.v0, mesh.v2 - mesh.v0
    N = np.cross(E1, E2)
    for lo in range(0, n, chunk):
        d = u_all[lo:lo + chunk]
        o = R0 * d
        with np.errstate(all="ignore"):
            tx, ty, tz = (o[:, k, None] - mesh.v0[None, :, k] for k in range(3))
            dx, dy, dz = (d[:, k, None] for k in range(3))
            ax, ay, az = (E1[None, :, k] for k in range(3))
            bx, by, bz = (E2[None, :, k] for k in range(3))
            px, py, pz = dy * bz - dz * by, dz * bx - dx * bz, dx * by - dy * bx
            inv = 1.0 / (ax * px + ay * py + az * pz)
            u = (tx * px + ty * py + tz * pz) * inv
            qx, qy, qz = ty * az - tz * ay, tz * ax - tx * az, tx * ay - ty * ax
            v = (dx * qx + dy * qy + dz * qz) * inv
            t = (bx * qx + by * qy + bz * qz) * inv
            in_t = np.isfinite(t) & (t > -R0) & (t < ABSURD)
            win = []
            for e in (EDGE, EPS_BARY, -EPS_BARY):      # the rule, loosened, tightened
                hit = (u >= -e) & (v >= -e) & (u + v <= 1.0 + e) & in_t
                tt = np.where(hit, t, -np.inf)
                j = tt.argmax(axis=1)
                win.append(np.where(np.isfinite(tt[np.arange(len(d)), j]), j, -1))
        j = win[0]
        rows = np.arange(len(d))
        is_hit = j >= 0
        jj = np.where(is_hit, j, 0)
        n_w = N[jj]
        nu = np.einsum("ck,ck->c", n_w, d)
        n_w = np.where((nu < 0)[:, None], -n_w, n_w)
        nh = n_w / np.linalg.norm(n_w, axis=1)[:, None]
        slope = np.degrees(np.arccos(np.clip(np.einsum("ck,ck->c", nh, d), -1.0, 1.0)))
        hxy = np.hypot(d[:, 0], d[:, 1])
        with np.errstate(all="ignore"):
            east = np.where((hxy > 0)[:, None], np.stack([-d[:, 1] / hxy, d[:, 0] / hxy, 0.0 * hxy], axis=-1), np.array([0.0, 1.0, 0.0]))
        north = np.cross(d, east)
        aspect = np.degrees(np.arctan2(np.einsum("ck,ck->c", nh, east), np.einsum("ck,ck->c", nh, north))) % 360.0
        rec = out[lo:lo + chunk]
        rec["kind"] = np.where(is_hit, TERRAIN, NONE)
        rec["height_m"] = np.where(is_hit, t[rows, jj], 0.0)
        rec["rank"] = np.where(is_hit, mesh.rank[jj], -1)
        rec["tri"] = np.where(is_hit, mesh.tri[jj], -1)
        rec["u"] = np.where(is_hit, u[rows, jj], 0.0)
        rec["v"] = np.where(is_hit, v[rows, jj], 0.0)
        rec["slope_deg"] = np.where(is_hit, slope, 0.0)
        rec["aspect_deg"] = np.where(is_hit, aspect, 0.0)
        rec["tri_ambiguous"] = (win[1] != win[2]) | (win[0] != win[1])
        rec["kind_ambiguous"] = ((win[1] >= 0) != (win[2] >= 0))
        out[lo:lo + chunk] = rec
    return out


def surface(mesh, lonlat):
    """(n, 2) degrees -> OUT_DTYPE records."""
    p = np.asarray(lonlat, np.float64).reshape(-1, 2)
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(p[:, 0]) & np.isfinite(p[:, 1]) & (np.abs(p[:, 1]) <= 90.0)
    out = np.zeros(len(p), OUT_DTYPE)
    out["kind"] = INVALID
    out["rank"] = out["tri"] = -1
    if valid.any():
        out[valid] = under(mesh, direction(p[valid, 0], p[valid, 1]))
    return out


def sample_points(segs, m):
    """The samples of segments (records with origin, dir, t_min, t_max): (positions (n, m, 3), line heights (n, m))."""
    f = np.arange(m, dtype=np.float64) / np.float64(m - 1)
    tk = segs["t_min"][:, None] + (segs["t_max"] - segs["t_min"])[:, None] * f[None, :]
    p = np.asarray(segs["origin"], np.float64)[:, None, :] + tk[..., None] * np.asarray(segs["dir"], np.float64)[:, None, :]
    return p, np.linalg.norm(p, axis=-1) - R0


def profile(mesh, segs, m):
    """(terrain (n, m) f64, NaN where there is none; line (n, m) f64; kind-ambiguous (n, m)) of valid segments."""
    p, line = sample_points(segs, m)
    u = (p / np.linalg.norm(p, axis=-1)[..., None]).reshape(-1, 3)
    rec = under(mesh, u)
    terrain = np.where(rec["kind"] == TERRAIN, rec["height_m"], np.nan).reshape(len(segs), m)
    return terrain, line, rec["kind_ambiguous"].reshape(len(segs), m)


def reduce_samples(samples):
    """The summary the stored samples (n, m, 2) f32 imply: (min clearance f32, NaN for none; its first sample, 0xFFFFFFFF for none;
    the number of samples with terrain).  The clearance of a sample is the f32 difference line - terrain."""
    s = np.asarray(samples, np.float32)
    has = ~np.isnan(s[..., 0])
    with np.errstate(invalid="ignore"):
        c = (s[..., 1] - s[..., 0]).astype(np.float32)
    big = np.where(has, c, np.float32(np.inf))
    k = big.argmin(axis=1)      # the first of equal values
    any_t = has.any(axis=1)
    least = np.where(any_t, c[np.arange(len(s)), k], np.float32(np.nan)).astype(np.float32)
    return least, np.where(any_t, k, 0xFFFFFFFF).astype(np.uint32), has.sum(axis=1).astype(np.uint32)
