"""An independent numpy f64 brute-force reference of the ray queries (topo_raycast_*): every ray against every triangle.

Vertices and topology come from oracle/ray_check.py (tile_vertices, tile_triangles); the rule is the one include/topo_hip.h states:
Moeller-Trumbore on vertices translated by the ray's origin, both faces, hit iff u >= 0, v >= 0, u + v <= 1, t_min <= t <= t_max and t
finite; the smallest t wins, then the earlier tile in draw order, then the lower triangle index; a triangle with a non-finite vertex
height does not exist.

Every ray is evaluated twice more, with the barycentric bounds loosened and tightened by 1e-6: a ray whose winner differs between the
two, or whose winning triangle it meets at |n . d| < 1e-3 (unit vectors), is AMBIGUOUS -- the f64 rounding of another implementation
may legitimately decide it the other way -- and is excluded from the comparisons; the tests cap the excluded share at 0.5 %."""
from __future__ import annotations

import numpy as np

from oracle import ray_check as RC

R0 = RC.R0
HIT, MISS, INVALID = 1, 0, -1
EPS_BARY = 1e-6
MIN_ND = 1e-3
OUT_DTYPE = np.dtype([("kind", "<i4"), ("t", "<f8"), ("rank", "<i8"), ("tri", "<i8"), ("front", "<u4"), ("u", "<f8"), ("v", "<f8"), ("ambiguous", "?"), ("any_ambiguous", "?")])


def geo_order(locs):
    """Draw order: the reference's BTreeMap order over (latitude degree, S < N, longitude degree, W < E)."""
    return sorted(locs, key=lambda l: (abs(l[0]), l[0] > 0, abs(l[1]), l[1] > 0))


class Mesh:
    """tiles: [(heights f32 (h, w), raster_point, model_point, pixel_scale)] in draw order."""

    def __init__(self, tiles):
        v0, v1, v2, rank, tri = [], [], [], [], []
        for r, (hts, rp, mp, ps) in enumerate(tiles):
            h, w = hts.shape
            with np.errstate(all="ignore"):
                P = RC.tile_vertices(hts, rp, mp, ps)
            T = RC.tile_triangles(w, h)
            ok = np.isfinite(hts.astype(np.float64))
            exists = ok[T[:, 0, 1], T[:, 0, 0]] & ok[T[:, 1, 1], T[:, 1, 0]] & ok[T[:, 2, 1], T[:, 2, 0]]
            idx = np.nonzero(exists)[0]
            v0.append(P[T[idx, 0, 1], T[idx, 0, 0]])
            v1.append(P[T[idx, 1, 1], T[idx, 1, 0]])
            v2.append(P[T[idx, 2, 1], T[idx, 2, 0]])
            rank.append(np.full(len(idx), r, np.int64))
            tri.append(idx.astype(np.int64))
        self.v0, self.v1, self.v2 = np.concatenate(v0), np.concatenate(v1), np.concatenate(v2)
        self.rank, self.tri = np.concatenate(rank), np.concatenate(tri)      # ascending (rank, tri): argmin's first minimum is the tie rule
        self.tile_h, self.tile_w = tiles[0][0].shape
        tris = 2 * (self.tile_w - 1) * (self.tile_h - 1)
        self.where = np.full((len(tiles), tris), -1, np.int64)      # (rank, triangle) -> its row here, -1: it does not exist
        self.where[self.rank, self.tri] = np.arange(len(self.rank))


def cast(mesh, rays, chunk=96, skip=None, open_t_min=False):
    """rays: records with origin, dir, t_min, t_max -> OUT_DTYPE records.  skip: (n, 2) (rank, triangle) of one triangle per ray that
    does not count; open_t_min: a hit needs t > t_min.  `ambiguous` is about the WINNER; `any_ambiguous` about whether there is a hit
    at all (the shadow rays' question)."""
    n = len(rays)
    out = np.zeros(n, OUT_DTYPE)
    o_all, d_all = np.asarray(rays["origin"], np.float64), np.asarray(rays["dir"], np.float64)
    tmin, tmax = np.asarray(rays["t_min"], np.float64), np.asarray(rays["t_max"], np.float64)
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(o_all).all(axis=1) & np.isfinite(d_all).all(axis=1) & (d_all != 0).any(axis=1) & (tmin <= tmax)
    out["kind"] = np.where(valid, MISS, INVALID)
    E1, E2 = mesh.v1 - mesh.v0, mesh.v2 - mesh.v0
    N = np.cross(E1, E2)
    Nn = N / np.linalg.norm(N, axis=1)[:, None]
    ids = np.nonzero(valid)[0]
    for lo in range(0, len(ids), chunk):
        k = ids[lo:lo + chunk]
        o, d = o_all[k], d_all[k]
        with np.errstate(all="ignore"):
            # component by component ((rays, triangles) planes: several times faster than np.cross / einsum on (c, n, 3) blocks)
            tx, ty, tz = (o[:, k, None] - mesh.v0[None, :, k] for k in range(3))      # origin - v0 = -(v0 translated by the origin)
            dx, dy, dz = (d[:, k, None] for k in range(3))
            ax, ay, az = (E1[None, :, k] for k in range(3))
            bx, by, bz = (E2[None, :, k] for k in range(3))
            px, py, pz = dy * bz - dz * by, dz * bx - dx * bz, dx * by - dy * bx      # pvec = d x e2
            inv = 1.0 / (ax * px + ay * py + az * pz)
            u = (tx * px + ty * py + tz * pz) * inv
            qx, qy, qz = ty * az - tz * ay, tz * ax - tx * az, tx * ay - ty * ax      # qvec = tvec x e1
            v = (dx * qx + dy * qy + dz * qz) * inv
            t = (bx * qx + by * qy + bz * qz) * inv
            in_t = ((t > tmin[k][:, None]) if open_t_min else (t >= tmin[k][:, None])) & (t <= tmax[k][:, None]) & np.isfinite(t)
            if skip is not None:
                at = mesh.where[skip[k, 0], skip[k, 1]]
                in_t[np.nonzero(at >= 0)[0], at[at >= 0]] = False
            win = []
            for e in (0.0, EPS_BARY, -EPS_BARY):      # exact, loosened, tightened
                hit = (u >= -e) & (v >= -e) & (u + v <= 1.0 + e) & in_t
                tt = np.where(hit, t, np.inf)
                j = tt.argmin(axis=1)
                win.append(np.where(np.isfinite(tt[np.arange(len(k)), j]), j, -1))
        j = win[0]
        rows = np.arange(len(k))
        is_hit = j >= 0
        jj = np.where(is_hit, j, 0)
        dn = d / np.linalg.norm(d, axis=1)[:, None]
        nd = np.einsum("ck,ck->c", Nn[jj], dn)
        rec = out[k]
        rec["kind"] = np.where(is_hit, HIT, MISS)
        rec["t"] = np.where(is_hit, t[rows, jj], 0.0)
        rec["rank"] = np.where(is_hit, mesh.rank[jj], -1)
        rec["tri"] = np.where(is_hit, mesh.tri[jj], -1)
        rec["front"] = np.where(is_hit & (nd < 0), 1, 0)
        rec["u"] = np.where(is_hit, u[rows, jj], 0.0)
        rec["v"] = np.where(is_hit, v[rows, jj], 0.0)
        rec["ambiguous"] = (win[1] != win[2]) | (is_hit & (np.abs(nd) < MIN_ND))
        rec["any_ambiguous"] = ((win[1] >= 0) != (win[2] >= 0)) | (is_hit & (np.abs(nd) < MIN_ND))
        out[k] = rec
    return out


def sun_direction(lon_deg, lat_deg, az_deg, el_deg):
    """The unit direction at azimuth (clockwise from north) / elevation in the east / north / up frame at (lon, lat)."""
    lo, la, az, el = (np.radians(x) for x in (lon_deg, lat_deg, az_deg, el_deg))
    up = np.array([np.cos(la) * np.cos(lo), np.cos(la) * np.sin(lo), np.sin(la)])
    east = np.array([-np.sin(lo), np.cos(lo), 0.0])
    north = np.cross(up, east)
    return np.cos(el) * (np.sin(az) * east + np.cos(az) * north) + np.sin(el) * up


NONE, LIT, AWAY, SHADOW = 0, 1, 2, 3


def sunlit(mesh, tiles, order, ground, sun):
    """The sunlit layer of one view from its expected ground points (ground_ref.ground's dict): (classes (H, W) uint8, ambiguous
    (H, W) bool).  The point's three weights are clamped to >= 0 and renormalised (the origin lies on the pixel's own triangle T0);
    N(T0) . sun <= 0: AWAY; else the ray along sun against every triangle but T0, 1e-3 < t <= 1e6: any hit SHADOW, none LIT."""
    sun = np.asarray(sun, np.float64) / np.linalg.norm(sun)
    fin = ground["kind"] == 1
    H, W = fin.shape
    cls, amb = np.zeros((H, W), np.uint8), np.zeros((H, W), bool)
    if not fin.any():
        return cls, amb
    hm1 = mesh.tile_h - 1
    rank_of = {tuple(o): r for r, o in enumerate(order)}
    rank = np.array([rank_of[(int(a), int(b))] for a, b in zip(ground["tile_lat_deg"][fin], ground["tile_lon_deg"][fin])], np.int64)
    tri = 2 * (ground["cell_x"][fin].astype(np.int64) * hm1 + ground["cell_y"][fin]) + ground["tri"][fin]
    T = RC.tile_triangles(mesh.tile_w, mesh.tile_h)
    v = np.zeros((3, len(rank), 3))
    for r, (hts, rp, mp, ps) in enumerate(tiles):
        sel = rank == r
        if sel.any():
            with np.errstate(all="ignore"):
                P = RC.tile_vertices(np.asarray(hts, np.float32), rp, mp, ps)
            t = T[tri[sel]]
            for k in range(3):
                v[k][sel] = P[t[:, k, 1], t[:, k, 0]]
    w1, w2 = ground["w1"][fin], ground["w2"][fin]
    w = np.clip(np.stack([1.0 - w1 - w2, w1, w2]), 0.0, None)
    w /= w.sum(axis=0)
    origin = (w[:, :, None] * v).sum(axis=0)
    n = np.cross(v[1] - v[0], v[2] - v[0])
    ns = n @ sun
    facing = ns > 0
    c = np.full(len(rank), AWAY, np.uint8)
    a = np.abs(ns) / np.linalg.norm(n, axis=1) < 1e-6
    rays = np.zeros(int(facing.sum()), [("origin", "<f8", 3), ("dir", "<f8", 3), ("t_min", "<f8"), ("t_max", "<f8")])
    rays["origin"], rays["dir"], rays["t_min"], rays["t_max"] = origin[facing], sun, 1e-3, 1e6
    res = cast(mesh, rays, skip=np.stack([rank[facing], tri[facing]], axis=1), open_t_min=True)
    c[facing] = np.where(res["kind"] == HIT, SHADOW, LIT)
    a[facing] |= res["any_ambiguous"]
    cls[fin], amb[fin] = c, a
    return cls, amb


def compare(ref, got, rays, order, tile_h, tol_m, what, max_excluded=0.005):
    """`got` (records with t, kind, tile_lat_deg, tile_lon_deg, cell_x, cell_y, tri, front) against the reference outside its
    ambiguous rays: the kind, and for a hit t * |dir| within tol_m and the same tile, cell, triangle and face.  Returns the largest
    difference of t * |dir| (metres)."""
    keep = ~ref["ambiguous"]
    share = 1.0 - float(keep.mean()) if len(ref) else 0.0
    n_hit = int(((ref["kind"] == HIT) & keep).sum())
    print(f"{what}: {len(ref)} rays, {n_hit} unambiguous hits, excluded {share:.4%}")
    assert share <= max_excluded, f"{what}: {share:.4%} of the rays are ambiguous"
    bad = np.nonzero(keep & (ref["kind"] != got["kind"]))[0]
    assert len(bad) == 0, f"{what}: kind differs for {len(bad)} rays, first {bad[0]}: ref {ref[bad[0]]} got {got[bad[0]]}"
    h = keep & (ref["kind"] == HIT)
    if not h.any():
        return 0.0
    hm1 = tile_h - 1
    lat = np.array([order[r][0] for r in ref["rank"][h]])
    lon = np.array([order[r][1] for r in ref["rank"][h]])
    cell = ref["tri"][h] >> 1
    g = got[h]
    same = (g["tile_lat_deg"] == lat) & (g["tile_lon_deg"] == lon) & (g["cell_x"] == cell // hm1) & (g["cell_y"] == cell % hm1) \
        & (g["tri"] == (ref["tri"][h] & 1)) & (g["front"] == ref["front"][h])
    assert same.all(), f"{what}: {int((~same).sum())} hits name another triangle or face, first ray {np.nonzero(h)[0][np.nonzero(~same)[0][0]]}"
    err = np.abs(g["t"] - ref["t"][h]) * np.linalg.norm(np.asarray(rays["dir"], np.float64)[h], axis=1)
    print(f"{what}: largest |t| difference {err.max():.3e} m")
    assert err.max() <= tol_m, f"{what}: t * |dir| differs by {err.max():.3e} m"
    return float(err.max())
