"""An independent numpy f64 brute-force reference of the skyline queries (topo_skyline_*): every azimuth against every edge of every
existing triangle.

Vertices and topology are those of los_ref.Mesh (oracle/ray_check.py: tile_vertices, tile_triangles) through visibility_ref.Meshes;
the observers are visibility_ref's.  The rule is the one include/topo_hip.h states: the frame up = O / |O|, east = z x up normalised,
north = up x east; azimuth a_k = az0 + k daz, h = cos a north + sin a east, m = h x up; for each edge (e, (e + 1) % 3) of each
existing triangle, endpoints in the order of their vertex indices y * w + x and translated by O: da = m . a, db = m . b, crossing iff
(da < 0) != (db < 0), X = a + (da / (da - db)) (b - a), s = h . X, z = up . X, counting iff min_range <= s <= max_range; the largest
z / s wins, then the smaller s, the earlier tile, the lower triangle, the lower edge.

An azimuth is AMBIGUOUS -- the f64 rounding of another implementation may legitimately decide it the other way -- when a vertex lies
within 1e-6 m of the plane; when the runner-up -- the best crossing on a geometrically different edge (the edge two triangles share
is one edge) -- comes within 1e-9 of the winner's z / s; or when the winner's s lies within 1e-3 m of a range limit.  All azimuths
of an observer whose own lookup is ambiguous are ambiguous.  A record names the winner and the runner-up."""
from __future__ import annotations

import numpy as np

import visibility_ref as VR
from oracle import ray_check as RC

R0 = VR.R0
NONE, TERRAIN, NO_OBSERVER = 0, 1, 4
EPS_PLANE = 1e-6      # metres
EPS_RATIO = 1e-9
EPS_RANGE = 1e-3      # metres
OUT_DTYPE = np.dtype([("kind", "<i4"), ("ratio", "<f8"), ("s", "<f8"), ("z", "<f8"), ("X", "<f8", 3), ("rank", "<i8"), ("tri", "<i8"), ("edge", "<i8"),
                      ("runner_ratio", "<f8"), ("runner_rank", "<i8"), ("runner_tri", "<i8"), ("runner_edge", "<i8"), ("shared", "?"), ("ambiguous", "?")])
# (runner_*: the best crossing on a geometrically different edge, -1 / -inf where there is none)


class Edges:
    """The three edges of every triangle of a los_ref.Mesh, in ascending (rank, triangle, edge): endpoints A, B in canonical order,
    a number `geo` that two edges share iff they join the same two vertices of the same tile, and whether two existing triangles do."""

    def __init__(self, mesh):
        w, h = mesh.tile_w, mesh.tile_h
        T = RC.tile_triangles(w, h)[mesh.tri]                                   # (n, 3, 2): (x, y) of the three vertices
        V = np.stack([mesh.v0, mesh.v1, mesh.v2], axis=1)                       # (n, 3, 3)
        idx = T[:, :, 1] * w + T[:, :, 0]                                       # (n, 3)
        nxt = np.array([1, 2, 0])
        ia, ib = idx, idx[:, nxt]                                               # edge e: vertex e -> vertex (e + 1) % 3
        swap = ia > ib
        Pa, Pb = V, V[:, nxt]
        self.A = np.where(swap[..., None], Pb, Pa).reshape(-1, 3)
        self.B = np.where(swap[..., None], Pa, Pb).reshape(-1, 3)
        lo, hi = np.minimum(ia, ib).reshape(-1), np.maximum(ia, ib).reshape(-1)
        self.rank = np.repeat(mesh.rank, 3)
        self.tri = np.repeat(mesh.tri, 3)
        self.edge = np.tile(np.arange(3), len(mesh.tri))
        self.geo = (self.rank * (w * h) + lo) * (w * h) + hi
        _, inverse, counts = np.unique(self.geo, return_inverse=True, return_counts=True)
        self.shared = counts[inverse] == 2
        assert counts.max() <= 2


def frames(O, usable):
    """(up, east, north, usable) at the observers O (n, 3)."""
    with np.errstate(all="ignore"):
        rho = np.linalg.norm(O, axis=1)
        up = O / rho[:, None]
        n = np.hypot(up[:, 0], up[:, 1])
        east = np.stack([-up[:, 1] / n, up[:, 0] / n, 0.0 * n], axis=1)
    ok = usable & (n > 0) & np.isfinite(east).all(axis=1)
    north = np.cross(up, east)
    return up, east, north, ok


def azimuths(az0, daz, n_az):
    """One rounded product and one rounded sum each, as the kernel forms them (degrees)."""
    return np.float64(az0) + np.arange(n_az, dtype=np.float64) * np.float64(daz)


def skyline(meshes, edges, obs, az0, daz, n_az, min_range, max_range, chunk=8):
    """-> (observers, n_az) OUT_DTYPE records, and the observers' points O (n, 3)."""
    O, usable, o_amb = VR.observers(meshes, obs)
    up, east, north, usable = frames(O, usable)
    out = np.zeros((len(O), n_az), OUT_DTYPE)
    out["kind"] = NO_OBSERVER
    out["ratio"] = out["runner_ratio"] = np.nan
    out["rank"] = out["tri"] = out["edge"] = out["runner_rank"] = out["runner_tri"] = out["runner_edge"] = -1
    az = np.radians(azimuths(az0, daz, n_az))
    for o in np.nonzero(usable)[0]:
        a, b = edges.A - O[o], edges.B - O[o]
        H = np.cos(az)[:, None] * north[o] + np.sin(az)[:, None] * east[o]      # (n_az, 3)
        M = np.cross(H, up[o])
        za, zb = a @ up[o], b @ up[o]
        for k0 in range(0, n_az, chunk):
            ks = np.arange(k0, min(k0 + chunk, n_az))
            with np.errstate(all="ignore"):
                da, db = a @ M[ks].T, b @ M[ks].T                               # (edges, c)
                near_vertex = ((np.abs(da) < EPS_PLANE) | (np.abs(db) < EPS_PLANE)).any(axis=0)
                e, c = np.nonzero((da < 0) != (db < 0))
                f = da[e, c] / (da[e, c] - db[e, c])
                X = a[e] + f[:, None] * (b[e] - a[e])
                s = np.einsum("nk,nk->n", X, H[ks][c])
                z = za[e] + f * (zb[e] - za[e])
                ratio = z / s
            counts = (s >= min_range) & (s <= max_range) & ~np.isnan(ratio)
            at_limit = (np.abs(s - min_range) < EPS_RANGE) | (np.abs(s - max_range) < EPS_RANGE)
            for j, k in enumerate(ks):
                rec = out[o, k]
                sel = np.nonzero(c == j)[0]
                cand = sel[counts[sel]]
                amb = bool(near_vertex[j]) or bool(o_amb[o])
                if len(cand) == 0:
                    rec["kind"] = NONE
                    rec["ambiguous"] = amb
                    out[o, k] = rec
                    continue
                order = np.lexsort((e[cand], s[cand], -ratio[cand]))            # ascending edge number = (rank, triangle, edge)
                win = cand[order[0]]
                ranked = cand[order]
                other = ranked[edges.geo[e[ranked]] != edges.geo[e[win]]]      # in the winner's order: the first is the runner-up
                runner = ratio[other[0]] if len(other) else -np.inf
                if len(other):
                    rec["runner_rank"], rec["runner_tri"], rec["runner_edge"] = edges.rank[e[other[0]]], edges.tri[e[other[0]]], edges.edge[e[other[0]]]
                amb = amb or runner >= ratio[win] - EPS_RATIO or bool(at_limit[win])
                rec["kind"], rec["ratio"], rec["s"], rec["z"], rec["X"] = TERRAIN, ratio[win], s[win], z[win], X[win]
                rec["rank"], rec["tri"], rec["edge"] = edges.rank[e[win]], edges.tri[e[win]], edges.edge[e[win]]
                rec["runner_ratio"], rec["shared"], rec["ambiguous"] = runner, edges.shared[e[win]], amb
                out[o, k] = rec
    return out, O


def direction(O, az_deg, elevation_rad):
    """The unit direction at azimuth az_deg (n) and elevation (n, radians) in the frame at the point O (3)."""
    up, east, north, _ = frames(O[None, :], np.ones(1, bool))
    a = np.radians(az_deg)
    h = np.cos(a)[:, None] * north[0] + np.sin(a)[:, None] * east[0]
    return np.cos(elevation_rad)[:, None] * h + np.sin(elevation_rad)[:, None] * up[0]
