"""An independent numpy f64 reference of the visibility queries (topo_visibility_*), composed from the two brute-force references it
rests on: surface_ref (the terrain under a longitude and latitude) and los_ref.cast (a ray against every triangle, with one triangle
left out and an open lower bound, as the sunlit layer's shadow ray).

The rule is the one include/topo_hip.h states.  Observer: O = ((R0 + base) + height) u, base the surface height under it with the
ABOVE_TERRAIN flag, else 0; unusable (class 4 for all its targets) when its point is invalid, its height not finite, or the flag is set
and there is no terrain.  Target: class 0 for an invalid point or one without terrain, else T = ((R0 + t) + h) u.  D = O - T, L = |D|,
d = D / L: !(L > 2e-3): 1; for h == 0, N of the target's triangle turned to the side of u, !(N . D > 0): 2; else the ray from T along
d, 1e-3 < t <= L, without the target's own triangle when h == 0: any hit 3, none 1.

A target is AMBIGUOUS -- another implementation's f64 rounding may legitimately decide it the other way -- when the surface lookup is
kind-ambiguous; at h == 0 when it is triangle-ambiguous; when |N . d| / |N| < 1e-6 at the AWAY test; or when the ray is any_ambiguous.
An observer whose own lookup is kind-ambiguous makes all its targets ambiguous."""
from __future__ import annotations

import numpy as np

import los_ref as LR
import surface_ref as SR

R0 = SR.R0
NONE, VISIBLE, AWAY, HIDDEN, NO_OBSERVER = 0, 1, 2, 3, 4
ABOVE_TERRAIN = 1
MIN_RANGE = 2.0e-3
T_MIN = 1.0e-3
MIN_ND = 1e-6


class Meshes:
    """The two meshes of a tile set: the surface's (heights within bounds) and the rays' (finite heights)."""

    def __init__(self, tiles):
        self.surface, self.rays = SR.Mesh(tiles), LR.Mesh(tiles)


def observers(meshes, obs):
    """OBSERVER records -> (O (n, 3), usable (n), ambiguous (n))."""
    lon, lat, hgt = (np.asarray(obs[f], np.float64) for f in ("lon_deg", "lat_deg", "height_m"))
    n = len(lon)
    with np.errstate(invalid="ignore"):
        usable = np.isfinite(lon) & np.isfinite(lat) & (np.abs(lat) <= 90.0) & np.isfinite(hgt)
    base, amb = np.zeros(n), np.zeros(n, bool)
    flagged = usable & ((np.asarray(obs["flags"]) & ABOVE_TERRAIN) != 0)
    if flagged.any():
        rec = SR.surface(meshes.surface, np.stack([lon[flagged], lat[flagged]], axis=1))
        base[flagged] = rec["height_m"]
        amb[flagged] = rec["kind_ambiguous"]
        usable[flagged] = rec["kind"] == SR.TERRAIN
    with np.errstate(invalid="ignore"):
        O = ((R0 + base) + hgt)[:, None] * SR.direction(np.where(usable, lon, 0.0), np.where(usable, lat, 0.0))
    return np.where(usable[:, None], O, 0.0), usable, amb


def visibility(meshes, obs, lonlat, h=0.0):
    """-> (classes (observers, n) uint8, ambiguous (observers, n) bool)."""
    p = np.asarray(lonlat, np.float64).reshape(-1, 2)
    O, usable, o_amb = observers(meshes, obs)
    n = len(p)
    cls = np.full((len(O), n), NO_OBSERVER, np.uint8)
    amb = np.zeros((len(O), n), bool)
    rec = SR.surface(meshes.surface, p)
    terrain = rec["kind"] == SR.TERRAIN
    t_amb = rec["kind_ambiguous"] | (rec["tri_ambiguous"] if h == 0.0 else False)
    idx = np.nonzero(terrain)[0]
    u = SR.direction(p[idx, 0], p[idx, 1])
    T = ((R0 + rec["height_m"][idx]) + h)[:, None] * u
    rank, tri = rec["rank"][idx], rec["tri"][idx]
    rows = meshes.rays.where[rank, tri]
    assert (rows >= 0).all(), "a triangle of the surface is a triangle of the rays"
    m = meshes.rays
    N = np.cross(m.v1[rows] - m.v0[rows], m.v2[rows] - m.v0[rows])
    N = np.where((np.einsum("ck,ck->c", N, u) < 0)[:, None], -N, N)
    Nn = N / np.linalg.norm(N, axis=1)[:, None]
    for o in np.nonzero(usable)[0]:
        c, a = np.full(n, NONE, np.uint8), t_amb | o_amb[o]
        D = O[o][None, :] - T
        L = np.linalg.norm(D, axis=1)
        at = ~(L > MIN_RANGE)
        with np.errstate(all="ignore"):
            d = D / L[:, None]
        k = np.full(len(idx), VISIBLE, np.uint8)
        need = ~at
        if h == 0.0:
            away = need & ~(np.einsum("ck,ck->c", N, D) > 0)
            with np.errstate(invalid="ignore"):
                a[idx] |= need & (np.abs(np.einsum("ck,ck->c", Nn, d)) < MIN_ND)
            k[away] = AWAY
            need &= ~away
        rays = np.zeros(int(need.sum()), [("origin", "<f8", 3), ("dir", "<f8", 3), ("t_min", "<f8"), ("t_max", "<f8")])
        rays["origin"], rays["dir"], rays["t_min"], rays["t_max"] = T[need], d[need], T_MIN, L[need]
        res = LR.cast(m, rays, skip=np.stack([rank[need], tri[need]], axis=1) if h == 0.0 else None, open_t_min=True)
        k[need] = np.where(res["kind"] == LR.HIT, HIDDEN, VISIBLE)
        ra = np.zeros(len(idx), bool)
        ra[need] = res["any_ambiguous"]
        c[idx] = k
        a[idx] |= ra
        cls[o], amb[o] = c, a
    return cls, amb
