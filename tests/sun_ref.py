"""An independent numpy f64 reference of the sun exposure queries (topo_sun_exposure_*), composed from the two brute-force references
it rests on: surface_ref (the terrain under a longitude and latitude) and los_ref.cast (a ray against every triangle, with one
triangle left out and an open lower bound, as the sunlit layer's shadow ray).

The rule is the one include/topo_hip.h states.  Target: class 0 for an invalid point or one without terrain, else T = (R0 + t) u and N
of the target's triangle turned to the side of u.  Per sun s (unit, towards the sun): !(u . s > 0): 4 (night); !(N . s > 0): 2 (away);
else the ray from T along s, 1e-3 < t <= 1e6, without the target's own triangle: any hit 3 (shadow), none 1 (lit).  lit / shadow: bit k
set iff sun k is 1 / 3; exposure: the sum in ascending k over the lit suns of weight_k (N . s_k) / |N|, f64, rounded once to f32; NaN
for class 0.

A pair (target, sun) is AMBIGUOUS -- another implementation's f64 rounding may legitimately decide it the other way -- when the surface
lookup is kind-ambiguous or triangle-ambiguous; when |u . s| < 1e-6; when |N^ . s| < 1e-6 at the AWAY test; or when the ray is
any_ambiguous."""
from __future__ import annotations

import numpy as np

import los_ref as LR
import surface_ref as SR
from visibility_ref import Meshes      # the two meshes of a tile set  # noqa: F401

R0 = SR.R0
NONE, LIT, AWAY, SHADOW, NIGHT = 0, 1, 2, 3, 4
T_MIN, T_MAX = 1.0e-3, 1.0e6
MIN_DOT = 1e-6
MAX_SUNS = 64


def unit_suns(suns):
    """Records with dir and weight -> (unit directions (s, 3), weights (s))."""
    d = np.asarray(suns["dir"], np.float64).reshape(-1, 3)
    return d / np.sqrt((d * d).sum(axis=1))[:, None], np.asarray(suns["weight"], np.float64).reshape(-1)


def sun_exposure(meshes, suns, lonlat):
    """-> (classes (suns, n) uint8, lit (n) uint64, shadow (n) uint64, exposure (n) float32, ambiguous (suns, n) bool)."""
    p = np.asarray(lonlat, np.float64).reshape(-1, 2)
    S, W = unit_suns(suns)
    n = len(p)
    cls = np.full((len(S), n), NONE, np.uint8)
    amb = np.zeros((len(S), n), bool)
    rec = SR.surface(meshes.surface, p)
    terrain = rec["kind"] == SR.TERRAIN
    t_amb = rec["kind_ambiguous"] | rec["tri_ambiguous"]
    idx = np.nonzero(terrain)[0]
    u = SR.direction(p[idx, 0], p[idx, 1])
    T = (R0 + rec["height_m"][idx])[:, None] * u
    rank, tri = rec["rank"][idx], rec["tri"][idx]
    m = meshes.rays
    rows = m.where[rank, tri]
    assert (rows >= 0).all(), "a triangle of the surface is a triangle of the rays"
    N = np.cross(m.v1[rows] - m.v0[rows], m.v2[rows] - m.v0[rows])
    N = np.where((np.einsum("ck,ck->c", N, u) < 0)[:, None], -N, N)
    n_len = np.linalg.norm(N, axis=1)
    total = np.zeros(len(idx), np.float64)
    for k, s in enumerate(S):
        a = t_amb.copy()
        us, ns = u @ s, N @ s
        night = ~(us > 0)
        away = ~night & ~(ns > 0)
        need = ~night & ~away
        c = np.full(len(idx), LIT, np.uint8)
        c[night], c[away] = NIGHT, AWAY
        ka = np.abs(us) < MIN_DOT
        ka |= ~night & (np.abs(ns / n_len) < MIN_DOT)
        rays = np.zeros(int(need.sum()), [("origin", "<f8", 3), ("dir", "<f8", 3), ("t_min", "<f8"), ("t_max", "<f8")])
        rays["origin"], rays["dir"], rays["t_min"], rays["t_max"] = T[need], s, T_MIN, T_MAX
        res = LR.cast(m, rays, skip=np.stack([rank[need], tri[need]], axis=1), open_t_min=True)
        c[need] = np.where(res["kind"] == LR.HIT, SHADOW, LIT)
        ka[need] |= res["any_ambiguous"]
        total += np.where(c == LIT, W[k] * ns / n_len, 0.0)
        cls[k, idx] = c
        a[idx] |= ka
        amb[k] = a
    exposure = np.full(n, np.nan, np.float32)
    exposure[idx] = total.astype(np.float32)
    return (cls,) + masks(cls) + (exposure, amb)


def masks(cls):
    """(suns, n) classes -> (lit (n) uint64, shadow (n) uint64)."""
    bit = (np.uint64(1) << np.arange(len(cls), dtype=np.uint64))[:, None]
    zero = np.uint64(0)
    return tuple(np.bitwise_or.reduce(np.where(cls == k, bit, zero), axis=0) if len(cls) else np.zeros(cls.shape[1], np.uint64) for k in (LIT, SHADOW))
