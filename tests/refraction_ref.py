"""An independent numpy f64 reference of the refracted visibility queries (topo_visibility_refracted_*).

Its own statement of the rule: for an observer at O and a coefficient k, a mesh vertex at v is seen where a vertex at
v (1 + c |v - O|^2 / |v|), c = k / (2 R0), would be seen along straight lines -- the same direction, |v| raised by c |v - O|^2, the
standard k s^2 / (2 R0) curvature-and-refraction correction with s the chord.  So per observer the vertex arrays of surface_ref.Mesh
(where a target lies) and of los_ref.Mesh (what a sight line can meet) are lifted in numpy, and from there on it is visibility_ref's
rule word for word: the target under (lon, lat) on the lifted surface, N of its lifted triangle, the mast height on top, los_ref.cast
from T towards O with the target's triangle left out at h == 0.  O itself comes from visibility_ref.observers on the UNLIFTED mesh.

A target is ambiguous exactly as in visibility_ref (judged on the lifted meshes)."""
from __future__ import annotations

import copy

import numpy as np

import los_ref as LR
import surface_ref as SR
import visibility_ref as VR

R0 = SR.R0
STANDARD = 0.13


def lift(O, v, k):
    """v (n, 3) seen from O under coefficient k."""
    v = np.asarray(v, np.float64)
    s2 = ((v - np.asarray(O, np.float64)) ** 2).sum(axis=-1)
    with np.errstate(all="ignore"):
        return v * (1.0 + (k / (2.0 * R0)) * s2 / np.linalg.norm(v, axis=-1))[..., None]


def lifted(mesh, O, k):
    """A copy of a surface_ref.Mesh or los_ref.Mesh with its vertices lifted for O."""
    m = copy.copy(mesh)
    m.v0, m.v1, m.v2 = lift(O, mesh.v0, k), lift(O, mesh.v1, k), lift(O, mesh.v2, k)
    return m


def _one(surface, rays, O, o_amb, p, h):
    """visibility_ref.visibility's loop body for one usable observer at O over the (lifted) meshes."""
    n = len(p)
    rec = SR.surface(surface, p)
    terrain = rec["kind"] == SR.TERRAIN
    c, a = np.full(n, VR.NONE, np.uint8), rec["kind_ambiguous"] | (rec["tri_ambiguous"] if h == 0.0 else False) | o_amb
    idx = np.nonzero(terrain)[0]
    u = SR.direction(p[idx, 0], p[idx, 1])
    T = ((R0 + rec["height_m"][idx]) + h)[:, None] * u
    rank, tri = rec["rank"][idx], rec["tri"][idx]
    rows = rays.where[rank, tri]
    assert (rows >= 0).all(), "a triangle of the surface is a triangle of the rays"
    N = np.cross(rays.v1[rows] - rays.v0[rows], rays.v2[rows] - rays.v0[rows])
    N = np.where((np.einsum("ck,ck->c", N, u) < 0)[:, None], -N, N)
    Nn = N / np.linalg.norm(N, axis=1)[:, None]
    D = O[None, :] - T
    L = np.linalg.norm(D, axis=1)
    with np.errstate(all="ignore"):
        d = D / L[:, None]
    k = np.full(len(idx), VR.VISIBLE, np.uint8)
    need = L > VR.MIN_RANGE
    if h == 0.0:
        away = need & ~(np.einsum("ck,ck->c", N, D) > 0)
        with np.errstate(invalid="ignore"):
            a[idx] |= need & (np.abs(np.einsum("ck,ck->c", Nn, d)) < VR.MIN_ND)
        k[away] = VR.AWAY
        need &= ~away
    q = np.zeros(int(need.sum()), [("origin", "<f8", 3), ("dir", "<f8", 3), ("t_min", "<f8"), ("t_max", "<f8")])
    q["origin"], q["dir"], q["t_min"], q["t_max"] = T[need], d[need], VR.T_MIN, L[need]
    res = LR.cast(rays, q, skip=np.stack([rank[need], tri[need]], axis=1) if h == 0.0 else None, open_t_min=True)
    k[need] = np.where(res["kind"] == LR.HIT, VR.HIDDEN, VR.VISIBLE)
    ra = np.zeros(len(idx), bool)
    ra[need] = res["any_ambiguous"]
    c[idx] = k
    a[idx] |= ra
    return c, a


def visibility(meshes, obs, lonlat, h=0.0, k=STANDARD):
    """meshes: visibility_ref.Meshes (unlifted) -> (classes (observers, n) uint8, ambiguous (observers, n) bool)."""
    p = np.asarray(lonlat, np.float64).reshape(-1, 2)
    O, usable, o_amb = VR.observers(meshes, obs)
    cls = np.full((len(O), len(p)), VR.NO_OBSERVER, np.uint8)
    amb = np.zeros((len(O), len(p)), bool)
    for o in np.nonzero(usable)[0]:
        cls[o], amb[o] = _one(lifted(meshes.surface, O[o], k), lifted(meshes.rays, O[o], k), O[o], o_amb[o], p, h)
    return cls, amb
