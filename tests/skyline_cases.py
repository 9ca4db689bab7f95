"""Cases of the skyline tests (tests/test_skyline_cpu.py, tests/test_skyline_gpu.py), on the tile sets of visibility_cases (which
builds them with los_cases' helpers): the smallest at which the traversal of topo_skyline.h and k_skyline can go wrong.  A case is a
tile set, observers, the azimuths az0 + k daz and a range interval; its reference (skyline_ref) and its emulation (skyline_emul: the
traversal and the every-triangle loop) are computed once and shared.

Every case has N_AZ = 90 azimuths 4 degrees apart, off the lattice of the DEM's meridians and parallels (az0 = 0.37 daz): ninety
waves leave the last workgroup a tail of two.  The observers of a case stand 2 m and 4000 m above the terrain at a point inside a
tile, outside the mosaic looking in (over the sphere), and nowhere (unusable); ridges_ne adds one in the gap between its tile rows,
where an observer above TERRAIN is unusable, over the sphere.  The `grid` tile has 85 raster blocks: the wave takes them in two
batches of 64."""
from __future__ import annotations

import numpy as np

import skyline_emul as SE
import skyline_ref as SR
import visibility_cases as VC

N_AZ = 90
DAZ = 360.0 / N_AZ
AZ0 = 0.37 * DAZ
MIN_RANGE, MAX_RANGE = 10.0, 1.0e6
MAX_AMBIGUOUS = VC.MAX_AMBIGUOUS      # the project's cap
UNUSABLE = VC.observer_records(np.nan, 46.0, 10.0)

_CASES, _EDGES, _REF, _EMU = {}, {}, {}, {}


def _standard(ts, at=(0.413, 0.387), outside=(-0.3, 0.52, 3000.0), extra=None, heights=(2.0, 4000.0)):
    """The observers of a tile set: `heights` above the terrain at box corner + at (degrees), `outside` (dlon from the box's west edge,
    fraction of its latitudes, height over the sphere), unusable, then `extra`."""
    box = VC.tileset(ts)[2]
    lon, lat = box[0] + at[0], box[2] + at[1]
    obs = [VC.observer_records(lon, lat, h) for h in heights]
    obs.append(VC.observer_records(box[0] + outside[0], box[2] + outside[1] * (box[3] - box[2]), outside[2], False))
    obs.append(UNUSABLE)
    return np.concatenate(obs + ([] if extra is None else [extra]))


def _case(ts, obs, min_range=MIN_RANGE, max_range=MAX_RANGE, unusable=(3,)):
    tiles, order, box = VC.tileset(ts)
    return dict(tileset=ts, tiles=tiles, order=order, obs=obs, az0=AZ0, daz=DAZ, n_az=N_AZ, min_range=min_range, max_range=max_range, unusable=list(unusable))


CASES = {
    "blocks": lambda: _case("blocks", _standard("blocks")),
    # the gap between the tile rows runs along 46N .. 46N + 1/32: observer 4 stands in it over a valley floor (the relief is about 200 m
    # at 16.1357E), 600 m over the sphere, between ridges of 3800 m
    "ridges_ne": lambda: _case("ridges_ne", _standard("ridges_ne", extra=VC.observer_records(16.1357, 46.0 + 1.0 / 64.0, 600.0, False))),
    "ridges_ne_min": lambda: _case("ridges_ne", _standard("ridges_ne")[:2], min_range=60.0e3, unusable=()),      # skips the nearest ridges
    "ridges_ne_max": lambda: _case("ridges_ne", _standard("ridges_ne")[:2], max_range=40.0e3, unusable=()),      # cuts the far ones
    "long": lambda: _case("long", _standard("long", at=(1.413, 0.387))),
    "void_nan": lambda: _case("void_nan", _standard("void_nan")),
    "antimeridian": lambda: _case("antimeridian", _standard("antimeridian", at=(1.213, 0.387))),      # stands east of the antimeridian
    "north84": lambda: _case("north84", _standard("north84")),
    "polar": lambda: _case("polar", _standard("polar", at=(0.413, 0.587))),
    "grid": lambda: _case("grid", _standard("grid")[:2], unusable=()),
}
RAY_CHECKED = ("ridges_ne", "blocks")


def case(name):
    if name not in _CASES:
        _CASES[name] = CASES[name]()
    return _CASES[name]


def edges(ts):
    if ts not in _EDGES:
        _EDGES[ts] = SR.Edges(VC.meshes(ts).rays)
    return _EDGES[ts]


def reference(name):
    """((observers, n_az) skyline_ref records, the observers' points) of the case; computed once."""
    if name not in _REF:
        c = case(name)
        _REF[name] = SR.skyline(VC.meshes(c["tileset"]), edges(c["tileset"]), c["obs"], c["az0"], c["daz"], c["n_az"], c["min_range"], c["max_range"])
    return _REF[name]


def emulation(name, brute=False):
    """(observers, n_az) skyline_emul records of the case, by the traversal or (brute) every triangle; computed once."""
    if (name, brute) not in _EMU:
        c = case(name)
        rec, bad = SE.skyline(c["tiles"], c["order"], c["obs"], c["az0"], c["daz"], c["n_az"], c["min_range"], c["max_range"], brute)
        assert bad == 0, f"{name}: {bad} index checks failed in the emulation"
        _EMU[(name, brute)] = rec
    return _EMU[(name, brute)]


def plane_point(rec):
    """(s, z) of records that carry an elevation (degrees) and a range: the crossing point in its half-plane."""
    el = np.radians(rec["elevation_deg"])
    return rec["range_m"] * np.cos(el), rec["range_m"] * np.sin(el)


def against_reference(got, name, what, tol_m=1e-3):
    """`got` (records with kind, tile, cell, tri, edge, elevation_deg, range_m, lon_deg, lat_deg, height_m) against the reference on its
    unambiguous azimuths: the kind, the same (tile, cell, triangle, edge), and the crossing point within tol_m -- in its half-plane
    (elevation within tol_m / range radians) and on the globe.  Returns the largest distance (metres)."""
    c = case(name)
    ref, O = reference(name)
    keep = ~ref["ambiguous"]
    share = 1.0 - float(keep.mean())
    assert share <= MAX_AMBIGUOUS, f"{what}: {share:.4%} of the azimuths are ambiguous"
    assert got.shape == ref.shape
    bad = np.argwhere(keep & (got["kind"] != ref["kind"]))
    assert len(bad) == 0, f"{what}: kind differs on {len(bad)} azimuths, first {tuple(bad[0])}: {got[tuple(bad[0])]} vs {ref[tuple(bad[0])]}"
    t = keep & (ref["kind"] == SR.TERRAIN)
    if not t.any():
        return 0.0
    hm1 = c["tiles"][0][0].shape[0] - 1
    r, g = ref[t], got[t]
    order = np.asarray(c["order"])
    cell = r["tri"] >> 1
    same = (g["tile_lat_deg"] == order[r["rank"], 0]) & (g["tile_lon_deg"] == order[r["rank"], 1]) & (g["cell_x"] == cell // hm1) & (g["cell_y"] == cell % hm1) \
        & (g["tri"] == (r["tri"] & 1)) & (g["edge"] == r["edge"])
    assert same.all(), f"{what}: {int((~same).sum())} azimuths name another edge, first {tuple(np.argwhere(t)[np.nonzero(~same)[0][0]])}"
    s, z = plane_point(g)
    err = np.hypot(s - r["s"], z - r["z"])
    P = O[np.nonzero(t)[0]] + r["X"]
    norm = np.linalg.norm(P, axis=1)
    lat, lon = np.degrees(np.arcsin(P[:, 2] / norm)), np.degrees(np.arctan2(P[:, 1], P[:, 0]))
    dlon = (g["lon_deg"] - lon + 180.0) % 360.0 - 180.0
    geo = np.hypot(np.radians(dlon) * np.cos(np.radians(lat)) * norm, np.radians(g["lat_deg"] - lat) * norm)
    print(f"{what}: {int(t.sum())} unambiguous terrain azimuths of {t.size}, excluded {share:.4%}, crossing point within {err.max():.3e} m in the plane, {geo.max():.3e} m on the globe")
    assert err.max() <= tol_m and geo.max() <= tol_m, f"{what}: the crossing point differs by {max(err.max(), geo.max()):.3e} m"
    assert np.abs(g["height_m"] - (norm - SR.R0)).max() <= max(tol_m, 1e-3)
    return float(max(err.max(), geo.max()))
