"""Tile sets, parameters and snap points of the summit tests (tests/test_summits_cpu.py, tests/test_summits_gpu.py): the smallest
shapes at which each part of topo_summits.h and kernels_summits.h can go wrong.  The tile sets are visibility_cases' (ragged raster
blocks, two batches of 64 blocks, dominators in another tile and across a gap, a window over three tiles, voids, the antimeridian, the
all-columns branch at 84N and at the pole) and surface_cases.overlap_tiles (posts duplicated bit for bit), plus two small ones whose
answers are known by hand.  Each tile set's reference (summits_ref) and emulation (summits_emul) are computed once per run and shared.

Runs per tile set, in units of its post spacing s along a meridian -- all off the lattice's own distances, so that the reference
reports no ambiguous membership (test_summits_cpu.py checks that it does not):
  near   radius 3.37 s, min isolation 1.63 s
  fine   radius 3.37 s, min isolation 0.31 of the SMALLEST post spacing: the prefilter must drop nothing
  wide   radius 400 km (the whole mosaic), min isolation 1.63 s
  high   near, with min_height_m just above the 97th percentile of the heights"""
from __future__ import annotations

import numpy as np

import los_cases as LC
import summits_emul as SE
import summits_ref as SR
import surface_cases as SC
import topo_renderer_amd as T
import visibility_cases as VC

R0 = 6371000.0
RUNS = ("near", "fine", "wide", "high")
_TILES, _POSTS, _REF, _EMU, _SNAP = {}, {}, {}, {}, {}


def _flat_tile(lat, lon, n, fn):
    rp, mp, ps = T.synth.tile_transform(lat, lon, n, n)
    vy, vx = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    return (np.ascontiguousarray(fn(vx, vy), np.float32), rp, mp, ps)


def _plateau():
    """A flat-topped hill (a 5 x 4 plateau of 700 m on a cone) and a wholly constant tile: one summit each, at the lowest index."""
    def hill(vx, vy):
        return np.minimum(700.0, 1000.0 - 60.0 * np.hypot(vx - 11.0, vy - 9.5))
    tiles = [_flat_tile(45, 15, 24, hill), _flat_tile(45, 16, 24, lambda vx, vy: 250.0 + 0.0 * vx)]
    return tiles, [(45, 15), (45, 16)], (15.0, 17.0, 45.0, 46.0)


SPIKES = ((5, 7, 300.0), (17, 4, 200.0), (9, 19, 100.0))      # (vx, vy, height)


def _spikes():
    def fn(vx, vy):
        h = np.zeros(vx.shape)
        for x, y, v in SPIKES:
            h[y, x] = v
        return h
    return [_flat_tile(45, 15, 24, fn)], [(45, 15)], (15.0, 16.0, 45.0, 46.0)


def _overlap():
    tiles, order = SC.overlap_tiles(LC.geo_relief)
    return tiles, order, (15.0, 15.5 + 23.0 / 32.0, 46.0 - 23.0 / 32.0, 46.0)


TILESETS = {name: (lambda name=name: VC.tileset(name)) for name in ("blocks", "grid", "ridges_ne", "long", "void_nan", "antimeridian", "north84", "polar")}
TILESETS.update({"overlap": _overlap, "plateau": _plateau, "spikes": _spikes})
SMALL = tuple(n for n in TILESETS if n != "grid")      # at most 20 000 posts: compared with brute force over every post


def tileset(name):
    """(tiles in draw order, their (lat, lon), the degree box)."""
    if name not in _TILES:
        _TILES[name] = TILESETS[name]()
    return _TILES[name]


def posts(name):
    if name not in _POSTS:
        _POSTS[name] = SR.Posts(tileset(name)[0])
    return _POSTS[name]


def spacing(name):
    """(along a meridian, the smallest along a parallel) in metres."""
    tiles = tileset(name)[0]
    ps = np.asarray(tiles[0][3], np.float32).astype(np.float64)
    p = posts(name)
    lat = np.abs(p.lat_deg[p.exists])
    lat = lat[lat < 89.999]      # (the posts of a pole row coincide)
    return R0 * np.radians(abs(ps[1])), R0 * np.radians(abs(ps[0])) * np.cos(np.radians(lat.max()))


def params(name, run):
    """(radius_m, min_isolation_m, min_height_m)."""
    s, smallest = spacing(name)
    p = posts(name)
    if run == "near":
        return 3.37 * s, 1.63 * s, -np.inf
    if run == "fine":
        return 3.37 * s, 0.31 * min(s, smallest), -np.inf
    if run == "wide":
        return 400.0e3 + 13.7, 1.63 * s, -np.inf
    return 3.37 * s, 1.63 * s, float(np.float32(np.quantile(p.h[p.exists].astype(np.float64), 0.97) + 0.123))


def reference(name, run):
    if (name, run) not in _REF:
        _REF[name, run] = SR.summits(posts(name), *params(name, run))
    return _REF[name, run]


def emulation(name, run):
    """(records in tile order, count, (after the prefilter, after the any-hit stage), failed index checks)."""
    if (name, run) not in _EMU:
        tiles, order, _ = tileset(name)
        _EMU[name, run] = SE.summits(tiles, order, *params(name, run))
    return _EMU[name, run]


# ---- snap ---------------------------------------------------------------------------------------------------------------------
def snap_points(name):
    """((n, 2) lon / lat degrees, the number of seeded random ones in front, the radius): random points over the box and a 2 % margin,
    exact posts, points in the gaps between tiles (where there are any), far outside, and invalid ones."""
    tiles, order, box = tileset(name)
    p = posts(name)
    if name == "polar":      # the posts of the pole row coincide, in every tile: which of them is "nearest" is rounding.  The random points stay out of their reach.
        box = box[:3] + (89.9,)
    rnd = SC.random_points(box[0], box[1], box[2], box[3], 160, 77)
    every = max(1, len(p.h) // 40)
    exact = np.stack([p.lon_deg[::every], p.lat_deg[::every]], axis=-1)
    gaps = np.array([[0.5 * (box[0] + box[1]) + 0.0137, 0.5 * (box[2] + box[3]) + 0.0071], [box[0] + 0.999, box[2] + 0.4071]])
    far = np.array([[box[0] - 7.3, box[2] - 3.0], [box[0] + 0.5, box[2] - 6.1]])      # (degrees of latitude away: out of reach at any latitude)
    bad = np.array([[np.nan, 45.0], [10.0, 90.5], [np.inf, 0.0], [10.0, np.nan]])
    s, _ = spacing(name)
    return np.concatenate([rnd, exact, gaps, far, bad]), len(rnd), 2.37 * s


def snap_reference(name):
    if name not in _SNAP:
        pts, _, radius = snap_points(name)
        tiles, order, _ = tileset(name)
        emu, bad = SE.snap(tiles, order, pts, radius)
        assert bad == 0
        _SNAP[name] = (SR.snap(posts(name), pts, radius), emu)
    return _SNAP[name]


# ---- comparisons ----------------------------------------------------------------------------------------------------------------
def compare_with_reference(name, run, got, what, tol=1e-3):
    """`got` (records with rank / idx / isolation_m / height_m / has_higher / higher_rank / higher_idx, tile order) against the
    reference: the same summit set, isolation within tol, the same dominator where the reference finds no runner-up."""
    ref = reference(name, run)
    assert not ref["member_ambiguous"].any(), f"{what}: the reference calls {int(ref['member_ambiguous'].sum())} memberships ambiguous: move the parameters off the lattice"
    want = ref[ref["member"]]
    assert len(got) == len(want), f"{what}: {len(got)} summits, the reference has {len(want)}"
    assert np.array_equal(got["rank"], want["rank"]) and np.array_equal(got["idx"], want["idx"]), f"{what}: another summit set"
    assert np.array_equal(got["height_m"].view(np.uint32), want["height_m"].view(np.uint32)), what
    sure = ~want["isolation_ambiguous"]
    both = sure & want["has_higher"]
    assert np.array_equal(got["has_higher"][sure] != 0, want["has_higher"][sure]), f"{what}: isolation finite / infinite differs"
    err = np.abs(got["isolation_m"][both] - want["isolation_m"][both])
    print(f"{what}: {len(want)} summits, {int(both.sum())} with a dominator in range, largest isolation difference {err.max() if len(err) else 0.0:.3e} m, "
          f"{int(want['higher_ambiguous'].sum())} with twin dominators")
    assert (err <= tol).all(), f"{what}: isolation differs by {err.max():.3e} m"
    assert np.isinf(got["isolation_m"][sure & ~want["has_higher"]]).all(), what
    ident = both & ~want["higher_ambiguous"]
    assert np.array_equal(got["higher_rank"][ident], want["higher_rank"][ident]) and np.array_equal(got["higher_idx"][ident], want["higher_idx"][ident]), f"{what}: another dominator"
    return want


def compare_snap(ref, got, n_random, what, tol=1e-3):
    share = float(ref["ambiguous"][:n_random].mean())
    print(f"{what}: {len(ref)} points, {int((ref['status'] == SR.FOUND).sum())} snapped, ambiguous among the {n_random} random ones {share:.4%}")
    assert share <= VC.MAX_AMBIGUOUS, f"{what}: {share:.4%} of the random points are ambiguous"
    sure = ~ref["ambiguous"]
    assert np.array_equal(got["status"][sure], ref["status"][sure]), f"{what}: status differs"
    f = sure & (ref["status"] == SR.FOUND)
    assert np.array_equal(got["rank"][f], ref["rank"][f]) and np.array_equal(got["idx"][f], ref["idx"][f]), f"{what}: another post"
    assert np.array_equal(got["height_m"][f].view(np.uint32), ref["height_m"][f].view(np.uint32)), what
    assert (np.abs(got["distance_m"][f] - ref["distance_m"][f]) <= tol).all(), f"{what}: distance differs"
