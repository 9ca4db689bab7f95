"""The summit rule without a GPU: the g++ build of csrc/topo_summits.h (tests/summits_emul.cpp) -- the windowed search the kernels
restate -- against the same header's brute force bit for bit, and against the independent numpy reference (tests/summits_ref.py);
the hand-known tiles; the host's orders; the ABI's struct sizes."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

import summits_cases as MC
import summits_emul as SE
import topo_renderer_amd as T

HERE = os.path.dirname(os.path.abspath(__file__))
RUN_RADII = ("near", "wide")      # (fine and high share near's radius)


def all_posts(name):
    p = MC.posts(name)
    ids = np.arange(len(p.h), dtype=np.int64)
    return np.stack([ids // p.per_tile, ids % p.per_tile], axis=-1).astype(np.uint32)


def same_bits(a, b, fields):
    return all(np.ascontiguousarray(a[f]).tobytes() == np.ascontiguousarray(b[f]).tobytes() for f in fields)


FIELDS = ("isolation_m", "higher_height_m", "higher_rank", "higher_idx", "has_higher", "height_m", "lon_deg", "lat_deg")


@pytest.mark.parametrize("name", MC.SMALL)
def test_windowed_equals_brute_force_over_every_post(name):
    tiles, order, _ = MC.tileset(name)
    posts = all_posts(name)
    for run in RUN_RADII:
        radius = MC.params(name, run)[0]
        fast, bad = SE.isolation(tiles, order, posts, radius)
        slow, bad2 = SE.isolation(tiles, order, posts, radius, brute=True)
        assert bad == 0 and bad2 == 0
        assert same_bits(fast, slow, FIELDS), (name, run, np.nonzero(fast["isolation_m"] != slow["isolation_m"])[0][:5])
        assert np.array_equal(fast["has_higher"] == -1, ~MC.posts(name).exists)


def test_windowed_equals_brute_force_on_the_grid_sample():
    """`grid` is 75 250 posts: a seeded sample of 512 posts and every summit the near, wide and high runs report, all of them kept.  The
    fine run reports nearly every post (its min isolation lies below the post spacing), so of ITS summits a seeded 2400 are added:
    brute force over all of them would be the every-post comparison this case is too large for."""
    tiles, order, _ = MC.tileset("grid")
    p = MC.posts("grid")
    rng = np.random.default_rng(5)
    sample = rng.choice(len(p.h), 512, replace=False)
    flat = lambda run: MC.emulation("grid", run)[0]["rank"].astype(np.int64) * p.per_tile + MC.emulation("grid", run)[0]["idx"]
    reported = np.concatenate([flat(run) for run in ("near", "wide", "high")])
    fine = flat("fine")
    assert len(reported) > 0 and len(fine) > 2400
    ids = np.unique(np.concatenate([sample, reported, rng.choice(fine, 2400, replace=False)]))
    assert np.isin(sample, ids).all() and np.isin(reported, ids).all()
    posts = np.stack([ids // p.per_tile, ids % p.per_tile], axis=-1).astype(np.uint32)
    for run in RUN_RADII:
        radius = MC.params("grid", run)[0]
        fast, bad = SE.isolation(tiles, order, posts, radius)
        slow, bad2 = SE.isolation(tiles, order, posts, radius, brute=True)
        assert bad == 0 and bad2 == 0 and same_bits(fast, slow, FIELDS), run


@pytest.mark.parametrize("name", MC.SMALL)
def test_staged_search_equals_brute_force(name):
    """The prefilter, the any-hit stage and the closest-hit stage together give what the rule gives from every post's brute-force
    isolation: the same summits with the same bytes, in tile order."""
    tiles, order, _ = MC.tileset(name)
    p = MC.posts(name)
    posts = all_posts(name)
    for run in MC.RUNS:
        radius, min_iso, min_h = MC.params(name, run)
        slow, _ = SE.isolation(tiles, order, posts, radius, brute=True)
        with np.errstate(invalid="ignore"):
            member = p.exists & (p.h >= np.float32(min_h)) & (slow["isolation_m"] >= min_iso)
        rec, count, stages, bad = MC.emulation(name, run)
        assert bad == 0 and count == int(member.sum()) == len(rec), (name, run, count, int(member.sum()))
        assert same_bits(rec, slow[member], FIELDS + ("rank", "idx")), (name, run)
        assert stages[0] >= stages[1] == count
        if run == "fine":      # below the post spacing the prefilter drops nothing but what does not exist ...
            dropped = 0
            if name == "polar":      # ... and, where row 0 is the pole, the posts of that row a neighbour in the row dominates: they coincide with it
                for hts, *_ in tiles:
                    row = np.asarray(hts)[0].astype(np.float64)
                    assert np.isfinite(row).all()
                    left = np.concatenate([[False], (row[:-1] >= row[1:])])       # the left neighbour is as high: the lower index wins a tie
                    right = np.concatenate([row[1:] > row[:-1], [False]])
                    dropped += int((left | right).sum())
                assert dropped > 0
            assert stages[0] == int(p.exists.sum()) - dropped, (name, stages, int(p.exists.sum()), dropped)


@pytest.mark.parametrize("name", tuple(MC.TILESETS))
@pytest.mark.parametrize("run", MC.RUNS)
def test_emulation_agrees_with_the_reference(name, run):
    rec, count, _, bad = MC.emulation(name, run)
    assert bad == 0 and count == len(rec)
    MC.compare_with_reference(name, run, rec, f"{name}/{run}")


@pytest.mark.parametrize("name", tuple(MC.TILESETS))
def test_snap(name):
    tiles, order, _ = MC.tileset(name)
    pts, n_random, radius = MC.snap_points(name)
    ref, emu = MC.snap_reference(name)
    MC.compare_snap(ref, emu, n_random, name)
    assert (emu["status"][-4:] == SE.INVALID).all() and (emu["status"][-6:-4] == SE.NONE).all()
    for f in ("lon_deg", "lat_deg", "distance_m", "height_m", "rank", "idx"):
        assert not emu[f][emu["status"] != SE.FOUND].any()
    if name != "grid":
        slow, bad = SE.snap(tiles, order, pts, radius, brute=True)
        assert bad == 0 and emu.tobytes() == slow.tobytes()
    p = MC.posts(name)
    found = emu["status"] == SE.FOUND
    flat = emu["rank"][found].astype(np.int64) * p.per_tile + emu["idx"][found]
    assert np.array_equal(emu["lon_deg"][found], p.lon_deg[flat]) and np.array_equal(emu["lat_deg"][found], p.lat_deg[flat])


def test_spikes_by_hand():
    """Three posts of 300, 200 and 100 m on a plain of 0 m, min_height 1 m: three summits, each isolated by the chord to the nearest
    higher spike, formed here from the posts' longitudes and latitudes."""
    tiles, order, _ = MC.tileset("spikes")
    rec, count, _, _ = SE.summits(tiles, order, 400.0e3, 0.0, 1.0)
    assert count == 3
    tile = tiles[0]
    ll = {h: np.radians(MC.SC.vertex_lonlat(tile, x, y)) for x, y, h in MC.SPIKES}
    def unit(l):
        return np.array([np.cos(l[1]) * np.cos(l[0]), np.cos(l[1]) * np.sin(l[0]), np.sin(l[1])])
    by_height = {float(r["height_m"]): r for r in rec}
    assert sorted(by_height) == [100.0, 200.0, 300.0]
    assert np.isinf(by_height[300.0]["isolation_m"]) and by_height[300.0]["has_higher"] == 0
    for h, higher in ((200.0, (300.0,)), (100.0, (300.0, 200.0))):
        d = min(MC.R0 * np.linalg.norm(unit(ll[h]) - unit(ll[q])) for q in higher)
        assert abs(by_height[h]["isolation_m"] - d) <= 1e-6, (h, by_height[h]["isolation_m"], d)
    order_xy = [(int(r["idx"]) % 24, int(r["idx"]) // 24) for r in rec]
    assert order_xy == sorted(order_xy, key=lambda p: p[1] * 24 + p[0])      # tile order


def test_plateau_has_one_summit_at_its_lowest_index():
    tiles, order, _ = MC.tileset("plateau")
    s, _ = MC.spacing("plateau")
    hill = tiles[0][0]
    flat = np.nonzero(hill.ravel() == hill.max())[0]
    assert len(flat) > 1
    for k, first in ((0, int(flat.min())), (1, 0)):      # each tile on its own: the hill's plateau, the constant tile
        rec, count, _, _ = SE.summits(tiles[k:k + 1], order[k:k + 1], 400.0e3, 8.0 * s, -np.inf)
        assert count == 1 and (int(rec[0]["rank"]), int(rec[0]["idx"])) == (0, first) and np.isinf(rec[0]["isolation_m"])
    rec, count, _, _ = SE.summits(tiles, order, 400.0e3, 8.0 * s, -np.inf)      # together: the hill stands over the constant tile
    assert count == 1 and (int(rec[0]["rank"]), int(rec[0]["idx"])) == (0, int(flat.min()))


def test_duplicated_posts_report_the_lower_rank_only():
    tiles, order, _ = MC.tileset("overlap")
    for run in ("near", "fine"):
        rec = MC.emulation("overlap", run)[0]
        dup = (rec["rank"] == 1) & (rec["idx"] % 24 < 8)      # columns 0 .. 7 of the second tile are columns 16 .. 23 of the first
        assert not dup.any(), run
    rec0 = SE.summits(tiles, order, *MC.params("overlap", "near")[:1], 0.0, -np.inf)[0]      # min_isolation 0: every post is a summit
    assert ((rec0["rank"] == 1) & (rec0["idx"] % 24 < 8)).any()


def test_min_height_is_honoured():
    for name in ("blocks", "ridges_ne"):
        low, high = MC.emulation(name, "near")[0], MC.emulation(name, "high")[0]
        cut = np.float32(MC.params(name, "high")[2])
        assert (high["height_m"] >= cut).all() and len(high) < len(low)
        keep = low[low["height_m"] >= cut]
        assert keep.tobytes() == high.tobytes()


def test_orders_and_truncation():
    """The host's orders, restated: T.order_summits is what topo_summits_read applies to the device's tile-order set."""
    rec = MC.emulation("blocks", "near")[0]
    assert len(rec) > 8
    h = T.order_summits(rec, T.SUMMIT_ORDER_HEIGHT)
    assert (np.diff(h["height_m"]) <= 0).all() and sorted(h.tolist()) == sorted(rec.tolist())
    i = T.order_summits(rec, T.SUMMIT_ORDER_ISOLATION)
    assert (np.diff(i["isolation_m"][np.isfinite(i["isolation_m"])]) <= 0).all() and np.isinf(i["isolation_m"][0])
    n_inf = int(np.isinf(i["isolation_m"]).sum())
    assert np.isinf(i["isolation_m"][:n_inf]).all() and (np.diff(i["height_m"][:n_inf]) <= 0).all()
    assert T.order_summits(rec, T.SUMMIT_ORDER_TILE).tobytes() == rec.tobytes()
    cut = SE.summits(*MC.tileset("blocks")[:2], *MC.params("blocks", "near"), capacity=5)
    assert cut[1] == len(rec) and cut[0].tobytes() == rec[:5].tobytes()


def test_struct_sizes_against_the_header(tmp_path):
    exe = str(tmp_path / "summits_abi_harness")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(os.path.dirname(HERE), "include"), os.path.join(HERE, "summits_abi_harness.c"), "-o", exe])
    out = subprocess.check_output([exe], text=True).split()
    assert out == ["24", "64", "48", "0", "1", "2", "1", "0", "-1"], out
    assert T.SUMMIT_DTYPE.itemsize == 64 and T.SUMMIT_SNAP_DTYPE.itemsize == 48 and T.SUMMIT_PARAMS_DTYPE.itemsize == 24
