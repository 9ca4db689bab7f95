"""Summit queries on the GPU (topo_summits_*, topo_summit_snap_*): the kernels of kernels_summits.h against the g++ build of the same
rule (tests/summits_emul.py) and the numpy reference (tests/summits_ref.py) on the tile sets of tests/summits_cases.py, the calls'
contract, and their side effects (none).

Comparison rule.  Identity -- the summit set, its order, tile, vx, vy, the heights, the count -- equals the emulation's exactly.
lon_deg / lat_deg within 1e-9 degrees and isolation_m / distance_m within 1e-6 m of the emulation's: the device's trig tables may
differ from the host's by an ulp (2e-16 of a direction), which moves a chord by about R0 2e-16 = 1e-9 m; 1e-6 m is that with three
decades to spare, not a tuned number.  Against the reference 1e-3 m.  Device and emulation may name another nearest dominator only
where the reference finds a runner-up within 1e-3 m."""
import hashlib

import numpy as np
import pytest

import summits_cases as MC
import summits_emul as SE
from gpu_support import checked_run, padded_device_output, renderer, strip

pytestmark = pytest.mark.gpu


def _device(g, params, capacity, pad=3):
    """summits_device into a 0xAB-filled tensor of capacity + pad records and a count word among three others:
    (records [:min(count, capacity)], count, everything else of both tensors)."""
    import torch
    import topo_renderer_amd as T
    cnt = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    raw, padding = padded_device_output(g, 1, 1, capacity, 64, lambda p, stride, pitch: g.summits_device(p, capacity, cnt.data_ptr(), *params), pad_cols=pad)
    words = cnt.cpu().numpy().view(np.uint32)
    count = int(words[0])
    rec = raw.reshape(-1).view(T.SUMMIT_DTYPE)
    n = min(count, capacity)
    rest = np.concatenate([padding, rec[n:].view(np.uint8), (words[1:] != 0xFFFFFFFF).astype(np.uint8) * 0xAB ^ 0xAB])
    return rec[:n].copy(), count, rest


def _as_device(emu, order, tile_w):
    """The emulation's records in topo_summit's identity fields."""
    import topo_renderer_amd as T
    out = np.zeros(len(emu), T.SUMMIT_DTYPE)
    ll = np.asarray(order, np.int32).reshape(-1, 2)
    has = emu["has_higher"] > 0
    out["tile_lat_deg"], out["tile_lon_deg"] = ll[emu["rank"], 0], ll[emu["rank"], 1]
    out["vx"], out["vy"] = emu["idx"] % tile_w, emu["idx"] // tile_w
    out["higher_tile_lat_deg"], out["higher_tile_lon_deg"] = np.where(has, ll[emu["higher_rank"], 0], 0), np.where(has, ll[emu["higher_rank"], 1], 0)
    out["higher_vx"], out["higher_vy"] = np.where(has, emu["higher_idx"] % tile_w, 0), np.where(has, emu["higher_idx"] // tile_w, 0)
    for f in ("lon_deg", "lat_deg", "isolation_m", "height_m", "higher_height_m"):
        out[f] = emu[f]
    return out


OWN = ("tile_lat_deg", "tile_lon_deg", "vx", "vy")
HIGHER = ("higher_tile_lat_deg", "higher_tile_lon_deg", "higher_vx", "higher_vy", "higher_height_m")


def _against_emulation(got, count, name, run, what):
    tiles, order, _ = MC.tileset(name)
    tile_w = tiles[0][0].shape[1]
    emu, n, _, _ = MC.emulation(name, run)
    want = _as_device(emu, order, tile_w)
    assert count == n == len(got), f"{what}: {count} summits, the emulation has {n}"
    for f in OWN:
        assert np.array_equal(got[f], want[f]), f"{what}: {f} differs"
    assert got["height_m"].tobytes() == want["height_m"].tobytes()
    assert np.abs(got["lon_deg"] - want["lon_deg"]).max(initial=0.0) <= 1e-9 and np.abs(got["lat_deg"] - want["lat_deg"]).max(initial=0.0) <= 1e-9
    fin = np.isfinite(want["isolation_m"])
    assert np.array_equal(np.isfinite(got["isolation_m"]), fin) and np.isinf(got["isolation_m"][~fin]).all(), f"{what}: finite / infinite isolation differs"
    err = np.abs(got["isolation_m"][fin] - want["isolation_m"][fin])
    ref = MC.reference(name, run)
    ref = ref[ref["member"]]
    differ = np.zeros(len(got), bool)
    for f in HIGHER:
        differ |= got[f] != want[f]
    print(f"{what}: {count} summits, isolation within {err.max(initial=0.0):.3e} m of the emulation's, {int(differ.sum())} other dominators "
          f"({int(ref['higher_ambiguous'].sum())} ambiguous)")
    assert (err <= 1e-6).all(), f"{what}: isolation differs from the emulation's by {err.max():.3e} m"
    assert not (differ & ~ref["higher_ambiguous"]).any(), f"{what}: another dominator where the reference finds no runner-up"
    none = ~fin
    for f in HIGHER:
        assert not got[f][none].any(), "no dominator: every higher_* field is 0"
    # the device's own records against the reference
    mine = np.zeros(len(got), SE.OUT_DTYPE)
    mine["rank"], mine["idx"], mine["height_m"], mine["isolation_m"], mine["has_higher"] = emu["rank"], emu["idx"], got["height_m"], got["isolation_m"], fin
    rank_of = {tuple(ll): r for r, ll in enumerate(order)}
    mine["higher_rank"] = [rank_of[(int(a), int(b))] if f else 0 for a, b, f in zip(got["higher_tile_lat_deg"], got["higher_tile_lon_deg"], fin)]
    mine["higher_idx"] = np.where(fin, got["higher_vy"] * tile_w + got["higher_vx"], 0)
    MC.compare_with_reference(name, run, mine, f"{what} (device)")


@pytest.mark.parametrize("name", tuple(MC.TILESETS))
def test_cases(topo, name):
    """Every tile set, every run: the device call into padded outputs, the host read, the emulation and the reference."""
    tiles, order, _ = MC.tileset(name)
    g = renderer(topo, tiles, order)
    for run in MC.RUNS:
        params = MC.params(name, run)
        n = MC.emulation(name, run)[1]
        rec, count, rest = _device(g, params, n + 2)
        assert (rest == 0xAB).all(), "nothing is written beyond the records and the count"
        read, n_read = g.summits(*params, capacity=n + 2)
        assert n_read == count and read.tobytes() == rec.tobytes(), "topo_summits_read gives the device call's bytes"
        _against_emulation(rec, count, name, run, f"{name}/{run}")
    g.close()


@pytest.mark.parametrize("name", tuple(MC.TILESETS))
def test_snap(topo, name):
    import torch
    tiles, order, _ = MC.tileset(name)
    tile_w = tiles[0][0].shape[1]
    pts, n_random, radius = MC.snap_points(name)
    ref, emu = MC.snap_reference(name)
    g = renderer(topo, tiles, order)
    src = torch.from_numpy(pts.copy()).cuda()
    raw, pad = padded_device_output(g, 1, 1, len(pts), 48, lambda p, stride, pitch: g.summit_snap_device(src.data_ptr(), len(pts), radius, p), pad_cols=2)
    got = raw.reshape(-1).view(topo.SUMMIT_SNAP_DTYPE)
    read = g.summit_snap(pts, radius)
    g.close()
    assert (pad == 0xAB).all() and read.tobytes() == got.tobytes()
    sure = ~ref["ambiguous"]
    ll = np.asarray(order, np.int32).reshape(-1, 2)
    found = emu["status"] == SE.FOUND
    assert np.array_equal(got["status"][sure], emu["status"][sure])
    same = sure & found
    assert np.array_equal(got["tile_lat_deg"][same], ll[emu["rank"][same], 0]) and np.array_equal(got["tile_lon_deg"][same], ll[emu["rank"][same], 1])
    assert np.array_equal(got["vx"][same], emu["idx"][same] % tile_w) and np.array_equal(got["vy"][same], emu["idx"][same] // tile_w)
    assert got["height_m"][same].tobytes() == emu["height_m"][same].tobytes()
    assert np.abs(got["distance_m"][same] - emu["distance_m"][same]).max(initial=0.0) <= 1e-6
    assert np.abs(got["lon_deg"][same] - emu["lon_deg"][same]).max(initial=0.0) <= 1e-9 and np.abs(got["lat_deg"][same] - emu["lat_deg"][same]).max(initial=0.0) <= 1e-9
    off = got["status"] != topo.SNAP_FOUND
    for f in ("lon_deg", "lat_deg", "distance_m", "height_m", "tile_lat_deg", "tile_lon_deg", "vx", "vy"):
        assert not got[f][off].any(), "not found: every other field is 0"
    mine = np.zeros(len(got), SE.SNAP_DTYPE)
    rank_of = {tuple(x): r for r, x in enumerate(order)}
    mine["status"], mine["height_m"], mine["distance_m"] = got["status"], got["height_m"], got["distance_m"]
    mine["rank"] = [rank_of[(int(a), int(b))] if s == 1 else 0 for a, b, s in zip(got["tile_lat_deg"], got["tile_lon_deg"], got["status"])]
    mine["idx"] = got["vy"] * tile_w + got["vx"]
    MC.compare_snap(ref, mine, n_random, f"{name} (device)")


def test_twice_and_in_bands_give_the_same_bytes(topo):
    for name, run, rows in (("ridges_ne", "near", 5), ("blocks", "fine", 3), ("grid", "wide", 64), ("overlap", "near", 1)):
        tiles, order, _ = MC.tileset(name)
        g = renderer(topo, tiles, order)
        params, n = MC.params(name, run), MC.emulation(name, run)[1]
        first = _device(g, params, n + 1)
        again = _device(g, params, n + 1)
        counts = g.debug_summit_counts()
        g.debug_set_summit_band_rows(rows)
        banded = _device(g, params, n + 1)
        banded_counts = g.debug_summit_counts()
        g.debug_set_summit_band_rows(0)
        whole = _device(g, params, n + 1)
        g.close()
        assert first[1] == again[1] == banded[1] == whole[1] == n and n > 0
        assert first[0].tobytes() == again[0].tobytes() == banded[0].tobytes() == whole[0].tobytes(), (name, run)
        assert (banded[2] == 0xAB).all() and counts == banded_counts and counts["summits"] == n
        assert counts["candidates"] == MC.emulation(name, run)[2][0], "the prefilter keeps what the emulation's keeps"


def test_capacity_smaller_than_the_count(topo):
    name, run = "blocks", "near"
    tiles, order, _ = MC.tileset(name)
    params, n = MC.params(name, run), MC.emulation(name, run)[1]
    g = renderer(topo, tiles, order)
    full, count, _ = _device(g, params, n)
    for cap in (n - 1, 7, 1, 0):
        rec, c, rest = _device(g, params, cap, pad=4) if cap else (full[:0], None, None)
        if cap:
            assert c == n and rec.tobytes() == full[:cap].tobytes() and (rest == 0xAB).all(), cap
        out = np.full(cap + 2, 0xAB, np.uint8).repeat(64).view(topo.SUMMIT_DTYPE)
        got = topo.C.c_uint32(0)
        p = topo.summit_params(*params, order=topo.SUMMIT_ORDER_HEIGHT)
        rc = topo.lib().topo_summits_read(g._h, p.ctypes.data_as(topo.C.c_void_p), out.ctypes.data_as(topo.C.c_void_p) if cap else None, cap, topo.C.byref(got))
        assert rc == topo.TOPO_ERR_CAPACITY and got.value == n
        assert out[:cap].tobytes() == topo.order_summits(full, topo.SUMMIT_ORDER_HEIGHT)[:cap].tobytes(), "ordered first, then truncated"
        assert (out[cap:].view(np.uint8) == 0xAB).all()
    for order_ in (topo.SUMMIT_ORDER_TILE, topo.SUMMIT_ORDER_HEIGHT, topo.SUMMIT_ORDER_ISOLATION):
        rec, c = g.summits(*params, order=order_)
        assert c == n and rec.tobytes() == topo.order_summits(full, order_).tobytes()
    g.close()


def test_errors_and_no_ops(topo):
    import torch
    tiles, order, _ = MC.tileset("blocks")
    radius, min_iso, _ = MC.params("blocks", "near")
    g = renderer(topo, tiles, order)
    out = torch.full((8 * 64 + 16,), 0xAB, dtype=torch.uint8, device="cuda")
    cnt = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    pts = torch.zeros((4, 2), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    o, c, q = out.data_ptr(), cnt.data_ptr(), pts.data_ptr()
    ok = dict(out_ptr=o, capacity=8, count_ptr=c, radius_m=radius, min_isolation_m=min_iso, min_height_m=0.0)
    for change in (dict(radius_m=0.0), dict(radius_m=-1.0), dict(radius_m=np.nan), dict(radius_m=np.inf), dict(radius_m=1.0e6 + 1.0), dict(min_isolation_m=-1.0),
                   dict(min_isolation_m=radius * 1.01), dict(min_isolation_m=np.nan), dict(min_height_m=np.nan), dict(order=topo.SUMMIT_ORDER_HEIGHT), dict(order=3),
                   dict(out_ptr=o + 8), dict(out_ptr=0), dict(count_ptr=0), dict(count_ptr=c + 2)):
        with pytest.raises(topo.TopoError) as err:
            g.summits_device(**dict(ok, **change))
        assert err.value.code == topo.TOPO_ERR_INVALID, change
    for args in ((q, 4, 0.0, o), (q, 4, np.nan, o), (q, 4, 1.0e6 + 1.0, o), (q + 8, 4, radius, o), (q, 4, radius, o + 8), (0, 4, radius, o), (q, 4, radius, 0)):
        with pytest.raises(topo.TopoError) as err:
            g.summit_snap_device(*args)
        assert err.value.code == topo.TOPO_ERR_INVALID, args
    with pytest.raises(topo.TopoError):
        g.summits(radius, min_iso, order=7)
    g.summit_snap_device(q, 0, radius, o)      # n == 0: a no-op
    assert len(g.summit_snap(np.zeros((0, 2)), radius)) == 0
    g.synchronize()
    assert (out.cpu().numpy() == 0xAB).all() and (cnt.cpu().numpy() == -1).all(), "a refused call and a no-op write nothing"
    g.summits_device(**dict(ok, min_height_m=-np.inf, min_isolation_m=radius, capacity=0, out_ptr=0))      # the limits are inside; no records wanted
    g.synchronize()
    assert cnt.cpu().numpy()[0] > 0 and (out.cpu().numpy() == 0xAB).all()
    g.close()
    empty = topo.TerrainRenderer(64, 48)      # no tiles: the count is 0, snap statuses are NONE
    cnt.fill_(-1)
    torch.cuda.synchronize()
    empty.summits_device(**ok)
    empty.synchronize()
    assert cnt.cpu().numpy().tolist() == [0, -1, -1, -1] and (out.cpu().numpy() == 0xAB).all()
    rec, n = empty.summits(radius, min_iso)
    assert n == 0 and len(rec) == 0
    snap = empty.summit_snap([[7.5, 46.5], [np.nan, 0.0]], radius)
    assert snap["status"].tolist() == [topo.SNAP_NONE, topo.SNAP_INVALID]
    empty.close()


def test_summit_calls_change_no_frame_and_follow_the_tile_set(topo):
    """The calls' bytes are the same before a frame, after one and beside two in flight; frames are those of a renderer that made no
    such call; after unload_terrain -- no frame in between -- the answer is that of the tiles that are left."""
    import torch
    from scenes import Scene, assert_same_frame
    sc = Scene(96, 2, 2, eye_dh=100.0)
    tiles, order = MC.LC.scene_tiles(sc)
    s = MC.R0 * np.radians(1.0 / 96.0)
    params = (4.37 * s, 2.13 * s, -np.inf)
    W, H = 256, 160
    a, b = topo.TerrainRenderer(W, H), topo.TerrainRenderer(W, H)
    sc.load(a)
    sc.load(b)
    pu = topo.post_uniforms(W, H)
    first, n = b.summits(*params)
    emu, n_emu, _, _ = SE.summits(tiles, order, *params)
    assert n == n_emu > 4 and np.array_equal(first["vx"], emu["idx"] % 96) and np.array_equal(first["vy"], emu["idx"] // 96)
    pts = np.stack([first["lon_deg"] + 0.003, first["lat_deg"] - 0.002], axis=-1)
    snap0 = b.summit_snap(pts, 3.0 * s)
    u = sc.uniforms(W, H, 40, 10, 70, 0)
    a.update(W, H, u, pu)
    b.update(W, H, u, pu)
    ra, rb = a.render(), b.render()
    assert_same_frame(ra, rb, "summit calls vs none")
    sha = hashlib.sha256(np.ascontiguousarray(rb[0]).tobytes() + np.ascontiguousarray(rb[1]).tobytes()).hexdigest()
    got, _ = b.summits(*params)
    assert got.tobytes() == first.tobytes() and b.summit_snap(pts, 3.0 * s).tobytes() == snap0.tobytes(), "the answers do not depend on a frame before them"
    rb2 = b.render()
    assert hashlib.sha256(np.ascontiguousarray(rb2[0]).tobytes() + np.ascontiguousarray(rb2[1]).tobytes()).hexdigest() == sha, "the same frame after a summit call"
    a.render()
    assert a.counters() == b.counters() and a.frame_status() == b.frame_status()
    # the terrain under every summit is that post (topo_surface_read at an exact post)
    surf = b.surface(np.stack([first["lon_deg"], first["lat_deg"]], axis=-1))
    assert (surf["kind"] == topo.SURFACE_TERRAIN).all() and np.abs(surf["height_m"] - first["height_m"]).max() <= 1e-3
    # two submissions in flight, the device variants queued before the join
    sw, sh = 48, 40
    us = sc.panorama(sw, sh, yaw0_deg=25.0)
    rec = torch.zeros(((n + 1) * 64,), dtype=torch.uint8, device="cuda")
    cnt = torch.zeros((4,), dtype=torch.int32, device="cuda")
    src = torch.from_numpy(pts.copy()).cuda()
    snp = torch.zeros((len(pts) * 48,), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    frames = []
    for r, ask in ((a, False), (b, True)):
        r.set_stream(torch.cuda.current_stream().cuda_stream)
        r.set_pipeline_depth(2)
        keep = [strip(r, us[:2], sw, sh), strip(r, us[2:7], sw, sh)]
        if ask:
            r.summits_device(rec.data_ptr(), n + 1, cnt.data_ptr(), *params)
            r.summit_snap_device(src.data_ptr(), len(pts), 3.0 * s, snp.data_ptr())
        r.join()
        r.synchronize()
        frames.append([(c.cpu().numpy(), d.cpu().numpy()) for c, d in keep])
    for (ca, da), (cb, db) in zip(frames[0], frames[1]):
        assert np.array_equal(ca, cb) and np.array_equal(da.view(np.uint32), db.view(np.uint32))
    assert int(cnt.cpu().numpy()[0]) == n and rec.cpu().numpy()[:n * 64].tobytes() == first.tobytes() and snp.cpu().numpy().tobytes() == snap0.tobytes()
    # a tile less, no frame in between
    lat, lon = order[1]
    b.unload_terrain(lat, lon)
    left_tiles, left_order = [t for k, t in enumerate(tiles) if k != 1], [o for k, o in enumerate(order) if k != 1]
    emu, n_emu, _, _ = SE.summits(left_tiles, left_order, *params)
    got, n_got = b.summits(*params)
    ll = np.asarray(left_order, np.int32)
    assert n_got == n_emu and np.array_equal(got["vx"], emu["idx"] % 96) and np.array_equal(got["vy"], emu["idx"] // 96) and np.array_equal(got["tile_lon_deg"], ll[emu["rank"], 1])
    assert np.abs(got["isolation_m"][np.isfinite(emu["isolation_m"])] - emu["isolation_m"][np.isfinite(emu["isolation_m"])]).max(initial=0.0) <= 1e-6
    a.close()
    b.close()


def _checked_run(T):
    """Ragged blocks, two batches of blocks in bands, a gap, voids and the pole, and a snap -> hash of every output, status."""
    import torch
    h = hashlib.sha256()
    status = 0
    for name, run, rows in (("blocks", "near", 0), ("grid", "wide", 37), ("ridges_ne", "fine", 5), ("void_nan", "near", 0), ("polar", "wide", 0)):
        tiles, order, _ = MC.tileset(name)
        g = renderer(T, tiles, order)
        g.debug_set_summit_band_rows(rows)
        rec, count = g.summits(*MC.params(name, run))
        pts, _, radius = MC.snap_points(name)
        h.update(rec.tobytes() + g.summit_snap(pts, radius).tobytes() + str(count).encode())
        status |= g.frame_status()["status"]
        g.close()
    torch.cuda.synchronize()
    return {"sha": h.hexdigest()[:24], "status": status}


def test_bounds_checked_build_records_no_out_of_range_index(topo):
    got = checked_run("test_summits_gpu")      # kStatusBounds: an index a summit kernel formed was out of range
    assert got["sha"] == _checked_run(topo)["sha"], "the bounds-checked build answers as the product build"
