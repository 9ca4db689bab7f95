"""The cull's reference (tests/cull_ref.py) and scenes (tests/cull_cases.py) held to what tests/test_cull_gpu.py needs of them, with no
device involved: the slab's faces are planes, the sideways bulge of a block's equator-side edge against its radial sagitta, every
bulge pose puts that bulge on the screen beyond the slab-corner box, every list scene shows all five classes of blocks, and the
oracle's f32 vertex positions stay within the 64 m the bounding spheres allow for them."""
import math

import numpy as np
import pytest

import cull_cases as CC
import cull_ref as CR


def _flat_block(first_row_deg, ratio, height=3000.0):
    """Block 0 of a 1200-row tile at `height` whose columns are `ratio` times as wide in degrees as its rows."""
    tw = 1200 // ratio
    tr = CC.transform(first_row_deg - 1, 15, tw, 1200)
    return CR.BlockRef(np.full((1200, tw), height, np.float32), tr, 0)


# first row (deg), lon cell / lat cell, sagitta (m), sideways bulge (m): a full 60 x 15 cell block of a 1200-row tile at 3000 m
BULGE_TABLE = [(46, 1, 0.33, 0.30), (56, 1, 0.23, 0.28), (61, 2, 0.61, 1.03), (71, 3, 0.62, 1.68), (81, 5, 0.41, 2.35),
               (86, 10, 0.33, 4.24)]      # (the last sagitta is 0.3346 m by block_bounds_store's expression; the issue's table prints 0.34)


@pytest.mark.parametrize("first_row,ratio,sagitta,bulge", BULGE_TABLE)
def test_bulge_against_sagitta(first_row, ratio, sagitta, bulge):
    """The radial sagitta gates the occlusion filter at 1 m; the equator-side edge's sideways excursion is another quantity, and in
    the COP90 width bands it exceeds 1 m where the sagitta does not."""
    b = _flat_block(first_row, ratio)
    ex = CR.excursions(b.edge_vertices(), b.faces())
    assert b.side == "last_row"
    assert round(b.sagitta, 2) == sagitta and round(ex[b.side], 2) == bulge, (b.sagitta, ex)
    # the edge's excursion is the block's: no vertex sticks out further sideways, none through the other three side faces
    every = CR.excursions(b.vertices, b.faces())
    assert abs(every[b.side] - ex[b.side]) < 1e-9 and all(every[k] < 1e-6 for k in ("west", "east", "first_row")), every
    # R (dlon^2 / 8) sin(lat) cos(lat), to the second order
    la = CR.lat_rad(CC.transform(first_row - 1, 15, 1200 // ratio, 1200), 15)
    dlon = math.radians(60.0 * ratio / 1200.0)
    assert ex[b.side] == pytest.approx((CR.R0 + 3000.0) * dlon ** 2 / 8.0 * math.sin(la) * math.cos(la), rel=2e-3)


def test_slab_faces_are_planes():
    """Eight slab corners, six faces of four corners each: every face is planar to 1e-6 m, the four side faces pass through the origin."""
    blocks = [_flat_block(r, k) for r, k, _, _ in BULGE_TABLE] + [CC.bulge_case(n).ref for n in CC.BULGE]
    for name, tw, th in CC.TABLE_CASES:
        t = CC.table_case(name, tw, th)
        blocks += [t.ref(loc, blk) for loc in t.locs for blk in range(t.n_blocks)]
    n = 0
    for b in blocks:
        if not (b.ordered and np.isfinite(b.hmin) and np.isfinite(b.hmax)):
            continue
        n += 1
        for face, (normal, d, flat) in b.faces().items():
            assert flat <= 1e-6, (b.blk, face, flat)
            if face not in ("top", "bottom"):
                assert abs(d) <= 1e-2, (b.blk, face, d)      # (a face a few metres thick, fitted 6400 km from the origin: 1e-2 m there is 2e-9 rad)
    assert n > 200


@pytest.mark.parametrize("name", list(CC.BULGE))
def test_bulge_pose_puts_the_bulge_on_the_screen(name):
    """By the reference alone: the chosen block's sphere lies wholly beyond the split, and its edge's vertices project at least 3 px
    beyond the unclamped slab-corner box (floor / ceil, 2 px outward) on a side the target does not clamp."""
    c = CC.bulge_case(name)
    cond = c.condition()
    print(f"{name}: bulge {cond['bulge_m']:.2f} m, sagitta {c.ref.sagitta:.2f} m, sphere from {cond['w_near']:.0f} m (split {c.split:.0f}), "
          f"box {cond['box']}, overshoot {cond['overshoot_px']:.2f} px")
    assert c.ref.sagitta <= 1.0
    assert cond["w_near"] > c.split
    assert cond["overshoot_px"] >= 3.0
    # the camera looks where it was told to: the near end of the edge on the target (its f32 eye and angles move it up to twenty
    # pixels off the centre at these focal lengths)
    s = CR.screen(CR.clip_coords(c.proj, c.ref.edge_vertices()[-1:]), CC.W, CC.H)[0]
    assert 8 < s[0] < CC.W - 8 and 8 < s[1] < CC.H - 8, s


@pytest.mark.parametrize("name", list(CC.LIST_SCENES))
def test_list_scene_shows_every_class(orc, name):
    """Over its poses a list scene has near blocks, far candidates, survivors, dropped candidates and frustum-culled blocks, by the
    reference's prediction and the oracle's frames."""
    sc = CC.list_scene(name)
    total = {k: 0 for k in CC.LIST_MINIMA}
    for what, u in sc.poses:
        e = CC.expected(orc, ("list", name), sc.tiles, u, sc.split)
        n = CC.predicted_counts(e)
        print(f"{name}, {what}: {n}; terrain in {float((e['depth'] < 1).mean()):.2f} of the frame")
        for k in total:
            total[k] += n[k]
    for k, least in CC.LIST_MINIMA.items():
        assert total[k] >= least, (name, k, total)
    if name == "void":
        loc = CC.LIST_SCENES[name][0]
        assert sum(1 for b in range(sc.tiles.n_blocks) if not sc.tiles.ref(loc, b).ordered) == 1
        assert sum(1 for b in range(sc.tiles.n_blocks) if sc.tiles.ref(loc, b).ordered and not sc.tiles.ref(loc, b).finite) >= 1


def test_f32_vertex_path_stays_within_the_spheres_allowance(orc):
    """The bounding spheres carry 64 m "for the f32 noise of the real vertex path": the oracle's f32 geometry_transform of a vertex
    (f32 longitude and latitude from the tile transform, as vs_main forms them) against the ideal f64 position, 2000 vertices with a finite height a scene.  Largest distances found:
    0.9 to 1.1 m at 45N 15E, on the equator and at 60 to 81 degrees of latitude, 1.45 to 1.82 m at longitude 180."""
    rng = np.random.default_rng(11)
    scenes = [(f"{n} {tw}x{th}", CC.table_case(n, tw, th)) for n, tw, th in CC.TABLE_CASES] + [(f"bulge {n}", CC.bulge_case(n).tiles) for n in CC.BULGE]
    worst = 0.0
    for what, t in scenes:
        w, measured = 0.0, 0
        while measured < 2000:      # vertices with a finite height, the tiles in turn
            loc = t.locs[measured % len(t.locs)]
            hts, tr = t.tiles[loc]
            rp, mp, ps = (np.asarray(a, np.float32) for a in tr)
            x, y = int(rng.integers(0, t.tw)), int(rng.integers(0, t.th))
            h = hts[y, x]
            if not np.isfinite(h):
                continue
            measured += 1
            lon, lat = (np.float32(x) - rp[0]) * ps[0] + mp[0], (np.float32(y) - rp[1]) * -ps[1] + mp[1]
            ideal = (CR.R0 + float(h)) * CR.direction(CR.lon_rad(tr, x), CR.lat_rad(tr, y))
            w = max(w, float(np.linalg.norm(orc.geometry_transform(h, lon, lat).astype(np.float64) - ideal)))
        print(f"{what}: f32 vertex path within {w:.2f} m of the ideal position ({measured} vertices)")
        assert measured >= 2000 and w < 64.0, (what, w)
        worst = max(worst, w)
    print(f"largest: {worst:.2f} m")
    # The far box's margin (kernels_frame.h, kFarNoiseM = 8 m) counts on this too: 1.8 m was the largest found when it was set (at
    # longitude 180, where an f32 degree has its coarsest step), and 1.5 m-equivalents of clip-space rounding come on top.
    assert worst + 1.5 < 8.0, worst


@pytest.mark.parametrize("name,tw,th", CC.TABLE_CASES)
def test_block_bounds_on_the_host(name, tw, th):
    """block_bounds_store (csrc/topo_cull.h, the function the load kernels call for every block) built for the host with the host's
    sin / cos: sphere, corner directions, sagitta and bulge of every block of every table case against the reference, with the GPU
    test's tolerances.  The block minima / maxima are the kernels' own reductions and are not emulated: the reference's are handed in."""
    import cull_emul
    tiles = CC.table_case(name, tw, th)

    def read(lat, lon):
        hts, tr = tiles.tiles[(lat, lon)]
        return cull_emul.tile_tables(hts, tr, [[tiles.ref((lat, lon), b).hmin, tiles.ref((lat, lon), b).hmax] for b in range(tiles.n_blocks)])

    CC.assert_tables(tiles, read, f"host {name} {tw}x{th}")
