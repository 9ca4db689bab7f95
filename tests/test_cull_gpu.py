"""The three filters every frame passes -- the load-time block tables, the frustum cull and the near / far split with the far
candidates' pixel box and depth bound -- against geometry computed another way: tests/cull_ref.py (numpy f64) for the tables and the
slab, the oracle's own f32 vertex path and its frame's winners for what the lists may leave out.  The scenes are tests/cull_cases.py's;
the lists come from topo_debug_read_cull_lists after one render."""
import numpy as np
import pytest

import cull_cases as CC
import cull_ref as CR
from scenes import assert_same_frame

pytestmark = pytest.mark.gpu


# ---- tables ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["default", "separate"])
@pytest.mark.parametrize("name,tw,th", CC.TABLE_CASES)
def test_block_tables_against_f64_geometry(topo, name, tw, th, path):
    """Every block of every table case, through the load path the tile size takes by default (480-column tiles: the one-pass path)
    and through k_block_tables + the LDS-tile normals kernel, after add_terrain and after the batched recompute_normals."""
    tiles = CC.table_case(name, tw, th)
    g = topo.TerrainRenderer(CC.W, CC.H)
    if path == "separate":
        g.set_normals_lds_rows(8)
    tiles.load(g)
    CC.assert_tables(tiles, g.read_tile_tables, f"{name} {tw}x{th} {path}")
    g.recompute_normals()
    CC.assert_tables(tiles, g.read_tile_tables, f"{name} {tw}x{th} {path}, batched")
    g.close()


# ---- lists ----------------------------------------------------------------------------------------------------------------------------
def _decode(items):
    """{(view, rank, block): [(first cell row, rows)]} of WorkItem records."""
    out = {}
    for vr, b in zip(items["view_rank"].tolist(), items["block"].tolist()):
        out.setdefault((vr >> 16, vr & 0xFFFF, b & 0xFFFFFF), []).append(((b >> 24) & 0xF, b >> 28))
    return out


def _assert_strips(tiles, items, what):
    """Every block of a work list appears once whole, or as strips that cover its cell rows exactly once."""
    for (view, rank, blk), strips in items.items():
        assert view == 0 and rank < len(tiles.order) and blk < tiles.n_blocks, (what, view, rank, blk)
        cell_rows = min(CR.BCY, tiles.th - 1 - (blk // tiles.bxc) * CR.BCY)
        if any(rows == 0 for _, rows in strips):
            assert strips == [(0, 0)], (what, rank, blk, strips)
            continue
        covered = np.zeros(cell_rows, np.int32)
        for first, rows in strips:
            assert first + rows <= cell_rows, (what, rank, blk, strips)
            covered[first:first + rows] += 1
        assert (covered == 1).all(), (what, rank, blk, strips)


def _check_lists(topo, orc, key, tiles, uniforms, split, g, tables, what, must_list=None):
    """One pose: render with the filter on, read the lists, and hold them against the reference and the oracle.  Returns the
    (rank, block) sets near, far, survivors, absent and the prediction."""
    e = CC.expected(orc, key, tiles, uniforms, split)
    o = CC.oracle_of(orc, key, tiles)      # (its last update is this pose's)
    ref_frame = o.render()
    pu = topo.post_uniforms(CC.W, CC.H)
    g.update(CC.W, CC.H, uniforms, pu)
    g.set_occlusion_split(split)
    frame = g.render()
    lists = g.debug_read_cull_lists()
    counters = g.counters()
    # -- partition
    near, surv = _decode(lists["near"]), _decode(lists["survivors"])
    _assert_strips(tiles, near, f"{what} near")
    _assert_strips(tiles, surv, f"{what} survivors")
    far_keys = [(int(v) >> 16, int(v) & 0xFFFF, int(b)) for v, b in zip(lists["far"]["view_rank"], lists["far"]["block"])]
    assert len(set(far_keys)) == len(far_keys), f"{what}: a far candidate appears twice"
    assert all(v == 0 and r < len(tiles.order) and b < tiles.n_blocks for v, r, b in far_keys), what
    far = {(r, b): lists["far"][i] for i, (_, r, b) in enumerate(far_keys)}
    near_set, surv_set = {(r, b) for _, r, b in near}, {(r, b) for _, r, b in surv}
    assert not (near_set & set(far)), f"{what}: near and far at once: {sorted(near_set & set(far))[:4]}"
    assert surv_set <= set(far), f"{what}: survivors that were no candidates: {sorted(surv_set - set(far))[:4]}"
    assert lists["far_tested"] == len(far_keys) == counters["far_tested"], (what, lists["far_tested"], len(far_keys))
    assert lists["far_survived"] == len(lists["survivors"]) == counters["far_survived"], (what, lists["far_survived"], len(lists["survivors"]))
    assert counters["near_blocks"] == len(lists["near"])
    everyone = {(r, b) for r in range(len(tiles.order)) for b in range(tiles.n_blocks)}
    absent = everyone - near_set - set(far)
    # -- classification
    for (rank, blk) in far:
        mm, sag = tables[rank]["minmax"][blk], tables[rank]["bounds"][16 * tiles.n_blocks + blk]
        assert mm[0] <= mm[1] and sag <= 1.0, (what, rank, blk, mm, sag)
    # A block with a NaN in it: the block minima / maxima are fminf / fmaxf folds (tests/test_voids_gpu.py pins them down), which a
    # NaN leaves alone, so only a block that is NaN all over has unordered min / max and is near in every view.  A block with SOME
    # NaN vertices has the ordered, finite min / max of its finite vertices and is filtered on them like any other block -- the
    # triangles at its NaN vertices do not exist -- so "near in every view" cannot hold for it; what holds is that its finite
    # vertices lie inside its sphere (here) and, where it is a candidate, inside its box and behind its zmin, and that it wins
    # no pixel outside them (the box test below: probe_block leaves the NaN vertices out, the winners are all its pixels).
    for rank, loc in enumerate(tiles.order):
        for blk in range(tiles.n_blocks):
            r = tiles.ref(loc, blk)
            if not r.ordered:
                assert (rank, blk) in near_set, f"{what}: block {blk} of tile {loc} is NaN all over and not near"
            elif not r.finite and np.isfinite(r.hmin) and np.isfinite(r.hmax):
                sph = tables[rank]["bounds"][4 * blk:4 * blk + 4]
                v = r.vertices.reshape(-1, 3)
                v = v[np.isfinite(v).all(axis=1)]
                assert float(np.sqrt(((v - sph[:3]) ** 2).sum(axis=1)).max()) <= sph[3] - 64.0, f"{what}: block {blk} of tile {loc}: a finite vertex outside its sphere"
                if (rank, blk) in absent:
                    assert (rank, blk) not in e["won"], f"{what}: block {blk} of tile {loc} (one NaN vertex) was culled and wins pixels"
    # -- frustum: what is absent wins no pixel and has no vertex inside the clip volume (the oracle's f32 vertex path; only the blocks
    # whose f64 vertices come within 16 m-equivalents of the volume are probed: the f32 path is off by a few metres at most)
    assert not (absent & set(e["won"])), f"{what}: culled blocks that win pixels in the oracle's frame: {sorted(absent & set(e['won']))[:4]}"
    m = np.asarray(CC.proj_of(uniforms), np.float64).reshape(4, 4).T
    tol = [16.0 * (np.linalg.norm(m[k, :3]) + 1.0) for k in range(3)]
    probed = 0
    for (rank, blk) in sorted(absent):
        loc = tiles.order[rank]
        c = CR.clip_coords(CC.proj_of(uniforms), tiles.ref(loc, blk).vertices)
        c = c[np.isfinite(c).all(axis=1)]
        close = (np.abs(c[:, 0]) <= c[:, 3] + tol[0]) & (np.abs(c[:, 1]) <= c[:, 3] + tol[1]) & (c[:, 2] >= -tol[2]) & (c[:, 2] <= c[:, 3] + tol[2])
        assert not CR.inside_clip(c).any(), f"{what}: block {blk} of tile {loc} was culled with an (f64) vertex inside the clip volume"
        if close.any():
            probed += 1
            inside = CR.inside_clip(CC.probe_block(o, tiles, loc, blk).astype(np.float64))
            assert not inside.any(), f"{what}: block {blk} of tile {loc} was culled with {int(inside.sum())} vertices inside the clip volume"
    # -- far box and depth bound, zero tolerance
    worst_px, worst_z = -np.inf, np.inf
    bad = []
    for (rank, blk), fi in far.items():
        loc = tiles.order[rank]
        s, z = CC.screen_f32(CC.probe_block(o, tiles, loc, blk))
        box = (int(fi["x0"]), int(fi["x1"]), int(fi["y0"]), int(fi["y1"]))
        over, dz = CC.overshoot(box, s), float(z.min()) - float(fi["zmin"])
        worst_px, worst_z = max(worst_px, over), min(worst_z, dz)
        if over > 0.0 or dz < 0.0:
            bad.append((rank, blk, box, round(over, 3), dz))
        if (rank, blk) in e["won"]:
            ys, xs, ds = e["won"][(rank, blk)]
            if not (xs.min() >= box[0] and xs.max() <= box[1] and ys.min() >= box[2] and ys.max() <= box[3] and ds.min() >= fi["zmin"]):
                bad.append((rank, blk, box, "a pixel it wins lies outside the box or in front of zmin"))
    print(f"{what}: near {len(near_set)} far {len(far)} survivors {len(surv_set)} dropped {len(set(far) - surv_set)} absent {len(absent)} "
          f"(probed {probed}); vertices beyond an unclamped box side by at most {worst_px:.2f} px (<= 0: inside), z - zmin at least {worst_z:.3e}")
    assert not bad, f"{what}: {len(bad)} far candidates whose box or depth bound does not hold their block: {bad[:6]}"
    # -- survivors
    missing = set(e["won"]) & set(far) - surv_set
    assert not missing, f"{what}: candidates that win pixels but did not survive: {sorted(missing)[:6]}"
    if must_list is not None:
        assert must_list in near_set or must_list in far, f"{what}: the chosen block {must_list} is in neither list"
    # -- frame
    assert_same_frame(frame, ref_frame, f"{what} filter on")
    g.set_occlusion_split(0.0)
    assert_same_frame(g.render(), ref_frame, f"{what} filter off")
    whole = _decode(g.debug_read_cull_lists()["near"])
    assert all(s == [(0, 0)] for s in whole.values()) and set((r, b) for _, r, b in whole) >= near_set | set(far), f"{what}: the unfiltered frame's work list"
    return dict(near=near_set, far=set(far), survivors=surv_set, absent=absent, expected=e)


def _renderer(topo, tiles):
    g = topo.TerrainRenderer(CC.W, CC.H)
    tiles.load(g)
    return g, [g.read_tile_tables(*loc) for loc in tiles.order]


@pytest.mark.parametrize("name", list(CC.LIST_SCENES))
def test_cull_lists_ordinary_poses(topo, orc, name):
    """The poses of a list scene: partition, classification, frustum, far box and depth bound, survivors and the frame; and over the
    scene's poses at least the near blocks, candidates, survivors, dropped candidates and culled blocks the reference predicts."""
    sc = CC.list_scene(name)
    g, tables = _renderer(topo, sc.tiles)
    got = {k: 0 for k in ("near", "far", "survivors", "dropped", "absent")}
    want = dict(got)
    for what, u in sc.poses:
        r = _check_lists(topo, orc, ("list", name), sc.tiles, u, sc.split, g, tables, f"{name}, {what}")
        e = r["expected"]
        classes = e["classes"]
        # (a block the reference calls far may be absent: its box can lie off the target where its sphere does not)
        flip = {k for k, c in classes.items() if (c == "culled" and k not in r["absent"]) or (c == "near" and k not in r["near"]) or (c == "far" and k in r["near"])}
        assert not flip, f"{name}, {what}: blocks the reference classifies otherwise: {[(k, classes[k]) for k in sorted(flip)][:6]}"
        assert e["must_drop"] <= r["far"] - r["survivors"], f"{name}, {what}: hidden candidates that survived: {sorted(e['must_drop'] & r['survivors'])[:6]}"
        for k, n in (("near", len(r["near"])), ("far", len(r["far"])), ("survivors", len(r["survivors"])), ("dropped", len(r["far"] - r["survivors"])), ("absent", len(r["absent"]))):
            got[k] += n
        for k, n in CC.predicted_counts(e).items():
            want[k] += n
    print(f"{name}: over the poses {got}; the reference predicts at least {want}")
    for k in got:
        assert want[k] >= CC.LIST_MINIMA[k] and got[k] >= want[k], (name, k, got[k], want[k])
    g.close()


@pytest.mark.parametrize("name", list(CC.BULGE))
def test_cull_lists_bulge_poses(topo, orc, name):
    """The eye on the extension of the chord of a block's equator-side edge: the edge's parallel bows out of the flat-faced slab
    sideways, and the pose puts that on the screen (tests/test_cull_cpu.py holds the pose to it).  The chosen block is in one of the
    lists, and every candidate's box and depth bound hold its block's vertices.

    Measured on an MI355X (reference bulge; the edge's ideal vertices beyond the slab-corner box; the oracle's f32 vertices beyond
    the box the cull recorded with its former +-2 px margin; the same with the margin that follows from bulge and vertex noise):
    60N 2x 1.04 m, 6.1 px, 6.9 px, inside by 45 px; 70N 3x 1.72 m, 5.8 px, 5.0 px, inside by 34 px; 80N 5x 2.47 m, 9.8 px, 8.2 px,
    inside by 39 px; 80N square 0.10 m, 4.5 px, 28.0 px (vertex noise, not bulge), inside by 364 px; 81S 5x 2.47 m, 9.4 px, 8.4 px,
    inside by 40 px.  With +-2 px the chosen block was a candidate in all five and failed the box test in all five; at 80N 5x and
    81S 5x pixels it wins in the oracle's frame lay outside its box."""
    c = CC.bulge_case(name)
    cond = c.condition()
    print(f"{name}: reference bulge {cond['bulge_m']:.2f} m, the edge's vertices {cond['overshoot_px']:.2f} px beyond the slab-corner box {cond['box']}")
    g, tables = _renderer(topo, c.tiles)
    r = _check_lists(topo, orc, ("bulge", name), c.tiles, c.uniforms, c.split, g, tables, f"bulge {name}", must_list=(0, c.blk))
    print(f"{name}: the chosen block is {'a far candidate' if (0, c.blk) in r['far'] else 'near'}")
    g.close()


@pytest.mark.parametrize("name,tw,th", CC.TABLE_CASES)
def test_cull_lists_table_cases(topo, orc, name, tw, th):
    """One oblique pose over every table case.  The full blocks of one-degree tiles of 24 to 480 columns have sagittas far above
    1 m and are never candidates (the one-cell sliver blocks of the 62 x 17 tiles, 0.9 m, are): what is at stake is the near list's
    partition into strips (sliver rows of 1, 8 and 15 cell rows), the frustum cull and the far box of sliver blocks, and the frame
    with the filter on and off."""
    tiles = CC.table_case(name, tw, th)
    g, tables = _renderer(topo, tiles)
    r = _check_lists(topo, orc, ("table", name, tw, th), tiles, CC.table_pose(tiles), 15000.0, g, tables, f"{name} {tw}x{th}")
    assert len(r["near"]) >= 4 and ((tw, th) != (62, 17) or len(r["far"]) >= 1)
    g.close()


def test_cull_lists_hook_refuses_what_it_cannot_answer(topo):
    sc = CC.list_scene("quadrant")
    g = topo.TerrainRenderer(CC.W, CC.H)
    sc.tiles.load(g)
    with pytest.raises(topo.TopoError) as err:
        g.debug_read_cull_lists()      # no submission yet
    assert err.value.code == topo.TOPO_ERR_INVALID
    g.update(CC.W, CC.H, sc.poses[0][1], topo.post_uniforms(CC.W, CC.H))
    g.render()
    assert len(g.debug_read_cull_lists()["near"]) > 0
    g.set_pipeline_depth(2)
    with pytest.raises(topo.TopoError) as err:
        g.debug_read_cull_lists()
    assert err.value.code == topo.TOPO_ERR_INVALID
    g.set_pipeline_depth(1)
    with pytest.raises(topo.TopoError) as err:
        g.debug_read_cull_lists()      # the submission from before the change of depth does not count
    assert err.value.code == topo.TOPO_ERR_INVALID
    g.render()
    assert len(g.debug_read_cull_lists()["near"]) > 0
    g.close()
