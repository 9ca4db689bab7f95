"""The surface rule and lookup on the CPU (no GPU): the g++ build of topo_surface.h (tests/surface_emul.py) against its own brute
force over every triangle -- the candidate-set claim -- and against the numpy reference (tests/surface_ref.py) on the cases of
tests/surface_cases.py; exact DEM posts; and a profile's summary against a numpy reduction of its samples."""
import numpy as np
import pytest

import los_cases as LC
import surface_cases as SC
import surface_emul as SE
import surface_ref as SR


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_lookup_equals_every_triangle_bit_for_bit(name):
    tiles, order, pts, _ = SC.case(name)
    got, bad = SC.emulation(name)
    brute, bad_b = SE.surface(tiles, order, pts, brute=True)
    assert bad == 0 and bad_b == 0
    assert (got["kind"] == SR.TERRAIN).sum() > 0.3 * len(pts)
    diff = np.nonzero(got.view(np.uint8).reshape(len(got), -1) != brute.view(np.uint8).reshape(len(got), -1))[0]
    assert len(diff) == 0, f"{name}: the lookup differs from the loop over every triangle at point {diff[0]} {pts[diff[0]]}: {got[diff[0]]} vs {brute[diff[0]]}"


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_emulation_against_reference(name):
    tiles, order, pts, label = SC.case(name)
    got, _ = SC.emulation(name)
    ref = SC.reference(name)
    SC.compare_reference(ref, got, order, tiles[0][0].shape[0], label, name, f32_record=False)
    gap = label == SC.GAP
    assert (got["kind"][gap] == SR.NONE).all() and (ref["kind"][gap] == SR.NONE).all()
    z = got[got["kind"] != SR.TERRAIN]
    assert not z["height_m"].any() and not z["slope_deg"].any() and not z["cell_x"].any() and not z["w1"].any(), "every other field of a non-terrain record is 0"
    t = got[got["kind"] == SR.TERRAIN]
    assert (t["aspect_deg"] >= 0.0).all() and (t["aspect_deg"] < 360.0).all() and (t["slope_deg"] >= 0.0).all() and (t["slope_deg"] <= 90.0).all()


def test_overlap_rules():
    """In the overlap of two tiles the higher surface wins; where both are the same surface, the tile that is drawn first."""
    for name in ("overlap_higher", "overlap_equal"):
        tiles, order, pts, _ = SC.case(name)
        got, _ = SC.emulation(name)
        s = 1.0 / 32.0
        inside = (pts[:, 0] > 15.5 + 0.1 * s) & (pts[:, 0] < 15.0 + 22.9 * s) & (pts[:, 1] < 46.0 - 0.1 * s) & (pts[:, 1] > 46.0 - 22.9 * s)
        assert inside.sum() > 100 and (got["kind"][inside] == SR.TERRAIN).all()
        alone = [SE.surface([t], [o], pts[inside])[0] for t, o in zip(tiles, order)]
        assert all((a["kind"] == SR.TERRAIN).all() for a in alone)
        first = got["tile_lon_deg"][inside] == 15
        if name == "overlap_equal":
            assert np.array_equal(alone[0]["height_m"], alone[1]["height_m"]), "the shifted vertices coincide bit for bit"
            assert first.all(), "on equal heights the lower rank wins"
        else:
            assert 0.2 < first.mean() < 0.8
            assert np.array_equal(first, alone[0]["height_m"] >= alone[1]["height_m"])
            assert np.array_equal(got["height_m"][inside], np.maximum(alone[0]["height_m"], alone[1]["height_m"]))


def test_sentinels():
    """A vertex below -R0 removes the triangles around it (all eight of its four cells: the vertex is an even one, every diagonal
    around it ends in it); -32768 is geometry."""
    tiles, order, pts, _ = SC.case("sentinels")
    got, _ = SC.emulation("sentinels")
    hole, pit = SC.vertex_lonlat(tiles[0], 7, 5), SC.vertex_lonlat(tiles[0], 12, 15)
    d_hole, d_pit = np.abs(pts - hole).max(axis=1) * 24.0, np.abs(pts - pit).max(axis=1) * 24.0
    near_hole = d_hole < 0.45
    assert near_hole.sum() >= 25 and (got["kind"][near_hole] == SR.NONE).all()
    near_pit = d_pit < 0.16      # (the pit's weight is at least 0.7 there)
    assert near_pit.sum() >= 9 and (got["kind"][near_pit] == SR.TERRAIN).all() and (got["height_m"][near_pit] < -20000.0).all()


def test_every_exact_vertex_of_blocks_is_terrain():
    tiles, order = [SC.blocks_tile()], [(46, 7)]
    pts, hts = SC.blocks_vertices()
    got, bad = SE.surface(tiles, order, pts)
    assert bad == 0 and len(pts) == 130 * 34
    assert (got["kind"] == SR.TERRAIN).all(), f"{int((got['kind'] != SR.TERRAIN).sum())} exact vertices have no terrain, first {pts[np.nonzero(got['kind'] != SR.TERRAIN)[0][0]]}"
    err = np.abs(got["height_m"] - hts.astype(np.float64))
    print(f"exact vertices: largest |height - f32 height| {err.max():.3e} m")
    assert err.max() <= 1e-6


@pytest.mark.parametrize("m", [2, 100, 257])
def test_profile_summary_is_the_reduction_of_its_samples(m):
    tiles, order, _, _ = SC.case("long")
    segs, invalid = SC.profile_segments()
    summary, samples, bad = SE.profile(tiles, order, segs, m)
    assert bad == 0
    SC.check_summaries(summary, samples, invalid, f"m = {m}")
    n = len(segs)
    assert summary["n_terrain"][n - 4] == 0, "the segment west of the mosaic meets no terrain"
    assert summary["min_sample"][n - 5] == 0 and summary["n_terrain"][n - 5] == m, "every sample of the zero-length segment ties: the first wins"
    if m >= 100:
        assert 0 < summary["n_terrain"][6] < m, "samples beyond the mosaic are counted out"
        assert summary["min_clearance_m"][7] < -100.0, "the steep segment ends under the ground"
        # the samples against the reference: terrain and line within 1e-3 m (f32 at these heights: 2.4e-4 m steps)
        valid = np.ones(n, bool)
        valid[invalid] = False
        terrain, line, amb = SR.profile(SR.Mesh(tiles), segs[valid], m)
        got = samples[valid].astype(np.float64)
        same = np.isnan(terrain) == np.isnan(got[..., 0])
        assert (same | amb).all()
        both = ~np.isnan(terrain) & ~np.isnan(got[..., 0])
        assert np.abs(got[..., 0] - terrain)[both].max() <= 1e-3 and np.abs(got[..., 1] - line).max() <= 1e-3


@pytest.mark.parametrize("scale", [(0.0, 1.0 / 24.0), (1.0 / 24.0, 0.0), (np.inf, 1.0 / 24.0), (1.0 / 24.0, np.nan)])
def test_a_tile_without_a_finite_pixel_scale_has_no_surface(scale):
    """Beside a sound tile, a tile whose pixel scale is zero or not finite: the answers are those of the sound tile alone -- also on
    the meridian and the parallel the degenerate tile collapses onto -- from the lookup (which must not walk the whole tile), from the
    loop over every triangle and from the reference."""
    tiles, order = LC.placed_tiles([(45, 15), (45, 16)], 24)
    bad_tile = (tiles[1][0], tiles[1][1], tiles[1][2], np.float32(scale))
    pts = np.concatenate([SC.random_points(15.0, 17.0, 45.0, 46.0, 300, 71), np.stack([np.full(20, 16.0), np.linspace(45.05, 45.95, 20)], axis=-1),
                          np.stack([np.linspace(16.05, 16.95, 20), np.full(20, 46.0)], axis=-1)])
    alone, _ = SE.surface(tiles[:1], order[:1], pts)
    got, bad = SE.surface([tiles[0], bad_tile], order, pts)
    brute, bad_b = SE.surface([tiles[0], bad_tile], order, pts, brute=True)
    assert bad == 0 and bad_b == 0 and (alone["kind"] == SR.TERRAIN).sum() > 100
    assert got.tobytes() == alone.tobytes() and brute.tobytes() == alone.tobytes()
    ref = SR.surface(SR.Mesh([tiles[0], bad_tile]), pts)
    SC.compare_reference(ref, got, order, 24, np.full(len(pts), SC.RANDOM), f"pixel scale {scale}", f32_record=False)
