"""The skyline rule on the CPU (topo_skyline.h under g++, tests/skyline_emul.py): the traversal against the loop over every triangle,
bit for bit; both against the independent numpy reference (tests/skyline_ref.py) outside the azimuths it marks ambiguous; the winner
against the ray reference (tests/los_ref.py) -- a ray just above the skyline misses, one just below hits -- and what the rule promises
of observers and range limits, on the cases of tests/skyline_cases.py."""
import numpy as np
import pytest

import los_ref as LR
import skyline_cases as SC
import skyline_emul as SE
import skyline_ref as SR
import visibility_cases as VC

ALL = sorted(SC.CASES)
RAY_EPS = 1e-6      # radians above and below the winner's elevation


@pytest.mark.parametrize("name", ALL)
def test_traversal_equals_every_triangle(name):
    """Bit for bit on every azimuth, the ambiguous ones included: the pruning drops nothing that could win or tie."""
    fast, brute = SC.emulation(name), SC.emulation(name, brute=True)
    assert fast.tobytes() == brute.tobytes(), f"{name}: {int((fast != brute).sum())} azimuths differ between the traversal and the every-triangle loop"


@pytest.mark.parametrize("name", ALL)
def test_reference_stays_under_the_ambiguity_cap(name):
    ref, _ = SC.reference(name)
    share = float(ref["ambiguous"].mean())
    print(f"{name}: {int(ref['ambiguous'].sum())} of {ref.size} azimuths ambiguous")
    assert share <= SC.MAX_AMBIGUOUS


@pytest.mark.parametrize("name", ALL)
def test_emulation_equals_reference(name):
    SC.against_reference(SC.emulation(name), name, name)


@pytest.mark.parametrize("name", ALL)
def test_kinds_and_fields(name):
    c = SC.case(name)
    emu = SC.emulation(name)
    ref, _ = SC.reference(name)
    for o in range(len(emu)):
        if o in c["unusable"]:
            assert (emu[o]["kind"] == SR.NO_OBSERVER).all() and (ref[o]["kind"] == SR.NO_OBSERVER).all()
        else:
            assert not (emu[o]["kind"] == SR.NO_OBSERVER).any()
    t = emu["kind"] == SR.TERRAIN
    assert t.sum() >= 80, "the case has a skyline"
    assert np.isnan(emu["elevation_deg"][~t]).all() and not emu["range_m"][~t].any() and not emu["cell_x"][~t].any(), "no terrain: NaN elevation, every other field 0"
    e = emu[t]
    assert (e["s"] >= c["min_range"]).all() and (e["s"] <= c["max_range"]).all()
    assert np.abs(np.degrees(np.arctan2(e["z"], e["s"])) - e["elevation_deg"]).max() < 1e-12
    assert np.abs(np.hypot(e["s"], e["z"]) - e["range_m"]).max() < 1e-6, "the crossing point lies in the half-plane: |X| = |(s, z)|"
    assert (e["edge"] < 3).all() and (e["tri"] < 2).all()


@pytest.mark.parametrize("name", SC.RAY_CHECKED)
def test_a_ray_above_the_skyline_misses_and_one_below_hits(name):
    """An independent cross-check through the ray reference: from O at the winner's elevation + 1e-6 rad, restricted to the same s
    interval, a ray meets no terrain on any unambiguous azimuth; at - 1e-6 rad it meets some wherever the winning edge is shared by
    two existing triangles (under an edge of the mesh's border a ray may pass).  The reference's own winners are put through the
    same check first: it is the yardstick."""
    c = SC.case(name)
    ref, O = SC.reference(name)
    mesh = VC.meshes(c["tileset"]).rays
    az = SR.azimuths(c["az0"], c["daz"], c["n_az"])
    emu = SC.emulation(name)
    for what, ratio_of in (("reference", lambda o: ref[o]["ratio"]), ("emulation", lambda o: emu[o]["ratio"])):
        n_above = n_below = 0
        for o in range(len(ref)):
            keep = (ref[o]["kind"] == SR.TERRAIN) & ~ref[o]["ambiguous"]
            if not keep.any():
                continue
            el = np.arctan(ratio_of(o)[keep])
            for sign, must_hit in ((+1.0, False), (-1.0, True)):
                sel = np.ones(int(keep.sum()), bool) if not must_hit else ref[o]["shared"][keep]
                e = el[sel] + sign * RAY_EPS
                rays = np.zeros(len(e), VC.LC.RAY_DTYPE)
                rays["origin"], rays["dir"] = O[o], SR.direction(O[o], az[keep][sel], e)
                rays["t_min"], rays["t_max"] = c["min_range"] / np.cos(e), c["max_range"] / np.cos(e)      # the same s interval
                res = LR.cast(mesh, rays)
                wrong = np.nonzero((res["kind"] == LR.HIT) != must_hit)[0]
                assert len(wrong) == 0, f"{name} {what} observer {o}: {len(wrong)} rays {'miss below' if must_hit else 'hit above'} the skyline, first azimuth " \
                                        f"{np.nonzero(keep)[0][np.nonzero(sel)[0][wrong[0]]]}"
                n_above, n_below = n_above + (0 if must_hit else len(e)), n_below + (len(e) if must_hit else 0)
        print(f"{name} {what}: {n_above} rays above the skyline miss, {n_below} below hit")
        assert n_above >= 200 and n_below >= 100


def test_range_limits_move_the_skyline():
    """min_range skips the nearest ridges and max_range cuts the far ones: the winners differ from those of the whole range where it
    lay outside, are the same where it lay inside, and never stand higher."""
    full = SC.emulation("ridges_ne")[:2]
    for name, inside in (("ridges_ne_min", lambda s: s >= 60.0e3), ("ridges_ne_max", lambda s: s <= 40.0e3)):
        cut = SC.emulation(name)
        was_in = (full["kind"] == SR.TERRAIN) & inside(full["s"])
        assert was_in.sum() >= 20 and (~was_in).sum() >= 20, (name, int(was_in.sum()))
        assert cut[was_in].tobytes() == full[was_in].tobytes(), f"{name}: a winner inside the limits stays"
        moved = ~was_in & (cut["kind"] == SR.TERRAIN)
        assert moved.sum() >= 20 and (cut["ratio"][moved] < full["ratio"][moved]).all(), f"{name}: what replaces a winner outside the limits stands lower"
        assert inside(cut["s"][cut["kind"] == SR.TERRAIN]).all()


def test_observer_in_the_gap_and_outside():
    """ridges_ne: the observer in the gap between the tile rows (over the sphere, on a valley floor) has terrain all around; the one
    outside the mosaic sees it on the azimuths that look in and nothing on the others."""
    emu = SC.emulation("ridges_ne")
    az = SR.azimuths(SC.AZ0, SC.DAZ, SC.N_AZ)
    gap = emu[4]["kind"] == SR.TERRAIN
    # (the two azimuths within a degree of east and west look along the gap itself: no terrain)
    assert gap.sum() >= 88 and (np.abs(az[~gap] % 180.0 - 90.0) < 1.0).all() and (emu[4]["elevation_deg"][gap] > 0).all()
    out = emu[2]["kind"] == SR.TERRAIN
    assert 20 <= out.sum() <= 60 and (az[out] < 180.0).all(), "west of the mosaic: it lies to the east"


def test_more_than_64_blocks_are_walked():
    """The winners of the `grid` tile (85 raster blocks) lie in blocks of both batches of 64."""
    emu = SC.emulation("grid")
    w = SC.case("grid")["tiles"][0][0].shape[1]
    blk = VC.LC.block_of(emu["cell_x"], emu["cell_y"], w)[emu["kind"] == SR.TERRAIN]
    assert (blk < 64).sum() >= 10 and (blk >= 64).sum() >= 10, np.bincount(blk // 64)


def test_header_constants_match_the_rule(topo):
    assert (topo.SKY_NONE, topo.SKY_TERRAIN, topo.SKY_NO_OBSERVER) == (SR.NONE, SR.TERRAIN, SR.NO_OBSERVER) and topo.SKY_NO_OBSERVER == topo.VIS_NO_OBSERVER
    assert topo.SKYLINE_DTYPE.itemsize == 64
    assert [n for n in topo.SKYLINE_DTYPE.names if n in SE.OUT_DTYPE.names] == list(topo.SKYLINE_DTYPE.names), "the emulation's record has every field of the product's"
    hdr = open(topo.HEADER_PATH).read()
    for k, v in (("TOPO_SKY_NONE", 0), ("TOPO_SKY_TERRAIN", 1), ("TOPO_SKY_NO_OBSERVER", 4)):
        assert f"#define {k} {v}" in hdr
