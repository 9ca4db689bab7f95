"""The visibility rule on the CPU (topo_visibility.h under g++, tests/visibility_emul.py): the lookup and the traversal against the
loop over every triangle, bit for bit; both against the independent numpy reference (tests/visibility_ref.py) outside the targets it
marks ambiguous; and what the rule promises -- balanced classes, unusable observers, an observer at its target, monotony in the
target height -- on the cases of tests/visibility_cases.py."""
import numpy as np
import pytest

import visibility_cases as VC
import visibility_emul as VE
import visibility_ref as VR

ALL = sorted(VC.CASES) + sorted(VC.NO_REFERENCE)

# what the cases were chosen for, from a prototype of the reference: (none, visible, away, hidden) of observer 0, and its ambiguous targets
EXPECTED = {"ridges_ne": ((148, 181, 590, 521), 0), "blocks": ((252, 406, 412, 370), 0), "long": ((174, 448, 322, 256), 3), "summit_h0": ((148, 57, 606, 629), 0),
            "summit_h30": ((148, 66, 0, 1226), 0)}


@pytest.mark.parametrize("name", ALL)
def test_traversal_equals_every_triangle(name):
    fast, eyes = VC.emulation(name)
    brute, eyes_b = VC.emulation(name, brute=True)
    assert fast.tobytes() == brute.tobytes(), f"{name}: {int((fast != brute).sum())} targets differ between the traversal and the every-triangle loop"
    assert eyes.tobytes() == eyes_b.tobytes()


@pytest.mark.parametrize("name", sorted(VC.CASES))
def test_emulation_equals_reference(name):
    ref, amb = VC.reference(name)
    emu, _ = VC.emulation(name)
    assert ref.shape == emu.shape
    share = float(amb.mean())
    assert share <= VC.MAX_AMBIGUOUS, f"{name}: {share:.4%} of the targets are ambiguous"
    for o in range(len(ref)):
        print(f"{name} observer {o}: {VC.counts(ref[o])}, ambiguous {int(amb[o].sum())} of {amb[o].size}, differences on ambiguous targets {int((ref[o] != emu[o]).sum())}")
        bad = np.nonzero((ref[o] != emu[o]) & ~amb[o])[0]
        assert len(bad) == 0, f"{name} observer {o}: {len(bad)} unambiguous targets differ, first {bad[0]}: reference {ref[o][bad[0]]}, emulation {emu[o][bad[0]]}"


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_counts_are_those_the_cases_were_chosen_for(name):
    ref, amb = VC.reference(name)
    want, n_amb = EXPECTED[name]
    clear = ~amb[0]
    got = VC.counts(ref[0])
    print(f"{name}: {got}, ambiguous {int(amb[0].sum())}")
    assert int(amb[0].sum()) <= max(n_amb, 3)
    assert all(abs(g - w) <= int(amb[0].sum()) for g, w in zip(got[:4], want)) and got[4] == 0, (got, want)
    assert clear.sum() >= 0.995 * clear.size


@pytest.mark.parametrize("name", VC.BALANCED)
def test_balanced_cases_have_every_class(name):
    """Each of VISIBLE, AWAY and HIDDEN is at least 5 % of the terrain targets: a constant answer cannot pass."""
    for cls in (VC.reference(name)[0][0], VC.emulation(name)[0][0]):
        terrain = int((cls != VR.NONE).sum())
        assert terrain > 0.8 * cls.size
        for k in (VR.VISIBLE, VR.AWAY, VR.HIDDEN):
            assert (cls == k).sum() >= 0.05 * terrain, (name, k, VC.counts(cls))


@pytest.mark.parametrize("name", VC.RIDGE_SCENES)
def test_raising_the_target_never_hides_a_visible_one(name):
    """A property of the rule on the ridge scenes, on unambiguous targets: the segment to the observer from h2 > h1 above a point lies
    above the one from h1 wherever both are over the same ground, so a target VISIBLE at h1 is not HIDDEN at h2."""
    heights = (0.0, 30.0, 120.0)
    runs = [(VC.reference(name, h), VC.emulation(name, h=h)[0]) for h in heights]
    for (ha, ((ra, aa), ea)), (hb, ((rb, ab), eb)) in zip(zip(heights, runs), zip(heights[1:], runs[1:])):
        clear = ~aa[0] & ~ab[0]
        for what, a, b in (("reference", ra[0], rb[0]), ("emulation", ea[0], eb[0])):
            bad = np.nonzero(clear & (a == VR.VISIBLE) & (b == VR.HIDDEN))[0]
            assert len(bad) == 0, f"{name} {what}: target {bad[0]} is visible at {ha} m and hidden at {hb} m"
            assert not ((a == VR.NONE) != (b == VR.NONE)).any(), "the target height does not move the terrain"
        if ha > 0.0:
            assert not (ea[0] == VR.AWAY).any(), "AWAY is a class of targets on the ground only"
    assert (runs[0][1][0] == VR.AWAY).sum() > 100 and (runs[-1][1][0] == VR.VISIBLE).sum() > (runs[0][1][0] == VR.VISIBLE).sum()


def test_summit_sees_more_of_masts_than_of_ground():
    g0, g30 = VC.emulation("summit_h0")[0][0], VC.emulation("summit_h30")[0][0]
    c = VC.case("summit_h0")
    assert g0[c["summit"]] == VR.VISIBLE and g30[c["summit"]] == VR.VISIBLE, "the target under the observer"
    assert (g30 == VR.VISIBLE).sum() > (g0 == VR.VISIBLE).sum() and (g0 == VR.AWAY).sum() > 400 and not (g30 == VR.AWAY).any()
    # a mast on a back slope is hidden by its own slope: most of what faced away at h = 0 is hidden at h = 30, nothing is skipped
    assert ((g0 == VR.AWAY) & (g30 == VR.HIDDEN)).sum() > 0.9 * (g0 == VR.AWAY).sum()


def test_voids_are_none_and_are_looked_through():
    c = VC.case("void_nan")
    emu, _ = VC.emulation("void_nan")
    ref, _ = VC.reference("void_nan")
    high, low = emu[0], emu[1]
    assert VC.counts(high) == (396, 1044, 0, 0, 0), "from 4000 m over the sphere: every terrain target is visible, every void NONE"
    assert np.array_equal(high == VR.NONE, low == VR.NONE)
    assert (low == VR.HIDDEN).sum() > 0 and (low == VR.VISIBLE).sum() > 100 and (low == VR.AWAY).sum() > 100
    # the same relief without its voids: no target that keeps its terrain changes class because a void opened elsewhere, except
    # that a HIDDEN one may become VISIBLE -- the sight line passes through the hole
    import los_cases as LC
    import void_scenes as VS
    clean = LC.scene_tiles(VS.relief_case("ne_2x2", "nan")[0])
    full, _, bad = VE.visibility(clean[0], clean[1], c["obs"], c["lonlat"], 0.0)
    assert bad == 0
    kept = low != VR.NONE
    changed = kept & (full[1] != low)
    assert ((full[1][changed] == VR.HIDDEN) & (low[changed] == VR.VISIBLE)).all()
    print(f"void_nan: {int(changed.sum())} targets are seen through a void")


def test_observers_of_every_kind():
    c = VC.case("observers")
    emu, eyes = VC.emulation("observers")
    ref, amb = VC.reference("observers")
    for o in c["unusable"]:
        assert eyes["usable"][o] == 0 and (emu[o] == VR.NO_OBSERVER).all() and (ref[o] == VR.NO_OBSERVER).all(), o
    usable = [o for o in range(len(emu)) if o not in c["unusable"]]
    assert (eyes["usable"][usable] == 1).all()
    for o in usable:
        assert (emu[o][c["extra"]] == VR.NONE).all(), "invalid targets and targets without terrain are NONE"
        assert not (emu[o] == VR.NO_OBSERVER).any()
    # far away over the sphere: usable, and the whole mosaic faces away or lies below the horizon
    assert not (emu[6] == VR.VISIBLE).any()
    # over the sphere: O is (R0 + h) u
    u = VR.SR.direction(c["obs"]["lon_deg"][7], c["obs"]["lat_deg"][7])
    assert np.abs(eyes["p"][7] - (VR.R0 + 9000.0) * u).max() < 1e-6
    # an observer at a target sees it, whatever the ground does there; its neighbours are judged as ever
    assert emu[8][c["at"][0]] == VR.VISIBLE and emu[9][c["at"][1]] == VR.VISIBLE
    assert emu[0][c["at"][0]] != VR.NONE and emu[0][c["at"][1]] != VR.NONE
    # underground: the ground above faces away from it or hides the rest
    assert (emu[10] == VR.VISIBLE).sum() <= 2


def test_placements_have_terrain_and_classes():
    for name in ("antimeridian", "north84", "polar"):
        emu, _ = VC.emulation(name)
        low, high = emu[0], emu[1]
        assert (low != VR.NONE).mean() > 0.7 and np.array_equal(low == VR.NONE, high == VR.NONE)
        assert (low == VR.AWAY).sum() > 50 and (low == VR.HIDDEN).sum() >= 1 and (high == VR.VISIBLE).sum() > (low == VR.VISIBLE).sum(), (name, VC.counts(low))
    # rows beyond the pole are invalid points
    c = VC.case("polar")
    assert (emu[0][c["lonlat"][:, 1] > 90.0] == VR.NONE).all() and (c["lonlat"][:, 1] > 90.0).sum() >= 24


def test_header_constants_match_the_rule(topo):
    assert (topo.VIS_NONE, topo.VIS_VISIBLE, topo.VIS_AWAY, topo.VIS_HIDDEN, topo.VIS_NO_OBSERVER) == (VR.NONE, VR.VISIBLE, VR.AWAY, VR.HIDDEN, VR.NO_OBSERVER)
    assert (topo.VIS_NONE, topo.VIS_VISIBLE, topo.VIS_AWAY, topo.VIS_HIDDEN) == (topo.SUN_NONE, topo.SUN_LIT, topo.SUN_AWAY, topo.SUN_SHADOW)
    assert topo.OBSERVER_DTYPE == VE.OBSERVER_DTYPE and topo.OBSERVER_ABOVE_TERRAIN == VR.ABOVE_TERRAIN
    ob = topo.observers([7.5, 8.0], 46.5, [2.0, 3.0], [True, False])
    assert ob.tobytes() == VC.observer_records([7.5, 8.0], 46.5, [2.0, 3.0], [True, False]).tobytes()
    hdr = open(topo.HEADER_PATH).read()
    for k, v in (("TOPO_VIS_NONE", 0), ("TOPO_VIS_VISIBLE", 1), ("TOPO_VIS_AWAY", 2), ("TOPO_VIS_HIDDEN", 3), ("TOPO_VIS_NO_OBSERVER", 4)):
        assert f"#define {k} {v}" in hdr


def test_ecef_from_lonlat(topo):
    """The host helper: (R0 + h) surface_direction, f64 -- the observer point of the emulation for an observer over the sphere."""
    rng = np.random.default_rng(5)
    lon, lat, h = rng.uniform(-180, 180, 50), rng.uniform(-90, 90, 50), rng.uniform(-400, 9000, 50)
    obs = VC.observer_records(lon, lat, h, False)
    tiles, order, _ = VC.tileset("blocks")
    _, eyes, _ = VE.visibility(tiles, order, obs, np.zeros((0, 2)), 0.0)
    got = np.stack([topo.ecef_from_lonlat(a, b, c) for a, b, c in zip(lon, lat, h)])
    assert got.tobytes() == eyes["p"].tobytes()
    assert np.abs(np.linalg.norm(got, axis=1) - (VR.R0 + h)).max() < 1e-8
    assert np.array_equal(topo.ecef_from_lonlat(0.0, 0.0, 0.0), [VR.R0, 0.0, 0.0])
