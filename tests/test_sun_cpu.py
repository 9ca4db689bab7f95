"""The sun exposure rule on the CPU (topo_sun.h under g++, tests/sun_emul.py): the lookup and the traversal against the loop over
every triangle, bit for bit; both against the independent numpy reference (tests/sun_ref.py) outside the pairs it marks ambiguous;
and what the rule promises -- every class under low suns, night under set ones, a sun's bit independent of its company and its
position, voids that are NONE and are shone through -- on the cases of tests/sun_cases.py."""
import numpy as np
import pytest

import sun_cases as SC
import sun_emul as SE
import sun_ref as SNR

ALL = sorted(SC.GRIDS)


@pytest.mark.parametrize("name", ALL)
def test_traversal_equals_every_triangle(name):
    fast, brute = SC.emulation(name), SC.emulation(name, brute=True)
    for what, a, b in zip(("classes", "lit", "shadow", "exposure"), fast, brute):
        assert a.tobytes() == b.tobytes(), f"{name}: {what} differ between the traversal and the every-triangle loop at {int((a != b).sum())} places"


@pytest.mark.parametrize("name", ALL)
def test_emulation_equals_reference(name):
    ref, r_lit, r_shadow, r_exp, amb = SC.reference(name)
    emu, e_lit, e_shadow, e_exp = SC.emulation(name)
    assert ref.shape == emu.shape == (13, len(SC.case(name)["lonlat"]))
    share = float(amb.mean())
    print(f"{name}: ambiguous share {share:.4%}")
    for k in range(len(ref)):
        print(f"{name} sun {k} {SC.ARC[k]}: {SC.counts(ref[k])}, ambiguous {int(amb[k].sum())}, differences on ambiguous pairs {int((ref[k] != emu[k]).sum())}")
    assert share <= SC.MAX_AMBIGUOUS, f"{name}: {share:.4%} of the pairs are ambiguous"
    bad = np.argwhere((ref != emu) & ~amb)
    assert len(bad) == 0, f"{name}: {len(bad)} unambiguous pairs differ, first (sun, target) {tuple(bad[0])}: reference {ref[tuple(bad[0])]}, emulation {emu[tuple(bad[0])]}"
    # the masks are the classes, bit by bit
    for cls, lit, shadow in ((ref, r_lit, r_shadow), (emu, e_lit, e_shadow)):
        want_lit, want_shadow = SNR.masks(cls)
        assert np.array_equal(lit, want_lit) and np.array_equal(shadow, want_shadow)
        assert not (lit & shadow).any()
    # exposure: non-negative f64 terms, each good to a few f64 ulps, summed in f64 and rounded once: within 1 f32 ulp of the reference
    clear = ~amb.any(axis=0)
    none = ref[0] == SNR.NONE
    assert np.array_equal(np.isnan(e_exp), emu[0] == SNR.NONE) and np.array_equal(np.isnan(r_exp), none)
    at = clear & ~none
    ulps = SC.ulp_distance_f32(e_exp[at], r_exp[at])
    print(f"{name}: exposure on {int(at.sum())} clear terrain targets: max {int(ulps.max())} f32 ulps apart, {int((ulps > 0).sum())} differ")
    assert ulps.max() <= 1
    assert (e_exp[at] >= 0).all() and (e_exp[at & ~(e_lit != 0)] == 0).all(), "terrain that is never lit has exposure 0"
    assert (e_exp[at & (e_lit != 0)] > 0).all()


@pytest.mark.parametrize("name", SC.BALANCED)
def test_low_suns_show_every_class_and_set_suns_are_night(name):
    for cls in (SC.reference(name)[0], SC.emulation(name)[0]):
        terrain = cls[0] != SNR.NONE
        assert terrain.mean() > 0.8
        for k in SC.EL4:
            got = SC.counts(cls[k])
            print(f"{name} sun {k} {SC.ARC[k]}: {got}")
            assert min(got[SNR.LIT], got[SNR.AWAY], got[SNR.SHADOW]) >= 1, (name, k, got)
        for k in SC.NIGHT_SUNS:
            assert (cls[k][terrain] == SNR.NIGHT).all() and (cls[k][~terrain] == SNR.NONE).all(), (name, k, SC.counts(cls[k]))


def test_long_mosaic_has_night_at_one_end_while_the_rest_is_in_daylight():
    """The sun is one direction for the call: at elevation 1 degree over the centre of a mosaic three degrees long it is below the
    horizontal plane of the targets at the far end."""
    cls = SC.emulation("long")[0]
    for k in SC.EL1:
        got = SC.counts(cls[k])
        print(f"long sun {k} {SC.ARC[k]}: {got}")
        assert got[SNR.NIGHT] >= 20 and got[SNR.NIGHT] < 0.2 * cls.shape[1] and got[SNR.LIT] > 0


def test_permuting_the_suns_permutes_the_bits_and_nothing_else():
    c = SC.case("ridges_ne")
    cls, lit, shadow, exposure = SC.emulation("ridges_ne")
    perm = np.random.default_rng(11).permutation(len(c["suns"]))
    p_cls, p_lit, p_shadow, p_exp, bad = SE.sun_exposure(c["tiles"], c["order"], c["suns"][perm], c["lonlat"])
    assert bad == 0
    assert np.array_equal(p_cls, cls[perm])
    want_lit, want_shadow = SNR.masks(cls[perm])
    assert np.array_equal(p_lit, want_lit) and np.array_equal(p_shadow, want_shadow)
    # the sum is formed in another order: the exposures agree within the f64 sum's rounding, seen through one f32 rounding
    at = ~np.isnan(exposure)
    assert np.array_equal(np.isnan(p_exp), ~at) and SC.ulp_distance_f32(p_exp[at], exposure[at]).max() <= 1


def test_one_sun_alone_gives_the_bit_it_gives_in_company():
    c = SC.case("blocks")
    cls, lit, shadow, exposure = SC.emulation("blocks")
    for k in (1, 2, 6, 12):
        a_cls, a_lit, a_shadow, a_exp, bad = SE.sun_exposure(c["tiles"], c["order"], c["suns"][k:k + 1], c["lonlat"])
        assert bad == 0
        assert np.array_equal(a_cls[0], cls[k])
        assert np.array_equal(a_lit, (lit >> np.uint64(k)) & np.uint64(1)) and np.array_equal(a_shadow, (shadow >> np.uint64(k)) & np.uint64(1))


def test_voids_are_none_and_are_shone_through():
    """The relief of void_nan is gentle: besides the standard suns, one at azimuth 80, elevation 1.5 degrees, whose shadows reach
    across a void."""
    import los_cases as LC
    import void_scenes as VS
    import visibility_cases as VC
    base = SC.case("void_nan")
    c = dict(base, suns=SC.arc_suns(VC.tileset("void_nan")[2], SC.ARC + ((80, 1.5),)))
    cls, lit, shadow, exposure = SC.emulate(c)
    assert np.array_equal(cls[:13], SC.emulation("void_nan")[0]), "a fourteenth sun changes nothing for the thirteen"
    none = cls[0] == SNR.NONE
    assert none.sum() == 396 and (cls[:, none] == SNR.NONE).all() and np.isnan(exposure[none]).all() and not lit[none].any() and not shadow[none].any()
    assert not (cls[:, ~none] == SNR.NONE).any() and (shadow[~none] != 0).sum() > 0
    # the same relief without its voids: no pair that keeps its terrain changes class because a void opened elsewhere, except that a
    # SHADOW may become LIT -- the sun shines through the hole
    clean = LC.scene_tiles(VS.relief_case("ne_2x2", "nan")[0])
    full = SE.sun_exposure(clean[0], clean[1], c["suns"], c["lonlat"])[0]
    changed = (full != cls) & ~none[None, :]
    assert changed.sum() > 0 and ((full[changed] == SNR.SHADOW) & (cls[changed] == SNR.LIT)).all()
    print(f"void_nan: {int(changed.sum())} pairs are lit through a void")


def test_placements_have_terrain_and_classes():
    for name in ("antimeridian", "north84", "polar"):
        cls = SC.emulation(name)[0]
        terrain = cls[0] != SNR.NONE
        assert terrain.mean() > 0.7
        noon = SC.counts(cls[6])
        assert noon[SNR.LIT] > 0.5 * terrain.sum() and noon[SNR.NIGHT] == 0, (name, noon)
        assert sum(SC.counts(cls[k])[SNR.AWAY] + SC.counts(cls[k])[SNR.SHADOW] for k in SC.EL1 + SC.EL4) > 0, name      # (gentle relief: the lowest suns)


def test_header_constants_match_the_rule(topo):
    k = SE.constants()
    assert (k["NONE"], k["LIT"], k["AWAY"], k["SHADOW"], k["NIGHT"]) == (SNR.NONE, SNR.LIT, SNR.AWAY, SNR.SHADOW, SNR.NIGHT)
    assert (topo.SUN_NONE, topo.SUN_LIT, topo.SUN_AWAY, topo.SUN_SHADOW, topo.SUN_NIGHT) == (SNR.NONE, SNR.LIT, SNR.AWAY, SNR.SHADOW, SNR.NIGHT)
    assert k["MAX_SUNS"] == SNR.MAX_SUNS == 64 and k["SUN_BYTES"] == 32
    assert topo.SUN_DTYPE == SE.SUN_DTYPE and topo.SUN_DTYPE.itemsize == 32
    d = np.array([[1.0, 2.0, 3.0], [0.0, -1.0, 0.5]])
    assert topo.suns(d, [15.0, 7.5]).tobytes() == SC.sun_records(d, [15.0, 7.5]).tobytes()
    assert topo.suns(d[0], 2.0).tobytes() == SC.sun_records(d[0], 2.0).tobytes()
    hdr = open(topo.HEADER_PATH).read()
    assert "#define TOPO_SUN_NIGHT 4" in hdr
    assert "typedef struct topo_sun { double dir[3]; double weight; } topo_sun;" in hdr
    for fn in ("topo_sun_exposure_grid_device", "topo_sun_exposure_device", "topo_sun_exposure_read"):
        assert hasattr(topo.lib(), fn)
