"""The refracted visibility rule on the CPU (topo_refraction.h under g++, tests/refraction_emul.py): the lookup and the traversal
against the loop over every triangle, bit for bit; k = 0 against the plain rule's bytes; both against an independent numpy reference
(tests/refraction_ref.py) outside the targets it marks ambiguous; against the composition that existed before -- the plain rule on
tiles whose heights were lifted on the host; and the two cases with a known answer (tests/refraction_cases.py)."""
import os
import subprocess

import numpy as np
import pytest

import refraction_cases as RCS
import refraction_emul as RE
import refraction_ref as RR
import visibility_cases as VC
import visibility_emul as VE
import visibility_ref as VR
from oracle import ray_check as RC

HERE = os.path.dirname(os.path.abspath(__file__))
PLAIN = sorted(VC.CASES) + sorted(VC.NO_REFERENCE)
# The cases on which the reference alone stays within the cap.  Not `flat`: its masts stand on a DEM row and their sight lines graze a
# faceted sphere, which the reference calls ambiguous for every twentieth of them; its answer is known in closed form instead
# (test_masts_over_a_smooth_sphere_end_at_the_horizon).  Not `gentle`: sight lines that graze 60 m relief over tens of kilometres are
# ambiguous for 1 to 2 % of the targets from any observer tried (30 m to 3000 m up, five places); it is compared with the reference
# outside those targets in test_gentle_relief_changes_class_under_refraction, without the cap.
REFERENCED = sorted(n for n in RCS.CASES if n not in ("flat", "gentle"))


@pytest.mark.parametrize("name", sorted(RCS.CASES))
def test_traversal_equals_every_triangle(name):
    fast, eyes = RCS.emulation(name)
    brute, eyes_b = RCS.emulation(name, brute=True)
    assert fast.tobytes() == brute.tobytes(), f"{name}: {int((fast != brute).sum())} targets differ between the traversal and the every-triangle loop"
    assert eyes.tobytes() == eyes_b.tobytes()


@pytest.mark.parametrize("name", PLAIN)
def test_k_zero_gives_the_plain_rule_bit_for_bit(name):
    c = VC.case(name)
    plain, eyes = VC.emulation(name)
    for brute in (False, True):
        got, eyes_r, bad = RE.visibility(c["tiles"], c["order"], c["obs"], c["lonlat"], c["h"], 0.0, brute)
        assert bad == 0
        assert got.tobytes() == plain.tobytes() and eyes_r.tobytes() == eyes.tobytes(), (name, brute, int((got != plain).sum()))


@pytest.mark.parametrize("name", PLAIN)
def test_traversal_equals_every_triangle_on_the_plain_cases(name):
    """The plain rule's cases (voids, the antimeridian, the pole, observers of every kind, exact posts) under k = 0.13."""
    c = VC.case(name)
    fast, _, bad = RE.visibility(c["tiles"], c["order"], c["obs"], c["lonlat"], c["h"], RCS.K)
    brute, _, bad_b = RE.visibility(c["tiles"], c["order"], c["obs"], c["lonlat"], c["h"], RCS.K, brute=True)
    assert bad == 0 and bad_b == 0
    assert fast.tobytes() == brute.tobytes(), f"{name}: {int((fast != brute).sum())} targets differ"


@pytest.mark.parametrize("name", REFERENCED)
def test_emulation_equals_reference(name):
    ref, amb = RCS.reference(name)
    share = float(amb.mean())
    assert share <= VC.MAX_AMBIGUOUS, f"{name}: the reference alone calls {share:.4%} of the targets ambiguous"
    emu, _ = RCS.emulation(name)
    assert ref.shape == emu.shape
    for o in range(len(ref)):
        print(f"{name} observer {o}: {VC.counts(ref[o])}, ambiguous {int(amb[o].sum())} of {amb[o].size}, differences on ambiguous targets {int((ref[o] != emu[o]).sum())}")
        bad = np.nonzero((ref[o] != emu[o]) & ~amb[o])[0]
        assert len(bad) == 0, f"{name} observer {o}: {len(bad)} unambiguous targets differ, first {bad[0]}: reference {ref[o][bad[0]]}, emulation {emu[o][bad[0]]}"


def _host_lifted(c, O, k):
    """The composition available before: the case's tiles with every f32 post lifted for the observer at O on the host (re-rounded
    to f32), and the observer restated over the sphere so that O stays where it was."""
    tiles = []
    for hts, rp, mp, ps in c["tiles"]:
        with np.errstate(all="ignore"):
            P = RC.tile_vertices(hts, rp, mp, ps)
        s2 = ((P - O[None, None, :]) ** 2).sum(axis=-1)
        tiles.append(((hts.astype(np.float64) + (k / (2.0 * VR.R0)) * s2).astype(np.float32), rp, mp, ps))
    rho = float(np.linalg.norm(O))
    lon, lat = np.degrees(np.arctan2(O[1], O[0])), np.degrees(np.arcsin(O[2] / rho))
    return tiles, VC.observer_records(lon, lat, rho - VR.R0, False)


@pytest.mark.parametrize("name", ["gentle", "ridges_ne", "blocks130"])
def test_plain_rule_on_host_lifted_tiles(name):
    """One observer at a time through code that existed before.  The lifted heights are re-rounded to f32 (up to half an ulp:
    0.25 mm at 4 km) and O moves by an ulp or so, hence differences are allowed on targets the reference calls ambiguous, only."""
    c = RCS.case(name)
    emu, eyes = RCS.emulation(name)
    _, amb = RCS.reference(name)
    for o in np.nonzero(eyes["usable"])[0]:
        tiles, ob = _host_lifted(c, eyes["p"][o], c["k"])
        got, eyes_l, bad = VE.visibility(tiles, c["order"], ob, c["lonlat"], c["h"])
        assert bad == 0 and eyes_l["usable"][0] == 1 and np.abs(eyes_l["p"][0] - eyes["p"][o]).max() < 1e-7
        differ = got[0] != emu[o]
        print(f"{name} observer {o}: {int(differ.sum())} of {differ.size} targets differ from the plain rule on host-lifted tiles, {int(amb[o].sum())} ambiguous")
        assert not (differ & ~amb[o]).any(), f"{name} observer {o}: {int((differ & ~amb[o]).sum())} unambiguous targets differ"


@pytest.mark.parametrize("k", [0.0, RCS.K])
def test_masts_over_a_smooth_sphere_end_at_the_horizon(k):
    """The flat case: the visible masts form one run from the observer, and the last visible and the first hidden one bracket
    sqrt(2 R0 H / (1 - k)) + sqrt(2 R0 h / (1 - k)), widened by one spacing each side."""
    c = RCS.case("flat")
    emu, _ = RCS.emulation("flat", k)
    dist, cls = RCS.visible_run(c, emu[0])
    assert len(cls) > 400 and set(np.unique(cls)) == {VR.VISIBLE, VR.HIDDEN}
    n_vis = int((cls == VR.VISIBLE).sum())
    assert (cls[:n_vis] == VR.VISIBLE).all() and (cls[n_vis:] == VR.HIDDEN).all(), "one run from the observer"
    spacing = float(np.diff(dist).min())
    want = float(RCS.horizon_range(c["H"], c["h"], k))
    print(f"k = {k}: last visible {dist[n_vis - 1] / 1e3:.2f} km, first hidden {dist[n_vis] / 1e3:.2f} km, horizon {want / 1e3:.2f} km, spacing {spacing:.0f} m")
    assert dist[n_vis - 1] - spacing <= want <= dist[n_vis] + spacing


def test_refraction_lengthens_the_run_of_masts():
    c = RCS.case("flat")
    runs = [int((RCS.visible_run(c, RCS.emulation("flat", k)[0][0])[1] == VR.VISIBLE).sum()) for k in (0.0, RCS.K)]
    print(f"visible masts: {runs[0]} at k = 0, {runs[1]} at k = {RCS.K}")
    assert runs[1] >= runs[0] + 5


def test_gentle_relief_changes_class_under_refraction():
    """At least 10 targets that neither reference calls ambiguous change class between k = 0 and k = 0.13."""
    straight, _ = RCS.emulation("gentle", 0.0)
    bent, _ = RCS.emulation("gentle")
    (r0, a0), (r1, a1) = RCS.reference("gentle", 0.0), RCS.reference("gentle")
    clear = ~a0 & ~a1
    for o in range(2):
        print(f"gentle observer {o}: {int((straight[o] != bent[o]).sum())} targets change class, {int(((straight[o] != bent[o]) & clear[o]).sum())} of them unambiguous")
    assert not ((straight != r0) & ~a0).any() and not ((bent != r1) & ~a1).any()
    assert ((straight != bent) & clear).sum() >= 10
    # the terrain is where it was; what refraction reveals was hidden or faced away
    assert np.array_equal(straight == VR.NONE, bent == VR.NONE)


def test_refraction_lift_against_numpy(topo):
    """topo_refraction_lift: the f64 formula, to a few ulps of the radius (1e-9 m each); k = 0 returns the point itself."""
    rng = np.random.default_rng(11)
    O = np.asarray(topo.ecef_from_lonlat(5.2, 44.5, 1700.0))
    for k in (0.0, 0.05, RCS.K, 0.999):
        for _ in range(25):
            p = np.asarray(topo.ecef_from_lonlat(5.2 + rng.uniform(-3, 3), 44.5 + rng.uniform(-2, 2), rng.uniform(-400, 8800)))
            got = topo.refraction_lift(O, p, k)
            want = RR.lift(O, p[None, :], k)[0]
            assert np.abs(got - want).max() < 1e-7, (k, p, got - want)
            assert got.tobytes() == RE.lift(O, p, k).tobytes(), "refraction_lift of topo_refraction.h under g++"
            if k == 0.0:
                assert got.tobytes() == p.tobytes()
            else:
                chord2 = ((p - O) ** 2).sum()
                assert abs((np.linalg.norm(got) - np.linalg.norm(p)) - k * chord2 / (2.0 * VR.R0)) < 1e-6
                assert np.abs(np.cross(got, p)).max() / np.linalg.norm(p) ** 2 < 1e-15, "the direction stays"
    for bad in (np.nan, -0.01, 1.0, np.inf):
        with pytest.raises(topo.TopoError) as e:
            topo.refraction_lift(O, O, bad)
        assert e.value.code == topo.TOPO_ERR_INVALID


def test_header_constant_and_binding(topo):
    assert topo.REFRACTION_STANDARD == RR.STANDARD == 0.13
    assert "#define TOPO_REFRACTION_STANDARD 0.13" in open(topo.HEADER_PATH).read()
    for fn in ("topo_visibility_refracted_grid_device", "topo_visibility_refracted_device", "topo_visibility_refracted_read", "topo_refraction_lift"):
        assert hasattr(topo.lib(), fn)


def build_harness(topo, tmp_path):
    exe = str(tmp_path / "refraction_abi_harness")
    libdir = os.path.dirname(topo.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(os.path.dirname(HERE), "include"), os.path.join(HERE, "refraction_abi_harness.c"), "-o",
                           exe, "-L", libdir, "-ltopo_hip", "-Wl,-rpath," + libdir, "-lm"])
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(os.path.dirname(__import__("torch").__file__), "lib") + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    return exe, env


def test_abi_harness_compiles_links_and_runs(topo, tmp_path):
    """The C99 view of the new declarations, and the part of the error contract that needs no GPU: topo_refraction_lift refuses
    k = NaN, -0.01 and 1.0, and the calls refuse a null context (the same harness run with `gpu` checks them on a context:
    tests/test_refraction_gpu.py)."""
    exe, env = build_harness(topo, tmp_path)
    out = subprocess.run([exe], env=env, capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    lines = out.stdout.strip().split("\n")
    assert lines[0].split() == ["0.13"]
    assert lines[1].split() == [str(topo.TOPO_ERR_INVALID)] * 4 + ["0", "0"], lines[1]
    assert lines[2].split() == [str(topo.TOPO_ERR_INVALID)] * 3
