"""Unwrap (topo_unwrap_*) without a GPU: the C ABI and its bindings; the product's per-pixel functions (topo_unwrap.h, built with g++:
tests/unwrap_emul.cpp) against the independent numpy reference (tests/unwrap_ref.py), against topo_pixel_angles and against
topo_unwrap_xy; the bilinear filter against the reference's f64 blend."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import unwrap_cases as UC
import unwrap_ref as UR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("topo_unwrap_device", "topo_unwrap_xy")
_DONE = {}


def located(name):
    """(case, the reference's locate, the emulation's nearest outputs over synthetic sources) of a case, computed once."""
    if name not in _DONE:
        import unwrap_emul
        views, sw, sh, params, how = UC.case(name)
        rgba, depth = UC.synthetic_sources(len(views), sw, sh)
        nearest = params.copy()
        nearest["filter"] = 0
        _DONE[name] = ((views, sw, sh, params, how), UR.locate(params, views, sw, sh), unwrap_emul.unwrap(nearest, views, sw, sh, rgba, depth), (rgba, depth))
    return _DONE[name]


def test_unwrap_symbols_are_declared_exported_and_bound(topo):
    header = open(topo.HEADER_PATH).read()
    assert re.search(r"\bint\s+topo_unwrap_device\s*\(", header) and re.search(r"\bvoid\s+topo_unwrap_xy\s*\(", header)
    nm = subprocess.run(["nm", "-D", "--defined-only", topo.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (topo_[a-z0-9_]+)", nm))
    L = topo.lib()
    for s in SYMBOLS:
        assert s in exported and s in L._topo_symbols, s
        assert getattr(L, s).argtypes is not None
    assert callable(getattr(topo.TerrainRenderer, "unwrap_device", None)) and callable(topo.unwrap_params) and callable(topo.unwrap_xy)
    for name, value in (("EQUIRECTANGULAR", 0), ("CYLINDRICAL", 1), ("NEAREST", 0), ("BILINEAR", 1)):
        assert getattr(topo, "UNWRAP_" + name) == value
        assert re.search(r"#define\s+TOPO_UNWRAP_%s\s+%du" % (name, value), header), name
    sys_src = open(os.path.join(ROOT, "rust", "topo-hip-sys", "src", "lib.rs")).read()
    assert "pub struct topo_unwrap_params" in sys_src
    for s in SYMBOLS:
        assert "pub fn " + s + "(" in sys_src
    out = subprocess.run(["strings", "-n", "6", topo.LIB_PATH], capture_output=True, text=True).stdout
    assert "k_unwrap" in out


def test_params_layout(topo):
    class Params(C.Structure):
        _fields_ = [("projection", C.c_uint32), ("filter", C.c_uint32), ("out_w", C.c_uint32), ("out_h", C.c_uint32), ("az0_deg", C.c_double),
                    ("az_span_deg", C.c_double), ("el_top_deg", C.c_double), ("el_bottom_deg", C.c_double)]
    D = topo.UNWRAP_PARAMS_DTYPE
    assert C.sizeof(Params) == 48 and D.itemsize == 48 and D.names == tuple(f for f, _ in Params._fields_)
    assert [D.fields[f][1] for f in D.names] == [getattr(Params, f).offset for f, _ in Params._fields_]
    src = '#include "topo_hip.h"\n_Static_assert(sizeof(topo_unwrap_params) == 48, "size");\n' \
          '_Static_assert(__builtin_offsetof(topo_unwrap_params, az0_deg) == 16 && __builtin_offsetof(topo_unwrap_params, el_bottom_deg) == 40, "offset");\n'
    res = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.dirname(topo.HEADER_PATH), "-x", "c", "-"], input=src, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    p = topo.unwrap_params(768, 160, 30.0, -30.0, az0_deg=5.0, az_span_deg=90.0, projection=1, filter=1)
    assert (int(p["out_w"][0]), int(p["out_h"][0]), int(p["projection"][0]), int(p["filter"][0])) == (768, 160, 1, 1)
    assert (float(p["az0_deg"][0]), float(p["az_span_deg"][0]), float(p["el_top_deg"][0]), float(p["el_bottom_deg"][0])) == (5.0, 90.0, 30.0, -30.0)


def test_argument_errors_without_a_device(topo):
    """No context exists without a device: the call refuses a null one; the host helper writes nothing for parameters out of range."""
    L = topo.lib()
    p = topo.unwrap_params(64, 32, 10.0, -10.0)
    u = np.zeros(160, np.uint8)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.topo_unwrap_device(None, ptr(p), 1, ptr(u), 8, 8, None, 0, 0, None, 0, 0, None, 0, None, 0, None, 0) == topo.TOPO_ERR_INVALID
    good = topo.unwrap_xy(p, [(180.0, 0.0)])
    assert np.allclose(good, [(32.0, 16.0)], atol=1e-12)
    for bad in (dict(out_w=0), dict(out_h=0), dict(az_span_deg=0.0), dict(az_span_deg=360.5), dict(el_top_deg=90.0), dict(el_bottom_deg=-90.0),
                dict(el_bottom_deg=10.0), dict(projection=2), dict(filter=2), dict(az0_deg=float("nan"))):
        q = p.copy()
        for k, v in bad.items():
            q[k] = v
        assert np.isnan(topo.unwrap_xy(q, [(180.0, 0.0)])).all(), bad
    L.topo_unwrap_xy(None, 1, None, None)      # (nothing to write to: must not crash)


@pytest.mark.parametrize("name", UC.NEAREST_CASES)
def test_source_map_equals_the_reference(topo, name):
    """Every pixel of the case: the g++ build of topo_unwrap.h names the texel the reference names.  The guard -- a pixel whose
    reference px / py lies within 1e-9 px of an integer or of a view edge, or whose two best cw agree to 1e-12 -- excludes NOTHING
    (f64 rounding is about 1e-13 px here; the closest approach is printed)."""
    (views, sw, sh, params, _), ref, emu, _ = located(name)
    print(f"case {name}: closest approach to an integer or an edge {ref['closest']:.2e} px; {int((ref['view'] < 0).sum())} pixels without a source, "
          f"{int((ref['n_containing'] > 1).sum())} in more than one view")
    assert not ref["fragile"].any(), int(ref["fragile"].sum())
    assert np.array_equal(emu["src"], ref["src"]), int((emu["src"] != ref["src"]).sum())
    has = ref["view"] >= 0
    assert has.any()
    assert np.abs(emu["pxy"][..., 0] - ref["px"])[has].max() < 1e-9 and np.abs(emu["pxy"][..., 1] - ref["py"])[has].max() < 1e-9
    assert np.isnan(emu["pxy"][~has]).all()


def test_cases_cover_what_they_are_for(topo):
    """Pitch 0: every direction inside the vertical field has exactly one containing sector and all eight are used; rows beyond the
    field are whole fill rows; pitch 10: gaps and overlaps, decided by the rule; three generic views overlap; a partial span."""
    a, c, d, f = (located(n)[1] for n in "acdf")
    assert (a["n_containing"] == 1).all() and set(np.unique(a["view"])) == set(range(8))
    fill_rows = (c["view"] < 0).all(axis=1)
    assert fill_rows[:20].all() and fill_rows[-20:].all() and not fill_rows[40:160].any() and (c["n_containing"] <= 1).all()
    assert (d["n_containing"] == 0).any() and (d["n_containing"] > 1).any()
    over = d["n_containing"] > 1
    print(f"case d: {100 * over.mean():.2f} % of the window in more than one sector, {100 * (d['n_containing'] == 0).mean():.2f} % in none")
    assert (f["n_containing"] >= 2).any() and (f["n_containing"] == 0).any() and set(np.unique(f["view"])) == {-1, 0, 1, 2}


@pytest.mark.parametrize("name", UC.NEAREST_CASES)
def test_fill_values_and_source_map_formula(topo, name):
    (views, sw, sh, params, _), ref, emu, (rgba, depth) = located(name)
    none = emu["src"] < 0
    assert np.array_equal(none, ref["view"] < 0)
    assert (emu["rgba"][none] == 0).all() and (emu["depth"].view(np.uint32)[none] == 0x7FC00000).all()
    sx, sy = np.floor(emu["pxy"][..., 0]), np.floor(emu["pxy"][..., 1])
    want = (ref["view"] * sh + sy) * sw + sx
    assert np.array_equal(emu["src"][~none], want[~none].astype(np.int64))
    assert emu["src"][~none].min() >= 0 and emu["src"].max() < len(views) * sw * sh
    # the nearest outputs are the sources gathered through the map
    assert np.array_equal(emu["rgba"], UR.gather(emu["src"], rgba, 0))
    assert np.array_equal(emu["depth"].view(np.uint32), UR.gather(emu["src"], depth.view(np.uint32), 0x7FC00000))


@pytest.mark.parametrize("name", UC.NEAREST_CASES)
def test_pixel_angles_of_the_source_point_are_the_output_pixels(topo, name):
    """An existing, independent helper: topo_pixel_angles inverts a view's whole camera_proj (translation included) and measures in
    the eye's frame.  For every covered pixel the source point (px, py) must look along the output pixel centre's azimuth and
    elevation within 1e-3 of the smallest angular width of a source pixel (the f32 rounding of the coordinates topo_pixel_angles
    takes is below 1e-5 px here; a wrong row, axis, sign or half-pixel offset is off by >= 0.5 px)."""
    (views, sw, sh, params, _), ref, emu, _ = located(name)
    corner = topo.pixel_angles(views[0], sw, sh, [(0.0, 0.0), (1.0, 0.0), (0.0, 1.0)])
    unit = lambda ae: np.array([np.cos(np.radians(ae[1])) * np.sin(np.radians(ae[0])), np.cos(np.radians(ae[1])) * np.cos(np.radians(ae[0])), np.sin(np.radians(ae[1]))])
    width = min(np.degrees(np.arccos(np.clip(unit(corner[0]) @ unit(corner[k]), -1, 1))) for k in (1, 2))      # the corner pixel: the smallest
    tol = 1e-3 * width
    az, el = np.broadcast_arrays(ref["az"][None, :], ref["el"][:, None])
    worst = 0.0
    for k in range(len(views)):
        sel = ref["view"] == k
        if not sel.any():
            continue
        got = topo.pixel_angles(views[k], sw, sh, emu["pxy"][sel])
        daz = np.abs((got[:, 0] - az[sel] + 180.0) % 360.0 - 180.0)
        dele = np.abs(got[:, 1] - el[sel])
        worst = max(worst, float(daz.max()), float(dele.max()))
    print(f"case {name}: worst angle error {worst:.2e} degrees = {worst / width:.2e} source pixels (bound 1e-3)")
    assert worst <= tol, (worst, tol)


@pytest.mark.parametrize("name", UC.NEAREST_CASES)
def test_unwrap_xy_round_trip(topo, name):
    (_, _, _, params, _), ref, _, _ = located(name)
    az, el = np.broadcast_arrays(ref["az"][None, :], ref["el"][:, None])
    xy = topo.unwrap_xy(params, np.stack([az % 360.0, el], axis=-1).reshape(-1, 2)).reshape(az.shape + (2,))
    yy, xx = np.mgrid[0:az.shape[0], 0:az.shape[1]]
    err = max(float(np.abs(xy[..., 0] - (xx + 0.5)).max()), float(np.abs(xy[..., 1] - (yy + 0.5)).max()))
    print(f"case {name}: round trip within {err:.2e} px")
    assert err <= 1e-9, err


# Channels (of 4 x 1536 x 320) on which the f32 blend and the reference's f64 blend may differ, by 1 LSB: only an f32 rounding at an
# encode threshold can do that.  Measured, emulation against reference, over the synthetic sources of case g (1 966 080 channels):
# 50 on an *Srgb format (25 per million), 174 on a plain one (89 per million); the test allows twice that.
BILINEAR_DIFF_MEASURED = {True: 50, False: 174}


@pytest.mark.parametrize("srgb", [True, False])
def test_bilinear_matches_the_f64_blend(topo, srgb):
    import unwrap_emul
    views, sw, sh, params, _ = UC.case("g")
    rgba, _ = UC.synthetic_sources(len(views), sw, sh)
    loc = UR.locate(params, views, sw, sh)
    assert not loc["fragile"].any()
    emu = unwrap_emul.unwrap(params, views, sw, sh, rgba, None, srgb=srgb)
    assert np.array_equal(emu["src"], loc["src"])
    want = UR.bilinear(loc, rgba, srgb)
    diff = np.abs(emu["rgba"].astype(np.int32) - want.astype(np.int32))
    n = int((diff != 0).sum())
    print(f"bilinear, srgb {srgb}: {n} of {diff.size} channels differ, largest difference {int(diff.max())} LSB")
    assert diff.max() <= 1
    assert n <= 2 * BILINEAR_DIFF_MEASURED[srgb], n
    # the blend is no gather: most pixels differ from the nearest texel
    assert (emu["rgba"] != UR.gather(loc["src"], rgba, 0)).any(axis=-1).mean() > 0.5
