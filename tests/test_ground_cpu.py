"""Ground points (topo_ground_*) without a GPU: the C ABI and its bindings; the numpy reference the GPU tests compare against
(tests/ground_ref.py) against the independent f64 ray caster; and the product's own lane function (topo_ground.h, built with g++:
tests/ground_emul.cpp) against that reference."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import geo_scenes as GS
import ground_ref as GR
from oracle import ray_check as RC
from scenes import RELIEF_SCENES as SCENES, Scene, relief
from viewshed_ref import geo_order

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("topo_ground_read", "topo_ground_device", "topo_ground_map_device")

# name: (Scene, W, H, yaw, pitch, fov) -- the ray-check scenes, then the two low-eye frames of the 96-texel 2 x 2 mosaic
CASES = {name: (dict(tile=c[0], n_lat=c[1], n_lon=c[2], lat0=c[3], lon0=c[4], eye_dh=c[10], height_fn=relief), c[5], c[6], c[7], c[8], c[9])
         for name, c in zip(("ne_2x2", "down_1x1", "sw_3x3"), SCENES)}
CASES["giants"] = (dict(tile=96, n_lat=2, n_lon=2, eye_dh=100.0), 200, 150, 120.0, 60.0, 90.0)      # near-clipped giants
CASES["low_eye"] = (dict(tile=96, n_lat=2, n_lon=2, eye_dh=50.0), 256, 128, 40.0, 10.0, 70.0)
for _name in GS.NAMES:      # off the 45N 15E quadrant: the scene of the pose's eye itself, one pose each and both eyes at the antimeridian
    for _k, (_eye, _yaw, _pitch, _fov) in enumerate(GS.placement(_name).poses[:2 if _name == "antimeridian" else 1]):
        CASES[_name + ("_west" if _k else "")] = (_eye, GS.W, GS.H, _yaw, _pitch, _fov)
_DONE = {}


def case(orc, name):
    """(scene, uniforms, oracle depth, oracle winners, reference) of a case, computed once."""
    if name not in _DONE:
        kw, W, H, yaw, pitch, fov = CASES[name]
        sc = kw if isinstance(kw, Scene) else Scene(**kw)
        o = orc.OracleRenderer(W, H)
        sc.load(o)
        u = sc.uniforms(W, H, yaw, pitch, fov, 1)
        o.update(W, H, u, np.array([W, H, 100.0, 0.0], np.float32))
        od, ow = o.render_winners()
        o.close()
        _DONE[name] = (sc, u, od, ow, GR.ground(od, ow, GR.scene_tiles(sc), sc.locs, u))
    return _DONE[name]


def test_ground_symbols_are_declared_exported_and_bound(topo):
    header = open(topo.HEADER_PATH).read()
    for s in SYMBOLS:
        assert re.search(r"\bint\s+" + s + r"\s*\(", header), s
    nm = subprocess.run(["nm", "-D", "--defined-only", topo.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (topo_[a-z0-9_]+)", nm))
    L = topo.lib()
    for s in SYMBOLS:
        assert s in exported and s in L._topo_symbols, s
        assert getattr(L, s).argtypes is not None
    for m in ("ground", "ground_device", "ground_map_device"):
        assert callable(getattr(topo.TerrainRenderer, m, None)), m
    for name, value in (("TERRAIN", 1), ("SKY", 0), ("INCOMPLETE", -2), ("DEGENERATE", -3)):
        assert getattr(topo, "GROUND_" + name) == value
        assert re.search(r"#define\s+TOPO_GROUND_%s\s+\(?%d\)?" % (name, value), header), name


def test_ground_calls_reject_null_arguments(topo):
    L = topo.lib()
    q, out = np.zeros(4, topo.GROUND_QUERY_DTYPE), np.zeros(4, topo.GROUND_DTYPE)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.topo_ground_read(None, 4, p(q), p(out)) == topo.TOPO_ERR_INVALID
    assert L.topo_ground_device(None, 4, p(q), p(out)) == topo.TOPO_ERR_INVALID
    assert L.topo_ground_map_device(None, 0, 1, p(out), 64, 64) == topo.TOPO_ERR_INVALID


def test_record_layouts(topo):
    class Point(C.Structure):
        _fields_ = [("lon_deg", C.c_double), ("lat_deg", C.c_double), ("height_m", C.c_float), ("range_m", C.c_float), ("depth", C.c_float),
                    ("kind", C.c_int32), ("tile_lat_deg", C.c_int32), ("tile_lon_deg", C.c_int32), ("cell_x", C.c_uint32), ("cell_y", C.c_uint32),
                    ("tri", C.c_uint32), ("fan", C.c_uint32), ("w1", C.c_float), ("w2", C.c_float)]

    class Query(C.Structure):
        _fields_ = [("view", C.c_uint32), ("x", C.c_uint32), ("y", C.c_uint32), ("_reserved", C.c_uint32)]
    assert C.sizeof(Point) == 64 and topo.GROUND_DTYPE.itemsize == 64
    assert [getattr(Point, f).offset for f, _ in Point._fields_] == [0, 8, 16, 20, 24, 28, 32, 36, 40, 44, 48, 52, 56, 60]
    assert topo.GROUND_DTYPE.names == tuple(f for f, _ in Point._fields_)
    assert [topo.GROUND_DTYPE.fields[f][1] for f in topo.GROUND_DTYPE.names] == [getattr(Point, f).offset for f, _ in Point._fields_]
    assert C.sizeof(Query) == 16 and topo.GROUND_QUERY_DTYPE.itemsize == 16
    assert [topo.GROUND_QUERY_DTYPE.fields[f][1] for f in topo.GROUND_QUERY_DTYPE.names] == [0, 4, 8, 12]
    # the header's own sizes, through a C compiler
    src = '#include "topo_hip.h"\n_Static_assert(sizeof(topo_ground_point) == 64 && sizeof(topo_ground_query) == 16, "size");\n' \
          '_Static_assert(__builtin_offsetof(topo_ground_point, kind) == 28 && __builtin_offsetof(topo_ground_point, w1) == 56, "offset");\n'
    res = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.dirname(topo.HEADER_PATH), "-x", "c", "-"], input=src, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    sys_src = open(os.path.join(ROOT, "rust", "topo-hip-sys", "src", "lib.rs")).read()
    assert "pub struct topo_ground_point" in sys_src and "pub struct topo_ground_query" in sys_src
    for s in SYMBOLS:
        assert "pub fn " + s + "(" in sys_src


def test_query_helper(topo):
    q = topo.ground_queries([(1, 2, 3), (4, 5, 6)])
    assert q.dtype == topo.GROUND_QUERY_DTYPE and list(q["view"]) == [1, 4] and list(q["x"]) == [2, 5] and list(q["y"]) == [3, 6]
    assert topo.ground_queries(q) is q or np.array_equal(topo.ground_queries(q), q)


@pytest.mark.parametrize("name", ["ne_2x2", "down_1x1", "sw_3x3"])
def test_reference_agrees_with_the_f64_ray_caster(orc, name):
    """Where the oracle's winner is the ray caster's, the reference's point, reprojected through the ray caster's OWN camera
    (RC.camera_basis: no matrix), lands on the pixel centre within 0.01 px + (4 m / range) x focal length in px -- 4 m is
    ray_check.compare's slack_clip, for the same reason: the f32 matrix places the eye to about a metre."""
    import topo_renderer_amd as T
    kw, W, H, yaw, pitch, fov = CASES[name]
    sc, u, od, ow, ref = case(orc, name)
    tile = kw["tile"]
    tiles = [(sc.heights[l],) + tuple(T.synth.tile_transform(l[0], l[1], tile, tile)) for l in geo_order(sc.locs)]
    _, rw, _, _ = RC.ray_cast(tiles, sc.eye, math.radians(yaw), math.radians(pitch), math.radians(fov), W, H)
    terrain = ref["terrain"]
    assert terrain.mean() > 0.25
    assert ref["finite"][terrain].all() and (ref["kind"][terrain] == 1).all()      # no pixel is non-finite
    same = terrain & (ow.astype(np.int64) == rw)
    agree = float(same.sum()) / float(terrain.sum())
    f, s, up = RC.camera_basis(np.asarray(sc.eye, np.float64), math.radians(yaw), math.radians(pitch))
    v = ref["p"] - np.asarray(sc.eye, np.float64)
    t = v @ f
    th = math.tan(0.5 * math.radians(fov))
    with np.errstate(all="ignore"):
        px = ((v @ s) / (t * th * (W / H)) + 1.0) * 0.5 * W
        py = (1.0 - (v @ up) / (t * th)) * 0.5 * H
    yy, xx = np.mgrid[0:H, 0:W]
    err = np.hypot(px - (xx + 0.5), py - (yy + 0.5))
    focal_px = 0.5 * H / th
    bound = 0.01 + 4.0 / ref["range_m"].clip(1.0) * focal_px
    worst = float((err / bound)[same].max())
    print(f"{name}: winners agree on {100 * agree:.2f} % of {int(terrain.sum())} terrain pixels; worst reprojection error {worst:.3f} of the bound")
    assert agree >= 0.998, agree
    assert np.isfinite(err[same]).all() and worst <= 1.0, worst


@pytest.mark.parametrize("name", list(CASES))
def test_lane_function_matches_the_reference(orc, name):
    """The product's topo_ground.h under g++ over every pixel of the frame: exact fields equal, ECEF point / height / range within
    1e-3 m (two independent f64 formulations of the definition differ by at most 4.7e-5 m and 3.4e-9 x range on these five
    scenes: the tolerance is about 20 x that and still 500 x below the f32 ECEF ulp), weights within 1e-6, no degenerate record
    (the reference has none), the point at most marginally outside its triangle."""
    import ground_emul
    sc, u, od, ow, ref = case(orc, name)
    got = ground_emul.ground(GR.scene_tiles(sc), geo_order(sc.locs), u, od, ow)
    assert (ref["kind"] != -3).all() and (got["kind"] != -3).all()
    assert (got["fan"] == 0).all()
    st = GR.compare(got, ref, name, f64=got)
    assert st["terrain"] > 0.25 * st["pixels"]
    t = got["kind"] == 1
    min_bary = float(np.minimum(np.minimum(got["w1"], got["w2"]), 1.0 - got["w1"] - got["w2"])[t].min())
    print(f"{name}: min barycentric {min_bary:.4f} (reference {st['min_bary']:.4f}); point within {st['point_m']:.2e} m = {st['point_over_range']:.2e} x range")
    assert min_bary >= -0.1 and st["min_bary"] >= -0.1
