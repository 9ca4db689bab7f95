#!/usr/bin/env python3
"""The visibility queries' cost on the c4 mosaic (100 tiles of 1200 x 1200): a 1024 x 1024 grid of targets over the mosaic's 10 x 10
degrees, seen from bench.py's viewpoint 2 m above the terrain (a hut: near-horizontal sight lines, the expensive rays) and from
1500 m above it (a summit or an aircraft).  For each observer
  (a) new       topo_visibility_grid_device;
  (b) composed  what a caller could do before: topo_surface_grid_device for the targets' heights (and the observer's), the sight
                lines built as topo_ray records with torch on the device (f64; the targets' unit directions are computed once, outside
                the timing), topo_raycast_device -- a FIRST-hit search with full records where any hit would do; it cannot leave out
                the target's own triangle nor tell ground that faces away, so its classes are only roughly those of (a);
  (c) lane      --lane-lib PATH: (a) through an experiment build of the launch shape that was not kept (a lane per target:
                tools/exp_build.sh visibility_lane "-DTOPO_VISIBILITY_LANE" -> exp/libtopo_visibility_lane.so), in a child step of its
                own, with the classes' hash beside the kept form's.
Each is timed with events over a few repetitions after a warm-up call.

Without --step the tool drives its child runs, each under its own `timeout`, and stops at the first that fails:
  1. `--step time`    the event timings and class shares;
  2. `--step lane`    (with --lane-lib) the new call alone through the experiment build;
  3. `--step trace`   (unless --no-trace) one repetition of (a) and (b) under `rocprofv3 --kernel-trace --stats` (the program after
                      `--`), for the kernels' own durations;
and writes all of it into --out (default profiles/visibility_c4.json)."""
import argparse
import csv
import glob
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEP_LIMIT_S = 240
GRID = 1024
OBSERVER_HEIGHTS_M = (2.0, 1500.0)
R0 = 6371000.0


def step(args):
    import numpy as np
    import torch
    import topo_renderer_amd as T
    from bench import LAT0, LON0, TILE, WORKLOADS
    deg = WORKLOADS["c4"][0]
    reps = 1 if args.step == "trace" else args.reps
    r = T.TerrainRenderer(64, 64)
    r.set_stream(torch.cuda.current_stream().cuda_stream)
    for (la, lo) in T.synth.mosaic_locations(LAT0, LON0, deg, deg):
        r.add_terrain(la, lo, T.synth_tile(la, lo, TILE, TILE), *T.synth.tile_transform(la, lo, TILE, TILE))
    r.synchronize()
    vlat, vlon = LAT0 + deg / 2 + 0.123, LON0 + deg / 2 + 0.217      # bench.py's viewpoint
    n = GRID * GRID
    dlon, dlat = deg / GRID, -deg / GRID
    lon0, lat0 = LON0 + 0.37 * dlon, LAT0 + deg + 0.41 * dlat      # off the DEM lattice
    out_dev = torch.zeros((GRID, GRID), dtype=torch.uint8, device="cuda")

    def timed(call):
        call()      # warm-up (the first call of all builds the tables)
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for s, e in ev:
            s.record()
            call()
            e.record()
        torch.cuda.synchronize()
        return sorted(s.elapsed_time(e) for s, e in ev)

    med = lambda v: v[len(v) // 2]
    stat = lambda v: {"median": round(med(v), 3), "min": round(v[0], 3), "max": round(v[-1], 3)}
    share = lambda k: round(float(k) / n, 6)

    # (b)'s fixed inputs: the targets' unit directions, the observer's
    lon = torch.deg2rad(lon0 + torch.arange(GRID, dtype=torch.float64, device="cuda") * dlon)
    lat = torch.deg2rad(lat0 + torch.arange(GRID, dtype=torch.float64, device="cuda") * dlat)
    U = torch.stack([torch.cos(lat)[:, None] * torch.cos(lon)[None, :], torch.cos(lat)[:, None] * torch.sin(lon)[None, :],
                     torch.sin(lat)[:, None].expand(GRID, GRID)], dim=-1).contiguous()
    uo = torch.tensor(T.ecef_from_lonlat(vlon, vlat, 1.0 - R0), dtype=torch.float64, device="cuda")
    hts = torch.zeros((GRID, GRID), dtype=torch.float32, device="cuda")
    base = torch.zeros((1, 1), dtype=torch.float32, device="cuda")
    rays = torch.zeros((n, 8), dtype=torch.float64, device="cuda")
    hits = torch.zeros((n, 64), dtype=torch.uint8, device="cuda")

    def composed(height):
        r.surface_grid_device(lon0, lat0, dlon, dlat, GRID, GRID, hts.data_ptr())
        r.surface_grid_device(vlon, vlat, 0.0, 0.0, 1, 1, base.data_ptr())
        Tp = (R0 + hts.double())[..., None] * U      # (a NaN height: a NaN origin, an invalid ray)
        D = (R0 + base.double().reshape(()) + height) * uo - Tp
        L = torch.linalg.norm(D, dim=-1)
        rays[:, 0:3] = Tp.reshape(n, 3)
        rays[:, 3:6] = (D / L[..., None]).reshape(n, 3)
        rays[:, 6] = 1.0e-3
        rays[:, 7] = L.reshape(n)
        r.raycast_device(rays.data_ptr(), hits.data_ptr(), n)

    res = {}
    for height in OBSERVER_HEIGHTS_M:
        obs = T.observers(vlon, vlat, height)
        ms_new = timed(lambda: r.visibility_grid_device(obs, lon0, lat0, dlon, dlat, GRID, GRID, out_dev.data_ptr()))
        cls = out_dev.cpu().numpy().reshape(-1)
        entry = {"observer_height_above_terrain_m": height, "ms": stat(ms_new), "mtargets_per_s": round(n / med(ms_new) / 1e3, 2),
                 "classes_sha": hashlib.sha256(cls.tobytes()).hexdigest()[:24]}
        if args.step != "lane":
            count = np.bincount(cls, minlength=5)
            entry["share"] = {"none": share(count[T.VIS_NONE]), "visible": share(count[T.VIS_VISIBLE]), "away": share(count[T.VIS_AWAY]),
                              "hidden": share(count[T.VIS_HIDDEN]), "no_observer": share(count[T.VIS_NO_OBSERVER])}
            ms_surface = timed(lambda: r.surface_grid_device(lon0, lat0, dlon, dlat, GRID, GRID, hts.data_ptr()))
            ms_all = timed(lambda: composed(height))
            ms_cast = timed(lambda: r.raycast_device(rays.data_ptr(), hits.data_ptr(), n))
            kind = hits.cpu().numpy().view(T.RAY_HIT_DTYPE).reshape(-1)["kind"]
            entry["composed"] = {"ms": stat(ms_all), "surface_grid_ms": stat(ms_surface), "raycast_ms": stat(ms_cast),
                                 "rays_built_with_torch_ms": round(med(ms_all) - med(ms_surface) - med(ms_cast), 3),
                                 "over_new": round(med(ms_all) / med(ms_new), 2),
                                 "share": {"invalid": share((kind == T.RAY_INVALID).sum()), "miss": share((kind == T.RAY_MISS).sum()), "hit": share((kind == T.RAY_HIT).sum())}}
        res[f"observer_{int(height)}m"] = entry
    print(json.dumps({"grid": {"nx": GRID, "ny": GRID, "reps": reps}, **res}))


def run_step(cmd, what, env=None):
    res = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT_S)] + cmd, capture_output=True, text=True, env=env)
    if res.returncode != 0:
        sys.exit(f"{what}: exit status {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-2000:]}")
    return res.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["time", "trace", "lane"])
    ap.add_argument("--lane-lib", help="an experiment build with -DTOPO_VISIBILITY_LANE: the grid call through it, in a child step")
    ap.add_argument("--no-trace", action="store_true", help="leave out the rocprofv3 step")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "visibility_c4.json"))
    args = ap.parse_args()
    if args.step:
        return step(args)
    me = os.path.abspath(__file__)
    out = {"what": "tools/visibility_profile.py: the c4 mosaic (100 tiles of 1200 x 1200); a 1024 x 1024 grid of targets over the mosaic from bench.py's "
                   "viewpoint 2 m and 1500 m above the terrain through topo_visibility_grid_device (a wave takes the rays of its 64 targets one at a time), "
                   "composed = topo_surface_grid_device + rays built with torch on the device + topo_raycast_device, lane_per_target = the grid call "
                   "through a -DTOPO_VISIBILITY_LANE build; event-timed repetitions after a warm-up"}
    out.update(json.loads(run_step([sys.executable, me, "--step", "time", "--reps", str(args.reps)], "timing step").strip().split("\n")[-1]))
    if args.lane_lib:
        lane = json.loads(run_step([sys.executable, me, "--step", "lane", "--reps", str(args.reps)], "lane step",
                                   env=dict(os.environ, TOPO_HIP_LIB=os.path.abspath(args.lane_lib))).strip().split("\n")[-1])
        for key, entry in lane.items():
            if key.startswith("observer_"):
                entry["same_bytes"] = entry.pop("classes_sha") == out[key]["classes_sha"]
                entry["over_wave_form"] = round(entry["ms"]["median"] / out[key]["ms"]["median"], 2)
                out[key]["lane_per_target"] = entry
    if not args.no_trace:
        with tempfile.TemporaryDirectory() as d:
            run_step(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "vis", "--", sys.executable, me, "--step", "trace"], "trace step")
            kernels = {}
            for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
                for row in csv.DictReader(open(path)):
                    for k in ("k_visibility_grid", "k_visibility_observers", "k_surface_grid", "k_raycast", "k_ground_tables"):
                        if k + "(" in row["Name"]:
                            kernels[k] = {"calls": int(row["Calls"]), "average_ms": round(float(row["AverageNs"]) / 1e6, 3), "max_ms": round(float(row["MaxNs"]) / 1e6, 3)}
            out["kernels_rocprofv3"] = kernels
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
