#!/usr/bin/env python3
"""The surface queries' cost on the c4 mosaic (100 tiles of 1200 x 1200):
  (a) points    1 048 576 uniformly random points of the mosaic's 10 x 10 degrees through the list call, topo_surface_device, and
                the SAME points as nadir rays from 20 km through topo_raycast_device -- the only way to ask before there was a
                direct lookup -- with the share of points whose tile, cell and triangle agree;
  (b) grid      topo_surface_grid_device, 4096 x 4096 over the mosaic;
  (c) profiles  topo_profile_device, 4096 segments of 100 km with 1024 samples each, from random points in random directions
                3 km over the sphere at both ends.
Each is timed with events over a few repetitions after a warm-up call and reported as ms and Mpoints/s.

Without --step the tool drives two child runs, each under its own `timeout`, and stops at the first that fails:
  1. `--step time`    the event timings, the agreement and the kinds' shares;
  2. `--step trace`   one repetition of each under `rocprofv3 --kernel-trace --stats` (the program after `--`), for the kernels' own
                      durations (k_surface, k_surface_grid, k_profile, k_raycast);
and writes both into --out (default profiles/surface_c4.json)."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEP_LIMIT_S = 180
N_POINTS, RAY_HEIGHT_M = 1 << 20, 20000.0
GRID = 4096
N_SEGMENTS, SEGMENT_M, SAMPLES, SEGMENT_HEIGHT_M = 4096, 100000.0, 1024, 3000.0
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
    rng = np.random.default_rng(7)
    pts = np.stack([rng.uniform(LON0, LON0 + deg, N_POINTS), rng.uniform(LAT0, LAT0 + deg, N_POINTS)], axis=-1)

    def up(lon, lat):
        lo, la = np.radians(lon), np.radians(lat)
        return np.stack([np.cos(la) * np.cos(lo), np.cos(la) * np.sin(lo), np.sin(la)], axis=-1)

    u = up(pts[:, 0], pts[:, 1])
    rays = T.rays((R0 + RAY_HEIGHT_M) * u, -u, 0.0, 1.0e6)
    # segments: from a random point of the inner 8 x 8 degrees, 100 km along a random azimuth (east / north frame at the start)
    slon, slat = rng.uniform(LON0 + 1, LON0 + deg - 1, N_SEGMENTS), rng.uniform(LAT0 + 1, LAT0 + deg - 1, N_SEGMENTS)
    az = rng.uniform(0.0, 2.0 * np.pi, N_SEGMENTS)
    su = up(slon, slat)
    east = np.stack([-np.sin(np.radians(slon)), np.cos(np.radians(slon)), 0.0 * slon], axis=-1)
    north = np.cross(su, east)
    a = (R0 + SEGMENT_HEIGHT_M) * su
    b = a + SEGMENT_M * (np.sin(az)[:, None] * east + np.cos(az)[:, None] * north)
    b *= ((R0 + SEGMENT_HEIGHT_M) / np.linalg.norm(b, axis=1))[:, None]
    segs = T.rays(a, b - a, 0.0, 1.0)

    pts_dev = torch.from_numpy(pts.copy()).cuda()
    rec_dev = torch.zeros((N_POINTS, 48), dtype=torch.uint8, device="cuda")
    rays_dev = torch.from_numpy(rays.view(np.uint8).reshape(-1, 64).copy()).cuda()
    hits_dev = torch.zeros((N_POINTS, 64), dtype=torch.uint8, device="cuda")
    grid_dev = torch.zeros((GRID, GRID), dtype=torch.float32, device="cuda")
    segs_dev = torch.from_numpy(segs.view(np.uint8).reshape(-1, 64).copy()).cuda()
    smp_dev = torch.zeros((N_SEGMENTS, SAMPLES, 2), dtype=torch.float32, device="cuda")
    sum_dev = torch.zeros((N_SEGMENTS, 16), dtype=torch.uint8, device="cuda")

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

    ms = {
        "surface": timed(lambda: r.surface_device(pts_dev.data_ptr(), rec_dev.data_ptr(), N_POINTS)),
        "raycast": timed(lambda: r.raycast_device(rays_dev.data_ptr(), hits_dev.data_ptr(), N_POINTS)),
        "grid": timed(lambda: r.surface_grid_device(LON0, LAT0 + deg, deg / GRID, -deg / GRID, GRID, GRID, grid_dev.data_ptr())),
        "profile": timed(lambda: r.profile_device(segs_dev.data_ptr(), N_SEGMENTS, SAMPLES, sum_dev.data_ptr(), smp_dev.data_ptr())),
    }
    if args.step == "trace":
        return
    med = lambda v: v[len(v) // 2]
    rate = lambda n, v: round(n / med(v) / 1e3, 2)
    stat = lambda v: {"median": round(med(v), 3), "min": round(v[0], 3), "max": round(v[-1], 3)}
    rec = rec_dev.cpu().numpy().view(T.SURFACE_DTYPE).reshape(-1)
    hits = hits_dev.cpu().numpy().view(T.RAY_HIT_DTYPE).reshape(-1)
    terrain = rec["kind"] == T.SURFACE_TERRAIN
    same = (terrain == (hits["kind"] == T.RAY_HIT)) & np.all([rec[f] == hits[f] for f in ("tile_lat_deg", "tile_lon_deg", "cell_x", "cell_y", "tri")], axis=0)
    both = terrain & (hits["kind"] == T.RAY_HIT)
    summary = sum_dev.cpu().numpy().view(T.PROFILE_SUMMARY_DTYPE).reshape(-1)
    grid = grid_dev.cpu().numpy()
    share = lambda k, total: round(float(k) / total, 6)
    print(json.dumps({
        "points": {"n": N_POINTS, "reps": reps, "surface_ms": stat(ms["surface"]), "surface_mpoints_per_s": rate(N_POINTS, ms["surface"]),
                   "raycast_ms": stat(ms["raycast"]), "raycast_mrays_per_s": rate(N_POINTS, ms["raycast"]),
                   "raycast_over_surface": round(med(ms["raycast"]) / med(ms["surface"]), 2),
                   "share": {"terrain": share(terrain.sum(), N_POINTS), "same_tile_cell_triangle": share(same.sum(), N_POINTS)},
                   "largest_height_difference_m": float(np.abs(RAY_HEIGHT_M - hits["t"][both] - rec["height_m"][both]).max())},
        "grid": {"nx": GRID, "ny": GRID, "reps": reps, "ms": stat(ms["grid"]), "mpoints_per_s": rate(GRID * GRID, ms["grid"]),
                 "share_terrain": share((~np.isnan(grid)).sum(), GRID * GRID)},
        "profiles": {"segments": N_SEGMENTS, "length_m": SEGMENT_M, "samples": SAMPLES, "reps": reps, "ms": stat(ms["profile"]),
                     "msamples_per_s": rate(N_SEGMENTS * SAMPLES, ms["profile"]), "share_samples_over_terrain": share(summary["n_terrain"].sum(), N_SEGMENTS * SAMPLES),
                     "share_segments_below_ground": share((summary["min_clearance_m"] < 0).sum(), N_SEGMENTS)}}))


def run_step(cmd, what):
    res = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT_S)] + cmd, capture_output=True, text=True)
    if res.returncode != 0:
        sys.exit(f"{what}: exit status {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-2000:]}")
    return res.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["time", "trace"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface_c4.json"))
    args = ap.parse_args()
    if args.step:
        return step(args)
    me = os.path.abspath(__file__)
    out = {"what": "tools/surface_profile.py: the c4 mosaic (100 tiles of 1200 x 1200); points = 1 048 576 random points through topo_surface_device and the "
                   "same points as nadir rays from 20 km through topo_raycast_device, grid = topo_surface_grid_device 4096 x 4096 over the mosaic, profiles = "
                   "topo_profile_device, 4096 segments of 100 km x 1024 samples; event-timed repetitions after a warm-up, then one repetition under "
                   "rocprofv3 --kernel-trace --stats"}
    out.update(json.loads(run_step([sys.executable, me, "--step", "time", "--reps", str(args.reps)], "timing step").strip().split("\n")[-1]))
    with tempfile.TemporaryDirectory() as d:
        run_step(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "surface", "--", sys.executable, me, "--step", "trace"], "trace step")
        kernels = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                for k in ("k_surface", "k_surface_grid", "k_profile", "k_raycast", "k_ground_tables"):
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
