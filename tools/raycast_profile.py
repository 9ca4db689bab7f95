#!/usr/bin/env python3
"""The ray queries' cost on the c4 mosaic (100 tiles of 1200 x 1200), for one 4096 x 1024 sector view from bench.py's viewpoint:
  (a) rays       1 048 576 pixel-centre rays of the sector (every fourth column) through the list call, topo_raycast_device;
  (b) sunlit     topo_sunlit_map_device over the sector's 4 194 304 pixels with the sun 10 degrees over the horizon.
Each is timed with events over a few repetitions and reported as ms, Mrays/s and the share of each class.  --lane-lib PATH: (a) also
through an experiment build of the launch shape that was not kept (a lane per ray: tools/exp_build.sh raycast_lane
"-DTOPO_RAYCAST_LANE" -> exp/libtopo_raycast_lane.so), in a child step of its own, with the records' hash beside the kept form's.

Without --step the tool drives two (three) child runs, each under its own `timeout`, and stops at the first that fails:
  1. `--step time`    the event timings and class shares;
  2. `--step trace`   one repetition of each under `rocprofv3 --kernel-trace --stats` (the program after `--`), for the kernels' own
                      durations (k_raycast, k_sunlit_map);
and writes both into --out (default profiles/raycast_c4.json)."""
import argparse
import csv
import glob
import hashlib
import json
import math
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEP_LIMIT_S = 120      # a step that cannot finish inside this has no pruning worth the name
SW, SH, RAY_COLUMN_STEP = 4096, 1024, 4
SUN_AZ_DEG, SUN_EL_DEG = 120.0, 10.0


def pixel_rays(T, np, u, W, H, xs, ys):
    """topo_ray records through the centres of pixels (xs, ys) of the view with uniforms u: the line between the points the inverse
    of camera_proj maps the pixel to on the near and the far plane, from the eye (camera_pos), f64."""
    f = np.ascontiguousarray(u).view(np.float32).reshape(-1)
    inv = np.linalg.inv(f[:16].astype(np.float64).reshape(4, 4).T)
    ndc = np.stack([(xs + 0.5) * 2.0 / W - 1.0, 1.0 - (ys + 0.5) * 2.0 / H], axis=-1)
    ends = []
    for z in (0.0, 1.0):
        p = np.concatenate([ndc, np.full((len(ndc), 1), z), np.ones((len(ndc), 1))], axis=1) @ inv.T
        ends.append(p[:, :3] / p[:, 3:4])
    d = ends[1] - ends[0]
    return T.rays(f[32:35].astype(np.float64), d / np.linalg.norm(d, axis=1)[:, None], 0.0, 1.0e6)


def step(args):
    import numpy as np
    import torch
    import topo_renderer_amd as T
    from bench import LAT0, LON0, TILE, WORKLOADS
    deg = WORKLOADS["c4"][0]
    reps = 1 if args.step == "trace" else args.reps
    r = T.TerrainRenderer(SW, SH)
    r.set_stream(torch.cuda.current_stream().cuda_stream)
    vlat, vlon = LAT0 + deg / 2 + 0.123, LON0 + deg / 2 + 0.217
    ground = None
    for (la, lo) in T.synth.mosaic_locations(LAT0, LON0, deg, deg):
        h = T.synth_tile(la, lo, TILE, TILE)
        if la == int(math.floor(vlat)) and lo == int(math.floor(vlon)):
            ground = T.synth.height_at(h, la, lo, vlon, vlat)
        r.add_terrain(la, lo, h, *T.synth.tile_transform(la, lo, TILE, TILE))
    r.synchronize()
    eye = T.geometry_transform(ground + 50.0, vlon, vlat)
    u = T.camera_uniforms(eye, 0.0, 0.0, float(T.lib().topo_sector_fov_y(SW, SH, T.N_SECTORS)), SW, SH, vlon, vlat, 0)
    ys, xs = np.mgrid[0:SH, 0:SW:RAY_COLUMN_STEP]
    rays = pixel_rays(T, np, u, SW, SH, xs.reshape(-1).astype(np.float64), ys.reshape(-1).astype(np.float64))
    n = len(rays)
    rays_dev = torch.from_numpy(rays.view(np.uint8).reshape(-1, 64).copy()).cuda()
    hits_dev = torch.zeros((n, 64), dtype=torch.uint8, device="cuda")
    rgba = torch.empty((1, SH, SW, 4), dtype=torch.uint8, device="cuda")
    depth = torch.empty((1, SH, SW), dtype=torch.float32, device="cuda")
    layer = torch.zeros((SH, SW), dtype=torch.uint8, device="cuda")
    sun = T.sun_direction(vlon, vlat, SUN_AZ_DEG, SUN_EL_DEG)
    r.render_views_device([u], SW, SH, rgba.data_ptr(), SH * SW * 4, SW * 4, depth.data_ptr(), SH * SW * 4, SW * 4)
    r.synchronize()

    def timed(call):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for a, b in ev:
            a.record()
            call()
            b.record()
        torch.cuda.synchronize()
        return sorted(a.elapsed_time(b) for a, b in ev)

    med = lambda ms: ms[len(ms) // 2]
    r.raycast_device(rays_dev.data_ptr(), hits_dev.data_ptr(), 256)      # (the first call builds the tables)
    torch.cuda.synchronize()
    ms_rays = timed(lambda: r.raycast_device(rays_dev.data_ptr(), hits_dev.data_ptr(), n))
    ms_sun = timed(lambda: r.sunlit_map_device(sun, layer.data_ptr())) if args.step != "lane" else [0.0]
    hits = hits_dev.cpu().numpy().view(T.RAY_HIT_DTYPE).reshape(-1)
    sha = hashlib.sha256(hits.tobytes()).hexdigest()[:24]
    if args.step == "lane":      # the experiment build: the list call alone
        print(json.dumps({"ms": {"median": round(med(ms_rays), 3), "min": round(ms_rays[0], 3), "max": round(ms_rays[-1], 3)},
                          "mrays_per_s": round(n / med(ms_rays) / 1e3, 2), "records_sha": sha}))
        return
    cls = np.bincount(layer.cpu().numpy().reshape(-1), minlength=4)
    lit_rays = int(cls[T.SUN_LIT] + cls[T.SUN_SHADOW])      # the pixels a shadow ray was cast for
    share = lambda k, total: round(float(k) / total, 4)
    print(json.dumps({
        "rays": {"n": n, "reps": reps, "form": "wave per ray", "ms": {"median": round(med(ms_rays), 3), "min": round(ms_rays[0], 3), "max": round(ms_rays[-1], 3)},
                 "mrays_per_s": round(n / med(ms_rays) / 1e3, 2),
                 "share": {"hit": share((hits["kind"] == T.RAY_HIT).sum(), n), "miss": share((hits["kind"] == T.RAY_MISS).sum(), n),
                           "invalid": share((hits["kind"] == T.RAY_INVALID).sum(), n)},
                 "records_sha": sha, "front_share_of_hits": share((hits["front"] == 1).sum(), max(1, int((hits["kind"] == T.RAY_HIT).sum())))},
        "sunlit": {"pixels": SW * SH, "reps": reps, "sun_az_el_deg": [SUN_AZ_DEG, SUN_EL_DEG],
                   "ms": {"median": round(med(ms_sun), 3), "min": round(ms_sun[0], 3), "max": round(ms_sun[-1], 3)},
                   "mpixels_per_s": round(SW * SH / med(ms_sun) / 1e3, 2), "shadow_rays": lit_rays,
                   "mrays_per_s": round(lit_rays / med(ms_sun) / 1e3, 2),
                   "share": {"none": share(cls[T.SUN_NONE], SW * SH), "lit": share(cls[T.SUN_LIT], SW * SH), "away": share(cls[T.SUN_AWAY], SW * SH),
                             "shadow": share(cls[T.SUN_SHADOW], SW * SH)}}}))


def run_step(cmd, what, env=None):
    res = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT_S)] + cmd, capture_output=True, text=True, env=env)
    if res.returncode != 0:
        sys.exit(f"{what}: exit status {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-2000:]}")
    return res.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["time", "trace", "lane"])
    ap.add_argument("--lane-lib", help="an experiment build with -DTOPO_RAYCAST_LANE: the list call through it, in a child step")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raycast_c4.json"))
    args = ap.parse_args()
    if args.step:
        return step(args)
    me = os.path.abspath(__file__)
    out = {"what": "tools/raycast_profile.py: the c4 mosaic (100 tiles of 1200 x 1200), one 4096 x 1024 sector view from bench.py's viewpoint; "
                   "rays = the pixel-centre rays of every fourth column through topo_raycast_device, sunlit = topo_sunlit_map_device of the "
                   "whole view; event-timed repetitions, then one repetition under rocprofv3 --kernel-trace --stats"}
    out.update(json.loads(run_step([sys.executable, me, "--step", "time", "--reps", str(args.reps)], "timing step").strip().split("\n")[-1]))
    if args.lane_lib:
        lane = json.loads(run_step([sys.executable, me, "--step", "lane", "--reps", str(args.reps)], "lane step",
                                   env=dict(os.environ, TOPO_HIP_LIB=os.path.abspath(args.lane_lib))).strip().split("\n")[-1])
        lane["same_records"] = lane.pop("records_sha") == out["rays"]["records_sha"]
        out["rays_lane_per_ray"] = lane
    with tempfile.TemporaryDirectory() as d:
        run_step(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "ray", "--", sys.executable, me, "--step", "trace"], "trace step")
        kernels = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                for k in ("k_raycast", "k_sunlit_map", "k_ground_tables"):
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
