#!/usr/bin/env python3
"""The refracted visibility query's cost on the c4 mosaic (100 tiles of 1200 x 1200): a 1024 x 1024 grid of targets over the mosaic's
10 x 10 degrees, seen from bench.py's viewpoint 2 m above the terrain (a hut: near-horizontal sight lines, the expensive rays) under
the standard coefficient k = 0.13.  In ONE process, alternating round by round:
  new        topo_visibility_refracted_grid_device at k = 0.13;
  (a) plain  topo_visibility_grid_device on the same grid: the difference is the price of refraction;
  (b) composed  what a caller could do before, for this one observer: lift every DEM post on the host (numpy, f64, re-rounded to
             f32), re-add the 100 tiles to a second context (one upload of the whole mosaic), then the plain call there.  Its classes
             are those of `new` up to the f32 re-rounding of the lifted heights; the share that differs is reported.
`new` and (a) are timed with events, (b) with a host clock around a synchronise (host work and uploads are most of it).

Without --step the tool runs the measurement in a child under its own `timeout` and writes medians and spreads into --out (default
profiles/refraction_c4.json)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEP_LIMIT_S = 400
GRID = 1024
HEIGHT_M = 2.0
R0 = 6371000.0


def step(args):
    import numpy as np
    import torch
    import topo_renderer_amd as T
    from bench import LAT0, LON0, TILE, WORKLOADS
    deg = WORKLOADS["c4"][0]
    k = T.REFRACTION_STANDARD
    locs = T.synth.mosaic_locations(LAT0, LON0, deg, deg)
    tiles = {loc: T.synth_tile(loc[0], loc[1], TILE, TILE) for loc in locs}
    r, r2 = T.TerrainRenderer(64, 64), T.TerrainRenderer(64, 64)
    for g in (r, r2):
        g.set_stream(torch.cuda.current_stream().cuda_stream)
        for (la, lo) in locs:
            g.add_terrain(la, lo, tiles[la, lo], *T.synth.tile_transform(la, lo, TILE, TILE))
        g.synchronize()
    vlat, vlon = LAT0 + deg / 2 + 0.123, LON0 + deg / 2 + 0.217      # bench.py's viewpoint
    n = GRID * GRID
    dlon, dlat = deg / GRID, -deg / GRID
    lon0, lat0 = LON0 + 0.37 * dlon, LAT0 + deg + 0.41 * dlat      # off the DEM lattice
    obs = T.observers(vlon, vlat, HEIGHT_M)
    out_new, out_plain, out_comp = (torch.zeros((GRID, GRID), dtype=torch.uint8, device="cuda") for _ in range(3))
    base = torch.zeros((1, 1), dtype=torch.float32, device="cuda")
    r.surface_grid_device(vlon, vlat, 0.0, 0.0, 1, 1, base.data_ptr())
    r.synchronize()
    ground = float(base.cpu().numpy()[0, 0])
    O = T.ecef_from_lonlat(vlon, vlat, ground + HEIGHT_M)
    over_sphere = T.observers(vlon, vlat, ground + HEIGHT_M, above_terrain=False)      # (b)'s observer: O stays where it was

    def lifted(la, lo):
        """The tile's posts lifted for O: |v - O|^2 = r^2 + |O|^2 - 2 r u . O with v = r u."""
        x = np.arange(TILE, dtype=np.float64) / TILE
        lon, lat = np.radians(lo + x)[None, :], np.radians(la + 1 - x)[:, None]
        u_o = np.cos(lat) * np.cos(lon) * O[0] + np.cos(lat) * np.sin(lon) * O[1] + np.sin(lat) * O[2]
        rad = R0 + tiles[la, lo].astype(np.float64)
        return (tiles[la, lo] + (k / (2.0 * R0)) * (rad * rad + O @ O - 2.0 * rad * u_o)).astype(np.float32)

    def event_timed(call):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        call()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e)

    def composed():
        t0 = time.perf_counter()
        for (la, lo) in locs:
            r2.add_terrain(la, lo, lifted(la, lo), *T.synth.tile_transform(la, lo, TILE, TILE))
        t1 = time.perf_counter()
        r2.visibility_grid_device(over_sphere, lon0, lat0, dlon, dlat, GRID, GRID, out_comp.data_ptr())
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), 1e3 * (t1 - t0)

    new = lambda: r.visibility_refracted_grid_device(obs, lon0, lat0, dlon, dlat, GRID, GRID, out_new.data_ptr(), 0.0, k)
    plain = lambda: r.visibility_grid_device(obs, lon0, lat0, dlon, dlat, GRID, GRID, out_plain.data_ptr())
    new()
    plain()      # warm-up (the first call of all builds the tables)
    torch.cuda.synchronize()
    ms = {"new": [], "plain": [], "composed": [], "composed_lift_and_upload": []}
    for i in range(args.reps):
        ms["new"].append(event_timed(new))
        ms["plain"].append(event_timed(plain))
        if i < args.composed_reps:
            total, upload = composed()
            ms["composed"].append(total)
            ms["composed_lift_and_upload"].append(upload)
    stat = lambda v: {"median": round(sorted(v)[len(v) // 2], 3), "min": round(min(v), 3), "max": round(max(v), 3), "n": len(v)}
    a, b, c = (t.cpu().numpy().reshape(-1) for t in (out_new, out_plain, out_comp))
    share = lambda cls: {name: round(float((cls == v).sum()) / n, 6) for name, v in (("none", T.VIS_NONE), ("visible", T.VIS_VISIBLE), ("away", T.VIS_AWAY),
                                                                                      ("hidden", T.VIS_HIDDEN))}
    res = {"grid": {"nx": GRID, "ny": GRID}, "observer_height_above_terrain_m": HEIGHT_M, "refraction_k": k,
           "ms": {key: stat(v) for key, v in ms.items() if v}, "share_refracted": share(a), "share_plain": share(b),
           "targets_that_change_class_under_refraction": int((a != b).sum())}
    res["refraction_over_plain"] = round(res["ms"]["new"]["median"] / res["ms"]["plain"]["median"], 3)
    if ms["composed"]:
        res["composed_over_new"] = round(res["ms"]["composed"]["median"] / res["ms"]["new"]["median"], 2)
        res["composed_targets_that_differ_from_new"] = int((a != c).sum())
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["time"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--composed-reps", type=int, default=3, help="how many of the rounds also run the host composition (b)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refraction_c4.json"))
    args = ap.parse_args()
    if args.step:
        return step(args)
    res = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--step", "time", "--reps", str(args.reps),
                          "--composed-reps", str(args.composed_reps)], capture_output=True, text=True)
    if res.returncode != 0:
        sys.exit(f"timing step: exit status {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-2000:]}")
    out = {"what": "tools/refraction_profile.py: the c4 mosaic (100 tiles of 1200 x 1200); a 1024 x 1024 grid of targets over the mosaic from bench.py's viewpoint "
                   "2 m above the terrain; new = topo_visibility_refracted_grid_device at k = 0.13, plain = topo_visibility_grid_device, composed = every post "
                   "lifted on the host for this observer, the 100 tiles re-added, then the plain call; one process, the three alternating round by round"}
    out.update(json.loads(res.stdout.strip().split("\n")[-1]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
