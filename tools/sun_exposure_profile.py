#!/usr/bin/env python3
"""The sun exposure queries' cost on the c4 mosaic (100 tiles of 1200 x 1200): a 1024 x 1024 grid of targets over the mosaic's 10 x 10
degrees under 48 suns along the arc of 21 December at the mosaic's centre (declination -23.44 degrees; the samples are evenly spaced
in time between sunrise and sunset of the sphere, the weight of each is its minutes).
  (a) new       topo_sun_exposure_grid_device, all three outputs -- on the full grid, and on a 256 x 256 subgrid (every fourth
                column and row: the same extent, the same rays, a sixteenth of the waves) that (c) is timed on;
  (b) composed  what a caller could do before, on both grids: topo_surface_device for the targets' heights, slopes and aspects;
                per sun, with torch on the device, the targets whose own horizontal plane and whose slope face the sun, and their
                topo_ray records (f64; the targets' unit directions and frames are computed once, outside the timing);
                topo_raycast_device once per sun -- a FIRST-hit search with full records where any hit would do; it cannot leave out
                the target's own triangle, so its classes are only roughly those of (a);
  (c) lane      --lane-lib PATH: (a) on the subgrid through an experiment build of the launch shape that was not kept (a lane per
                target: tools/exp_build.sh sun_lane "-DTOPO_SUN_LANE" -> exp/libtopo_sun_lane.so), in a child step of its own, with
                the outputs' hash beside the kept form's.
Each is timed with events over a few repetitions after a warm-up call.

Without --step the tool drives its child runs, each under its own `timeout`, and stops at the first that fails:
  1. `--step time`       (a) on both grids, the class shares;
  2. `--step composed`   (b);
  3. `--step lane`       (with --lane-lib) (a) on the subgrid through the experiment build;
and writes all of it into --out (default profiles/sun_exposure_c4.json)."""
import argparse
import hashlib
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEP_LIMIT_S = 420
GRID, SUB = 1024, 256
N_SUNS = 48
DECLINATION_DEG = -23.44
R0 = 6371000.0


def winter_arc(lat_deg):
    """[(azimuth, elevation, minutes)] of N_SUNS samples at the centres of equal time steps between sunrise and sunset."""
    phi, dec = math.radians(lat_deg), math.radians(DECLINATION_DEG)
    h0 = math.acos(-math.tan(phi) * math.tan(dec))      # the hour angle of sunset
    minutes = 2.0 * math.degrees(h0) * 4.0 / N_SUNS
    arc = []
    for k in range(N_SUNS):
        h = -h0 + (k + 0.5) * 2.0 * h0 / N_SUNS
        el = math.asin(math.sin(phi) * math.sin(dec) + math.cos(phi) * math.cos(dec) * math.cos(h))
        az = math.atan2(-math.cos(dec) * math.sin(h), math.sin(dec) * math.cos(phi) - math.cos(dec) * math.cos(h) * math.sin(phi))
        arc.append((math.degrees(az) % 360.0, math.degrees(el), minutes))
    return arc


def step(args):
    import numpy as np
    import torch
    import topo_renderer_amd as T
    from bench import LAT0, LON0, TILE, WORKLOADS
    deg = WORKLOADS["c4"][0]
    r = T.TerrainRenderer(64, 64)
    r.set_stream(torch.cuda.current_stream().cuda_stream)
    for (la, lo) in T.synth.mosaic_locations(LAT0, LON0, deg, deg):
        r.add_terrain(la, lo, T.synth_tile(la, lo, TILE, TILE), *T.synth.tile_transform(la, lo, TILE, TILE))
    r.synchronize()
    clat, clon = LAT0 + deg / 2, LON0 + deg / 2
    arc = winter_arc(clat)
    suns = T.suns([T.sun_direction(clon, clat, az, el) for az, el, _ in arc], [m for _, _, m in arc])
    S = torch.tensor(np.ascontiguousarray(suns["dir"]), dtype=torch.float64, device="cuda")
    S = S / torch.linalg.norm(S, dim=1, keepdim=True)

    def grid(g):
        dlon, dlat = deg / GRID, -deg / GRID
        lon0, lat0 = LON0 + 0.37 * dlon, LAT0 + deg + 0.41 * dlat      # off the DEM lattice
        k = GRID // g
        return lon0, lat0, k * dlon, k * dlat, g, g

    def timed(call, reps):
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

    def new(g, reps):
        lit, shadow = torch.zeros((g, g), dtype=torch.int64, device="cuda"), torch.zeros((g, g), dtype=torch.int64, device="cuda")
        exposure = torch.zeros((g, g), dtype=torch.float32, device="cuda")
        ms = timed(lambda: r.sun_exposure_grid_device(suns, *grid(g), lit.data_ptr(), shadow.data_ptr(), exposure.data_ptr()), reps)
        l, s, e = lit.cpu().numpy().view(np.uint64), shadow.cpu().numpy().view(np.uint64), exposure.cpu().numpy()
        bits = lambda m: int(np.unpackbits(m.reshape(-1).view(np.uint8)).sum())
        pairs = g * g * N_SUNS
        terrain = ~np.isnan(e)
        entry = {"grid": g, "ms": stat(ms), "mpairs_per_s": round(pairs / med(ms) / 1e3, 2),
                 "outputs_sha": hashlib.sha256(l.tobytes() + s.tobytes() + e.tobytes()).hexdigest()[:24]}
        if args.step == "time":
            entry["share_of_pairs"] = {"lit": round(bits(l) / pairs, 6), "shadow": round(bits(s) / pairs, 6), "needed_a_ray": round((bits(l) + bits(s)) / pairs, 6),
                                       "no_terrain": round(float((~terrain).mean()), 6)}
            entry["exposure_minutes"] = {"mean": round(float(e[terrain].mean()), 3), "max": round(float(e[terrain].max()), 3),
                                         "never_lit_share_of_terrain": round(float((l[terrain] == 0).mean()), 6)}
        return entry

    def composed_form(g):
        n = g * g
        lon0, lat0, dlon, dlat, _, _ = grid(g)
        lon_d = lon0 + torch.arange(g, dtype=torch.float64, device="cuda") * dlon
        lat_d = lat0 + torch.arange(g, dtype=torch.float64, device="cuda") * dlat
        lonlat = torch.stack([lon_d[None, :].expand(g, g), lat_d[:, None].expand(g, g)], dim=-1).reshape(n, 2).contiguous()
        lo, la = torch.deg2rad(lonlat[:, 0]), torch.deg2rad(lonlat[:, 1])
        up = torch.stack([torch.cos(la) * torch.cos(lo), torch.cos(la) * torch.sin(lo), torch.sin(la)], dim=1)
        east = torch.stack([-torch.sin(lo), torch.cos(lo), torch.zeros_like(lo)], dim=1)
        north = torch.linalg.cross(up, east)
        rec = torch.zeros((n, 48), dtype=torch.uint8, device="cuda")
        rays = torch.zeros((n, 8), dtype=torch.float64, device="cuda")
        hits = torch.zeros((n, 64), dtype=torch.uint8, device="cuda")
        exposure = torch.zeros((n,), dtype=torch.float64, device="cuda")
        weights = [m for _, _, m in arc]
        cast = [0]

        def composed():
            r.surface_device(lonlat.data_ptr(), rec.data_ptr(), n)
            height = rec[:, 0:8].contiguous().view(torch.float64).reshape(n)
            sa = torch.deg2rad(rec[:, 8:16].contiguous().view(torch.float32).double())
            terrain = rec[:, 16:20].contiguous().view(torch.int32).reshape(n) == T.SURFACE_TERRAIN
            N = torch.sin(sa[:, 0:1]) * (torch.sin(sa[:, 1:2]) * east + torch.cos(sa[:, 1:2]) * north) + torch.cos(sa[:, 0:1]) * up
            Tp = (R0 + height)[:, None] * up
            exposure.zero_()
            cast[0] = 0
            for k in range(N_SUNS):
                ns = N @ S[k]
                idx = torch.nonzero(terrain & (up @ S[k] > 0) & (ns > 0)).reshape(-1)
                m = int(idx.numel())
                if m == 0:
                    continue
                rays[:m, 0:3] = Tp[idx]
                rays[:m, 3:6] = S[k]
                rays[:m, 6] = 1.0e-3
                rays[:m, 7] = 1.0e6
                r.raycast_device(rays.data_ptr(), hits.data_ptr(), m)
                lit = hits[:m, 28:32].contiguous().view(torch.int32).reshape(m) != T.RAY_HIT
                exposure[idx] += torch.where(lit, weights[k] * ns[idx], torch.zeros_like(ns[idx]))
                cast[0] += m

        ms = timed(composed, args.reps)
        return {"grid": g, "ms": stat(ms), "rays_cast": cast[0], "share_of_pairs_cast": round(cast[0] / (n * N_SUNS), 6),
                "exposure_minutes_mean": round(float(exposure.mean()), 3)}

    res = {"suns": {"n": N_SUNS, "declination_deg": DECLINATION_DEG, "lat_deg": clat, "lon_deg": clon, "minutes_per_sample": round(arc[0][2], 3),
                    "elevation_deg": [round(arc[0][1], 2), round(max(el for _, el, _ in arc), 2)]}, "reps": args.reps}
    if args.step == "time":
        res["new"] = new(GRID, args.reps)
        res["new_subgrid"] = new(SUB, args.reps)
    elif args.step == "lane":
        res["lane_per_target_subgrid"] = new(SUB, args.reps)
    else:
        res["composed_subgrid"] = composed_form(SUB)
        res["composed"] = composed_form(GRID)
    print(json.dumps(res))


def run_step(cmd, what, env=None):
    res = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT_S)] + cmd, capture_output=True, text=True, env=env)
    if res.returncode != 0:
        sys.exit(f"{what}: exit status {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-2000:]}")
    return json.loads(res.stdout.strip().split("\n")[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["time", "composed", "lane"])
    ap.add_argument("--lane-lib", help="an experiment build with -DTOPO_SUN_LANE: the subgrid call through it, in a child step")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sun_exposure_c4.json"))
    args = ap.parse_args()
    if args.step:
        return step(args)
    me = os.path.abspath(__file__)
    out = {"what": "tools/sun_exposure_profile.py: the c4 mosaic (100 tiles of 1200 x 1200); a 1024 x 1024 grid of targets over the mosaic under 48 suns along the "
                   "arc of 21 December at the mosaic's centre through topo_sun_exposure_grid_device (a wave looks its 64 targets up once and takes each sun's rays "
                   "one at a time), and the same call on a 256 x 256 subgrid; composed = topo_surface_device + per sun the facing targets' rays built with torch "
                   "on the device + topo_raycast_device, on both grids; lane_per_target = the subgrid call through a -DTOPO_SUN_LANE build; event-timed "
                   "repetitions after a warm-up"}
    out.update(run_step([sys.executable, me, "--step", "time", "--reps", str(args.reps)], "timing step"))
    out.update(run_step([sys.executable, me, "--step", "composed", "--reps", str(args.reps)], "composed step"))
    sub = out["new_subgrid"]
    for new, comp in ((out["new"], out["composed"]), (sub, out["composed_subgrid"])):      # on the same targets
        comp["over_new"] = round(comp["ms"]["median"] / new["ms"]["median"], 2)
        comp["new_faster_by_more_than_the_spread"] = bool(new["ms"]["max"] < comp["ms"]["min"] and comp["ms"]["median"] - new["ms"]["median"] > comp["ms"]["max"] - comp["ms"]["min"])
    if args.lane_lib:
        lane = run_step([sys.executable, me, "--step", "lane", "--reps", str(args.reps)], "lane step", env=dict(os.environ, TOPO_HIP_LIB=os.path.abspath(args.lane_lib)))
        entry = lane["lane_per_target_subgrid"]
        entry["same_bytes"] = entry.pop("outputs_sha") == sub["outputs_sha"]
        entry["over_wave_form"] = round(entry["ms"]["median"] / sub["ms"]["median"], 2)
        out["lane_per_target_subgrid"] = entry
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
