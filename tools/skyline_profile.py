#!/usr/bin/env python3
"""The skyline queries' cost on the c4 mosaic (100 tiles of 1200 x 1200): 64 observers on an 8 x 8 grid over the mosaic's inner 8 x 8
degrees, 3600 azimuths each (0.1 degrees apart), 10 m <= s <= 400 km, from 2 m and from 1000 m above the terrain.  For each height
  (a) new        topo_skyline_device, both outputs;
  (b) bisection  what a caller could do before: the same skylines by 24 steps of bisection of the elevation in [-90, 90] degrees over
                 topo_raycast_device -- per step one ray an azimuth from O along cos(el) h + sin(el) up with t limited to the same s
                 interval, a hit moving the lower bound and a miss the upper; the rays are built with torch on the device (f64), the
                 observers' points from topo_surface_read once, outside the timing.  It needs 24 full traversals an azimuth and never
                 names the ridge;
and the difference between the two elevations, signed (bisection - skyline).  The bisection's lower bound is a ray that HIT terrain
inside the s interval: where it lies more than the bisection's resolution ABOVE the reported skyline there is terrain over the
skyline -- the kernel dropped a crossing, or a triangle straddles a range limit -- so those azimuths are counted, the lower-bound ray
is cast once more for the s of its hit, and the tool fails if any such hit lies more than 200 m (two cells) inside the limits.  A
bisection BELOW the skyline is only its own assumption ("hit below, miss above") failing.  (a) is event-timed over a few repetitions after a warm-up call, (b) once after one
warm-up step.  The registers of k_skyline are read from the code object (tools/kernel_resources.py) where hipcc is at hand.

Without --step the tool runs the measurement in a child under its own `timeout` and writes --out (default profiles/skyline_c4.json)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEP_LIMIT_S = 420
N_SIDE, N_AZ, DAZ = 8, 3600, 0.1
MIN_RANGE_M, MAX_RANGE_M = 10.0, 4.0e5
HEIGHTS_M = (2.0, 1000.0)
BISECTION_STEPS = 24
LIMIT_MARGIN_M = 200.0


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
    g = 1.0 + (deg - 2.0) * (np.arange(N_SIDE) + 0.37) / N_SIDE      # off the DEM lattice and the tile borders
    lon, lat = (LON0 + g)[None, :].repeat(N_SIDE, 0).reshape(-1), (LAT0 + g)[:, None].repeat(N_SIDE, 1).reshape(-1)
    n_obs, n = N_SIDE * N_SIDE, N_SIDE * N_SIDE * N_AZ
    az0 = 0.37 * DAZ
    el_dev = torch.zeros((n_obs, N_AZ), dtype=torch.float32, device="cuda")
    rec_dev = torch.zeros((n * 64,), dtype=torch.uint8, device="cuda")
    base = r.surface(np.stack([lon, lat], axis=1))
    assert (base["kind"] == T.SURFACE_TERRAIN).all()

    def timed(call, reps):
        call()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for s, e in ev:
            s.record()
            call()
            e.record()
        torch.cuda.synchronize()
        return sorted(s.elapsed_time(e) for s, e in ev)

    stat = lambda v: {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}
    res = {}
    for height in HEIGHTS_M:
        obs = T.observers(lon, lat, height)
        ms_new = timed(lambda: r.skyline_device(obs, az0, DAZ, N_AZ, el_dev.data_ptr(), rec_dev.data_ptr(), MIN_RANGE_M, MAX_RANGE_M), args.reps)
        el_new = el_dev.cpu().numpy().astype(np.float64)
        rec = rec_dev.cpu().numpy().view(T.SKYLINE_DTYPE).reshape(n_obs, N_AZ)
        # (b): the frame at every observer and the azimuths' horizontal directions, f64 on the device
        O = torch.tensor(np.stack([T.ecef_from_lonlat(a, b, float(c) + height) for a, b, c in zip(lon, lat, base["height_m"])]), dtype=torch.float64, device="cuda")
        up = O / torch.linalg.norm(O, dim=1, keepdim=True)
        east = torch.stack([-up[:, 1], up[:, 0], torch.zeros_like(up[:, 0])], dim=1)
        east = east / torch.linalg.norm(east, dim=1, keepdim=True)
        north = torch.linalg.cross(up, east)
        az = torch.deg2rad(az0 + torch.arange(N_AZ, dtype=torch.float64, device="cuda") * DAZ)
        Hd = torch.cos(az)[None, :, None] * north[:, None, :] + torch.sin(az)[None, :, None] * east[:, None, :]      # (observers, azimuths, 3)
        rays = torch.zeros((n, 8), dtype=torch.float64, device="cuda")
        rays[:, 0:3] = O[:, None, :].expand(n_obs, N_AZ, 3).reshape(n, 3)
        hits = torch.zeros((n, 16), dtype=torch.int32, device="cuda")
        lo_hi = [None, None]

        def one(el):
            c, s = torch.cos(el), torch.sin(el)
            rays[:, 3:6] = (c[..., None] * Hd + s[..., None] * up[:, None, :]).reshape(n, 3)
            rays[:, 6] = (MIN_RANGE_M / c).reshape(n)
            rays[:, 7] = (MAX_RANGE_M / c).reshape(n)
            r.raycast_device(rays.data_ptr(), hits.data_ptr(), n)
            return (hits[:, 7] == T.RAY_HIT).reshape(n_obs, N_AZ)      # kind: the eighth 32-bit word of topo_ray_hit

        def bisect():
            lo = torch.full((n_obs, N_AZ), -0.5 * np.pi + 1e-9, dtype=torch.float64, device="cuda")
            hi = -lo
            for _ in range(BISECTION_STEPS):
                mid = 0.5 * (lo + hi)
                hit = one(mid)
                lo, hi = torch.where(hit, mid, lo), torch.where(hit, hi, mid)
            lo_hi[0], lo_hi[1] = lo, hi

        one(torch.zeros((n_obs, N_AZ), dtype=torch.float64, device="cuda"))      # warm-up
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        bisect()
        e.record()
        torch.cuda.synchronize()
        ms_bis = s.elapsed_time(e)
        el_new = rec["elevation_deg"]      # (f64)
        el_bis = np.degrees(0.5 * (lo_hi[0] + lo_hi[1]).cpu().numpy())
        lo_deg = np.degrees(lo_hi[0].cpu().numpy())
        found = (rec["kind"] == T.SKY_TERRAIN) & (lo_hi[0].cpu().numpy() > -0.5 * np.pi + 1e-6)
        signed = (el_bis - el_new)[found]
        diff = np.abs(signed)
        resolution = 180.0 / 2 ** BISECTION_STEPS
        # terrain over the skyline: the lower bound -- a ray that hit -- above it; where does that ray hit?
        hit_lo = one(lo_hi[0]).cpu().numpy()
        s_hit = (hits.view(torch.float64)[:, 0].reshape(n_obs, N_AZ) * torch.cos(lo_hi[0])).cpu().numpy()
        over = found & hit_lo & (lo_deg - el_new > resolution)
        inside = over & (s_hit > MIN_RANGE_M + LIMIT_MARGIN_M) & (s_hit < MAX_RANGE_M - LIMIT_MARGIN_M)
        med = stat(ms_new)["median"]
        res[f"observer_{int(height)}m"] = {
            "observer_height_above_terrain_m": height, "ms": stat(ms_new), "kazimuths_per_s": round(n / med, 1),
            "share_terrain": round(float((rec["kind"] == T.SKY_TERRAIN).mean()), 6),
            "elevation_deg": {"min": round(float(np.nanmin(el_new)), 4), "median": round(float(np.nanmedian(el_new)), 4), "max": round(float(np.nanmax(el_new)), 4)},
            "range_m_median": round(float(np.median(rec["range_m"][rec["kind"] == T.SKY_TERRAIN])), 1),
            "bisection": {"steps": BISECTION_STEPS, "ms": round(ms_bis, 1), "over_new": round(ms_bis / med, 1), "azimuths_compared": int(found.sum()),
                          "elevation_difference_deg": {"median": float(f"{np.median(diff):.3e}"), "p99": float(f"{np.quantile(diff, 0.99):.3e}"), "max": float(f"{diff.max():.3e}")},
                          "signed_difference_deg": {"min": float(f"{signed.min():.3e}"), "max": float(f"{signed.max():.3e}"),
                                                    "below_skyline_by_more_than_resolution": int((signed < -resolution).sum())},
                          "lower_bound_over_skyline_by_more_than_resolution": {"azimuths": int(over.sum()), "hit_more_than_200m_inside_the_limits": int(inside.sum())},
                          "bisection_resolution_deg": float(f"{resolution:.3e}")}}
    print(json.dumps({"shape": {"observers": n_obs, "azimuths": N_AZ, "daz_deg": DAZ, "min_range_m": MIN_RANGE_M, "max_range_m": MAX_RANGE_M, "reps": args.reps}, **res}))


def resources():
    """k_skyline's row of tools/kernel_resources.py, or None where hipcc is not at hand."""
    try:
        text = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py")], capture_output=True, text=True, timeout=900).stdout
    except (OSError, subprocess.SubprocessError):
        return None
    for line in text.split("\n"):
        if line.startswith("k_skyline"):
            w = line.split()
            return {"vgpr": int(w[2]), "sgpr": int(w[4]), "lds_bytes": int(w[6]), "scratch_bytes": int(w[8]), "vgpr_spills": int(w[10][1:]), "sgpr_spills_to_vgpr_lanes": int(w[11][1:])}
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["time"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-resources", action="store_true", help="leave out the compile that reads k_skyline's registers")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "skyline_c4.json"))
    args = ap.parse_args()
    if args.step:
        return step(args)
    out = {"what": "tools/skyline_profile.py: the c4 mosaic (100 tiles of 1200 x 1200); 64 observers x 3600 azimuths, 10 m <= s <= 400 km, from 2 m and 1000 m above "
                   "the terrain through topo_skyline_device (a wave per observer and azimuth), bisection = the same skylines by 24 steps of bisection of the "
                   "elevation over topo_raycast_device with rays built with torch on the device; (a) event-timed repetitions after a warm-up, (b) timed once"}
    res = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--step", "time", "--reps", str(args.reps)],
                         capture_output=True, text=True)
    if res.returncode != 0:
        sys.exit(f"timing step: exit status {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-2000:]}")
    out.update(json.loads(res.stdout.strip().split("\n")[-1]))
    if not args.no_resources:
        out["k_skyline_resources"] = resources()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    over = {k: v["bisection"]["lower_bound_over_skyline_by_more_than_resolution"]["hit_more_than_200m_inside_the_limits"] for k, v in out.items() if k.startswith("observer_")}
    if any(over.values()):
        sys.exit(f"terrain over the reported skyline, away from the range limits: {over}")


if __name__ == "__main__":
    main()
