#!/usr/bin/env python3
"""The horizon query's cost on bench.py's workload (default c4: 100 tiles of 1200 x 1200, one 8-sector 16384 x 4096 panorama):
one panorama frame, then topo_horizon_device behind it again and again, each query timed with events; what the query found (terrain
columns, row range, tiles on the skyline) and the skyline's elevation range.  Prints one JSON line.  Meant to run under
`rocprofv3 --kernel-trace --stats -- python tools/horizon_profile.py` for k_horizon's kernel time (profiles/README.md)."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c4")
    ap.add_argument("--queries", type=int, default=20)
    args = ap.parse_args()
    import numpy as np
    import torch
    import topo_renderer_amd as T
    from bench import LAT0, LON0, N_SECTORS, TILE, WORKLOADS
    deg, PW, PH = WORKLOADS[args.workload]
    SW = PW // N_SECTORS
    locs = T.synth.mosaic_locations(LAT0, LON0, deg, deg)
    r = T.TerrainRenderer(SW, PH)
    r.set_stream(torch.cuda.current_stream().cuda_stream)
    vlat, vlon = LAT0 + deg / 2 + 0.123, LON0 + deg / 2 + 0.217
    ground = None
    for (la, lo) in locs:
        h = T.synth_tile(la, lo, TILE, TILE)
        if la == int(math.floor(vlat)) and lo == int(math.floor(vlon)):
            ground = T.synth.height_at(h, la, lo, vlon, vlat)
        r.add_terrain(la, lo, h, *T.synth.tile_transform(la, lo, TILE, TILE))
    r.synchronize()
    eye = T.geometry_transform(ground + 50.0, vlon, vlat)
    views = T.panorama_uniforms(eye, 0.0, SW, PH, vlon, vlat, 0)
    rgba = torch.empty((N_SECTORS, PH, SW, 4), dtype=torch.uint8, device="cuda")
    depth = torch.empty((N_SECTORS, PH, SW), dtype=torch.float32, device="cuda")
    out = torch.empty((N_SECTORS * SW * 32,), dtype=torch.uint8, device="cuda")
    for _ in range(3):
        r.render_views_device(views, SW, PH, rgba.data_ptr(), PH * SW * 4, SW * 4, depth.data_ptr(), PH * SW * 4, SW * 4)
    r.synchronize()
    r.horizon_device(out.data_ptr())      # (the first query builds the rank -> tile table)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.queries)]
    for a, b in ev:
        a.record()
        r.horizon_device(out.data_ptr())
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    hz = r.horizon()
    dev = out.cpu().numpy().view(T.HORIZON_DTYPE).reshape(N_SECTORS, SW)
    assert np.array_equal(dev, hz)
    rows = hz["row"]
    terrain = rows >= 0
    xy = np.column_stack([np.arange(SW) + 0.5, np.zeros(SW)])
    el = []
    for s in range(N_SECTORS):
        xy[:, 1] = np.maximum(rows[s], 0) + 0.5
        el.append(T.pixel_angles(views[s], SW, PH, xy)[terrain[s], 1])
    el = np.concatenate(el) if len(el) else np.zeros(0)
    print(json.dumps({"workload": args.workload, "views": N_SECTORS, "width": SW, "height": PH, "queries": args.queries,
                      "query_event_ms": {"median": round(ms[len(ms) // 2], 4), "min": round(ms[0], 4), "max": round(ms[-1], 4)},
                      "terrain_columns": int(terrain.sum()), "sky_columns": int((rows == -1).sum()),
                      "row_min": int(rows[terrain].min()) if terrain.any() else -1, "row_max": int(rows[terrain].max()) if terrain.any() else -1,
                      "skyline_tiles": len({(int(a), int(b)) for a, b in zip(hz["lat_deg"][terrain], hz["lon_deg"][terrain])}),
                      "elevation_deg": [round(float(el.min()), 3), round(float(el.max()), 3)] if len(el) else None}))


if __name__ == "__main__":
    main()
