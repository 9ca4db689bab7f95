#!/usr/bin/env python3
"""The ground queries' cost on bench.py's workload (default c4: 100 tiles of 1200 x 1200, one 8-sector 16384 x 4096 panorama): one
panorama frame, then behind it, again and again and each timed with events, topo_ground_device over the panorama's horizon pixels
(one per column: 16384 queries) and topo_ground_map_device over all 8 sectors; k_resolve's duration of the same run beside them, the
map against its HBM floor of 24 B per pixel (8 B key in, 16 B out), what the queries found, and that the map equals the list at the
queried pixels.  Prints one JSON line.  Meant to run under `rocprofv3 --kernel-trace --stats -- python tools/ground_profile.py`
for the kernels' own times (profiles/README.md)."""
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
    ap.add_argument("--queries", type=int, default=10, help="timed repetitions of each query")
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
    dense = torch.empty((N_SECTORS, PH, SW, 4), dtype=torch.float32, device="cuda")
    r.set_timing_slots(("resolve",), total=False)
    for _ in range(3):
        r.render_views_device(views, SW, PH, rgba.data_ptr(), PH * SW * 4, SW * 4, depth.data_ptr(), PH * SW * 4, SW * 4)
    r.synchronize()
    resolve_ms = r.timings()["resolve"]
    hz = r.horizon()
    v, x = np.nonzero(hz["row"] >= 0)
    q = T.ground_queries(np.stack([v, x, hz["row"][v, x]], axis=-1))
    q_dev = torch.from_numpy(q.view(np.uint32).reshape(-1, 4).copy()).cuda()
    out = torch.empty((len(q) * 64,), dtype=torch.uint8, device="cuda")
    r.ground_device(q_dev.data_ptr(), out.data_ptr(), len(q))      # (the first query uploads the submission's views)
    r.ground_map_device(dense.data_ptr())
    torch.cuda.synchronize()

    def timed(call):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.queries)]
        for a, b in ev:
            a.record()
            call()
            b.record()
        torch.cuda.synchronize()
        ms = sorted(a.elapsed_time(b) for a, b in ev)
        return {"median": round(ms[len(ms) // 2], 4), "min": round(ms[0], 4), "max": round(ms[-1], 4)}

    list_ms = timed(lambda: r.ground_device(q_dev.data_ptr(), out.data_ptr(), len(q)))
    map_ms = timed(lambda: r.ground_map_device(dense.data_ptr()))
    rec = out.cpu().numpy().view(T.GROUND_DTYPE)
    assert np.array_equal(rec.view(np.uint8), r.ground(q).view(np.uint8))
    at = dense[torch.from_numpy(v), torch.from_numpy(hz["row"][v, x].astype(np.int64)), torch.from_numpy(x)].cpu().numpy()
    t = rec["kind"] == 1
    want = np.stack([rec["lon_deg"].astype(np.float32), rec["lat_deg"].astype(np.float32), rec["height_m"], rec["range_m"]], axis=-1)
    assert np.array_equal(at[t].view(np.uint32), want[t].view(np.uint32)) and np.isnan(at[~t]).all()
    assert np.array_equal(rec["depth"], hz["depth"][v, x])
    # what the f64 range corrects: topo_dist_from_depth of the same pixels' f32 depth
    d = np.array([float(rec["range_m"][i]) - T.dist_from_depth(float(rec["depth"][i])) for i in np.nonzero(t)[0][::64]])
    terrain_px = int(torch.isfinite(dense[..., 0]).sum().item())
    pixels = N_SECTORS * PH * SW
    floor_bytes = 24 * pixels
    print(json.dumps({"workload": args.workload, "views": N_SECTORS, "width": SW, "height": PH, "repetitions": args.queries,
                      "list_queries": int(len(q)), "list_event_ms": list_ms, "map_event_ms": map_ms, "resolve_event_ms": round(resolve_ms, 4),
                      "map_pixels": pixels, "map_terrain_pixels": terrain_px, "map_floor_bytes": floor_bytes,
                      "map_floor_TBps_at_median": round(floor_bytes / (map_ms["median"] * 1e-3) / 1e12, 3),
                      "list_kinds": {str(k): int((rec["kind"] == k).sum()) for k in np.unique(rec["kind"])},
                      "skyline_range_m": [round(float(rec["range_m"][t].min()), 1), round(float(rec["range_m"][t].max()), 1)] if t.any() else None,
                      "skyline_height_m": [round(float(rec["height_m"][t].min()), 1), round(float(rec["height_m"][t].max()), 1)] if t.any() else None,
                      "range_minus_dist_from_depth_m": [round(float(d.min()), 1), round(float(d.max()), 1)] if len(d) else None}))


if __name__ == "__main__":
    main()
