#!/usr/bin/env python3
"""The unwrap's cost on bench.py's workload (default c4: 100 tiles of 1200 x 1200, one 8-sector 16384 x 4096 panorama): one panorama
frame, then behind it, again and again and each timed with events, topo_unwrap_device of the strip into one 16384 x 4096
equirectangular image (elevation +-37 degrees: inside every sector's vertical field) in four forms -- nearest colour; nearest colour +
depth; nearest colour + depth + source map; bilinear colour + depth -- each beside two yardsticks of the same run: its byte floor
(what it must read and write, from the shapes, over 5 TB/s) and a plain device-to-device copy that moves the same number of bytes
(half of them read, half written).  Checks the nearest outputs against a gather through the source map.  Prints one JSON line.  Meant
to run under `rocprofv3 --kernel-trace --stats -- python tools/unwrap_profile.py` for the kernel's own times (profiles/README.md)."""
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
    ap.add_argument("--repetitions", type=int, default=10, help="timed repetitions of each form")
    ap.add_argument("--elevation", type=float, default=37.0, help="the window is +- this many degrees")
    args = ap.parse_args()
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
    r.render_panorama(None, eye, 0.0, SW, PH, vlon, vlat, rgba.data_ptr(), depth.data_ptr())
    r.synchronize()
    out_rgba = torch.zeros((PH, PW, 4), dtype=torch.uint8, device="cuda")
    out_depth = torch.zeros((PH, PW), dtype=torch.float32, device="cuda")
    out_src = torch.zeros((PH, PW), dtype=torch.int32, device="cuda")
    pixels = PW * PH

    def unwrap(filt, want):
        p = T.unwrap_params(PW, PH, args.elevation, -args.elevation, filter=filt)
        r.unwrap_device(p, views, SW, PH, rgba_src_ptr=rgba.data_ptr() if "r" in want else 0, depth_src_ptr=depth.data_ptr() if "d" in want else 0,
                        rgba_out_ptr=out_rgba.data_ptr() if "r" in want else 0, depth_out_ptr=out_depth.data_ptr() if "d" in want else 0,
                        src_out_ptr=out_src.data_ptr() if "s" in want else 0)

    def timed(call):
        call()      # (the first call of a parameter set builds and uploads the tables)
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.repetitions)]
        for a, b in ev:
            a.record()
            call()
            b.record()
        torch.cuda.synchronize()
        ms = sorted(a.elapsed_time(b) for a, b in ev)
        return {"median": round(ms[len(ms) // 2], 4), "min": round(ms[0], 4), "max": round(ms[-1], 4)}

    forms = {"nearest_colour": (T.UNWRAP_NEAREST, "r", 8), "nearest_colour_depth": (T.UNWRAP_NEAREST, "rd", 16),
             "nearest_colour_depth_source": (T.UNWRAP_NEAREST, "rds", 20), "bilinear_colour_depth": (T.UNWRAP_BILINEAR, "rd", 16)}
    res = {}
    for name, (filt, want, bpp) in forms.items():
        floor = bpp * pixels      # every output texel written once, as many source texels read once
        a, b = (torch.empty(floor // 2, dtype=torch.uint8, device="cuda") for _ in range(2))
        copy_ms = timed(lambda: b.copy_(a))
        ms = timed(lambda: unwrap(filt, want))
        res[name] = {"event_ms": ms, "floor_bytes": floor, "floor_ms_at_5_TBps": round(floor / 5e12 * 1e3, 4), "copy_same_bytes_event_ms": copy_ms,
                     "over_floor": round(ms["median"] / (floor / 5e12 * 1e3), 2), "over_copy": round(ms["median"] / copy_ms["median"], 2)}
        del a, b
    unwrap(T.UNWRAP_NEAREST, "rds")
    torch.cuda.synchronize()
    src = out_src.long()
    covered = src >= 0
    flat = src.clamp(min=0).reshape(-1)
    ok_rgba = torch.equal(out_rgba.reshape(-1, 4)[covered.reshape(-1)], rgba.reshape(-1, 4)[flat][covered.reshape(-1)])
    ok_depth = torch.equal(out_depth.reshape(-1)[covered.reshape(-1)].view(torch.int32), depth.reshape(-1)[flat][covered.reshape(-1)].view(torch.int32))
    assert ok_rgba and ok_depth
    print(json.dumps({"workload": args.workload, "views": N_SECTORS, "src_w": SW, "src_h": PH, "out_w": PW, "out_h": PH, "elevation_deg": args.elevation,
                      "repetitions": args.repetitions, "pixels": pixels, "covered_pixels": int(covered.sum().item()),
                      "terrain_pixels": int((out_depth < 1).sum().item()), "forms": res}))


if __name__ == "__main__":
    main()
