#!/usr/bin/env python3
"""The viewshed's cost on bench.py's workload (default c4: 100 tiles of 1200 x 1200, one 8-sector 16384 x 4096 panorama per
frame): frames with accumulation off, then on, timed with events around each frame; what k_viewshed did (terrain keys read,
mask-word updates after combining lanes, atomics issued) and the cells it marked.  Prints one JSON line.  Meant to run under
`rocprofv3 --kernel-trace --stats -- python tools/viewshed_profile.py` for the per-kernel times (profiles/README.md)."""
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
    ap.add_argument("--frames", type=int, default=10)
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

    def frame():
        r.render_views_device(views, SW, PH, rgba.data_ptr(), PH * SW * 4, SW * 4, depth.data_ptr(), PH * SW * 4, SW * 4)

    def timed(n):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for a, b in ev:
            a.record()
            frame()
            b.record()
        torch.cuda.synchronize()
        ms = sorted(a.elapsed_time(b) for a, b in ev)
        return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4)}

    for _ in range(3):
        frame()
    off = timed(args.frames)
    r.viewshed_enable(True)
    r.viewshed_reset()
    frame()                                    # the first frame: every visible cell is new
    r.synchronize()
    first = r.debug_viewshed_stats()
    marked = sum(int(r.viewshed(*loc).sum()) for loc in locs)
    r.viewshed_reset()
    on = timed(args.frames)                     # the same panorama again and again: the words are set after the first
    again = r.debug_viewshed_stats()
    tiles_seen = sum(1 for loc in locs if r.viewshed(*loc).any())
    print(json.dumps({"workload": args.workload, "pixels": N_SECTORS * SW * PH,
                      "accumulation_off": off, "accumulation_on": on, "first_frame": first, "marked_cells": marked,
                      "tiles_with_marks": tiles_seen, "frames_on": args.frames, "repeated_frames": again}))


if __name__ == "__main__":
    main()
