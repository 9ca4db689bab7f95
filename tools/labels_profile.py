#!/usr/bin/env python3
"""The peak labels' cost on the c4 mosaic (100 tiles of 1200 x 1200): 5000 peaks at seeded DEM posts, lifted 5 m, label widths in
[30, 120] px, the reference's 8 rows of 20 px.
  (a) panorama   one 8 x 2048 x 4096 panorama (bench.py's c4 viewpoint, topo_render_panorama with depth): one image of 16384 columns;
  (b) batch      64 viewpoints of the c5 shape (bench.py's first 64, 8 x 512 x 1024 each) in one topo_render_batch buffer: 512 views,
                 64 images of 4096 columns.
For each:
  new        topo_labels_device, views_per_image = 8: one launch, labels, counts and states stay on the device;
  composed   what the parent commit's API allows on the same inputs: per view topo_visible_peaks_device, one device-to-host copy of
             the visibility bytes and one of the pixels, the host-side merge to strip columns (the first view that shows a peak), and
             topo_label_layout on the host -- itself new, standing for what a caller would have written.
Both are timed wall-clock from a drained device to a drained device (the composition ends on the host), after a warm-up call, and
the new call with events as well; the tool fails if the two disagree on a label.

Without --step the tool drives its child runs, each under its own `timeout`, and stops at the first that fails; it writes all of it,
with k_labels' registers, LDS and scratch from tools/kernel_resources.py, into --out (default profiles/labels_c4.json)."""
import argparse
import json
import math
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEP_LIMIT_S = 420
N_PEAKS, PEAK_SEED, LIFT_M = 5000, 20261019, 5.0
ROW_HEIGHT, MAX_ROWS = 20.0, 8
BATCH_VIEWPOINTS = 64


def step(args):
    import numpy as np
    import torch
    import topo_renderer_amd as T
    import bench
    from bench import LAT0, LON0, TILE, WORKLOADS, N_SECTORS
    deg = WORKLOADS["c4"][0]
    PW, PH = WORKLOADS["c4" if args.step == "panorama" else "c5"][1:]
    SW = PW // N_SECTORS
    r = T.TerrainRenderer(SW, PH)
    r.set_stream(torch.cuda.current_stream().cuda_stream)
    tiles = {}
    for (la, lo) in T.synth.mosaic_locations(LAT0, LON0, deg, deg):
        tiles[(la, lo)] = T.synth_tile(la, lo, TILE, TILE)
        r.add_terrain(la, lo, tiles[(la, lo)], *T.synth.tile_transform(la, lo, TILE, TILE))
    r.synchronize()

    # peaks at DEM posts (row 0 = north), lifted; widths
    rng = np.random.default_rng(PEAK_SEED)
    peaks = np.zeros((N_PEAKS, 3), np.float32)
    for i in range(N_PEAKS):
        la, lo = LAT0 + int(rng.integers(0, deg)), LON0 + int(rng.integers(0, deg))
        row, col = int(rng.integers(0, TILE)), int(rng.integers(0, TILE))
        peaks[i] = T.geometry_transform(float(tiles[(la, lo)][row, col]) + LIFT_M, lo + col / TILE, la + 1 - row / TILE)
    widths = rng.uniform(30.0, 120.0, N_PEAKS).astype(np.float32)
    d_peaks, d_widths = torch.from_numpy(peaks).cuda(), torch.from_numpy(widths).cuda()

    if args.step == "panorama":
        vlat, vlon = LAT0 + deg / 2 + 0.123, LON0 + deg / 2 + 0.217
        key = (int(math.floor(vlat)), int(math.floor(vlon)))
        eye = T.geometry_transform(T.synth.height_at(tiles[key], key[0], key[1], vlon, vlat) + 50.0, vlon, vlat)
        views = T.panorama_uniforms(eye, 0.0, SW, PH, vlon, vlat, 0)
        rgba = torch.empty((N_SECTORS, PH, SW, 4), dtype=torch.uint8, device="cuda")
        depth = torch.empty((N_SECTORS, PH, SW), dtype=torch.float32, device="cuda")
        r.render_panorama(None, eye, 0.0, SW, PH, vlon, vlat, rgba.data_ptr(), depth.data_ptr(), 0)
        r.join()
    else:
        state, eyes, yaws, suns, views = 0x5EED0005, [], [], [], []
        for _ in range(BATCH_VIEWPOINTS):      # bench.py's c5 viewpoints, the first 64
            u = []
            for _k in range(3):
                state, z = bench._splitmix64(state)
                u.append(z / 2.0 ** 64)
            lat, lon, yaw = LAT0 + 1.0 + 8.0 * u[0], LON0 + 1.0 + 8.0 * u[1], 2.0 * math.pi * u[2]
            key = (int(math.floor(lat)), int(math.floor(lon)))
            eye = T.geometry_transform(T.synth.height_at(tiles[key], key[0], key[1], lon, lat) + 50.0, lon, lat)
            eyes.append(eye), yaws.append(yaw), suns.append((lon, lat))
            views += T.panorama_uniforms(eye, np.float32(yaw), SW, PH, np.float32(lon), np.float32(lat), 0)
        rgba = torch.empty((BATCH_VIEWPOINTS, N_SECTORS, PH, SW, 4), dtype=torch.uint8, device="cuda")
        depth = torch.empty((BATCH_VIEWPOINTS, N_SECTORS, PH, SW), dtype=torch.float32, device="cuda")
        r.render_batch(np.stack(eyes), np.array(yaws, np.float32), np.array(suns, np.float32), SW, PH, rgba.data_ptr(), depth.data_ptr(), 0)
        r.join()
    torch.cuda.synchronize()
    del rgba
    n_views = len(views)
    images = n_views // N_SECTORS
    us = np.ascontiguousarray(np.stack([np.ascontiguousarray(u).view(np.uint8).reshape(160) for u in views]))
    params = T.label_params(ROW_HEIGHT, MAX_ROWS, N_SECTORS, N_PEAKS)
    d_labels = torch.zeros((images, N_PEAKS, 8), dtype=torch.int32, device="cuda")
    d_counts = torch.zeros(images, dtype=torch.int32, device="cuda")
    d_state = torch.zeros((images, N_PEAKS), dtype=torch.uint8, device="cuda")

    def new():
        r.labels_device(params, us, SW, PH, depth.data_ptr(), N_PEAKS, d_peaks.data_ptr(), d_widths.data_ptr(), d_labels.data_ptr(), d_counts.data_ptr(), d_state.data_ptr())

    d_vis = torch.zeros((n_views, N_PEAKS), dtype=torch.uint8, device="cuda")
    d_xy = torch.zeros((n_views, N_PEAKS, 2), dtype=torch.int32, device="cuda")
    composed_out = [None]

    def composed():
        for v in range(n_views):
            r.visible_peaks_device(views[v], SW, PH, depth[v // N_SECTORS, v % N_SECTORS].data_ptr() if depth.dim() == 4 else depth[v].data_ptr(), 4 * SW, N_PEAKS,
                                   d_peaks.data_ptr(), d_vis[v].data_ptr(), d_xy[v].data_ptr())
        vis = d_vis.cpu().numpy().reshape(images, N_SECTORS, N_PEAKS) != 0
        xy = d_xy.cpu().numpy().view(np.uint32).reshape(images, N_SECTORS, N_PEAKS, 2)
        out = []
        for i in range(images):
            first = vis[i].argmax(axis=0)      # the first view that shows the peak
            idx = np.flatnonzero(vis[i].any(axis=0))
            x = first[idx].astype(np.uint32) * SW + xy[i, first[idx], idx, 0]
            rows, recs = T.label_layout(x, widths[idx], N_SECTORS * SW, ROW_HEIGHT, MAX_ROWS)
            out.append((idx, first[idx], xy[i, first[idx], idx, 1], rows, recs))
        composed_out[0] = out

    def wall(call, reps):
        call()      # warm-up
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return sorted(ms)

    def events(call, reps):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for s, e in ev:
            s.record()
            call()
            e.record()
        torch.cuda.synchronize()
        return sorted(s.elapsed_time(e) for s, e in ev)

    stat = lambda v: {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}
    new_wall, new_ev, comp_wall = wall(new, args.reps), events(new, args.reps), wall(composed, args.reps)
    counts, labels = d_counts.cpu().numpy().view(np.uint32), d_labels.cpu().numpy().view(np.uint8).reshape(images, N_PEAKS, 32).copy().view(T.LABEL_DTYPE).reshape(images, N_PEAKS)
    state = d_state.cpu().numpy()
    for i, (idx, first, ys, rows, recs) in enumerate(composed_out[0]):      # the two must agree, label for label
        want = recs.copy()
        placed = rows >= 0
        want["peak"], want["view"], want["peak_y"] = idx[placed], first[placed], ys[placed].astype(np.float32)
        if int(counts[i]) != len(want) or labels[i, :len(want)].tobytes() != want.tobytes():
            sys.exit(f"image {i}: the composition and topo_labels_device disagree ({len(want)} vs {int(counts[i])} labels)")
    res = {"views": n_views, "images": images, "view_size": [SW, PH], "image_columns": N_SECTORS * SW, "peaks": N_PEAKS, "reps": args.reps,
           "labels_placed": int(counts.sum()), "labels_per_image": {"min": int(counts.min()), "max": int(counts.max())},
           "peaks_visible": int((state != 0).sum()), "peaks_without_a_row": int((state == T.LABEL_NO_ROW).sum()),
           "new_ms_wall": stat(new_wall), "new_ms_events": stat(new_ev), "composed_ms_wall": stat(comp_wall),
           "composed_over_new": round(comp_wall[len(comp_wall) // 2] / new_wall[len(new_wall) // 2], 2),
           "new_faster_by_more_than_the_spread": bool(new_wall[-1] < comp_wall[0]), "same_labels": True}
    print(json.dumps({args.step: res}))


def run_step(cmd, what):
    res = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT_S)] + cmd, capture_output=True, text=True)
    if res.returncode != 0:
        sys.exit(f"{what}: exit status {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-2000:]}")
    return json.loads(res.stdout.strip().split("\n")[-1])


def resources():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py")], capture_output=True, text=True).stdout
    m = re.search(r"k_labels\S*\s+vgpr\s+(\d+)\s+sgpr\s+(\d+)\s+lds\s+(\d+)\s+scratch\s+(\d+)", out)
    return {"vgpr": int(m.group(1)), "sgpr": int(m.group(2)), "static_lds": int(m.group(3)), "scratch": int(m.group(4))} if m else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["panorama", "batch"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-resources", action="store_true")
    ap.add_argument("--resources-only", action="store_true", help="add k_labels' resources to an existing --out (needs no GPU)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "labels_c4.json"))
    args = ap.parse_args()
    if args.step:
        return step(args)
    if args.resources_only:
        with open(args.out) as f:
            out = json.load(f)
        out["k_labels"] = resources()
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        return print(json.dumps(out["k_labels"]))
    me = os.path.abspath(__file__)
    out = {"what": "tools/labels_profile.py: the c4 mosaic (100 tiles of 1200 x 1200), 5000 peaks at seeded DEM posts lifted 5 m, widths in [30, 120], 8 rows of 20 px; "
                   "panorama = one 8 x 2048 x 4096 panorama as one image, batch = 64 viewpoints of 8 x 512 x 1024 in one buffer as 64 images; new = "
                   "topo_labels_device (one launch, a wave per image); composed = per view topo_visible_peaks_device + one device-to-host copy of the bytes and "
                   "one of the pixels + the host merge to strip columns + topo_label_layout on the host; wall-clock from a drained device to a drained device "
                   "after a warm-up call, the new call with events as well"}
    out.update(run_step([sys.executable, me, "--step", "panorama", "--reps", str(args.reps)], "panorama step"))
    out.update(run_step([sys.executable, me, "--step", "batch", "--reps", str(args.reps)], "batch step"))
    if not args.no_resources:
        out["k_labels"] = resources()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
