#!/usr/bin/env python3
"""The map view's cost on the c4 mosaic (100 tiles of 1200 x 1200), all layers on, for a 1024 x 1024 and a 256 x 256 map over the
mosaic's 10 x 10 degrees, next to what exists without it:
  map          topo_map_device, RGBA and flags;
  (a) grid     topo_surface_grid_device on the same grid: less work per pixel (heights only), but every lane walks every tile;
  (b) compose  what a caller can do today: the grid's points through topo_surface_device, the 48-byte records read back, and the
               shading, the contours and the mask lookup in numpy on the host (the tiles' normals and masks already on the host:
               fetching them is not counted).  Wall-clock time, since most of it is host work.
map and (a) are timed with events; each figure is the median of --reps repetitions (at least 15) after a warm-up, with the spread.

Without --step the tool drives child runs, each under its own `timeout`, and stops at the first that fails:
  1. `--step time`     the three timings per grid with the product library;
  2. `--step variant`  the map timings alone with each ablation build found in exp/ (tools/exp_build.sh NAME FLAGS, selected with
                       TOPO_HIP_LIB): map_recompute (-DTOPO_MAP_RECOMPUTE: three lookups per pixel, no halo and no exchange),
                       map_alltiles (-DTOPO_MAP_ALL_TILES: no tile list), map_rows2 / map_rows8 / map_rows16 (-DTOPO_MAP_ROWS=2 / 8 / 16);
  3. `--step trace`    one repetition of each under `rocprofv3 --kernel-trace --stats` (the program after `--`), for the kernels' own
                       durations (k_map, k_surface_grid, k_surface);
and writes all of it into --out (default profiles/map_c4.json)."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEP_LIMIT_S = 240
GRIDS = (1024, 256)
INTERVAL_M, INDEX_EVERY = 100.0, 5
VARIANTS = ("map_recompute", "map_alltiles", "map_rows2", "map_rows8", "map_rows16")


def host_compose(T, np, rec, n, p, normals, masks, tile_index, tile_h):
    """Flags and RGBA of an n x n map from topo_surface_device's records, in numpy: the rule of csrc/topo_map.h in f64."""
    terrain = rec["kind"] == T.SURFACE_TERRAIN
    flags = np.where(terrain, T.MAP_FLAG_TERRAIN, 0).astype(np.uint8)
    grey = np.full(len(rec), 255, np.int64)
    idx = np.nonzero(terrain)[0]
    r = rec[idx]
    tile = tile_index[r["tile_lat_deg"] - tile_index.lat0, r["tile_lon_deg"] - tile_index.lon0]
    cx, cy, k = r["cell_x"].astype(np.int64), r["cell_y"].astype(np.int64), r["tri"].astype(np.int64)
    even = (cx + cy) % 2 == 0
    # triangle_vertices: k = 0: a, b, (even ? d : c); k = 1: d, c, (even ? a : b) with a = (i, j), b = (i, j + 1), c = (i + 1, j), d = (i + 1, j + 1)
    vx = np.stack([cx + k, cx + k, cx + 1 - k], axis=1)
    vy = np.stack([cy + k, cy + 1 - k, cy + np.where(k == 0, even, ~even)], axis=1)
    nv = 2.0 * normals[tile[:, None], vy, vx, :3].astype(np.float64) / 255.0 - 1.0
    nv = np.einsum("tij,tvj->tvi", tile_index.rot[tile], nv)
    w1, w2 = r["w1"].astype(np.float64), r["w2"].astype(np.float64)
    nn = nv[:, 0] * (1.0 - w1 - w2)[:, None] + nv[:, 1] * w1[:, None] + nv[:, 2] * w2[:, None]
    nn /= np.linalg.norm(nn, axis=1)[:, None]
    lin = 0.01 + 0.7 * np.maximum(nn @ np.asarray(p["sun_direction"][0], np.float64), 0.0)
    s = np.where(lin <= 0.0031308, 12.92 * lin, 1.055 * lin ** (1.0 / 2.4) - 0.055)
    grey[idx] = np.floor(255.0 * s + 0.5).astype(np.int64)
    cell = cx * (tile_h - 1) + cy
    seen = (masks[tile, cell >> 5] >> (cell & 31).astype(np.uint32)) & 1
    flags[idx] |= (seen * T.MAP_FLAG_SEEN).astype(np.uint8)
    level = np.floor(rec["height_m"] / INTERVAL_M).reshape(n, n)
    tg, fl = terrain.reshape(n, n), flags.reshape(n, n)
    for dy, dx in ((0, 1), (1, 0)):
        a, b = level[:n - dy, :n - dx], level[dy:, dx:]
        differ = tg[:n - dy, :n - dx] & tg[dy:, dx:] & (a != b)
        index = differ & (np.floor(np.maximum(a, b) / INDEX_EVERY) > np.floor(np.minimum(a, b) / INDEX_EVERY))
        fl[:n - dy, :n - dx] |= (differ * T.MAP_FLAG_CONTOUR + index * T.MAP_FLAG_INDEX).astype(np.uint8)

    def blend(c, s4):
        a = int(s4[3])
        return (c * (255 - a) + np.asarray(s4[:3], np.int64) * a + 127) // 255

    col = np.repeat(grey.reshape(n, n)[..., None], 3, axis=-1)
    for bit, key in ((T.MAP_FLAG_SEEN, "seen_rgba"), (T.MAP_FLAG_CONTOUR, "contour_rgba"), (T.MAP_FLAG_INDEX, "index_rgba")):
        sel = (fl & bit) != 0 if bit != T.MAP_FLAG_CONTOUR else ((fl & T.MAP_FLAG_CONTOUR) != 0) & ((fl & T.MAP_FLAG_INDEX) == 0)
        col[sel] = blend(col[sel], p[key][0])
    rgba = np.empty((n, n, 4), np.uint8)
    rgba[...] = p["void_rgba"][0]
    rgba[tg, :3] = col[tg]
    rgba[tg, 3] = 255
    return rgba, fl


def step(args):
    import numpy as np
    import torch
    import topo_renderer_amd as T
    from bench import LAT0, LON0, TILE, WORKLOADS
    deg = WORKLOADS["c4"][0]
    reps = 1 if args.step == "trace" else max(args.reps, 15)
    W, H = 512, 256
    r = T.TerrainRenderer(W, H)
    r.set_stream(torch.cuda.current_stream().cuda_stream)
    locs = T.synth.mosaic_locations(LAT0, LON0, deg, deg)
    for (la, lo) in locs:
        r.add_terrain(la, lo, T.synth_tile(la, lo, TILE, TILE), *T.synth.tile_transform(la, lo, TILE, TILE))
    # a frame from the middle of the mosaic, so that the seen layer has marks to show
    r.viewshed_enable(True)
    vlon, vlat = LON0 + 0.5 * deg + 0.0123, LAT0 + 0.5 * deg + 0.0217
    eye = T.geometry_transform(4000.0, vlon, vlat)
    r.update(W, H, T.camera_uniforms(eye, 0.7, -0.15, 1.2, W, H, vlon, vlat, 0), T.post_uniforms(W, H))
    r.render(want_depth=False)
    r.synchronize()
    sun = T.sun_direction(LON0 + 0.5 * deg, LAT0 + 0.5 * deg, 315.0, 45.0).astype(np.float32)
    med = lambda v: v[len(v) // 2]
    stat = lambda v: {"median": round(med(v), 3), "min": round(v[0], 3), "max": round(v[-1], 3)}

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

    host = None
    if args.step == "time":      # what (b) has on the host before it starts
        order = sorted(locs)
        host = type("Host", (), {})()
        host.lat0, host.lon0 = min(l[0] for l in locs), min(l[1] for l in locs)
        index = np.zeros((deg, deg), np.int64)
        for i, (la, lo) in enumerate(order):
            index[la - host.lat0, lo - host.lon0] = i
        normals = np.stack([r.read_normals(la, lo) for la, lo in order])
        words = ((TILE - 1) * (TILE - 1) + 31) // 32
        masks = np.zeros((len(order), words), np.uint32)
        for i, (la, lo) in enumerate(order):
            bits = np.zeros(words * 32, np.uint8)
            m = r.viewshed(la, lo)
            bits[:m.size] = np.ascontiguousarray(m.T).ravel()
            masks[i] = np.packbits(bits.reshape(-1, 32)[:, ::-1], axis=1).view(">u4").ravel()
        rot = np.stack([T.terrain_uniforms(*T.synth.tile_transform(la, lo, TILE, TILE), TILE, TILE)[8:24].reshape(4, 4).T[:3, :3] for la, lo in order]).astype(np.float64)

        class Index:
            def __getitem__(self, key):
                return index[key]
        host.index = Index()
        host.index.lat0, host.index.lon0, host.index.rot = host.lat0, host.lon0, rot
        host.normals, host.masks = normals, masks

    out = {}
    for n in GRIDS:
        p = T.map_params(LON0, LAT0 + deg, deg / n, -deg / n, n, n, sun_direction=sun, contour_interval_m=INTERVAL_M, index_every=INDEX_EVERY)
        rgba = torch.zeros((n, n, 4), dtype=torch.uint8, device="cuda")
        flags = torch.zeros((n, n), dtype=torch.uint8, device="cuda")
        grid = torch.zeros((n, n), dtype=torch.float32, device="cuda")
        res = {"nx": n, "ny": n, "reps": reps, "map_ms": stat(timed(lambda: r.map_device(p, rgba, flags)))}
        if args.step != "variant":
            res["surface_grid_ms"] = stat(timed(lambda: r.surface_grid_device(LON0, LAT0 + deg, deg / n, -deg / n, n, n, grid.data_ptr())))
        if args.step == "trace":
            pts = torch.zeros((n * n, 2), dtype=torch.float64, device="cuda")
            rec = torch.zeros((n * n, 48), dtype=torch.uint8, device="cuda")
            r.surface_device(pts.data_ptr(), rec.data_ptr(), n * n)
            torch.cuda.synchronize()
        if args.step == "time":
            f = flags.cpu().numpy()
            res["share"] = {k: round(float(((f & bit) != 0).mean()), 4) for k, bit in (("terrain", 1), ("contour", 2), ("index", 4), ("seen", 8))}
            c, rr = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64))
            pts = np.stack([LON0 + c * (deg / n), (LAT0 + deg) + rr * (-deg / n)], axis=-1).reshape(-1, 2)

            def compose():
                rec = r.surface(pts)
                return host_compose(T, np, rec, n, p, host.normals, host.masks, host.index, TILE)

            compose()
            wall = []
            for _ in range(reps):
                t0 = time.perf_counter()
                got = compose()
                wall.append(1e3 * (time.perf_counter() - t0))
            res["compose_wall_ms"] = stat(sorted(wall))
            res["compose_flags_equal_share"] = round(float((got[1] == f).mean()), 5)
        out[f"{n}x{n}"] = res
    if args.step != "trace":
        print(json.dumps(out))


def run_step(cmd, what, env=None):
    print(f"map_profile: {what}", file=sys.stderr, flush=True)
    res = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT_S)] + cmd, capture_output=True, text=True, env=env)
    if res.returncode != 0:
        sys.exit(f"{what}: exit status {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-2000:]}")
    return res.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["time", "variant", "trace"])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_c4.json"))
    args = ap.parse_args()
    if args.step:
        return step(args)
    me = os.path.abspath(__file__)
    out = {"what": "tools/map_profile.py: the c4 mosaic (100 tiles of 1200 x 1200), a 1024 x 1024 and a 256 x 256 map over it with all layers on (interval 100 m, "
                   "every 5th an index contour, one frame's viewshed marks); map = topo_map_device, surface_grid = topo_surface_grid_device on the same grid, compose = "
                   "topo_surface_read of the grid's points and the shading, contours and mask lookup in numpy (wall clock); medians of the repetitions after a "
                   "warm-up, then the map alone with each ablation build, then one repetition under rocprofv3 --kernel-trace --stats"}
    out["product"] = json.loads(run_step([sys.executable, me, "--step", "time", "--reps", str(args.reps)], "timing step").strip().split("\n")[-1])
    out["variants"] = {}
    for name in VARIANTS:
        lib = os.path.join(ROOT, "exp", f"libtopo_{name}.so")
        if os.path.exists(lib):
            got = run_step([sys.executable, me, "--step", "variant", "--reps", str(args.reps)], f"variant {name}", env=dict(os.environ, TOPO_HIP_LIB=lib))
            out["variants"][name] = {k: v["map_ms"] for k, v in json.loads(got.strip().split("\n")[-1]).items()}
    with tempfile.TemporaryDirectory() as d:
        run_step(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "map", "--", sys.executable, me, "--step", "trace"], "trace step")
        kernels = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                for k in ("k_map", "k_surface_grid", "k_surface"):
                    if k + "(" in row["Name"]:
                        kernels[k] = {"calls": int(row["Calls"]), "average_ms": round(float(row["AverageNs"]) / 1e6, 3), "min_ms": round(float(row["MinNs"]) / 1e6, 3),
                                      "max_ms": round(float(row["MaxNs"]) / 1e6, 3)}
        out["kernels_rocprofv3"] = kernels
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
