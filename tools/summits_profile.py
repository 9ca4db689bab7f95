#!/usr/bin/env python3
"""The summit queries' cost on the c4 mosaic (100 tiles of 1200 x 1200, 144 M posts):
  (a) summits    topo_summits_device at radius 5 km, min isolation 1 km, min height 0, event-timed over --reps repetitions after a
                 warm-up call (every value is kept: ms_all); the wall time the host takes to queue one call on an idle device, and the
                 events' time of a call queued behind three others -- the two figures that tell a host-bound call from a device-bound
                 one; what it found: the posts left after k_summit_candidates, the summits, their isolations;
  (b) snap       topo_summit_snap_device of 5000 seeded points over the mosaic at 500 m, timed the same way;
  (c) baseline   (--baseline) the g++ build of the same rule in its windowed form (tests/summits_emul.py: -O2, ONE thread, on the
                 host this runs on) over the same mosaic with the same parameters, timed once with the wall clock -- and the check
                 that it finds the summits the device found.
Per-kernel times come from a run of their own:
  rocprofv3 --kernel-trace --stats --output-format csv -d out/summits_trace -- python tools/summits_profile.py --step time --reps 1
(seven summit calls in all: the warm-up, one timed, one for the host's time, four for the queued one).
The registers of the kernels are read from the code objects (tools/kernel_resources.py) where hipcc is at hand.

Without --step the tool runs the measurement in a child under its own `timeout` and writes --out (default profiles/summits_c4.json)."""
import argparse
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEP_LIMIT_S = 540
RADIUS_M, MIN_ISOLATION_M, MIN_HEIGHT_M = 5000.0, 1000.0, 0.0
SNAP_POINTS, SNAP_RADIUS_M = 5000, 500.0


def mosaic():
    import topo_renderer_amd as T
    from bench import LAT0, LON0, TILE, WORKLOADS
    deg = WORKLOADS["c4"][0]
    locs = sorted(T.synth.mosaic_locations(LAT0, LON0, deg, deg))      # (draw order: the emulation's tile ranks are the renderer's)
    return locs, [(T.synth_tile(la, lo, TILE, TILE),) + tuple(T.synth.tile_transform(la, lo, TILE, TILE)) for la, lo in locs], (LAT0, LON0, deg, TILE)


def step(args):
    import numpy as np
    import torch
    import topo_renderer_amd as T
    locs, tiles, (lat0, lon0, deg, tile) = mosaic()
    r = T.TerrainRenderer(64, 64)
    r.set_stream(torch.cuda.current_stream().cuda_stream)
    for (la, lo), t in zip(locs, tiles):
        r.add_terrain(la, lo, *t)
    r.synchronize()
    cap = 1 << 20
    rec_dev = torch.zeros((cap * 64,), dtype=torch.uint8, device="cuda")
    cnt_dev = torch.zeros((4,), dtype=torch.int32, device="cuda")
    pts = np.random.default_rng(11).uniform([lon0, lat0], [lon0 + deg, lat0 + deg], (SNAP_POINTS, 2))
    pts_dev = torch.from_numpy(pts).cuda()
    snap_dev = torch.zeros((SNAP_POINTS * 48,), dtype=torch.uint8, device="cuda")

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
    call = lambda: r.summits_device(rec_dev.data_ptr(), cap, cnt_dev.data_ptr(), RADIUS_M, MIN_ISOLATION_M, MIN_HEIGHT_M)
    ms = timed(call, args.reps)
    # how long the host takes to queue one call's launches on an idle device (the call returns before the device has finished), and
    # the events' time of calls queued behind a busy device: `lead` of them first, so that the host is ahead when the events are recorded
    torch.cuda.synchronize()
    host = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        call()
        host.append(1e3 * (time.perf_counter() - t0))
        torch.cuda.synchronize()
    host.sort()
    lead, behind = 3, []
    for _ in range(args.reps):
        for _ in range(lead):
            call()
        s0, e0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s0.record()
        call()
        e0.record()
        torch.cuda.synchronize()
        behind.append(s0.elapsed_time(e0))
    behind.sort()
    n = int(cnt_dev.cpu().numpy().view(np.uint32)[0])
    assert n <= cap
    rec = rec_dev.cpu().numpy()[:n * 64].view(T.SUMMIT_DTYPE)
    counts = r.debug_summit_counts()
    ms_snap = timed(lambda: r.summit_snap_device(pts_dev.data_ptr(), SNAP_POINTS, SNAP_RADIUS_M, snap_dev.data_ptr()), args.reps)
    snap = snap_dev.cpu().numpy().view(T.SUMMIT_SNAP_DTYPE)
    posts = len(tiles) * tile * tile
    fin = np.isfinite(rec["isolation_m"])
    out = {"shape": {"tiles": len(tiles), "posts": posts, "radius_m": RADIUS_M, "min_isolation_m": MIN_ISOLATION_M, "min_height_m": MIN_HEIGHT_M, "reps": args.reps},
           "summits": {"ms": stat(ms), "ms_all": [round(v, 3) for v in ms], "host_enqueue_ms": stat(host), "ms_queued_behind_three_calls": stat(behind), "mposts_per_s": round(posts / stat(ms)["median"] / 1e3, 1), "after_candidates": counts["candidates"], "summits": n,
                       "isolation_infinite": int((~fin).sum()), "isolation_m_median": round(float(np.median(rec["isolation_m"][fin])), 1) if fin.any() else None,
                       "height_m_max": round(float(rec["height_m"].max()), 1) if n else None},
           "snap": {"points": SNAP_POINTS, "radius_m": SNAP_RADIUS_M, "ms": stat(ms_snap), "found": int((snap["status"] == T.SNAP_FOUND).sum()),
                    "distance_m_median": round(float(np.median(snap["distance_m"][snap["status"] == T.SNAP_FOUND])), 1)}}
    if args.baseline:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import summits_emul as SE
        SE.lib()
        t0 = time.perf_counter()
        emu, n_emu, stages, bad = SE.summits(tiles, locs, RADIUS_M, MIN_ISOLATION_M, MIN_HEIGHT_M, capacity=cap)
        wall = time.perf_counter() - t0
        same = n_emu == n and bad == 0 and np.array_equal(emu["idx"] % tile, rec["vx"]) and np.array_equal(emu["idx"] // tile, rec["vy"])
        out["baseline_g++_windowed_one_thread"] = {"s": round(wall, 2), "over_device": round(1e3 * wall / stat(ms)["median"], 1), "after_candidates": stages[0], "summits": n_emu,
                                                   "same_summits_as_device": bool(same)}
    print(json.dumps(out))
    if args.baseline and not out["baseline_g++_windowed_one_thread"]["same_summits_as_device"]:
        sys.exit("the emulation found other summits than the device")


def resources():
    """The summit kernels' rows of tools/kernel_resources.py, or None where hipcc is not at hand."""
    try:
        text = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py")], capture_output=True, text=True, timeout=900).stdout
    except (OSError, subprocess.SubprocessError):
        return None
    rows = {}
    for line in text.split("\n"):
        if line.startswith("k_summit"):
            w = line.split()
            rows.setdefault(re.match(r"k_summit_[a-z]+", w[0]).group(0), {"vgpr": int(w[2]), "sgpr": int(w[4]), "lds_bytes": int(w[6]), "scratch_bytes": int(w[8]), "vgpr_spills": int(w[10][1:]), "sgpr_spills": int(w[11][1:])})
    return rows or None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=["c4"], default="c4")
    ap.add_argument("--step", choices=["time"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--baseline", action="store_true", help="also time the g++ emulation over the same mosaic (one thread: about a minute)")
    ap.add_argument("--no-resources", action="store_true", help="leave out the compile that reads the kernels' registers")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "summits_c4.json"))
    args = ap.parse_args()
    if args.step:
        return step(args)
    out = {"what": "tools/summits_profile.py: the c4 mosaic (100 tiles of 1200 x 1200); topo_summits_device at radius 5 km, min isolation 1 km, min height 0 and "
                   "topo_summit_snap_device of 5000 points at 500 m, event-timed repetitions after a warm-up; baseline = the g++ build of the same rule, windowed, "
                   "-O2, one thread, wall clock, on the same host"}
    cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--step", "time", "--reps", str(args.reps)] + (["--baseline"] if args.baseline else [])
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        sys.exit(f"timing step: exit status {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-2000:]}")
    out.update(json.loads(res.stdout.strip().split("\n")[-1]))
    if not args.no_resources:
        out["kernel_resources"] = resources()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
