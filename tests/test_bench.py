"""bench.py's own contract: a plain run reports the headline alone, --full the breakdown, and --dump-outputs writes what the
timed path computed in its last step (every pixel of a small panorama, a fixed seeded sample of a large one)."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(*args, timeout=300):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], cwd=ROOT, capture_output=True, text=True,
                       timeout=timeout)
    return p


def test_dump_outputs_every_pixel_or_a_fixed_sample(tmp_path, monkeypatch):
    import torch
    import bench
    g = torch.Generator().manual_seed(7)
    rgba = torch.randint(0, 256, (8, 64, 32, 4), dtype=torch.uint8, generator=g)
    depth = torch.rand((8, 64, 32), generator=g)
    n = 8 * 64 * 32

    info = bench.dump_outputs(str(tmp_path / "all"), np, torch, rgba, depth)          # small output: every pixel
    a, d = np.load(tmp_path / "all" / "rgba.npy"), np.load(tmp_path / "all" / "depth.npy")
    assert info["pixels"] == info["of"] == n and a.dtype == d.dtype == np.float32
    assert np.array_equal(a, rgba.reshape(n, 4).numpy().astype(np.float32)) and np.array_equal(d, depth.reshape(n).numpy())

    monkeypatch.setattr(bench, "DUMP_PIXELS", 1000)                                    # large output: one pixel per run
    for sub in ("s1", "s2"):
        info = bench.dump_outputs(str(tmp_path / sub), np, torch, rgba, depth)
        assert info["pixels"] == 1000 and info["of"] == n
    a, d = np.load(tmp_path / "s1" / "rgba.npy"), np.load(tmp_path / "s1" / "depth.npy")
    assert np.array_equal(a, np.load(tmp_path / "s2" / "rgba.npy")) and np.array_equal(d, np.load(tmp_path / "s2" / "depth.npy"))
    assert a.shape == (1000, 4) and d.shape == (1000,) and a.dtype == d.dtype == np.float32
    # each sampled pixel is the one at its position in the output, and the positions fall one into each equal run
    flat_d = depth.reshape(n).numpy()
    pos = [int(np.flatnonzero(flat_d == v)[0]) for v in d]
    edges = np.arange(1001) * n // 1000
    assert all(edges[k] <= pos[k] < edges[k + 1] for k in range(1000))
    assert np.array_equal(a, rgba.reshape(n, 4).numpy()[pos].astype(np.float32))

    info = bench.dump_outputs(str(tmp_path / "rgba_only"), np, torch, rgba, None)
    assert info["files"] == ["rgba.npy"] and not (tmp_path / "rgba_only" / "depth.npy").exists()


def test_bench_rejects_what_it_cannot_do():
    # (argument checks come before anything touches a device)
    p = _bench("--steps", "0", timeout=60)
    assert p.returncode == 2 and "--steps" in p.stderr
    p = _bench("--check", timeout=60)
    assert p.returncode == 2 and "--full" in p.stderr


def _c1_oracle(T, O, bench):
    deg, PW, PH = bench.WORKLOADS["c1"]
    SW = PW // bench.N_SECTORS
    locs = T.synth.mosaic_locations(bench.LAT0, bench.LON0, deg, deg)
    vlat, vlon = bench.LAT0 + deg / 2 + 0.123, bench.LON0 + deg / 2 + 0.217
    la, lo = int(math.floor(vlat)), int(math.floor(vlon))
    ground = T.synth.height_at(T.synth_tile(la, lo, bench.TILE, bench.TILE), la, lo, vlon, vlat)
    views = T.panorama_uniforms(T.geometry_transform(ground + 50.0, vlon, vlat), 0.0, SW, PH, vlon, vlat, 0, pitch=0.0)
    o = O.OracleRenderer(SW, PH)
    for (la, lo) in locs:
        o.add_terrain(la, lo, T.synth_tile(la, lo, bench.TILE, bench.TILE), *T.synth.tile_transform(la, lo, bench.TILE, bench.TILE))
    o.update(SW, PH, views[0], T.post_uniforms(SW, PH))
    return o.render_views(views, threads=min(len(views), os.cpu_count() or 1))


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_dumps_the_last_step(topo, orc, tmp_path):
    p = _bench("--gpus", "1", "--workload", "c1", "--steps", "7", "--warmup", "2", "--dump-outputs", str(tmp_path))
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads(p.stdout.strip().split("\n")[-1])
    assert all(k in line for k in HEADLINE) and line["steps"] == 7 and line["ms_per_step"] > 0
    assert abs(line["value"] - 1024 * 256 / 1e6 / (line["ms_per_step"] / 1e3)) <= 1e-3 * line["value"]
    assert not any(k in line for k in ("kernel_ms", "roofline", "cpu_baseline", "load_ms", "pipelined"))
    import bench
    rgba, depth = _c1_oracle(topo, orc, bench)                  # c1 has fewer pixels than DUMP_PIXELS: all of them are written
    got_rgba, got_depth = np.load(tmp_path / "rgba.npy"), np.load(tmp_path / "depth.npy")
    assert got_rgba.dtype == got_depth.dtype == np.float32
    assert np.array_equal(got_rgba, rgba.reshape(-1, 4).astype(np.float32))
    assert np.array_equal(got_depth.view(np.uint32), depth.reshape(-1).view(np.uint32))


@pytest.mark.gpu
def test_full_run_keeps_the_breakdown(topo):
    p = _bench("--gpus", "1", "--workload", "c1", "--steps", "8", "--warmup", "2", "--full", "--no-pmc", "--no-cpu-baseline",
               "--no-host-path")
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads(p.stdout.strip().split("\n")[-1])
    assert all(k in line for k in HEADLINE) and line["steps"] == 8
    for k in ("kernel_ms", "roofline", "per_kernel", "load_ms", "counters", "pipelined"):
        assert k in line, k
    assert line["kernel_ms"]["resolve"] > 0 and line["counters"]["status"] == 0
