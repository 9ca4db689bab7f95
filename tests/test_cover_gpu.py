"""The covered-region path on the GPU (k_raster_rare's claims, k_raster_cover, k_raster_big's skip): frames with the path on against
frames with it off (TOPO_COVER=0, a fresh child process per setting: the switch is read once per process) and against the oracle,
the six counters, the hook's statistics against the CPU emulation of the same scenes (tests/cover_emul.cpp), frames in flight, and
a big queue too small for the items.

The scenes (cover_emul.CASES): the coarse mesh Scene(12, 2, 2, eye_dh=60) at 640 x 480, 333 x 200 and as two-view submissions at
333 x 200 (the second view's keys start at 66 600, not a multiple of 64), with the views of
test_gpu_parity.py::test_big_triangle_queue_and_clipping_paths_are_exercised and one more pitched 80 degrees down -- and, because
NO triangle of that scene covers a region (its giants are cut by the near plane so close to the eye that the guard band discards
them: 0.7 % of a frame is terrain, the CPU emulation counts 0 covering items in every view), a table mountain at the same three
shapes, whose views the CPU emulation picked: tests/test_cover_cpu.py::test_the_scenes_exercise_every_branch holds what they
exercise (claims won and lost, rows stored blind, merged rows in which an older key wins)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cover_emul as CE
from scenes import assert_same_frame

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _child(tmp, setting):
    out = os.path.join(tmp, f"cover_{setting}.npz")
    env = dict(os.environ, TOPO_COVER=setting)
    p = subprocess.run([sys.executable, os.path.join(HERE, "cover_worker.py"), out], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, f"TOPO_COVER={setting}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"
    z = np.load(out)
    return {"meta": json.loads(bytes(z["meta"]).decode()), "z": z}


@pytest.fixture(scope="module")
def runs(topo, tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("cover"))
    return {"on": _child(tmp, "1"), "off": _child(tmp, "0")}


@pytest.fixture(scope="module")
def oracle_frames(topo, orc):
    """(case, submission, view) -> the oracle's frame; one oracle renderer per scene and size."""
    out = {}
    for case, (scene, W, H, subs) in CE.CASES.items():
        sc = CE.case_scene(scene)
        o = orc.OracleRenderer(W, H)
        sc.load(o)
        for i, sub in enumerate(subs):
            for k, pose in enumerate(sub):
                same = next((key for key in out if CE.CASES[key[0]][:3] == (scene, W, H) and CE.CASES[key[0]][3][key[1]][key[2]] == pose), None)
                if same is None:
                    o.update(W, H, sc.uniforms(W, H, *pose, 0), topo.post_uniforms(W, H))
                    out[(case, i, k)] = o.render()
                else:
                    out[(case, i, k)] = out[same]
    return out


def _frame(run, name, k):
    return run["z"][name + "/rgba"][k], run["z"][name + "/depth"][k]


def _submissions():
    return [(case, i) for case, (_, _, _, subs) in CE.CASES.items() for i in range(len(subs))]


def test_frames_equal_with_the_path_on_and_off_and_equal_the_oracle(runs, oracle_frames):
    for case, i in _submissions():
        for k in range(len(CE.CASES[case][3][i])):
            on, off = _frame(runs["on"], f"{case}/{i}", k), _frame(runs["off"], f"{case}/{i}", k)
            assert_same_frame(on, off, f"{case} submission {i} view {k}: cover path on against off")
            assert_same_frame(on, oracle_frames[(case, i, k)], f"{case} submission {i} view {k}: cover path on against the oracle")
            assert_same_frame(off, oracle_frames[(case, i, k)], f"{case} submission {i} view {k}: cover path off against the oracle")


def test_counters_and_status_equal_with_the_path_on_and_off(runs):
    for case, i in _submissions():
        on, off = runs["on"]["meta"][f"{case}/{i}"], runs["off"]["meta"][f"{case}/{i}"]
        assert on["counters"] == off["counters"], (case, i, on["counters"], off["counters"])
        assert on["status"]["status"] == 0 and off["status"]["status"] == 0 and not on["status"]["bounds_violation"], (case, i, on["status"], off["status"])


def test_hook_reports_the_claims_the_cpu_emulation_predicts(runs, topo):
    """With the path on: per submission, the covering items, the claims won (one per covered region) and the claims lost are the
    CPU emulation's counts, claims are won, and on the table mountain a claim is lost; with TOPO_COVER=0 all three are 0."""
    won, lost = {}, {}
    for case, i in _submissions():
        scene, W, H, subs = CE.CASES[case]
        sc = CE.case_scene(scene)
        want = {"candidates": 0, "won": 0, "lost": 0}
        for k, pose in enumerate(subs[i]):
            st = CE.cover_frame(topo, sc, W, H, sc.uniforms(W, H, *pose, 0), key_base=k * W * H)
            for name in want:
                want[name] += st[name]
        got = runs["on"]["meta"][f"{case}/{i}"]["cover"]
        print(case, i, "hook", got, "emulation", want)
        assert got == want, (case, i, got, want)
        assert runs["off"]["meta"][f"{case}/{i}"]["cover"] == {"candidates": 0, "won": 0, "lost": 0}, (case, i)
        won[case] = won.get(case, 0) + got["won"]
        lost[case] = lost.get(case, 0) + got["lost"]
    for case in CE.CASES:      # case by case: every table-mountain case wins claims and loses one, no coarse-mesh case has any
        assert (won[case] > 0 and lost[case] > 0) if case.startswith("mesa") else (won[case] == 0 and lost[case] == 0), (case, won, lost)


def test_path_holds_with_frames_in_flight(runs, oracle_frames):
    case = "mesa_333x200"
    subs = CE.CASES[case][3]
    for j in range(2 * len(subs)):
        i = j % len(subs)
        for k in range(len(subs[i])):
            on, off = _frame(runs["on"], f"in_flight/{j}", k), _frame(runs["off"], f"in_flight/{j}", k)
            assert_same_frame(on, oracle_frames[(case, i, k)], f"frame {j} in flight, view {k}: cover path on against the oracle")
            assert_same_frame(off, on, f"frame {j} in flight, view {k}: cover path off against on")
    assert runs["on"]["meta"]["in_flight"]["status"]["status"] == 0
    assert runs["on"]["meta"]["in_flight"]["cover"]["won"] > 0 and runs["off"]["meta"]["in_flight"]["cover"]["won"] == 0


def test_path_holds_with_a_big_queue_too_small_for_the_items(runs, oracle_frames):
    """The triangles the queue has no room for are rasterised in place and claim nothing: every claim names a queue slot.  The queue
    holds 96 of the view's 107 items, so claims and overflow meet in one frame."""
    case = "mesa_333x200"
    on, off = runs["on"]["meta"]["small_queue"], runs["off"]["meta"]["small_queue"]
    assert on["status"]["big_overflow"] and off["status"]["big_overflow"] and not on["status"]["bounds_violation"]
    assert_same_frame(_frame(runs["on"], "small_queue", 0), oracle_frames[(case, 2, 0)], "small big queue, cover path on against the oracle")
    assert_same_frame(_frame(runs["off"], "small_queue", 0), _frame(runs["on"], "small_queue", 0), "small big queue, cover path off against on")
    assert on["counters"] == off["counters"], (on["counters"], off["counters"])
    print("small queue: hook", on["cover"], "with room for every item", runs["on"]["meta"][f"{case}/2"]["cover"])
    assert 0 < on["cover"]["won"] <= min(CE.SMALL_BIG_CAP, runs["on"]["meta"][f"{case}/2"]["cover"]["won"]), on["cover"]
    assert on["cover"]["candidates"] <= runs["on"]["meta"][f"{case}/2"]["cover"]["candidates"], on["cover"]
