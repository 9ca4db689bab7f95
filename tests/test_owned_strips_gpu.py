"""k_resolve's owned strips on the GPU (k_raster_cover's strip records, the ownership test, the route from the record): frames with
the path on against frames with it off and against the oracle, bit for bit, and the counting hook against the CPU emulation of the
same scenes.  One child process (tests/owned_worker.py, TOPO_COVER=1) renders everything on one renderer per colour format, so every
frame finds the records of earlier frames, other viewpoints and other target shapes in the table.

The cases (owned_emul.CASES): the table mountain of tests/cover_cases.py at 128 x 72 and as two views of 200 x 150 -- regions cut
by both edges, a second view whose first key is no multiple of 64 --, at cover_cases' own 333 x 200, where its viewpoints lose a bid
(view 3) and meet a row in which an older, nearer key wins inside a claimed region (view 4: strips of a claimed region that must NOT
be owned, and owners cut by the near plane), and a plain under a 5 degree lens whose owners are of record kind 2.  Then view modes
1 and 2, the three other surface formats, and pipeline depth 2.

TOPO_HIP_LIB=<the bounds-checking library> runs the same file through every TOPO_CHK site (the status record must stay clean)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cover_emul as CE
import owned_emul as OE
import owned_worker as OW
from scenes import assert_same_frame

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def run(topo, tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("owned")), "owned.npz")
    env = dict(os.environ, TOPO_COVER="1")
    env.pop("TOPO_RESOLVE_OWNED", None)
    p = subprocess.run([sys.executable, os.path.join(HERE, "owned_worker.py"), out], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, f"exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"
    z = np.load(out)
    return {"meta": json.loads(bytes(z["meta"]).decode()), "z": z}


@pytest.fixture(scope="module")
def emulated(topo):
    """(case, submission) -> per view the CPU emulation of the near phase (the scenes have no far phase): its claim counts and,
    from its keys, the strips with one winner."""
    out = {}
    for case, (scene, W, H, subs) in OE.CASES.items():
        sc = OE.case_scene(scene)
        for i, sub in enumerate(subs):
            views = []
            for k, pose in enumerate(sub):
                st = CE.cover_frame(topo, sc, W, H, sc.uniforms(W, H, *pose, 0), key_base=k * W * H, want_keys=True)
                st["one_winner"] = OE.one_winner_strips(st.pop("keys"))
                views.append(st)
            out[(case, i)] = views
    return out


def _oracle(orc, topo, scene, W, H, pose, mode=0, fmt=None):
    sc = OE.case_scene(scene)
    o = orc.OracleRenderer(W, H) if fmt is None else orc.OracleRenderer(W, H, color_format=fmt)
    sc.load(o)
    o.update(W, H, sc.uniforms(W, H, *pose, mode), topo.post_uniforms(W, H))
    return o.render()


@pytest.fixture(scope="module")
def oracle_frames(topo, orc):
    """(scene, W, H, pose) -> the oracle's frame (view mode 0, Rgba8UnormSrgb); one oracle renderer per scene and size."""
    out, renderers = {}, {}
    for case, (scene, W, H, subs) in OE.CASES.items():
        for sub in subs:
            for pose in sub:
                if (scene, W, H, pose) in out:
                    continue
                if (scene, W, H) not in renderers:
                    renderers[(scene, W, H)] = orc.OracleRenderer(W, H)
                    OE.case_scene(scene).load(renderers[(scene, W, H)])
                o = renderers[(scene, W, H)]
                o.update(W, H, OE.case_scene(scene).uniforms(W, H, *pose, 0), topo.post_uniforms(W, H))
                out[(scene, W, H, pose)] = o.render()
    return out


def _frame(run, name, k=0):
    return run["z"][name + "/rgba"][k], run["z"][name + "/depth"][k]


def _submissions():
    return [(case, i) for case, (_, _, _, subs) in OE.CASES.items() for i in range(len(subs))]


def _marked(view, H):
    """The strips of a view's claimed regions that start inside the target, from the emulation's counts: a whole region has 64 rows and
    8 strips, one cut by the lower edge H % 64 rows; the rows of the claimed regions are those stored blind and those merged."""
    rows, cut = view["rows_blind"] + view["rows_merged"], H % 64
    whole = view["won"] if cut == 0 else (rows - cut * view["won"]) // (64 - cut)
    return 8 * whole + (view["won"] - whole) * ((cut + 7) // 8)


def test_frames_equal_with_the_path_on_and_off_and_equal_the_oracle(run, oracle_frames):
    for case, i in _submissions():
        scene, W, H, subs = OE.CASES[case]
        for k, pose in enumerate(subs[i]):
            on, off = _frame(run, f"{case}/{i}/on", k), _frame(run, f"{case}/{i}/off", k)
            assert_same_frame(on, off, f"{case} submission {i} view {k}: owned strips on against off")
            assert_same_frame(on, oracle_frames[(scene, W, H, pose)], f"{case} submission {i} view {k}: owned strips on against the oracle")
        on, off = run["meta"][f"{case}/{i}/on"], run["meta"][f"{case}/{i}/off"]
        assert on["counters"] == off["counters"] and on["cover"] == off["cover"], (case, i, on, off)
        assert on["status"]["status"] == 0 and off["status"]["status"] == 0 and not on["status"]["bounds_violation"] and not off["status"]["bounds_violation"], (case, i, on, off)


def test_hook_counts_what_the_cpu_emulation_predicts(run, emulated):
    """Marked strips: the strips of the claimed regions that start inside the target, as the emulation's claims give them.
    Owned strips: among them those with one winner -- no more than the marked strips and no more than the one-winner strips of the
    emulated keys (which count the strips outside the claimed regions too).  With the path off the hook reports nothing."""
    total = {}
    for case, i in _submissions():
        views, H = emulated[(case, i)], OE.CASES[case][2]
        won, lost = sum(v["won"] for v in views), sum(v["lost"] for v in views)
        one_winner = sum(len(v["one_winner"]) for v in views)
        got, cover = run["meta"][f"{case}/{i}/on"]["owned"], run["meta"][f"{case}/{i}/on"]["cover"]
        print(case, i, "hook", got, cover, "emulation: won", won, "lost", lost, "one-winner strips", one_winner)
        assert cover["won"] == won and cover["lost"] == lost, (case, i, cover, won, lost)
        assert got["marked"] == sum(_marked(v, H) for v in views) and got["owned"] <= min(got["marked"], one_winner), (case, i, got, won, one_winner)
        assert run["meta"][f"{case}/{i}/off"]["owned"] == {"owned": 0, "marked": 0}, (case, i)
        t = total.setdefault(case, {"owned": 0, "marked": 0})
        t["owned"] += got["owned"]
        t["marked"] += got["marked"]
    for case, t in total.items():      # every case owns strips
        assert t["owned"] > 0, (case, total)
    # every region of the plain is claimed and every strip of it is owned: 4 x 3 regions, 19 strip rows in 150 px
    assert run["meta"]["giant_200x150/0/on"]["owned"] == {"owned": 4 * 19, "marked": 4 * 19}


def test_merged_row_scene_owns_fewer_strips_than_the_claimed_regions_hold(run, emulated):
    """mesa_333x200 view 4: a triangle drawn in place lies in front of the owner inside a claimed region (the emulation's older_wins),
    so strips of that region carry two ids and must go the long way; its owners are cut by the near plane (record kind 3).  View 3
    loses a bid."""
    v4, v3 = emulated[("mesa_333x200", 4)][0], emulated[("mesa_333x200", 3)][0]
    assert v4["older_wins"] > 0 and v4["won"] > 0 and v3["lost"] > 0
    got = run["meta"]["mesa_333x200/4/on"]["owned"]
    print("merged-row scene:", got, "claims", v4["won"])
    assert 0 < got["owned"] < got["marked"], got
    two = run["meta"]["mesa_333x200_two_views/2/on"]["owned"]      # the same view as the second of two
    assert 0 < two["owned"] < two["marked"], two
    assert run["meta"]["mesa_333x200/3/on"]["owned"]["owned"] > 0


def test_view_modes_and_surface_formats(run, topo, orc):
    scene, W, H, subs = OE.CASES[OW.MODE_CASE[0]]
    for mode in (1, 2):
        on, off = _frame(run, f"mode{mode}/on"), _frame(run, f"mode{mode}/off")
        assert_same_frame(on, off, f"view mode {mode}: owned strips on against off")
        assert_same_frame(on, _oracle(orc, topo, scene, W, H, subs[OW.MODE_CASE[1]][0], mode), f"view mode {mode}: owned strips on against the oracle")
        assert run["meta"][f"mode{mode}/on"]["owned"]["owned"] > 0
    scene, W, H, subs = OE.CASES[OW.FORMAT_CASE[0]]
    for fmt in (topo.FORMAT_BGRA8_UNORM_SRGB, topo.FORMAT_RGBA8_UNORM, topo.FORMAT_BGRA8_UNORM):
        on, off = _frame(run, f"format{fmt}/on"), _frame(run, f"format{fmt}/off")
        assert_same_frame(on, off, f"format {fmt}: owned strips on against off")
        assert_same_frame(on, _oracle(orc, topo, scene, W, H, subs[OW.FORMAT_CASE[1]][0], 0, fmt), f"format {fmt}: owned strips on against the oracle")
        assert run["meta"][f"format{fmt}/on"]["owned"]["owned"] > 0 and not run["meta"][f"format{fmt}/on"]["status"]["bounds_violation"]


def test_path_holds_with_frames_in_flight(run, oracle_frames):
    scene, W, H, subs = OE.CASES["mesa_333x200"]
    for j in range(2 * len(subs)):
        pose = subs[j % len(subs)][0]
        on, off = _frame(run, f"in_flight/{j}/on"), _frame(run, f"in_flight/{j}/off")
        assert_same_frame(on, oracle_frames[(scene, W, H, pose)], f"frame {j} in flight: owned strips on against the oracle")
        assert_same_frame(off, on, f"frame {j} in flight: owned strips off against on")
    assert run["meta"]["in_flight/on"]["status"]["status"] == 0 and not run["meta"]["in_flight/on"]["status"]["bounds_violation"]
    assert run["meta"]["in_flight/on"]["owned"]["owned"] > 0 and run["meta"]["in_flight/off"]["owned"]["owned"] == 0
