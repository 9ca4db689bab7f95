"""The covered-region path on the CPU (tests/cover_emul.cpp over topo_pipeline.h): item_covers_region against its definition by brute
force, every lane of big_cover_lane under a bounds-checking sink against triangle_pixel, and the near phase of the GPU tests' scenes
as the kernels order it -- which says, without a GPU, which of those scenes have a lost claim, a merged row in which an older key
wins, and rows stored blind."""
import numpy as np
import pytest

import cover_emul as CE

SIZES = ((333, 200), (640, 480))


def _regions(W, H):
    return [(rx, ry) for ry in range((H + 63) // 64) for rx in range((W + 63) // 64)]


def _tri(rng, W, H, scale):
    """A random front-facing triangle (1/256 px) about the target, `scale` target sizes across."""
    c = rng.uniform(-0.2, 1.2, 2) * (W, H)
    p = c + rng.normal(0.0, scale * max(W, H), (3, 2))
    X, Y = np.rint(p[:, 0] * 256).astype(np.int64), np.rint(p[:, 1] * 256).astype(np.int64)
    if (X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0]) >= 0:      # front face: negative doubled area
        X[[1, 2]], Y[[1, 2]] = X[[2, 1]], Y[[2, 1]]
    return X.astype(np.int32), Y.astype(np.int32)


@pytest.mark.parametrize("W,H", SIZES)
def test_item_covers_region_is_the_brute_force_definition(W, H):
    rng = np.random.default_rng(W)
    n_true = 0
    for scale in (0.15, 0.4, 1.0, 3.0, 40.0):
        for _ in range(120):
            X, Y = _tri(rng, W, H, scale)
            for rx, ry in _regions(W, H):
                got, want = CE.covers(X, Y, W, H, rx, ry), CE.covers_brute(X, Y, W, H, rx, ry)
                assert got == want, (X.tolist(), Y.tolist(), rx, ry, got, want)
                n_true += got
    assert n_true > 200, n_true      # both answers are exercised
    # regions outside the target, a back face, a degenerate triangle: never
    big = next((X, Y) for X, Y in (_tri(rng, W, H, 40.0) for _ in range(200)) if CE.covers(X, Y, W, H, 0, 0))
    assert not CE.covers(*big, W, H, (W + 63) // 64, 0) and not CE.covers(*big, W, H, 0, (H + 63) // 64) and not CE.covers(*big, W, H, -1, 0)
    assert not CE.covers(big[0][[0, 2, 1]], big[1][[0, 2, 1]], W, H, 0, 0)
    assert not CE.covers(np.array([0, 256, 512], np.int32), np.array([0, 256, 512], np.int32), W, H, 0, 0)


@pytest.mark.parametrize("W,H", SIZES)
def test_fill_rule_and_one_sub_pixel_misses(W, H):
    """Edges that run exactly through pixel centres (a left edge owns them, a right or bottom edge does not), and triangles that
    miss one corner pixel of a region by one sub-pixel."""
    cx = lambda p: 256 * p + 128
    last_rx, last_ry = (W - 1) // 64, (H - 1) // 64
    for rx, ry in ((0, 0), (1, 1), (last_rx, 0), (0, last_ry), (last_rx, last_ry)):
        x0, y0 = rx * 64, ry * 64
        x1, y1 = min(x0 + 63, W - 1), min(y0 + 63, H - 1)
        n = 4 * 64
        # legs on the centres of column x0 (a left edge: owned) and row y0 (a top edge: owned), hypotenuse far away
        X = np.array([cx(x0), cx(x0), cx(x0 + n)], np.int32)
        Y = np.array([cx(y0), cx(y0 + n), cx(y0)], np.int32)
        assert CE.covers_brute(X, Y, W, H, rx, ry) and CE.covers(X, Y, W, H, rx, ry)
        for dX, dY in (((1, 1, 0), (0, 0, 0)), ((0, 0, 0), (1, 0, 1))):      # the leg one sub-pixel inside: column x0 / row y0 is lost
            Xs, Ys = X + np.array(dX, np.int32), Y + np.array(dY, np.int32)
            assert not CE.covers_brute(Xs, Ys, W, H, rx, ry) and not CE.covers(Xs, Ys, W, H, rx, ry)
        # mirrored: legs on the centres of column x1 (a right edge) and row y1 (a bottom edge) are NOT owned ...
        X = np.array([cx(x1), cx(x1), cx(x1 - n)], np.int32)
        Y = np.array([cx(y1), cx(y1 - n), cx(y1)], np.int32)
        assert not CE.covers_brute(X, Y, W, H, rx, ry) and not CE.covers(X, Y, W, H, rx, ry)
        Xs, Ys = X + np.array((1, 1, 0), np.int32), Y + np.array((1, 0, 1), np.int32)      # ... one sub-pixel further out they hold the centres
        assert CE.covers_brute(Xs, Ys, W, H, rx, ry) and CE.covers(Xs, Ys, W, H, rx, ry)
        for dX, dY in (((1, 1, 0), (0, 0, 0)), ((0, 0, 0), (1, 0, 1))):      # only one of the two legs moved out: the other still misses
            Xs, Ys = X + np.array(dX, np.int32), Y + np.array(dY, np.int32)
            assert not CE.covers_brute(Xs, Ys, W, H, rx, ry) and not CE.covers(Xs, Ys, W, H, rx, ry)
        # the hypotenuse (x + y = S: neither a left nor a top edge, so it does not own its centres) through the centre of the
        # region's far corner pixel, and one sub-pixel either side: the corner pixel is missed, covered, missed
        for shift, want in ((0, False), (1, True), (-1, False)):
            X = np.array([cx(x0) - 5, cx(x0) - 5, cx(x1) + (cx(y1) - cx(y0)) + 5 + shift], np.int32)
            Y = np.array([cx(y0) - 5, cx(y1) + (cx(x1) - cx(x0)) + 5 + shift, cx(y0) - 5], np.int32)
            assert CE.covers_brute(X, Y, W, H, rx, ry) == want and CE.covers(X, Y, W, H, rx, ry) == want, (rx, ry, shift)


def _check_item(X, Y, z, W, H, rx, ry, covering):
    r = CE.cover_item(X, Y, z, 0x1234567, W, H, rx, ry)
    assert r["violations"] == 0, (X.tolist(), Y.tolist(), rx, ry, r["violations"])
    if covering:      # every pixel exactly once, with triangle_pixel's key
        assert r["missing"] == 0 and r["wrong"] == 0, (X.tolist(), Y.tolist(), rx, ry, r["missing"], r["wrong"])
    return r["fragments"]


@pytest.mark.parametrize("W,H", SIZES)
def test_every_lane_of_the_cover_walk_under_the_checking_sink(W, H):
    """Random triangles, covering and not: no index outside the region or the target, no pixel twice; covering ones: every pixel
    of the region inside the target exactly once, keys = vis_key(triangle_pixel)."""
    rng = np.random.default_rng(H)
    n_cover = n_frag = 0
    for scale in (0.4, 1.0, 3.0, 40.0):
        for _ in range(40):
            X, Y = _tri(rng, W, H, scale)
            z = rng.uniform(0.0, 0.999, 3).astype(np.float32)
            for rx, ry in _regions(W, H):
                cov = CE.covers(X, Y, W, H, rx, ry)
                n = _check_item(X, Y, z, W, H, rx, ry, cov)
                if cov:
                    n_cover += 1
                    n_frag += n
                    assert n == (min(rx * 64 + 63, W - 1) - rx * 64 + 1) * (min(ry * 64 + 63, H - 1) - ry * 64 + 1)
    assert n_cover > 100, n_cover


@pytest.mark.parametrize("W,H", SIZES)
def test_cover_walk_depths_above_and_below_the_narrow_limit_and_at_the_planes(W, H):
    """Triangles whose doubled area is below and above 2^48 (the two int64 -> f32 conversions), vertices from a near-plane cut
    (z = 0 exactly), depths that cross 1 (the far plane clips those pixels) and that dip below 0 (clamped)."""
    rng = np.random.default_rng(7)
    seen = {"narrow": 0, "wide": 0, "clipped": 0}
    for half_px, name in ((3000, "narrow"), (20000, "narrow"), (39000, "narrow"), (45000, "wide"), (300000, "wide"), (1000000, "wide")):
        for k in range(12):
            c = rng.uniform(0.0, 1.0, 2) * (W, H)
            ang = rng.uniform(0, 2 * np.pi) + np.array([0.0, 2.1, 4.2])
            p = c + half_px * np.stack([np.cos(ang), np.sin(ang)], 1)
            X, Y = np.rint(p[:, 0] * 256).astype(np.int64), np.rint(p[:, 1] * 256).astype(np.int64)
            area2 = (X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0])
            if area2 >= 0:
                X[[1, 2]], Y[[1, 2]] = X[[2, 1]], Y[[2, 1]]
                area2 = -area2
            assert (-area2 < 2 ** 48) == (name == "narrow"), (half_px, area2)
            assert np.abs(X).max() < 2 ** 28 and np.abs(Y).max() < 2 ** 28      # inside the guard band
            X, Y = X.astype(np.int32), Y.astype(np.int32)
            z = [np.array([0.0, 0.7, 0.9993], np.float32), np.array([0.0, 0.0, 0.5], np.float32),      # near-plane cut: fan vertices at z = 0
                 np.array([0.9, 1.0, 1.1], np.float32) if k % 8 < 4 else np.array([-0.1, 0.0, 0.1], np.float32),      # the depth crosses 1 / 0 about the target's middle
                 rng.uniform(0, 1, 3).astype(np.float32)][k % 4]
            for rx, ry in _regions(W, H):
                if CE.covers(X, Y, W, H, rx, ry):
                    n = _check_item(X, Y, z, W, H, rx, ry, True)
                    seen[name] += 1
                    full = (min(rx * 64 + 63, W - 1) - rx * 64 + 1) * (min(ry * 64 + 63, H - 1) - ry * 64 + 1)
                    seen["clipped"] += n < full
    assert seen["narrow"] > 20 and seen["wide"] > 20 and seen["clipped"] > 0, seen


# ---- the scenes of tests/test_cover_gpu.py, as the kernels order their near phase ---------------------------------------------

@pytest.fixture(scope="module")
def frames(topo):
    out = {}
    for name, (scene, W, H, subs) in CE.CASES.items():
        sc = CE.case_scene(scene)
        for i, sub in enumerate(subs):
            for k, pose in enumerate(sub):
                out[(name, i, k)] = CE.cover_frame(topo, sc, W, H, sc.uniforms(W, H, *pose, 0), key_base=k * W * H)
    return out


def test_cover_order_gives_the_plain_minimum_on_every_scene(frames):
    for key, st in frames.items():
        assert st["violations"] == 0 and st["blind_dirty"] == 0 and st["differ"] == 0, (key, st)
        assert st["candidates"] == st["won"] + st["lost"], (key, st)


def test_the_scenes_exercise_every_branch(frames):
    """What tests/test_cover_gpu.py relies on: claims won, a lost claim (two covering triangles on one region), a claimed region
    in which an older key wins a pixel (the merged-row path with a real minimum), rows stored blind -- and views of a second
    view whose keys do not start on a segment boundary."""
    def case(name, view=None):
        return {k: sum(st[k] for key, st in frames.items() if key[0] == name and view in (None, key[2])) for k in CE.STAT_NAMES}
    for name in CE.CASES:      # case by case: none may lose what it is there for while another keeps it
        st = case(name)
        if name.startswith("coarse"):
            assert st["candidates"] == 0 and st["big_items"] > 50, (name, st)      # big items, and none of them covers a region
        else:
            assert st["won"] > 0 and st["lost"] > 0 and st["rows_blind"] > 0, (name, st)
    for name in ("mesa_333x200", "mesa_333x200_two_views"):
        st = case(name)
        assert st["older_wins"] > 0 and st["rows_merged"] > 0, (name, st)
    second = case("mesa_333x200_two_views", view=1)      # the view whose keys do not start on a segment boundary
    assert second["won"] > 0 and second["lost"] > 0 and second["older_wins"] > 0 and second["rows_blind"] > 0 and second["rows_merged"] > 0, second
    for name, (_, W, H, subs) in CE.CASES.items():
        if any(len(s) > 1 for s in subs):
            assert (W * H) % 64 != 0, name
