"""Peak labels (topo_label_layout, topo_labels_*) without a GPU: the layout rule of the built library (host_math.cpp over
topo_labels.h's occupancy grid), the g++ build of the same header (tests/labels_emul.py) and the independent edge-set reference
(tests/labels_ref.py, decided as the reference's process_label_layout decides) on the reference's own ten cases and on seeded random
layouts; the C ABI and its bindings; and the emulation's candidates against the oracle's visible peaks.  Everything is bit-exact:
the rule has no ambiguous cases, so nothing is excluded from a comparison."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import labels_cases as LC
import labels_emul as LE
import labels_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("topo_label_layout", "topo_labels_device", "topo_labels_read")


def _same(a, b, what):
    assert a.dtype == b.dtype == LR.LABEL_DTYPE and a.tobytes() == b.tobytes(), f"{what}: the records differ\n{a}\n{b}"


def test_reference_cases(topo):
    """The ten cases of the reference's test_layout (text_renderer.rs:382-431; tests/golden/label_layout_cases.json holds their
    numbers), as that test runs them -- line height 1, eight rows -- through topo_label_layout of the built library, the emulation and
    the edge-set reference: (floor(label_x), floor(label_y)) of every label equals the fixture."""
    cases = LC.golden_cases()
    assert len(cases) == 10
    for pos, wid, expected in cases:
        for name, fn in (("library", lambda x, w: topo.label_layout(x, w, 64, 1.0, 8)), ("emulation", lambda x, w: LE.layout(x, w, 64, 1.0, 8)),
                         ("reference", lambda x, w: LR.layout(x, w, 1.0, 8))):
            rows, out = fn(np.array(pos, np.uint32), np.array(wid, np.float32))
            got = [(int(np.floor(r["label_x"])), int(np.floor(r["label_y"]))) for r in out]
            assert got == expected, (name, pos, wid, got, expected)
            assert list(out["peak"]) == [0, 1, 2] and list(rows) == [e[1] for e in expected]


def test_random_layouts(topo):
    """The library, the emulation and the edge-set reference on 2000 seeded layouts; the seeds' conditions are confirmed with the
    reference alone."""
    layouts = LC.random_layouts()
    assert len(layouts) == 2000
    assert {l[0] for l in layouts} == set(LC.IMAGE_WIDTHS) and {l[1] for l in layouts} == set(LC.MAX_ROWS)
    assert {(l[0], l[1]) for l in layouts} == {(a, b) for a in LC.IMAGE_WIDTHS for b in LC.MAX_ROWS}
    placed = upper = dropped = usable = touching = 0
    seen_widths = set()
    for Wi, max_rows, x, w in layouts:
        r_rows, r_out = LR.layout(x, w, LC.ROW_HEIGHT, max_rows)
        placed += len(r_out)
        upper += int((r_out["row"] >= 1).sum())
        dropped += int((r_rows == -1).sum())
        usable += int((r_rows != -2).sum())
        touching += LC.touching_pairs(Wi, x, w)
        seen_widths |= {"zero" if v == 0 else "quarter" if v == 0.25 else "nan" if np.isnan(v) else "inf" if np.isinf(v) else "neg" if v < 0 else
                        "past" if int(xi) + v > Wi - 1 else "integral" if v == int(v) else "fraction" for xi, v in zip(x, w)}
        if (w > Wi).any() and np.isfinite(w[w > Wi]).any():
            seen_widths.add("over the image")
        if (np.isfinite(w) & (w > 64 * 32)).any():
            seen_widths.add("over 64 words")
        for name, (rows, out) in (("library", topo.label_layout(x, w, Wi, LC.ROW_HEIGHT, max_rows)), ("emulation", LE.layout(x, w, Wi, LC.ROW_HEIGHT, max_rows))):
            assert np.array_equal(rows, r_rows), (name, Wi, max_rows, x, w, rows, r_rows)
            _same(out, r_out, f"{name} Wi {Wi} rows {max_rows}")
    print(f"{placed} placed, {upper} in a row >= 1, {dropped} of {usable} usable dropped, {touching} touching pairs, widths {sorted(seen_widths)}")
    assert seen_widths == {"zero", "quarter", "integral", "fraction", "past", "nan", "inf", "neg", "over the image", "over 64 words"}
    assert 3 * upper >= placed and 20 * dropped >= usable and touching >= 100


@pytest.mark.parametrize("row_height", [20.0, 17.3])
def test_label_y_is_one_add_and_one_multiply(topo, row_height):
    x = np.full(64, 5, np.uint32)      # all at one column: label j lands in row j
    rows, out = topo.label_layout(x, np.full(64, 3.0, np.float32), 64, row_height, 64)
    assert list(rows) == list(range(64))
    want = np.array([np.float32(row_height) * (np.float32(0.5) + np.float32(k)) for k in range(64)], np.float32)
    assert out["label_y"].tobytes() == want.tobytes()
    assert LE.layout(x, np.full(64, 3.0, np.float32), 64, row_height, 64)[1]["label_y"].tobytes() == want.tobytes()
    assert (out["label_x"] == 5).all() and (out["peak_x"] == 5).all() and (out["peak_y"] == 0).all() and (out["view"] == 0).all() and (out["label_width"] == 3).all()


def test_abi_and_layouts(topo):
    k = LE.constants()
    assert (k["HIDDEN"], k["PLACED"], k["NO_ROW"], k["BAD_WIDTH"]) == (LR.HIDDEN, LR.PLACED, LR.NO_ROW, LR.BAD_WIDTH) == (0, 1, 2, 3)
    assert (topo.LABEL_HIDDEN, topo.LABEL_PLACED, topo.LABEL_NO_ROW, topo.LABEL_BAD_WIDTH) == (0, 1, 2, 3)
    assert k["MAX_ROWS"] == 64 and k["MAX_GRID_BITS"] == 524288 and k["LABEL_BYTES"] == 32
    assert topo.LABEL_DTYPE == LR.LABEL_DTYPE and topo.LABEL_DTYPE.itemsize == 32 and topo.LABEL_PARAMS_DTYPE.itemsize == 16
    assert [topo.LABEL_DTYPE.fields[f][1] for f in topo.LABEL_DTYPE.names] == [0, 4, 8, 12, 16, 20, 24, 28]
    assert [topo.LABEL_PARAMS_DTYPE.fields[f][1] for f in topo.LABEL_PARAMS_DTYPE.names] == [0, 4, 8, 12]
    p = topo.label_params(20.0, 8, 8, 100)
    assert (float(p["row_height"][0]), int(p["max_rows"][0]), int(p["views_per_image"][0]), int(p["cap"][0])) == (20.0, 8, 8, 100)
    # the header's own sizes, through a C compiler
    src = '#include "topo_hip.h"\n_Static_assert(sizeof(topo_label) == 32 && sizeof(topo_label_params) == 16, "size");\n' \
          '_Static_assert(__builtin_offsetof(topo_label, label_x) == 12 && __builtin_offsetof(topo_label, peak_y) == 28 && ' \
          '__builtin_offsetof(topo_label_params, cap) == 12, "offset");\n'
    res = subprocess.run(["gcc", "-std=c99", "-fsyntax-only", "-I", os.path.dirname(topo.HEADER_PATH), "-x", "c", "-"], input=src, capture_output=True, text=True)
    if res.returncode != 0 and "_Static_assert" in res.stderr:      # (a compiler that keeps _Static_assert to C11)
        res = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.dirname(topo.HEADER_PATH), "-x", "c", "-"], input=src, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    sys_src = open(os.path.join(ROOT, "rust", "topo-hip-sys", "src", "lib.rs")).read()
    assert "pub struct topo_label {" in sys_src and "pub struct topo_label_params {" in sys_src
    for s in SYMBOLS:
        assert hasattr(topo.lib(), s) and "pub fn " + s + "(" in sys_src
    for m in ("labels_device", "labels_read"):
        assert callable(getattr(topo.TerrainRenderer, m, None))


def test_label_calls_refuse_to_work_without_a_context(topo):
    """topo_labels_* need a context, and a context needs a GPU: without one topo_create fails with the project's usual error."""
    import torch
    L = topo.lib()
    p = topo.label_params(20.0, 8, 1, 4)
    u = np.zeros((1, 160), np.uint8)
    buf = np.zeros(64, np.uint32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.topo_labels_device(None, ptr(p), 1, ptr(u), 8, 8, ptr(buf), 256, 32, 0, None, None, ptr(buf), ptr(buf), None) == topo.TOPO_ERR_INVALID
    assert L.topo_labels_read(None, ptr(p), 1, ptr(u), 8, 8, ptr(buf), 256, 32, 0, None, None, ptr(buf), ptr(buf), None) == topo.TOPO_ERR_INVALID
    if not torch.cuda.is_available():
        with pytest.raises(topo.TopoError) as e:
            topo.TerrainRenderer(64, 64)
        assert e.value.code == topo.TOPO_ERR_HIP and "no CPU fallback" in str(e.value)


def test_layout_argument_errors(topo):
    L = topo.lib()
    x, w = np.array([1, 2, 3], np.uint32), np.array([1, 1, 1], np.float32)
    rows, out = np.full(3, 99, np.int32), np.zeros(3, topo.LABEL_DTYPE)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    call = lambda n, xs, ws, Wi, max_rows, ro, o: L.topo_label_layout(n, xs, ws, Wi, 20.0, max_rows, ro, o)
    assert call(3, ptr(x), ptr(w), 64, 8, ptr(rows), None) == 3 and list(rows) == [0, 1, 0]      # out is optional; [1, 2], [2, 3] touch, [3, 4] is free of [1, 2]
    assert call(0, None, None, 64, 8, None, None) == 0
    for bad in ((3, None, ptr(w), 64, 8, ptr(rows), ptr(out)), (3, ptr(x), None, 64, 8, ptr(rows), ptr(out)), (3, ptr(x), ptr(w), 64, 8, None, ptr(out)),
                (3, ptr(x), ptr(w), 0, 8, ptr(rows), ptr(out)), (3, ptr(x), ptr(w), 64, 0, ptr(rows), ptr(out)), (3, ptr(x), ptr(w), 3, 8, ptr(rows), ptr(out))):
        rows[:] = 99
        assert call(*bad) == topo.TOPO_ERR_INVALID and (rows == 99).all(), bad
    assert call(3, ptr(x), ptr(w), 64, 65, ptr(rows), ptr(out)) == topo.TOPO_ERR_UNSUPPORTED
    assert call(3, ptr(x), ptr(w), 8193, 64, ptr(rows), ptr(out)) == topo.TOPO_ERR_UNSUPPORTED and (rows == 99).all()
    assert call(3, ptr(x), ptr(w), 8192, 64, ptr(rows), ptr(out)) == 3      # Wi * max_rows = 524288: the limit itself
    assert call(3, ptr(x), ptr(w), 524288, 1, ptr(rows), ptr(out)) == 2 and list(rows) == [0, -1, 0]      # one row: the middle label touches the first
    with pytest.raises(topo.TopoError) as e:
        topo.label_layout(x, w, 64, 20.0, 65)
    assert e.value.code == topo.TOPO_ERR_UNSUPPORTED
    with pytest.raises(topo.TopoError) as e:
        topo.label_layout(x, w, 2, 20.0, 8)
    assert e.value.code == topo.TOPO_ERR_INVALID


def test_emulation_candidates_are_the_oracles_visible_peaks(orc):
    """Scene(96, 2, 2, eye_dh=300) at 200 x 120, rendered view by view with the oracle: with one view per image the emulation's
    candidates are exactly oracle.visible_peaks on random_peaks(sc, 1500), and so are the numpy reference's."""
    depth, seen = LC.oracle_strip()
    pk, w = LC.peaks(), np.full(LC.N_PEAKS, 10.0, np.float32)
    P = LC.projs(LC.views())
    out, counts, state = LE.labels(P, depth, pk, w, LC.SW, LC.SH, 1, LC.ROW_HEIGHT, 64, LC.N_PEAKS)
    total = 0
    for v, (vis, xy) in enumerate(seen):
        assert np.array_equal(state[v] != 0, vis), f"view {v}"
        got = np.zeros((LC.N_PEAKS, 2), np.uint32)
        recs = out[v][:counts[v]]
        got[recs["peak"], 0], got[recs["peak"], 1] = recs["peak_x"].astype(np.uint32), recs["peak_y"].astype(np.uint32)
        placed = state[v] == LR.PLACED
        assert np.array_equal(got[placed], xy[placed]) and (recs["view"] == 0).all()
        found, view, xs, ys = LR.candidates(P[v:v + 1], depth[v:v + 1], pk, LC.SW, LC.SH)
        assert np.array_equal(found, vis) and np.array_equal(np.stack([xs, ys], -1)[vis], xy[vis].astype(np.int64))
        total += int(vis.sum())
    assert total > 10


def test_panorama_scene_meets_the_gpu_tests_conditions(orc):
    """What tests/test_labels_gpu.py asks of its views-per-image-8 scene, confirmed here with the oracle's depth and the emulation:
    at least 60 labels from at least 6 of the 8 views, at least 10 in a row >= 1, a label whose span crosses a view seam, and with two
    rows at least 10 peaks without a free row.  The emulation and the edge-set reference agree on all of it."""
    depth, _ = LC.oracle_strip()
    pk, w, P = LC.peaks(), LC.widths(), LC.projs(LC.views())
    for max_rows in (8, 2):
        out, counts, state = LE.labels(P, depth, pk, w, LC.SW, LC.SH, 8, LC.ROW_HEIGHT, max_rows, LC.N_PEAKS)
        (r_out, r_state), = LR.labels(P, depth, pk, w, LC.SW, LC.SH, 8, LC.ROW_HEIGHT, max_rows)
        recs = out[0][:counts[0]]
        _same(recs, r_out, f"strip, {max_rows} rows")
        assert np.array_equal(state[0], r_state)
        seam = int((recs["peak_x"].astype(np.int64) // LC.SW != np.minimum(np.ceil(recs["peak_x"] + recs["label_width"]), 8 * LC.SW - 1).astype(np.int64) // LC.SW).sum())
        print(f"{max_rows} rows: {len(recs)} labels from views {sorted(set(recs['view'].tolist()))}, {int((recs['row'] >= 1).sum())} in a row >= 1, "
              f"{int((state[0] == LR.NO_ROW).sum())} without a row, {int((state[0] == LR.BAD_WIDTH).sum())} with a bad width, {seam} across a seam")
        if max_rows == 8:
            assert len(recs) >= 60 and len(set(recs["view"].tolist())) >= 6 and (recs["row"] >= 1).sum() >= 10 and seam >= 1
            assert (state[0] == LR.BAD_WIDTH).sum() >= 1
        else:
            assert (state[0] == LR.NO_ROW).sum() >= 10
