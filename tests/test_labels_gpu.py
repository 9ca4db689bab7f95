"""Peak labels on the GPU (topo_labels_device / topo_labels_read: k_labels) on the scene of test_visible_peaks_device_entry_point --
Scene(96, 2, 2, eye_dh=300), an 8-view panorama at 200 x 120 from yaw 33 degrees, the reference's pad_256 depth pitch, 1500 random
peaks, widths in [20, 90] with a few of 0, of 2000 and bad ones (tests/labels_cases.py).

Comparison rule: bit-exact, nothing excluded.  The labels (the first min(count, cap) records of every image), the counts and the state
bytes equal the g++ build of the same header over the device's own depth (tests/labels_emul.py) and the independent edge-set
reference (tests/labels_ref.py); with one view per image they also equal topo_visible_peaks_device composed with topo_label_layout.
Whatever lies behind an image's records and behind the outputs keeps its 0xAB fill."""
import hashlib

import numpy as np
import pytest

import labels_cases as LC
import labels_emul as LE
import labels_ref as LR
from gpu_support import checked_run, padded_device_output

pytestmark = pytest.mark.gpu

FILL = 0xAB


class Strip:
    """A renderer over the scene and one submission of `views` at SW x SH with the pad_256 depth pitch, everything on the device."""

    def __init__(self, T, views):
        import torch
        self.T, self.views = T, views
        self.g = T.TerrainRenderer(LC.SW, LC.SH)
        LC.scene().load(self.g)
        n = len(views)
        self.pitch = T.pad_256(4 * LC.SW)
        self.rgba = torch.zeros((n, LC.SH, LC.SW, 4), dtype=torch.uint8, device="cuda")
        self.depth = torch.zeros((n, LC.SH, self.pitch // 4), dtype=torch.float32, device="cuda")
        self.g.set_stream(torch.cuda.current_stream().cuda_stream)
        self.g.render_views_device(views, LC.SW, LC.SH, self.rgba.data_ptr(), LC.SH * LC.SW * 4, LC.SW * 4, self.depth.data_ptr(), LC.SH * self.pitch, self.pitch)
        torch.cuda.synchronize()
        self.depth_host = self.depth.cpu().numpy()
        self.projs = LC.projs(views)
        self.d_peaks = torch.from_numpy(LC.peaks()).cuda()
        self.d_widths = torch.from_numpy(LC.widths()).cuda()

    def close(self):
        self.g.close()


def run(T, g, views, depth, pitch, d_peaks, d_widths, n_peaks, vpi, max_rows, cap, row_height=LC.ROW_HEIGHT, want_state=True, sw=LC.SW, sh=LC.SH):
    """topo_labels_device into 0xAB-filled tensors with spare room behind -> ((images, cap) records as raw LABEL_DTYPE, (images,)
    counts, (images, n_peaks) states or None); the spare room must keep its fill."""
    import torch
    images = len(views) // vpi
    labels = torch.full(((images * cap + 2) * 32,), FILL, dtype=torch.uint8, device="cuda")
    counts = torch.full(((images + 2) * 4,), FILL, dtype=torch.uint8, device="cuda")
    state = torch.full((images * n_peaks + 7,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    g.labels_device(T.label_params(row_height, max_rows, vpi, cap), views, sw, sh, depth.data_ptr(), n_peaks, d_peaks.data_ptr(), d_widths.data_ptr(),
                    labels.data_ptr(), counts.data_ptr(), state.data_ptr() if want_state else 0, depth_view_stride=sh * pitch, depth_pitch=pitch)
    g.synchronize()
    lab, cnt, st = labels.cpu().numpy(), counts.cpu().numpy(), state.cpu().numpy()
    assert (lab[images * cap * 32:] == FILL).all() and (cnt[images * 4:] == FILL).all() and (st[images * n_peaks if want_state else 0:] == FILL).all(), "written past an output"
    return (lab[:images * cap * 32].copy().view(LR.LABEL_DTYPE).reshape(images, cap), cnt[:images * 4].copy().view(np.uint32),
            st[:images * n_peaks].reshape(images, n_peaks).copy() if want_state else None)


def expect(projs, depth_host, n_peaks, vpi, max_rows, cap, row_height=LC.ROW_HEIGHT, sw=LC.SW, sh=LC.SH, peaks=None, widths=None):
    pk = LC.peaks()[:n_peaks] if peaks is None else peaks
    w = LC.widths()[:n_peaks] if widths is None else widths
    return LE.labels(projs, depth_host, pk, w, sw, sh, vpi, row_height, max_rows, cap)


def same(got, want, cap, what):
    """Device outputs against the emulation's: counts, states, and the first min(count, cap) records of every image; the rest of an
    image's block keeps its fill."""
    (g_lab, g_cnt, g_st), (e_lab, e_cnt, e_st) = got, want
    assert np.array_equal(g_cnt, e_cnt), f"{what}: counts {g_cnt} vs {e_cnt}"
    if g_st is not None:
        bad = np.argwhere(g_st != e_st)
        assert len(bad) == 0, f"{what}: {len(bad)} states differ, first (image, peak) {tuple(bad[0])}: {g_st[tuple(bad[0])]} vs {e_st[tuple(bad[0])]}"
    for i in range(len(g_cnt)):
        n = min(int(g_cnt[i]), cap)
        assert g_lab[i, :n].tobytes() == e_lab[i, :n].tobytes(), f"{what}: image {i}: the records differ\n{g_lab[i, :n]}\n{e_lab[i, :n]}"
        assert (g_lab[i, n:].view(np.uint8) == FILL).all(), f"{what}: image {i}: records behind the count were written"


def same_as_reference(got, projs, depth_host, n_peaks, vpi, max_rows, cap, what, sw=LC.SW, sh=LC.SH, peaks=None, widths=None):
    pk = LC.peaks()[:n_peaks] if peaks is None else peaks
    w = LC.widths()[:n_peaks] if widths is None else widths
    ref = LR.labels(projs, depth_host, pk, w, sw, sh, vpi, LC.ROW_HEIGHT, max_rows)
    g_lab, g_cnt, g_st = got
    for i, (r_lab, r_st) in enumerate(ref):
        assert int(g_cnt[i]) == len(r_lab) and np.array_equal(g_st[i], r_st), f"{what}: image {i} against the edge-set reference"
        n = min(len(r_lab), cap)
        assert g_lab[i, :n].tobytes() == r_lab[:n].tobytes(), f"{what}: image {i}: records differ from the edge-set reference"


@pytest.fixture(scope="module")
def S(topo):
    s = Strip(topo, LC.views())
    yield s
    s.close()


def test_one_view_per_image_is_visible_peaks_then_label_layout(topo, S):
    import torch
    n, cap = LC.N_PEAKS, 400
    got = run(topo, S.g, S.views, S.depth, S.pitch, S.d_peaks, S.d_widths, n, 1, 8, cap)
    same(got, expect(S.projs, S.depth_host, n, 1, 8, cap), cap, "one view per image")
    same_as_reference(got, S.projs, S.depth_host, n, 1, 8, cap, "one view per image")
    lab, cnt, st = got
    d_vis = torch.zeros(n, dtype=torch.uint8, device="cuda")
    d_xy = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
    w = LC.widths()
    seen = 0
    for v in range(8):
        S.g.visible_peaks_device(S.views[v], LC.SW, LC.SH, S.depth[v].data_ptr(), S.pitch, n, S.d_peaks.data_ptr(), d_vis.data_ptr(), d_xy.data_ptr())
        torch.cuda.synchronize()
        vis, xy = d_vis.cpu().numpy().astype(bool), d_xy.cpu().numpy().view(np.uint32)
        assert np.array_equal(st[v] != 0, vis), f"view {v}: state != 0 is topo_visible_peaks_device's byte"
        idx = np.flatnonzero(vis)
        rows, out = topo.label_layout(xy[idx, 0], w[idx], LC.SW, LC.ROW_HEIGHT, 8)
        want = out.copy()
        want["peak"], want["peak_y"] = idx[out["peak"]], xy[idx[out["peak"]], 1].astype(np.float32)
        assert int(cnt[v]) == len(want) <= cap and lab[v, :len(want)].tobytes() == want.tobytes(), f"view {v}: the composition of the two calls"
        want_state = np.zeros(n, np.uint8)
        want_state[idx] = np.where(rows >= 0, LR.PLACED, np.where(rows == -1, LR.NO_ROW, LR.BAD_WIDTH))
        assert np.array_equal(st[v], want_state)
        seen += int(vis.sum())
    assert seen > 100


@pytest.mark.parametrize("max_rows", [8, 2])
def test_strip_of_eight_views_is_one_image(topo, S, max_rows):
    n, cap = LC.N_PEAKS, 400
    got = run(topo, S.g, S.views, S.depth, S.pitch, S.d_peaks, S.d_widths, n, 8, max_rows, cap)
    same(got, expect(S.projs, S.depth_host, n, 8, max_rows, cap), cap, f"strip, {max_rows} rows")
    same_as_reference(got, S.projs, S.depth_host, n, 8, max_rows, cap, f"strip, {max_rows} rows")
    lab, cnt, st = got
    recs = lab[0, :cnt[0]]
    seam = int((recs["peak_x"].astype(np.int64) // LC.SW != np.minimum(np.ceil(recs["peak_x"] + recs["label_width"]), 8 * LC.SW - 1).astype(np.int64) // LC.SW).sum())
    print(f"{max_rows} rows: {len(recs)} labels, views {sorted(set(recs['view'].tolist()))}, {int((recs['row'] >= 1).sum())} in a row >= 1, "
          f"{int((st[0] == LR.NO_ROW).sum())} without a row, {seam} across a seam")
    if max_rows == 8:
        assert len(recs) >= 60 and len(set(recs["view"].tolist())) >= 6 and (recs["row"] >= 1).sum() >= 10 and seam >= 1
    else:
        assert (st[0] == LR.NO_ROW).sum() >= 10
    # a row height whose product with 0.5 + k is not exact: label_y is one f32 add and one f32 multiply, not a fused one
    odd = run(topo, S.g, S.views, S.depth, S.pitch, S.d_peaks, S.d_widths, n, 8, max_rows, cap, row_height=17.3)
    same(odd, expect(S.projs, S.depth_host, n, 8, max_rows, cap, row_height=17.3), cap, f"strip, {max_rows} rows of 17.3")
    k = odd[0][0, :cnt[0]]["row"]
    assert odd[0][0, :cnt[0]]["label_y"].tobytes() == (np.float32(17.3) * (np.float32(0.5) + k.astype(np.float32))).astype(np.float32).tobytes()
    shown = LC.widths()[st[0] != 0]      # the widths the layout met: bad ones, zero ones and ones wider than the image among them
    assert (st[0] == LR.BAD_WIDTH).sum() >= 1 and (shown == 0).any() and (shown == 2000).any()


@pytest.mark.parametrize("n_peaks", [1, 63, 64, 65, 257])
def test_chunk_edges(topo, S, n_peaks):
    for vpi in (8, 1):
        got = run(topo, S.g, S.views, S.depth, S.pitch, S.d_peaks, S.d_widths, n_peaks, vpi, 8, 64)
        same(got, expect(S.projs, S.depth_host, n_peaks, vpi, 8, 64), 64, f"{n_peaks} peaks, {vpi} views per image")


def test_no_peaks_and_no_room(topo, S):
    """No peaks: every count is 0.  cap = 0: the counts and states are the full ones and no record is written (labels may be null)."""
    import torch
    for vpi in (8, 1):
        lab, cnt, st = run(topo, S.g, S.views, S.depth, S.pitch, S.d_peaks, S.d_widths, 0, vpi, 8, 4)
        assert (cnt == 0).all() and (lab.view(np.uint8) == FILL).all()
    n = 300
    e_lab, e_cnt, e_st = expect(S.projs, S.depth_host, n, 8, 8, 0)
    same(run(topo, S.g, S.views, S.depth, S.pitch, S.d_peaks, S.d_widths, n, 8, 8, 0), (e_lab, e_cnt, e_st), 0, "cap 0")
    counts = torch.zeros(1, dtype=torch.int32, device="cuda")
    S.g.labels_device(topo.label_params(LC.ROW_HEIGHT, 8, 8, 0), S.views, LC.SW, LC.SH, S.depth.data_ptr(), n, S.d_peaks.data_ptr(), S.d_widths.data_ptr(), 0,
                      counts.data_ptr(), 0, depth_view_stride=LC.SH * S.pitch, depth_pitch=S.pitch)
    S.g.synchronize()
    assert int(counts.cpu().numpy()[0]) == int(e_cnt[0]) > 0


def test_cap_smaller_than_the_count(topo, S):
    n, cap = LC.N_PEAKS, 17
    e_lab, e_cnt, e_st = expect(S.projs, S.depth_host, n, 8, 8, cap)
    assert e_cnt[0] > cap
    same(run(topo, S.g, S.views, S.depth, S.pitch, S.d_peaks, S.d_widths, n, 8, 8, cap), (e_lab, e_cnt, e_st), cap, "cap 17")
    # per view: eight blocks of cap records, two more behind them
    import torch
    counts = torch.zeros(8, dtype=torch.int32, device="cuda")
    e1_lab, e1_cnt, _ = expect(S.projs, S.depth_host, n, 1, 8, 5)
    vals, pad = padded_device_output(S.g, 1, 8, 5, 32, lambda p, stride, pitch: S.g.labels_device(
        topo.label_params(LC.ROW_HEIGHT, 8, 1, 5), S.views, LC.SW, LC.SH, S.depth.data_ptr(), n, S.d_peaks.data_ptr(), S.d_widths.data_ptr(), p, counts.data_ptr(), 0,
        depth_view_stride=LC.SH * S.pitch, depth_pitch=S.pitch), pad_rows=2)
    assert (pad == FILL).all() and len(pad) == 2 * 5 * 32
    got_cnt = counts.cpu().numpy().view(np.uint32)
    assert np.array_equal(got_cnt, e1_cnt) and (got_cnt > 5).any()
    lab = vals.reshape(8, 5 * 32).copy().view(LR.LABEL_DTYPE)
    for v in range(8):
        k = min(int(got_cnt[v]), 5)
        assert lab[v, :k].tobytes() == e1_lab[v, :k].tobytes() and (lab[v, k:].view(np.uint8) == FILL).all()


def test_several_images_in_one_call(topo):
    """Three viewpoints x 8 views in one submission: 3 images of 8 views, 24 (and 23) images of one view -- image counts that do not
    fill the last workgroup; every image equals its own single-image call."""
    views = [u for yaw in (33.0, 100.0, 211.0) for u in LC.views(yaw)]
    s = Strip(topo, views)
    try:
        n, cap = 700, 200
        for vpi, n_views in ((8, 24), (1, 24), (1, 23)):
            vs = views[:n_views]
            got = run(topo, s.g, vs, s.depth, s.pitch, s.d_peaks, s.d_widths, n, vpi, 8, cap)
            same(got, expect(s.projs[:n_views], s.depth_host[:n_views], n, vpi, 8, cap), cap, f"{n_views} views, {vpi} per image")
            for i in range(n_views // vpi):
                one = run(topo, s.g, vs[i * vpi:(i + 1) * vpi], s.depth[i * vpi:], s.pitch, s.d_peaks, s.d_widths, n, vpi, 8, cap)
                k = int(one[1][0])
                assert k == int(got[1][i]) and one[0][0, :min(k, cap)].tobytes() == got[0][i, :min(k, cap)].tobytes() and np.array_equal(one[2][0], got[2][i]), (vpi, i)
            if vpi == 8:
                assert (got[1] >= 30).all() and len({bytes(got[2][i]) for i in range(3)}) == 3
    finally:
        s.close()


def test_overlapping_views_label_every_peak_in_the_first(topo, S):
    import torch
    n, cap = LC.N_PEAKS, 300
    for v in (0, 5):
        depth2 = torch.stack([S.depth[v], S.depth[v]]).contiguous()
        got = run(topo, S.g, [S.views[v], S.views[v]], depth2, S.pitch, S.d_peaks, S.d_widths, n, 2, 8, cap)
        one = run(topo, S.g, [S.views[v]], S.depth[v:], S.pitch, S.d_peaks, S.d_widths, n, 1, 8, cap)
        k = int(got[1][0])
        assert k >= 5 and (got[0][0, :k]["view"] == 0).all() and (got[0][0, :k]["peak_x"] < LC.SW).all()
        assert np.array_equal(got[2][0] != 0, one[2][0] != 0), "the same peaks show"
        same(got, expect(np.stack([S.projs[v]] * 2), np.stack([S.depth_host[v]] * 2), n, 2, 8, cap), cap, f"view {v} twice")


def test_grid_limits(topo, S):
    """Wi * max_rows = 524288 exactly: one view of 8192 x 4 and 64 rows over a synthetic depth at the far value (every peak inside the
    frustum shows), 65 peaks that do, half of them wider than the image so that the rows fill.  One column more is TOPO_ERR_UNSUPPORTED
    and writes nothing."""
    import torch
    W, H, rows = 8192, 4, 64
    view, P = [S.views[0]], S.projs[:1]
    far = np.ones((1, H, W + 1), np.float32)
    found = LR.candidates(P, far, LC.peaks(), W, H)[0]
    idx = np.flatnonzero(found)[:65]
    assert len(idx) == 65
    pk = np.ascontiguousarray(LC.peaks()[idx])
    w = LC.widths()[idx].copy()
    w[::2] = 9000.0
    d_far, d_pk, d_w = torch.from_numpy(far).cuda(), torch.from_numpy(pk).cuda(), torch.from_numpy(w).cuda()
    pitch = 4 * (W + 1)
    got = run(topo, S.g, view, d_far, pitch, d_pk, d_w, 65, 1, rows, 65, sw=W, sh=H)
    same(got, expect(P, far, 65, 1, rows, 65, sw=W, sh=H, peaks=pk, widths=w), 65, "at the grid limit")
    same_as_reference(got, P, far, 65, 1, rows, 65, "at the grid limit", sw=W, sh=H, peaks=pk, widths=w)
    assert got[1][0] >= 33 and got[0][0, :got[1][0]]["row"].max() >= 30
    labels = torch.full((65 * 32,), FILL, dtype=torch.uint8, device="cuda")
    counts = torch.full((4,), FILL, dtype=torch.uint8, device="cuda")
    state = torch.full((65,), FILL, dtype=torch.uint8, device="cuda")
    for max_rows, width in ((rows, W + 1), (65, 64)):
        with pytest.raises(topo.TopoError) as e:
            S.g.labels_device(topo.label_params(LC.ROW_HEIGHT, max_rows, 1, 65), view, width, H, d_far.data_ptr(), 65, d_pk.data_ptr(), d_w.data_ptr(), labels.data_ptr(),
                              counts.data_ptr(), state.data_ptr(), depth_view_stride=H * pitch, depth_pitch=pitch)
        assert e.value.code == topo.TOPO_ERR_UNSUPPORTED
    S.g.synchronize()
    assert (labels.cpu().numpy() == FILL).all() and (counts.cpu().numpy() == FILL).all() and (state.cpu().numpy() == FILL).all()


def test_argument_errors(topo, S):
    import torch
    out = torch.zeros(64, dtype=torch.int32, device="cuda")
    ok = dict(params=topo.label_params(LC.ROW_HEIGHT, 8, 8, 4), views=S.views, w=LC.SW, h=LC.SH, depth=S.depth.data_ptr(), n=10, peaks=S.d_peaks.data_ptr(),
              widths=S.d_widths.data_ptr(), labels=out.data_ptr(), counts=out.data_ptr() + 128, state=0, stride=LC.SH * S.pitch, pitch=S.pitch)
    call = lambda a: S.g.labels_device(a["params"], a["views"], a["w"], a["h"], a["depth"], a["n"], a["peaks"], a["widths"], a["labels"], a["counts"], a["state"],
                                       depth_view_stride=a["stride"], depth_pitch=a["pitch"])
    call(ok)
    for change in (dict(params=topo.label_params(LC.ROW_HEIGHT, 0, 8, 4)), dict(params=topo.label_params(LC.ROW_HEIGHT, 8, 0, 4)),
                   dict(params=topo.label_params(LC.ROW_HEIGHT, 8, 3, 4)), dict(w=0), dict(h=0), dict(pitch=4 * LC.SW - 4), dict(stride=LC.SH * S.pitch - 1024),
                   dict(depth=0), dict(peaks=0), dict(widths=0), dict(labels=0), dict(counts=0)):
        with pytest.raises(topo.TopoError) as e:
            call(dict(ok, **change))
        assert e.value.code == topo.TOPO_ERR_INVALID, change
    S.g.synchronize()


def test_read_equals_the_device_call(topo, S):
    n, cap = LC.N_PEAKS, 90
    for vpi in (8, 1):
        dev = run(topo, S.g, S.views, S.depth, S.pitch, S.d_peaks, S.d_widths, n, vpi, 8, cap)
        lab, cnt, st = S.g.labels_read(topo.label_params(LC.ROW_HEIGHT, 8, vpi, cap), S.views, LC.SW, LC.SH, S.depth.data_ptr(), LC.peaks(), LC.widths(),
                                       depth_view_stride=LC.SH * S.pitch, depth_pitch=S.pitch)
        assert np.array_equal(cnt, dev[1]) and np.array_equal(st, dev[2])
        for i in range(len(cnt)):
            k = min(int(cnt[i]), cap)
            assert lab[i, :k].tobytes() == dev[0][i, :k].tobytes() and not lab[i, k:].view(np.uint8).any()


def test_the_frame_is_untouched(topo, S):
    import torch
    rgba, depth = S.rgba.clone(), S.depth.clone()
    before = S.g.frame_status()["status"]
    run(topo, S.g, S.views, S.depth, S.pitch, S.d_peaks, S.d_widths, LC.N_PEAKS, 8, 8, 100)
    S.g.labels_read(topo.label_params(LC.ROW_HEIGHT, 8, 1, 10), S.views, LC.SW, LC.SH, S.depth.data_ptr(), LC.peaks(), LC.widths(), depth_view_stride=LC.SH * S.pitch,
                    depth_pitch=S.pitch)
    torch.cuda.synchronize()
    assert torch.equal(rgba, S.rgba) and torch.equal(depth.view(torch.int32), S.depth.view(torch.int32))
    assert S.g.frame_status()["status"] == before
    # and the next submission renders what the first did
    rgba2, depth2 = torch.zeros_like(S.rgba), torch.zeros_like(S.depth)
    S.g.render_views_device(S.views, LC.SW, LC.SH, rgba2.data_ptr(), LC.SH * LC.SW * 4, LC.SW * 4, depth2.data_ptr(), LC.SH * S.pitch, S.pitch)
    torch.cuda.synchronize()
    assert torch.equal(rgba2, S.rgba) and torch.equal(depth2[:, :, :LC.SW].view(torch.int32), S.depth[:, :, :LC.SW].view(torch.int32))


def _checked_run(T):
    """The strip as one image (8 and 2 rows), a cap smaller than the count, and three strips as 3 and 24 images -> hash of every
    output, status."""
    import torch
    h = hashlib.sha256()
    views = [u for yaw in (33.0, 100.0, 211.0) for u in LC.views(yaw)]
    s = Strip(T, views)
    for n_views, vpi, max_rows, cap in ((8, 8, 8, 400), (8, 8, 2, 400), (8, 8, 8, 17), (24, 8, 8, 200), (24, 1, 8, 50), (23, 1, 8, 50)):
        for x in run(T, s.g, views[:n_views], s.depth, s.pitch, s.d_peaks, s.d_widths, LC.N_PEAKS, vpi, max_rows, cap):
            h.update(x.tobytes())
    for x in s.g.labels_read(T.label_params(LC.ROW_HEIGHT, 8, 8, 30), views, LC.SW, LC.SH, s.depth.data_ptr(), LC.peaks(), LC.widths(), depth_view_stride=LC.SH * s.pitch,
                             depth_pitch=s.pitch):
        h.update(x.tobytes())
    status = s.g.frame_status()["status"]
    s.close()
    torch.cuda.synchronize()
    return {"sha": h.hexdigest()[:24], "status": status}


def test_bounds_checked_build_records_no_out_of_range_index(topo):
    got = checked_run("test_labels_gpu")      # kStatusBounds: an index k_labels formed was out of range
    assert got["sha"] == _checked_run(topo)["sha"], "the bounds-checked build answers as the product build"
