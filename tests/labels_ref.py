"""An independent restatement of the peak-label rule (include/topo_hip.h, "peak labels") for the tests: the layout the way the
reference's process_label_layout decides it (text_renderer.rs:300-372) -- per row a SORTED LIST OF (position, side) EDGES, a row free
when no edge lies in [Left(l), Right(r)] and the next edge after Right(r) is not a Right edge -- written the other way round from the
product's occupancy grid on purpose, and without the grid's clamp of r to the image; and the candidate rule over numpy f32."""
from __future__ import annotations

import bisect
import math

import numpy as np

LEFT, RIGHT = 0, 1      # Side: Left sorts before Right at the same position
HIDDEN, PLACED, NO_ROW, BAD_WIDTH = 0, 1, 2, 3
LABEL_DTYPE = np.dtype([("peak", "<u4"), ("view", "<u4"), ("row", "<u4"), ("label_x", "<f4"), ("label_y", "<f4"), ("label_width", "<f4"), ("peak_x", "<f4"),
                        ("peak_y", "<f4")])
NEAR, FAR = np.float32(50.0), np.float32(500000.0)


def sat_u32(v) -> int:
    """Rust's `f32 as u32`."""
    v = float(v)
    if math.isnan(v) or v <= 0.0:
        return 0
    return min(int(v), 0xFFFFFFFF)


def usable(w) -> bool:
    return bool(np.isfinite(w)) and float(w) >= 0.0


class Rows:
    """The reference's Vec<BTreeSet<LabelEdge>>, max_rows standing for its MAX_ROWS."""

    def __init__(self, max_rows):
        self.max_rows = max_rows
        self.edges = []

    def place(self, x: int, width) -> int | None:
        left = (sat_u32(math.floor(np.float32(x))), LEFT)
        right = (sat_u32(np.ceil(np.float32(x) + np.float32(width))), RIGHT)
        row_i = None
        for i, row in enumerate(self.edges):
            a = bisect.bisect_left(row, left)
            if a < len(row) and row[a] <= right:
                continue      # an edge inside [left, right]
            b = bisect.bisect_left(row, right)
            if b < len(row) and row[b][1] == RIGHT:
                continue      # the first edge to the right is the right end of a label that encloses this one
            row_i = i
            break
        if row_i is None:
            self.edges.append([])
            row_i = len(self.edges) - 1
        if row_i >= self.max_rows:
            return None
        bisect.insort(self.edges[row_i], left)
        bisect.insort(self.edges[row_i], right)
        return row_i


def layout(x, widths, row_height, max_rows):
    """Positions and widths -> ((n,) int32 rows: -1 no row free, -2 unusable width; the placed labels in order, peak = the index)."""
    rows = Rows(max_rows)
    row_out = np.zeros(len(x), np.int32)
    out = []
    for j, (xj, w) in enumerate(zip(x, widths)):
        if not usable(w):
            row_out[j] = -2
            continue
        k = rows.place(int(xj), w)
        row_out[j] = -1 if k is None else k
        if k is not None:
            out.append((j, 0, k, np.float32(xj), np.float32(row_height) * (np.float32(0.5) + np.float32(k)), np.float32(w), np.float32(xj), np.float32(0)))
    return row_out, np.array(out, LABEL_DTYPE)


def linear_depth(d):
    return (FAR * NEAR) / (FAR - d.astype(np.float32) * (FAR - NEAR))


def project(proj, peaks, width, height):
    """project_peak over numpy f32, one rounding per operation: (inside (n,) bool, x_pos, y_pos (n,) int64, peak_dist (n,) f32)."""
    m = np.asarray(proj, np.float32).reshape(16)
    x, y, z = (np.ascontiguousarray(peaks[:, k], np.float32) for k in range(3))
    res = []
    for r in range(4):
        t = m[r] * x
        t = m[4 + r] * y + t
        t = m[8 + r] * z + t
        res.append(m[12 + r] + t)
    with np.errstate(all="ignore"):
        px, py, pz = res[0] / res[3], res[1] / res[3], res[2] / res[3]
        inside = (px > -1) & (px < 1) & (py > -1) & (py < 1) & (pz < 1)
        one, half = np.float32(1.0), np.float32(0.5)
        xf = half * (px + one) * np.float32(width)
        yf = -half * (py - one) * np.float32(height)
        x_pos = np.where(inside, xf, 0).astype(np.int64)
        y_pos = np.where(inside, yf, 0).astype(np.int64)
        dist = linear_depth(pz)
    return inside, x_pos, y_pos, dist


def candidates(projs, depth, peaks, width, height):
    """One image: projs (views, 16) f32, depth (views, height, >= width) f32 -> (found (n,) bool, view, x_pos, y_pos (n,) int64): the
    first view in ascending order in which the peak passes the visibility test."""
    n = len(peaks)
    found, view = np.zeros(n, bool), np.zeros(n, np.int64)
    xs, ys = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for v in range(len(projs)):
        inside, x_pos, y_pos, dist = project(projs[v], peaks, width, height)
        ok = inside & (x_pos < width) & (y_pos < height)
        d = depth[v][np.where(ok, y_pos, 0), np.where(ok, x_pos, 0)]
        with np.errstate(all="ignore"):
            vis = ok & (dist - np.float32(10.0) < linear_depth(d)) & ~found
        view[vis], xs[vis], ys[vis] = v, x_pos[vis], y_pos[vis]
        found |= vis
    return found, view, xs, ys


def labels(projs, depth, peaks, widths, width, height, views_per_image, row_height, max_rows):
    """All images of a submission: projs (n_views, 16), depth (n_views, height, >= width) -> per image (labels LABEL_DTYPE in placement
    order, uncapped; state (n_peaks,) uint8)."""
    out = []
    for i in range(len(projs) // views_per_image):
        sl = slice(i * views_per_image, (i + 1) * views_per_image)
        found, view, xs, ys = candidates(projs[sl], depth[sl], peaks, width, height)
        rows = Rows(max_rows)
        state = np.zeros(len(peaks), np.uint8)
        recs = []
        for p in np.flatnonzero(found):
            w = widths[p]
            if not usable(w):
                state[p] = BAD_WIDTH
                continue
            peak_x = int(view[p]) * width + int(xs[p])
            k = rows.place(peak_x, w)
            state[p] = NO_ROW if k is None else PLACED
            if k is not None:
                recs.append((p, view[p], k, np.float32(peak_x), np.float32(row_height) * (np.float32(0.5) + np.float32(k)), np.float32(w), np.float32(peak_x),
                             np.float32(ys[p])))
        out.append((np.array(recs, LABEL_DTYPE), state))
    return out
