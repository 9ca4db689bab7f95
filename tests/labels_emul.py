"""ctypes wrapper over tests/labels_emul.cpp (TEST-ONLY g++ build of the product's peak-label rule, topo_labels.h)."""
from __future__ import annotations

import ctypes as C

import numpy as np

import native
from labels_ref import LABEL_DTYPE

_LIB = None


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def lib():
    global _LIB
    if _LIB is None:
        _LIB = native.load("liblabels_emul.so", ["labels_emul.cpp"], {"emul_label_layout": C.c_int, "emul_labels": None, "emul_label_constants": None})
        assert LABEL_DTYPE.itemsize == 32
    return _LIB


def layout(x, widths, image_width, row_height, max_rows):
    """-> ((n,) int32 rows: -1 no row free, -2 unusable width; the placed labels in order)."""
    xs, ws = np.ascontiguousarray(x, np.uint32), np.ascontiguousarray(widths, np.float32)
    rows, out = np.zeros(len(xs), np.int32), np.zeros(len(xs), LABEL_DTYPE)
    n = lib().emul_label_layout(C.c_uint32(len(xs)), vp(xs), vp(ws), C.c_uint32(image_width), C.c_float(row_height), C.c_uint32(max_rows), vp(rows), vp(out))
    return rows, out[:n]


def labels(projs, depth, peaks, widths, width, height, views_per_image, row_height, max_rows, cap):
    """projs (n_views, 16) f32, depth (n_views, height, pitch >= width) f32 on the host -> ((images, cap) LABEL_DTYPE, zero behind
    each image's labels; (images,) uint32 counts; (images, n_peaks) uint8 states)."""
    projs = np.ascontiguousarray(projs, np.float32).reshape(-1, 16)
    depth = np.ascontiguousarray(depth, np.float32)
    pk, ws = np.ascontiguousarray(peaks, np.float32).reshape(-1, 3), np.ascontiguousarray(widths, np.float32)
    n_views, images = len(projs), len(projs) // views_per_image
    assert depth.shape[:2] == (n_views, height) and depth.shape[2] >= width and len(pk) == len(ws)
    out, counts, state = np.zeros((images, cap), LABEL_DTYPE), np.zeros(images, np.uint32), np.zeros((images, len(pk)), np.uint8)
    lib().emul_labels(C.c_uint32(n_views), vp(projs), C.c_uint32(width), C.c_uint32(height), vp(depth), C.c_size_t(depth.shape[1] * depth.shape[2]),
                      C.c_size_t(depth.shape[2]), C.c_uint32(len(pk)), vp(pk), vp(ws), C.c_uint32(views_per_image), C.c_float(row_height), C.c_uint32(max_rows),
                      C.c_uint32(cap), vp(out), vp(counts), vp(state))
    return out, counts, state


def constants():
    out = np.zeros(8, np.uint32)
    lib().emul_label_constants(vp(out))
    return dict(HIDDEN=int(out[0]), PLACED=int(out[1]), NO_ROW=int(out[2]), BAD_WIDTH=int(out[3]), MAX_ROWS=int(out[4]), MAX_GRID_BITS=int(out[5]),
                LABEL_BYTES=int(out[6]))
