"""ctypes wrapper over tests/map_emul.cpp (TEST-ONLY g++ build of the product's map rule, topo_map.h)."""
from __future__ import annotations

import ctypes as C

import numpy as np

import native
import topo_renderer_amd as T
from emul_tiles import EmulTile, emul_tile, vp as _vp

_LIB = None
WAVES, ALL_TILES, BRUTE = 0, 1, 2      # emul_map's modes: waves over their tile lists, waves over every tile, the plain loop


def lib():
    global _LIB
    if _LIB is None:
        _LIB = native.load("libmap_emul.so", ["map_emul.cpp"], {"emul_map": C.c_int, "emul_map_box_tile": C.c_int, "emul_map_rows": C.c_uint32,
                                                                 "emul_map_blend": C.c_uint32, "emul_map_floor_div": C.c_int64})
        _LIB.emul_map_floor_div.argtypes = [C.c_int64, C.c_int64]
        _LIB.emul_map_blend.argtypes = [C.c_uint32, C.c_uint32]
    return _LIB


def rows_per_wave() -> int:
    """R of the header the emulation was built from."""
    return int(lib().emul_map_rows())


def tile_array(tiles, normals):
    """tiles: [(heights f32 (h, w), raster_point, model_point, pixel_scale)] in draw order, normals: their (h, w, 4) u8 textures ->
    (EmulTile array, what it points into: keep it alive as long as the array)."""
    keep = []
    arr = (EmulTile * max(len(tiles), 1))()
    for i, (t, nrm) in enumerate(zip(tiles, normals)):
        hts = np.ascontiguousarray(t[0], np.float32)
        n32 = np.ascontiguousarray(nrm, np.uint8).reshape(hts.shape + (4,)).view(np.uint32).reshape(hts.shape).copy()
        tu = T.terrain_uniforms(np.float32(t[1]), np.float32(t[2]), np.float32(t[3]), hts.shape[1], hts.shape[0])
        keep += [hts, n32]
        arr[i] = emul_tile(hts, n32, tu)
    return arr, keep


def mask_words(tile_w, tile_h) -> int:
    return ((tile_w - 1) * (tile_h - 1) + 31) // 32


def pack_mask(mask) -> np.ndarray:
    """A (h - 1, w - 1) bool mask as topo_viewshed_read reports it -> the tile's words: bit = x (h - 1) + y."""
    m = np.asarray(mask, bool)
    bits = np.ascontiguousarray(m.T).ravel()      # column-major: x outer, y inner
    padded = np.zeros(((len(bits) + 31) // 32) * 32, np.uint8)
    padded[:len(bits)] = bits
    return np.packbits(padded.reshape(-1, 32)[:, ::-1], axis=1).view(">u4").astype(np.uint32).ravel()


def run(tiles, normals, params, masks=None, mode=WAVES, rows=None):
    """-> ((ny, nx, 4) u8 RGBA, (ny, nx) u8 flags, failed index checks, (tiles listed, waves, overflowed waves)).  masks: None, or a
    (h - 1, w - 1) bool mask per tile."""
    arr, keep = tile_array(tiles, normals)
    th, tw = (keep[0].shape if keep else (2, 2))
    p = np.ascontiguousarray(params, dtype=T.MAP_PARAMS_DTYPE).reshape(-1)[:1]
    nx, ny = int(p["nx"][0]), int(p["ny"][0])
    rgba, flags = np.zeros((ny, nx, 4), np.uint8), np.zeros((ny, nx), np.uint8)
    words, table = None, None
    if masks is not None:
        words = [pack_mask(m) for m in masks]
        table = (C.c_void_p * max(len(words), 1))(*[w.ctypes.data for w in words])
    stats = np.zeros(3, np.uint64)
    bad = lib().emul_map(arr, len(tiles), tw, th, table, mask_words(tw, th), _vp(p), mode, rows_per_wave() if rows is None else rows, _vp(rgba), _vp(flags), _vp(stats))
    return rgba, flags, int(bad), tuple(int(s) for s in stats)


def box_keeps(tiles, normals, rank, params, ca, cb, ra, rb) -> bool:
    arr, keep = tile_array(tiles, normals)
    th, tw = keep[0].shape
    p = np.ascontiguousarray(params, dtype=T.MAP_PARAMS_DTYPE).reshape(-1)[:1]
    return bool(lib().emul_map_box_tile(arr, rank, tw, th, _vp(p), ca, cb, ra, rb))
