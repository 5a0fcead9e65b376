# -*- coding:utf-8 -*-
"""Shared by the host and the GPU tests of csrc/dense_tiled.hip: the geometry query as a Python call, and the named cases
with the geometry each of them is there to reach (tests/test_dense_tiled_host.py asserts it without a GPU,
tests/test_dense_tiled_edges_gpu.py runs them)."""
import ctypes

FWD, GRAD_X, GRAD_W = 0, 1, 2


def geometry(N, K, M, product):
    """(tile, splits, steps_per_split) of one product's launch, from dt_dense_tiled_geometry"""
    from deeptables_amd import _lib
    tile, splits, per = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    _lib.check(_lib.lib().dt_dense_tiled_geometry(N, K, M, product, ctypes.byref(tile), ctypes.byref(splits),
                                                  ctypes.byref(per)), 'dt_dense_tiled_geometry')
    return tile.value, splits.value, per.value


# One product at 128 x 128 at a time: (N, K, M, bias) -> (tile, splits, steps_per_split) of forward, grad_x, grad_W.
# Even row lengths and fresh allocations give 16-byte staging loads, odd ones 4-byte loads.
ONE_BIG_TILE = {
    'fwd128_vec': ((4100, 36, 1028, True), ((128, 1, 2), (64, 1, 33), (64, 17, 8))),
    'fwd128_scalar': ((4099, 37, 1027, False), ((128, 1, 2), (64, 1, 33), (64, 17, 8))),
    'gx128_vec': ((4100, 1028, 36, False), ((64, 1, 33), (128, 1, 2), (64, 17, 8))),
    'gx128_scalar': ((4099, 1027, 37, False), ((64, 1, 33), (128, 1, 2), (64, 17, 8))),
    'gw128_vec': ((37, 2052, 1924, True), ((64, 1, 65), (64, 1, 61), (128, 1, 2))),
    'gw128_scalar': ((37, 2051, 1925, True), ((64, 1, 65), (64, 1, 61), (128, 1, 2))),
}

# The 64 x 64 shapes of the alignment, guard-band and special-value tests: one tile size, no batch split.
SMALL_TILE = {(70, 1204, 132): ((64, 1, 38), (64, 1, 5), (64, 1, 3)),
              (67, 133, 69): ((64, 1, 5), (64, 1, 3), (64, 1, 3))}

# grad_W's batch split: (N, K, M) -> (splits, steps_per_split, rows of the last split).  (2570, 3400, 6) is the shape at which
# the second computation of `splits` lowers the first: 54 tiles ask for ceil(512 / 54) = 10 splits, 81 steps in 10 splits are
# 9 steps each, and 9 splits of 9 steps already hold all 81.
SPLIT = {(1300, 70, 6): (6, 7, 1300 - 5 * 7 * 32), (4100, 36, 1028): (17, 8, 4), (2570, 3400, 6): (9, 9, 2570 - 8 * 9 * 32)}
SHRINKING = (2570, 3400, 6)

DEGENERATE = [(1, 1, 2), (1, 3, 2), (2, 2, 3), (1, 5, 130), (129, 1, 65), (3, 4, 2)]
