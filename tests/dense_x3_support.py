# -*- coding:utf-8 -*-
"""Shared by the host and the GPU tests of csrc/dense_tiled_x3.hip: the claim table of the two modes, the geometry query as
a Python call, the float64 reference (yardstick A as tests/test_dense_tiled_gpu.py::_reference builds it, with the width of
the kink mask following the forward's class) and the named cases with the path each of them is there to reach."""
import ctypes
import functools

import numpy as np
import torch

from tests import precision as P
from tests.dense_tiled_support import FWD, GRAD_W, GRAD_X, ONE_BIG_TILE, SMALL_TILE, SPLIT

# mode -> (forward class, backward class) of tests/precision.py; grad_b is an fp32 column sum in both modes
CLAIM = {'bf16x3': ('fp32', 'b17'), 'bf16': ('bf16', 'bf16')}
GRAD_B_CLASS = 'fp32'
# cap on the share of relu units kink_mask may zero (a condition on the reference, checked before any kernel runs)
MASK_CAP = {'bf16x3': 0.001, 'bf16': 0.20}
STEP = 32           # contraction indices per step, the unit of steps_per_split


def mode_code(mode):
    from deeptables_amd import _lib
    return {'bf16x3': _lib.DT_DENSE_X3, 'bf16': _lib.DT_DENSE_BF16}[mode]


def geometry(N, K, M, mode, product):
    """(tile_rows, tile_cols, splits, steps_per_split) of one product's launch, from dt_dense_x3_geometry"""
    from deeptables_amd import _lib
    out = [ctypes.c_int(-1) for _ in range(4)]
    _lib.check(_lib.lib().dt_dense_x3_geometry(N, K, M, mode_code(mode), product, *[ctypes.byref(v) for v in out]),
               'dt_dense_x3_geometry')
    return tuple(v.value for v in out)


# (N, K, M, act, bias).  The first eight are the issue's; the rest are there for one path each (PATHS says which, and
# tests/test_dense_x3_host.py asserts it through the geometry query).  With K above 1,932 the bf16-wide kink mask zeroes more
# than a fifth of the relu units (37.6 % at K = 10,413): those shapes run with the linear activation in bf16 mode.
BASE = [(33, 1201, 128, 'relu', True), (257, 600, 64, 'relu', True), (40, 64, 1300, 'relu', False),
        (5, 1203, 3, None, True), (37, 301, 2, None, True), (129, 1443, 128, 'relu', True),
        (45, 10413, 128, 'relu', False), (70, 2912, 832, None, True)]
BIG = [v[0][:3] + ('relu', v[0][3]) for v in ONE_BIG_TILE.values()]      # one product at 128 x 128 each, even and odd rows
SHORT_K = [(320, 20, 1300, 'relu', True)]                                # a forward contraction below one step, a grad_W one of whole steps
CASES = BASE + BIG + SHORT_K
# grad_W's batch split, merged with float atomics: run onto a random prefill and a second time onto the result
SPLIT_CASES = [(257, 600, 64), (4100, 36, 1028)]     # 2 splits with a one-row last step; 17 splits


def act_in_mode(mode, K, act):
    return None if (mode == 'bf16' and K > 1932) else act


def _rnd(g, shape, scale=1.0):
    """float64 values that float32 holds exactly: the kernel and the reference see the same inputs"""
    return (torch.randn(shape, generator=g, dtype=torch.float64) * scale).float().double()


@functools.lru_cache(maxsize=None)
def reference(seed, N, K, M, act, bias, cls):
    """float64 forward / backward of one Dense and the |A| |B| scales of yardstick A; computed once per argument list and
    shared: callers must not modify it.  `masked` is the share of units kink_mask zeroed at class `cls`."""
    g = torch.Generator().manual_seed(seed)
    x, W = _rnd(g, (N, K)), _rnd(g, (K, M), 1.0 / np.sqrt(K))
    b = _rnd(g, (M,), 0.3) if bias else None
    lin = lambda x_, W_, b_: x_ @ W_ + (b_ if b_ is not None else 0)
    pre = lin(x, W, b)
    up0 = _rnd(g, (N, M))
    up = P.kink_mask(pre, P.abs_forward(lin, (x, W, b)), up0, act, cls)
    masked = float(((up == 0) & (up0 != 0)).double().mean())
    xr, Wr = x.clone().requires_grad_(True), W.clone().requires_grad_(True)
    br = b.clone().requires_grad_(True) if bias else None
    ref = xr @ Wr + (br if bias else 0)
    ref = torch.relu(ref) if act == 'relu' else ref
    (ref * up).sum().backward()
    upl = up * (pre > 0) if act == 'relu' else up
    s_out, (s_x, s_W, s_b) = P.abs_scale(lin, (x, W, b), upl)
    return dict(x=x, W=W, b=b, up=up, y=ref.detach(), dx=xr.grad, dW=Wr.grad, db=br.grad if bias else None,
                s_y=s_out, s_x=s_x, s_W=s_W, s_b=s_b, masked=masked)


def reference_for(mode, N, K, M, act, bias):
    return reference(7 * N + K + M, N, K, M, act_in_mode(mode, K, act), bias, CLAIM[mode][0])
