# -*- coding:utf-8 -*-
"""CPU: the tiled Dense entry points (csrc/dense_tiled.hip) — their shape predicate, their argument validation and which
of the two kernel families ops.dense sends a shape to.  No launch happens here."""
import pytest
import torch

from tests.infer_support import Recorder


def test_tiled_predicate_takes_every_2d_shape_but_the_gemv():
    from deeptables_amd import _lib
    h = _lib.lib()
    for shape in [(1, 1, 2), (70, 10413, 128), (40, 64, 1300), (8192, 2912, 832), (212992, 10413, 128)]:
        assert h.dt_dense_tiled_supported(*shape) == 1, shape
    for shape in [(5, 7, 1), (8192, 429, 1), (0, 4, 4), (-1, 4, 4), (4, 0, 4), (4, -3, 4), (4, 4, 0), (4, 4, -2)]:
        assert h.dt_dense_tiled_supported(*shape) == 0, shape
    assert h.dt_dense_tiled_workspace_bytes(70, 10413, 128) >= 0
    # the shapes of the issue's table are exactly the ones the LDS-slab kernels refuse
    for K, M in [(10413, 128), (2912, 832), (1792, 832), (2093, 128)]:
        assert h.dt_dense_supported(8192, K, M) == 0 and h.dt_dense_tiled_supported(8192, K, M) == 1


def test_tiled_argument_validation_without_a_gpu():
    """bad sizes, a bad activation code and null pointers are rejected before any launch -> exercisable on CPU"""
    from deeptables_amd import _lib
    h = _lib.lib()
    bad = [(-1, 4, 4), (4, 0, 4), (4, 4, 0), (4, -2, 4)]
    for N, K, M in bad:
        assert h.dt_dense_tiled_fwd(None, None, None, _lib.DT_ACT_RELU, N, K, M, None, None) == -1, (N, K, M)
        assert b'dt_dense_tiled_fwd' in h.dt_last_error()
        assert h.dt_dense_tiled_bwd(None, None, None, None, _lib.DT_ACT_RELU, N, K, M, None, None, None, None, None) == -1
        assert b'dt_dense_tiled_bwd' in h.dt_last_error()
    assert h.dt_dense_tiled_fwd(None, None, None, 7, 4, 4, 4, None, None) == -1              # act
    assert h.dt_dense_tiled_bwd(None, None, None, None, 2, 4, 4, 4, None, None, None, None, None) == -1
    assert h.dt_dense_tiled_fwd(None, None, None, _lib.DT_ACT_RELU, 4, 4, 4, None, None) == -1    # null pointers
    assert b'null' in h.dt_last_error()
    assert h.dt_dense_tiled_bwd(None, None, None, None, _lib.DT_ACT_LINEAR, 4, 4, 4, None, None, None, None, None) == -1
    assert b'null' in h.dt_last_error()
    # an empty batch is a no-op, and M == 1 belongs to the GEMV kernels of dt_dense_*
    assert h.dt_dense_tiled_fwd(None, None, None, _lib.DT_ACT_RELU, 0, 4, 4, None, None) == 0
    assert h.dt_dense_tiled_bwd(None, None, None, None, _lib.DT_ACT_RELU, 0, 4, 4, None, None, None, None, None) == 0
    one = torch.zeros(4)
    p = _lib.ptr(one)
    assert h.dt_dense_tiled_fwd(p, p, None, _lib.DT_ACT_LINEAR, 4, 1, 1, p, None) not in (0, -1)
    assert h.dt_dense_tiled_bwd(p, p, p, p, _lib.DT_ACT_LINEAR, 4, 1, 1, None, p, None, None, None) not in (0, -1)


class _FakeCuda(torch.Tensor):
    """a CPU tensor that says it lives on the GPU: enough for ops.dense's host side when no launch is made"""

    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t)

    @property
    def is_cuda(self):
        return True


@pytest.mark.parametrize('N,K,M,tiled', [(33, 429, 128, False), (64, 39, 1, False), (257, 600, 64, True),
                                         (70, 2912, 832, True), (45, 10413, 128, True), (40, 64, 1300, True)])
def test_ops_dense_picks_the_kernel_family_by_the_old_predicate(monkeypatch, N, K, M, tiled):
    from deeptables_amd import _lib, ops
    fwd = ['dt_dense_fwd', 'dt_dense_tiled_fwd']
    bwd = ['dt_dense_bwd', 'dt_dense_tiled_bwd']
    r = Recorder(_lib.lib(), fwd + bwd)
    monkeypatch.setattr(ops, 'lib', lambda: r)
    monkeypatch.setattr(ops, 'stream_ptr', lambda: None)
    monkeypatch.setattr(ops, 'require_cuda', lambda *a: None)
    assert bool(_lib.lib().dt_dense_supported(N, K, M)) == (not tiled)
    x = torch.zeros(N, K, requires_grad=True)
    W = torch.zeros(K, M, requires_grad=True)
    b = torch.zeros(M, requires_grad=True)
    assert ops.dense_supported(_FakeCuda(x.detach()), W)
    y = ops.dense(x, W, b, 'relu')
    assert y.shape == (N, M)
    assert r.names() == [fwd[tiled]]
    y.sum().backward()
    assert r.names() == [fwd[tiled], bwd[tiled]]
    assert x.grad.shape == (N, K) and W.grad.shape == (K, M) and b.grad.shape == (M,)


# ---------------------------------------------------------------------------------------------------------------------
# dt_dense_tiled_geometry: the tile and the batch split the launches use, asked without a launch
# ---------------------------------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def test_geometry_of_the_named_gpu_cases():
    """tests/test_dense_tiled_edges_gpu.py's cases reach the tile and the split they are named for"""
    from tests.dense_tiled_support import (DEGENERATE, FWD, GRAD_W, GRAD_X, ONE_BIG_TILE, SHRINKING, SMALL_TILE, SPLIT,
                                           geometry)
    for name, ((N, K, M, _), want) in ONE_BIG_TILE.items():
        got = tuple(geometry(N, K, M, p) for p in (FWD, GRAD_X, GRAD_W))
        assert got == want, name
        assert [g[0] for g in got].count(128) == 1, name                   # one product switched alone
        assert got[FWD][2] == _cdiv(K, 32) and got[GRAD_X][2] == _cdiv(M, 32), name
    for (N, K, M), want in SMALL_TILE.items():
        assert tuple(geometry(N, K, M, p) for p in (FWD, GRAD_X, GRAD_W)) == want
    for (N, K, M), (splits, per, last_rows) in SPLIT.items():
        assert geometry(N, K, M, GRAD_W)[1:] == (splits, per)
        assert splits > 1 and N - (splits - 1) * per * 32 == last_rows
    assert SPLIT[(4100, 36, 1028)][0] == 17 and SPLIT[(1300, 70, 6)][0] == 6
    assert SPLIT[(1300, 70, 6)][2] % 32 != 0 and SPLIT[SHRINKING][2] % 32 != 0         # a last split with a partial step
    for N, K, M in DEGENERATE:
        assert all(geometry(N, K, M, p)[:2] == (64, 1) for p in (FWD, GRAD_X, GRAD_W))


# (K, M) with 1, 2, 17, 100 and 255 tiles of 64 x 64, and 54: the count at which the second computation of `splits` bites
SCAN = [(60, 60, 1), (70, 60, 2), (1028, 36, 17), (640, 640, 100), (960, 1088, 255), (3400, 6, 54)]


def test_batch_split_owns_every_step_once():
    """grad_W over N in [1, 5000]: no split is empty, no step is lost, a split has at least 256 rows' worth of steps, and a
    grid that K x M alone fills is not split.  The one place this test repeats the kernel's arithmetic is `first`, the split
    count before every split is made to own a step: it is what tells where the second computation lowers it."""
    from tests.dense_tiled_support import GRAD_W, SHRINKING, SPLIT, geometry
    shrinking = {}
    for K, M, tiles in SCAN:
        tile = geometry(1, K, M, GRAD_W)[0]
        assert tile == 64 and _cdiv(K, tile) * _cdiv(M, tile) == tiles
        for N in range(1, 5001):
            t, splits, per = geometry(N, K, M, GRAD_W)
            steps = _cdiv(N, 32)
            assert t == tile and splits >= 1
            assert (splits - 1) * per < steps <= splits * per, (N, K, M)
            if splits > 1:
                assert splits <= _cdiv(N, 256), (N, K, M)
            first = min(_cdiv(512, tiles), _cdiv(N, 256))
            assert splits <= first
            if splits < first:
                shrinking.setdefault((K, M), []).append(N)
    # with a cap of ceil(N / 256) splits of >= 8 steps each, only an uncapped count of >= 10 can end with an empty split:
    # of the six tile counts, within N <= 5000, that is the 54-tile one alone
    assert set(shrinking) == {(3400, 6)}
    assert SHRINKING[1:] == (3400, 6) and SHRINKING[0] in shrinking[(3400, 6)] and SHRINKING in SPLIT
    # 256 tiles and more: one block per CU without a split, whatever N
    for K, M in [(1024, 1024), (2052, 1924)]:
        for N in (1, 257, 5000, 100000):
            t, splits, per = geometry(N, K, M, GRAD_W)
            assert _cdiv(K, t) * _cdiv(M, t) >= 256 and splits == 1 and per == _cdiv(N, 32)


def test_geometry_argument_validation():
    import ctypes
    from deeptables_amd import _lib
    h = _lib.lib()
    assert h.dt_dense_tiled_geometry(70, 1204, 132, 0, None, None, None) == 0          # NULL outputs
    tile = ctypes.c_int(-1)
    assert h.dt_dense_tiled_geometry(70, 1204, 132, 2, ctypes.byref(tile), None, None) == 0 and tile.value == 64
    for shape in [(5, 7, 1), (0, 4, 4), (4, -3, 4), (4, 4, 0)]:
        assert h.dt_dense_tiled_supported(*shape) == 0
        tile = ctypes.c_int(-1)
        assert h.dt_dense_tiled_geometry(*shape, 0, ctypes.byref(tile), None, None) == -2, shape
        assert b'dt_dense_tiled_geometry' in h.dt_last_error() and tile.value == -1
        assert 'N=%d K=%d M=%d' % shape in h.dt_last_error().decode()
    for product in (-1, 3):
        assert h.dt_dense_tiled_geometry(70, 1204, 132, product, None, None, None) == -1
        assert b'dt_dense_tiled_geometry' in h.dt_last_error() and b'product' in h.dt_last_error()
