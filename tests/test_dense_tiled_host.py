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
