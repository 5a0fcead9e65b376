# -*- coding:utf-8 -*-
"""Host: tests/bn_reference.py (the float64 reference of tests/test_bn_gpu.py) against torch's own batch_norm, against
oracle.reference_layers.keras_batchnorm where both are defined, and against the closed forms it restates."""
import pytest
import torch
import torch.nn.functional as TF

from oracle import reference_layers as R
from tests import bn_reference as B

TOL = 1e-12
CASES = [((33, 5), True, True), ((33, 5), True, False), ((33, 5), False, True), ((33, 5), False, False),
         ((1, 4), True, True), ((7, 5, 16), True, True), ((7, 5, 16), False, False), ((1000, 1), True, True)]
HYPER = [(1e-3, 0.99), (1e-5, 0.9), (1e-1, 0.0)]


def _data(shape, has_gamma, has_beta, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    C = shape[-1]
    x = torch.randn(shape, generator=g, dtype=torch.float64) * 2.0 + 3.0
    gamma = torch.randn(C, generator=g, dtype=torch.float64) if has_gamma else None
    beta = torch.randn(C, generator=g, dtype=torch.float64) if has_beta else None
    mm = torch.randn(C, generator=g, dtype=torch.float64)
    mv = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    gy = torch.randn(shape, generator=g, dtype=torch.float64)
    return x, gamma, beta, mm, mv, gy


def _close(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype
    assert (a - b).abs().max().item() <= TOL * max(b.abs().max().item(), 1.0)


@pytest.mark.parametrize('eps,momentum', HYPER)
@pytest.mark.parametrize('shape,has_gamma,has_beta', CASES)
def test_against_torch_batch_norm(shape, has_gamma, has_beta, eps, momentum):
    x, gamma, beta, mm, mv, _ = _data(shape, has_gamma, has_beta)
    x2 = x.reshape(-1, shape[-1])                                        # F.batch_norm normalises axis 1
    out = B.keras_batchnorm(x, gamma, beta, mm, mv, True, eps, momentum)
    if x2.shape[0] > 1:                                                  # torch refuses one value per channel in training
        _close(out.y, TF.batch_norm(x2, None, None, gamma, beta, True, 0.0, eps).reshape(shape))
    else:
        _close(out.y, (beta if has_beta else torch.zeros(shape[-1], dtype=torch.float64)).expand(shape))
    ev = B.keras_batchnorm(x, gamma, beta, mm, mv, False, eps, momentum)
    _close(ev.y, TF.batch_norm(x2, mm, mv, gamma, beta, False, 0.0, eps).reshape(shape))
    assert ev.moving_mean is mm and ev.moving_var is mv
    _close(ev.mean, mm)
    _close(ev.rstd, (mv + eps).rsqrt())


@pytest.mark.parametrize('eps,momentum', HYPER)
@pytest.mark.parametrize('shape', [(33, 5), (1, 4), (7, 5, 16), (1000, 1)])
def test_against_oracle_keras_batchnorm(shape, eps, momentum):
    x, gamma, beta, mm, mv, _ = _data(shape, True, True, seed=1)
    for training in (True, False):
        out = B.keras_batchnorm(x, gamma, beta, mm, mv, training, eps, momentum)
        y, nm, nv = R.keras_batchnorm(x, gamma, beta, mm, mv, training=training, eps=eps, momentum=momentum)
        _close(out.y, y)
        _close(out.moving_mean, nm)
        _close(out.moving_var, nv)
    # no moving statistics: both leave them None
    out = B.keras_batchnorm(x, gamma, beta, None, None, True, eps, momentum)
    assert out.moving_mean is None and out.moving_var is None
    _close(out.y, R.keras_batchnorm(x, gamma, beta, training=True, eps=eps, momentum=momentum)[0])


@pytest.mark.parametrize('eps,momentum', HYPER)
@pytest.mark.parametrize('shape,has_gamma,has_beta', CASES)
def test_statistics_moving_update_and_sums_in_closed_form(shape, has_gamma, has_beta, eps, momentum):
    x, gamma, beta, mm, mv, gy = _data(shape, has_gamma, has_beta, seed=2)
    C = shape[-1]
    x2, g2 = x.reshape(-1, C), gy.reshape(-1, C)
    N = x2.shape[0]
    mean = x2.sum(0) / N
    var = (x2 * x2).sum(0) / N - mean * mean                             # biased; float64 carries the cancellation here
    out = B.keras_batchnorm(x, gamma, beta, mm, mv, True, eps, momentum, gy=gy)
    _close(out.mean, mean)
    assert (out.rstd - (var + eps).rsqrt()).abs().max().item() <= 1e-9 * out.rstd.abs().max().item()
    _close(out.moving_mean, momentum * mm + (1 - momentum) * mean)
    assert (out.moving_var - (momentum * mv + (1 - momentum) * var)).abs().max().item() <= 1e-9
    if N == 1:
        assert torch.equal(out.moving_var, momentum * mv)
        _close(out.rstd, torch.full((C,), eps ** -0.5, dtype=torch.float64))
    if momentum == 0.0:
        assert torch.equal(out.moving_mean, out.mean)
    xhat = (x2 - out.mean) * out.rstd
    _close(out.sum_g, g2.sum(0))
    _close(out.sum_gx, (g2 * xhat).sum(0))
    s_g, s_gx = B.sum_scales(x, gy, eps)
    _close(s_g, g2.abs().sum(0))
    _close(s_gx, (g2 * xhat).abs().sum(0))
    assert bool((s_g >= out.sum_g.abs()).all()) and bool((s_gx + 1e-300 >= out.sum_gx.abs()).all())


@pytest.mark.parametrize('shape,has_gamma,has_beta', CASES)
def test_gradients_by_autograd_are_the_textbook_ones(shape, has_gamma, has_beta):
    """dbeta = sum_g, dgamma = sum_gx, dx = gamma rstd (gy - sum_g / N - xhat sum_gx / N): what csrc/bn.hip evaluates"""
    x, gamma, beta, mm, mv, gy = _data(shape, has_gamma, has_beta, seed=3)
    C = shape[-1]
    xs = [None if t is None else t.clone().requires_grad_(True) for t in (x, gamma, beta)]
    out = B.keras_batchnorm(*xs, mm, mv, True, 1e-3, 0.99, gy=gy)
    (out.y * gy).sum().backward()
    N = x.numel() // C
    xhat = (x - out.mean) * out.rstd
    ga = gamma if has_gamma else torch.ones(C, dtype=torch.float64)
    _close(xs[0].grad, ga * out.rstd * (gy - out.sum_g / N - xhat * (out.sum_gx / N)))
    if has_gamma:
        _close(xs[1].grad, out.sum_gx)
    if has_beta:
        _close(xs[2].grad, out.sum_g)
    assert not out.mean.requires_grad and not out.rstd.requires_grad and not out.moving_mean.requires_grad


def test_float32_in_float32_out_and_bad_rank():
    x, gamma, beta, mm, mv, gy = (t.float() for t in _data((33, 5), True, True))
    out = B.keras_batchnorm(x, gamma, beta, mm, mv, True, 1e-3, 0.99, gy=gy)
    assert all(t.dtype == torch.float32 for t in out)
    with pytest.raises(ValueError):
        B.keras_batchnorm(torch.zeros(2, 3, 4, 5))
    with pytest.raises(ValueError):
        B.keras_batchnorm(torch.zeros(5))
