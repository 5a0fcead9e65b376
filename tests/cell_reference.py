# -*- coding:utf-8 -*-
"""Restatements of the tower cell (csrc/cell.hip) for the tests: every activation name as a torch expression that is evaluated
in float64 (the reference) and, unchanged, in float32 on the CPU (yardstick B's fp32 class); derivatives by autograd in the
same precision; and a `Dense -> (BN) -> act -> keep` chain in both cell orders that takes the keep-scale as an input.

The expressions are the definitions functional.get_activation registers (so autograd takes the same derivative at a kink),
written in the form that keeps its digits where the plain form cancels: softplus as logaddexp(x, 0), gelu through erfc on the
side where Phi is small."""
import math

import torch
import torch.nn.functional as F

# every name ops.cell takes (None / 'linear' included), aliases last
NAMES = ['linear', 'relu', 'sigmoid', 'tanh', 'elu', 'selu', 'softplus', 'softsign', 'exponential',
         'relu6', 'leaky_relu', 'silu', 'gelu', 'mish', 'hard_sigmoid', 'hard_silu', 'swish', 'hard_swish']
NEW_NAMES = ['relu6', 'leaky_relu', 'silu', 'mish', 'hard_sigmoid', 'hard_silu', 'hard_swish']        # ValueError before the cell
INPUT_KINDS = ('silu', 'swish', 'gelu', 'mish', 'hard_silu', 'hard_swish')                            # act' from the input

# the derivative at each kink, as torch's CPU autograd takes it for the registered definition (asserted in test_cell_host.py)
KINKS = {
    'relu': {0.0: 0.0},
    'relu6': {0.0: 0.0, 6.0: 0.0},
    'leaky_relu': {0.0: 0.2},
    'elu': {0.0: 1.0},
    'selu': {0.0: 1.0507009873554805 * 1.6732632423543772},
    'hard_sigmoid': {-3.0: 0.0, 3.0: 0.0, 0.0: 1.0 / 6.0},
    'hard_silu': {-3.0: 0.0, 3.0: 1.0, 0.0: 0.5},
    'hard_swish': {-3.0: 0.0, 3.0: 1.0, 0.0: 0.5},
}


def _gelu(x):
    h = 0.5 * torch.special.erfc(x.abs() / math.sqrt(2.0))
    return x * torch.where(x < 0, h, 1.0 - h)


_ACTS = {
    'linear': lambda x: x * 1.0,
    'relu': torch.relu,
    'sigmoid': torch.sigmoid,
    'tanh': torch.tanh,
    'elu': F.elu,
    'selu': torch.selu,
    'softplus': lambda x: torch.logaddexp(x, torch.zeros_like(x)),
    'softsign': F.softsign,
    'exponential': torch.exp,
    'relu6': F.relu6,
    'leaky_relu': lambda x: F.leaky_relu(x, 0.2),
    'silu': F.silu,
    'swish': F.silu,
    'gelu': _gelu,
    'mish': F.mish,
    'hard_sigmoid': lambda x: F.relu6(x + 3.0) / 6.0,      # F.hardsigmoid's backward carries float32(1 / 6) in float64 too
    'hard_silu': F.hardswish,
    'hard_swish': F.hardswish,
}


def act(name, x):
    return _ACTS[name or 'linear'](x)


def value_and_grad(name, x, g, keep=None, dtype=torch.float64):
    """(out, dx) of out = keep * act(x) under the upstream gradient g, evaluated in `dtype` on the CPU"""
    xd = x.detach().to('cpu', dtype).requires_grad_(True)
    y = act(name, xd)
    if keep is not None:
        y = y * keep.to('cpu', dtype)
    (dx,) = torch.autograd.grad(y, xd, g.detach().to('cpu', dtype))
    return y.detach(), dx


def batchnorm(h, gamma, beta, eps=1e-3):
    """keras BatchNormalization in training: batch mean and BIASED variance over the rows"""
    mean = h.mean(0, keepdim=True)
    var = ((h - mean) ** 2).mean(0, keepdim=True)
    return (h - mean) / torch.sqrt(var + eps) * gamma + beta


def chain(x, p, name, keep, order='dnn', dtype=torch.float64):
    """Input -> Dense(W1[, b1]) -> (BN) -> act -> keep -> Dense(W2, b2)   (order 'dnn', deepnets.dnn), or
    Input -> Dense(W1, b1) -> act -> keep -> (BN) -> Dense(W2, b2)        (order 'dadb', deepnets.custom_dnn_D_A_D_B)
    p: {'W1', 'b1' | None, 'gamma' | None, 'beta' | None, 'W2', 'b2'} -> (output, {name: leaf}) with the leaves in `dtype`"""
    leaf = {k: v.detach().to('cpu', dtype).requires_grad_(True) for k, v in p.items() if v is not None}
    h = x.detach().to('cpu', dtype) @ leaf['W1']
    if 'b1' in leaf:
        h = h + leaf['b1']
    if order == 'dnn' and 'gamma' in leaf:
        h = batchnorm(h, leaf['gamma'], leaf['beta'])
    h = act(name, h) * keep.to('cpu', dtype)
    if order == 'dadb' and 'gamma' in leaf:
        h = batchnorm(h, leaf['gamma'], leaf['beta'])
    return h @ leaf['W2'] + leaf['b2'], leaf
