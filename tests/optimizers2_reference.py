# -*- coding:utf-8 -*-
"""Keras 3's SGD with momentum, Adamax and Ftrl restated on torch tensors, for the tests of `deeptables_amd.training.SGD`
(momentum != 0), `Adamax` and `Ftrl`.  The functions compute in the dtype of their inputs: float64 for the reference,
float32 where a test wants the same formulas evaluated in the kernels' precision.

    SGD:    m = mu*m - lr*g ;  p = p + m                        (nesterov: p = p + mu*m - lr*g)             m starts at 0
    Adamax: m = m + (g - m)*(1 - b1) ;  u = max(b2*u, |g|) ;  p = p - lr*m / ((1 - b1^t)*(u + eps))          t 1-based
    Ftrl:   g' = g + 2*l2_shrinkage*p ;  n' = n + g^2 ;  linear = linear + g' - (n'^(-lr_power) - n^(-lr_power))/lr * p
            q = n'^(-lr_power)/lr + 2*l2' ;  p = (clip(linear, -l1, l1) - linear)/q ;  n = n'     l2' = l2 + beta/(2 lr)
            n starts at initial_accumulator_value, linear at 0; where q == 0 (n' == 0 and l2' == 0) p = 0 (Keras: NaN)

Sparse gradients (rows [n] int64, -1 = skipped; values [n, D]): duplicates are summed first (`optim_reference.summed`), every
looked-up row takes the update once, and every other row keeps its weights and slots — the row-sparse behaviour of the
library (TensorFlow's sparse apply), not Keras' dense one: Ftrl's shrinkage, for one, reaches the touched rows only."""
import torch

from tests.optim_reference import summed

SGD_DEFAULTS = dict(learning_rate=0.01, momentum=0.0, nesterov=False)
ADAMAX_DEFAULTS = dict(learning_rate=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-7)
FTRL_DEFAULTS = dict(learning_rate=1e-3, learning_rate_power=-0.5, initial_accumulator_value=0.1,
                     l1_regularization_strength=0.0, l2_regularization_strength=0.0,
                     l2_shrinkage_regularization_strength=0.0, beta=0.0)


def sgdm_step(p, g, m, lr=0.01, momentum=0.9, nesterov=False):
    m = momentum * m - lr * g
    return (p + momentum * m - lr * g if nesterov else p + m), m


def adamax_step(p, g, m, u, t, lr=1e-3, b1=0.9, b2=0.999, eps=1e-7):
    m = m + (g - m) * (1 - b1)
    u = torch.maximum(b2 * u, g.abs())
    return p - lr * m / ((1 - b1 ** t) * (u + eps)), m, u


def ftrl_step(p, g, n, linear, lr=1e-3, lr_power=-0.5, l1=0.0, l2=0.0, l2_shrinkage=0.0, beta=0.0):
    l2 = l2 + beta / (2.0 * lr)
    gs = g + 2 * l2_shrinkage * p
    n2 = n + g * g
    linear = linear + gs - (n2 ** -lr_power - n ** -lr_power) / lr * p
    q = n2 ** -lr_power / lr + 2 * l2
    num = linear.clamp(-l1, l1) - linear
    p = torch.where(q == 0, torch.zeros_like(p), num / torch.where(q == 0, torch.ones_like(q), q))
    return p, n2, linear


def rows_step(step, p, slots, rows, values, *args, **kw):
    """`step` (one of the dense functions above, slots passed and returned as a tuple) on the looked-up rows only"""
    g, touched = summed(rows, values, p.shape[0])
    out = step(p, g, *slots, *args, **kw)
    w = touched[:, None]
    return torch.where(w, out[0], p), tuple(torch.where(w, a, b) for a, b in zip(out[1:], slots))
