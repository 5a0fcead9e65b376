# -*- coding:utf-8 -*-
"""The losses of a train step restated from the LOGITS in torch, in whatever precision the inputs carry (float64: the
reference; float32 on the CPU: the fp32 class of yardstick B) — the contract of csrc/loss.hip (dt_loss) and of
losses.device_loss.  Gradients come from autograd on these forms, never from a second derivation.

    total = sum_b w_b l_b / B             (Keras SUM_OVER_BATCH_SIZE; w_b = sample_weight x class_weight, 1 without weights)

    bce                l_b = mean_c max(z,0) - z t + log1p(exp(-|z|))        (oracle.reference_layers.binary_crossentropy_from_logits
                       is its unweighted mean over all elements), written here as the identical -t log sigmoid(z) - (1 - t) log
                       sigmoid(-z): the stable form has two kinks at z = 0 that cancel (clamp and |z|), and autograd adds their
                       one-sided derivatives to 1 - t there instead of sigmoid(0) - t
    cce                l_b = -sum_c t_c log_softmax(z)_c                      (soft labels need not sum to 1)
    mse / mae          l_b = mean_c (z - t)^2 / mean_c |z - t|
    categorical_focal  l_b = oracle.reference_layers.categorical_focal_loss(t, softmax(z))_b        (layers.py:1062-1076)
    binary_focal       total = oracle.reference_layers.binary_focal_loss(t, sigmoid(z))             (layers.py:1006-1017) — one
                       scalar already averaged over batch and classes: it takes no per-row weight

The focal losses clamp the probabilities to [eps, 1 - eps], eps = 1e-7: the loss has a kink where a probability crosses a
bound (the derivative jumps to zero), so two precisions agree only on inputs that keep away from it.  `clamp_margin` measures
that distance on the float64 reference: |z| against ln((1 - eps) / eps) = 16.1181 for the binary loss, log p against ln eps
and ln(1 - eps) for the categorical one."""
import math

import torch

from oracle import reference_layers as R

KINDS = ('bce', 'cce', 'mse', 'mae', 'binary_focal', 'categorical_focal')
ELEMENTWISE = ('bce', 'mse', 'mae', 'binary_focal')
CATEGORICAL = ('cce', 'categorical_focal')
EPS = 1e-7
Z_CLAMP = math.log((1.0 - EPS) / EPS)            # 16.1181: sigmoid(z) leaves [eps, 1 - eps] beyond it
LOG_EPS, LOG_ONE_MINUS_EPS = math.log(EPS), math.log1p(-EPS)


def kind_code(kind):
    from deeptables_amd import _lib
    return {'bce': _lib.DT_LOSS_BCE, 'cce': _lib.DT_LOSS_CCE, 'mse': _lib.DT_LOSS_MSE, 'mae': _lib.DT_LOSS_MAE,
            'binary_focal': _lib.DT_LOSS_BINARY_FOCAL, 'categorical_focal': _lib.DT_LOSS_CATEGORICAL_FOCAL}[kind]


def per_row(kind, z, t, gamma=2.0, alpha=0.25):
    """l_b [B] of a per-row kind, in the dtype of z"""
    if kind == 'bce':
        ls = torch.nn.functional.logsigmoid
        return (-t * ls(z) - (1.0 - t) * ls(-z)).mean(-1)
    if kind == 'cce':
        return -(t * torch.log_softmax(z, dim=-1)).sum(-1)
    if kind == 'mse':
        return ((z - t) ** 2).mean(-1)
    if kind == 'mae':
        return (z - t).abs().mean(-1)
    if kind == 'categorical_focal':
        return R.categorical_focal_loss(t, torch.softmax(z, dim=-1), gamma=gamma, alpha=alpha)
    raise ValueError(kind)


def total(kind, z, t, w=None, gamma=2.0, alpha=0.25):
    """the scalar loss of logits z [B, C] and targets t [B, C] with per-row weights w [B] (None: 1)"""
    B = z.shape[0]
    if kind == 'binary_focal':
        if w is not None:
            raise ValueError('the binary focal loss is one mean over all elements: it takes no per-row weight')
        return R.binary_focal_loss(t, torch.sigmoid(z), gamma=gamma, alpha=alpha)
    per = per_row(kind, z, t, gamma, alpha)
    if w is not None:
        per = per * w.reshape(B).to(per.dtype)
    return per.sum() / B


def value_and_grad(kind, z, t, w=None, gamma=2.0, alpha=0.25, dtype=torch.float64):
    """(loss, d loss / d z) by autograd in `dtype` on the CPU, both returned as float64"""
    z = z.detach().to('cpu', dtype).clone().requires_grad_(True)
    t = t.detach().to('cpu', dtype)
    w = None if w is None else w.detach().to('cpu', dtype)
    loss = total(kind, z, t, w, gamma, alpha)
    (dz,) = torch.autograd.grad(loss, z)
    return loss.detach().double(), dz.double()


def clamp_margin(kind, z):
    """distance of the nearest element from a clamp bound of a focal loss, on the float64 reference (inf for the others)"""
    z = z.detach().to('cpu', torch.float64)
    if kind == 'binary_focal':
        return float((z.abs() - Z_CLAMP).abs().min())
    if kind == 'categorical_focal':
        lp = torch.log_softmax(z, dim=-1)
        return float(torch.minimum((lp - LOG_EPS).abs(), (lp - LOG_ONE_MINUS_EPS).abs()).min())
    return math.inf
