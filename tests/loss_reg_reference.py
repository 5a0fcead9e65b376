# -*- coding:utf-8 -*-
"""Keras 3's regression losses and the GHM-C loss restated in torch, in whatever precision the inputs carry (float64: the
reference; float32 on the CPU: the fp32 class of yardstick B) — the contract of csrc/loss_reg.hip (dt_loss_reg, dt_ghmc).
Gradients come from autograd on these forms, never from a second derivation.

    total = sum_b w_b mean_c f(p, t) / B          (Keras SUM_OVER_BATCH_SIZE; w_b = 1 without weights), e = p - t, eps = 1e-7

    huber      f = 0.5 e^2 where |e| <= delta, else delta |e| - 0.5 delta^2
    log_cosh   f = log cosh e.  Keras writes e + softplus(-2e) - ln 2; that is the float32 restatement.  It cancels for small
               e even in float64 (1e-16 absolute against a value of e^2 / 2), so the float64 REFERENCE is the identical
               log1p(2 sinh^2(e / 2)), which does not
    msle       f = (log(max(p, eps) + 1) - log(max(t, eps) + 1))^2; torch's clamp passes the gradient at p == eps
    mape       f = 100 |(t - p) / max(|t|, eps)|
    poisson    f = p - t log(p + eps)

    ghmc       GHMCLoss.calc with a mask (oracle.reference_layers.ghmc_loss is the case without one)

Kinks, where two precisions need not agree: e = 0 for mape (the derivative jumps), p = eps for msle, p + eps = 0 for poisson
(the value becomes NaN), and for GHM-C every bin edge (an element changes its bin, and with it every weight).  `kink_margin`
measures the distance of the nearest element from its kind's kink on the float64 reference.  Huber's kink at |e| = delta is
continuous in value and gradient and needs no margin."""
import math

import torch

KINDS = ('huber', 'log_cosh', 'msle', 'mape', 'poisson')
EPS = 1e-7


def kind_code(kind):
    from deeptables_amd import _lib
    return {'huber': _lib.DT_LOSS_HUBER, 'log_cosh': _lib.DT_LOSS_LOG_COSH, 'msle': _lib.DT_LOSS_MSLE,
            'mape': _lib.DT_LOSS_MAPE, 'poisson': _lib.DT_LOSS_POISSON}[kind]


def per_element(kind, p, t, delta=1.0):
    e = p - t
    if kind == 'huber':
        a = e.abs()
        return torch.where(a <= delta, 0.5 * e * e, delta * a - 0.5 * delta * delta)
    if kind == 'log_cosh':
        if p.dtype == torch.float64:
            return torch.log1p(2.0 * torch.sinh(0.5 * e) ** 2)
        return e + torch.nn.functional.softplus(-2.0 * e) - math.log(2.0)
    if kind == 'msle':
        return (torch.log(torch.clamp(p, min=EPS) + 1.0) - torch.log(torch.clamp(t, min=EPS) + 1.0)) ** 2
    if kind == 'mape':
        return 100.0 * ((t - p) / torch.clamp(t.abs(), min=EPS)).abs()
    if kind == 'poisson':
        return p - t * torch.log(p + EPS)
    raise ValueError(kind)


def total(kind, p, t, w=None, delta=1.0):
    """the scalar loss of predictions p [B, C] and targets t [B, C] with per-row weights w [B] (None: 1)"""
    B = p.shape[0]
    per = per_element(kind, p, t, delta).mean(-1)
    if w is not None:
        per = per * w.reshape(B).to(per.dtype)
    return per.sum() / B


def value_and_grad(kind, p, t, w=None, delta=1.0, dtype=torch.float64):
    """(loss, d loss / d p) by autograd in `dtype` on the CPU, both returned as float64"""
    p = p.detach().to('cpu', dtype).clone().requires_grad_(True)
    t = t.detach().to('cpu', dtype)
    w = None if w is None else w.detach().to('cpu', dtype)
    loss = total(kind, p, t, w, delta)
    (dz,) = torch.autograd.grad(loss, p)
    return loss.detach().double(), dz.double()


def ghmc_edges(bins, dtype):
    left = torch.tensor([float(x) / bins for x in range(bins)], dtype=dtype)
    right = [float(x) / bins for x in range(1, bins + 1)]
    right[-1] += 1e-6
    return left, torch.tensor(right, dtype=dtype)


def ghmc(input, target, acc_sum, bins=10, momentum=0.75, mask=None):
    """GHMCLoss.calc (layers.py:1111-1163) with is_mask = (mask is not None), in the dtype of `input`.
    Returns (loss, updated acc_sum)."""
    dt = input.dtype
    left, right = ghmc_edges(bins, dt)
    left, right = left.reshape(bins, 1, 1), right.reshape(bins, 1, 1)
    g = torch.abs(torch.sigmoid(input) - target).detach().unsqueeze(0)
    in_bin = (g >= left) & (g < right)
    if mask is not None:
        pos = mask.reshape(input.shape) > 0
        inds = (in_bin & pos).to(dt)
        tot = torch.clamp(pos.to(dt).sum(), min=1.0)
    else:
        inds = in_bin.to(dt)
        tot = torch.tensor(max(float(input.numel()), 1.0), dtype=dt)
    num = inds.sum(dim=(1, 2))
    nonempty = num > 0
    nvalid = nonempty.to(dt).sum()
    if momentum > 0:
        acc_sum = torch.where(nonempty, momentum * acc_sum + (1 - momentum) * num, acc_sum)
        denom = acc_sum.reshape(-1, 1, 1) + torch.zeros_like(inds)
    else:
        denom = num.reshape(-1, 1, 1) + torch.zeros_like(inds)
    weights = torch.where(inds == 1, tot / denom, torch.zeros_like(inds)).sum(0) / nvalid
    loss = torch.clamp(input, min=0) - input * target + torch.log1p(torch.exp(-torch.abs(input)))
    return torch.sum(loss * weights) / tot, acc_sum


def ghmc_counts(input, target, bins, mask=None):
    """the integer count of every bin from the float64 gradient lengths -> int64 [bins]"""
    z, t = input.detach().double(), target.detach().double()
    left, right = ghmc_edges(bins, torch.float32)
    g = (torch.sigmoid(z) - t).abs().reshape(1, -1)
    inb = (g >= left.double().reshape(-1, 1)) & (g < right.double().reshape(-1, 1))
    if mask is not None:
        inb = inb & (mask.reshape(1, -1) > 0)
    return inb.sum(1)


def kink_margin(kind, z, t, bins=None):
    """distance of the nearest element from the kink of its kind, on the float64 reference (inf: the kind has none)"""
    z, t = z.detach().to('cpu', torch.float64), t.detach().to('cpu', torch.float64)
    if kind == 'mape':
        return float((z - t).abs().min())
    if kind == 'msle':
        return float((z - EPS).abs().min())
    if kind == 'poisson':
        return float((z + EPS).abs().min())
    if kind == 'ghmc':
        left, right = ghmc_edges(bins, torch.float32)         # the float32 edges every precision compares against
        edges = torch.cat([left, right[-1:]]).double()
        g = (torch.sigmoid(z) - t).abs().reshape(-1, 1)
        return float((g - edges.reshape(1, -1)).abs().min())
    return math.inf
