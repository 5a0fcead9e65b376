# -*- coding:utf-8 -*-
"""Plain restatement of keras.layers.BatchNormalization over the last axis, in whatever dtype `x` has (float64: the
reference; float32: the fp32 class of tests/precision.py's yardstick B).

Unlike oracle.reference_layers.keras_batchnorm it takes gamma=None (scale=False) and / or beta=None (center=False), any eps
and momentum, inputs of rank 2 or 3, and it also returns what the kernels of csrc/bn.hip save and reduce: the batch mean and
rstd, and for an upstream gradient `gy` the two backward sums  sum_g = sum_n gy  and  sum_gx = sum_n gy * xhat  (= the
gradients of beta and gamma).  `y` stays on the autograd tape: dx, dgamma and dbeta are taken by autograd on this function."""
import collections

import torch

BN = collections.namedtuple('BN', 'y moving_mean moving_var mean rstd sum_g sum_gx')


def keras_batchnorm(x, gamma=None, beta=None, moving_mean=None, moving_var=None, training=True, eps=1e-3, momentum=0.99,
                    gy=None):
    """x [..., C] of rank 2 or 3 -> BN.  training: the batch statistics (biased variance) normalise, and the moving
    statistics move by  m * momentum + batch * (1 - momentum)  with the same biased variance; otherwise the moving statistics
    normalise and come back unchanged.  mean / rstd are what normalised; sum_g / sum_gx are None without `gy`."""
    if x.dim() not in (2, 3):
        raise ValueError(f'keras_batchnorm: rank 2 or 3, got {x.dim()}')
    red = tuple(range(x.dim() - 1))
    if training:
        mean = x.mean(dim=red)
        var = ((x - mean) ** 2).mean(dim=red)                            # biased
        nm = None if moving_mean is None else moving_mean * momentum + mean.detach() * (1 - momentum)
        nv = None if moving_var is None else moving_var * momentum + var.detach() * (1 - momentum)
    else:
        mean, var, nm, nv = moving_mean, moving_var, moving_mean, moving_var
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = (x - mean) * rstd
    y = xhat
    if gamma is not None:
        y = y * gamma
    if beta is not None:
        y = y + beta
    sum_g = sum_gx = None
    if gy is not None:
        with torch.no_grad():
            sum_g = gy.to(x.dtype).sum(dim=red)
            sum_gx = (gy.to(x.dtype) * xhat).sum(dim=red)
    return BN(y, nm, nv, mean.detach(), rstd.detach(), sum_g, sum_gx)


def sum_scales(x, gy, eps=1e-3):
    """(sum_n |gy|, sum_n |gy * xhat|) per column in float64: what one rounding of a term of sum_g / sum_gx is measured
    against (a sum of N signed terms is ill-conditioned: its error is relative to the sum of the magnitudes)."""
    x, gy = x.detach().double(), gy.detach().double()
    red = tuple(range(x.dim() - 1))
    mean = x.mean(dim=red)
    var = ((x - mean) ** 2).mean(dim=red)
    xhat = (x - mean) / torch.sqrt(var + eps)
    return gy.abs().sum(dim=red), (gy * xhat).abs().sum(dim=red)
