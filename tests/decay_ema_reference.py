# -*- coding:utf-8 -*-
"""Restatements of Keras 3's BaseOptimizer stages around the update step (written from the documented formulas; no Keras is
installed here): decoupled weight decay ahead of the update, the exponential moving average of the weights behind it.

  * float32, in the operation order csrc/optim_stages.hip states (numpy rounds every float32 operation, nothing contracts):
    `decay32`, `ema32`;
  * float64: `decay`, `ema`, the closed form for a row that sat out k steps `catch_up`, the dense average iterated over a
    recorded weight trajectory `ema_trajectory`, and Keras' Adam behind the decay, `adamw_steps`."""
import math

import numpy as np

F32 = np.float32


def decay32(p, wd, lr):
    """p - (p * wd) * lr, every operation rounded to float32"""
    p = np.asarray(p, dtype=F32)
    return p - (p * F32(wd)) * F32(lr)


def ema32(a, p, momentum, t):
    """step t (1-based): m_eff * a + (1 - m_eff) * p with m_eff = 0 at t == 1, every operation rounded to float32"""
    m = F32(0.0) if t == 1 else F32(momentum)
    a, p = np.asarray(a, dtype=F32), np.asarray(p, dtype=F32)
    return m * a + (F32(1.0) - m) * p


def decay(p, wd, lr):
    p = np.asarray(p, dtype=np.float64)
    return p - (p * wd) * lr


def ema(a, p, momentum, t):
    m = 0.0 if t == 1 else momentum
    return m * np.asarray(a, dtype=np.float64) + (1.0 - m) * np.asarray(p, dtype=np.float64)


def catch_up(a, w, momentum, k):
    """k average steps (none of them the first) on a constant weight w, in closed form: w + m^k (a - w)"""
    a, w = np.asarray(a, dtype=np.float64), np.asarray(w, dtype=np.float64)
    return w + momentum ** k * (a - w)


def ema_trajectory(weights, momentum):
    """the dense average iterated over the recorded weights [w_1, w_2, ..] (w_t: the weights after step t) -> after the last"""
    a = None
    for t, w in enumerate(weights, start=1):
        a = ema(np.zeros_like(w, dtype=np.float64) if a is None else a, w, momentum, t)
    return a


def adam_step(p, g, m, v, t, lr=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-7):
    """keras.optimizers.Adam's update_step at step t (1-based), float64 -> (p, m, v)"""
    alpha = lr * math.sqrt(1.0 - beta_2 ** t) / (1.0 - beta_1 ** t)
    m = m + (g - m) * (1.0 - beta_1)
    v = v + (g * g - v) * (1.0 - beta_2)
    return p - alpha * m / (np.sqrt(v) + epsilon), m, v


def adamw_steps(p, grads, wd, lr=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-7):
    """`Adam(weight_decay=wd)`: per step the decay with the plain lr, then Adam's update with the gradient as given -> p"""
    p = np.asarray(p, dtype=np.float64)
    m, v = np.zeros_like(p), np.zeros_like(p)
    for t, g in enumerate(grads, start=1):
        p = decay(p, wd, lr)
        p, m, v = adam_step(p, np.asarray(g, dtype=np.float64), m, v, t, lr, beta_1, beta_2, epsilon)
    return p
