# -*- coding:utf-8 -*-
"""Precision classes of the kernels, and the yardsticks that hold each kernel to the class it claims.

Metrics (kernel result `got` against the float64 reference `ref`):
  max_rel   max |e| / max |ref|                        (the blanket metric of the older tests)
  l2_rel    ||e||_2 / ||ref||_2
  row_rel   per row: max |e| / max |ref| of that row, then the max over the rows whose reference is not zero — a table
            row seen once, or one input feature's row of a weight gradient, is measured against itself
  cond_rms  per element: |e| / (|A| |B|) of the same contraction in float64 (`abs_scale`), then the root mean square
  elem_cond per element: |e| / (|A| |B|) of the same contraction, then the max (tests/test_pairwise_kernels_gpu.py)
  col_cond  per column of a column sum: |e| / sum_n |term| in float64, then the max over the columns (the BatchNorm backward
            sums, tests/test_bn_gpu.py)

Yardstick A (one GEMM-shaped product: dense, cin, cin_bf16, one cross layer): cond_rms <= COND_BAR[class].  The units are
those of tests/test_split_bf16_arithmetic.py, so the classes carry over: ~2^-24 for fp32 arithmetic and for six products of
three bf16 parts, 2^-16 / sqrt(K) for three products of two parts, 2^-9 / sqrt(K) .. 2^-8 for one bf16 product.  The root
mean square and not the max: over millions of elements the max is a tail statistic, and at K = 1664 the fp32 and
three-product maxima are only ~3x apart while their rms are ~12x apart (test_precision_classes.py).

Yardstick B (composed kernels: a whole fused step, the AutoInt layer): the same oracle evaluated in float32 on the CPU is
the fp32 class for that shape and data; err_gpu <= STEP_BAR[class] x max(err_f32, FLOOR) in the same metric.

A relu unit whose float64 input is within the forward's rounding of zero has no derivative two precisions agree on:
yardstick A zeroes the upstream gradient of those units, with a width that follows the forward's class (`kink_mask`);
whole steps of fp32-class forwards move the tower biases off them (`oracle.headline.shift_tower_biases`).  A plain-bf16
forward inside a whole step flips units no shift can clear: there only the forward figures are held to the class."""
import json
import math
import os

import torch

U = 2.0 ** -24          # the unit of the class bars: one fp32 rounding

# (kernel, mode) -> (forward class, backward class), as the kernels state it:
#   'fp32'  24 bits: exact fp32 arithmetic, or six products of three-part split-bf16 operands
#   'b17'   16 bits: three products of two-part operands (2^-17 per product)
#   'bf16'   8 bits: one bf16 x bf16 product (2^-9 per operand)
CLAIMS = {
    ('tower', 'bf16x3'): ('fp32', 'b17'),       # csrc/tower_x3.h:8-16; k_wgrad_rows' wgrad_heavy_bf16 (csrc/deepfm.hip)
    ('tower', 'f32'): ('fp32', 'fp32'),         # k_mlp_fwd3, wgrad_heavy
    ('tower', 'bf16'): ('bf16', 'bf16'),        # DT_STEP_TOWER_BF16: north_star's 1e-2 mode
    ('cin', 'float32'): ('fp32', 'fp32'),       # csrc/cin.hip
    ('cin', 'bf16x3'): ('fp32', 'b17'),         # csrc/cin_bf16.hip, NP = 3 forward / NP = 2 backward
    ('cin', 'bf16'): ('bf16', 'bf16'),          # csrc/cin_bf16.hip, NP = 1
    ('autoint', 'float32'): ('fp32', 'fp32'),   # csrc/autoint.hip, fp32 MFMA
    ('autoint', 'bf16x2'): ('fp32', 'b17'),     # DT_AI_BF16X2: six products forward, three backward
    ('autoint', 'bf16'): ('b17', 'bf16'),       # DT_AI_BF16: two-part forward projection, plain bf16 backward (autoint.hip:138-144)
    ('mha', 'float32'): ('fp32', 'fp32'),       # csrc/mha.hip: the attention core of every shape the fused layer does not take
    ('dense', 'float32'): ('fp32', 'fp32'),     # csrc/dense.hip
    ('cross', 'float32'): ('fp32', 'fp32'),     # csrc/cross.hip
    ('fm', 'float32'): ('fp32', 'fp32'),        # csrc/embedding.hip
    ('embed_fm_linear', 'float32'): ('fp32', 'fp32'),   # csrc/embedding.hip
    ('inner', 'float32'): ('fp32', 'fp32'),     # csrc/product.hip
    ('outer', 'float32'): ('fp32', 'fp32'),     # csrc/product.hip
    ('bilinear', 'float32'): ('fp32', 'fp32'),  # csrc/interaction.hip
    ('afm', 'float32'): ('fp32', 'fp32'),       # csrc/interaction.hip
    ('bn', 'float32'): ('fp32', 'fp32'),        # csrc/bn.hip
    ('field_pool', 'float32'): ('fp32', 'fp32'),    # csrc/interaction.hip: SENET squeeze
    ('field_scale', 'float32'): ('fp32', 'fp32'),   # csrc/interaction.hip: SENET re-weight
}

# Yardstick A: bar on cond_rms, per class, in units U = 2^-24.  "GPU worst" is the largest figure test_precision_gpu.py
# measured on the MI355X for a kernel that claims the class; "next class" is the numpy emulation of the class below it at
# the same K (test_precision_classes.py, K = 16 .. 1664):
#   fp32: GPU worst 0.90 U (dense dW at K = 5), 0.62 U (cin dW, K = 16);   three products: 28 U (K = 16), 5.5 U (K = 448),
#         2.9 U (K = 1664).  The two classes are only ~12x apart in rms at K = 1664, so no bar keeps 3x on both sides
#         there: this one sits 2.2x over the worst measured and rejects the three-product emulation at every K (by 1.4x
#         at K = 1664, 2.7x at 448, 14x at 16).
#   b17:  GPU worst 40 U (cin bf16x3 dW, K = 16);   plain bf16: 1500 U (K = 1664) .. 15000 U (K = 16)
#   bf16: GPU worst 2.5e4 U (cin NP = 1 dW, K = 16); the bar is 2^-8, the most one bf16 product per operand pair can lose
#         per term: the loosest class claimed, nothing below it is told apart
COND_BAR = {'fp32': 2.0 * U, 'b17': 128 * U, 'bf16': 65536 * U}

# Yardstick B: factor over the float32 CPU oracle's own error, per class, and the floor of that error.
#   fp32: GPU worst 5.1x (SENET mean pooling, D = 33 summed in order), 4.2x (BN moving mean, mean 0 / std 1 at N = 16385), 3.7x (BN gamma
#         through the timed step's m, exact tower), 2.5x (bilinear dx, outer product dW);   the attention core (csrc/mha.hip,
#         tests/test_mha_kernels_gpu.py, max_rel and row_rel over 80 runs): grad_q 3.6x, out 2.1x, lse 2.1x, grad_v 2.1x, grad_k 1.5x,
#         through ops.dense + split_cols + mha_core: grad_x 1.2x, grad_b 0.9x, grad_W 0.7x;   a two-part (16-bit) tower forward: logits
#         ~40x (2e-5 against 5.3e-7)
#   b17:  GPU worst 59x (autoint bf16x2 dx), 52x (timed step BN gamma, wgrad_heavy_bf16);   an 8-bit backward: >= 2e3x
#   bf16: GPU worst 2.3e4x (autoint bf16 dx), 1.3e4x (plain-bf16 tower logits)
STEP_BAR = {'fp32': 12.0, 'b17': 200.0, 'bf16': 8.0e4}
FLOOR = U


def _d(t):
    return t.detach().to('cpu', torch.float64)


def max_rel(got, ref):
    got, ref = _d(got).reshape(-1), _d(ref).reshape(-1)
    return (got - ref).abs().max().item() / max(ref.abs().max().item(), 1e-300)


def l2_rel(got, ref):
    got, ref = _d(got).reshape(-1), _d(ref).reshape(-1)
    return (got - ref).norm().item() / max(ref.norm().item(), 1e-300)


def row_rel(got, ref):
    got, ref = _d(got), _d(ref)
    got, ref = got.reshape(ref.shape[0], -1), ref.reshape(ref.shape[0], -1)
    top = ref.abs().amax(1)
    live = top > 0
    if not bool(live.any()):
        return (got - ref).abs().max().item()
    return ((got - ref).abs().amax(1)[live] / top[live]).max().item()


def col_cond(got, ref, scale):
    """per column: |got - ref| / scale, then the max over the columns — for a column sum of N signed terms, with `scale` the
    sum of the terms' magnitudes in float64 (a sum near zero has no relative error two summation orders agree on).  A
    column whose scale is zero has only zero terms and the sum zero: its error counts as it is, as row_rel counts the
    error against a reference that is zero everywhere."""
    err, scale = (_d(got).reshape(-1) - _d(ref).reshape(-1)).abs(), _d(scale).reshape(-1)
    live = scale > 0
    return max((err[live] / scale[live]).max().item() if bool(live.any()) else 0.0,
               err[~live].max().item() if not bool(live.all()) else 0.0)


def elem_cond(got, ref, scale):
    """per element: |got - ref| / scale, then the max over the elements — `scale` the |A| |B| of the same contraction
    (`abs_scale`).  For a tensor whose rows mix magnitudes (fields scaled 1e-3 .. 1e3) or whose terms cancel, where row_rel
    measures the small entries against the row's largest.  An element whose scale is zero has only zero terms: its error
    counts as it is."""
    return col_cond(got, ref, scale)


def cond_rms(got, ref, scale):
    """root mean square of |got - ref| / scale over the elements with a nonzero scale"""
    got, ref, scale = _d(got).reshape(-1), _d(ref).reshape(-1), _d(scale).reshape(-1)
    live = scale > 0
    assert bool(live.any())
    return ((got - ref).abs()[live] / scale[live]).pow(2).mean().sqrt().item()


def abs_scale(fn, inputs, up):
    """|A| |B| of every contraction in `fn`: fn (sums and products only, no activation) on |inputs| in float64, backward of
    |up| -> (output scale, [scale of each input's gradient])"""
    xs = [None if t is None else _d(t).abs().requires_grad_(True) for t in inputs]
    y = fn(*xs)
    (y * _d(up).abs()).sum().backward()
    return y.detach(), [None if t is None else t.grad for t in xs]


# per-element reach of each class, in units of the contraction's |A| |B|: a relu unit whose float64 pre-activation lies
# closer to zero than this may take either derivative in a kernel of that class (fp32: a few roundings; three products:
# 2^-16 per product; one bf16 product: 2^-8 per term)
KINK_TOL = {'fp32': 2.0 ** -20, 'b17': 2.0 ** -14, 'bf16': 2.0 ** -7}


def kink_mask(pre, scale, up, act, cls):
    """`up` with the units of a relu zeroed whose float64 pre-activation `pre` lies within KINK_TOL[cls] x `scale` (|A| |B|
    of the forward contraction) of zero — the units a forward of class `cls` may put on either side of the kink.  relu'
    itself is the caller's to apply."""
    if act != 'relu':
        return up
    near = _d(pre).abs() < KINK_TOL[cls] * _d(scale)
    return torch.where(near, torch.zeros_like(up), up)


def abs_forward(fn, inputs):
    """|A| |B| of the forward contraction alone: fn on |inputs| in float64"""
    with torch.no_grad():
        return fn(*[None if t is None else _d(t).abs() for t in inputs])


def bar_of(kernel, mode, direction):
    return CLAIMS[(kernel, mode)][0 if direction == 'fwd' else 1]


def record(test, **figures):
    """DT_PRECISION_LOG=<file>: append the measured figures (the calibration of the bars above)"""
    path = os.environ.get('DT_PRECISION_LOG')
    if path:
        with open(path, 'a') as f:
            f.write(json.dumps({'test': test, **{k: (float(v) if isinstance(v, (int, float)) else v)
                                                 for k, v in figures.items()}}) + '\n')


def check_cond(test, kernel, mode, figures):
    """figures: {name: (direction, cond_rms)}; every figure within the bar of its direction's class"""
    record(test, **{k: v / U for k, (_, v) in figures.items()})
    bad = {k: (v / U, COND_BAR[bar_of(kernel, mode, d)] / U) for k, (d, v) in figures.items()
           if not v <= COND_BAR[bar_of(kernel, mode, d)]}
    assert not bad, f'{kernel}/{mode}: cond_rms in units of 2^-24 (measured, bar): {bad}'


def check_step(test, kernel, mode, figures):
    """figures: {name: (direction, err_gpu, err_f32)}; err_gpu <= STEP_BAR[class] x max(err_f32, FLOOR)"""
    ratios = {k: g / max(f, FLOOR) for k, (_, g, f) in figures.items()}
    record(test, **ratios)
    bad = {k: (ratios[k], STEP_BAR[bar_of(kernel, mode, d)], g, f) for k, (d, g, f) in figures.items()
           if not (math.isfinite(ratios[k]) and ratios[k] <= STEP_BAR[bar_of(kernel, mode, d)])}
    assert not bad, f'{kernel}/{mode}: err_gpu / max(err_f32, 2^-24) (measured, bar, err_gpu, err_f32): {bad}'
