# -*- coding:utf-8 -*-
"""The losses of a train step (keras.losses.* selected by DeepModel.__compile_model, deepmodel.py:324-338, and the layers
module's focal and GHM-C losses): value and gradient from the model output in a few HIP launches (csrc/loss.hip,
csrc/loss_reg.hip), and ONE torch statement of each named formula (`_per_row_loss`) for everything outside the kernels'
domain.  `named_loss` serves the loss strings, `focal_from_logits` and `ghmc_from_logits` the loss objects."""
import ctypes
import math
import os

import torch

from . import _lib
from ._lib import check, lib, ptr, stream_ptr

_UNIT_GRAD = {}


def unit_grad(device):
    """the constant 1.0 `loss.backward()` would allocate and fill at every step: a cached 0-dim tensor per device.  A loss
    function that sees it as its incoming gradient (same storage) skips the multiplication by it."""
    key = str(device)
    if key not in _UNIT_GRAD:
        _UNIT_GRAD[key] = torch.ones((), dtype=torch.float32, device=device)
    return _UNIT_GRAD[key]


def _is_unit_grad(g):
    u = _UNIT_GRAD.get(str(g.device))
    return u is not None and g.dim() == 0 and g.data_ptr() == u.data_ptr()


LOSS_KINDS = {'binary_crossentropy': _lib.DT_LOSS_BCE, 'categorical_crossentropy': _lib.DT_LOSS_CCE,
              'mse': _lib.DT_LOSS_MSE, 'mean_squared_error': _lib.DT_LOSS_MSE,
              'mae': _lib.DT_LOSS_MAE, 'mean_absolute_error': _lib.DT_LOSS_MAE}
# Keras' regression losses (csrc/loss_reg.hip, dt_loss_reg): they see the model's OUTPUT, which is the logit for the regression
# task only — any other task evaluates the torch restatement on the activated output
REG_LOSS_KINDS = {'huber': _lib.DT_LOSS_HUBER, 'log_cosh': _lib.DT_LOSS_LOG_COSH, 'logcosh': _lib.DT_LOSS_LOG_COSH,
                  'msle': _lib.DT_LOSS_MSLE, 'mean_squared_logarithmic_error': _lib.DT_LOSS_MSLE,
                  'mape': _lib.DT_LOSS_MAPE, 'mean_absolute_percentage_error': _lib.DT_LOSS_MAPE,
                  'poisson': _lib.DT_LOSS_POISSON}
LOSS_KINDS.update(REG_LOSS_KINDS)
LOSS_NAMES = tuple(LOSS_KINDS)            # the loss strings DeepModel compiles
_CATEGORICAL_KINDS = (_lib.DT_LOSS_CCE, _lib.DT_LOSS_CATEGORICAL_FOCAL)
K_EPSILON = 1e-7            # keras.backend.epsilon()


def _on_device(t):
    return torch.is_tensor(t) and t.is_cuda


def device_loss_enabled():
    """DT_AMD_DEVICE_LOSS=0 restores the torch op chains everywhere (the comparison leg of the tests and of
    tools/loss_bench.py)"""
    return os.environ.get('DT_AMD_DEVICE_LOSS', '1') != '0'


# ---------------------------------------------------------------------------------------------
# the library calls as autograd functions
# ---------------------------------------------------------------------------------------------
class _LossFunction(torch.autograd.Function):
    """A loss entry point of the library: loss and d loss / d z together in the forward, dz written only when z asks for a
    gradient (evaluate runs under no_grad: value only).  backward hands out the saved dz itself when the incoming gradient is
    `unit_grad`, else one multiply.  A subclass' forward holds its library call; z is its first input."""

    @staticmethod
    def launch(ctx, entry, shape, z, want_dz, head):
        """`entry`(*head, loss, dz, workspace, stream) over the workspace that `entry`_workspace_bytes(*shape) asks for"""
        h = lib()
        need = getattr(h, entry + '_workspace_bytes')(*shape)
        if need < 0:
            check(int(need), entry + '_workspace_bytes')
        # one allocation: the loss word (8 bytes, so that the partials behind it are 8-byte aligned), then the workspace
        buf = torch.empty(2 + int(need) // 4, dtype=torch.float32, device=z.device)
        dz = torch.empty_like(z) if want_dz else None
        check(getattr(h, entry)(*head, ptr(buf), ptr(dz), ctypes.c_void_p(buf.data_ptr() + 8), stream_ptr()), entry)
        if dz is not None:
            ctx.save_for_backward(dz)
        return buf[0]

    @staticmethod
    def backward(ctx, g):
        (dz,) = ctx.saved_tensors
        return (dz if _is_unit_grad(g) else dz * g,) + (None,) * (len(ctx.needs_input_grad) - 1)


def _contiguous(*tensors):
    return [None if t is None else t.contiguous() for t in tensors]


class _BceFromLogits(_LossFunction):
    """dt_bce_logits: no workspace, dz always"""

    @staticmethod
    def forward(ctx, z, y):
        z, y = _contiguous(z, y)
        loss = torch.empty(1, dtype=torch.float32, device=z.device)
        dz = torch.empty_like(z)
        check(lib().dt_bce_logits(ptr(z), ptr(y), z.numel(), ptr(loss), ptr(dz), stream_ptr()), 'dt_bce_logits')
        ctx.save_for_backward(dz)
        return loss[0]


class _DeviceLoss(_LossFunction):
    @staticmethod
    def forward(ctx, z, t, w, kind, gamma, alpha, want_dz):
        z, t, w = _contiguous(z, t, w)
        rows, classes = z.shape
        return _LossFunction.launch(ctx, 'dt_loss', (rows, classes), z, want_dz,
                                    (int(kind), ptr(z), ptr(t), ptr(w), rows, classes, float(gamma), float(alpha)))


class _DeviceRegLoss(_LossFunction):
    @staticmethod
    def forward(ctx, p, t, w, kind, delta, want_dz):
        p, t, w = _contiguous(p, t, w)
        rows, classes = p.shape
        return _LossFunction.launch(ctx, 'dt_loss_reg', (rows, classes), p, want_dz,
                                    (int(kind), ptr(p), ptr(t), ptr(w), rows, classes, float(delta)))


class _DeviceGhmc(_LossFunction):
    """dt_ghmc: GHMCLoss.calc's value, gradient and in-place `acc_sum` update in at most four launches"""

    @staticmethod
    def forward(ctx, z, t, mask, acc, bins, momentum, want_dz):
        z, t = _contiguous(z, t)
        n, bins, momentum = z.numel(), int(bins), float(momentum)
        # float32(1 - momentum) rounded from the double, as torch rounds the scalar of `(1 - mmt) * num_in_bin`
        return _LossFunction.launch(ctx, 'dt_ghmc', (n, bins), z, want_dz,
                                    (ptr(z), ptr(t), ptr(mask), n, bins, momentum, 1.0 - momentum, ptr(acc)))


# ---------------------------------------------------------------------------------------------
# dispatch
# ---------------------------------------------------------------------------------------------
def device_loss_supported(kind, z, t, w=None):
    """True when `device_loss` serves this call: DT_AMD_DEVICE_LOSS not '0', float32 tensors on the GPU, z [rows, classes]
    inside dt_loss' domain with as many targets, one weight per row — and none for the binary focal loss"""
    if not device_loss_enabled():
        return False
    if not (_on_device(z) and z.dtype == torch.float32 and z.dim() == 2 and _on_device(t) and t.dtype == torch.float32 and
            t.shape == z.shape):
        return False
    rows, classes = z.shape
    if not (1 <= rows < (1 << 31) and 1 <= classes <= _lib.DT_LOSS_MAX_CLASSES and rows * classes < (1 << 40)):
        return False
    if kind in _CATEGORICAL_KINDS and classes < 2:
        return False
    if w is not None:
        if kind == _lib.DT_LOSS_BINARY_FOCAL:
            return False
        if not (_on_device(w) and w.dtype == torch.float32 and w.numel() == rows):
            return False
    return True


def _device_loss(kind, z, t, w, gamma=0.0, alpha=0.0, delta=1.0):
    """`device_loss` behind its reshapes: z and t [rows, classes], w [rows] or None"""
    if not device_loss_supported(kind, z, t, w):
        return None
    want_dz = torch.is_grad_enabled() and z.requires_grad
    if kind >= _lib.DT_LOSS_HUBER:
        return _DeviceRegLoss.apply(z, t, w, kind, delta, want_dz)
    return _DeviceLoss.apply(z, t, w, kind, gamma, alpha, want_dz)


def device_loss(kind, out, y, w=None, gamma=0.0, alpha=0.0, delta=1.0):
    """The loss `kind` (any DT_LOSS_*) of the model output [B, ...] — the logits, for the kinds of dt_loss — against targets y
    with per-row weights w [B] (None: 1) through dt_loss (kinds 0-5) or dt_loss_reg (kinds 6-10), or None when the call is
    outside `device_loss_supported` — the caller then takes its torch path."""
    B = out.shape[0]
    if B == 0 or y.numel() != out.numel():
        return None
    z = out.reshape(B, -1)
    t = y.reshape(z.shape)
    t = t if t.dtype == z.dtype else t.to(z.dtype)
    return _device_loss(kind, z, t, None if w is None else w.reshape(-1), gamma, alpha, delta)


def _per_row_loss(loss_name, z, t, delta=1.0):
    """l_b [B] of a named loss in torch ops, in the dtype of z: the definition the kernels are held to (Keras 3's own forms)"""
    kind = LOSS_KINDS.get(loss_name)
    if kind == _lib.DT_LOSS_HUBER:
        e = z - t
        a = e.abs()
        return torch.where(a <= delta, 0.5 * e * e, delta * a - 0.5 * delta * delta).mean(-1)
    if kind == _lib.DT_LOSS_LOG_COSH:
        e = z - t
        return (e + torch.nn.functional.softplus(-2.0 * e) - math.log(2.0)).mean(-1)
    if kind == _lib.DT_LOSS_MSLE:
        d = torch.log(torch.clamp(z, min=K_EPSILON) + 1.0) - torch.log(torch.clamp(t, min=K_EPSILON) + 1.0)
        return (d * d).mean(-1)
    if kind == _lib.DT_LOSS_MAPE:
        return 100.0 * ((t - z) / torch.clamp(t.abs(), min=K_EPSILON)).abs().mean(-1)
    if kind == _lib.DT_LOSS_POISSON:
        return (z - t * torch.log(z + K_EPSILON)).mean(-1)
    if kind == _lib.DT_LOSS_BCE:
        return (torch.clamp(z, min=0) - z * t + torch.log1p(torch.exp(-z.abs()))).mean(-1)
    if kind == _lib.DT_LOSS_CCE:
        return -(torch.log_softmax(z, dim=-1) * t).sum(-1)
    if kind == _lib.DT_LOSS_MSE:
        return ((z - t) ** 2).mean(-1)
    if kind == _lib.DT_LOSS_MAE:
        return (z - t).abs().mean(-1)
    raise ValueError(f'Unsupported loss: {loss_name}')


def check_huber_delta(delta):
    delta = float(delta)
    if not (math.isfinite(delta) and delta > 0):
        raise ValueError(f'Huber: delta must be finite and > 0, got {delta!r}')
    return delta


def named_loss(name, out, y, w=None, delta=1.0, device=True):
    """The loss string `name` (LOSS_NAMES) of the model output `out` [B, ...] against y with Keras' `sample_weight` /
    `class_weight` semantics, reduction SUM_OVER_BATCH_SIZE: per-row loss times the row's weight w [B] (None: 1), summed,
    divided by the batch size.  `out` is the logits for the crossentropies.  Float32 GPU tensors: one dt_bce_logits launch for
    the unweighted binary crossentropy, `device_loss` for everything else.  CPU tensors, other dtypes, DT_AMD_DEVICE_LOSS=0 and
    device=False (an output that is an activation of the logits: autograd carries the gradient through it): `_per_row_loss`
    in torch ops."""
    if name not in LOSS_KINDS:
        raise ValueError(f'Unsupported loss: {name}')
    kind = LOSS_KINDS[name]
    B = y.shape[0]
    z = out.reshape(B, -1)
    if y.numel() != z.numel():
        raise ValueError(f'loss {name!r}: targets of shape {tuple(y.shape)} for an output of shape {tuple(out.shape)}')
    t = y.reshape(z.shape)
    t = t if t.dtype == z.dtype else t.to(z.dtype)
    w = None if w is None else w.reshape(-1).to(z.dtype)
    if kind == _lib.DT_LOSS_HUBER:
        delta = check_huber_delta(delta)
    if device:
        if kind == _lib.DT_LOSS_BCE and w is None:
            loss = _BceFromLogits.apply(z, t) if z.is_cuda and z.dtype == torch.float32 else None
        else:
            loss = _device_loss(kind, z, t, w, delta=delta)
        if loss is not None:
            return loss
    per = _per_row_loss(name, z, t, delta)
    return per.mean() if w is None else (per * w).sum() / B


def focal_from_logits(kind, loss_obj, logit, y, w, activate):
    """layers.BinaryFocalLoss / CategoricalFocalLoss (reduction 'auto') of a step: from the logits through dt_loss on the
    device, carrying the object's gamma and alpha; otherwise the object's own `call` on `activate(logit)` — for the
    categorical loss, whose `call` returns one value per row, with Keras' per-row weights."""
    if _on_device(logit):
        loss = device_loss(kind, logit, y, w, loss_obj.gamma, loss_obj.alpha)
        if loss is not None:
            return loss
    if w is None:
        return loss_obj(y, activate(logit))
    B = y.shape[0]
    prob = activate(logit)
    return (loss_obj.call(y, prob).reshape(B) * w.reshape(B).to(prob.dtype)).sum() / B


def ghmc_from_logits(loss_obj, logit, target, mask=None):
    """layers.GHMCLoss.calc on the device, or None when the call is outside dt_ghmc's domain (the caller then runs its torch
    body): float32 GPU logits with as many targets (and mask entries), 1 <= bins <= DT_GHMC_MAX_BINS, 0 <= momentum < 1,
    DT_AMD_DEVICE_LOSS not '0'.  `loss_obj.acc_sum` becomes ONE float32 tensor on the logits' device at the first call and is
    updated in place from then on — by every replay of a captured graph too."""
    if not (device_loss_enabled() and _on_device(logit) and logit.dtype == torch.float32 and torch.is_tensor(target)):
        return None
    n, bins, mmt = logit.numel(), int(loss_obj.bins), float(loss_obj.momentum)
    if not (1 <= n < (1 << 40) and target.numel() == n and 1 <= bins <= _lib.DT_GHMC_MAX_BINS and 0 <= mmt < 1):
        return None
    if mask is not None and not (torch.is_tensor(mask) and mask.numel() == n):
        return None
    t = target.reshape(logit.shape).to(device=logit.device, dtype=torch.float32)
    m = None if mask is None else mask.reshape(logit.shape).to(device=logit.device, dtype=torch.float32).contiguous()
    acc = None
    if mmt > 0:
        acc = loss_obj.acc_sum
        if not (acc.is_cuda and acc.device == logit.device and acc.dtype == torch.float32 and acc.is_contiguous()):
            acc = loss_obj.acc_sum = acc.detach().to(device=logit.device, dtype=torch.float32).contiguous()
    return _DeviceGhmc.apply(logit, t, m, acc, bins, mmt, torch.is_grad_enabled() and logit.requires_grad)


# the serialised form of a loss, {'class_name': ..., 'config': {...}}, as `optimizer=` takes it: Keras class name -> loss string
LOSS_CLASSES = {'BinaryCrossentropy': 'binary_crossentropy', 'CategoricalCrossentropy': 'categorical_crossentropy',
                'MeanSquaredError': 'mean_squared_error', 'MeanAbsoluteError': 'mean_absolute_error',
                'Huber': 'huber', 'LogCosh': 'log_cosh', 'MeanSquaredLogarithmicError': 'mean_squared_logarithmic_error',
                'MeanAbsolutePercentageError': 'mean_absolute_percentage_error', 'Poisson': 'poisson'}
_LOSS_REDUCTIONS = ('auto', 'sum_over_batch_size')


def resolve_loss(spec):
    """{'class_name': 'Huber', 'config': {'delta': 2.0}} -> ('huber', {'delta': 2.0}).  Accepted config keys: `delta` (Huber
    only), `name`, `reduction` in ('auto', 'sum_over_batch_size'), and `from_logits` / `label_smoothing` at their defaults —
    the steps evaluate one reduction and no smoothing, so anything else raises instead of being ignored."""
    cls = spec.get('class_name')
    if cls not in LOSS_CLASSES:
        raise ValueError(f'Unsupported loss: {cls!r} (class names: {sorted(LOSS_CLASSES)})')
    config = dict(spec.get('config') or {})
    config.pop('name', None)
    reduction = config.pop('reduction', 'auto')
    if reduction not in _LOSS_REDUCTIONS:
        raise ValueError(f'loss {cls!r}: reduction {reduction!r} is not supported (accepted: {_LOSS_REDUCTIONS})')
    if config.pop('from_logits', False) not in (False, None):
        raise ValueError(f'loss {cls!r}: from_logits=True is not supported (the model output carries the task activation)')
    if config.pop('label_smoothing', 0.0) not in (0, 0.0, None):
        raise ValueError(f'loss {cls!r}: label_smoothing is not supported')
    params = {}
    if cls == 'Huber' and 'delta' in config:
        params['delta'] = check_huber_delta(config.pop('delta'))
    if config:
        raise ValueError(f'loss {cls!r}: unknown config keys {sorted(config)} (accepted: delta (Huber), name, reduction)')
    return LOSS_CLASSES[cls], params
