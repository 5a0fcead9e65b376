# -*- coding:utf-8 -*-
"""Epoch metrics: one table of names, one row per kind, and the three functions that walk them — `compute_metric` on host
arrays, `compute_metrics_device` on device tensors (csrc/metrics.hip: the same values, computed where the outputs already
are), and `device_metrics_supported`, which says when the second serves.  `epoch_metrics` picks between them.  All of it
runs at the end of an epoch, outside any timed region."""
import ctypes
import math
import os
from collections import namedtuple
from functools import partial

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, stream_ptr
from .utils import consts

CLIP_LO = float(np.float32(1e-7))                         # Keras clips probabilities to [epsilon, 1 - epsilon] ...
CLIP_HI = float(np.float32(1) - np.float32(1e-7))         # ... with both bounds formed in float32
TOP_K = 5


def metric_name(m):
    if isinstance(m, str):
        return m
    return getattr(m, 'name', None) or getattr(m, '__name__', str(m))


# ---------------------------------------------------------------------------------------------
# host values.  The five first kinds are numpy's in the arrays' own dtype; the others are Keras 3's definitions (average
# precision: sklearn's) in float64 from the float32 values, sums exact (math.fsum), counts integers.  numpy.clip and
# numpy.maximum keep a NaN, as Keras' ops do.
# ---------------------------------------------------------------------------------------------
_quiet = np.errstate(all='ignore')


def _exact_sum(a):
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    return math.fsum(a.tolist()) if np.isfinite(a).all() else float(a.sum())      # (NaN / Inf: what numpy gives)


def label_classes(y, C):
    """the class a float label names ((int) label when 0 <= label < C), -1 where it names none (a NaN too)"""
    y = np.asarray(y, dtype=np.float32).reshape(-1)
    ok = (y >= 0) & (y.astype(np.float64) < C)
    return np.where(ok, np.where(ok, y, 0).astype(np.int64), -1)


def first_max(t):
    """per row of t [n, C]: the class a `v > best` scan from class 0 ends on (numpy.argmax when the row holds no NaN)"""
    best, idx = t[:, 0].copy(), np.zeros(t.shape[0], dtype=np.int64)
    for c in range(1, t.shape[1]):
        m = t[:, c] > best
        best, idx = np.where(m, t[:, c], best), np.where(m, c, idx)
    return idx


def confusion_counts(y, p):
    """(TP, FP, FN, TN): predicted positive is p > 0.5 (strict; a NaN is not), label positive is y != 0"""
    pp, yp = p > np.float32(0.5), y != 0
    return int((pp & yp).sum()), int((pp & ~yp).sum()), int((~pp & yp).sum()), int((~pp & ~yp).sum())


def _ratio(tp, other):                                    # precision (other = FP), recall (other = FN)
    return tp / (tp + other) if tp + other else 0.0


def _elementwise_labels(y_true, y_prob, name, expand):
    """y as float64 and p as float32, both flat: y_true as it is when it has y_prob's size, [n] labels against [n, C]
    expanded to one-hot when `expand`"""
    p = np.asarray(y_prob, dtype=np.float32)
    if y_true.size == p.size:
        return np.asarray(y_true, dtype=np.float32).astype(np.float64).reshape(-1), p.reshape(-1)
    if expand and p.ndim == 2 and p.shape[1] > 1 and y_true.size == p.shape[0]:
        y = label_classes(y_true, p.shape[1])[:, None] == np.arange(p.shape[1])[None, :]
        return y.astype(np.float64).reshape(-1), p.reshape(-1)
    raise ValueError(f'{name}: y_true {y_true.shape} does not match y_prob {p.shape}')


def _rows_and_targets(y_true, y_prob, name):
    p = np.asarray(y_prob, dtype=np.float32)
    if p.ndim != 2 or p.shape[1] < 2:
        raise ValueError(f'{name} needs y_prob [n, C] with C >= 2, got {p.shape}')
    y = np.asarray(y_true, dtype=np.float32)
    if y.shape == p.shape:
        return p, y, first_max(y)
    if y.size == p.shape[0]:
        return p, None, label_classes(y, p.shape[1])
    raise ValueError(f'{name}: y_true {y.shape} does not match y_prob {p.shape}')


@_quiet
def _flat64(y_true, y_prob, name):
    y = np.asarray(y_true, dtype=np.float32).astype(np.float64).reshape(-1)
    p = np.asarray(y_prob, dtype=np.float32).astype(np.float64).reshape(-1)
    if y.size != p.size:
        raise ValueError(f'{name}: y_true {np.shape(y_true)} does not match y_prob {np.shape(y_prob)}')
    return y, p


_host_threshold_accuracy = lambda name, y, p: ((p.reshape(-1) > 0.5).astype(np.int64) == y.reshape(-1).astype(np.int64)).mean()
_host_argmax_accuracy = lambda name, y, p: (p.argmax(-1) == (y.argmax(-1) if y.ndim == 2 else y)).mean()
_host_mse = lambda name, y, p: ((p.reshape(-1) - y.reshape(-1)) ** 2).mean()
_host_mae = lambda name, y, p: np.abs(p.reshape(-1) - y.reshape(-1)).mean()


def _host_auc(name, y_true, y_prob):
    from sklearn.metrics import roc_auc_score
    try:
        if y_prob.ndim == 2 and y_prob.shape[1] > 1:
            return roc_auc_score(y_true, y_prob, multi_class='ovr')
        return roc_auc_score(y_true.reshape(-1), y_prob.reshape(-1))
    except ValueError:
        return float('nan')


@_quiet
def _host_bce(name, y_true, y_prob):
    y, p = _elementwise_labels(y_true, y_prob, name, expand=False)
    q = np.clip(p.astype(np.float64), CLIP_LO, CLIP_HI)
    return _exact_sum(-(y * np.log(q) + (1.0 - y) * np.log(1.0 - q))) / p.size


@_quiet
def _host_tp_ratio(other, name, y_true, y_prob):       # other: 1 = FP (precision), 2 = FN (recall)
    counts = confusion_counts(*_elementwise_labels(y_true, y_prob, name, expand=True))
    return _ratio(counts[0], counts[other])


@_quiet
def _host_topk(name, y_true, y_prob):
    p32, _, target = _rows_and_targets(y_true, y_prob, name)
    n = p32.shape[0]
    pt = p32[np.arange(n), np.maximum(target, 0)]
    above = (p32 > pt[:, None]).sum(1)
    return int(((target >= 0) & (pt == pt) & (above < TOP_K)).sum()) / n


@_quiet
def _host_cce(name, y_true, y_prob):
    p32, onehot, target = _rows_and_targets(y_true, y_prob, name)
    n, C = p32.shape
    p = p32.astype(np.float64)
    s = np.zeros(n)
    for c in range(C):                                  # (class order)
        s += p[:, c]
    q = np.clip(p / s[:, None], CLIP_LO, CLIP_HI)
    if onehot is None:
        loss = np.where(target >= 0, -np.log(q[np.arange(n), np.maximum(target, 0)]), np.nan)
    else:
        acc = np.zeros(n)
        for c in range(C):
            acc += onehot[:, c].astype(np.float64) * np.log(q[:, c])
        loss = -acc
    return _exact_sum(loss) / n


@_quiet
def _host_msle(name, y_true, y_prob):
    y, p = _flat64(y_true, y_prob, name)
    d = np.log(np.maximum(p, CLIP_LO) + 1.0) - np.log(np.maximum(y, CLIP_LO) + 1.0)
    return _exact_sum(d * d) / p.size


@_quiet
def _host_mape(name, y_true, y_prob):
    y, p = _flat64(y_true, y_prob, name)
    return 100.0 * (_exact_sum(np.abs(y - p) / np.maximum(np.abs(y), CLIP_LO)) / p.size)


def _host_ap(name, y_true, y_prob):
    y, p = _flat64(y_true, y_prob, name)
    from sklearn.metrics import average_precision_score
    if np.ndim(y_prob) == 2 and np.shape(y_prob)[1] > 1:
        raise ValueError(f'{name} takes binary scores, got y_prob {np.shape(y_prob)}')
    if not (y == 1).any():
        return float('nan')
    try:
        return average_precision_score(y, p)
    except ValueError:
        return float('nan')


# the launches of csrc/metrics.hip and the 8-byte words each writes into the result buffer, in the buffer's order.  'ranking'
# is dt_score_ranking, or dt_metric_auc when no average precision is asked for: the latter's five words are the former's
# first five, so either way they are where the AUC reads them.
_PASS_WORDS = (('ranking', _lib.DT_SCORE_RANKING_WORDS), ('sums', _lib.DT_METRIC_SUMS_WORDS), ('argmax', 1),
               ('binary', _lib.DT_SCORE_BINARY_WORDS), ('rows', _lib.DT_SCORE_CATEGORICAL_WORDS),
               ('regression', _lib.DT_SCORE_REGRESSION_WORDS))
_AT, _OUT_WORDS = {}, 0                                   # pass -> its first word; the buffer's size
for _p, _w in _PASS_WORDS:
    _AT[_p], _OUT_WORDS = _OUT_WORDS, _OUT_WORDS + _w

# One row per kind.  shape: what the device path needs of the two tensors (device_metrics_supported); launch: the pass that
# writes its words; value(i, f, n, rows): the metric from that pass's first words read as integers (i) and as float64 (f),
# n = y_prob.numel(), rows = y_prob.shape[0]; host(name, y_true, y_prob): the metric from host arrays.
# The ranking words: U2, P, N, non-finite scores, labels other than 0 / 1, the sum of the groups' precisions.
Kind = namedtuple('Kind', 'shape launch value host')
_nan = float('nan')
KINDS = {
    'auc': Kind('flat column', 'ranking',
                lambda i, f, n, rows: _nan if i[1] == 0 or i[2] == 0 or i[3] > 0 else i[0] / (2 * i[1] * i[2]), _host_auc),
    'ap': Kind('flat column', 'ranking', lambda i, f, n, rows: _nan if i[1] == 0 or i[3] > 0 else f[5] / i[1], _host_ap),
    'accuracy': Kind('flat', 'sums', lambda i, f, n, rows: i[0] / n, _host_threshold_accuracy),
    'argmax_accuracy': Kind('rows', 'argmax', lambda i, f, n, rows: i[0] / rows, _host_argmax_accuracy),
    'mse': Kind('flat', 'sums', lambda i, f, n, rows: f[1] / n, _host_mse),
    'rmse': Kind('flat', 'sums', lambda i, f, n, rows: math.sqrt(f[1] / n), lambda *a: np.sqrt(_host_mse(*a))),
    'mae': Kind('flat', 'sums', lambda i, f, n, rows: f[2] / n, _host_mae),
    'bce': Kind('flat', 'binary', lambda i, f, n, rows: f[4] / n, _host_bce),
    'precision': Kind('flat or labels', 'binary', lambda i, f, n, rows: _ratio(i[0], i[1]), partial(_host_tp_ratio, 1)),
    'recall': Kind('flat or labels', 'binary', lambda i, f, n, rows: _ratio(i[0], i[2]), partial(_host_tp_ratio, 2)),
    'topk': Kind('rows', 'rows', lambda i, f, n, rows: i[0] / rows, _host_topk),
    'cce': Kind('rows', 'rows', lambda i, f, n, rows: f[1] / rows, _host_cce),
    'msle': Kind('flat', 'regression', lambda i, f, n, rows: f[0] / n, _host_msle),
    'mape': Kind('flat', 'regression', lambda i, f, n, rows: 100.0 * (f[1] / n), _host_mape),
}
# lower-case name -> kind; _kind resolves 'logloss' by the task and 'accuracy' by the task and the outputs' shape
NAMES = {name: kind for kind, names in {
    'auc': 'auc', 'accuracy': 'accuracy acc', 'mse': 'mse mean_squared_error',
    'rmse': 'rmse rootmeansquarederror root_mean_squared_error', 'mae': 'mae mean_absolute_error',
    'logloss': 'logloss log_loss', 'bce': 'binary_crossentropy binarycrossentropy',
    'cce': 'categorical_crossentropy categoricalcrossentropy', 'precision': 'precision', 'recall': 'recall',
    'topk': 'top_k_categorical_accuracy topkcategoricalaccuracy',
    'msle': 'msle mean_squared_logarithmic_error meansquaredlogarithmicerror',
    'mape': 'mape mean_absolute_percentage_error meanabsolutepercentageerror', 'ap': 'average_precision pr_auc',
}.items() for name in names.split()}


def _kind(key, task, shape=()):
    """the key of KINDS for a lower-case metric name and outputs of `shape`, None for a name NAMES does not hold"""
    kind = NAMES.get(key)
    if kind == 'logloss':
        return 'cce' if task == consts.TASK_MULTICLASS else 'bce'
    if kind == 'accuracy' and task == consts.TASK_MULTICLASS and len(shape) == 2 and shape[1] > 1:
        return 'argmax_accuracy'
    return kind


def score_kind(key, task):
    """'bce' / 'cce' / 'precision' / 'recall' / 'topk' / 'msle' / 'mape' / 'ap' for a lower-case metric name, else None"""
    kind = _kind(key, task)
    return None if kind in ('auc', 'accuracy', 'mse', 'rmse', 'mae') else kind


def compute_metric(m, y_true, y_prob, task):
    name = metric_name(m)
    y_true, y_prob = np.asarray(y_true), np.asarray(y_prob)
    if callable(m) and not isinstance(m, str):
        return float(m(y_true, y_prob))
    kind = _kind(name.lower(), task, y_prob.shape)
    if kind is None:
        raise ValueError(f'Unsupported metric: {name}')
    return float(KINDS[kind].host(name, y_true, y_prob))


_metric_buffers = {}        # device -> {'ws': uint8 workspace (grown on demand), 'out': int64 result words}


def device_metrics_supported(metrics, y_true, y_prob, task):
    """True when compute_metrics_device serves every one of `metrics`: float32 tensors on the GPU, metric names it knows
    (by name only, a callable is the host's), shapes the kernels cover, and DT_AMD_DEVICE_METRICS not '0'."""
    if os.environ.get('DT_AMD_DEVICE_METRICS', '1') == '0' or not metrics:
        return False
    if not (torch.is_tensor(y_true) and torch.is_tensor(y_prob) and y_true.is_cuda and y_prob.is_cuda and
            y_true.dtype == torch.float32 and y_prob.dtype == torch.float32 and y_prob.numel() > 0):
        return False
    flat = y_true.numel() == y_prob.numel()
    wide = y_prob.dim() == 2 and y_prob.shape[1] > 1      # (multiclass one-vs-rest AUC: the host's)
    labels = wide and y_true.numel() == y_prob.shape[0]
    holds = {'flat': flat, 'flat column': flat and not wide, 'flat or labels': flat or labels,
             'rows': labels or (wide and y_true.dim() == 2 and y_true.shape == y_prob.shape)}
    for m in metrics:
        kind = _kind(m.lower(), task, y_prob.shape) if isinstance(m, str) else None
        if kind is None or not holds[KINDS[kind].shape]:
            return False
    return True


def compute_metrics_device(metrics, y_true, y_prob, task):
    """{name: value} for metrics that device_metrics_supported accepts, from device tensors: at most one radix sort (AUC,
    average precision), one reduction (accuracy / mse / rmse / mae), one element-wise pass (log loss, precision, recall), one
    row pass (categorical cross-entropy, top-k accuracy) and one regression pass (msle, mape) whatever the number of metrics,
    and one small device-to-host read.  The values are compute_metric's: AUC is the exact ROC AUC U2 / (2 P N) in integers
    and average precision the groups' sum / P (both nan where sklearn raises or has no positive: one class only, a NaN / Inf
    score); labels other than 0 / 1 send both to compute_metric on the host."""
    if not device_metrics_supported(metrics, y_true, y_prob, task):
        raise ValueError(f'compute_metrics_device does not cover {[metric_name(m) for m in metrics]} for these outputs')
    h = lib()
    y_true, y_prob = y_true.detach().contiguous(), y_prob.detach().contiguous()
    n = y_prob.numel()
    rows = y_prob.shape[0] if y_prob.dim() == 2 else n
    kinds = [_kind(m.lower(), task, y_prob.shape) for m in metrics]
    passes = {KINDS[kind].launch for kind in kinds}
    buf = _metric_buffers.setdefault(y_prob.device, {})
    if 'out' not in buf:
        buf['out'] = torch.zeros(_OUT_WORDS, dtype=torch.int64, device=y_prob.device)
    out = buf['out']
    word = lambda launch: ctypes.c_void_p(out.data_ptr() + 8 * _AT[launch])
    labels_kind = _lib.DT_METRIC_Y_ONEHOT if y_true.dim() == 2 and y_true.shape == y_prob.shape else _lib.DT_METRIC_Y_LABELS
    with torch.cuda.device(y_prob.device):
        if 'ranking' in passes:                                     # one sort serves both
            entry = 'dt_score_ranking' if 'ap' in kinds else 'dt_metric_auc'
            need = getattr(h, entry + '_workspace_bytes')(n)
            if need < 0:
                check(int(need), 'dt_metric_auc_workspace_bytes')
            if buf.get('ws') is None or buf['ws'].numel() < need:
                buf['ws'] = None                                    # (release before the larger one is allocated)
                buf['ws'] = torch.empty(int(need), dtype=torch.uint8, device=y_prob.device)
            check(getattr(h, entry)(ptr(y_prob), ptr(y_true), n, ptr(buf['ws']), word('ranking'), stream_ptr()), entry)
        if 'sums' in passes:
            check(h.dt_metric_sums(ptr(y_true), ptr(y_prob), n, word('sums'), stream_ptr()), 'dt_metric_sums')
        if 'argmax' in passes:
            check(h.dt_metric_argmax_hits(ptr(y_prob), ptr(y_true), labels_kind, rows, y_prob.shape[1], word('argmax'),
                                          stream_ptr()), 'dt_metric_argmax_hits')
        if 'binary' in passes:                                      # element against element, whatever the two shapes
            args = (_lib.DT_METRIC_Y_ONEHOT, n, 1) if y_true.numel() == n else (_lib.DT_METRIC_Y_LABELS, rows, y_prob.shape[1])
            check(h.dt_score_binary(ptr(y_true), ptr(y_prob), *args, word('binary'), stream_ptr()), 'dt_score_binary')
        if 'rows' in passes:
            check(h.dt_score_categorical(ptr(y_prob), ptr(y_true), labels_kind, rows, y_prob.shape[1], TOP_K, word('rows'),
                                         stream_ptr()), 'dt_score_categorical')
        if 'regression' in passes:
            check(h.dt_score_regression(ptr(y_true), ptr(y_prob), n, word('regression'), stream_ptr()), 'dt_score_regression')
        host = out.cpu()                                            # the one read: 27 KB
    res = {}
    for m, kind in zip(metrics, kinds):
        row = KINDS[kind]
        words = host[_AT[row.launch]:_AT[row.launch] + 6]           # (no pass has more result words)
        i, f = words.tolist(), words.view(torch.float64).tolist()
        if row.launch == 'ranking' and i[4] > 0:                    # labels other than 0 / 1
            v = compute_metric(m, y_true.cpu().numpy(), y_prob.cpu().numpy(), task)
        else:
            v = row.value(i, f, n, rows)
        res[metric_name(m)] = float(v)
    return res


def epoch_metrics(metrics, y_true, y_prob, task):
    """{name: value} for an epoch's concatenated labels and outputs (tensors): on the device when
    device_metrics_supported, else exactly the host path — copy both to the host and compute_metric each."""
    if not metrics:
        return {}
    if device_metrics_supported(metrics, y_true, y_prob, task):
        return compute_metrics_device(metrics, y_true, y_prob, task)
    yt, yp = y_true.cpu().numpy(), y_prob.cpu().numpy()
    return {metric_name(m): compute_metric(m, yt, yp, task) for m in metrics}
