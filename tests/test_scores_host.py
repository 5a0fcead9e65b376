# -*- coding:utf-8 -*-
"""CPU: the reference of the dt_score_* kernels (tests/scores_reference.py) against sklearn where the definitions coincide
and against brute force where they do not; metrics.compute_metric / epoch_metrics for the new metric names; their routing;
and the C-ABI surface and argument checks of the dt_score_* entry points (no launch)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import scores_reference as S
from tests.test_metrics_host import _FakeCuda

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {'dt_score_binary', 'dt_score_regression', 'dt_score_categorical', 'dt_score_ranking_workspace_bytes',
           'dt_score_ranking'}
ALIASES = {
    'bce': ['binary_crossentropy', 'binarycrossentropy', 'logloss', 'log_loss'],
    'cce': ['categorical_crossentropy', 'categoricalcrossentropy', 'logloss', 'log_loss'],
    'precision': ['precision'], 'recall': ['recall'],
    'topk': ['top_k_categorical_accuracy', 'topkcategoricalaccuracy'],
    'msle': ['msle', 'mean_squared_logarithmic_error', 'meansquaredlogarithmicerror'],
    'mape': ['mape', 'mean_absolute_percentage_error', 'meanabsolutepercentageerror'],
    'ap': ['average_precision', 'pr_auc'],
}


def _rel(got, want):
    return abs(got - want) / abs(want)


def _binary(n, seed, lo=1e-6):
    rng = np.random.default_rng(seed)
    y = (rng.random(n) < 0.3).astype(np.float32)
    p = np.clip(rng.random(n), lo, 1 - lo).astype(np.float32)
    p = np.clip(p, np.float32(lo), np.float32(1 - lo))                 # (the float32 rounding may step outside)
    p[::7] = np.float32(0.5)                                           # on the threshold: not a predicted positive
    return y, p


def _multiclass(n, C, seed, decimals=None):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n, C))
    p = np.exp(z) / np.exp(z).sum(1, keepdims=True)
    if decimals is not None:
        p = np.round(p, decimals)
    labels = rng.integers(0, C, n)
    return p.astype(np.float32), labels.astype(np.float32), np.eye(C, dtype=np.float32)[labels]


# ---- the reference against sklearn -----------------------------------------------------------------------------------------
def test_constants_are_keras_float32_epsilons():
    assert S.LO == float(np.float32(1e-7)) and abs(S.HI - 0.99999988079) < 1e-11 and S.HI == float(np.float32(0.9999999))
    assert math.isnan(float(S.clip(np.nan))) and float(S.clip(np.inf)) == S.HI and float(S.clip(-np.inf)) == S.LO


@pytest.mark.parametrize('n,seed', [(1, 0), (50, 1), (4097, 2)])
def test_precision_and_recall_equal_sklearn(n, seed):
    from sklearn.metrics import precision_score, recall_score
    y, p = _binary(n, seed)
    tp, fp, fn, tn, _ = S.binary_words(y, p)
    assert tp + fp + fn + tn == n
    pred = (p > 0.5).astype(np.int64)
    assert S.ratio(tp, tp + fp) == precision_score(y.astype(np.int64), pred, zero_division=0)
    assert S.ratio(tp, tp + fn) == recall_score(y.astype(np.int64), pred, zero_division=0)
    # all-negative labels, and nothing predicted positive: 0.0 both, as zero_division=0
    assert S.binary_words(np.zeros(n, np.float32), p)[0] == 0 and S.ratio(0, 0) == 0.0
    tp0, fp0, _, _, _ = S.binary_words(y, np.zeros(n, np.float32))
    assert (tp0, fp0) == (0, 0)


def test_multiclass_precision_counts_equal_sklearn_micro_average():
    from sklearn.metrics import precision_score, recall_score
    p, labels, onehot = _multiclass(500, 4, 3)
    words = S.binary_words(labels, p)
    assert words == S.binary_words(onehot, p)                  # labels expanded on the fly = one-hot
    pred = (p > 0.5).astype(np.int64)
    assert S.ratio(words[0], words[0] + words[1]) == precision_score(onehot.astype(np.int64), pred, average='micro', zero_division=0)
    assert S.ratio(words[0], words[0] + words[2]) == recall_score(onehot.astype(np.int64), pred, average='micro', zero_division=0)


@pytest.mark.parametrize('pattern', ['ties', 'million'])
def test_average_precision_equals_sklearn(pattern):
    from sklearn.metrics import average_precision_score
    rng = np.random.default_rng(11)
    if pattern == 'ties':
        n = 5000
        label = (rng.random(n) < 0.4).astype(np.float32)
        score = (rng.integers(0, 8, n) / 8).astype(np.float32)
    else:
        n = 1 << 20
        label = (rng.random(n) < 0.03).astype(np.float32)
        score = (1 / (1 + np.exp(-(rng.standard_normal(n) + 0.8 * label - 2)))).astype(np.float32)
    got, want = S.average_precision(score, label), float(average_precision_score(label, score))
    print('reference - average_precision_score =', got - want)
    assert abs(got - want) <= 1e-12
    assert S.ranking_words(score, label)[:5] == S.R.auc_words_fast(score, label)


def test_average_precision_edges():
    s = np.array([0.1, 0.4, 0.4, 0.9], dtype=np.float32)
    assert S.average_precision(s, np.ones(4, np.float32)) == 1.0               # N = 0: the formula gives 1
    assert math.isnan(S.average_precision(s, np.zeros(4, np.float32)))         # P = 0
    for bad in (np.nan, np.inf, -np.inf):
        assert math.isnan(S.average_precision(np.array([0.1, bad, 0.4, 0.9], dtype=np.float32), np.array([0, 1, 0, 1], np.float32)))
    # one group holding everything: AP = P / n
    assert S.average_precision(np.full(4, 0.5, np.float32), np.array([0, 1, 0, 1], np.float32)) == 0.5


def test_log_loss_equals_sklearn():
    from sklearn.metrics import log_loss
    y, p = _binary(3000, 4)
    got = S.binary_words(y, p)[4] / y.size
    want = log_loss(y.astype(np.int64), p.astype(np.float64))
    print('binary: rel', _rel(got, want))
    assert _rel(got, want) <= 1e-12
    # multiclass: rows in [1e-6, 1 - 1e-6] that sum to one in float32 up to rounding; sklearn renormalises too
    pm, labels, onehot = _multiclass(2000, 5, 5)
    pm = np.clip(pm, np.float32(1e-6), np.float32(1 - 1e-6))
    want = log_loss(labels.astype(np.int64), pm.astype(np.float64) / pm.astype(np.float64).sum(1, keepdims=True),
                    labels=list(range(5)))
    for yt in (labels, onehot):
        got = S.categorical_words(pm, yt, 5, 32)[1] / pm.shape[0]
        print('multiclass: rel', _rel(got, want))
        assert _rel(got, want) <= 1e-12


def test_msle_and_mape_equal_sklearn():
    from sklearn.metrics import mean_absolute_percentage_error, mean_squared_log_error
    rng = np.random.default_rng(6)
    y = (0.01 + np.exp(rng.standard_normal(4000))).astype(np.float32)
    p = (0.01 + np.exp(rng.standard_normal(4000))).astype(np.float32)
    sl, pe, _ = S.regression_sums(y, p)
    y64, p64 = y.astype(np.float64), p.astype(np.float64)
    assert _rel(sl / 4000, mean_squared_log_error(y64, p64)) <= 1e-12
    assert _rel(100 * pe / 4000, 100 * mean_absolute_percentage_error(y64, p64)) <= 1e-12


def test_top_k_equals_sklearn_without_ties_and_brute_force_with():
    from sklearn.metrics import top_k_accuracy_score
    p, labels, onehot = _multiclass(800, 9, 7)
    assert all(len(set(r)) == 9 for r in p.tolist())           # no ties
    want = top_k_accuracy_score(labels.astype(np.int64), p, k=5, labels=list(range(9)), normalize=False)
    assert S.categorical_words(p, labels, 5, 32)[0] == want == S.categorical_words(p, onehot, 5, 32)[0]
    # ties across the boundary are all in; C <= k: every row whose target score is not a NaN hits
    for C, decimals in ((9, 1), (12, 1), (5, 1), (3, 2), (70, 2)):
        q, lab, oh = _multiclass(400, C, 8 + C, decimals)
        q[3, int(lab[3])] = np.nan                              # a NaN at the target misses
        q[5, (int(lab[5]) + 1) % C] = np.nan                    # elsewhere it is just not above
        want = S.top_k_brute_force(q, lab.astype(np.int64), 5)
        assert S.categorical_words(q, lab, 5, 32)[0] == want == S.categorical_words(q, oh, 5, 32)[0], C
        if C <= 5:
            assert want == 399
    tied = np.array([[.2, .2, .2, .2, .2, .2, .1]], dtype=np.float32)          # six classes tied for first: all in
    assert S.categorical_words(tied, np.array([5], np.float32), 5, 32)[0] == 1
    assert S.categorical_words(tied, np.array([6], np.float32), 5, 32)[0] == 0


def test_first_max_and_label_classes():
    t = np.array([[0, 0, 0], [0, 1, 1], [np.nan, 5, 1], [1, np.nan, 7], [-0.0, 0.0, -1]], dtype=np.float32)
    assert S.first_max(t).tolist() == [0, 1, 0, 2, 0] == S.first_max_fast(t).tolist()
    rng = np.random.default_rng(1)
    r = np.round(rng.random((200, 6)), 1).astype(np.float32)
    assert S.first_max(r).tolist() == r.argmax(1).tolist() == S.first_max_fast(r).tolist()
    assert S.label_classes(np.array([0, 2, 2.7, 3, -1, np.nan, np.inf, -0.0], np.float32), 3).tolist() == [0, 2, 2, -1, -1, -1, -1, 0]


def test_row_sum_orders():
    rng = np.random.default_rng(2)
    x = rng.random((5, 200)) * 10.0 ** rng.integers(-8, 8, (5, 200))
    seq = np.array([sum(row[1:], row[0]) for row in x.tolist()])
    assert np.array_equal(S.row_sum(x, 200), seq)
    wave = S.row_sum(x, 32)
    assert np.allclose(wave, seq, rtol=1e-13) and not np.array_equal(wave, seq)        # another order: other roundings
    assert np.array_equal(S.row_sum(x[:, :32], 32), seq * 0 + np.array([sum(r[1:32], r[0]) for r in x.tolist()]))


# ---- compute_metric / epoch_metrics ----------------------------------------------------------------------------------------
def _cases():
    y, p = _binary(400, 20)
    pm, labels, onehot = _multiclass(300, 7, 21, 2)
    rng = np.random.default_rng(22)
    yr = np.exp(rng.standard_normal(300)).astype(np.float32)
    pr = np.exp(rng.standard_normal((300, 1))).astype(np.float32)
    ml_y, ml_p = (rng.random((200, 3)) < 0.4).astype(np.float32), rng.random((200, 3)).astype(np.float32)
    return {'binary': (y, p.reshape(-1, 1), 'binary'), 'labels': (labels, pm, 'multiclass'), 'onehot': (onehot, pm, 'multiclass'),
            'regression': (yr, pr, 'regression'), 'multilabel': (ml_y, ml_p, 'multilabel')}


def _reference_value(kind, y, p):
    n = p.shape[0]
    if kind == 'bce':
        return S.binary_words(y, p)[4] / p.size
    if kind in ('precision', 'recall'):
        tp, fp, fn, _, _ = S.binary_words(y, p)
        return S.ratio(tp, tp + (fp if kind == 'precision' else fn))
    if kind == 'cce':
        return S.categorical_words(p, y, 5, 10 ** 9)[1] / n           # (the host path adds in class order at every width)
    if kind == 'topk':
        return S.categorical_words(p, y, 5, 32)[0] / n
    if kind == 'msle':
        return S.regression_sums(y, p)[0] / n
    if kind == 'mape':
        return 100 * S.regression_sums(y, p)[1] / n
    return S.average_precision(p, y)


@pytest.mark.parametrize('case,kinds', [('binary', ['bce', 'precision', 'recall', 'ap', 'msle', 'mape']),
                                        ('multilabel', ['bce', 'precision', 'recall']),
                                        ('labels', ['cce', 'topk', 'precision', 'recall']),
                                        ('onehot', ['cce', 'topk', 'precision', 'recall', 'bce']),
                                        ('regression', ['msle', 'mape'])])
def test_compute_metric_serves_every_name_in_any_case(case, kinds):
    from deeptables_amd import metrics
    y, p, task = _cases()[case]
    for kind in kinds:
        want = _reference_value(kind, y, p)
        for alias in ALIASES[kind]:
            if alias in ('logloss', 'log_loss') and (kind == 'cce') != (task == 'multiclass'):
                continue
            for name in (alias, alias.upper(), alias.title()):
                got = metrics.compute_metric(name, y, p, task)
                assert isinstance(got, float)
                assert got == want or abs(got - want) <= 1e-13 * abs(want), (name, got, want)
                assert metrics.epoch_metrics([name], torch.from_numpy(y), torch.from_numpy(p), task) == {name: got}
    with pytest.raises(ValueError, match='Unsupported metric'):
        metrics.compute_metric('f1', y, p, task)
    with pytest.raises(ValueError, match='Unsupported metric'):
        metrics.compute_metric('r2', y, p, task)


def test_compute_metric_special_values():
    from deeptables_amd import metrics
    y, p, _ = _cases()['binary']
    n = y.shape[0]
    assert math.isnan(metrics.compute_metric('average_precision', np.zeros(n, np.float32), p, 'binary'))
    assert metrics.compute_metric('average_precision', np.ones(n, np.float32), p, 'binary') == 1.0
    bad = p.copy()
    bad[3] = np.nan
    assert math.isnan(metrics.compute_metric('pr_auc', y, bad, 'binary'))
    assert math.isnan(metrics.compute_metric('binary_crossentropy', y, bad, 'binary'))        # the clip keeps the NaN
    bad[3] = np.inf
    assert math.isfinite(metrics.compute_metric('binary_crossentropy', y, bad, 'binary'))     # ... and clips an Inf
    assert metrics.compute_metric('precision', np.zeros(n, np.float32), p, 'binary') == 0.0
    assert metrics.compute_metric('recall', np.zeros(n, np.float32), p, 'binary') == 0.0
    assert metrics.compute_metric('precision', y, np.zeros_like(p), 'binary') == 0.0
    y2 = y.copy()
    y2[y2 == 1] = 0.5                                          # precision counts any y != 0 as positive
    assert metrics.compute_metric('precision', y2, p, 'binary') == metrics.compute_metric('precision', y, p, 'binary')
    with pytest.raises(ValueError):
        metrics.compute_metric('average_precision', *_cases()['onehot'][:2], 'multiclass')
    with pytest.raises(ValueError):
        metrics.compute_metric('categorical_crossentropy', y, p, 'binary')                    # one column


# ---- routing ---------------------------------------------------------------------------------------------------------------
def test_routing_accepts_the_new_names_where_the_kernels_cover_them(monkeypatch):
    from deeptables_amd import metrics
    monkeypatch.setattr(torch, 'is_tensor', lambda t: isinstance(t, (torch.Tensor, _FakeCuda)))
    monkeypatch.delenv('DT_AMD_DEVICE_METRICS', raising=False)
    ok = metrics.device_metrics_supported
    y, p = _FakeCuda(torch.tensor([0., 1, 1, 0])), _FakeCuda(torch.tensor([[.2], [.7], [.6], [.4]]))
    assert ok(['AUC', 'average_precision', 'binary_crossentropy', 'Precision', 'Recall', 'accuracy', 'LogLoss', 'pr_auc'], y, p, 'binary')
    assert ok(['mse', 'msle', 'MAPE', 'mean_squared_logarithmic_error'], y, p, 'regression')
    pm = _FakeCuda(torch.tensor([[.2, .5, .3], [.7, .2, .1], [.1, .1, .8], [.3, .4, .3]]))
    onehot, labels = _FakeCuda(torch.eye(3)[[1, 0, 2, 1]]), _FakeCuda(torch.tensor([1., 0, 2, 1]))
    names = ['accuracy', 'categorical_crossentropy', 'top_k_categorical_accuracy', 'precision', 'recall', 'logloss']
    assert ok(names, onehot, pm, 'multiclass') and ok(names, labels, pm, 'multiclass')
    assert ok(['binary_crossentropy', 'precision', 'recall'], onehot, pm, 'multilabel')
    # refused: shapes the kernels do not cover, other dtypes, ranking metrics on [n, C], unknown names, callables
    assert not ok(['binary_crossentropy'], labels, pm, 'multiclass')                  # sizes differ
    assert not ok(['msle'], labels, pm, 'regression') and not ok(['mape'], labels, pm, 'regression')
    assert not ok(['categorical_crossentropy'], y, p, 'binary') and not ok(['top_k_categorical_accuracy'], y, p, 'binary')
    three = _FakeCuda(torch.tensor([1., 0, 2]))
    assert not ok(['categorical_crossentropy'], three, pm, 'multiclass') and not ok(['precision'], three, pm, 'multiclass')
    assert not ok(['average_precision'], onehot, pm, 'multiclass') and not ok(['pr_auc'], labels, pm, 'multiclass')
    yd = _FakeCuda(torch.tensor([0., 1, 1, 0]).double())
    for name in ('binary_crossentropy', 'precision', 'msle', 'average_precision'):
        assert not ok([name], yd, p, 'binary') and not ok([name], y, _FakeCuda(p.t.double()), 'binary')
    assert not ok(['precision', 'f1'], y, p, 'binary')
    assert not ok(['precision', lambda a, b: 1.0], y, p, 'binary')
    assert not ok(['precision'], torch.tensor([0., 1, 1, 0]), torch.tensor([[.2], [.7], [.6], [.4]]), 'binary')     # CPU tensors
    monkeypatch.setenv('DT_AMD_DEVICE_METRICS', '0')
    assert not ok(['precision'], y, p, 'binary')


def test_every_name_reaches_the_same_table_row_on_the_host_and_the_device_path(monkeypatch):
    """compute_metric and device_metrics_supported look a name up in metrics.KINDS: for every name of metrics.NAMES in
    lower, upper and mixed case and every task, on one column and on [n, C], both take the same row; a name the table does not
    hold is refused by both"""
    from deeptables_amd import metrics
    monkeypatch.setattr(torch, 'is_tensor', lambda t: isinstance(t, (torch.Tensor, _FakeCuda)))
    monkeypatch.delenv('DT_AMD_DEVICE_METRICS', raising=False)
    seen = []

    class Spy(dict):
        def __getitem__(self, kind):
            seen.append(kind)
            return dict.__getitem__(self, kind)._replace(host=lambda name, y_true, y_prob: 0.5)

    monkeypatch.setattr(metrics, 'KINDS', Spy(metrics.KINDS))
    y = torch.tensor([0., 1, 1, 0])
    column, wide = torch.tensor([[.2], [.7], [.6], [.4]]), torch.tensor([[.2, .5, .3], [.7, .2, .1], [.1, .1, .8], [.3, .4, .3]])
    assert len(metrics.NAMES) == 28 and set(metrics.NAMES.values()) - {'logloss'} <= set(metrics.KINDS)
    rows = set()
    for key in metrics.NAMES:
        for name in (key, key.upper(), key.title()):
            for task in ('binary', 'multiclass', 'regression'):
                for p in (column, wide):
                    del seen[:]
                    assert metrics.compute_metric(name, y.numpy(), p.numpy(), task) == 0.5
                    host_row = list(seen)
                    del seen[:]
                    metrics.device_metrics_supported([name], _FakeCuda(y), _FakeCuda(p), task)
                    assert len(host_row) == 1 and seen == host_row and host_row[0] in metrics.KINDS, (name, task, host_row, seen)
                    rows.add(host_row[0])
    assert rows == set(metrics.KINDS)                              # (every row is some name's)
    for name in ('f1', 'r2', 'logloss_', 'argmax_accuracy', ''):
        for task in ('binary', 'multiclass', 'regression'):
            del seen[:]
            with pytest.raises(ValueError, match='Unsupported metric'):
                metrics.compute_metric(name, y.numpy(), column.numpy(), task)
            assert metrics.device_metrics_supported([name], _FakeCuda(y), _FakeCuda(column), task) is False and seen == []


# ---- the C-ABI surface -----------------------------------------------------------------------------------------------------
def test_header_exports_and_binding_name_the_same_score_entry_points():
    from deeptables_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'dt_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(dt_score_[a-z0-9_]+)\s*\(', text))
    assert declared == ENTRIES == {n for n in _lib.SIGNATURES if n.startswith('dt_score_')}
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for n in ENTRIES:
        assert hasattr(handle, n), n
    B = _lib.DT_SCORE_BLOCKS
    assert (_lib.DT_SCORE_BINARY_WORDS, _lib.DT_SCORE_REGRESSION_WORDS, _lib.DT_SCORE_CATEGORICAL_WORDS,
            _lib.DT_SCORE_RANKING_WORDS) == (5 + 5 * B, 2 + 2 * B, 2 + 2 * B, 6 + B)
    defs = dict(re.findall(r'^#define (DT_SCORE_[A-Z_]+) (\d+)\s*$', open(os.path.join(ROOT, 'include', 'dt_hip.h')).read(), re.M))
    assert len(defs) == 6 and all(getattr(_lib, k) == int(v) for k, v in defs.items())


def test_score_entry_points_refuse_bad_arguments_before_any_launch():
    from deeptables_amd import _lib
    h = _lib.lib()
    A, ODD = 0x10000, 0x10002            # never dereferenced: every call below is refused, or is the n == 0 no-op
    big = 1 << 31
    EL, LB = _lib.DT_METRIC_Y_ONEHOT, _lib.DT_METRIC_Y_LABELS

    def refused(rc, *words):
        assert rc == -1
        msg = h.dt_last_error().decode()
        assert all(w in msg for w in words), msg

    # the element-wise pass
    name = 'dt_score_binary'
    refused(h.dt_score_binary(A, A, EL, -1, 1, A, None), name, '2^31')
    refused(h.dt_score_binary(A, A, EL, big, 1, A, None), name, '2^31')
    refused(h.dt_score_binary(A, A, EL, 5, 0, A, None), name, 'C = 0')
    refused(h.dt_score_binary(A, A, LB, 5, 1, A, None), name, 'C = 1')
    refused(h.dt_score_binary(A, A, 7, 5, 3, A, None), name, 'y_kind')
    refused(h.dt_score_binary(A, A, EL, 1 << 30, 2, A, None), name, 'overflows')
    refused(h.dt_score_binary(A, A, EL, (1 << 31) - 1, (1 << 31) - 1, A, None), name, 'overflows')
    refused(h.dt_score_binary(None, A, EL, 5, 1, A, None), name, 'null pointer')
    refused(h.dt_score_binary(A, None, EL, 5, 1, A, None), name, 'null pointer')
    refused(h.dt_score_binary(A, A, EL, 5, 1, None, None), name, 'null pointer')
    refused(h.dt_score_binary(ODD, A, EL, 5, 1, A, None), name, 'aligned')
    refused(h.dt_score_binary(A, ODD, LB, 5, 3, A, None), name, 'aligned')
    refused(h.dt_score_binary(A, A, EL, 5, 1, A + 4, None), name, 'out', 'aligned')
    assert h.dt_score_binary(None, None, EL, 0, 1, None, None) == 0
    assert h.dt_score_binary(None, None, LB, 0, 3, None, None) == 0
    # the regression pass
    name = 'dt_score_regression'
    refused(h.dt_score_regression(A, A, -1, A, None), name, '2^31')
    refused(h.dt_score_regression(A, A, big, A, None), name, '2^31')
    refused(h.dt_score_regression(None, A, 5, A, None), name, 'null pointer')
    refused(h.dt_score_regression(A, None, 5, A, None), name, 'null pointer')
    refused(h.dt_score_regression(A, A, 5, None, None), name, 'null pointer')
    refused(h.dt_score_regression(ODD, A, 5, A, None), name, 'aligned')
    refused(h.dt_score_regression(A, ODD, 5, A, None), name, 'aligned')
    refused(h.dt_score_regression(A, A, 5, A + 4, None), name, 'out', 'aligned')
    assert h.dt_score_regression(None, None, 0, None, None) == 0
    # the row pass
    name = 'dt_score_categorical'
    refused(h.dt_score_categorical(A, A, LB, -1, 3, 5, A, None), name, '2^31')
    refused(h.dt_score_categorical(A, A, LB, big, 3, 5, A, None), name, '2^31')
    refused(h.dt_score_categorical(A, A, LB, 5, 1, 5, A, None), name, 'C = 1')
    refused(h.dt_score_categorical(A, A, LB, 0, 1, 5, A, None), name, 'C = 1')
    refused(h.dt_score_categorical(A, A, LB, 5, 3, 0, A, None), name, 'k = 0')
    refused(h.dt_score_categorical(A, A, 2, 5, 3, 5, A, None), name, 'y_kind')
    refused(h.dt_score_categorical(A, A, EL, 1 << 29, 4, 5, A, None), name, 'overflows')
    refused(h.dt_score_categorical(None, A, EL, 5, 3, 5, A, None), name, 'null pointer')
    refused(h.dt_score_categorical(A, None, LB, 5, 3, 5, A, None), name, 'null pointer')
    refused(h.dt_score_categorical(A, A, LB, 5, 3, 5, None, None), name, 'null pointer')
    refused(h.dt_score_categorical(ODD, A, LB, 5, 3, 5, A, None), name, 'aligned')
    refused(h.dt_score_categorical(A, ODD, EL, 5, 3, 5, A, None), name, 'aligned')
    refused(h.dt_score_categorical(A, A, LB, 5, 3, 5, A + 4, None), name, 'out', 'aligned')
    assert h.dt_score_categorical(None, None, EL, 0, 3, 5, None, None) == 0
    # ranking
    name = 'dt_score_ranking'
    refused(h.dt_score_ranking(A, A, -1, A, A, None), name, '2^31')
    refused(h.dt_score_ranking(A, A, big, A, A, None), name, '2^31')
    refused(h.dt_score_ranking(None, A, 5, A, A, None), name, 'null pointer')
    refused(h.dt_score_ranking(A, None, 5, A, A, None), name, 'null pointer')
    refused(h.dt_score_ranking(A, A, 5, A, None, None), name, 'null pointer')
    refused(h.dt_score_ranking(A, A, 5, None, A, None), name, 'null workspace')
    refused(h.dt_score_ranking(ODD, A, 5, A, A, None), name, 'aligned')
    refused(h.dt_score_ranking(A, ODD, 5, A, A, None), name, 'aligned')
    refused(h.dt_score_ranking(A, A, 5, A, A + 4, None), name, 'out', 'aligned')
    refused(h.dt_score_ranking(A, A, 5, A + 8, A, None), name, 'workspace', 'aligned')
    assert h.dt_score_ranking(None, None, 0, None, None, None) == 0


def test_ranking_workspace_query_is_monotone_and_covers_the_auc_s():
    from deeptables_amd import _lib
    h = _lib.lib()
    T = h.dt_metric_sort_tile()
    sizes = [0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17, (1 << 20) + 77, 8192 * 1024, (1 << 31) - 1]
    got = [h.dt_score_ranking_workspace_bytes(n) for n in sizes]
    assert all(b > 0 for b in got) and got == sorted(got), got
    assert all(b >= h.dt_metric_auc_workspace_bytes(n) for b, n in zip(got, sizes))
    assert h.dt_score_ranking_workspace_bytes(-1) == -1 and b'2^31' in h.dt_last_error()
    assert h.dt_score_ranking_workspace_bytes(1 << 31) == -1 and b'2^31' in h.dt_last_error()
