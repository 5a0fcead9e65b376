# -*- coding:utf-8 -*-
"""GPU: the device metrics of csrc/metrics.hip — the stable radix sort, the five integers of the exact AUC, the accuracy / MSE /
MAE reductions and `DeepModel.fit` / `evaluate` on top of them — against tests/metrics_reference.py: integers exactly,
float64 sums within the rounding bound of the sum."""
import functools

import numpy as np
import pandas as pd
import pytest
import torch

from tests import metrics_reference as R

pytestmark = pytest.mark.gpu

PAD = 64            # sentinel words behind every output: a write past the end shows
SENTINEL = 0x5A5A5A5A


def _tile():
    from deeptables_amd import _lib
    return _lib.lib().dt_metric_sort_tile()


def _sizes():
    T = _tile()
    return [1, 2, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17, (1 << 20) + 77]


SIZE_IDS = ['1', '2', '63', '64', '65', 'T-1', 'T', 'T+1', '3T+17', '2^20+77']
SIZE_INDEX = list(range(len(SIZE_IDS)))


def _dev_u32(a, dev):
    return torch.from_numpy(np.array(a, dtype=np.uint32).view(np.int32)).to(dev)


def _padded(n, dev):
    return torch.full((n + PAD,), SENTINEL, dtype=torch.int32, device=dev)


def _workspace(nbytes, dev):
    return torch.full((nbytes + 4 * PAD,), 0x5A, dtype=torch.uint8, device=dev)


# ---- sort ------------------------------------------------------------------------------------------------------------------
SORT_PATTERNS = ['random', 'byte0', 'byte1', 'byte2', 'byte3', 'equal', 'sorted', 'reversed']


@functools.lru_cache(maxsize=None)
def _sort_case(pattern, n):
    rng = np.random.default_rng(1000 + n)
    if pattern == 'random':
        keys = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        if n > 2:
            keys[:2] = (0, 0xFFFFFFFF)
    elif pattern.startswith('byte'):        # keys that differ in exactly one byte: a skipped, mis-shifted or unstable pass shows
        b = int(pattern[4:])
        keys = (np.uint32(0xA5C33C5A & ~(0xFF << (8 * b))) | (rng.integers(0, 256, n).astype(np.uint32) << np.uint32(8 * b)))
    elif pattern == 'equal':
        keys = np.full(n, 0xDEADBEEF, dtype=np.uint32)
    else:
        keys = np.sort(rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32))
        if pattern == 'reversed':
            keys = keys[::-1].copy()
    keys = np.ascontiguousarray(keys, dtype=np.uint32)
    vals = np.arange(n, dtype=np.uint32)
    want_k, want_v = R.stable_sort_pairs(keys, vals)
    for a in (keys, vals, want_k, want_v):
        a.setflags(write=False)
    return keys, vals, want_k, want_v


@pytest.mark.parametrize('size', SIZE_INDEX, ids=SIZE_IDS)
@pytest.mark.parametrize('pattern', SORT_PATTERNS)
def test_sort_pairs_equals_the_stable_argsort(dev, pattern, size):
    from deeptables_amd import _lib
    h = _lib.lib()
    n = _sizes()[size]
    keys, vals, want_k, want_v = _sort_case(pattern, n)
    k, v = _dev_u32(keys, dev), _dev_u32(vals, dev)
    ko, vo = _padded(n, dev), _padded(n, dev)
    need = h.dt_metric_sort_workspace_bytes(n)
    ws = _workspace(need, dev)
    _lib.check(h.dt_metric_sort_pairs(_lib.ptr(k), _lib.ptr(v), n, _lib.ptr(ko), _lib.ptr(vo), _lib.ptr(ws), _lib.stream_ptr()),
               'dt_metric_sort_pairs')
    torch.cuda.synchronize()
    got_k, got_v = ko.cpu().numpy().view(np.uint32), vo.cpu().numpy().view(np.uint32)
    assert np.array_equal(got_k[:n], want_k)
    assert np.array_equal(got_v[:n], want_v)
    assert np.all(got_k[n:] == SENTINEL) and np.all(got_v[n:] == SENTINEL)
    assert bool((ws[need:] == 0x5A).all())
    assert np.array_equal(k.cpu().numpy().view(np.uint32), keys) and np.array_equal(v.cpu().numpy().view(np.uint32), vals)


def test_sort_pairs_in_place(dev):
    from deeptables_amd import _lib
    h = _lib.lib()
    n = 3 * _tile() + 17
    keys, vals, want_k, want_v = _sort_case('random', n)
    k, v = _dev_u32(keys, dev), _dev_u32(vals, dev)
    ws = _workspace(h.dt_metric_sort_workspace_bytes(n), dev)
    _lib.check(h.dt_metric_sort_pairs(_lib.ptr(k), _lib.ptr(v), n, _lib.ptr(k), _lib.ptr(v), _lib.ptr(ws), _lib.stream_ptr()),
               'dt_metric_sort_pairs')
    assert np.array_equal(k.cpu().numpy().view(np.uint32), want_k) and np.array_equal(v.cpu().numpy().view(np.uint32), want_v)


# ---- AUC -------------------------------------------------------------------------------------------------------------------
AUC_PATTERNS = ['uniform', 'quantised', 'equal', 'separated_up', 'separated_down', 'signed_zeros', 'logits_denormals',
                'rare_positives']


@functools.lru_cache(maxsize=None)
def _auc_case(pattern, n):
    rng = np.random.default_rng(2000 + n)
    label = (rng.random(n) < 0.3).astype(np.float32)
    if pattern == 'uniform':
        score = rng.random(n).astype(np.float32)
    elif pattern == 'quantised':            # eight levels: massive ties
        score = (rng.integers(0, 8, n) / 8).astype(np.float32)
    elif pattern == 'equal':
        score = np.full(n, 0.7, dtype=np.float32)
    elif pattern == 'separated_up':
        score = (label + 0.5 * rng.random(n)).astype(np.float32)
    elif pattern == 'separated_down':
        score = (-label - 0.5 * rng.random(n)).astype(np.float32)
    elif pattern == 'signed_zeros':         # every positive at -0.0, every negative at +0.0: all ties; bit order would give U2 = 0
        score = np.where(label == 1, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    elif pattern == 'logits_denormals':
        score = (4 * rng.standard_normal(n)).astype(np.float32)
        tiny = rng.random(n) < 0.2
        score[tiny] = (rng.integers(-3, 4, int(tiny.sum())) * np.float32(1e-45)).astype(np.float32)
        score[rng.random(n) < 0.05] = np.float32(-0.0)
    else:                                   # 3 % positives, scores that know something about the label
        label = (rng.random(n) < 0.03).astype(np.float32)
        score = (1 / (1 + np.exp(-(rng.standard_normal(n) + 0.8 * label - 2)))).astype(np.float32)
    words = R.auc_words_fast(score, label)
    if n <= 65:
        assert words == R.auc_words(score, label) and words[0] == R.brute_force_u2(score, label)
    score.setflags(write=False)
    label.setflags(write=False)
    return score, label, words


def _auc_words_device(score, label, dev):
    from deeptables_amd import _lib
    h = _lib.lib()
    n = score.shape[0]
    s, y = torch.from_numpy(np.array(score)).to(dev), torch.from_numpy(np.array(label)).to(dev)
    need = h.dt_metric_auc_workspace_bytes(n)
    ws = _workspace(need, dev)
    out = torch.full((5 + PAD,), -7, dtype=torch.int64, device=dev)
    both = []
    for _ in range(2):
        _lib.check(h.dt_metric_auc(_lib.ptr(s), _lib.ptr(y), n, _lib.ptr(ws), _lib.ptr(out), _lib.stream_ptr()), 'dt_metric_auc')
        both.append(tuple(out[:5].cpu().tolist()))
    assert bool((out[5:] == -7).all()) and bool((ws[need:] == 0x5A).all())
    assert np.array_equal(s.cpu().numpy().view(np.uint32), np.asarray(score).view(np.uint32))      # inputs are not written
    assert np.array_equal(y.cpu().numpy().view(np.uint32), np.asarray(label).view(np.uint32))
    return both


@pytest.mark.parametrize('size', SIZE_INDEX, ids=SIZE_IDS)
@pytest.mark.parametrize('pattern', AUC_PATTERNS)
def test_auc_words_equal_the_reference(dev, pattern, size):
    n = _sizes()[size]
    score, label, want = _auc_case(pattern, n)
    first, second = _auc_words_device(score, label, dev)
    assert first == want, (first, want)
    assert second == first                      # bit-reproducible from call to call
    u2, P, N = want[:3]
    if pattern == 'equal' or pattern == 'signed_zeros':
        assert u2 == P * N                      # AUC exactly 0.5
    elif pattern == 'separated_up':
        assert u2 == 2 * P * N                  # 1.0
    elif pattern == 'separated_down':
        assert u2 == 0                          # 0.0


def test_auc_counts_nonfinite_scores_and_bad_labels(dev):
    n = _tile() + 5
    rng = np.random.default_rng(9)
    score = rng.standard_normal(n).astype(np.float32)
    label = (rng.random(n) < 0.5).astype(np.float32)
    score[[3, n - 1]] = np.nan, -np.inf
    score[700] = np.inf
    label[[0, 64, n - 2]] = 2.0, 0.5, np.nan
    want = R.auc_words_fast(score, label)
    assert want[3:] == (3, 3)
    assert _auc_words_device(score, label, dev)[0] == want


def _device_metrics(names, y, p, task, dev):
    from deeptables_amd import metrics
    return metrics.compute_metrics_device(names, torch.from_numpy(np.array(y)).to(dev), torch.from_numpy(np.array(p)).to(dev), task)


def test_auc_through_compute_metrics_device(dev, monkeypatch):
    from deeptables_amd import metrics
    n = 2 * _tile() + 3
    score, label, words = _auc_case('rare_positives', n)
    got = _device_metrics(['AUC'], label, score.reshape(-1, 1), 'binary', dev)
    assert got == {'AUC': words[0] / (2 * words[1] * words[2])}
    assert abs(got['AUC'] - metrics.compute_metric('AUC', label, score, 'binary')) <= 1e-12
    # one class only, a NaN, an Inf: nan, as the host path (roc_auc_score raises there)
    assert np.isnan(_device_metrics(['auc'], np.zeros(n, dtype=np.float32), score, 'binary', dev)['auc'])
    assert np.isnan(_device_metrics(['auc'], np.ones(n, dtype=np.float32), score, 'binary', dev)['auc'])
    for bad in (np.nan, np.inf):
        s = np.array(score)
        s[n // 2] = bad
        assert np.isnan(_device_metrics(['AUC'], label, s, 'binary', dev)['AUC'])
        assert np.isnan(metrics.compute_metric('AUC', label, s, 'binary'))
    # a label 2.0: the host path's value, whatever it is (here: roc_auc_score takes 2 for the positive class)
    y2 = np.array(label) * 2
    want = metrics.compute_metric('AUC', y2, score, 'binary')
    assert np.isfinite(want) and _device_metrics(['AUC'], y2, score, 'binary', dev)['AUC'] == want
    y3 = np.array(label)
    y3[5] = 2.0
    assert np.isnan(metrics.compute_metric('AUC', y3, score, 'binary')) and np.isnan(_device_metrics(['AUC'], y3, score, 'binary', dev)['AUC'])


# ---- accuracy / MSE / MAE --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sums_case(kind, n):
    rng = np.random.default_rng(3000 + n)
    if kind == 'binary':
        y = (rng.random(n) < 0.4).astype(np.float32)
        p = rng.random(n).astype(np.float32)
        p[rng.random(n) < 0.1] = np.float32(0.5)          # on the threshold: (p > 0.5) is false
    else:
        y = (10 * rng.standard_normal(n)).astype(np.float32)
        p = (y + rng.standard_normal(n) * np.float32(10.0) ** rng.integers(-6, 3, n)).astype(np.float32)
    want = R.sums(y, p)
    y.setflags(write=False)
    p.setflags(write=False)
    return y, p, want


@pytest.mark.parametrize('size', SIZE_INDEX, ids=SIZE_IDS)
@pytest.mark.parametrize('kind', ['binary', 'regression'])
def test_sums_hits_exact_and_float64_sums_within_the_rounding_bound(dev, kind, size):
    from deeptables_amd import _lib
    h = _lib.lib()
    n = _sizes()[size]
    y, p, (hits, sq, ab) = _sums_case(kind, n)
    yd, pd_ = torch.from_numpy(np.array(y)).to(dev), torch.from_numpy(np.array(p)).to(dev)
    out = torch.full((_lib.DT_METRIC_SUMS_WORDS + PAD,), -7, dtype=torch.int64, device=dev)
    both = []
    for _ in range(2):
        _lib.check(h.dt_metric_sums(_lib.ptr(yd), _lib.ptr(pd_), n, _lib.ptr(out), _lib.stream_ptr()), 'dt_metric_sums')
        both.append(out[:3].cpu())
    assert torch.equal(both[0], both[1])
    assert bool((out[_lib.DT_METRIC_SUMS_WORDS:] == -7).all())
    got_hits = int(both[0][0])
    got_sq, got_ab = (float(v) for v in both[0][1:3].view(torch.float64))
    bound = R.sum_bound(n)
    print(f'{kind} n={n}: hits {got_hits} / {hits}; rel err sq {abs(got_sq - sq) / max(sq, 1e-300):.3e} '
          f'ab {abs(got_ab - ab) / max(ab, 1e-300):.3e}; bound {bound:.3e}')
    assert got_hits == hits
    assert abs(got_sq - sq) <= bound * sq and abs(got_ab - ab) <= bound * ab
    task = 'binary' if kind == 'binary' else 'regression'
    got = _device_metrics(['accuracy', 'mse', 'rmse', 'mae'], y, p.reshape(-1, 1), task, dev)
    assert got['accuracy'] == hits / n
    assert got['mse'] == got_sq / n and got['mae'] == got_ab / n and got['rmse'] == np.sqrt(got_sq / n)


@pytest.mark.parametrize('size', SIZE_INDEX, ids=SIZE_IDS)
@pytest.mark.parametrize('C', [3, 10])
def test_multiclass_hits_exact(dev, C, size):
    from deeptables_amd import _lib, metrics
    h = _lib.lib()
    n = _sizes()[size]
    rng = np.random.default_rng(4000 + n + C)
    p = np.round(rng.random((n, C)), 1).astype(np.float32)      # one decimal: many rows have tied maxima, the first one wins
    assert n < 1000 or int(((p == p.max(1, keepdims=True)).sum(1) > 1).sum()) > n // 20
    labels = np.where(rng.random(n) < 0.5, p.argmax(-1), rng.integers(0, C, n)).astype(np.float32)
    onehot = np.eye(C, dtype=np.float32)[labels.astype(np.int64)]
    pd_ = torch.from_numpy(p).to(dev)
    for y, kind in ((labels, _lib.DT_METRIC_Y_LABELS), (onehot, _lib.DT_METRIC_Y_ONEHOT)):
        want = R.argmax_hits(p, y)
        yd = torch.from_numpy(y).to(dev)
        out = torch.full((1 + PAD,), -7, dtype=torch.int64, device=dev)
        _lib.check(h.dt_metric_argmax_hits(_lib.ptr(pd_), _lib.ptr(yd), kind, n, C, _lib.ptr(out), _lib.stream_ptr()),
                   'dt_metric_argmax_hits')
        assert int(out[0]) == want and bool((out[1:] == -7).all())
        got = metrics.compute_metrics_device(['accuracy'], yd, pd_, 'multiclass')
        assert got == {'accuracy': metrics.compute_metric('accuracy', y, p, 'multiclass')} == {'accuracy': want / n}


# ---- end to end ------------------------------------------------------------------------------------------------------------
F, ND, D, V, ROWS = 6, 3, 8, 30, 600


def _frame(task):
    rng = np.random.RandomState(11)
    df = pd.DataFrame({f'C{i}': rng.randint(0, V + i, ROWS) for i in range(F)})
    for j in range(ND):
        df[f'I{j}'] = rng.randn(ROWS).astype(np.float32)
    y = (rng.rand(ROWS) < 0.3).astype(np.float32) if task == 'binary' else rng.randn(ROWS).astype(np.float32)
    return df, y


def _model(task, metrics):
    from deeptables_amd import functional
    from deeptables_amd.models import ModelConfig, DeepModel, deepnets
    from deeptables_amd.models.metainfo import CategoricalColumn, ContinuousColumn
    functional.set_seed(4)
    conf = ModelConfig(nets=deepnets.DeepFM, fixed_embedding_dim=True, embeddings_output_dim=D, embedding_dropout=0,
                       metrics=metrics)
    cats = [CategoricalColumn(f'C{i}', V + i, D) for i in range(F)]
    conts = [ContinuousColumn('input_continuous_all', [f'I{j}' for j in range(ND)])]
    dm = DeepModel(task, 2 if task == 'binary' else 1, conf, cats, conts)
    dm.build()
    return dm


def _forbid_the_host_path(monkeypatch):
    import sklearn.metrics
    from deeptables_amd import metrics

    def forbidden(*a, **k):
        raise AssertionError('the host metric path was taken')

    monkeypatch.setattr(sklearn.metrics, 'roc_auc_score', forbidden)
    monkeypatch.setattr(metrics, 'compute_metric', forbidden)


def test_fit_and_evaluate_score_on_the_device_binary(dev, monkeypatch):
    from deeptables_amd import metrics
    df, y = _frame('binary')
    dm = _model('binary', ['AUC', 'accuracy'])
    with monkeypatch.context() as mp:
        _forbid_the_host_path(mp)
        hist = dm.fit(df, y, batch_size=64, epochs=2, verbose=0, validation_split=0.2)
        ev = dm.evaluate(df, y, batch_size=64)
    for k in ('AUC', 'accuracy', 'val_AUC', 'val_accuracy'):
        assert k in hist.history and len(hist.history[k]) == 2 and all(np.isfinite(hist.history[k])), (k, hist.history)
    assert all(k in ev for k in ('loss', 'AUC', 'accuracy'))
    again = dm.evaluate(df, y, batch_size=64)
    prob = dm.predict(df, batch_size=64)
    assert abs(again['AUC'] - metrics.compute_metric('AUC', y, prob, 'binary')) <= 1e-12
    assert again['accuracy'] == metrics.compute_metric('accuracy', y, prob, 'binary')
    assert again['AUC'] == ev['AUC'] and again['accuracy'] == ev['accuracy']


def test_fit_and_evaluate_score_on_the_device_regression(dev, monkeypatch):
    df, y = _frame('regression')
    dm = _model('regression', ['mse', 'mae'])
    with monkeypatch.context() as mp:
        _forbid_the_host_path(mp)
        hist = dm.fit(df, y, batch_size=64, epochs=2, verbose=0, validation_split=0.2)
        ev = dm.evaluate(df, y, batch_size=64)
    for k in ('mse', 'mae', 'val_mse', 'val_mae'):
        assert k in hist.history and len(hist.history[k]) == 2 and all(np.isfinite(hist.history[k])), (k, hist.history)
    pred = dm.predict(df, batch_size=64)
    _, sq, ab = R.sums(y, pred)
    bound = R.sum_bound(ROWS)
    print(f'mse {ev["mse"]!r} vs {sq / ROWS!r}; mae {ev["mae"]!r} vs {ab / ROWS!r}; bound {bound:.3e}')
    assert abs(ev['mse'] - sq / ROWS) <= bound * (sq / ROWS)
    assert abs(ev['mae'] - ab / ROWS) <= bound * (ab / ROWS)


def test_the_switch_restores_the_host_path(dev, monkeypatch):
    """DT_AMD_DEVICE_METRICS=0: evaluate scores on the host as before, and the two paths agree"""
    df, y = _frame('binary')
    dm = _model('binary', ['AUC', 'accuracy'])
    dm.fit(df, y, batch_size=64, epochs=1, verbose=0, validation_split=0)
    on = dm.evaluate(df, y, batch_size=64)
    monkeypatch.setenv('DT_AMD_DEVICE_METRICS', '0')
    off = dm.evaluate(df, y, batch_size=64)
    assert abs(on['AUC'] - off['AUC']) <= 1e-12 and on['accuracy'] == off['accuracy']
