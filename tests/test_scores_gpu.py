# -*- coding:utf-8 -*-
"""GPU: the dt_score_* entry points of csrc/metrics.hip — log loss + precision / recall counts, MSLE / MAPE, top-k hits +
categorical cross-entropy, AUC + average precision — called through the C-ABI against tests/scores_reference.py: integers
exactly, float64 sums within the bounds derived there; then metrics.compute_metrics_device and fit / evaluate on top."""
import functools
import math

import numpy as np
import pandas as pd
import pytest
import torch

from tests import scores_reference as S

pytestmark = pytest.mark.gpu

PAD = 64            # sentinel words behind every output: a write past the end shows
K = 5
DENORMAL = np.float32(1e-45)


def _lib():
    from deeptables_amd import _lib
    return _lib


def _dev(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _call(words, dev, launch, inputs):
    """run `launch(out)` twice on an output of `words` words with sentinels behind: the result words (int64 tensor on the host),
    the same bits both times, nothing written past the end, the inputs untouched"""
    L = _lib()
    out = torch.full((words + PAD,), -7, dtype=torch.int64, device=dev)
    before = [_bits(t).copy() for t in inputs]
    got = []
    for _ in range(2):
        L.check(launch(L.ptr(out)), 'dt_score')
        got.append(out[:words].cpu())
    assert torch.equal(got[0], got[1])                       # bit-reproducible from call to call (partials included)
    assert bool((out[words:] == -7).all())
    for t, b in zip(inputs, before):
        assert np.array_equal(_bits(t), b)
    return got[0]


def _f64(words, k):
    return float(words[k:k + 1].view(torch.float64))


def _check_sum(what, got, want, bound_abs):
    err = abs(got - want) if math.isfinite(want) and math.isfinite(got) else float('nan')
    print(f'{what}: got {got!r} want {want!r} abs err {err:.3e} bound {bound_abs:.3e}'
          + (f' (rel err {err / abs(want):.3e})' if want and math.isfinite(err) else ''))
    if math.isnan(want):
        assert math.isnan(got), what
    elif math.isinf(want):
        assert got == want, what
    else:
        assert abs(got - want) <= bound_abs, what


# ---- the element-wise pass -------------------------------------------------------------------------------------------------
FLAT_SIZES = [1, 2, 63, 64, 65, 1023, 1024, 1025, 256 * 1024 + 1, (1 << 20) + 77]


@functools.lru_cache(maxsize=None)
def _binary_case(pattern, n):
    rng = np.random.default_rng(5000 + n)
    if pattern == 'labels':
        C = 3
        p = rng.random((n, C)).astype(np.float32)
        y = rng.integers(0, C, n).astype(np.float32)
        y[3::41] = 3.0                                   # labels that name no class: a row of zeros
        y[5::43] = -1.0
        y[7::47] = np.nan
    else:
        p = rng.random(n).astype(np.float32)
        if pattern == 'hard':
            y = (rng.random(n) < 0.4).astype(np.float32)
        else:                                            # soft labels, the ends and the middle among them
            y = rng.random(n).astype(np.float32)
            y[1::13], y[2::13], y[3::13] = 0.0, 1.0, 0.5
    flat = p.reshape(-1)
    specials = [0.0, 1.0, 0.5, np.nextafter(np.float32(0.5), np.float32(1)), -0.0, DENORMAL, -DENORMAL, -0.3, 1.7, 1e-7,
                0.99999994, 3e38]
    for j, v in enumerate(specials):                     # threshold, the clip's ends, outside [0, 1], signed zero, denormals
        flat[j::17 + j] = np.float32(v)
    want = S.binary_words(y, p)
    assert math.isfinite(want[4]) and want[4] > 0
    y.setflags(write=False)
    p.setflags(write=False)
    return y, p, want


def _binary_device(y, p, dev):
    L = _lib()
    h = L.lib()
    yd, pd_ = _dev(y, dev), _dev(p, dev)
    if y.size == p.size:
        args = (L.DT_METRIC_Y_ONEHOT, p.size, 1)
    else:
        args = (L.DT_METRIC_Y_LABELS, p.shape[0], p.shape[1])
    words = _call(L.DT_SCORE_BINARY_WORDS, dev,
                  lambda out: h.dt_score_binary(L.ptr(yd), L.ptr(pd_), *args, out, L.stream_ptr()), [yd, pd_])
    return tuple(int(v) for v in words[:4]) + (_f64(words, 4),)


@pytest.mark.parametrize('n', FLAT_SIZES)
@pytest.mark.parametrize('pattern', ['hard', 'soft', 'labels'])
def test_binary_pass_counts_exact_and_log_loss_within_the_bound(dev, pattern, n):
    if pattern == 'labels':
        n = {256 * 1024 + 1: (256 * 1024) // 3 + 1, (1 << 20) + 77: 200003}[n] if n > 2000 else n     # n * 3 elements
    y, p, want = _binary_case(pattern, n)
    got = _binary_device(y, p, dev)
    assert got[:4] == want[:4], (got, want)
    assert sum(got[:4]) == p.size
    # scores_reference.E_BCE: T = the number of elements
    _check_sum(f'bce {pattern} n={n}', got[4], want[4], S.sum_bound(p.size, S.E_BCE) * want[4])


def test_binary_pass_nan_and_inf_come_out_as_numpy_gives_them(dev):
    base_y = np.array([0, 1, 1, 0, 0.25, 1, 0, 1], dtype=np.float32)
    base_p = np.array([0.2, 0.7, 0.4, 0.6, 0.5, 0.9, 0.1, 0.3], dtype=np.float32)
    seen = set()
    for where, value in [('p', np.nan), ('p', np.inf), ('p', -np.inf), ('y', np.nan), ('y', np.inf), ('y', -np.inf),
                         ('y', 2.0), ('y', 0.5), ('y', -0.0)]:
        y, p = base_y.copy(), base_p.copy()
        (p if where == 'p' else y)[2] = value
        want = S.binary_words(y, p)
        got = _binary_device(y, p, dev)
        assert got[:4] == want[:4], (where, value, got, want)
        _check_sum(f'bce {where}[2]={value}', got[4], want[4], S.sum_bound(8, S.E_BCE) * abs(want[4]))
        seen.add('nan' if math.isnan(want[4]) else 'finite')
    assert seen == {'nan', 'finite'}            # a NaN p and NaN / Inf labels poison the sum; an Inf p is clipped
    # the clip keeps a NaN (fmin / fmax would turn it into a bound) and clips +-Inf
    p = base_p.copy()
    p[0] = np.nan
    assert math.isnan(_binary_device(base_y, p, dev)[4])
    p[0] = np.inf
    assert math.isfinite(_binary_device(base_y, p, dev)[4])
    # label 2 and label 0.5 are positives for precision / recall; a NaN label too (NaN != 0)
    y = np.array([2, 0.5, np.nan, 0, -0.0], dtype=np.float32)
    p = np.array([0.9, 0.1, 0.8, 0.7, 0.2], dtype=np.float32)
    assert _binary_device(y, p, dev)[:4] == (2, 1, 1, 1) == S.binary_words(y, p)[:4]
    # all-positive and all-negative labels, nothing predicted positive
    n = 300
    p = np.random.default_rng(1).random(n).astype(np.float32)
    for y in (np.ones(n, np.float32), np.zeros(n, np.float32)):
        assert _binary_device(y, p, dev)[:4] == S.binary_words(y, p)[:4]
    assert _binary_device(np.ones(n, np.float32), p * np.float32(0.5), dev)[:2] == (0, 0)


# ---- the regression pass ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _regression_case(pattern, n):
    rng = np.random.default_rng(6000 + n)
    if pattern == 'positive':
        y = (0.01 + np.exp(2 * rng.standard_normal(n))).astype(np.float32)
        p = (y * np.exp(rng.standard_normal(n) * 10.0 ** rng.integers(-6, 1, n))).astype(np.float32)
    else:                                                # both signs, zeros of both signs, denormals, equal pairs
        y = (10 * rng.standard_normal(n)).astype(np.float32)
        p = (y + rng.standard_normal(n)).astype(np.float32)
        for j, v in enumerate([0.0, -0.0, DENORMAL, -DENORMAL, 1e-7, 3e38, -3e38]):
            y[j::19 + j] = np.float32(v)
            p[j + 1::23 + j] = np.float32(v)
        p[4::29] = y[4::29]
    want = S.regression_sums(y, p)
    assert all(math.isfinite(v) for v in want)
    y.setflags(write=False)
    p.setflags(write=False)
    return y, p, want


def _regression_device(y, p, dev):
    L = _lib()
    h = L.lib()
    yd, pd_ = _dev(y, dev), _dev(p, dev)
    words = _call(L.DT_SCORE_REGRESSION_WORDS, dev,
                  lambda out: h.dt_score_regression(L.ptr(yd), L.ptr(pd_), y.size, out, L.stream_ptr()), [yd, pd_])
    return _f64(words, 0), _f64(words, 1)


@pytest.mark.parametrize('n', FLAT_SIZES)
@pytest.mark.parametrize('pattern', ['positive', 'mixed'])
def test_regression_pass_sums_within_the_bound(dev, pattern, n):
    y, p, (sl, pe, kappa) = _regression_case(pattern, n)
    got_sl, got_pe = _regression_device(y, p, dev)
    _check_sum(f'msle {pattern} n={n}', got_sl, sl, S.msle_bound(n, sl, kappa))
    _check_sum(f'mape {pattern} n={n}', got_pe, pe, S.sum_bound(n, S.E_MAPE) * pe)


def test_regression_pass_nan_and_inf_come_out_as_numpy_gives_them(dev):
    base_y = np.array([1, 2, 3, 4, 0.5], dtype=np.float32)
    base_p = np.array([1.5, 1, 3, 5, 0.25], dtype=np.float32)
    for where, value in [('p', np.nan), ('p', np.inf), ('p', -np.inf), ('y', np.nan), ('y', np.inf), ('y', -np.inf), ('b', np.inf)]:
        y, p = base_y.copy(), base_p.copy()
        if where in ('p', 'b'):
            p[1] = value
        if where in ('y', 'b'):
            y[1] = value
        sl, pe, kappa = S.regression_sums(y, p)
        got_sl, got_pe = _regression_device(y, p, dev)
        _check_sum(f'msle {where}[1]={value}', got_sl, sl, S.msle_bound(5, sl, kappa) if math.isfinite(sl) else 0.0)
        _check_sum(f'mape {where}[1]={value}', got_pe, pe, S.sum_bound(5, S.E_MAPE) * pe if math.isfinite(pe) else 0.0)


# ---- the row pass ----------------------------------------------------------------------------------------------------------
ROW_C = [2, 3, 5, 7, 32, 33, 64, 65, 257]              # 32 | 33: a thread per row | a wave per row


def _row_sizes(C):
    L = _lib()
    per_block = 256 if C <= L.DT_SCORE_THREAD_ROW_MAX_C else 4
    return [1, 255, 256, 257, L.DT_SCORE_BLOCKS * per_block + 1]          # the last: one row past the grid-stride cap


@functools.lru_cache(maxsize=None)
def _rows_case(n, C, thread_row_max_c):
    rng = np.random.default_rng(7000 + n + C)
    z = rng.standard_normal((n, C))
    p = np.exp(z) / np.exp(z).sum(1, keepdims=True)
    p = (np.round(p * 8 * C) / (8 * C)).astype(np.float32)          # a grid: ties in every row
    p[:, 0] += np.float32(0.25)                                      # (no row sums to zero here)
    r = np.arange(n)
    p[r % 11 == 1] *= np.float32(3)                                  # rows summing to about 3
    p[r % 13 == 2, :min(C, 7)] = np.float32(0.125)                   # up to seven classes tied: across the top-5 boundary
    p[r % 17 == 3, 0] = np.float32(1.5)                              # outside [0, 1]
    p[r % 19 == 4, C - 1] = np.float32(-0.05)
    p[r % 29 == 6, 1] = DENORMAL
    p[r % 31 == 7, C - 1] = np.float32(-0.0)
    labels = rng.integers(0, C, n).astype(np.float32)
    onehot = np.eye(C, dtype=np.float32)[labels.astype(np.int64)]
    onehot[r % 23 == 5] = 0                                          # an all-zero row: the target is class 0
    want = {'labels': S.categorical_words(p, labels, K, thread_row_max_c), 'onehot': S.categorical_words(p, onehot, K, thread_row_max_c)}
    assert all(math.isfinite(w[1]) and w[1] > 0 for w in want.values())
    for a in (p, labels, onehot):
        a.setflags(write=False)
    return p, labels, onehot, want


def _rows_device(p, y, k, dev):
    L = _lib()
    h = L.lib()
    kind = L.DT_METRIC_Y_ONEHOT if y.shape == p.shape else L.DT_METRIC_Y_LABELS
    pd_, yd = _dev(p, dev), _dev(y, dev)
    words = _call(L.DT_SCORE_CATEGORICAL_WORDS, dev,
                  lambda out: h.dt_score_categorical(L.ptr(pd_), L.ptr(yd), kind, p.shape[0], p.shape[1], k, out, L.stream_ptr()),
                  [pd_, yd])
    return int(words[0]), _f64(words, 1)


@pytest.mark.parametrize('size', range(5), ids=['1', '255', '256', '257', 'cap+1'])
@pytest.mark.parametrize('C', ROW_C)
def test_row_pass_hits_exact_and_cross_entropy_within_the_bound(dev, C, size):
    n = _row_sizes(C)[size]
    p, labels, onehot, want = _rows_case(n, C, _lib().DT_SCORE_THREAD_ROW_MAX_C)
    for form, y in (('labels', labels), ('onehot', onehot)):
        hits, ce = _rows_device(p, y, K, dev)
        assert hits == want[form][0], (form, hits, want[form][0])
        if C <= K:
            assert hits == n
        # scores_reference.E_CCE: T = n rows + the C terms of a row's inner sum
        _check_sum(f'cce {form} n={n} C={C}', ce, want[form][1], S.sum_bound(n + C, S.E_CCE) * want[form][1])


@pytest.mark.parametrize('C', [7, 65])
def test_row_pass_other_k(dev, C):
    p, labels, onehot, _ = _rows_case(257, C, _lib().DT_SCORE_THREAD_ROW_MAX_C)
    for k in (1, 3, 7, 1000):
        want = S.categorical_words(p, labels, k, 32)[0]
        assert want == S.top_k_brute_force(p, labels.astype(np.int64), k)
        assert _rows_device(p, labels, k, dev)[0] == want
        assert _rows_device(p, onehot, k, dev)[0] == S.categorical_words(p, onehot, k, 32)[0]


@pytest.mark.parametrize('C', [3, 70])
def test_row_pass_hard_rows_one_at_a_time(dev, C):
    """every hard input alone in a one-row call, so that the NaN (or the miss) shows exactly where the reference has it"""
    T = _lib().DT_SCORE_THREAD_ROW_MAX_C
    rng = np.random.default_rng(C)
    base = (0.05 + rng.random(C)).astype(np.float32)
    t = 1                                                            # the target class of the plain rows
    eye = np.eye(C, dtype=np.float32)

    def row(**changes):
        p = base.copy()
        for c, v in changes.items():
            p[int(c[1:])] = v
        return p[None, :]

    cases = [
        ('plain', row(), eye[t][None, :]),
        ('NaN at the target', row(c1=np.nan), eye[t][None, :]),
        ('NaN elsewhere', row(c2=np.nan), eye[t][None, :]),
        ('+Inf elsewhere', row(c2=np.inf), eye[t][None, :]),
        ('+Inf at the target', row(c1=np.inf), eye[t][None, :]),
        ('-Inf elsewhere', row(c0=-np.inf), eye[t][None, :]),
        ('a row of zeros', np.zeros((1, C), np.float32), eye[t][None, :]),
        ('a row summing to 3', row() * np.float32(3) / base.sum(), eye[t][None, :]),
        ('ties everywhere', np.full((1, C), 0.25, np.float32), eye[t][None, :]),
        ('one-hot row of zeros', row(), np.zeros((1, C), np.float32)),
        ('NaN in the one-hot row, class 0', row(), np.where(np.arange(C) == 0, np.nan, eye[t])[None, :].astype(np.float32)),
        ('NaN in the one-hot row, class 2', row(), np.where(np.arange(C) == 2, np.nan, eye[t])[None, :].astype(np.float32)),
        ('Inf in the one-hot row', row(), np.where(np.arange(C) == 2, np.inf, eye[t])[None, :].astype(np.float32)),
        ('soft one-hot row', row(), (eye[t] * 0.7 + eye[2] * 0.3)[None, :].astype(np.float32)),
        ('-0.0 and denormal scores', row(c0=-0.0, c2=DENORMAL), eye[0][None, :]),
    ]
    for v in (float(t), 1.5, float(C - 1), float(C), -1.0, np.nan, np.inf, -0.0):
        cases.append((f'label {v}', row(), np.array([v], dtype=np.float32)))
    cases.append(('label, NaN at the target', row(c1=np.nan), np.array([1.0], dtype=np.float32)))
    nan_seen = 0
    for what, p, y in cases:
        want_hits, want_ce = S.categorical_words(p, y, K, T)
        hits, ce = _rows_device(np.ascontiguousarray(p, dtype=np.float32), y, K, dev)
        assert hits == want_hits, (what, hits, want_hits)
        _check_sum(f'C={C} {what}', ce, want_ce, S.sum_bound(1 + C, S.E_CCE) * abs(want_ce) if math.isfinite(want_ce) else 0.0)
        nan_seen += math.isnan(want_ce)
    assert 6 <= nan_seen < len(cases)


# ---- ranking ---------------------------------------------------------------------------------------------------------------
RANK_PATTERNS = ['uniform', 'quantised', 'equal', 'rare_positives', 'signed_zeros', 'all_positive', 'all_negative']
SIZE_IDS = ['1', '2', '63', '64', '65', 'T-1', 'T', 'T+1', '3T+17', '2^20+77']


def _rank_sizes():
    T = _lib().lib().dt_metric_sort_tile()
    return [1, 2, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17, (1 << 20) + 77]


@functools.lru_cache(maxsize=None)
def _rank_case(pattern, n):
    rng = np.random.default_rng(8000 + n)
    label = (rng.random(n) < 0.3).astype(np.float32)
    if pattern == 'uniform':
        score = rng.random(n).astype(np.float32)
    elif pattern == 'quantised':            # eight levels: massive ties
        score = (rng.integers(0, 8, n) / 8).astype(np.float32)
    elif pattern == 'equal':                # one group spanning every tile
        score = np.full(n, 0.7, dtype=np.float32)
    elif pattern == 'signed_zeros':
        score = np.where(label == 1, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    elif pattern == 'rare_positives':
        label = (rng.random(n) < 0.03).astype(np.float32)
        score = (1 / (1 + np.exp(-(rng.standard_normal(n) + 0.8 * label - 2)))).astype(np.float32)
    else:
        label = np.full(n, 1.0 if pattern == 'all_positive' else 0.0, dtype=np.float32)
        score = (rng.integers(0, 64, n) / 64).astype(np.float32)
    want = S.ranking_words(score, label)
    score.setflags(write=False)
    label.setflags(write=False)
    return score, label, want


def _ranking_device(score, label, dev):
    L = _lib()
    h = L.lib()
    n = score.shape[0]
    s, y = _dev(score, dev), _dev(label, dev)
    need = h.dt_score_ranking_workspace_bytes(n)
    assert need >= h.dt_metric_auc_workspace_bytes(n)
    ws = torch.full((need + 4 * PAD,), 0x5A, dtype=torch.uint8, device=dev)
    words = _call(L.DT_SCORE_RANKING_WORDS, dev,
                  lambda out: h.dt_score_ranking(L.ptr(s), L.ptr(y), n, L.ptr(ws), out, L.stream_ptr()), [s, y])
    assert bool((ws[need:] == 0x5A).all())
    out5 = torch.full((5 + PAD,), -7, dtype=torch.int64, device=dev)
    L.check(h.dt_metric_auc(L.ptr(s), L.ptr(y), n, L.ptr(ws), L.ptr(out5), L.stream_ptr()), 'dt_metric_auc')
    assert torch.equal(out5[:5].cpu(), words[:5])                  # the five words are dt_metric_auc's
    return tuple(int(v) for v in words[:5]), _f64(words, 5)


@pytest.mark.parametrize('size', range(10), ids=SIZE_IDS)
@pytest.mark.parametrize('pattern', RANK_PATTERNS)
def test_ranking_words_exact_and_average_precision_within_the_bound(dev, pattern, size):
    n = _rank_sizes()[size]
    score, label, want = _rank_case(pattern, n)
    words, total = _ranking_device(score, label, dev)
    assert words == want[:5], (words, want[:5])
    groups, P = want[6], want[1]
    # scores_reference.E_AP: T = the number of groups
    _check_sum(f'ap {pattern} n={n} groups={groups}', total, want[5], S.sum_bound(groups, S.E_AP) * want[5])
    if P == 0:
        assert total == 0.0
    elif pattern == 'all_positive':
        assert abs(total / P - 1.0) <= S.sum_bound(groups, S.E_AP)
    elif pattern in ('equal', 'signed_zeros'):
        assert groups == 1 and total == P * P / n                   # one group: AP = P / n


def test_ranking_counts_nonfinite_scores_and_bad_labels(dev):
    n = _lib().lib().dt_metric_sort_tile() + 5
    rng = np.random.default_rng(9)
    score = rng.standard_normal(n).astype(np.float32)
    label = (rng.random(n) < 0.5).astype(np.float32)
    score[[3, n - 1]] = np.nan, -np.inf
    score[700] = np.inf
    label[[0, 64, n - 2]] = 2.0, 0.5, np.nan
    want = S.ranking_words(score, label)
    assert want[3:5] == (3, 3)
    words, total = _ranking_device(score, label, dev)
    assert words == want[:5]
    _check_sum('ap with non-finite scores', total, want[5], S.sum_bound(want[6], S.E_AP) * want[5])


# ---- compute_metrics_device ------------------------------------------------------------------------------------------------
def _device_and_host(names, y, p, task, dev, monkeypatch):
    from deeptables_amd import metrics
    yd, pd_ = _dev(y, dev), _dev(p, dev)
    assert metrics.device_metrics_supported(names, yd, pd_, task)
    got = metrics.compute_metrics_device(names, yd, pd_, task)
    assert metrics.epoch_metrics(names, yd, pd_, task) == got
    with monkeypatch.context() as mp:
        mp.setenv('DT_AMD_DEVICE_METRICS', '0')
        mp.setattr(metrics, 'compute_metrics_device', lambda *a, **k: pytest.fail('device path taken'))
        host = metrics.epoch_metrics(names, yd, pd_, task)
    assert list(got) == list(names) == list(host)
    return got, host


def _within(what, got, want, rel):
    # the value is the sum over the count: one more rounding on each side
    print(f'{what}: device {got!r} host {want!r} rel err {abs(got - want) / abs(want):.3e} bound {rel + 2 * S.U:.3e}')
    assert abs(got - want) <= (rel + 2 * S.U) * abs(want), what


def test_compute_metrics_device_binary_set(dev, monkeypatch):
    from deeptables_amd import metrics
    n = 2 * _lib().lib().dt_metric_sort_tile() + 3
    score, label, want = _rank_case('rare_positives', n)
    p = score.reshape(-1, 1)
    names = ['AUC', 'average_precision', 'binary_crossentropy', 'Precision', 'Recall', 'accuracy']
    got, host = _device_and_host(names, label, p, 'binary', dev, monkeypatch)
    two = metrics.compute_metrics_device(['AUC', 'accuracy'], _dev(label, dev), _dev(p, dev), 'binary')
    assert two == {'AUC': got['AUC'], 'accuracy': got['accuracy']}                  # bit-equal: the same integers
    assert got['Precision'] == host['Precision'] and got['Recall'] == host['Recall'] and got['accuracy'] == host['accuracy']
    assert abs(got['AUC'] - host['AUC']) <= 1e-12
    # (the host's value is sklearn's own arithmetic, which test_scores_host.py holds to the reference at 1e-12)
    ap_bound = (S.sum_bound(want[6], S.E_AP) + 2 * S.U) * host['average_precision'] + 1e-12
    print(f"average_precision: device {got['average_precision']!r} host {host['average_precision']!r} bound {ap_bound:.3e}")
    assert abs(got['average_precision'] - host['average_precision']) <= ap_bound
    assert abs(got['average_precision'] - S.average_precision(score, label)) <= S.sum_bound(want[6], S.E_AP)
    _within('binary_crossentropy', got['binary_crossentropy'], host['binary_crossentropy'], S.sum_bound(n, S.E_BCE))
    # where AUC is nan, average precision is: no positive, a NaN, an Inf; with positives only it is 1.0
    yd, pd_ = _dev(np.zeros(n, np.float32), dev), _dev(p, dev)
    r = metrics.compute_metrics_device(['pr_auc', 'precision', 'recall'], yd, pd_, 'binary')
    assert math.isnan(r['pr_auc']) and r['precision'] == 0.0 and r['recall'] == 0.0
    r = metrics.compute_metrics_device(['pr_auc', 'AUC'], _dev(np.ones(n, np.float32), dev), pd_, 'binary')
    assert abs(r['pr_auc'] - 1.0) <= S.sum_bound(n, S.E_AP) and math.isnan(r['AUC'])
    for bad in (np.nan, np.inf):
        s = np.array(p)
        s[n // 2] = bad
        r = metrics.compute_metrics_device(['average_precision'], _dev(label, dev), _dev(s, dev), 'binary')
        assert math.isnan(r['average_precision']) and math.isnan(metrics.compute_metric('average_precision', label, s, 'binary'))
    # labels 2 and 0.5: average precision is the host's value, precision counts them positive
    for other in (2.0, 0.5):
        y2 = np.array(label)
        y2[y2 == 1] = other
        r = metrics.compute_metrics_device(['average_precision', 'precision'], _dev(y2, dev), pd_, 'binary')
        h = metrics.compute_metric('average_precision', y2, p, 'binary')
        assert (math.isnan(h) and math.isnan(r['average_precision'])) or r['average_precision'] == h
        assert r['precision'] == got['Precision']


@pytest.mark.parametrize('form', ['labels', 'onehot'])
def test_compute_metrics_device_multiclass_set(dev, monkeypatch, form):
    n, C = 3001, 7
    p, labels, onehot, want = _rows_case(n, C, _lib().DT_SCORE_THREAD_ROW_MAX_C)
    if form == 'onehot':
        onehot = np.eye(C, dtype=np.float32)[labels.astype(np.int64)]       # (accuracy's argmax and the scan agree on these)
    y = labels if form == 'labels' else onehot
    names = ['accuracy', 'categorical_crossentropy', 'top_k_categorical_accuracy', 'precision', 'recall', 'logloss']
    got, host = _device_and_host(names, y, p, 'multiclass', dev, monkeypatch)
    for k in ('accuracy', 'top_k_categorical_accuracy', 'precision', 'recall'):
        assert got[k] == host[k], k
    assert got['top_k_categorical_accuracy'] == S.categorical_words(p, y, K, 32)[0] / n
    assert got['logloss'] == got['categorical_crossentropy']
    _within('categorical_crossentropy', got['categorical_crossentropy'], host['categorical_crossentropy'], S.sum_bound(n + C, S.E_CCE))


def test_compute_metrics_device_regression_set(dev, monkeypatch):
    n = 5003
    y, p, (sl, pe, kappa) = _regression_case('positive', n)
    got, host = _device_and_host(['mse', 'msle', 'mape', 'mae'], y, p.reshape(-1, 1), 'regression', dev, monkeypatch)
    _within('mape', got['mape'], host['mape'], S.sum_bound(n, S.E_MAPE) + S.U)
    print(f"msle: device {got['msle']!r} host {host['msle']!r} bound {S.msle_bound(n, sl, kappa) / n:.3e}")
    assert abs(got['msle'] - host['msle']) <= S.msle_bound(n, sl, kappa) / n + 2 * S.U * host['msle']
    assert abs(got['mse'] - host['mse']) <= 1e-6 * host['mse']          # (the host's mse is a float32 mean)


# ---- end to end ------------------------------------------------------------------------------------------------------------
F, ND, D, V, ROWS = 5, 3, 8, 20, 400
TASKS = {
    'binary': (2, ['AUC', 'binary_crossentropy', 'Precision', 'Recall', 'average_precision', 'logloss']),
    'multiclass': (3, ['accuracy', 'categorical_crossentropy', 'top_k_categorical_accuracy', 'precision', 'recall', 'log_loss']),
    'multilabel': (3, ['binary_crossentropy', 'precision', 'recall']),
    'regression': (1, ['mse', 'msle', 'mape']),
}
EXACT = {'precision', 'recall', 'top_k_categorical_accuracy', 'accuracy'}


def _frame(task):
    rng = np.random.RandomState(11)
    df = pd.DataFrame({f'C{i}': rng.randint(0, V + i, ROWS) for i in range(F)})
    for j in range(ND):
        df[f'I{j}'] = rng.randn(ROWS).astype(np.float32)
    if task == 'binary':
        y = (rng.rand(ROWS) < 0.3).astype(np.float32)
    elif task == 'multiclass':
        y = rng.randint(0, 3, ROWS)
    elif task == 'multilabel':
        y = (rng.rand(ROWS, 3) < 0.4).astype(np.float32)
    else:
        y = np.exp(0.5 * rng.randn(ROWS)).astype(np.float32)
    return df, y


def _model(task, num_classes, metrics):
    from deeptables_amd import functional
    from deeptables_amd.models import ModelConfig, DeepModel
    from deeptables_amd.models.metainfo import CategoricalColumn, ContinuousColumn
    functional.set_seed(4)
    conf = ModelConfig(nets=['linear', 'dnn_nets'], fixed_embedding_dim=True, embeddings_output_dim=D, embedding_dropout=0,
                       metrics=metrics)
    cats = [CategoricalColumn(f'C{i}', V + i, D) for i in range(F)]
    conts = [ContinuousColumn('input_continuous_all', [f'I{j}' for j in range(ND)])]
    dm = DeepModel(task, num_classes, conf, cats, conts)
    dm.build()
    return dm


@pytest.mark.parametrize('task', list(TASKS))
def test_fit_and_evaluate_report_the_new_metrics(dev, monkeypatch, task):
    """fit(metrics=['AUC', 'binary_crossentropy', 'Precision', 'Recall']) raised 'Unsupported metric' before these kernels"""
    from deeptables_amd import metrics
    num_classes, names = TASKS[task]
    df, y = _frame(task)
    dm = _model(task, num_classes, names)
    with monkeypatch.context() as mp:
        mp.setattr(metrics, 'compute_metric', lambda *a, **k: pytest.fail('the host metric path was taken'))
        hist = dm.fit(df, y, batch_size=64, epochs=2, verbose=0, validation_split=0.2)
        on = dm.evaluate(df, y, batch_size=64)
    for k in names:
        for key in (k, 'val_' + k):
            assert key in hist.history and len(hist.history[key]) == 2 and all(np.isfinite(hist.history[key])), (key, hist.history)
        assert k in on
    monkeypatch.setenv('DT_AMD_DEVICE_METRICS', '0')
    off = dm.evaluate(df, y, batch_size=64)
    n_out = ROWS * (num_classes if task == 'multilabel' else 1)
    # T and e of each sum as in the kernel tests above: the elements (log loss), the rows + classes (categorical
    # cross-entropy), the groups, at most the rows (average precision), the rows (MAPE)
    rel = {'bce': S.sum_bound(n_out, S.E_BCE), 'cce': S.sum_bound(ROWS + num_classes, S.E_CCE),
           'ap': S.sum_bound(ROWS, S.E_AP), 'mape': S.sum_bound(ROWS, S.E_MAPE)}
    for k in names:
        kind = metrics.score_kind(k.lower(), task)
        print(f'{task} {k}: device {on[k]!r} host {off[k]!r}')
        if k.lower() in EXACT:
            assert on[k] == off[k], k
        elif k == 'AUC':
            assert abs(on[k] - off[k]) <= 1e-12, k
        elif k == 'mse':
            assert abs(on[k] - off[k]) <= 1e-6 * abs(off[k]), k          # (the host's mse is a float32 mean)
        elif kind == 'msle':         # differences of logarithms: the cancellation weight of msle_bound from the outputs themselves
            pred = dm.predict(df, batch_size=64)
            sl, _, kappa = S.regression_sums(y, pred)
            assert abs(on[k] - off[k]) <= S.msle_bound(ROWS, sl, kappa) / ROWS + 2 * S.U * off[k], k
        else:                        # (sklearn's own arithmetic is held to the reference at 1e-12 in test_scores_host.py)
            assert abs(on[k] - off[k]) <= (rel[kind] + 2 * S.U) * abs(off[k]) + (1e-12 if kind == 'ap' else 0.0), k


def test_deeptable_fit_reports_log_loss_and_precision(dev):
    from deeptables_amd.models import DeepTable, ModelConfig
    rng = np.random.default_rng(0)
    n = 600
    df = pd.DataFrame({'job': rng.choice(['admin', 'tech', 'services', 'retired'], n), 'marital': rng.choice(['m', 's', 'd'], n),
                       'age': rng.integers(18, 80, n).astype(np.float32), 'balance': rng.normal(1000, 500, n).astype(np.float32)})
    y = ((df['age'] > 50) ^ (df['job'] == 'tech')).map({True: 'yes', False: 'no'})
    names = ['AUC', 'logloss', 'Precision', 'Recall', 'pr_auc']
    conf = ModelConfig(nets=['linear', 'fm_nets'], metrics=names, embedding_dropout=0, earlystopping_patience=0)
    dt = DeepTable(config=conf)
    _, history = dt.fit(df, y, batch_size=128, epochs=2, verbose=0)
    res = dt.evaluate(df, y)
    for k in names:
        assert k in res and math.isfinite(res[k]) and 'val_' + k in history.history, (k, res)
    assert 0.0 <= res['Precision'] <= 1.0 and res['logloss'] > 0.0
