# -*- coding:utf-8 -*-
"""CPU: the device metrics' reference (tests/metrics_reference.py) against a brute-force pair count and sklearn, the C-ABI
surface and argument checks of the dt_metric_* entry points (no launch), and the routing of metrics.epoch_metrics."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import metrics_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {'dt_metric_sort_tile', 'dt_metric_sort_workspace_bytes', 'dt_metric_sort_pairs', 'dt_metric_auc_workspace_bytes',
           'dt_metric_auc', 'dt_metric_sums', 'dt_metric_argmax_hits'}
DENORMAL = np.float32(1e-45)
FMAX = np.finfo(np.float32).max


# ---- the reference ---------------------------------------------------------------------------------------------------------
def _tie_heavy(n, seed):
    """heavy ties, -0.0 / +0.0 pairs, denormals of both signs and negative scores"""
    rng = np.random.default_rng(seed)
    pool = np.array([-3.5, -1.0, -0.0, 0.0, -DENORMAL, DENORMAL, 2 * DENORMAL, 0.25, 0.25, 1.0, -FMAX, FMAX], dtype=np.float32)
    score = pool[rng.integers(0, len(pool), n)]
    label = (rng.random(n) < 0.4).astype(np.float32)
    return score, label


@pytest.mark.parametrize('n,seed', [(1, 0), (2, 1), (17, 2), (100, 3), (300, 4), (300, 5)])
def test_reference_equals_the_brute_force_pair_count(n, seed):
    score, label = _tie_heavy(n, seed)
    u2, P, N, nonfinite, bad = R.auc_words(score, label)
    assert (P, N, nonfinite, bad) == (int((label == 1).sum()), int((label == 0).sum()), 0, 0)
    assert u2 == R.brute_force_u2(score, label)
    assert R.auc_words_fast(score, label) == (u2, P, N, nonfinite, bad)


def test_reference_ties_of_signed_zeros_count_one_half():
    # a positive at -0.0 against a negative at +0.0 (and the reverse): a tie either way, U2 = 1 per pair
    score = np.array([-0.0, 0.0, 0.0, -0.0], dtype=np.float32)
    label = np.array([1, 0, 1, 0], dtype=np.float32)
    assert R.auc_words(score, label)[0] == 4 == R.brute_force_u2(score, label)
    assert R.auc(score, label) == 0.5


def test_reference_counts_nonfinite_scores_and_bad_labels():
    score = np.array([0.1, np.nan, np.inf, -np.inf, 0.3], dtype=np.float32)
    label = np.array([0, 1, 2, 0.5, np.nan], dtype=np.float32)
    assert R.auc_words(score, label)[1:] == (1, 4, 3, 3)
    assert np.isnan(R.auc(score, label))
    assert np.isnan(R.auc(np.array([0.1, 0.2], dtype=np.float32), np.ones(2, dtype=np.float32)))
    assert np.isnan(R.auc(np.array([0.1, 0.2], dtype=np.float32), np.zeros(2, dtype=np.float32)))


def test_reference_agrees_with_sklearn_at_a_million_rows():
    from sklearn.metrics import roc_auc_score
    rng = np.random.default_rng(20)
    n = 1 << 20
    label = (rng.random(n) < 0.03).astype(np.float32)
    score = (1 / (1 + np.exp(-(rng.standard_normal(n) + 0.8 * label - 2)))).astype(np.float32)
    got, want = R.auc(score, label), float(roc_auc_score(label, score))
    print('reference - roc_auc_score =', got - want)
    assert abs(got - want) <= 1e-12


def test_key_transform_is_strictly_order_preserving():
    ladder = np.array([-FMAX, -1.0, -DENORMAL, 0.0, DENORMAL, 1.0, FMAX], dtype=np.float32)
    keys = R.score_keys(ladder).astype(np.int64)
    assert np.all(np.diff(keys) > 0), keys
    assert R.score_keys(np.array([-0.0], dtype=np.float32))[0] == R.score_keys(np.array([0.0], dtype=np.float32))[0]
    rng = np.random.default_rng(3)
    x = rng.standard_normal(4096).astype(np.float32) * np.float32(10.0) ** rng.integers(-40, 38, 4096).astype(np.float32)
    k = R.score_keys(x)
    order = np.argsort(k, kind='stable')
    assert np.all(np.diff(x[order]) >= 0)
    assert np.array_equal(x[:-1] < x[1:], k[:-1] < k[1:])


# ---- the C-ABI surface -----------------------------------------------------------------------------------------------------
def test_header_exports_and_binding_name_the_same_metric_entry_points():
    from deeptables_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'dt_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(dt_metric_[a-z0-9_]+)\s*\(', text))
    assert declared == ENTRIES == {n for n in _lib.SIGNATURES if n.startswith('dt_metric_')}
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for n in ENTRIES:
        assert hasattr(handle, n), n
    assert _lib.DT_METRIC_SUMS_WORDS == 3 + 3 * _lib.DT_METRIC_SUMS_BLOCKS


def test_entry_points_refuse_bad_arguments_before_any_launch():
    from deeptables_amd import _lib
    h = _lib.lib()
    A, ODD = 0x10000, 0x10002            # never dereferenced: every call below is refused, or is the n == 0 no-op
    big = 1 << 31

    def refused(rc, *words):
        assert rc == -1
        msg = h.dt_last_error().decode()
        assert all(w in msg for w in words), msg

    T = h.dt_metric_sort_tile()
    assert T > 0 and T % 64 == 0
    # sort
    refused(h.dt_metric_sort_pairs(A, A, -1, A, A, A, None), 'dt_metric_sort_pairs', '2^31')
    refused(h.dt_metric_sort_pairs(A, A, big, A, A, A, None), 'dt_metric_sort_pairs', '2^31')
    for bad in range(4):
        args = [A, A, A, A]
        args[bad] = None
        refused(h.dt_metric_sort_pairs(args[0], args[1], 5, args[2], args[3], A, None), 'dt_metric_sort_pairs', 'null pointer')
        args[bad] = ODD
        refused(h.dt_metric_sort_pairs(args[0], args[1], 5, args[2], args[3], A, None), 'dt_metric_sort_pairs', 'aligned')
    refused(h.dt_metric_sort_pairs(A, A, 5, A, A, None, None), 'dt_metric_sort_pairs', 'null workspace')
    refused(h.dt_metric_sort_pairs(A, A, 5, A, A, A + 8, None), 'dt_metric_sort_pairs', 'workspace', 'aligned')
    assert h.dt_metric_sort_pairs(None, None, 0, None, None, None, None) == 0
    # auc
    refused(h.dt_metric_auc(A, A, -1, A, A, None), 'dt_metric_auc', '2^31')
    refused(h.dt_metric_auc(A, A, big, A, A, None), 'dt_metric_auc', '2^31')
    refused(h.dt_metric_auc(None, A, 5, A, A, None), 'dt_metric_auc', 'null pointer')
    refused(h.dt_metric_auc(A, None, 5, A, A, None), 'dt_metric_auc', 'null pointer')
    refused(h.dt_metric_auc(A, A, 5, A, None, None), 'dt_metric_auc', 'null pointer')
    refused(h.dt_metric_auc(A, A, 5, None, A, None), 'dt_metric_auc', 'null workspace')
    refused(h.dt_metric_auc(ODD, A, 5, A, A, None), 'dt_metric_auc', 'aligned')
    refused(h.dt_metric_auc(A, ODD, 5, A, A, None), 'dt_metric_auc', 'aligned')
    refused(h.dt_metric_auc(A, A, 5, A, A + 4, None), 'dt_metric_auc', 'out5', 'aligned')
    refused(h.dt_metric_auc(A, A, 5, A + 4, A, None), 'dt_metric_auc', 'workspace', 'aligned')
    assert h.dt_metric_auc(None, None, 0, None, None, None) == 0
    # sums
    refused(h.dt_metric_sums(A, A, -1, A, None), 'dt_metric_sums', '2^31')
    refused(h.dt_metric_sums(A, A, big, A, None), 'dt_metric_sums', '2^31')
    refused(h.dt_metric_sums(None, A, 5, A, None), 'dt_metric_sums', 'null pointer')
    refused(h.dt_metric_sums(A, None, 5, A, None), 'dt_metric_sums', 'null pointer')
    refused(h.dt_metric_sums(A, A, 5, None, None), 'dt_metric_sums', 'null pointer')
    refused(h.dt_metric_sums(ODD, A, 5, A, None), 'dt_metric_sums', 'aligned')
    refused(h.dt_metric_sums(A, A, 5, A + 4, None), 'dt_metric_sums', 'out', 'aligned')
    assert h.dt_metric_sums(None, None, 0, None, None) == 0
    # argmax hits
    refused(h.dt_metric_argmax_hits(A, A, 0, -1, 3, A, None), 'dt_metric_argmax_hits', '2^31')
    refused(h.dt_metric_argmax_hits(A, A, 0, big, 3, A, None), 'dt_metric_argmax_hits', '2^31')
    refused(h.dt_metric_argmax_hits(A, A, 0, 5, 1, A, None), 'dt_metric_argmax_hits', 'C = 1')
    refused(h.dt_metric_argmax_hits(A, A, 0, 0, 1, A, None), 'dt_metric_argmax_hits', 'C = 1')
    refused(h.dt_metric_argmax_hits(A, A, 7, 5, 3, A, None), 'dt_metric_argmax_hits', 'y_kind')
    refused(h.dt_metric_argmax_hits(None, A, 0, 5, 3, A, None), 'dt_metric_argmax_hits', 'null pointer')
    refused(h.dt_metric_argmax_hits(A, None, 1, 5, 3, A, None), 'dt_metric_argmax_hits', 'null pointer')
    refused(h.dt_metric_argmax_hits(A, A, 1, 5, 3, None, None), 'dt_metric_argmax_hits', 'null pointer')
    refused(h.dt_metric_argmax_hits(A, ODD, 1, 5, 3, A, None), 'dt_metric_argmax_hits', 'aligned')
    refused(h.dt_metric_argmax_hits(A, A, 1, 5, 3, A + 4, None), 'dt_metric_argmax_hits', 'out', 'aligned')
    assert h.dt_metric_argmax_hits(None, None, 0, 0, 3, None, None) == 0


def test_workspace_queries_are_monotone_and_refuse_sizes_outside_the_domain():
    from deeptables_amd import _lib
    h = _lib.lib()
    T = h.dt_metric_sort_tile()
    sizes = [0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17, (1 << 20) + 77, 8192 * 1024, (1 << 31) - 1]
    for query in (h.dt_metric_sort_workspace_bytes, h.dt_metric_auc_workspace_bytes):
        got = [query(n) for n in sizes]
        assert all(b > 0 for b in got) and got == sorted(got), got
        assert got[-1] >= 2 * 4 * sizes[-1]              # at least the second buffer of keys and values
        assert query(-1) == -1 and b'2^31' in h.dt_last_error()
        assert query(1 << 31) == -1 and b'2^31' in h.dt_last_error()
    assert all(h.dt_metric_auc_workspace_bytes(n) > h.dt_metric_sort_workspace_bytes(n) for n in sizes)


# ---- routing ---------------------------------------------------------------------------------------------------------------
class _FakeCuda:
    """a CPU tensor that says it lives on the GPU: routing looks at is_cuda, dtype and shapes only"""

    def __init__(self, t):
        self.t = t
        self.is_cuda, self.dtype, self.shape = True, t.dtype, t.shape

    def numel(self):
        return self.t.numel()

    def dim(self):
        return self.t.dim()

    def cpu(self):
        return self.t


@pytest.fixture
def host_calls(monkeypatch):
    from deeptables_amd import metrics
    calls = []

    def fake(m, y_true, y_prob, task):
        assert isinstance(y_true, np.ndarray) and isinstance(y_prob, np.ndarray)
        calls.append(metrics.metric_name(m))
        return 0.25

    monkeypatch.setattr(metrics, 'compute_metric', fake)
    monkeypatch.setattr(metrics, 'compute_metrics_device', lambda *a, **k: pytest.fail('device path taken'))
    monkeypatch.setattr(torch, 'is_tensor', lambda t: isinstance(t, (torch.Tensor, _FakeCuda)))
    monkeypatch.delenv('DT_AMD_DEVICE_METRICS', raising=False)
    return calls


def test_routing_takes_the_host_path_for_cpu_tensors(host_calls):
    from deeptables_amd import metrics
    y, p = torch.tensor([0., 1, 1, 0]), torch.tensor([[.2], [.7], [.6], [.4]])
    assert not metrics.device_metrics_supported(['AUC'], y, p, 'binary')
    assert metrics.epoch_metrics(['AUC', 'accuracy'], y, p, 'binary') == {'AUC': 0.25, 'accuracy': 0.25}
    assert host_calls == ['AUC', 'accuracy']


def test_routing_takes_the_host_path_when_switched_off(host_calls, monkeypatch):
    from deeptables_amd import metrics
    y, p = _FakeCuda(torch.tensor([0., 1, 1, 0])), _FakeCuda(torch.tensor([[.2], [.7], [.6], [.4]]))
    assert metrics.device_metrics_supported(['AUC', 'acc', 'mse', 'RMSE', 'mae'], y, p, 'binary')   # (the tensors qualify)
    monkeypatch.setenv('DT_AMD_DEVICE_METRICS', '0')
    assert not metrics.device_metrics_supported(['AUC'], y, p, 'binary')
    assert metrics.epoch_metrics(['AUC'], y, p, 'binary') == {'AUC': 0.25}
    assert host_calls == ['AUC']


def test_routing_takes_the_host_path_for_a_callable_metric(host_calls):
    from deeptables_amd import metrics

    def my_metric(y_true, y_prob):
        return 1.0

    y, p = _FakeCuda(torch.tensor([0., 1, 1, 0])), _FakeCuda(torch.tensor([[.2], [.7], [.6], [.4]]))
    assert not metrics.device_metrics_supported(['AUC', my_metric], y, p, 'binary')
    assert metrics.epoch_metrics(['AUC', my_metric], y, p, 'binary') == {'AUC': 0.25, 'my_metric': 0.25}
    assert host_calls == ['AUC', 'my_metric']


def test_routing_takes_the_host_path_for_multiclass_auc(host_calls):
    from deeptables_amd import metrics
    p = _FakeCuda(torch.tensor([[.2, .5, .3], [.7, .2, .1], [.1, .1, .8], [.3, .4, .3]]))
    y = _FakeCuda(torch.eye(3)[[1, 0, 2, 1]])
    assert metrics.device_metrics_supported(['accuracy'], y, p, 'multiclass')
    assert metrics.device_metrics_supported(['accuracy'], _FakeCuda(torch.tensor([1., 0, 2, 1])), p, 'multiclass')
    assert not metrics.device_metrics_supported(['AUC'], y, p, 'multiclass')
    assert metrics.epoch_metrics(['AUC', 'accuracy'], y, p, 'multiclass') == {'AUC': 0.25, 'accuracy': 0.25}
    assert host_calls == ['AUC', 'accuracy']


def test_routing_keeps_other_dtypes_and_no_metrics_on_the_host(host_calls):
    from deeptables_amd import metrics
    y, p = _FakeCuda(torch.tensor([0., 1, 1, 0]).double()), _FakeCuda(torch.tensor([[.2], [.7], [.6], [.4]]))
    assert not metrics.device_metrics_supported(['mse'], y, p, 'regression')
    assert metrics.epoch_metrics([], y, p, 'regression') == {} and host_calls == []


def test_an_unknown_metric_name_still_raises():
    from deeptables_amd import metrics
    y, p = torch.tensor([0., 1, 1, 0]), torch.tensor([[.2], [.7], [.6], [.4]])
    with pytest.raises(ValueError, match='Unsupported metric'):
        metrics.epoch_metrics(['AUC', 'f1'], y, p, 'binary')
    with pytest.raises(ValueError, match='Unsupported metric'):
        metrics.compute_metric('f1', y.numpy(), p.numpy(), 'binary')
    yc, pc = _FakeCuda(y), _FakeCuda(p)
    assert not metrics.device_metrics_supported(['f1'], yc, pc, 'binary')


def test_host_path_values_are_unchanged():
    """epoch_metrics on CPU tensors is compute_metric on their arrays, value for value"""
    from deeptables_amd import metrics
    rng = np.random.default_rng(5)
    y = (rng.random(500) < 0.3).astype(np.float32)
    p = rng.random((500, 1)).astype(np.float32)
    names = ['AUC', 'accuracy', 'mse', 'rmse', 'mae']
    got = metrics.epoch_metrics(names, torch.from_numpy(y), torch.from_numpy(p), 'binary')
    assert got == {m: metrics.compute_metric(m, y, p, 'binary') for m in names}
    assert abs(got['AUC'] - R.auc(p, y)) <= 1e-12
