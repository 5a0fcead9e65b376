# -*- coding:utf-8 -*-
"""GPU: the column profile kernels (csrc/prep_fit.hip) against numpy / pandas / math.fsum, and DefaultPreprocessor.fit_feed against
the host fit.  Equality everywhere but the sum, which is held to the bound of any summation order."""
import math
import pickle

import numpy as np
import pandas as pd
import pytest
import torch

from tests import device_transform_support as S
from tests import prep_fit_support as P

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CAP = 4
DTYPES = ['bool', 'int8', 'uint8', 'int32', 'int64', 'float32', 'float64']
SIZES = [1, 2, 255, 257, 65537, 3 * 4096 + 1234]
FLOAT_ONLY = ('all_nan', 'half_nan', 'zeros', 'inf_denormal')
PATTERNS = ('equal', 'distinct', 'extremes', 'ties', 'at_cap', 'above_cap') + FLOAT_ONLY


def ordered(a):
    """the order-mapped keys of the issue's definition, written out independently of ops.profile_keys"""
    if a.dtype == np.bool_:
        return a.astype(np.uint64)
    w = a.dtype.itemsize
    bits = a.view(f'u{w}').astype(np.uint64)
    top, full = np.uint64(1 << (8 * w - 1)), np.uint64((1 << (8 * w)) - 1)
    if a.dtype.kind == 'u':
        return bits
    if a.dtype.kind == 'i':
        return bits ^ top
    k = np.where(bits & top != 0, bits ^ full, bits | top)
    k[np.isnan(a)] = 0xFFC00000 if w == 4 else 0xFFF8000000000000
    return k


def column(pattern, dtype, N, rng):
    dt = np.dtype(dtype)
    i = rng.permutation(N)
    if dt.kind == 'f':
        info = np.finfo(dt)
        base = {'equal': np.full(N, 3.5), 'distinct': i - N / 2 + 0.25, 'ties': np.array([-1.5, 0.0, 7.0])[i % 3],
                'extremes': np.array([info.max / 2 ** 20, -info.max / 2 ** 20, 1.0])[i % 3], 'at_cap': (i % CAP) / 8, 'above_cap': (i % (CAP + 1)) / 8,
                'all_nan': np.full(N, np.nan), 'half_nan': np.where(i % 2 == 0, np.nan, i / 8),
                'zeros': np.array([0.0, -0.0, 1.0, -0.0, 0.0])[i % 5],
                'inf_denormal': np.array([np.inf, -np.inf, info.smallest_subnormal, -info.smallest_subnormal, info.tiny, 0.0])[i % 6]}
        return base[pattern].astype(dt)
    if dt == np.bool_:
        return {'equal': np.ones(N, bool)}.get(pattern, i % 2 == 0)
    info = np.iinfo(dt)
    base = {'equal': np.full(N, 3), 'distinct': i - (N // 2 if info.min < 0 else 0), 'ties': np.array([info.min, 0, 7])[i % 3],
            'extremes': np.array([info.min, info.max, info.max - 1, info.min + 1], dtype=dt)[i % 4], 'at_cap': i % CAP,
            'above_cap': i % (CAP + 1)}
    return base[pattern].astype(dt)                 # (a narrow dtype wraps: as many distinct values as it has)


def check_column(prof, c, a, fill):
    from deeptables_amd import ops
    N, k = len(a), ordered(a)
    nan = np.isnan(a) if a.dtype.kind == 'f' else np.zeros(N, bool)
    got_sorted = prof.sorted_keys(c).cpu().numpy().view(np.uint64)
    assert np.array_equal(got_sorted, np.sort(k))
    assert np.array_equal(ops.profile_values(got_sorted[:N - nan.sum()], a.dtype), np.sort(a[~nan]))
    uniq, counts = np.unique(k[~nan], return_counts=True)
    assert (prof.n_distinct[c], prof.nan_count[c]) == (len(uniq), nan.sum())
    assert prof.nunique[c] == pd.Series(a).nunique()
    if len(uniq) <= CAP:
        values, got_counts = prof.distinct(c)
        assert values.dtype == a.dtype and np.array_equal(ordered(values), uniq) and np.array_equal(got_counts, counts)
    else:
        assert prof.distinct(c) is None
    x = a[~nan].astype(np.float64)
    if len(x):
        assert prof.minimum(c) == a[~nan].min() and prof.maximum(c) == a[~nan].max()
    else:
        assert prof.minimum(c) is None and prof.maximum(c) is None
    if np.isfinite(x).all():
        bound = max(len(x) - 1, 0) * 2.0 ** -53 * math.fsum(np.abs(x))
        assert abs(prof.sums[c] - math.fsum(x)) <= bound
    else:
        with np.errstate(invalid='ignore'):
            assert np.array_equal(prof.sums[c], np.sum(x), equal_nan=True)
    # ranks 0, the last one, and both sides of the block of fills
    virtual = np.sort(np.where(nan, fill, a.astype(np.float64)))
    lo = int(np.searchsorted(np.sort(x), fill, side='left'))
    ranks = np.clip([0, N - 1, lo - 1, lo, lo + nan.sum() - 1, lo + nan.sum()], 0, N - 1)
    return ranks, virtual[ranks]


@pytest.mark.parametrize('N', SIZES)
@pytest.mark.parametrize('pattern', PATTERNS)
def test_column_profile_against_numpy(pattern, N):
    from deeptables_amd import ops
    rng = np.random.default_rng(N)
    dtypes = [d for d in DTYPES if pattern not in FLOAT_ONLY or d.startswith('float')]
    cols = [column(pattern, d, N, rng) for d in dtypes]          # several dtypes in one call: the segmentation
    prof = ops.column_profile([torch.from_numpy(a).to(DEV) for a in cols], cap=CAP)
    assert prof.dtypes == dtypes
    with np.errstate(invalid='ignore'):
        fills = [0.125 if np.isnan(a.astype(np.float64)).all() else float(np.nanmean(a.astype(np.float64))) for a in cols]
    fills = [f if np.isfinite(f) else 0.0 for f in fills]
    want = [check_column(prof, c, a, fills[c]) for c, a in enumerate(cols)]
    got = prof.order_stats([r for r, _ in want], fills)
    for c, (_, values) in enumerate(want):
        assert np.array_equal(got[c], values), (dtypes[c], got[c], values)
    # a narrow dtype does not pay eight digit passes
    for c, d in enumerate(dtypes):
        assert prof.passes[c] <= np.dtype(d).itemsize and (pattern != 'equal' or prof.passes[c] == 0)


def test_two_calls_give_identical_bits():
    from deeptables_amd import ops
    rng = np.random.default_rng(5)
    cols = [torch.from_numpy(rng.standard_normal(65537).astype(d)).to(DEV) for d in ('float32', 'float64')]
    a, b = ops.column_profile(cols, cap=CAP), ops.column_profile(cols, cap=CAP)
    assert np.array_equal(a.host(), b.host())
    assert all(torch.equal(a.sorted_keys(c), b.sorted_keys(c)) for c in range(2))
    ranks = [[0, 1000, 65536]] * 2
    assert np.array_equal(a.order_stats(ranks, [0.0, 0.0]), b.order_stats(ranks, [0.0, 0.0]))


# ---- fit_feed against fit_transform -------------------------------------------------------------------------------------------
def feeds_equal(a, b):
    return len(a.blocks) == len(b.blocks) and all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a.blocks, b.blocks)) \
        and torch.equal(a.y, b.y)


@pytest.mark.parametrize('config', sorted(S.numeric_configs()))
@pytest.mark.parametrize('frame', ['plain', 'host_columns'])
def test_fit_feed_equals_fit_transform_on_dyadic_frames(frame, config):
    from deeptables_amd import training
    from deeptables_amd.models.preprocessor import DefaultPreprocessor
    X, y, extra = P.dyadic_frame(with_host_columns=frame == 'host_columns')
    conf = P.config_of(S.numeric_configs()[config], extra)
    host, dev = DefaultPreprocessor(conf), DefaultPreprocessor(conf)
    Xt, yt = host.fit_transform(X, y)
    want = training.TableBatches(Xt, yt, host.categorical_columns, host.continuous_columns, DEV, host.task_, len(host.labels_) or 1,
                                 cat_dtype=torch.int32, var_len_categorical_columns=host.var_len_categorical_columns)
    feed = dev.fit_feed(X, y, device=DEV, mode=True)
    assert feed.fit_path == 'device' and feed.fit_refusal is None
    assert P.fitted_state(dev) == P.fitted_state(host)
    assert feeds_equal(feed, want)
    again = pickle.loads(pickle.dumps(dev))
    assert feeds_equal(again.transform_feed(X, y, device=DEV), want)
    assert again.transform_X(X).equals(host.transform_X(X))


def test_fit_feed_on_general_data():
    from deeptables_amd.models.preprocessor import DefaultPreprocessor
    from deeptables_amd.models import ModelConfig
    X, y = P.random_frame()
    conf = ModelConfig(metrics=['AUC'], apply_gbm_features=False)
    host, dev = DefaultPreprocessor(conf), DefaultPreprocessor(conf)
    host.fit_transform(X, y)
    feed = dev.fit_feed(X, y, device=DEV, mode=True)
    loose = ('means_', 'range_', 'edges_')
    assert P.fitted_state(dev, skip=loose) == P.fitted_state(host, skip=loose)
    for c, mean in dev.X_transformers['imputation'].means_.items():
        x = X[c].values[~np.isnan(X[c].values)].astype(np.float64)
        exact = math.fsum(x) / len(x)
        bound = (len(x) - 1) * 2.0 ** -53 * math.fsum(np.abs(x)) / len(x) + abs(exact) * 2.0 ** -53
        if X[c].dtype == np.float32:
            bound += abs(exact) * 2.0 ** -24              # the mean of a float32 column is rounded to float32
        assert abs(mean - exact) <= bound, c
    assert feeds_equal(feed, dev.transform_feed(X, y, device=DEV, mode=True))


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_fit_feed_refusals(monkeypatch):
    from deeptables_amd.models import ModelConfig
    from deeptables_amd.models.preprocessor import DefaultPreprocessor
    X, y, _ = P.dyadic_frame(with_host_columns=False)
    conf = ModelConfig(metrics=['AUC'], apply_gbm_features=False)
    host = DefaultPreprocessor(conf)
    host.fit_transform(X, y)
    with pytest.raises(ValueError, match='not a GPU'):
        DefaultPreprocessor(conf).fit_feed(X, y, device='cpu', mode=True)
    with pytest.raises(ValueError, match='max_resident_bytes'):
        DefaultPreprocessor(conf).fit_feed(X, y, device=DEV, mode=True, max_resident_bytes=1000)
    for env, kw, why in (('1', dict(mode=False), 'mode=False'), ('0', {}, 'DT_AMD_DEVICE_FIT=0'),
                         ('1', dict(max_resident_bytes=1000), 'max_resident_bytes')):
        monkeypatch.setenv('DT_AMD_DEVICE_FIT', env)
        pp = DefaultPreprocessor(conf)
        feed = pp.fit_feed(X, y, device=DEV, **kw)
        assert feed.fit_path == 'host' and why in feed.fit_refusal
        assert P.fitted_state(pp) == P.fitted_state(host)


@pytest.fixture
def rng_left_alone():
    """training draws from the global numpy / torch generators; later tests of the suite see the stream they saw before"""
    saved = np.random.get_state(), torch.get_rng_state(), torch.cuda.get_rng_state(DEV)
    yield
    np.random.set_state(saved[0])
    torch.set_rng_state(saved[1])
    torch.cuda.set_rng_state(saved[2], DEV)


def test_deeptable_fit_feed(tmp_path, rng_left_alone):
    from deeptables_amd.models import DeepTable, ModelConfig
    X, y, _ = P.dyadic_frame(with_host_columns=True)
    X = X.drop(columns=['tags'])
    conf = dict(nets=['dnn_nets'], metrics=['AUC'], apply_gbm_features=False, earlystopping_patience=0)
    a, b = DeepTable(ModelConfig(**conf)), DeepTable(ModelConfig(**conf))
    model_a, history_a = a.fit_feed(X, y, batch_size=64, epochs=1, verbose=0, mode=True)
    model_b, history_b = b.fit(X, y, batch_size=64, epochs=1, verbose=0)
    assert type(model_a) is type(model_b) and set(history_a.history) == set(history_b.history)
    assert a.fit_path == 'device' and P.fitted_state(a.preprocessor) == P.fitted_state(b.preprocessor)
    assert a.leaderboard['model'].tolist() == b.leaderboard['model'].tolist() and a.get_model() is model_a
    proba = a.predict_proba(X)
    assert proba.shape[0] == len(X) and np.isfinite(proba).all()
    assert {'loss', 'auc'} <= {k.lower() for k in a.evaluate(X, y, batch_size=64, verbose=0)}
    a.save(str(tmp_path))
    assert np.array_equal(DeepTable.load(str(tmp_path)).predict_proba(X), proba)
    model_c, history_c = DeepTable(ModelConfig(**conf)).fit_feed(X, y, batch_size=64, verbose=0, validation_data=(X[:50], y[:50]),
                                                                 class_weight={0: 1.0, 1: 2.0})
    assert set(history_c.history) == set(history_b.history)
