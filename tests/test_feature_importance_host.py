# -*- coding:utf-8 -*-
"""CPU: permutation feature importance (deeptables_amd/utils/feature_importance.py) — the preprocessors' column maps, the host
path against the loop written out with the functions the project had before, the feed path on CPU tensors (ops.permute_columns'
torch branch), a planted signal, the refusals and routing, and the argument checks of dt_column_gather / dt_column_swap.

The models run on CPU tensors with torch restatements of the three kernels a ['dnn_nets'] forward launches
(tests/feature_importance_support.py); nothing here launches."""
import ctypes

import numpy as np
import pandas as pd
import pytest
import torch

from deeptables_amd.utils import feature_importance as F
from tests import feature_importance_support as FS


@pytest.fixture(scope='module', autouse=True)
def _cpu_kernels():
    mp = pytest.MonkeyPatch()
    FS.cpu_kernels(mp)
    yield
    mp.undo()


@pytest.fixture(scope='module')
def fitted(_cpu_kernels):
    """one small CPU-trained DeepTable per task, shared (and left unchanged) by the tests below"""
    out = {}
    for task in ('binary', 'multiclass', 'regression'):
        df, y = FS.task_frame(task)
        out[task] = (FS.fit_cpu(df, y, FS.task_config(task), epochs=10), df, y)
    return out


CASES = [('binary', 'auc'), ('binary', 'log_loss'), ('binary', 'accuracy'), ('regression', 'rmse'), ('multiclass', 'accuracy')]


# ---- 1. column map --------------------------------------------------------------------------------------------------------
def _cells(col):
    first = col.iloc[0]
    return np.array(col.tolist()) if isinstance(first, (list, np.ndarray)) else col.values


def _check_column_map(pp, df, perm):
    """for every raw column: transform_X(frame with that column permuted) against transform_X(frame) — of the model's inputs
    exactly the declared columns change, they equal the jointly permuted originals, every other input is unchanged.  (An
    excluded or single-valued column rides along in the transformed frame; the metadata lists it nowhere, the feed never
    reads it, and the map gives it no input.)"""
    smap = pp.source_columns()
    assert set(smap) == set(df.columns)
    base = pp.transform_X(df)
    inputs = pp.get_categorical_columns() + pp.get_var_len_categorical_columns() + pp.get_continuous_columns()
    assert set(inputs) <= set(base.columns)
    for raw in df.columns:
        frame = df.copy()
        frame[raw] = df[raw].values[perm]
        got = pp.transform_X(frame)
        assert list(got.columns) == list(base.columns)
        changed = [c for c in inputs if not np.array_equal(_cells(got[c]), _cells(base[c]), equal_nan=False)]
        assert set(changed) == set(smap[raw]), (raw, changed, smap[raw])
        for c in smap[raw]:
            assert np.array_equal(_cells(got[c]), _cells(base[c])[perm]), (raw, c)
    return smap


def test_default_preprocessor_declares_the_columns_a_raw_column_feeds():
    from deeptables_amd.models.preprocessor import DefaultPreprocessor
    df = FS.mixed_frame(400)
    y = np.random.default_rng(1).integers(0, 2, len(df))
    pp = DefaultPreprocessor(FS.mixed_config())
    pp.fit_transform(df, y)
    perm = torch.randperm(len(df), generator=torch.Generator().manual_seed(5)).numpy()
    smap = _check_column_map(pp, df, perm)
    assert set(smap['c_int']) == {'c_int', 'c_int_cat', 'c_int_discrete'}
    assert smap['const'] == [] and smap['excluded'] == [] and smap['tags'] == ['tags'] and smap['c_str'] == ['c_str']
    assert set(smap['f_nan']) == {'f_nan', 'f_nan_discrete'}
    # the two categorical inputs of c_int are not adjacent in the id block
    cats = pp.get_categorical_columns()
    assert abs(cats.index('c_int_cat') - cats.index('c_int_discrete')) > 1
    listed = set(cats) | set(pp.get_var_len_categorical_columns()) | set(pp.get_continuous_columns())
    assert set(sum(smap.values(), [])) == listed                       # every model input has exactly one source
    assert len(sum(smap.values(), [])) == len(listed)


def test_integer_column_labels_and_the_simple_preprocessor():
    from deeptables_amd.models import ModelConfig
    from deeptables_amd.models.deeptable import SimplePreprocessor
    from deeptables_amd.models.preprocessor import DefaultPreprocessor
    rng = np.random.default_rng(2)
    n = 200
    df = pd.DataFrame(np.stack([rng.normal(size=n), rng.integers(0, 4, n).astype(float), rng.normal(size=n)], 1))
    y = rng.integers(0, 2, n)
    pp = DefaultPreprocessor(ModelConfig(auto_categorize=True, auto_discrete=True))
    pp.fit_transform(df, y)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(6)).numpy()
    smap = _check_column_map(pp, df, perm)
    assert list(smap) == [0, 1, 2] and smap[0] == ['x_0', 'x_0_discrete']
    assert set(smap[1]) == {'x_1', 'x_1_cat', 'x_1_discrete'}
    with pytest.raises(ValueError, match='not fitted'):
        DefaultPreprocessor(ModelConfig()).source_columns()
    df2 = pd.DataFrame({'a': rng.choice(['x', 'y', 'z'], n), 'b': rng.normal(size=n), 'gone': rng.normal(size=n)})
    sp = SimplePreprocessor(ModelConfig(exclude_columns=['gone']))
    sp.fit_transform(df2, y)
    assert sp.source_columns() == {'a': ['a'], 'b': ['b']}
    base = sp.transform_X(df2)
    for raw in ('a', 'b', 'gone'):
        frame = df2.copy()
        frame[raw] = df2[raw].values[perm]
        got = sp.transform_X(frame)
        for c in base.columns:
            want = base[c].values[perm] if c == raw else base[c].values
            assert np.array_equal(got[c].values, want), (raw, c)


# ---- 2. host path against the loop written out --------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['min', 'max'])
@pytest.mark.parametrize('task,metric', CASES)
def test_host_path_is_the_hand_written_loop(fitted, task, metric, mode):
    dt, df, y = fitted[task]
    base, dec = FS.hand_loop(dt, df, y, metric, 2, mode, seed=11)
    res = F.permutation_scores(dt, df, y, metric, n_iter=2, mode=mode, random_state=11)
    assert res['path'] == 'host' and res['columns'] == df.columns.to_list()
    assert res['base_score'] == base and np.array_equal(res['score_decreases'], dec)       # the same arithmetic
    assert res['score_decreases'].dtype == np.float64 and res['score_decreases'].shape == (2, df.shape[1])
    assert np.abs(dec).max() > 0
    # ... and the score is what evaluate reports under that name
    ev = dt.model.evaluate(dt.preprocessor.transform_X(df), dt.preprocessor.transform_y(y), batch_size=128)
    assert abs(abs(base) - ev[metric]) <= FS.metric_bar(metric, len(df), ev[metric])


# ---- 3. the feed path on CPU tensors --------------------------------------------------------------------------------------
def _feed_bits(feed):
    return [b.clone() for b in feed.blocks] + [feed.y.clone()]


def _same_bits(feed, before):
    now = feed.blocks + [feed.y]
    return all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(now, before))


@pytest.mark.parametrize('mode', ['min', 'max'])
@pytest.mark.parametrize('task,metric', CASES)
def test_feed_path_on_cpu_tensors_is_the_host_path(fitted, task, metric, mode):
    dt, df, y = fitted[task]
    sign = -1.0 if mode == 'min' else 1.0
    entries = F._entries(df, None)
    y_enc = dt.preprocessor.transform_y(y)
    host_out, feed_out = [], []
    hb, hd = F.host_scores(dt, df, y_enc, entries, metric, 2, sign, F._generator('cpu', 11), 128,
                           on_pass=lambda i, c, out: host_out.append(np.array(out)))
    feed = F.make_feed(dt, df, y_enc)
    before = _feed_bits(feed)
    fb, fd = F.feed_scores(dt, feed, entries, metric, 2, sign, F._generator('cpu', 11), 128,
                           on_pass=lambda i, c, out: feed_out.append(out.numpy().copy()))
    assert _same_bits(feed, before)
    assert len(host_out) == len(feed_out) == 1 + 2 * df.shape[1]
    for a, b in zip(host_out, feed_out):
        assert np.array_equal(a, b)                                  # the same rows through the same model
    n_out = len(df)
    assert abs(fb - hb) <= FS.metric_bar(metric, n_out, hb)
    for i in range(2):
        for c in range(df.shape[1]):
            assert abs(fd[i, c] - hd[i, c]) <= FS.decrease_tolerance(metric, n_out, hb, hd[i, c]), (i, c, fd[i, c], hd[i, c])


def test_feed_is_restored_when_a_pass_raises(fitted, monkeypatch):
    from deeptables_amd import metrics
    dt, df, y = fitted['binary']
    feed = F.make_feed(dt, df, dt.preprocessor.transform_y(y))
    before = _feed_bits(feed)
    real, calls, seen = metrics.epoch_metrics, [0], []

    def third_pass_raises(metrics, y_true, y_prob, task):
        calls[0] += 1
        if calls[0] == 3:
            seen.append(not _same_bits(feed, before))                 # (the feed IS permuted while the pass runs)
            raise RuntimeError('metric failed')
        return real(metrics, y_true, y_prob, task)

    monkeypatch.setattr(metrics, 'epoch_metrics', third_pass_raises)
    with pytest.raises(RuntimeError, match='metric failed'):
        F.feed_scores(dt, feed, F._entries(df, None), 'auc', 2, 1.0, F._generator('cpu', 3), 128)
    assert seen == [True] and _same_bits(feed, before)


def test_permute_columns_torch_branch_and_runs():
    from deeptables_amd import ops
    assert ops.column_runs([5, 0, 1, 3, 1]) == [(0, 2), (3, 1), (5, 1)]
    g = torch.Generator().manual_seed(0)
    block = torch.randint(0, 100, (37, 6), generator=g, dtype=torch.int32)
    want, perm = block.clone(), torch.randperm(37, generator=g)
    h = ops.permute_columns(block, [4, 0, 1], perm)
    for c in range(6):
        assert torch.equal(block[:, c], want[perm, c] if c in (0, 1, 4) else want[:, c])
    h.restore()
    h.restore()
    assert torch.equal(block, want)
    with pytest.raises(ValueError):
        ops.permute_columns(block, [6], perm)
    with pytest.raises(ValueError):
        ops.permute_columns(block, [0], perm[:-1])
    with pytest.raises(ValueError):
        ops.permute_columns(block, [0], perm.int())


# ---- 4. planted signal ----------------------------------------------------------------------------------------------------
def test_planted_signal_is_ranked_first_and_dead_columns_are_exactly_zero():
    """y = [cat in {a, b}] xor [x > 0]; noise_a / noise_b are pure noise, `excluded` is excluded, `const` is constant.
    Chosen on the CPU: frame seed 0, 600 rows, model seed 3, 30 passes of Adam(0.01), importance seed 1, n_iter 3 — the host
    path then gives both signal columns a mean AUC decrease near 0.5 and the noise columns below 1e-3."""
    from deeptables_amd.models import ModelConfig
    rng = np.random.default_rng(0)
    n = 600
    df = pd.DataFrame({'cat': rng.choice(['a', 'b', 'c', 'd'], n), 'noise_a': rng.integers(0, 5, n).astype(str),
                       'x': rng.normal(size=n), 'noise_b': rng.normal(size=n), 'const': 1.0, 'excluded': rng.normal(size=n)})
    y = (df['cat'].isin(['a', 'b']) ^ (df['x'] > 0)).astype(int).values
    conf = ModelConfig(nets=['dnn_nets'], dnn_params=FS.TOWER, embedding_dropout=0, exclude_columns=['excluded'],
                       earlystopping_patience=0)
    dt = FS.fit_cpu(df, y, conf, epochs=30, seed=3)
    res = F.permutation_scores(dt, df, y, 'auc', n_iter=3, mode='max', random_state=1)
    assert res['path'] == 'host'
    means = dict(zip(res['columns'], res['score_decreases'].mean(0)))
    print('planted signal, mean AUC decrease:', means)
    assert min(means['cat'], means['x']) > max(means['noise_a'], means['noise_b'])
    k = {c: i for i, c in enumerate(res['columns'])}
    assert (res['score_decreases'][:, [k['const'], k['excluded']]] == 0.0).all()
    fi = F.get_score_importances(dt, df, y, 'auc', n_iter=3, mode='max', random_state=1)
    assert fi.shape == (6, 2) and set(fi[:2, 0]) == {'cat', 'x'}
    assert [float(v) for v in fi[:, 1]] == sorted((float(v) for v in fi[:, 1]), reverse=True)
    assert {float(fi[r, 1]) for r in range(6)} == {float(np.float64(v)) for v in means.values()}
    selected, discard = F.select_features(fi, threshold=0.)
    assert {'const', 'excluded'} <= set(discard) and {'cat', 'x'} <= set(selected)
    assert set(selected) | set(discard) == set(df.columns) and not set(selected) & set(discard)


def test_importances_are_ordered_by_value_not_by_their_text(monkeypatch):
    """'9e-05' sorts above '0.3' as text; ties keep the order of `columns`"""
    dec = np.array([[9e-05, 0.3, 0.0, 0.3, -0.2]])
    monkeypatch.setattr(F, 'permutation_scores', lambda *a, **k: {'columns': ['a', 'b', 'c', 'd', 'e'], 'base_score': 0.0,
                                                                  'score_decreases': dec, 'path': 'host'})
    fi = F.get_score_importances(None, None, None, 'auc')
    assert fi[:, 0].tolist() == ['b', 'd', 'a', 'c', 'e'] and [float(v) for v in fi[:, 1]] == [0.3, 0.3, 9e-05, 0.0, -0.2]
    assert fi.dtype.kind == 'U'                                        # numpy.stack of names and means, as the reference's
    assert F.select_features(fi) == (['b', 'd', 'a'], ['c', 'e'])
    assert F.select_features(fi, threshold=0.1) == (['b', 'd'], ['a', 'c', 'e'])
    assert F.select_features(np.array([['a', 'nan']])) == ([], [])


# ---- 5. refusals and routing ------------------------------------------------------------------------------------------------
def test_argument_errors(fitted):
    from deeptables_amd.models import DeepTable
    dt, df, y = fitted['binary']
    with pytest.raises(ValueError, match='Unsupported mode:sideways'):
        F.permutation_scores(dt, df, y, 'auc', mode='sideways')
    with pytest.raises(ValueError, match='Unsupported metric'):
        F.permutation_scores(dt, df, y, 'no_such_metric')
    with pytest.raises(ValueError, match='n_iter'):
        F.permutation_scores(dt, df, y, 'auc', n_iter=0)
    with pytest.raises(ValueError, match='entries for'):
        F.permutation_scores(dt, df, y[:-1], 'auc')
    with pytest.raises(ValueError, match='empty'):
        F.permutation_scores(dt, df.iloc[:0], y[:0], 'auc')
    with pytest.raises(ValueError, match="'nope' is not a column"):
        F.permutation_scores(dt, df, y, 'auc', columns=['age', 'nope'])
    with pytest.raises(ValueError, match="'nope' is not a column"):
        F.permutation_scores(dt, df, y, 'auc', columns=[['age', 'nope']])
    with pytest.raises(ValueError, match='not fitted'):
        F.get_score_importances(DeepTable(config=FS.task_config('binary')), df, y, 'auc')


def test_routing_and_device_refusals(fitted, monkeypatch):
    dt, df, y = fitted['binary']
    kw = dict(n_iter=1, random_state=2, columns=['age'])
    assert F.permutation_scores(dt, df, y, 'auc', device=False, **kw)['path'] == 'host'
    assert F.permutation_scores(dt, df, y, 'auc', **kw)['path'] == 'host'             # 'auto' on a CPU model
    with pytest.raises(ValueError, match='device=True: the model is on cpu, not on a GPU'):
        F.permutation_scores(dt, df, y, 'auc', device=True, **kw)
    # past the device check: every other condition of 'auto', by name
    with monkeypatch.context() as mp:
        mp.setattr(F, 'device_refusal', lambda dt_model, feed=None: None)
        assert F.permutation_scores(dt, df, y, 'auc', **kw)['path'] == 'device'
        assert F.permutation_scores(dt, df, y, 'auc', device=True, **kw)['path'] == 'device'
        mp.setenv('DT_AMD_DEVICE_IMPORTANCE', '0')
        assert F.permutation_scores(dt, df, y, 'auc', **kw)['path'] == 'host'
        assert F.permutation_scores(dt, df, y, 'auc', device=True, **kw)['path'] == 'device'       # the switch is for 'auto'
    y_enc = dt.preprocessor.transform_y(y)
    wide = F.make_feed(dt, df, y_enc, cat_dtype=torch.int64)
    assert 'torch.int64' in F.feed_refusal(dt, wide) and "'cat' block" in F.feed_refusal(dt, wide)
    with pytest.raises(ValueError, match="the feed's 'cat' block is torch.int64"):
        F.feed_scores(dt, wide, F._entries(df, ['age']), 'auc', 1, 1.0, F._generator('cpu', 0), 128)
    streamed = F.make_feed(dt, df, y_enc, resident=False)
    assert F.feed_refusal(dt, streamed) == 'the feed is not resident on the device'

    class Bare:
        """a preprocessor that declares no map"""
        def __init__(self, inner):
            self.inner = inner

        def __getattr__(self, name):
            if name == 'source_columns':
                raise AttributeError(name)
            return getattr(self.inner, name)

    pp = dt.preprocessor
    try:
        dt.preprocessor = Bare(pp)
        assert F.feed_refusal(dt, F.make_feed(dt, df, y_enc)) == 'Bare declares no source_columns()'
        res = F.permutation_scores(dt, df, y, 'auc', **kw)                 # 'auto': the host path serves it
        assert res['path'] == 'host'
    finally:
        dt.preprocessor = pp
    assert np.array_equal(res['score_decreases'], F.permutation_scores(dt, df, y, 'auc', device=False, **kw)['score_decreases'])


def test_a_group_is_permuted_with_one_permutation(fitted):
    dt, df, y = fitted['binary']
    res = F.permutation_scores(dt, df, y, 'auc', n_iter=2, mode='max', random_state=4, columns=[['age', 'job'], 'rate'])
    assert res['columns'] == [('age', 'job'), 'rate']
    # by hand: the same stream, ONE permutation for both members
    pp, dm = dt.preprocessor, dt.model
    from deeptables_amd import metrics
    g = torch.Generator().manual_seed(4)
    y_enc = pp.transform_y(y)
    score = lambda f: metrics.compute_metric('auc', y_enc, dm.predict(pp.transform_X(f), batch_size=128), dm.task)
    base, want = score(df), np.zeros((2, 2))
    for i in range(2):
        for c, members in enumerate((['age', 'job'], ['rate'])):
            perm = torch.randperm(len(df), generator=g).numpy()
            frame = df.copy()
            for m in members:
                frame[m] = df[m].values[perm]
            want[i, c] = base - score(frame)
    assert np.array_equal(res['score_decreases'], want)
    # ... and on the feed the two members' inputs move together
    feed = F.make_feed(dt, df, y_enc)
    tg = F.feed_targets(dm, feed, pp.source_columns(), ['age', 'job'])
    assert tg == {0: [dm.categorical_columns.index(next(c for c in dm.categorical_columns if c.name == 'job'))],
                  1: [list(dm.continuous_columns[0].column_names).index('age')]}
    fi = F.get_score_importances(dt, df, y, 'auc', n_iter=2, mode='max', random_state=4, columns=[['age', 'job'], 'rate'])
    assert fi.dtype == object and ('age', 'job') in fi[:, 0].tolist() and isinstance(fi[0, 1], float)


# ---- 6. C-ABI -----------------------------------------------------------------------------------------------------------------
def test_column_entry_points_check_their_arguments_before_any_launch():
    from deeptables_amd import _lib
    lib = _lib.lib()
    P = ctypes.c_void_p(0x10000)                    # never dereferenced: every call below returns before a launch
    ODD = ctypes.c_void_p(0x10002)

    def gather(block=P, N=8, C=4, col0=1, width=2, perm=P, out=P):
        return lib.dt_column_gather(block, N, C, col0, width, perm, out, None)

    def swap(block=P, N=8, C=4, col0=1, width=2, buf=P):
        return lib.dt_column_swap(block, N, C, col0, width, buf, None)

    for name, f, ptrs in (('dt_column_gather', gather, ('block', 'perm', 'out')), ('dt_column_swap', swap, ('block', 'buf'))):
        assert f(N=0) == 0
        bad = [dict(N=-1), dict(C=0), dict(C=-3), dict(width=0), dict(width=-1), dict(col0=-1), dict(col0=3, width=2),
               dict(col0=0, width=5), dict(col0=4, width=1), dict(col0=2 ** 31 - 1, width=2 ** 31 - 1, C=2 ** 31 - 1)]
        bad += [{p: None} for p in ptrs] + [{p: ODD} for p in ptrs]
        bad += [dict(N=0, C=0), dict(N=0, block=None)]                 # N == 0 does not excuse the rest
        for kw in bad:
            assert f(**kw) == -1, (name, kw)
            assert name.encode() in lib.dt_last_error(), (name, kw, lib.dt_last_error())
