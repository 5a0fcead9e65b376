# -*- coding:utf-8 -*-
"""CPU: DeepTable.fit_cross_validation's host path and the model set around it (models/cross_validation.py, models/modelset.py),
with the fold fit replaced (tests/cross_validation_support.py: the layers have no CPU training path) — the folds are sklearn's,
the out-of-fold NaN pattern, the result shapes, the means against their numpy restatement from the set's own models, the
selectors, save / load of a set; the torch branches of ops.take_rows / put_rows / ensemble_mean against numpy bit for bit; and
the argument checks of dt_rows_take / dt_rows_put / dt_ensemble_mean before any launch."""
import ctypes
import os
import pickle

import numpy as np
import pytest
import torch

from tests import cross_validation_support as CS
from tests import feature_importance_support as FS

FOLDS, BS = 3, 32


@pytest.fixture(scope='module')
def _cpu():
    mp = pytest.MonkeyPatch()
    FS.cpu_kernels(mp)
    from deeptables_amd.models import cross_validation as CV, deepmodel
    mp.setattr(CV, '_fit_fold', CS.CpuFoldFit())
    mp.setattr(deepmodel, 'default_device', lambda: torch.device('cpu'))      # DeepTable.load builds where this says
    yield mp
    mp.undo()


def _run(task, **kw):
    from deeptables_amd.models import DeepTable
    df, y = CS.host_frame(task)
    dt = DeepTable(config=CS.host_config(task))
    mp = pytest.MonkeyPatch()
    spy = CS.PreprocessorSpy(mp, dt.preprocessor)
    try:
        out = dt.fit_cross_validation(df, y, X_eval=df.iloc[:50], X_test=df.iloc[100:170], num_folds=FOLDS, batch_size=BS,
                                      epochs=2, verbose=0, **kw)
    finally:
        mp.undo()                                   # (the spy's closures must not ride along into a pickle)
    return dt, df, y, out, spy


@pytest.fixture(scope='module', params=['binary', 'multiclass', 'regression'])
def cv(request, _cpu):
    return (request.param,) + _run(request.param)


# ---- 1. the kernels' C-ABI and torch branches ---------------------------------------------------------------------------------
def test_row_entry_points_check_their_arguments_before_any_launch():
    from deeptables_amd import _lib
    lib = _lib.lib()
    P = ctypes.c_void_p(0x10000)                    # never dereferenced: every call below returns before a launch
    ODD, ODD8 = ctypes.c_void_p(0x10002), ctypes.c_void_p(0x10004)

    def take(block=P, N=8, C=4, idx=P, n=8, out=P):
        return lib.dt_rows_take(block, N, C, idx, n, out, None)

    def put(block=P, N=8, C=4, idx=P, n=8, src=P):
        return lib.dt_rows_put(block, N, C, idx, n, src, None)

    for name, f, other in (('dt_rows_take', take, 'out'), ('dt_rows_put', put, 'src')):
        assert f(n=0) == 0                                              # no row to move: no launch
        bad = [dict(N=-1), dict(C=0), dict(C=-3), dict(n=-1), dict(idx=ODD8), dict(idx=ODD)]
        bad += [{p: None} for p in ('block', 'idx', other)] + [{p: ODD} for p in ('block', other)]
        bad += [dict(n=0, C=0), dict(n=0, block=None), dict(n=0, N=-1)]            # n == 0 does not excuse the rest
        for kw in bad:
            assert f(**kw) == -1, (name, kw)
            assert name.encode() in lib.dt_last_error(), (name, kw, lib.dt_last_error())
    assert put(N=0) == 0                                                # no row to write to: every entry is out of range

    def mean(parts=(0x10000, 0x10000), K=None, total=8, mode=0, out=P, table=True):
        arr = (ctypes.c_void_p * max(len(parts), 1))(*parts)
        return lib.dt_ensemble_mean(arr if table else None, len(parts) if K is None else K, total, mode, out, None)

    assert mean(total=0) == 0 and mean(total=0, mode=1) == 0
    bad = [dict(K=0), dict(parts=(0x10000,) * 65), dict(K=-1), dict(total=-1), dict(mode=2), dict(mode=-1), dict(out=None),
           dict(table=False), dict(parts=(0x10000, 0)), dict(parts=(0x10002, 0x10000)), dict(out=ODD), dict(out=ODD, mode=1),
           dict(out=ODD8, mode=0), dict(total=0, K=0), dict(total=0, mode=5), dict(total=0, out=None)]
    for kw in bad:
        assert mean(**kw) == -1, kw
        assert b'dt_ensemble_mean' in lib.dt_last_error(), (kw, lib.dt_last_error())
    assert mean(parts=(0x10000,) * 64, total=0) == 0 and mean(out=ODD8, mode=1, total=0) == 0


def _special_words(N, C, g):
    x = torch.randn(N * C, generator=g).view(torch.int32).clone()
    special = torch.tensor([0x7FC00001, 0x7FC12345, 0x7F800001, -0x3FFFFF, 0, -0x80000000, 1, 0x007FFFFF, -0x7FFFFFFF,
                            0x7F800000, -0x00800000], dtype=torch.int64).to(torch.int32)
    pos = torch.randperm(N * C, generator=g)[:max(1, N * C // 3)]
    x[pos] = special[torch.arange(pos.numel()) % special.numel()]
    return x.view(N, C)


def test_take_and_put_rows_torch_branches_against_numpy():
    from deeptables_amd import ops
    g = torch.Generator().manual_seed(5)
    for N, C in ((1, 1), (7, 3), (40, 4), (33, 26)):
        words = _special_words(N, C, g)
        for dtype in (torch.int32, torch.float32):
            block = words.view(dtype).clone()
            idxs = [torch.arange(N), torch.arange(N).flip(0), torch.randint(0, N, (2 * N,), generator=g),
                    torch.tensor([-1, 0, N, N - 1, 2 ** 40, 0]), torch.zeros(0, dtype=torch.int64)]
            for idx in idxs:
                out = ops.take_rows(block, idx)
                i = idx.numpy()
                ok = (i >= 0) & (i < N)
                want = np.zeros((len(i), C), dtype=np.int32)
                want[ok] = words.numpy()[i[ok]]
                assert out.dtype == dtype and np.array_equal(out.view(torch.int32).numpy(), want)
                assert torch.equal(block.view(torch.int32), words)                      # only read
            for idx in (torch.randperm(N, generator=g)[:max(1, N // 2)], torch.tensor([-1, N, 2 ** 40, 0]),
                        torch.zeros(0, dtype=torch.int64)):
                src = _special_words(idx.numel(), C, g)
                target = block.clone()
                assert ops.put_rows(target, idx, src.view(dtype)) is target
                i = idx.numpy()
                ok = (i >= 0) & (i < N)
                want = words.numpy().copy()
                want[i[ok]] = src.numpy()[ok]
                assert np.array_equal(target.view(torch.int32).numpy(), want)
        y = torch.randn(N, generator=g)                                                 # a 1-D y moves too
        assert torch.equal(ops.take_rows(y, torch.arange(N).flip(0)), y.flip(0))
    block = torch.zeros(4, 2, dtype=torch.int32)
    for bad in (lambda: ops.take_rows(block.double(), torch.arange(2)), lambda: ops.take_rows(block, torch.arange(2).int()),
                lambda: ops.take_rows(block.t(), torch.arange(2)), lambda: ops.put_rows(block, torch.arange(2), block),
                lambda: ops.put_rows(block, torch.arange(2), block[:2].float())):
        with pytest.raises(ValueError):
            bad()


def test_ensemble_mean_torch_branch_against_numpy():
    from deeptables_amd import ops
    g = torch.Generator().manual_seed(6)
    for K in (1, 2, 5, 64):
        parts = [torch.randn(37, 3, generator=g) * 10 ** float(torch.randint(-3, 4, (1,), generator=g)) for _ in range(K)]
        parts[0][0, 0], parts[-1][1, 1], parts[0][2, 2] = float('nan'), float('inf'), float('-inf')
        acc = np.zeros((37, 3))
        for p in parts:
            acc += p.numpy()
        acc /= K
        got = ops.ensemble_mean(parts, mode=0)
        assert got.dtype == torch.float64 and CS.same_bits(got.numpy(), acc)
        run = parts[0].numpy() / K
        for p in parts[1:]:
            run += p.numpy() / K
        got = ops.ensemble_mean(parts, mode=1)
        assert run.dtype == np.float32 and got.dtype == torch.float32 and CS.same_bits(got.numpy(), run)
        alias = parts[1 % K].numpy()                                                    # K parts that are one buffer
        acc, run = np.zeros((37, 3)), alias / K
        for k in range(K):
            acc += alias
            run = run + alias / K if k else run
        assert CS.same_bits(ops.ensemble_mean([parts[1 % K]] * K, mode=0).numpy(), acc / K)
        assert CS.same_bits(ops.ensemble_mean([parts[1 % K]] * K, mode=1).numpy(), run)
    for bad in (lambda: ops.ensemble_mean([]), lambda: ops.ensemble_mean([parts[0]] * 65),
                lambda: ops.ensemble_mean(parts[:2], mode=2), lambda: ops.ensemble_mean([parts[0], parts[1].double()]),
                lambda: ops.ensemble_mean([parts[0], parts[1][:5]])):
        with pytest.raises(ValueError):
            bad()


# ---- 2. fit_cross_validation on the host path ---------------------------------------------------------------------------------
def test_folds_are_sklearns(_cpu):
    from sklearn.model_selection import KFold, StratifiedKFold
    from deeptables_amd.models import DeepTable, cross_validation as CV
    for task in ('binary', 'regression'):
        df, y = CS.host_frame(task)
        dt = DeepTable(config=CS.host_config(task))
        X_t, y_t = dt.preprocessor.fit_transform(df, y)
        for stratified in (False, True):
            got = CV.make_folds(dt, X_t, np.asarray(y_t), 5, stratified, None, 9527)
            cls = StratifiedKFold if stratified and task != 'regression' else KFold
            want = list(cls(n_splits=5, shuffle=True, random_state=9527).split(X_t, y_t))
            assert len(got) == 5
            for (tr, va), (wtr, wva) in zip(got, want):
                assert tr.dtype == np.int64 and np.array_equal(tr, wtr) and np.array_equal(va, wva)
        if task == 'binary':                                    # the two differ, so the switch is seen to act
            a = CV.make_folds(dt, X_t, np.asarray(y_t), 5, False, None, 9527)
            b = CV.make_folds(dt, X_t, np.asarray(y_t), 5, True, None, 9527)
            assert any(not np.array_equal(x[1], z[1]) for x, z in zip(a, b))


def test_host_results_shapes_and_restatement(cv):
    task, dt, df, y, (oof, ev, te), spy = cv
    n = len(df)
    assert dt.last_cv_path == 'host'
    width = {'binary': 2, 'multiclass': 3, 'regression': 1}[task]
    assert oof.shape == ((n,) if task == 'regression' else (n, width)) and oof.dtype == np.float64
    assert ev.shape == (50, width) and te.shape == (70, width) and ev.dtype == np.float32
    assert not np.isnan(oof).any()                               # KFold: every row is validated once
    if task != 'regression':
        assert np.allclose(oof.sum(1), 1.0, atol=1e-6) and np.allclose(te.sum(1), 1.0, atol=1e-6)
    if task == 'binary':
        assert np.array_equal(oof[:, 0], 1.0 - oof[:, 1]) and np.array_equal(ev[:, 0], 1.0 - ev[:, 1])
    from deeptables_amd.models import cross_validation as CV
    folds = CV.make_folds(dt, spy.X_t, np.asarray(spy.y_t), FOLDS, False, None, 9527)
    want = CS.host_restatement(dt, spy.X_t, folds, df.iloc[:50], df.iloc[100:170], BS)
    for got, w in zip((oof, ev, te), want):
        assert CS.same_bits(got, w)
    assert spy.fits == 1 and spy.transforms == 2 * FOLDS        # one fit_transform; X_eval and X_test once per fold


def test_model_set_after_cross_validation(cv):
    task, dt, df, y, out, spy = cv
    names = [f'dnn_nets-kfold-{i + 1}' for i in range(FOLDS)]
    infos = dt.modelset.get_modelinfos()
    assert [mi.name for mi in infos] == names and all(mi.type == 'val' for mi in infos)
    metric = dt.config.first_metric_name.lower()
    assert dt.modelset.metric == metric and dt.modelset.best_mode == 'auto'
    for mi in infos:
        assert mi.model.optimizer is None                       # kept without optimizer state
        assert 'loss' in mi.score and f'val_{metric}' in mi.score and len(mi.meta['history']['loss']) == 2
    board = dt.leaderboard
    assert list(board.columns[:2]) == ['model', 'type'] and sorted(board['model']) == names
    assert dt.get_model('current') is infos[-1].model and dt.model is infos[-1].model
    assert dt.get_model() is dt.get_model('current')
    assert dt.get_model('best') is dt.modelset.best_model().model and dt.best_model is dt.get_model('best')
    assert dt.get_model('best') is dt.modelset.get_modelinfo(board['model'][0]).model
    assert dt.get_model('all') == [mi.model for mi in infos]
    assert dt.get_model(names[1]) is infos[1].model
    with pytest.raises(ValueError, match='does not exist'):
        dt.get_model('dnn_nets-kfold-9')
    with pytest.raises(ValueError, match='Wrong model_selector'):
        dt.evaluate(df, y, model_selector='all')
    with pytest.raises(ValueError, match='Wrong model_selector'):
        dt.apply(df, ['task_output'], model_selector='all')


def test_selectors_on_predict(cv):
    task, dt, df, y, out, spy = cv
    X = df.iloc[20:90]
    pp, models = dt.preprocessor, dt.get_model('all')
    fix = (lambda p: np.hstack([1.0 - p, p])) if task == 'binary' else (lambda p: p)
    each = [fix(m.predict(pp.transform_X(X), batch_size=BS)) for m in models]
    assert CS.same_bits(dt.predict_proba(X, batch_size=BS), each[-1])                           # 'current' is the last fold
    assert CS.same_bits(dt.predict_proba(X, BS, 0, model_selector='current'), each[-1])
    names = [mi.name for mi in dt.modelset.get_modelinfos()]
    assert CS.same_bits(dt.predict_proba(X, batch_size=BS, model_selector=names[0]), each[0])
    best = names.index(dt.modelset.best_model().name)
    assert CS.same_bits(dt.predict_proba(X, batch_size=BS, model_selector='best'), each[best])
    acc = np.zeros(each[0].shape)
    for p in each:
        acc += p
    acc /= len(each)
    got = dt.predict_proba(X, batch_size=BS, model_selector='all')
    assert got.dtype == np.float64 and CS.same_bits(got, acc)
    assert CS.same_bits(dt.predict_proba(pp.transform_X(X), batch_size=BS, model_selector='all', auto_transform_data=False), acc)
    all_ = dt.predict_proba_all(X, batch_size=BS)
    assert list(all_) == names and all(CS.same_bits(all_[k], p) for k, p in zip(names, each))
    pred = dt.predict(X, batch_size=BS, model_selector='all')
    if task == 'regression':
        assert np.array_equal(pred, acc.reshape(-1)) and dt.proba2predict(acc) is acc
    else:
        labels = np.asarray(dt.classes_)[acc.argmax(-1)]
        assert np.array_equal(pred, labels) and np.array_equal(dt.proba2predict(acc), labels)
        assert np.array_equal(dt.proba2predict(acc, encode_to_label=False), acc.argmax(-1))
        if task == 'binary':
            assert np.array_equal(dt.proba2predict(acc[:, 1:], encode_to_label=False), (acc[:, 1] > 0.5).astype('int32'))
    res = dt.evaluate(df, y, batch_size=BS, model_selector=names[0])
    assert 'loss' in res


def test_left_out_rows_are_nan_and_scores_per_fold(_cpu):
    from deeptables_amd.models import DeepTable
    df, y = CS.host_frame('binary')
    left = np.arange(7, 207, 20)
    assert left.size == 10
    dt = DeepTable(config=CS.host_config('binary'))
    w = np.linspace(0.5, 2.0, len(df))
    oof, ev, te, scores = dt.fit_cross_validation(df, y, X_test=df.iloc[:30], iterators=CS.LeaveOut(FOLDS, left), batch_size=BS,
                                                  epochs=1, verbose=0, oof_metrics=['auc', 'accuracy'], sample_weight=w,
                                                  class_weight={0: 1.0, 1: 2.0})
    assert ev is None and te.shape == (30, 2)
    assert np.array_equal(np.flatnonzero(np.isnan(oof).any(1)), left) and np.isnan(oof[left]).all()
    assert len(scores) == FOLDS and all(set(s) == {'auc', 'accuracy'} for s in scores)
    from deeptables_amd import metrics
    y_enc = dt.preprocessor.transform_y(y)
    for (tr, va), s in zip(CS.LeaveOut(FOLDS, left).split(df), scores):
        assert s['auc'] == metrics.compute_metric('auc', y_enc[va], oof[va][:, 1:].astype(np.float32), 'binary')
    with pytest.raises(ValueError, match='sample_weight'):
        dt.fit_cross_validation(df, y, num_folds=FOLDS, sample_weight=w[:-1], verbose=0)


def test_routing_and_refusals(_cpu, monkeypatch):
    from deeptables_amd.models import DeepTable
    df, y = CS.host_frame('binary')
    dt = DeepTable(config=CS.host_config('binary'))
    with pytest.raises(ValueError, match=r'device=True: the model is on cpu, not on a GPU'):
        dt.fit_cross_validation(df, y, num_folds=FOLDS, verbose=0, device=True)
    with pytest.raises(ValueError, match='device must be'):
        dt.fit_cross_validation(df, y, num_folds=FOLDS, verbose=0, device='gpu')
    with pytest.raises(ValueError, match='empty'):
        dt.fit_cross_validation(df.iloc[:0], y[:0])
    dt.fit_cross_validation(df, y, num_folds=2, batch_size=BS, verbose=0, device=False)
    assert dt.last_cv_path == 'host' and len(dt.modelset.get_modelinfos()) == 2


def test_device_logic_on_cpu_feeds_equals_the_host_path(_cpu, monkeypatch):
    """models/cross_validation.py's device path over CPU feeds (the ops' torch branches) against the host restatement from the
    models it leaves: the fold feeds equal the feeds of `iloc` slices, weight column included, and the results the same bits"""
    from deeptables_amd import training
    from deeptables_amd.models import DeepTable, cross_validation as CV
    df, y = CS.host_frame('binary')
    dt = DeepTable(config=CS.host_config('binary', apply_class_weight=True))
    pp = dt.preprocessor
    X_t, y_t = pp.fit_transform(df, y)
    y_t = np.asarray(y_t)
    left = np.arange(3, 203, 20)
    folds = CV.make_folds(dt, X_t, y_t, FOLDS, False, CS.LeaveOut(FOLDS, left), 9527)
    weights = CV.row_weights(y_t, dt.get_class_weight(y_t), np.linspace(0.5, 2.0, len(df)))
    feed = CV.make_feed(dt, X_t, y_t, 'cpu', weights)
    ev, te = CV.make_feed(dt, pp.transform_X(df.iloc[:50]), None, 'cpu'), CV.make_feed(dt, pp.transform_X(df.iloc[60:99]), None, 'cpu')
    spy = CS.FeedSpy(monkeypatch)
    kw = CV._fit_kwargs(BS, 1, 0, None, True, 0, None, None, 1)
    oof, em, tm, scores = CV.device_cross_validation(dt, feed, folds, ev, te, kw, ['auc'])
    assert len(spy.cuts) == FOLDS and len(scores) == FOLDS
    for (f, tr, va, train, val), (wtr, wva) in zip(spy.cuts, folds):
        assert f is feed and np.array_equal(tr, wtr) and np.array_equal(va, wva)
        args = (dt.preprocessor.categorical_columns, dt.preprocessor.continuous_columns, 'cpu', dt.task, dt.num_classes)
        assert CS.feeds_equal(train, training.TableBatches(X_t.iloc[tr], y_t[tr], *args, sample_weight=weights[tr]))
        assert CS.feeds_equal(val, training.TableBatches(X_t.iloc[va], y_t[va], *args))
    want = CS.host_restatement(dt, X_t, folds, df.iloc[:50], df.iloc[60:99], BS)
    oof = np.hstack([1.0 - oof, oof])
    for got, w in zip((oof, CV.fix_binary(dt, em), CV.fix_binary(dt, tm)), want):
        assert CS.same_bits(got, w)
    assert np.array_equal(np.flatnonzero(np.isnan(oof).any(1)), left)


def test_fit_keeps_its_return_value_and_fills_the_set(_cpu, monkeypatch):
    """DeepTable.fit: (model, history) as before, `model` and `_models['dt-1']` as before; the set holds that one model"""
    from deeptables_amd.models import DeepTable, deepmodel
    df, y = CS.host_frame('binary')
    fold_fit = CS.CpuFoldFit()

    def fit(self, X, y, validation_data=None, batch_size=None, epochs=1, class_weight=None, sample_weight=None, **kw):
        return fold_fit(self, (X, y), (X.iloc[:40], y[:40]), batch_size=batch_size, epochs=epochs)

    monkeypatch.setattr(deepmodel.DeepModel, 'fit', fit)
    dt = DeepTable(config=CS.host_config('binary'))
    assert dt.modelset.get_modelinfos() == [] and dt.leaderboard is None
    model, history = dt.fit(df, y, batch_size=BS, epochs=2, verbose=0)
    assert dt.model is model and dt._models['dt-1'] is model and len(history.history['loss']) == 2
    [mi] = dt.modelset.get_modelinfos()
    assert (mi.type, mi.name, mi.model) == ('val', 'dnn_nets', model) and mi.meta['history'] is history.history
    assert dt.get_model('current') is model and dt.get_model('best') is model and dt.get_model('dnn_nets') is model
    dt.fit(df, y, batch_size=BS, epochs=1, verbose=0)                  # a second fit clears the set first
    assert len(dt.modelset.get_modelinfos()) == 1 and dt.get_model('all') == [dt.model]


# ---- 3. save / load -----------------------------------------------------------------------------------------------------------
def test_save_and_load_round_trip_of_a_set(cv, tmp_path):
    task, dt, df, y, out, spy = cv
    from deeptables_amd.models import DeepTable
    path = str(tmp_path / 'saved')
    dt.save(path)
    names = [mi.name for mi in dt.modelset.get_modelinfos()]
    assert sorted(os.listdir(path)) == sorted(['dt.pkl', 'dt-1.safetensors'] + [f'{n}.safetensors' for n in names[:-1]])
    back = DeepTable.load(path)
    infos = back.modelset.get_modelinfos()
    assert [mi.name for mi in infos] == names and [mi.type for mi in infos] == ['val'] * FOLDS
    assert [mi.score for mi in infos] == [mi.score for mi in dt.modelset.get_modelinfos()]
    assert back.modelset.metric == dt.modelset.metric and back.modelset.best_mode == 'auto'
    assert infos[-1].model is back.model and all(isinstance(mi.model, str) for mi in infos[:-1])      # lazy
    X = df.iloc[:64]
    assert CS.same_bits(back.predict_proba(X, batch_size=BS), dt.predict_proba(X, batch_size=BS))
    assert isinstance(infos[0].model, str)
    assert CS.same_bits(back.predict_proba(X, batch_size=BS, model_selector=names[0]),
                        dt.predict_proba(X, batch_size=BS, model_selector=names[0]))
    assert not isinstance(infos[0].model, str) and isinstance(infos[1].model, str)                    # ... one at a time
    assert CS.same_bits(back.predict_proba(X, batch_size=BS, model_selector='all'),
                        dt.predict_proba(X, batch_size=BS, model_selector='all'))
    assert back.modelset.best_model().name == dt.modelset.best_model().name


def test_a_directory_in_the_earlier_format_loads(cv, tmp_path):
    """what `save` wrote before there was a model set: one weights file and a pickle without the 'modelset' key"""
    task, dt, df, y, out, spy = cv
    from deeptables_amd.models import DeepTable
    path = str(tmp_path / 'old')
    os.makedirs(path)
    dt.model.save(os.path.join(path, 'dt-1.safetensors'))
    with open(os.path.join(path, 'dt.pkl'), 'wb') as f:
        pickle.dump({'config': dt.config._replace(distribute_strategy=None), 'preprocessor': dt.preprocessor,
                     'model_file': 'dt-1.safetensors'}, f, protocol=4)
    back = DeepTable.load(path)
    assert back.modelset.get_modelinfos() == [] and back.get_model('current') is back.model
    X = df.iloc[:64]
    assert CS.same_bits(back.predict_proba(X, batch_size=BS), dt.predict_proba(X, batch_size=BS))


def test_fold_models_are_written_only_under_home_dir(_cpu, tmp_path, monkeypatch):
    from deeptables_amd.models import DeepTable
    monkeypatch.chdir(tmp_path)
    df, y = CS.host_frame('regression')
    dt = DeepTable(config=CS.host_config('regression'))
    dt.fit_cross_validation(df, y, num_folds=2, batch_size=BS, verbose=0)
    assert os.listdir(tmp_path) == []                           # no home_dir: the fold models live in memory only
    home = tmp_path / 'home'
    dt = DeepTable(config=CS.host_config('regression', home_dir=str(home)))
    assert not home.exists()
    dt.fit_cross_validation(df, y, num_folds=2, batch_size=BS, verbose=0)
    assert sorted(os.listdir(home)) == ['dnn_nets-kfold-1.safetensors', 'dnn_nets-kfold-2.safetensors']


def test_constructing_a_deeptable_creates_no_directory(tmp_path, monkeypatch):
    from deeptables_amd.models import DeepTable, ModelConfig
    monkeypatch.chdir(tmp_path)
    DeepTable(config=ModelConfig(nets=['dnn_nets'], home_dir=str(tmp_path / 'home')))
    DeepTable()
    assert os.listdir(tmp_path) == []
