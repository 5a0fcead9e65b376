# -*- coding:utf-8 -*-
"""GPU: k-fold cross-validation on the device — dt_rows_take / dt_rows_put / dt_ensemble_mean (csrc/feed_rows.hip) against torch
indexing on int32 words and numpy at the launch's edges, on sentinel-framed buffers; the device path of
models/cross_validation.py: its fold feeds against the feeds of `iloc` slices, its results against the host restatement from the
fold models it leaves (bit for bit), the resident feeds untouched, the transform counts, and the routing.

Bit equality of computed values treats NaN as NaN: IEEE 754 leaves the sign and payload of a NaN an operation produces open
(x86 gives the negative default NaN, the GPU the positive one); every other value, and every word take / put move — NaN payloads
included — is compared as bits."""
import numpy as np
import pytest
import torch

from tests import cross_validation_support as CS
from tests import feature_importance_support as FS

pytestmark = pytest.mark.gpu

SENTINEL = 0x5EA7BEE
FRAME = 64                      # words of sentinel on either side of every buffer
GRID_CAP_BLOCKS = 2048          # csrc/feed_rows.hip kRowsMaxBlocks: one element past it strides
OOB = (-1, None, 2 ** 40)       # None: N itself


# ---- 1. the kernels -----------------------------------------------------------------------------------------------------------
def _framed(dev, numel, skew=0):
    """-> (the whole sentinel-filled allocation, a [numel] int32 view FRAME words in; skew: words off 16-byte alignment)"""
    raw = torch.full((numel + 2 * FRAME + 4,), SENTINEL, dtype=torch.int32, device=dev)
    assert raw.data_ptr() % 16 == 0
    return raw, raw[FRAME + skew:FRAME + skew + numel]


def _frames_intact(raw, numel, skew=0):
    return bool((raw[:FRAME + skew] == SENTINEL).all()) and bool((raw[FRAME + skew + numel:] == SENTINEL).all())


def _words(kind, N, C, g):
    """[N, C] int32 words: random ids, or float32 bit patterns with NaNs of distinct payloads, +-0.0, denormals and +-Inf"""
    if kind == 'int32':
        return torch.randint(-2 ** 31, 2 ** 31 - 1, (N, C), generator=g, dtype=torch.int64).to(torch.int32)
    w = torch.randn(N * C, generator=g).view(torch.int32).clone()
    special = torch.tensor([0x7FC00001, 0x7FC12345, 0x7F800001, -0x3FFFFF, 0x00000000, -0x80000000, 0x00000001, 0x007FFFFF,
                            -0x7FFFFFFF, 0x7F800000, -0x00800000], dtype=torch.int64).to(torch.int32)
    pos = torch.randperm(N * C, generator=g)[:max(1, (N * C) // 3)]
    w[pos] = special[torch.arange(pos.numel()) % special.numel()]
    return w.view(N, C)


def _plant_oob(idx, N):
    idx = idx.clone()
    n = idx.numel()
    for pos, v in zip((0, n // 2, n - 1), OOB):
        if n:
            idx[pos] = N if v is None else v
    return idx


def _kfold_train(N):
    from sklearn.model_selection import KFold
    if N < 3:
        return []
    tr, _ = next(iter(KFold(n_splits=3, shuffle=True, random_state=9527).split(np.arange(N))))
    return [torch.from_numpy(np.sort(tr).astype(np.int64))]


def _take_indices(N, g):
    out = []
    for n in sorted({0, 1, 255, 256, 257, N, 2 * N}):
        ar = torch.arange(n, dtype=torch.int64)
        rep = torch.randint(0, N, (n,), generator=g)
        out += [ar % N, (N - 1 - ar) % N, rep, _plant_oob(rep, N)]           # identity, reversed, repeats, out of range
    return out + _kfold_train(N)


def _put_indices(N, g):
    """distinct in-range entries (a duplicate is the caller's error); where n exceeds N the rest is out of range"""
    out = []
    for n in sorted({0, 1, 255, 256, 257, N}):
        pad = torch.tensor([(N if v is None else v) for v in OOB] * (n // 3 + 1), dtype=torch.int64)[:max(n - N, 0)]
        k = min(n, N)
        ar = torch.arange(k, dtype=torch.int64)
        rnd = torch.randperm(N, generator=g)[:k]
        for idx in (ar, N - 1 - ar, rnd):
            out.append(torch.cat([idx, pad])[torch.randperm(n, generator=g)] if pad.numel() else idx)
        out.append(_plant_oob(rnd, N))
    return out + _kfold_train(N)


def _take_case(dev, words, idx, skew=0):
    from deeptables_amd._lib import lib, ptr, stream_ptr
    N, C = words.shape
    n = idx.numel()
    raw_b, block = _framed(dev, N * C, skew)
    raw_o, out = _framed(dev, max(n * C, 1), skew)
    block.copy_(words.reshape(-1).to(dev))
    raw_b0 = raw_b.clone()
    idx_d = torch.cat([idx, torch.tensor([2 ** 62])]).to(dev)               # one entry more: never a null pointer, also for n == 0
    ok = (idx >= 0) & (idx < N)
    want = torch.zeros(n, C, dtype=torch.int32)
    want[ok] = words[idx[ok]]
    h = lib()
    assert h.dt_rows_take(ptr(block), N, C, ptr(idx_d), n, ptr(out), stream_ptr()) == 0, h.dt_last_error()
    assert torch.equal(raw_b, raw_b0)                                       # the block is only read
    assert torch.equal(out[:n * C].view(n, C).cpu(), want)
    if n == 0:
        assert bool((raw_o == SENTINEL).all())
    else:
        assert _frames_intact(raw_o, n * C, skew)


def _put_case(dev, words, idx, g, skew=0):
    from deeptables_amd._lib import lib, ptr, stream_ptr
    N, C = words.shape
    n = idx.numel()
    raw_b, block = _framed(dev, N * C, skew)
    raw_s, src = _framed(dev, max(n * C, 1), skew)
    block.copy_(words.reshape(-1).to(dev))
    rows = _words('int32', max(n, 1), C, g)[:n]
    src[:n * C].copy_(rows.reshape(-1).to(dev))
    raw_s0 = raw_s.clone()
    idx_d = torch.cat([idx, torch.tensor([2 ** 62])]).to(dev)
    ok = (idx >= 0) & (idx < N)
    want = words.clone()
    want[idx[ok]] = rows[ok]
    h = lib()
    assert h.dt_rows_put(ptr(block), N, C, ptr(idx_d), n, ptr(src), stream_ptr()) == 0, h.dt_last_error()
    assert torch.equal(block.view(N, C).cpu(), want)                        # rows idx does not name keep their bits
    assert _frames_intact(raw_b, N * C, skew) and torch.equal(raw_s, raw_s0)


@pytest.mark.parametrize('kind', ['int32', 'float32'])
@pytest.mark.parametrize('N', [1, 2, 257, 1000])
def test_rows_take_against_torch_indexing(dev, N, kind):
    g = torch.Generator().manual_seed(300 + N)
    for C in (1, 3, 4, 8, 26):
        words = _words(kind, N, C, g)
        for idx in _take_indices(N, g):
            for skew in (0, 1):                     # C % 4 == 0 and skew 0: uint4 words; one word off: the 4-byte kernel
                _take_case(dev, words, idx, skew)


@pytest.mark.parametrize('kind', ['int32', 'float32'])
@pytest.mark.parametrize('N', [1, 2, 257, 1000])
def test_rows_put_against_torch_indexing(dev, N, kind):
    g = torch.Generator().manual_seed(400 + N)
    for C in (1, 3, 4, 8, 26):
        words = _words(kind, N, C, g)
        for idx in _put_indices(N, g):
            for skew in (0, 1):
                _put_case(dev, words, idx, g, skew)


def test_rows_one_element_past_the_grid_cap(dev):
    """C = 1, n = 2048 blocks x 256 threads + 1: the last row is reached by the stride, not by the grid"""
    n = GRID_CAP_BLOCKS * 256 + 1
    g = torch.Generator().manual_seed(9)
    words = _words('int32', 1000, 1, g)
    _take_case(dev, words, torch.randint(0, 1000, (n,), generator=g))
    big = _words('int32', n, 1, g)
    _take_case(dev, big, torch.arange(n, dtype=torch.int64).flip(0))
    _put_case(dev, big, torch.randperm(n, generator=g), g)


def test_duplicate_put_entries_leave_one_of_the_rows(dev):
    from deeptables_amd import ops
    g = torch.Generator().manual_seed(2)
    block = _words('int32', 50, 8, g).to(dev)
    before = block.cpu()
    src = _words('int32', 6, 8, g)
    idx = torch.tensor([3, 7, 3, 3, 7, 9])
    ops.put_rows(block, idx.to(dev), src.to(dev))
    now = block.cpu()
    rest = torch.ones(50, dtype=torch.bool)
    rest[idx] = False
    assert torch.equal(now[rest], before[rest]) and torch.equal(now[9], src[5])
    for row, sources in ((3, (0, 2, 3)), (7, (1, 4))):
        assert all(any(now[row, c] == src[s, c] for s in sources) for c in range(8))       # one of them wins, word by word


def _mean_parts(K, total, g, mode):
    parts = []
    for k in range(K):
        p = torch.randn(total, generator=g) * 10.0 ** float(torch.randint(-6, 7, (1,), generator=g))
        if total:
            pos = torch.randperm(total, generator=g)[:max(1, total // 16)]
            special = torch.tensor([float('nan'), float('inf'), float('-inf'), 0.0, -0.0, 3.0e38, -3.0e38, 2.0 ** -100])
            p[pos] = special[torch.arange(pos.numel()) % special.numel()]
        p[(p.abs() < 2.0 ** -100) & (p != 0)] = 0.0    # mode 1: no quotient p / K is subnormal (K <= 64 = 2^6)
        parts.append(p)
    return parts


def _numpy_means(parts):
    K = len(parts)
    acc = np.zeros(parts[0].shape)
    for p in parts:
        acc += p.numpy()
    acc /= K
    with np.errstate(all='ignore'):
        run = parts[0].numpy() / K
        for p in parts[1:]:
            run += p.numpy() / K
    return acc, run


@pytest.mark.parametrize('K', [1, 2, 5, 64])
def test_ensemble_mean_against_numpy(dev, K):
    from deeptables_amd._lib import lib, ptr, stream_ptr
    import ctypes
    g = torch.Generator().manual_seed(500 + K)
    h = lib()
    for total in (0, 1, 255, 257, GRID_CAP_BLOCKS * 256 + 1):
        for alias in (False, True):
            if alias and total > 257:
                continue
            parts = _mean_parts(1 if alias else K, total, g, 1) * (K if alias else 1)
            dparts = [p.to(dev) for p in (parts[:1] if alias else parts)] * (K if alias else 1)
            snap = [p.clone() for p in dparts[:1 if alias else K]]
            with np.errstate(all='ignore'):
                wants = _numpy_means(parts)
            table = (ctypes.c_void_p * K)(*[p.data_ptr() if total else 0x10000 for p in dparts])
            for mode, want in enumerate(wants):
                words = max(total, 1) * (2 if mode == 0 else 1)
                raw, out = _framed(dev, words)
                assert h.dt_ensemble_mean(table, K, total, mode, ptr(out), stream_ptr()) == 0, h.dt_last_error()
                if total == 0:
                    assert bool((raw == SENTINEL).all())
                    continue
                assert _frames_intact(raw, words)
                got = out.view(torch.float64 if mode == 0 else torch.float32).cpu().numpy()
                assert CS.same_bits(got, want), (K, total, mode, alias)
            assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(dparts, snap))


def test_ops_wrappers_on_device_tensors(dev):
    from deeptables_amd import ops
    g = torch.Generator().manual_seed(12)
    block = _words('float32', 300, 7, g).view(torch.float32).to(dev)
    idx = torch.randint(0, 300, (450,), generator=g)
    got = ops.take_rows(block, idx.to(dev))
    assert got.dtype == torch.float32 and torch.equal(got.view(torch.int32).cpu(), block.view(torch.int32).cpu()[idx])
    y = torch.randn(300, generator=g).to(dev)
    assert torch.equal(ops.take_rows(y, idx.to(dev)), y[idx.to(dev)])
    assert ops.take_rows(block, torch.zeros(0, dtype=torch.int64, device=dev)).shape == (0, 7)
    assert ops.put_rows(block, torch.zeros(0, dtype=torch.int64, device=dev), block[:0].contiguous()) is block
    parts = [torch.randn(40, 3, generator=g).to(dev) for _ in range(3)]
    cpu = [p.cpu() for p in parts]
    for mode in (0, 1):
        assert CS.same_bits(ops.ensemble_mean(parts, mode).cpu().numpy(), ops.ensemble_mean(cpu, mode).numpy())
    assert ops.ensemble_mean([p[:0] for p in parts], 0).shape == (0, 3)
    with pytest.raises(ValueError):
        ops.take_rows(block, idx)                                               # idx on another device


# ---- 2. the paths ---------------------------------------------------------------------------------------------------------------
FOLDS, EPOCHS, BS, N_ROWS = 3, 2, 64, 600
LEFT_OUT = np.arange(11, 600, 60)                      # 10 rows no fold validates
CONFIGS = {
    'deepfm_binary': dict(task='binary', nets='DeepFM', metrics=['AUC'], conf=dict(apply_class_weight=True), cv=dict()),
    'dnn_multiclass': dict(task='multiclass', nets=['dnn_nets'], metrics=['accuracy'], conf=dict(),
                           cv=dict(iterators=lambda: CS.LeaveOut(FOLDS, LEFT_OUT), oof_metrics=['accuracy'])),
    'deepfm_regression': dict(task='regression', nets='DeepFM', metrics=['mse'], conf=dict(), cv=dict(stratified=True)),
}


def _config(spec):
    from deeptables_amd.models import ModelConfig, deepnets
    nets = deepnets.DeepFM if spec['nets'] == 'DeepFM' else spec['nets']
    return ModelConfig(nets=nets, dnn_params=FS.TOWER, embedding_dropout=0, task=spec['task'], auto_categorize=False,
                       metrics=spec['metrics'], earlystopping_patience=0, **spec['conf'])


def _frames(spec):
    df, y = FS.task_frame(spec['task'], n=N_ROWS)
    return df, y, df.iloc[:150], df.iloc[200:431]


def _cross_validate(spec, mp, **kw):
    from deeptables_amd import functional
    from deeptables_amd.models import DeepTable
    functional.set_seed(21)
    df, y, X_eval, X_test = _frames(spec)
    dt = DeepTable(config=_config(spec))
    pps = CS.PreprocessorSpy(mp, dt.preprocessor)
    feeds = CS.FeedSpy(mp)
    cv_kw = {k: (v() if callable(v) else v) for k, v in spec['cv'].items()}
    cv_kw.update(kw)
    out = dt.fit_cross_validation(df, y, X_eval=X_eval, X_test=X_test, num_folds=FOLDS, batch_size=BS, epochs=EPOCHS, verbose=0,
                                  **cv_kw)
    # (taken now: later predictions over the set make feeds and transform frames of their own)
    return dict(dt=dt, out=out, pps=pps, feeds=feeds, counts=(pps.fits, pps.transforms), made=list(feeds.made),
                untouched=feeds.untouched(), frames=(df, y, X_eval, X_test))


@pytest.fixture(scope='module', params=list(CONFIGS))
def run(request, dev):
    mp = pytest.MonkeyPatch()
    try:
        r = _cross_validate(CONFIGS[request.param], mp)
        r['name'], r['spec'] = request.param, CONFIGS[request.param]
        yield r
    finally:
        mp.undo()


def _folds(r):
    from deeptables_amd.models import cross_validation as CV
    it = r['spec']['cv'].get('iterators')
    return CV.make_folds(r['dt'], r['pps'].X_t, np.asarray(r['pps'].y_t), FOLDS, r['spec']['cv'].get('stratified', False),
                         it() if it else None, 9527)


def test_routing_counts_and_feeds_left_alone(run):
    dt, feeds = run['dt'], run['feeds']
    assert dt.last_cv_path == 'device'
    assert run['counts'] == (1, 2)                      # ONE fit_transform, X_eval and X_test transformed once each
    made = run['made']
    assert len(made) == 3 and len(feeds.cuts) == FOLDS and all(c[0] is made[0][0] for c in feeds.cuts)
    assert [f.n for f, _ in made] == [N_ROWS, 150, 231] and all(f.resident for f, _ in made)
    assert made[0][0].weighted == (run['name'] == 'deepfm_binary')
    assert run['untouched']                             # the resident feeds are bit for bit what they were
    names = [mi.name for mi in dt.modelset.get_modelinfos()]
    nets = '+'.join(dt.nets)
    assert names == [f'{nets}-kfold-{i + 1}' for i in range(FOLDS)] and dt.model is dt.get_model(names[-1])
    assert all(m.optimizer is None and m.device.type == 'cuda' for m in dt.get_model('all'))


def test_fold_feeds_equal_the_feeds_of_frame_slices(run, dev):
    from deeptables_amd import training
    from deeptables_amd.models import cross_validation as CV
    dt, X_t, y_t = run['dt'], run['pps'].X_t, np.asarray(run['pps'].y_t)
    pp = dt.preprocessor
    weights = CV.row_weights(y_t, dt.get_class_weight(y_t), None) if run['name'] == 'deepfm_binary' else None
    folds = _folds(run)
    assert len(run['feeds'].cuts) == len(folds)
    for (_, tr, va, train, val), (wtr, wva) in zip(run['feeds'].cuts, folds):
        assert np.array_equal(tr, wtr) and np.array_equal(va, wva)
        args = (pp.categorical_columns, pp.continuous_columns, dev, dt.task, dt.num_classes)
        assert CS.feeds_equal(train, training.TableBatches(X_t.iloc[tr], y_t[tr], *args, resident=True,
                                                           sample_weight=None if weights is None else weights[tr]))
        assert CS.feeds_equal(val, training.TableBatches(X_t.iloc[va], y_t[va], *args, resident=True))


def test_out_of_fold_rows_sit_against_their_own_labels(run, dev):
    """the project's metric of oof_proba[idx_valid] against y[idx_valid] is the fold's last val_<metric> of its history exactly:
    the same weights in eval mode on the same rows at the same batch size, scored by the same code"""
    from deeptables_amd import metrics, training
    dt, oof = run['dt'], run['out'][0]
    y_t = np.asarray(run['pps'].y_t)
    metric = run['spec']['metrics'][0]
    for (tr, va), mi in zip(_folds(run), dt.modelset.get_modelinfos()):
        p = oof[va]
        p = p[:, 1:] if dt.task == 'binary' else p.reshape(len(va), -1)
        val = training.TableBatches(run['pps'].X_t.iloc[va], y_t[va], dt.preprocessor.categorical_columns,
                                    dt.preprocessor.continuous_columns, dev, dt.task, dt.num_classes)
        got = metrics.epoch_metrics([metric], val.y, torch.from_numpy(p.astype(np.float32)).to(dev), dt.task)
        assert got[metrics.metric_name(metric)] == mi.meta['history'][f'val_{metric}'][-1], (mi.name, got)


def test_device_results_equal_the_host_restatement(run):
    dt = run['dt']
    df, y, X_eval, X_test = run['frames']
    oof, ev, te = run['out'][:3]
    want = CS.host_restatement(dt, run['pps'].X_t, _folds(run), X_eval, X_test, BS)
    for name, got, w in zip(('oof', 'eval', 'test'), (oof, ev, te), want):
        assert CS.same_bits(got, w), (run['name'], name, np.abs(np.nan_to_num(got) - np.nan_to_num(w)).max())
    nan_rows = np.flatnonzero(np.isnan(oof.reshape(N_ROWS, -1)).any(1))
    assert np.array_equal(nan_rows, LEFT_OUT if run['name'] == 'dnn_multiclass' else [])
    if run['name'] == 'dnn_multiclass':
        from deeptables_amd import metrics
        scores, y_t = run['out'][3], np.asarray(run['pps'].y_t)
        assert len(scores) == FOLDS
        for (tr, va), s in zip(_folds(run), scores):
            assert s['accuracy'] == metrics.compute_metric('accuracy', y_t[va], oof[va].astype(np.float32), dt.task)
    if dt.task == 'binary':
        assert oof.shape == (N_ROWS, 2) and ev.shape == (150, 2) and np.array_equal(te[:, 0], 1.0 - te[:, 1])
    if dt.task == 'regression':
        assert oof.shape == (N_ROWS,) and te.shape == (231, 1)


def test_predict_over_the_set_equals_the_host_loop(run, monkeypatch):
    dt = run['dt']
    X = run['frames'][0].iloc[300:533]
    pp, models = dt.preprocessor, dt.get_model('all')
    names = [mi.name for mi in dt.modelset.get_modelinfos()]
    fix = (lambda p: np.hstack([1.0 - p, p])) if dt.task == 'binary' else (lambda p: p)
    each = [fix(m.predict(pp.transform_X(X), batch_size=BS)) for m in models]
    acc = np.zeros(each[0].shape)
    for p in each:
        acc += p
    acc /= len(each)
    pps = CS.PreprocessorSpy(monkeypatch, pp)
    got = dt.predict_proba(X, batch_size=BS, model_selector='all')
    assert pps.transforms == 1                          # one transform for the whole set
    assert got.dtype == np.float64 and CS.same_bits(got, acc)
    all_ = dt.predict_proba_all(X, batch_size=BS)
    assert list(all_) == names and all(CS.same_bits(all_[k], p) for k, p in zip(names, each))
    monkeypatch.setenv('DT_AMD_DEVICE_CV', '0')         # ... and the host loop of the same call gives the same bits
    assert CS.same_bits(dt.predict_proba(X, batch_size=BS, model_selector='all'), acc)
    assert CS.same_bits(dt.predict_proba(X, batch_size=BS, model_selector='current'), each[-1])


def test_host_path_end_to_end_and_routing(dev, monkeypatch):
    """the two paths train separately: compared in shape and NaN pattern only"""
    from deeptables_amd.models import cross_validation as CV
    spec = CONFIGS['dnn_multiclass']
    monkeypatch.setenv('DT_AMD_DEVICE_CV', '0')
    host = _cross_validate(spec, monkeypatch)
    assert host['dt'].last_cv_path == 'host' and host['made'] == []
    assert host['counts'] == (1, 2 * FOLDS)             # the hand-written loop: X_eval and X_test once per fold
    monkeypatch.delenv('DT_AMD_DEVICE_CV')
    device = _cross_validate(spec, monkeypatch, device=True)
    assert device['dt'].last_cv_path == 'device'
    for a, b in zip(host['out'][:3], device['out'][:3]):
        assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.isnan(a), np.isnan(b))
    assert np.array_equal(np.flatnonzero(np.isnan(host['out'][0]).any(1)), LEFT_OUT)
    assert [set(s) for s in host['out'][3]] == [set(s) for s in device['out'][3]] == [{'accuracy'}] * FOLDS
    monkeypatch.setattr(CV, 'target_device', lambda dt: torch.device('cpu'))
    with pytest.raises(ValueError, match=r'device=True: the model is on cpu, not on a GPU'):
        _cross_validate(spec, monkeypatch, device=True)
