# -*- coding:utf-8 -*-
"""k-fold cross-validation and model-set prediction for `DeepTable` (deeptables/models/deeptable.py:373-517 `fit_cross_validation`
and :538-571 `predict_proba` / `predict_proba_all` over the model set).  `DeepTable` only delegates to this module.

Two paths compute the same thing:
  * host: the loop a user writes with the functions the project had before — per fold `iloc` slices of the transformed frame,
    `DeepModel.fit(X_tr, y_tr, validation_data=(X_val, y_val))`, `DeepModel.predict` on the validation slice and on the
    freshly transformed X_eval / X_test, numpy `oof[idx] = p` and the running float32 `mean += p / folds`.  Any device.
  * device: ONE `fit_transform`, ONE resident `training.TableBatches` of all rows with y (the per-row weight as y's last
    column); X_eval and X_test are transformed and uploaded once.  Per fold the two index arrays are uploaded, the fold's feeds
    are cut out of the resident blocks and y with `ops.take_rows` (csrc/feed_rows.hip), a fresh `DeepModel` is fitted on them
    (`DeepModel.fit(feed, validation_data=feed)`), `DeepModel.score_batches` scores the validation, eval and test feeds,
    `ops.put_rows` writes the validation outputs into the NaN-filled out-of-fold buffer; after the last fold
    `ops.ensemble_mean(parts, mode=1)` averages the kept parts and every result crosses to the host once.
The folds, the batch boundaries and the feeds' bits are the same on both paths, and both averages are defined operation by
operation, so with the same fold models the two paths give the same bits; the fits themselves draw their own shuffles.

Deviations from the reference, all declared: no CSV file is written; `n_jobs` is accepted and the folds run one after another
on the one device; dask inputs are refused; no early-stopping callback is injected; `sample_weight` (length n) is sliced to
each fold's training rows (the reference passes it whole, which fails); the means divide by the number of folds the iterator
yields (the reference by `num_folds`, which is the same number for its own iterators); `oof_metrics` are this project's metric
names (`metrics.epoch_metrics`), one dict per fold."""
import os
import time
import types

import numpy as np
import torch

from . import deepmodel
from .modelset import ModelInfo
from .. import metrics, ops, training
from ..utils import consts
from ..utils import feature_importance as FI

DEFAULT_BATCH_SIZE = 128            # DeepModel.fit's and predict's default
TIMINGS = None                      # a dict: the phases of the next runs are timed into it (tools/cross_validation_bench.py)


def device_cv_enabled():
    """DT_AMD_DEVICE_CV=0 (read at every call) keeps device='auto' on the host path"""
    return os.environ.get('DT_AMD_DEVICE_CV', '1') != '0'


class _Phase:
    """adds the wall time of a `with` block to TIMINGS[name], the device drained at both ends; free when TIMINGS is None"""

    def __init__(self, name, device=None):
        self.name, self.device = name, device

    def _drain(self):
        if self.device is not None and torch.device(self.device).type == 'cuda':
            torch.cuda.synchronize(self.device)

    def __enter__(self):
        if TIMINGS is not None:
            self._drain()
            self.t0 = time.perf_counter()

    def __exit__(self, *exc):
        if TIMINGS is not None:
            self._drain()
            TIMINGS[self.name] = TIMINGS.get(self.name, 0.0) + time.perf_counter() - self.t0


# ---- pieces both paths share ------------------------------------------------------------------------------------------------
def target_device(dt):
    """where a fresh fold model will be built: the strategy's device, else the current GPU, else the CPU (on which only a
    replaced `_fit_fold` can train: the layers have no CPU training path)"""
    st = dt.config.distribute_strategy
    if st is not None and getattr(st, 'device', None) is not None:
        return torch.device(st.device)
    try:
        return deepmodel.default_device()
    except RuntimeError:
        return torch.device('cpu')


def _probe(dt, device):
    """what feature_importance.device_refusal / feed_refusal look at, before any fold model exists"""
    return types.SimpleNamespace(model=types.SimpleNamespace(device=device, config=dt.config), preprocessor=dt.preprocessor)


def new_model(dt):
    pp = dt.preprocessor
    return deepmodel.DeepModel(dt.task, dt.num_classes, dt.config, pp.categorical_columns, pp.continuous_columns,
                               var_categorical_len_columns=getattr(pp, 'var_len_categorical_columns', None))


def _fit_fold(dm, train, val, **fit_kwargs):
    """The fit of one fold: `train` and `val` are (X, y) pairs of the transformed frame on the host path, `TableBatches` on the
    device path.  The one place a fold trains (host tests replace it: the layers have no CPU training path)."""
    if isinstance(train, training.TableBatches):
        return dm.fit(train, validation_data=val, **fit_kwargs)
    return dm.fit(train[0], train[1], validation_data=val, **fit_kwargs)


def make_folds(dt, X_t, y_t, num_folds, stratified, iterators, random_state):
    """[(train_idx, valid_idx)] int64 arrays: sklearn's KFold(shuffle=True, random_state), StratifiedKFold when `stratified`
    and the task is not regression, or any `iterators` with .split(X, y)"""
    if iterators is None:
        from sklearn.model_selection import KFold, StratifiedKFold
        if stratified and dt.task != consts.TASK_REGRESSION:
            iterators = StratifiedKFold(n_splits=num_folds, shuffle=True, random_state=random_state)
        else:
            iterators = KFold(n_splits=num_folds, shuffle=True, random_state=random_state)
    folds = [(np.asarray(tr, dtype=np.int64), np.asarray(va, dtype=np.int64)) for tr, va in iterators.split(X_t, y_t)]
    if not folds:
        raise ValueError('fit_cross_validation: the iterator yields no fold')
    n = len(X_t)
    for tr, va in folds:
        for idx in (tr, va):
            if idx.size and (idx.min() < 0 or idx.max() >= n):
                raise ValueError(f'fit_cross_validation: a fold names a row outside [0, {n})')
        if np.unique(va).size != va.size:
            raise ValueError('fit_cross_validation: a validation fold names a row twice')
    return folds


def row_weights(y_t, class_weight, sample_weight):
    """Keras fit's per-row weight sample_weight x class_weight[label] as float32 [n] (DeepModel.fit's own arithmetic, which
    works row by row: slicing the result equals computing it on the slice), or None without either"""
    if class_weight is None and sample_weight is None:
        return None
    n = len(y_t)
    weights = np.ones(n, dtype=np.float32) if sample_weight is None else \
        np.asarray(sample_weight, dtype=np.float32).reshape(-1).copy()
    if len(weights) != n:
        raise ValueError(f'sample_weight has {len(weights)} entries for {n} rows')
    if class_weight is not None:
        yl = np.asarray(y_t)
        yl = yl.argmax(-1) if yl.ndim > 1 and yl.shape[-1] > 1 else yl.reshape(-1)
        cw = {int(k): float(v) for k, v in dict(class_weight).items()}
        weights = weights * np.array([cw.get(int(v), 1.0) for v in yl], dtype=np.float32)
    return weights


def output_width(dt):
    return dt.num_classes if dt.task in (consts.TASK_MULTICLASS, consts.TASK_MULTILABEL) else 1


def fix_binary(dt, proba):
    """the reference's fix_binary_predict_proba_result: a binary task's [n, 1] output becomes [1 - p, p]"""
    if proba is None or dt.task != consts.TASK_BINARY or proba.shape[-1] != 1:
        return proba
    if torch.is_tensor(proba):
        return torch.cat([1.0 - proba, proba], 1).contiguous()
    return np.hstack([1.0 - proba, proba])


def _fit_kwargs(batch_size, epochs, verbose, callbacks, shuffle, initial_epoch, steps_per_epoch, validation_steps,
                validation_freq):
    return dict(batch_size=batch_size, epochs=epochs, verbose=verbose, callbacks=callbacks, shuffle=shuffle,
                initial_epoch=initial_epoch, steps_per_epoch=steps_per_epoch, validation_steps=validation_steps,
                validation_freq=validation_freq)


def _keep(dt, dm, history, fold):
    """a fitted fold model enters the set, without its optimizer state; written to disk only under config.home_dir"""
    name = f'{"+".join(dt.nets)}-kfold-{fold + 1}'
    dm.release_training_state()
    if dt.config.home_dir:
        dm.save(os.path.join(os.path.expanduser(dt.config.home_dir), f'{name}.safetensors'))
    dt._push_model('val', name, dm, history.history)


# ---- the host path ----------------------------------------------------------------------------------------------------------
def host_cross_validation(dt, X_t, y_t, folds, X_eval, X_test, fit_kwargs, class_weight, sample_weight, oof_metrics):
    """-> (oof float64 [n, O] with NaN where no fold validated, eval mean, test mean (float32 or None), oof_scores or None)"""
    pp, bs, K = dt.preprocessor, fit_kwargs['batch_size'] or DEFAULT_BATCH_SIZE, len(folds)
    oof = np.full((len(X_t), output_width(dt)), np.nan)
    means = {'eval': None, 'test': None}
    scores = [] if oof_metrics is not None else None
    for fold, (tr, va) in enumerate(folds):
        with _Phase('cut'):
            X_tr, y_tr, X_va, y_va = X_t.iloc[tr], y_t[tr], X_t.iloc[va], y_t[va]
            sw = None if sample_weight is None else np.asarray(sample_weight).reshape(-1)[tr]
        dm = new_model(dt)
        with _Phase('train', target_device(dt)):
            history = _fit_fold(dm, (X_tr, y_tr), (X_va, y_va), class_weight=class_weight, sample_weight=sw, **fit_kwargs)
        with _Phase('score', dm.device):
            p_va = dm.predict(X_va, batch_size=bs)
            oof[va] = p_va
        for key, frame in (('eval', X_eval), ('test', X_test)):
            if frame is None:
                continue
            with _Phase('transform'):
                frame_t = pp.transform_X(frame)
            with _Phase('score', dm.device):
                p = dm.predict(frame_t, batch_size=bs)
            with _Phase('mean'):
                means[key] = p / K if means[key] is None else means[key] + p / K
        if scores is not None:
            scores.append({metrics.metric_name(m): metrics.compute_metric(m, y_va, p_va, dt.task) for m in oof_metrics})
        _keep(dt, dm, history, fold)
    return oof, means['eval'], means['test'], scores


# ---- the device path --------------------------------------------------------------------------------------------------------
def make_feed(dt, X_t, y_t, device, weights=None):
    """a transformed frame -> ONE resident feed on `device` (y_t None: inputs only)"""
    pp = dt.preprocessor
    return training.TableBatches(X_t, y_t, pp.categorical_columns, pp.continuous_columns, device, dt.task, dt.num_classes,
                                 var_len_categorical_columns=getattr(pp, 'var_len_categorical_columns', None), resident=True,
                                 sample_weight=weights)


def fold_feeds(feed, train_idx, valid_idx):
    """The training and validation feeds of one fold, cut out of the resident feed of all rows with `ops.take_rows` (index
    tensors: int64 on the feed's device).  The training feed keeps the weight column; the validation feed carries plain y."""
    tr_blocks = [ops.take_rows(b, train_idx) for b in feed.blocks]
    va_blocks = [ops.take_rows(b, valid_idx) for b in feed.blocks]
    y_tr, y_va = ops.take_rows(feed.y, train_idx), ops.take_rows(feed.y, valid_idx)
    if feed.weighted:
        y_va = y_va[:, :-1]
        y_va = (y_va.reshape(-1) if feed.y_ndim == 1 else y_va).contiguous()
    train = training.TableBatches.from_device(tr_blocks, feed.kinds, y=y_tr, y_ndim=feed.y_ndim, weighted=feed.weighted)
    val = training.TableBatches.from_device(va_blocks, feed.kinds, y=y_va, y_ndim=feed.y_ndim, weighted=False)
    return train, val


def device_refusal(dt, device, n_folds=None):
    """None when the device path can serve this DeepTable on `device`, else the condition that fails, in words"""
    reason = FI.device_refusal(_probe(dt, device))
    if reason is None and n_folds is not None and n_folds > ops.ENSEMBLE_MAX_PARTS:
        reason = f'{n_folds} folds, ops.ensemble_mean serves {ops.ENSEMBLE_MAX_PARTS}'
    return reason


def device_cross_validation(dt, feed, folds, eval_feed, test_feed, fit_kwargs, oof_metrics):
    """The folds over ready feeds (GPU tensors: the HIP row kernels; CPU tensors: the ops' torch branches) -> the host path's
    tuple.  `feed`, `eval_feed` and `test_feed` are only read."""
    bs = fit_kwargs['batch_size'] or DEFAULT_BATCH_SIZE
    dev = feed.device
    oof = torch.full((feed.n, output_width(dt)), float('nan'), dtype=torch.float32, device=dev)
    parts = {'eval': [], 'test': []}
    scores = [] if oof_metrics is not None else None
    for fold, (tr, va) in enumerate(folds):
        with _Phase('cut', dev):
            tr_d, va_d = torch.from_numpy(tr).to(dev), torch.from_numpy(va).to(dev)
            train, val = fold_feeds(feed, tr_d, va_d)
        dm = new_model(dt)
        with _Phase('train', dev):
            history = _fit_fold(dm, train, val, **fit_kwargs)
        with _Phase('score', dev):
            p_va = dm.score_batches(val, bs).reshape(val.n, -1).contiguous()
            ops.put_rows(oof, va_d, p_va)
            for key, f in (('eval', eval_feed), ('test', test_feed)):
                if f is not None:
                    parts[key].append(dm.score_batches(f, bs).reshape(f.n, -1).contiguous())
            if scores is not None:
                scores.append(metrics.epoch_metrics(list(oof_metrics), val.y, p_va, dt.task))
        _keep(dt, dm, history, fold)
    with _Phase('mean', dev):
        means = {k: ops.ensemble_mean(v, mode=1) if v else None for k, v in parts.items()}
    with _Phase('copy', dev):
        out = (oof.cpu().numpy().astype(np.float64), *(None if means[k] is None else means[k].cpu().numpy()
                                                        for k in ('eval', 'test')))
    return out + (scores,)


# ---- the entry point --------------------------------------------------------------------------------------------------------
def fit_cross_validation(dt, X, y, X_eval=None, X_test=None, num_folds=5, stratified=False, iterators=None, batch_size=None,
                         epochs=1, verbose=1, callbacks=None, n_jobs=1, random_state=9527, shuffle=True, class_weight=None,
                         sample_weight=None, initial_epoch=0, steps_per_epoch=None, validation_steps=None, validation_freq=1,
                         max_queue_size=10, workers=1, use_multiprocessing=False, oof_metrics=None, device='auto'):
    if X is None or len(X) == 0:
        raise ValueError('X can not be empty.')
    if device not in ('auto', True, False):
        raise ValueError(f"device must be 'auto', True or False, got {device!r}")
    for frame in (X, y, X_eval, X_test):
        if type(frame).__module__.split('.')[0] == 'dask':
            raise ValueError('fit_cross_validation: dask inputs are not served; pass pandas / numpy data')
    dt._modelset.clear()
    dt.model = None
    pp = dt.preprocessor
    with _Phase('transform'):
        X_t, y_t = pp.fit_transform(X, y)
    y_t = np.asarray(y_t)
    if len(pp.categorical_columns) == 0 and len(pp.continuous_columns) == 0:
        raise ValueError('No valid input columns.')
    folds = make_folds(dt, X_t, y_t, num_folds, stratified, iterators, random_state)
    if class_weight is None and dt.config.apply_class_weight and dt.task == consts.TASK_BINARY:
        class_weight = dt.get_class_weight(y_t)                     # reference deeptable.py:428-429
    if sample_weight is not None and len(np.asarray(sample_weight).reshape(-1)) != len(X_t):
        raise ValueError(f'sample_weight has {len(np.asarray(sample_weight).reshape(-1))} entries for {len(X_t)} rows')
    fit_kwargs = _fit_kwargs(batch_size, epochs, verbose, callbacks, shuffle, initial_epoch, steps_per_epoch, validation_steps,
                             validation_freq)
    dev = target_device(dt)
    feed = None
    if device is not False:
        reason = device_refusal(dt, dev, len(folds))
        if reason is None and device == 'auto' and not device_cv_enabled():
            reason = 'DT_AMD_DEVICE_CV=0'
        if reason is None:
            with _Phase('upload', dev):
                feed = make_feed(dt, X_t, y_t, dev, row_weights(y_t, class_weight, sample_weight))
            reason = FI.feed_refusal(_probe(dt, dev), feed)
        if reason is not None:
            if device is True:
                raise ValueError(f'device=True: {reason}')
            feed = None
    if feed is not None:
        side = []
        for frame in (X_eval, X_test):
            if frame is None:
                side.append(None)
                continue
            with _Phase('transform'):
                frame_t = pp.transform_X(frame)
            with _Phase('upload', dev):
                side.append(make_feed(dt, frame_t, None, dev))
        oof, eval_mean, test_mean, scores = device_cross_validation(dt, feed, folds, side[0], side[1], fit_kwargs, oof_metrics)
    else:
        oof, eval_mean, test_mean, scores = host_cross_validation(dt, X_t, y_t, folds, X_eval, X_test, fit_kwargs,
                                                                  class_weight, sample_weight, oof_metrics)
    dt.last_cv_path = 'device' if feed is not None else 'host'
    # the out-of-fold rows no fold validated stay NaN in every column (reference deeptable.py:480-490)
    if dt.task == consts.TASK_BINARY:
        oof = fix_binary(dt, oof)
    elif dt.task == consts.TASK_REGRESSION:
        oof = oof.reshape(len(X_t))
    eval_mean, test_mean = fix_binary(dt, eval_mean), fix_binary(dt, test_mean)
    if oof_metrics is not None:
        return oof, eval_mean, test_mean, scores
    return oof, eval_mean, test_mean


# ---- prediction over the model set --------------------------------------------------------------------------------------------
def _device_models(dt, models):
    """the condition under which the set is scored on one resident feed, or None"""
    if not device_cv_enabled():
        return 'DT_AMD_DEVICE_CV=0'
    if len(models) > ops.ENSEMBLE_MAX_PARTS:
        return f'{len(models)} models, ops.ensemble_mean serves {ops.ENSEMBLE_MAX_PARTS}'
    devices = {str(m.device) for m in models}
    if len(devices) != 1:
        return f'the models are on {sorted(devices)}'
    return FI.device_refusal(_probe(dt, models[0].device))


def predict_set(dt, X, models, batch_size=DEFAULT_BATCH_SIZE, auto_transform_data=True):
    """[proba of every model, binary outputs as [1 - p, p]] as numpy arrays on the host path, as device tensors on the device path
    (ONE transform, ONE upload, one score_batches per model) -> (list, on_device)"""
    X_t = dt.preprocessor.transform_X(X) if auto_transform_data else X
    if _device_models(dt, models) is None:
        feed = make_feed(dt, X_t, None, models[0].device)
        if FI.feed_refusal(_probe(dt, models[0].device), feed) is None:
            return [fix_binary(dt, m.score_batches(feed, batch_size).reshape(feed.n, -1).contiguous()) for m in models], True
    return [fix_binary(dt, m.predict(X_t, batch_size=batch_size)) for m in models], False


def predict_proba_mean(dt, X, models, batch_size=DEFAULT_BATCH_SIZE, auto_transform_data=True):
    """the float64 mean of every model's proba (reference deeptable.py:542-553: a float64 zero array, += per model, /= K)"""
    probas, on_device = predict_set(dt, X, models, batch_size, auto_transform_data)
    if on_device:
        return ops.ensemble_mean(probas, mode=0).cpu().numpy()
    acc = np.zeros(probas[0].shape)
    for p in probas:
        acc += p
    acc /= len(probas)
    return acc


def predict_proba_each(dt, X, names, models, batch_size=DEFAULT_BATCH_SIZE, auto_transform_data=True):
    probas, on_device = predict_set(dt, X, models, batch_size, auto_transform_data)
    return {name: (p.cpu().numpy() if on_device else p) for name, p in zip(names, probas)}
