# -*- coding:utf-8 -*-
"""Shared by tests/test_cross_validation_host.py and tests/test_cross_validation_gpu.py: the frames, a leave-out fold iterator,
spies on the preprocessor and on the feeds of models/cross_validation.py, the fold fit the host tests swap in (the layers have
no CPU training path, tests/feature_importance_support.py), and the host restatement of fit_cross_validation's results from the
model set's own models — per fold `DeepModel.predict` on `iloc` slices of the transformed frame, numpy `oof[idx] = p`, the
reference's running float32 `mean += p / folds` (deeptables/models/deeptable.py:454-465) — which is the yardstick."""
import numpy as np
import pandas as pd
import torch

from tests import feature_importance_support as FS

TOWER = FS.TOWER


def host_frame(task, n=240, seed=0):
    """3 string + 1 int categorical, 3 float columns with NaNs; labels that depend on one of each"""
    rng = np.random.default_rng(seed)
    df = pd.DataFrame({'s1': rng.choice(['a', 'b', 'c', 'd'], n), 's2': rng.choice(['x', 'y', 'z'], n),
                       's3': rng.choice(['p', 'q'], n), 'k': rng.integers(0, 5, n),
                       'f1': rng.normal(size=n), 'f2': rng.normal(size=n) * 3 + 1, 'f3': rng.random(n)})
    for c in ('f1', 'f2', 'f3'):
        v = df[c].values.copy()
        v[rng.random(n) < 0.1] = np.nan
        df[c] = v
    z = np.nan_to_num(df['f1'].values) + (df['s1'] == 'b').values * 1.5 + rng.normal(size=n) * 0.3
    if task == 'binary':
        y = np.where(z > 0.3, 'yes', 'no')
    elif task == 'multiclass':
        y = np.digitize(z, [-0.4, 0.9])
    else:
        y = z * 2 + 1 + rng.normal(size=n) * 1e-3
    return df, y


def host_config(task, **kw):
    from deeptables_amd.models import ModelConfig
    metrics = {'binary': ['AUC'], 'multiclass': ['accuracy'], 'regression': ['mse']}[task]
    return ModelConfig(nets=['dnn_nets'], dnn_params=TOWER, embedding_dropout=0, task=task, auto_categorize=True,
                       categorical_columns=['s1', 's2', 's3', 'k'], metrics=metrics, earlystopping_patience=0, **kw)


class LeaveOut:
    """KFold over all rows but `left_out`: those are in no validation fold (and in no training fold)"""

    def __init__(self, n_splits, left_out, random_state=9527):
        self.n_splits, self.left_out, self.random_state = n_splits, np.asarray(left_out), random_state

    def split(self, X, y=None):
        from sklearn.model_selection import KFold
        kept = np.setdiff1d(np.arange(len(X)), self.left_out)
        for tr, va in KFold(n_splits=self.n_splits, shuffle=True, random_state=self.random_state).split(kept):
            yield kept[tr], kept[va]


class PreprocessorSpy:
    """counts fit_transform / transform_X of one preprocessor and keeps what fit_transform returned"""

    def __init__(self, mp, pp):
        self.fits, self.transforms, self.X_t, self.y_t = 0, 0, None, None
        fit, tx = pp.fit_transform, pp.transform_X

        def fit_transform(X, y, *a, **kw):
            self.fits += 1
            self.X_t, self.y_t = fit(X, y, *a, **kw)
            return self.X_t, self.y_t

        def transform_X(X, *a, **kw):
            self.transforms += 1
            return tx(X, *a, **kw)

        mp.setattr(pp, 'fit_transform', fit_transform, raising=False)
        mp.setattr(pp, 'transform_X', transform_X, raising=False)


def _snapshot(feed):
    return [b.clone() for b in feed.blocks] + ([] if feed.y is None else [feed.y.clone()])


def _tensors(feed):
    return list(feed.blocks) + ([] if feed.y is None else [feed.y])


class FeedSpy:
    """records the feeds models/cross_validation.py makes (with a copy of their bits at birth) and every fold's cut"""

    def __init__(self, mp):
        from deeptables_amd.models import cross_validation as CV
        self.made, self.cuts = [], []
        make, cut = CV.make_feed, CV.fold_feeds

        def make_feed(*a, **kw):
            feed = make(*a, **kw)
            self.made.append((feed, _snapshot(feed)))
            return feed

        def fold_feeds(feed, tr, va):
            train, val = cut(feed, tr, va)
            self.cuts.append((feed, tr.cpu().numpy(), va.cpu().numpy(), train, val))
            return train, val

        mp.setattr(CV, 'make_feed', make_feed)
        mp.setattr(CV, 'fold_feeds', fold_feeds)

    def untouched(self):
        return all(torch.equal(a.view(torch.int32), b.view(torch.int32))
                   for feed, snap in self.made for a, b in zip(_tensors(feed), snap))


def feeds_equal(a, b):
    """blocks, y (its weight column included) and the bookkeeping of two feeds, as bits"""
    if a.kinds != b.kinds or a.n != b.n or a.weighted != b.weighted or a.y_ndim != b.y_ndim or len(a.blocks) != len(b.blocks):
        return False
    pairs = list(zip(_tensors(a), _tensors(b)))
    return all(x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32))
               for x, y in pairs)


# ---- the fold fit of the host tests -------------------------------------------------------------------------------------------
class CpuFoldFit:
    """Stands in for cross_validation._fit_fold under FS.cpu_kernels: builds the model on the CPU and trains it with torch's Adam
    on the project's own feed, losses and metrics; returns a History with the last epoch's validation logs.  Takes what either
    path hands over: (X, y) pairs with class_weight / sample_weight, or TableBatches."""

    def __init__(self, seed=11, lr=0.02):
        self.seed, self.lr, self.calls = seed, lr, 0

    def __call__(self, dm, train, val, batch_size=None, epochs=1, class_weight=None, sample_weight=None, **_):
        from deeptables_amd import functional, training
        from deeptables_amd.models import cross_validation as CV
        from deeptables_amd.models.deepmodel import IgnoreCaseDict
        self.calls += 1
        functional.set_seed(self.seed + self.calls)
        dm.build('cpu')
        bs = batch_size or 128

        def as_feed(pair, weights=None):
            if isinstance(pair, training.TableBatches):
                return pair
            return training.TableBatches(pair[0], pair[1], dm.categorical_columns, dm.continuous_columns, 'cpu', dm.task,
                                         dm.num_classes, sample_weight=weights)

        weights = None if isinstance(train, training.TableBatches) else CV.row_weights(train[1], class_weight, sample_weight)
        train, val = as_feed(train, weights), as_feed(val)
        opt = torch.optim.Adam(dm.model.parameters(), lr=self.lr)
        g = torch.Generator().manual_seed(self.seed + self.calls)
        history = training.History()
        for epoch in range(epochs):
            dm.model.train()
            losses = []
            for ins, yb in train.iterate(min(bs, train.n), True, True, generator=g):
                wb = None
                if train.weighted:
                    wb, yb = yb[:, -1].contiguous(), yb[:, :-1].contiguous()
                    if train.y_ndim == 1:
                        yb = yb.reshape(-1)
                opt.zero_grad()
                loss = dm._loss(dm.model(ins), yb, wb)
                loss.backward()
                opt.step()
                losses.append(float(loss.detach()))
            logs = {'loss': float(np.mean(losses))}
            logs.update({f'val_{k}': v for k, v in dm._evaluate_batches(val, bs, list(dm.config.metrics or [])).items()})
            history.add(epoch, logs)
        dm.model.eval()
        history.history = IgnoreCaseDict(history.history)
        return history


# ---- the yardstick ------------------------------------------------------------------------------------------------------------
def host_restatement(dt, X_t, folds, X_eval, X_test, batch_size):
    """fit_cross_validation's three results recomputed from the model set's fold models the way the host loop computes them"""
    pp, models = dt.preprocessor, dt.get_model('all')
    K = len(folds)
    assert len(models) == K
    width = dt.num_classes if dt.task == 'multiclass' else 1
    oof = np.full((len(X_t), width), np.nan)
    means = [None, None]
    for (tr, va), dm in zip(folds, models):
        oof[va] = dm.predict(X_t.iloc[va], batch_size=batch_size)
        for j, frame in enumerate((X_eval, X_test)):
            if frame is not None:
                p = dm.predict(pp.transform_X(frame), batch_size=batch_size)
                assert p.dtype == np.float32
                if means[j] is None:
                    means[j] = p / K
                else:
                    means[j] += p / K
    if dt.task == 'binary':
        oof = np.hstack([1.0 - oof, oof])
        means = [None if m is None else np.hstack([1.0 - m, m]) for m in means]
    elif dt.task == 'regression':
        oof = oof.reshape(len(X_t))
    return oof, means[0], means[1]


def same_bits(a, b):
    """equal shape, dtype and bits, NaN against NaN (every NaN here is numpy's or torch's own fill value, never computed)"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.isnan(a), np.isnan(b)) and \
        np.array_equal(a[~np.isnan(a)].view(np.uint8), b[~np.isnan(b)].view(np.uint8))
