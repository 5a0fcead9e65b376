# -*- coding:utf-8 -*-
"""TF-free, hypernets-free stand-in for `deeptables.models.preprocessor` (SURVEY §8 f4;
deeptables/models/preprocessor.py:26-515): same class names, config switches, step order and column metadata, on
pandas + scikit-learn only, so `DeepTable.fit(df, y)` runs on raw frames.

Step order of `fit_transform` (preprocessor.py:165-204): y label-encode -> feature typing (`_prepare_features`)
-> imputation -> min-max scale -> categorical label encoding -> discretisation -> var-len encoding.
`X_transformers` keeps the fitted steps in that order and `transform_X` replays them (preprocessor.py:249-260).

Where the reference defers to `hypernets.tabular.sklearn_ex` (absent here) the behaviour assumed is written next
to the transformer: it only has to be self-consistent between fit and transform — the embedding gather sees ids in
`[0, vocabulary_size)` either way (vocabulary_size = nunique + 2, preprocessor.py:333).
GBM leaf features (`apply_gbm_features`) come from `GbmLeavesEncoder`, a histogram GBDT trained by this library's own HIP
kernels (csrc/gbdt.hip) in place of hypernets' LgbmLeavesEncoder; the fit cache is not provided.
"""
import collections
import copy
import os
import time

import numpy as np
import pandas as pd

from .config import ModelConfig
from .metainfo import CategoricalColumn, ContinuousColumn, VarLenCategoricalColumn
from ..utils import consts


# ---------------------------------------------------------------------------------------------
# transformers (stand-ins for hypernets.tabular.sklearn_ex)
# ---------------------------------------------------------------------------------------------
class PassThroughEstimator:
    def fit(self, X, y=None):
        return self

    def transform(self, X):
        return X

    def fit_transform(self, X, y=None):
        return X


class CategorizeEncoder:
    """Low-cardinality numeric columns become categorical: with `remain_numeric` a string copy `<c>_cat` is added
    and the numeric column stays (preprocessor.py:320-327), otherwise the column itself is converted."""

    def __init__(self, columns, remain_numeric=True):
        self.columns = list(columns)
        self.remain_numeric = remain_numeric
        self.new_columns = []

    def fit(self, X, y=None):
        return self.fit_counts({c: X[c].nunique() for c in self.columns} if self.remain_numeric else {})

    def fit_counts(self, nuniques):
        """`fit` from the columns' nunique alone"""
        self.new_columns = [(c + '_cat', 'str', int(nuniques[c])) for c in self.columns] if self.remain_numeric else []
        return self

    def transform(self, X):
        for c in self.columns:
            target = c + '_cat' if self.remain_numeric else c
            X[target] = X[c].astype(str)
        return X

    def fit_transform(self, X, y=None):
        return self.fit(X).transform(X)


class ColumnImputer:
    """SimpleImputer per column group: mean for continuous, '' / 0 constants for object / numeric categoricals
    (preprocessor.py:337-381)."""

    def __init__(self, continuous, obj_cats, num_cats):
        self.continuous, self.obj_cats, self.num_cats = list(continuous), list(obj_cats), list(num_cats)
        self.means_ = {}

    def fit(self, X, y=None):
        for c in self.continuous:
            col = pd.to_numeric(X[c], errors='coerce')
            self.means_[c] = float(col.mean()) if col.notna().any() else 0.0
        return self

    def transform(self, X):
        for c in self.continuous:
            X[c] = pd.to_numeric(X[c], errors='coerce').fillna(self.means_[c])
        for c in self.obj_cats:
            X[c] = X[c].astype(object).where(X[c].notna(), '')
        for c in self.num_cats:
            X[c] = X[c].fillna(0)
        return X

    def fit_transform(self, X, y=None):
        return self.fit(X).transform(X)


class MinMaxScalerTransformer:
    def __init__(self, columns):
        self.columns = list(columns)
        self.min_, self.range_ = {}, {}

    def fit(self, X, y=None):
        for c in self.columns:
            lo, hi = float(X[c].min()), float(X[c].max())
            self.min_[c], self.range_[c] = lo, (hi - lo) if hi > lo else 1.0
        return self

    def transform(self, X):
        for c in self.columns:
            X[c] = (X[c].astype('float64') - self.min_[c]) / self.range_[c]
        return X

    def fit_transform(self, X, y=None):
        return self.fit(X).transform(X)


class MultiLabelEncoder:
    """One safe label encoder per column: known values -> 0..n-1 (sorted by their string form), values unseen at
    fit time -> n.  n+1 <= nunique+2 = the column's vocabulary_size, so every id has an embedding row."""

    def __init__(self, columns):
        self.columns = list(columns)
        self.maps_ = {}

    def fit(self, X, y=None):
        for c in self.columns:
            values = sorted(pd.unique(X[c].astype(str)))
            self.maps_[c] = {v: i for i, v in enumerate(values)}
        return self

    def transform(self, X):
        for c in self.columns:
            m = self.maps_[c]
            X[c] = X[c].astype(str).map(m).fillna(len(m)).astype('int64')
        return X

    def fit_transform(self, X, y=None):
        return self.fit(X).transform(X)


class MultiKBinsDiscretizer:
    """Quantile bins per continuous column into a new ordinal column `<c>_discrete`
    (bins = min(nunique, 10) assumed; the reference takes the count from hypernets).  new_columns holds
    (name, new_name, bins) as preprocessor.py:410 expects."""

    def __init__(self, columns, max_bins=10):
        self.columns = list(columns)
        self.max_bins = max_bins
        self.new_columns = []
        self.edges_ = {}

    def fit(self, X, y=None):
        self.new_columns = []
        for c in self.columns:
            col = X[c].astype('float64')
            bins = int(max(2, min(self.max_bins, col.nunique())))
            edges = np.unique(np.quantile(col, np.linspace(0, 1, bins + 1)))
            self.edges_[c] = edges[1:-1]
            self.new_columns.append((c, c + '_discrete', len(edges) - 1 if len(edges) > 1 else 1))
        return self

    def transform(self, X):
        for c, new, _bins in self.new_columns:
            X[new] = np.searchsorted(self.edges_[c], X[c].astype('float64').values, side='right').astype('int64')
        return X

    def fit_transform(self, X, y=None):
        return self.fit(X).transform(X)


class MultiVarLenFeatureEncoder:
    """'a|b|c' strings -> zero-padded id lists of the column's max length; id 0 = padding / unseen, tokens 1..n
    (config.var_len_categorical_columns entries are (name, sep, pooling), config.py:138-144)."""

    def __init__(self, features):
        self.features = [(f[0], f[1]) for f in features]
        self.maps_, self.max_length_ = {}, {}

    @staticmethod
    def _split(v, sep):
        if v is None or (isinstance(v, float) and np.isnan(v)) or v == '':
            return []
        return [t for t in str(v).split(sep) if t != '']

    def fit(self, X, y=None):
        for name, sep in self.features:
            toks = [self._split(v, sep) for v in X[name]]
            vocab = sorted({t for row in toks for t in row})
            self.maps_[name] = {t: i + 1 for i, t in enumerate(vocab)}
            self.max_length_[name] = max([len(r) for r in toks] + [1])
        return self

    def transform(self, X):
        for name, sep in self.features:
            m, L = self.maps_[name], self.max_length_[name]
            rows = []
            for v in X[name]:
                ids = [m.get(t, 0) for t in self._split(v, sep)][:L]
                rows.append(np.asarray(ids + [0] * (L - len(ids)), dtype=np.int64))
            X[name] = rows
        return X

    def fit_transform(self, X, y=None):
        return self.fit(X).transform(X)

    def vocabulary_size(self, name):
        return len(self.maps_[name]) + 1


GBM_DEFAULTS = {'n_estimators': 100, 'num_leaves': 31, 'learning_rate': 0.1, 'max_bin': 255, 'min_child_samples': 20,
                'reg_lambda': 0.0, 'min_split_gain': 0.0}


def gbm_bin_edges(values, max_bin):
    """The ascending float64 bin edges of one feature (bin = the number of edges <= x, NaN -> the last bin): with at most
    `max_bin` distinct finite values the midpoints between neighbours (a midpoint that rounds onto its lower neighbour is moved to
    the upper one, so neighbours always part), otherwise the max_bin - 1 quantiles k / max_bin, deduplicated."""
    v = np.asarray(values, dtype=np.float64)
    u = np.unique(v[np.isfinite(v)])
    if len(u) <= max_bin:
        mid = (u[:-1] + u[1:]) / 2
        return np.where(mid > u[:-1], mid, u[1:])
    return np.unique(np.quantile(v[np.isfinite(v)], np.arange(1, max_bin) / max_bin))


class FeedRefusal(ValueError):
    """a condition under which a device path hands the call to the host path"""


def gbm_feed_edges(blocks, names, max_bin):
    """`gbm_bin_edges` of every column of the device blocks ([N, width] int32 / float32 tensors; names: one per column, for
    messages) without bringing a column to the host -> a list of float64 arrays.  `ops.column_profile` sorts a transposed copy
    of the blocks (the profile wants contiguous columns) with cap = max_bin + 1: one more than the rule needs, so that a column
    whose max_bin + 1 distinct keys hold both -0.0 and +0.0 — one value to np.unique — still gets its midpoints.  Columns with
    more values get np.quantile's 'linear' rule on order statistics (`ColumnProfile.order_stats`, 32 ranks per launch; the ranks
    are those of the non-NaN values: NaN fills sort first, so every rank moves up by the NaN count).  The host does float64
    arithmetic on at most 2 (max_bin - 1) values per column.  An infinite value raises and names the column: np.quantile over
    the finite values alone has no counterpart in the profile."""
    from .. import ops
    columns = [col for b in blocks for col in b.t().contiguous()]
    prof = ops.column_profile(columns, cap=max_bin + 1)
    prof.host()
    C, edges, wide = len(columns), [None] * len(columns), []
    for j, name in enumerate(names):
        lo, hi = prof.minimum(j), prof.maximum(j)
        if lo is not None and not (np.isfinite(np.float64(lo)) and np.isfinite(np.float64(hi))):
            raise FeedRefusal(f'apply_gbm_features: column {name!r} holds an infinite value; the in-feed fit takes finite values '
                              f'and NaN (fit_transform bins the finite ones)')
        d = prof.distinct(j)
        u = None if d is None else np.unique(d[0].astype(np.float64))
        if u is not None and len(u) <= max_bin:
            mid = (u[:-1] + u[1:]) / 2
            edges[j] = np.where(mid > u[:-1], mid, u[1:])
        else:
            wide.append(j)
    if wide:
        q = np.arange(1, max_bin) / max_bin
        ranks, gamma = np.full((C, 2 * len(q)), -1, dtype=np.int64), {}
        for j in wide:
            nans = int(prof.nan_count[j])
            n = prof.N - nans
            virtual = (n - 1) * q
            prev = np.floor(virtual)
            gamma[j] = virtual - prev
            ranks[j, :len(q)] = prev.astype(np.int64) + nans
            ranks[j, len(q):] = np.minimum(prev.astype(np.int64) + 1, n - 1) + nans
        R = ops.PROFILE_MAX_RANKS
        got = np.concatenate([prof.order_stats(ranks[:, s:s + R], np.nan) for s in range(0, ranks.shape[1], R)], axis=1)
        for j in wide:
            a, b, t = got[j, :len(q)], got[j, len(q):], gamma[j]
            diff = b - a
            edges[j] = np.unique(np.where(t >= 0.5, b - diff * (1 - t), a + diff * t))
    return edges


class GbmLeavesEncoder:
    """Stand-in for hypernets' LgbmLeavesEncoder (preprocessor.py:431-438): a gradient-boosted tree ensemble is fitted on the
    prepared categorical and continuous columns and every tree's leaf index becomes a new column `gbm_leaf_<t>`.  The trees are
    grown by this library's histogram GBDT on the GPU (ops.gbdt_*, csrc/gbdt.hip): LightGBM's algorithm in outline, NOT LightGBM
    and not compared with it.  Deviations: categorical codes are binned as ordinal integers (LightGBM partitions the categories);
    no row or column subsampling and no max_depth; binary log loss, L2 regression and, with `num_classes` = K in [3, 64], softmax
    cross-entropy with LightGBM's K / (K - 1) hessian factor: round t grows one tree per class, stored at index t K + c, and the
    new columns gbm_leaf_0 .. gbm_leaf_{T K - 1} are in that order (LightGBM's pred_leaf order).  The fitted state is numpy only."""

    MAX_CLASSES = 64                    # include/dt_hip.h DT_GBDT_MAX_CLASSES

    def __init__(self, cat_vars, cont_vars, task, num_classes=None, **gbm_params):
        unknown = sorted(set(gbm_params) - set(GBM_DEFAULTS))
        if unknown:
            raise ValueError(f'gbm_params: unsupported key(s) {unknown}; GbmLeavesEncoder takes {sorted(GBM_DEFAULTS)}')
        if task == consts.TASK_MULTICLASS and num_classes is None:
            raise ValueError(f'apply_gbm_features: task {task!r} needs num_classes (3 to {self.MAX_CLASSES}) to size one tree per '
                             f'class and round; only multilabel boosting remains a follow-up')
        if task not in (consts.TASK_BINARY, consts.TASK_REGRESSION, consts.TASK_MULTICLASS):
            raise ValueError(f'apply_gbm_features: task {task!r} is not supported; multilabel boosting is a follow-up, the GBM '
                             f'leaf features take binary, regression and multiclass')
        if task == consts.TASK_MULTICLASS and not 3 <= int(num_classes) <= self.MAX_CLASSES:
            raise ValueError(f'apply_gbm_features: num_classes must be in [3, {self.MAX_CLASSES}] for a multiclass task, got '
                             f'{num_classes} (two classes are the binary task)')
        self.cat_vars, self.cont_vars, self.task = list(cat_vars), list(cont_vars), task
        self.num_classes = np.int64(num_classes) if task == consts.TASK_MULTICLASS else None
        self.params = dict(GBM_DEFAULTS, **gbm_params)
        p = self.params
        if not 2 <= int(p['max_bin']) <= 255:
            raise ValueError(f"gbm_params: max_bin must be in [2, 255], got {p['max_bin']}")
        if int(p['n_estimators']) < 1 or int(p['num_leaves']) < 2 or int(p['min_child_samples']) < 0 or \
                float(p['reg_lambda']) < 0 or float(p['min_split_gain']) < 0:
            raise ValueError(f'gbm_params: n_estimators >= 1, num_leaves >= 2, min_child_samples, reg_lambda and min_split_gain >= 0: {p}')
        self.columns = self.cat_vars + self.cont_vars
        self.new_columns = []
        self.edges_ = None
        self.timings = None         # a dict: seconds per kernel role of the next fit (tools/gbm_bench.py)

    @staticmethod
    def _device():
        import torch
        from .._lib import DtHipError
        if not torch.cuda.is_available():
            raise DtHipError('deeptables_amd kernels run on the GPU only (apply_gbm_features fits its trees there); '
                             'there is deliberately no CPU fallback for the hot path.')
        return torch.device('cuda', torch.cuda.current_device())

    def _upload(self, X, device):
        """the feature columns as device tensors the binning kernel reads: int32 / int64 / float32 / float64 as they are,
        every other numeric dtype as float64"""
        import torch
        cols = []
        for c in self.columns:
            a = np.asarray(X[c].values)
            if a.dtype.kind not in 'biuf':
                raise ValueError(f'apply_gbm_features: column {c!r} has dtype {a.dtype}; the trees need numeric columns '
                                 f'(auto_encode_label encodes the categorical ones)')
            if a.dtype.name not in ('int32', 'int64', 'float32', 'float64'):
                a = a.astype(np.float64)
            cols.append(torch.from_numpy(np.ascontiguousarray(a)).to(device))
        return cols

    def _append(self, X, leaves):
        return pd.concat([X, pd.DataFrame(leaves, columns=self.new_columns, index=X.index)], axis=1)

    def fit_transform(self, X, y):
        import torch
        from .. import ops
        device = self._device()
        p = self.params
        T, L, N = int(p['n_estimators']), int(p['num_leaves']), len(X)
        if not self.columns or N < 1:
            raise ValueError('apply_gbm_features: no categorical or continuous column to fit the trees on')
        K = None if self.num_classes is None else int(self.num_classes)
        yv = np.asarray(y, dtype=np.float64).reshape(-1)
        init = self._init_score(yv)
        self.edges_ = [gbm_bin_edges(X[c].values, int(p['max_bin'])) for c in self.columns]
        bins = ops.gbdt_bin(self._upload(X, device), self.edges_)
        ws = ops.GbdtWorkspace(bins, L, num_classes=K)
        yd = torch.from_numpy(yv.astype(np.float32)).to(device)
        leaves = torch.empty((T * (K or 1), N), dtype=torch.int32, device=device)
        self._boost(bins, ws, yd, init, leaves)
        return self._append(X, leaves.t().contiguous().cpu().numpy())

    def _init_score(self, yv):
        """the score every row starts from: the log odds, the mean, or per class the log prior (a label outside [0, K)
        counts nowhere)"""
        if self.num_classes is not None:
            prior = np.array([(yv == c).mean() for c in range(int(self.num_classes))])
            return np.log(np.maximum(prior, 1e-15)).astype(np.float32)
        if self.task == consts.TASK_BINARY:
            pbar = min(max(float(yv.mean()), 1e-15), 1 - 1e-15)
            return np.float32(np.log(pbar / (1 - pbar)))
        return np.float32(yv.mean())

    def _boost(self, bins, ws, yd, init, leaves=None):
        """the boosting loop on the bin matrix and its workspace; the fitted state becomes numpy.  leaves: int32 [T (K), N] that
        receives every tree's leaf id per row (the host fit); None: one scratch row per class is reused (the in-feed fit walks
        the finished trees instead)"""
        import torch
        from .. import ops
        p, device, N = self.params, bins.device, bins.shape[1]
        T, L = int(p['n_estimators']), int(p['num_leaves'])
        objective = 'binary' if self.task == consts.TASK_BINARY else 'regression'
        i32 = dict(dtype=torch.int32, device=device)
        if self.num_classes is not None:
            return self._boost_softmax(bins, ws, yd, init, leaves)
        scratch = torch.empty(N, **i32) if leaves is None else None
        kernel_timings = self.timings if leaves is not None else None       # the in-feed fit reports whole roles (fit_feed)
        scores = torch.full((N,), float(init), dtype=torch.float32, device=device)
        trees = {'node_feat': torch.empty((T, L - 1), **i32), 'node_bin': torch.empty((T, L - 1), **i32),
                 'node_child': torch.empty((T, L - 1, 2), **i32), 'n_nodes': torch.empty(T, **i32),
                 'leaf_value': torch.empty((T, L), dtype=torch.float32, device=device)}
        sexp = torch.empty((T, 2), **i32)
        max_bits = torch.zeros(T, dtype=torch.int64, device=device)
        grads = (torch.empty(N, **i32), torch.empty(N, **i32))
        grow = {k: p[k] for k in ('num_leaves', 'min_child_samples', 'reg_lambda', 'min_split_gain', 'learning_rate')}
        for t in range(T):              # launches only: the scale and the choice of leaves stay on the device
            qg, qh, s = ops.gbdt_gradients(scores, yd, objective, max_slot=max_bits[t:t + 1], out=grads + (sexp[t],))
            out = {k: (v[t:t + 1] if k == 'n_nodes' else v[t]) for k, v in trees.items()}
            out['row_leaf'] = scratch if leaves is None else leaves[t]
            ops.gbdt_grow_tree(bins, qg, qh, dict(grow, sexp=s), workspace=ws, scores=scores, out=out, timings=kernel_timings)
        self._keep_trees(trees, sexp, init)

    def _keep_trees(self, trees, sexp, init):
        """the fitted state, numpy only (one read-back per tree array)"""
        t0 = self._role(None, 0.0, sexp.device)
        for k, v in trees.items():
            setattr(self, k + '_', v.cpu().numpy())
        self.scale_exponents_ = sexp.cpu().numpy()
        self.init_score_ = init
        self.new_columns = [f'gbm_leaf_{j}' for j in range(len(self.n_nodes_))]
        self._role('state_readback', t0, sexp.device)

    def _boost_softmax(self, bins, ws, yd, init, leaves):
        """the boosting loop of a multiclass task: per round one gradient launch over the class-major scores [K, N] and the
        launches of one tree, which grow the K class trees in lock-step into rows t K .. t K + K - 1 of the tree arrays"""
        import torch
        from .. import ops
        p, K, N, device = self.params, int(self.num_classes), bins.shape[1], bins.device
        T, L = int(p['n_estimators']), int(p['num_leaves'])
        i32 = dict(dtype=torch.int32, device=device)
        scores = torch.from_numpy(init).to(device)[:, None].expand(K, N).contiguous()
        trees = {'node_feat': torch.empty((T * K, L - 1), **i32), 'node_bin': torch.empty((T * K, L - 1), **i32),
                 'node_child': torch.empty((T * K, L - 1, 2), **i32), 'n_nodes': torch.empty(T * K, **i32),
                 'leaf_value': torch.empty((T * K, L), dtype=torch.float32, device=device)}
        scratch = torch.empty((K, N), **i32) if leaves is None else None
        kernel_timings = self.timings if leaves is not None else None
        sexp = torch.empty((T, 2), **i32)
        grads = (torch.empty((K, N), **i32), torch.empty((K, N), **i32))
        grow = {k: p[k] for k in ('num_leaves', 'min_child_samples', 'reg_lambda', 'min_split_gain', 'learning_rate')}
        for t in range(T):
            qg, qh, s = ops.gbdt_gradients_softmax(scores, yd, K, out=grads + (sexp[t],))
            out = {k: v[t * K:(t + 1) * K] for k, v in trees.items()}
            out['row_leaf'] = scratch if leaves is None else leaves[t * K:(t + 1) * K]
            ops.gbdt_grow_trees(bins, qg, qh, dict(grow, sexp=s), workspace=ws, scores=scores, out=out, timings=kernel_timings)
        self._keep_trees(trees, sexp, init)

    def fit(self, X, y):
        self.fit_transform(X, y)
        return self

    def transform(self, X):
        import torch
        from .. import ops
        if self.edges_ is None:
            raise ValueError('GbmLeavesEncoder is not fitted')
        device = self._device()
        if len(X) == 0:
            return self._append(X, np.zeros((0, len(self.new_columns)), dtype=np.int32))
        cols = self._upload(X, device)
        if getattr(self, 'feed_fitted_', False):        # the edges come from a feed's float32 values: bin what a feed would hold
            cols = [c.to(torch.float32) if name in self.cont_vars else c for name, c in zip(self.columns, cols)]
        packed = ops.gbdt_pack(ops.gbdt_bin(cols, self.edges_))
        return self._append(X, ops.gbdt_predict_leaves(packed, self._device_trees(device), int(self.params['num_leaves'])).cpu().numpy())

    def _device_trees(self, device):
        import torch
        return {k: torch.from_numpy(getattr(self, k + '_')).to(device) for k in ('node_feat', 'node_bin', 'node_child', 'n_nodes')}

    # -- inside a resident feed: the features are the columns of the id block and of the continuous blocks, where they lie ----
    def _feed_features(self, blocks, kinds):
        ids = next((b for b, k in zip(blocks, kinds) if k == 'cat'), None)
        conts = [b for b, k in zip(blocks, kinds) if k == 'cont']
        if (0 if ids is None else ids.shape[1]) != len(self.cat_vars) or sum(b.shape[1] for b in conts) != len(self.cont_vars):
            raise ValueError(f'GbmLeavesEncoder: the feed holds {0 if ids is None else ids.shape[1]} id and '
                             f'{sum(b.shape[1] for b in conts)} continuous columns, the encoder {len(self.cat_vars)} and '
                             f'{len(self.cont_vars)}')
        return ids, conts

    def feed_bytes(self, n_rows, feature_type):
        """device bytes the in-feed fit and transform hold besides the feed's blocks: both bin matrices, the widened block,
        and (fit) the profile's transposed columns with the sort's two key buffers"""
        P, T = len(self.columns), int(self.params['n_estimators']) * int(self.num_classes or 1)
        wide = len(self.cat_vars) + T if feature_type == consts.GBM_FEATURE_TYPE_EMB else T
        return int(n_rows) * (2 * ((P + 7) // 8 * 8) + 4 * wide), int(n_rows) * 20 * P

    def _widen(self, blocks, kinds, packed, feature_type, device):
        """the leaf launch: the id block grows by the leaf columns, or one float block of leaf ids joins the end"""
        from .. import ops
        blocks, kinds = list(blocks), list(kinds)
        L, trees = int(self.params['num_leaves']), self._device_trees(device)
        if feature_type == consts.GBM_FEATURE_TYPE_EMB:
            at = kinds.index('cat') if 'cat' in kinds else None
            wide = ops.gbdt_leaves_feed(packed, trees, L, 'embedding', ids=None if at is None else blocks[at])
            if at is None:
                blocks.insert(0, wide)
                kinds.insert(0, 'cat')
            else:
                blocks[at] = wide
        else:
            blocks.append(ops.gbdt_leaves_feed(packed, trees, L, 'dense'))
            kinds.append('cont')
        return blocks, kinds

    def _role(self, role, t0, device):
        """with `timings`: drain the device and add the seconds since t0 to `role` (None: only start the clock)"""
        import torch
        if getattr(self, 'timings', None) is not None:
            torch.cuda.synchronize(device)
            if role is not None:
                self.timings[role] = self.timings.get(role, 0.0) + time.perf_counter() - t0
        return time.perf_counter()

    def fit_feed(self, blocks, kinds, y, feature_type=consts.GBM_FEATURE_TYPE_EMB):
        """`fit_transform` on the blocks of a resident feed (`DefaultPreprocessor.feed_blocks`): the edges from a device profile
        of the blocks' columns (`gbm_feed_edges`), one binning launch over the blocks (ops.gbdt_bin_feed), the boosting loop,
        one leaf launch (ops.gbdt_leaves_feed).  y: the encoded targets (class numbers), uploaded once; nothing else of size N
        crosses the bus and only the fitted trees come back.  -> the widened (blocks, kinds)"""
        import torch
        from .. import ops
        p = self.params
        ids, conts = self._feed_features(blocks, kinds)
        if not self.columns or blocks[0].shape[0] < 1:
            raise ValueError('apply_gbm_features: no categorical or continuous column to fit the trees on')
        device = blocks[0].device
        K = None if self.num_classes is None else int(self.num_classes)
        yv = np.asarray(y, dtype=np.float64).reshape(-1)
        t0 = self._role(None, 0.0, device)
        self.edges_ = gbm_feed_edges(([ids] if ids is not None else []) + conts, self.columns, int(p['max_bin']))
        t0 = self._role('profile_edges', t0, device)
        bins, packed = ops.gbdt_bin_feed(ids, conts, self.edges_)
        t0 = self._role('bin_launch', t0, device)
        ws = ops.GbdtWorkspace(bins, int(p['num_leaves']), num_classes=K, packed=packed)
        self._boost(bins, ws, torch.from_numpy(yv.astype(np.float32)).to(device), self._init_score(yv))
        self.feed_fitted_ = True
        t0 = self._role('boosting_loop', t0, device)
        if self.timings is not None:                            # (_keep_trees timed its read-back inside the loop's span)
            self.timings['boosting_loop'] -= self.timings.get('state_readback', 0.0)
        out = self._widen(blocks, kinds, packed, feature_type, device)
        self._role('leaf_launch', t0, device)
        return out

    def transform_feed(self, blocks, kinds, feature_type=consts.GBM_FEATURE_TYPE_EMB):
        """the blocks of a feed -> the widened (blocks, kinds): one binning launch, one leaf launch"""
        from .. import ops
        if self.edges_ is None or not getattr(self, 'feed_fitted_', False):
            raise ValueError('GbmLeavesEncoder.transform_feed: the encoder was not fitted by fit_feed')
        ids, conts = self._feed_features(blocks, kinds)
        tabs = getattr(self, '_edge_tabs', None)                # the edge tables stay on the device between calls
        if tabs is None or tabs[0].device != blocks[0].device:
            tabs = self._edge_tabs = ops.gbdt_edge_table(self.edges_, blocks[0].device)
        _bins, packed = ops.gbdt_bin_feed(ids, conts, tabs[0], tabs[1])
        return self._widen(blocks, kinds, packed, feature_type, blocks[0].device)

    def __getstate__(self):
        state = dict(self.__dict__)
        state.pop('_edge_tabs', None)                           # device tensors never travel
        return state

    def raw_scores(self, leaves):
        """the ensemble's raw scores (logits / predictions) float32 [N] of rows whose leaf ids [N, T] are given; a multiclass
        encoder: float32 [N, K] from the leaf ids [N, T K], tree j adding to class j mod K"""
        if getattr(self, 'num_classes', None) is not None:
            K = int(self.num_classes)
            s = np.tile(np.asarray(self.init_score_, dtype=np.float32), (len(leaves), 1))
            for j in range(leaves.shape[1]):
                s[:, j % K] = s[:, j % K] + self.leaf_value_[j][np.asarray(leaves)[:, j]]
            return s
        s = np.full(len(leaves), self.init_score_, dtype=np.float32)
        for t in range(leaves.shape[1]):
            s = s + self.leaf_value_[t][np.asarray(leaves)[:, t]]
        return s


class LabelEncoder:
    def fit(self, y):
        self.classes_ = np.asarray(sorted(pd.unique(pd.Series(np.asarray(y).ravel()))))
        self._map = {v: i for i, v in enumerate(self.classes_)}
        return self

    def transform(self, y):
        s = pd.Series(np.asarray(y).ravel()).map(self._map)
        if s.isna().any():
            raise ValueError('y contains previously unseen labels')
        return s.values.astype('int64')

    def fit_transform(self, y):
        return self.fit(y).transform(y)

    def inverse_transform(self, idx):
        return self.classes_[np.asarray(idx).astype('int64')]


def infer_task_type(y):
    """hypernets' toolbox rule as used by preprocessor.py:208-209: float targets with many values -> regression,
    two classes -> binary, otherwise multiclass."""
    ys = pd.Series(np.asarray(y).ravel())
    n = ys.nunique()
    if ys.dtype.kind == 'f' and n > 2 and not np.all(np.mod(ys.dropna(), 1) == 0):
        return consts.TASK_REGRESSION, []
    if ys.dtype.kind in 'fiu' and n > 100:
        return consts.TASK_REGRESSION, []
    labels = sorted(ys.dropna().unique())
    return (consts.TASK_BINARY if n == 2 else consts.TASK_MULTICLASS), labels


# ---------------------------------------------------------------------------------------------
# the device path of transform: which columns the kernel serves and with which constants (ops.prep_transform)
# ---------------------------------------------------------------------------------------------
TIMINGS = None                      # a dict: the phases of the next transform_feed calls are timed into it (tools/transform_bench.py)


class _Phase:
    """adds the wall time of a `with` block to TIMINGS[name], the device drained at both ends; free when TIMINGS is None"""

    def __init__(self, name, device):
        self.name, self.device = name, device

    def _drain(self):
        import torch
        if torch.device(self.device).type == 'cuda':
            torch.cuda.synchronize(self.device)

    def __enter__(self):
        if TIMINGS is not None:
            self._drain()
            self.t0 = time.perf_counter()

    def __exit__(self, *exc):
        if TIMINGS is not None:
            self._drain()
            TIMINGS[self.name] = TIMINGS.get(self.name, 0.0) + time.perf_counter() - self.t0


def served_dtype(dtype):
    """a plain numpy dtype the transform kernel reads: bool, (u)int8..64, float32, float64"""
    return isinstance(dtype, np.dtype) and ((dtype.kind in 'biu' and dtype.itemsize <= 8) or
                                            (dtype.kind == 'f' and dtype.itemsize in (4, 8)))


def distinct_raw_values(values):
    """the distinct values of a numeric array BY BIT PATTERN, every NaN one value (-0.0 and 0.0 stay two: `astype(str)` tells
    them apart, `pd.unique` does not) -> an array of the same dtype"""
    a = np.ascontiguousarray(values)
    if a.dtype.kind != 'f':
        return np.unique(a)
    bits = a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64).copy()
    bits[np.isnan(a)] = np.array(np.nan, dtype=a.dtype).view(bits.dtype)
    return np.unique(bits).view(a.dtype)


class DeviceOutput:
    """One column of a feed block as the device path makes it: `name` (the transformed column), `source` (the prepared raw
    column it is computed from), `op` ('lookup' / 'cont' / 'bin' / 'copy') and the operation's host-side constants."""
    __slots__ = ('name', 'source', 'op', 'keys', 'ids', 'miss', 'edges', 'fill', 'min', 'range', 'flags')

    def __init__(self, name, source, op, keys=None, ids=None, miss=0, edges=None, fill=0.0, min=0.0, range=1.0, flags=0):
        self.name, self.source, self.op, self.keys, self.ids, self.miss = name, source, op, keys, ids, miss
        self.edges, self.fill, self.min, self.range, self.flags = edges, fill, min, range, flags


class DevicePlan:
    """What `DefaultPreprocessor.transform_feed` needs beyond the fitted steps, built once per fitted preprocessor on the host:
      cat      [DeviceOutput] in `categorical_columns` order (None: the model has no id block)
      conts    [[DeviceOutput]] per ContinuousColumn
      var      the var-len column names (always host-served)
      refused  {raw column: why the kernel cannot serve it whatever the frame} (dtype at fit, constants)
      whole    None, or why no frame can take the device path
    `partition(X)` adds the frame's own reasons (a dtype other than at fit) and leaves the result in `host_columns`.
    Tables and edges are uploaded once per device and kept in `_resident`; nothing of a plan is pickled."""

    def __init__(self):
        self.cat, self.conts, self.var, self.refused, self.whole = None, [], [], {}, None
        self.sources, self.host_columns, self.device_columns, self.fit_dtypes = [], [], [], {}
        self._resident = {}

    def outputs(self):
        return list(self.cat or []) + [o for blk in self.conts for o in blk]

    def partition(self, X):
        """(device-served, host-served) raw columns of the prepared frame X, each in `sources` order"""
        dev, host = [], []
        for c in self.sources:
            why = self.refused.get(c)
            if why is None and X[c].dtype != self.fit_dtypes[c]:
                why = f'dtype {X[c].dtype} in this frame, {self.fit_dtypes[c]} at fit'
            (dev if why is None else host).append(c)
        self.device_columns, self.host_columns = dev, host
        return dev, host

    def resident(self, device):
        """{(output name, 'keys' / 'ids' / 'edges'): tensor on `device`}, uploaded on first use"""
        import torch
        key = str(torch.device(device))
        if key not in self._resident:
            tabs = {}
            for o in self.outputs():
                if o.op == 'lookup':
                    tabs[o.name, 'keys'] = torch.from_numpy(o.keys.view(np.int64)).to(device)
                    tabs[o.name, 'ids'] = torch.from_numpy(o.ids).to(device)
                elif o.op == 'bin':
                    tabs[o.name, 'edges'] = torch.from_numpy(o.edges).to(device)
            self._resident[key] = tabs
        return self._resident[key]


# ---------------------------------------------------------------------------------------------
# preprocessors
# ---------------------------------------------------------------------------------------------
class AbstractPreprocessor:
    def __init__(self, config: ModelConfig):
        self.config = config
        self.labels_ = None
        self.task_ = None

    @property
    def pos_label(self):
        if self.labels_ is not None and len(self.labels_) == 2:
            return self.labels_[1]
        return None

    @property
    def labels(self):
        return self.labels_

    @property
    def task(self):
        return self.task_

    def fit_transform(self, X, y, copy_data=True):
        raise NotImplementedError

    def transform_X(self, X, copy_data=True):
        raise NotImplementedError

    def transform_y(self, y, copy_data=True):
        raise NotImplementedError

    def transform(self, X, y, copy_data=True):
        raise NotImplementedError

    def inverse_transform_y(self, y_indicator):
        raise NotImplementedError

    def get_categorical_columns(self):
        raise NotImplementedError

    def get_continuous_columns(self):
        raise NotImplementedError


class DefaultPreprocessor(AbstractPreprocessor):
    def __init__(self, config: ModelConfig):
        super().__init__(config)
        self.reset()

    def reset(self):
        self.metainfo = None
        self.categorical_columns = None
        self.var_len_categorical_columns = None
        self.continuous_columns = None
        self.y_lable_encoder = None
        self.X_transformers = collections.OrderedDict()
        self.raw_columns_ = None            # {column label as given to fit: its name after _prepare_X}
        self.fit_dtypes_ = None             # {prepared column: its dtype at fit}
        self.raw_keys_ = None               # {numeric column that feeds a label-encoded output: its distinct raw values at fit}
        self._device_plan = None            # DevicePlan, built on first use; never pickled

    # -- validation / preparation (preprocessor.py:116-157) ---------------------------------------
    def _validate_fit_transform(self, X, y):
        if X is None:
            raise ValueError('X cannot be none.')
        if y is None:
            raise ValueError('y cannot be none.')
        if len(X.shape) != 2:
            raise ValueError('X must be a 2D datasets.')
        if X.shape[0] != np.shape(y)[0]:
            raise ValueError(f'The number of samples of X and y must be the same. X.shape:{X.shape}, '
                             f'y.shape{np.shape(y)}')
        if pd.DataFrame(y).isnull().sum().sum() > 0:
            raise ValueError('Missing values in y.')

    def _prepare_X(self, X):
        if not isinstance(X, pd.DataFrame):
            X = pd.DataFrame(X)
        if len(set(X.columns)) != len(list(X.columns)):
            cols = [item for item, count in collections.Counter(X.columns).items() if count > 1]
            raise ValueError(f'Columns with duplicate names in X: {cols}')
        if X.columns.dtype != 'object':
            X.columns = ['x_' + str(c) for c in X.columns]
        return X

    # -- fit ----------------------------------------------------------------------------------------
    def fit_transform(self, X, y, copy_data=True):
        self.reset()
        self._validate_fit_transform(X, y)
        X = copy.deepcopy(X)
        y = copy.deepcopy(y)
        y = self.fit_transform_y(y)
        if not isinstance(X, pd.DataFrame):
            X = pd.DataFrame(X)
        raw = list(X.columns)
        X = self._prepare_X(X)
        self.raw_columns_ = dict(zip(raw, X.columns))
        self.fit_dtypes_ = {c: X[c].dtype for c in X.columns}
        raw_values = {c: X[c].values for c in X.columns if served_dtype(X[c].dtype)}     # before any step rewrites a column
        X = self._prepare_features(X)
        self._record_raw_keys(raw_values)
        if self.config.auto_imputation:
            X = self._imputation(X)
        if self.config.auto_scale:
            X = self._standard_scale(X)
        if self.config.auto_encode_label:
            X = self._categorical_encoding(X)
        if self.config.auto_discrete:
            X = self._discretization(X)
        if self.config.apply_gbm_features:
            X = self._apply_gbm_features(X, y)
        var_len = self.config.var_len_categorical_columns
        if var_len is not None and len(var_len) > 0:
            X = self._var_len_encoder(X, var_len)
        self.X_transformers['last'] = PassThroughEstimator()
        cont_cols = self.get_continuous_columns()
        if len(cont_cols) > 0:
            X[cont_cols] = X[cont_cols].astype('float')
        return X, y

    def fit_transform_y(self, y):
        if self.config.task == consts.TASK_AUTO:
            self.task_, self.labels_ = infer_task_type(y)
        else:
            self.task_ = self.config.task
        if self.task_ in [consts.TASK_BINARY, consts.TASK_MULTICLASS]:
            self.y_lable_encoder = LabelEncoder()
            y = self.y_lable_encoder.fit_transform(y)
            self.labels_ = self.y_lable_encoder.classes_
        elif self.task_ == consts.TASK_MULTILABEL:
            self.labels_ = list(range(np.shape(y)[-1]))
        else:
            self.labels_ = []
            y = np.asarray(y)
        return y

    # -- transform ------------------------------------------------------------------------------------
    def transform(self, X, y, copy_data=True):
        return self.transform_X(X, copy_data), self.transform_y(y, copy_data)

    def transform_y(self, y, copy_data=True):
        if self.y_lable_encoder is not None:
            return self.y_lable_encoder.transform(y)
        return np.asarray(y)

    def transform_X(self, X, copy_data=True):
        if copy_data:
            X = copy.deepcopy(X)
        X = self._prepare_X(X)
        for step in self.X_transformers.values():
            X = step.transform(X)
        cont_cols = self.get_continuous_columns()
        if len(cont_cols) > 0:
            X[cont_cols] = X[cont_cols].astype('float')
        return X

    def inverse_transform_y(self, y_indicator):
        if self.y_lable_encoder is not None:
            return self.y_lable_encoder.inverse_transform(y_indicator)
        return y_indicator

    # -- steps ----------------------------------------------------------------------------------------
    def _prepare_features(self, X, nuniques=None):
        """Column typing, preprocessor.py:267-336.  nuniques ({column: nunique}, the device fit): the counts are taken from
        it and the CategorizeEncoder is sized without being run on X."""
        num_vars, convert2cat_vars, cat_vars = [], [], []
        if self.config.cat_exponent >= 1:
            raise ValueError(f'"cat_exponent" must be less than 1, not {self.config.cat_exponent} .')
        var_len = self.config.var_len_categorical_columns
        var_len_sep = {}
        if var_len is not None and len(var_len) > 0:
            for v in var_len:
                if not isinstance(v, (tuple, list)) or len(v) != 3:
                    raise ValueError('Var len column config should be a tuple 3.')
                var_len_sep[v[0]] = v[1]
        unique_upper_limit = round(X.shape[0] ** self.config.cat_exponent)
        for c in X.columns:
            nunique = X[c].nunique() if nuniques is None else int(nuniques[c])
            dtype = str(X[c].dtype)
            if nunique <= 1 and self.config.auto_discard_unique:
                continue
            if c in (self.config.exclude_columns or []):
                continue
            if c in var_len_sep:
                self._append_var_len_categorical_col(c, nunique, var_len_sep[c])
                continue
            cc = self.config.categorical_columns
            if cc is not None and isinstance(cc, list):
                if c in cc:
                    cat_vars.append((c, dtype, nunique))
                elif np.issubdtype(X[c].dtype, np.number):
                    num_vars.append((c, dtype, nunique))
            else:
                if dtype in ('object', 'category', 'bool') or dtype.startswith('str'):
                    cat_vars.append((c, dtype, nunique))
                elif self.config.auto_categorize and nunique < unique_upper_limit:
                    convert2cat_vars.append((c, dtype, nunique))
                else:
                    num_vars.append((c, dtype, nunique))
        if len(convert2cat_vars) > 0:
            ce = CategorizeEncoder([c for c, d, n in convert2cat_vars], self.config.cat_remain_numeric)
            if nuniques is None:
                X = ce.fit_transform(X)
            else:
                ce.fit_counts(nuniques)
            self.X_transformers['categorize'] = ce
            if self.config.cat_remain_numeric:
                cat_vars = cat_vars + ce.new_columns
                num_vars = num_vars + convert2cat_vars
            else:
                cat_vars = cat_vars + convert2cat_vars
        self._append_categorical_cols([(c[0], c[2] + 2) for c in cat_vars])
        self._append_continuous_cols([c[0] for c in num_vars], consts.INPUT_PREFIX_NUM + 'all')
        return X

    def _imputation(self, X):
        obj_cats, num_cats = [], []
        for c in self.get_categorical_columns() + self.get_var_len_categorical_columns():
            dtype = str(X[c].dtype)
            (obj_cats if dtype.startswith('obj') or dtype.startswith('str') or dtype == 'category'
             else num_cats).append(c)
        imp = ColumnImputer(self.get_continuous_columns(), obj_cats, num_cats)
        X = imp.fit_transform(X)
        self.X_transformers['imputation'] = imp
        return X

    def _categorical_encoding(self, X):
        mle = MultiLabelEncoder(self.get_categorical_columns())
        X = mle.fit_transform(X)
        self.X_transformers['label_encoder'] = mle
        return X

    def _standard_scale(self, X):
        ss = MinMaxScalerTransformer(self.get_continuous_columns())
        X = ss.fit_transform(X)
        self.X_transformers['standard_scale'] = ss
        return X

    def _discretization(self, X):
        mkbd = MultiKBinsDiscretizer(self.get_continuous_columns())
        X = mkbd.fit_transform(X)
        self._append_categorical_cols([(new_name, bins + 1) for name, new_name, bins in mkbd.new_columns])
        self.X_transformers['discreter'] = mkbd
        return X

    def _gbm_encoder(self):
        return GbmLeavesEncoder(self.get_categorical_columns(), self.get_continuous_columns(), self.task_,
                                num_classes=len(self.labels_) if self.task_ == consts.TASK_MULTICLASS else None,
                                **(self.config.gbm_params or {}))

    def _apply_gbm_features_feed(self, enc, blocks, kinds, y):
        """`_apply_gbm_features` on the blocks of the training feed: the same step name, column names, order and
        gbm_feature_type handling; the vocabulary of leaf column t is its tree's leaf count n_nodes + 1 (every leaf holds a
        training row, so this is the host's max + 1).  The step goes where fit_transform puts it: before the var-len encoder.
        -> the widened (blocks, kinds)"""
        kind = self.config.gbm_feature_type
        blocks, kinds = enc.fit_feed(blocks, kinds, y, kind)
        self.X_transformers['gbm_features'] = enc
        for later in ('var_len_encoder', 'last'):
            if later in self.X_transformers:
                self.X_transformers.move_to_end(later)
        if kind == consts.GBM_FEATURE_TYPE_EMB:
            self._append_categorical_cols([(name, int(n) + 1) for name, n in zip(enc.new_columns, enc.n_nodes_)])
        else:
            self._append_continuous_cols(enc.new_columns, consts.INPUT_PREFIX_NUM + 'gbm_leaves')
        return blocks, kinds

    def _apply_gbm_features(self, X, y):
        """preprocessor.py:431-445 with GbmLeavesEncoder: the leaf columns join the categorical columns (vocabulary max + 1) or
        form one continuous block"""
        enc = self._gbm_encoder()
        X = enc.fit_transform(X, y)
        self.X_transformers['gbm_features'] = enc
        if self.config.gbm_feature_type == consts.GBM_FEATURE_TYPE_EMB:
            self._append_categorical_cols([(name, int(X[name].max()) + 1) for name in enc.new_columns])
        else:
            self._append_continuous_cols(enc.new_columns, consts.INPUT_PREFIX_NUM + 'gbm_leaves')
        return X

    def _var_len_encoder(self, X, var_len_categorical_columns):
        transformer = MultiVarLenFeatureEncoder(var_len_categorical_columns)
        X = transformer.fit_transform(X)
        updated = []
        for c in self.var_len_categorical_columns:
            # the column was sized from nunique of the raw strings; the table must cover the TOKEN vocabulary
            vc = VarLenCategoricalColumn(c.name, max(c.vocabulary_size, transformer.vocabulary_size(c.name)),
                                         c.embeddings_output_dim, sep=c.sep)
            vc.max_elements_length = transformer.max_length_[c.name]
            updated.append(vc)
        self.var_len_categorical_columns = updated
        self.X_transformers['var_len_encoder'] = transformer
        return X

    # -- column metadata (preprocessor.py:452-515) ----------------------------------------------------
    def _embedding_dim(self, voc_size):
        if self.config.fixed_embedding_dim:
            d = self.config.embeddings_output_dim if self.config.embeddings_output_dim > 0 \
                else consts.EMBEDDING_OUT_DIM_DEFAULT
            return d
        return min(4 * int(pow(voc_size, 0.25)), 20)

    def _append_var_len_categorical_col(self, name, voc_size, sep):
        if self.var_len_categorical_columns is None:
            self.var_len_categorical_columns = []
        self.var_len_categorical_columns.append(
            VarLenCategoricalColumn(name, voc_size, self._embedding_dim(voc_size), sep=sep))

    def _append_categorical_cols(self, cols):
        if self.categorical_columns is None:
            self.categorical_columns = []
        if cols is not None and len(cols) > 0:
            self.categorical_columns = self.categorical_columns + \
                [CategoricalColumn(name, voc_size, self._embedding_dim(voc_size)) for name, voc_size in cols]

    def _append_continuous_cols(self, cols, input_name):
        if self.continuous_columns is None:
            self.continuous_columns = []
        if cols is not None and len(cols) > 0:
            self.continuous_columns = self.continuous_columns + \
                [ContinuousColumn(name=input_name, column_names=[c for c in cols])]

    # -- the device path: raw frame -> resident feed (ops.prep_transform, csrc/prep_transform.hip) -------------------------
    def __getstate__(self):
        state = dict(self.__dict__)
        state['_device_plan'] = None                # host tables are rebuilt, device tensors never travel
        return state

    def _record_raw_keys(self, raw_values):
        """raw_keys_: the distinct raw values of every served-dtype column that feeds a label-encoded output — a categorical
        column itself, or the source of a `<c>_cat` copy.  One np.unique each; continuous-only columns record nothing."""
        self.raw_keys_ = {}
        if not self.config.auto_encode_label:
            return
        ce = self.X_transformers.get('categorize')
        wanted = set(self.get_categorical_columns()) | set(ce.columns if ce is not None else [])
        for c, values in raw_values.items():
            if c in wanted:
                self.raw_keys_[c] = distinct_raw_values(values)

    def _output_sources(self):
        """{transformed column: the prepared raw column it is computed from}"""
        src, derived = {}, self.source_columns()
        for raw, prepared in self.raw_columns_.items():
            for name in derived[raw]:
                src[name] = prepared
        return src

    def _replay_host(self, X, cols):
        """The fitted steps on a frame holding only the raw columns `cols`: `transform_X` with each step's column lists
        restricted to those columns and what derives from them.  X is rewritten."""
        cols = set(cols)
        avail = set(cols)
        for name, source in self._output_sources().items():
            if source in cols:
                avail.add(name)
        for step in self.X_transformers.values():
            s = copy.copy(step)
            if isinstance(step, CategorizeEncoder):
                s.columns = [c for c in step.columns if c in cols]
            elif isinstance(step, ColumnImputer):
                s.continuous = [c for c in step.continuous if c in avail]
                s.obj_cats = [c for c in step.obj_cats if c in avail]
                s.num_cats = [c for c in step.num_cats if c in avail]
            elif isinstance(step, (MinMaxScalerTransformer, MultiLabelEncoder)):
                s.columns = [c for c in step.columns if c in avail]
            elif isinstance(step, MultiKBinsDiscretizer):
                s.new_columns = [t for t in step.new_columns if t[0] in cols]
            elif isinstance(step, MultiVarLenFeatureEncoder):
                s.features = [f for f in step.features if f[0] in cols]
            elif isinstance(step, GbmLeavesEncoder):
                continue                                # its columns derive from ALL columns: the feed adds them (transform_feed)
            elif not isinstance(step, PassThroughEstimator):
                raise ValueError(f'_replay_host: unknown step {type(step).__name__}')
            X = s.transform(X)
        cont_cols = [c for c in self.get_continuous_columns() if c in cols]
        if len(cont_cols) > 0:
            X[cont_cols] = X[cont_cols].astype('float')
        return X

    def device_plan(self):
        """The DevicePlan of this fitted preprocessor (built once, on the host)."""
        if getattr(self, '_device_plan', None) is not None:
            return self._device_plan
        if getattr(self, 'raw_columns_', None) is None or getattr(self, 'fit_dtypes_', None) is None or \
                getattr(self, 'raw_keys_', None) is None:
            raise ValueError('device_plan: the preprocessor is not fitted, or was fitted before it recorded fit_dtypes_ / raw_keys_')
        plan = DevicePlan()
        plan.fit_dtypes = dict(self.fit_dtypes_)
        sources = self._output_sources()
        steps = self.X_transformers
        imp, ss, mle, mkbd = (steps.get(k) for k in ('imputation', 'standard_scale', 'label_encoder', 'discreter'))
        discrete = {new: c for c, new, _b in mkbd.new_columns} if mkbd is not None else {}
        plan.var = self.get_var_len_categorical_columns()
        for c in plan.var:
            plan.refused[c] = 'a var-len column'

        def refuse(c, why):
            plan.refused.setdefault(c, why)

        def cont_constants(c):
            dtype = self.fit_dtypes_[c]
            kw = dict(flags=0, fill=0.0, min=0.0, range=1.0)
            if imp is not None and c in imp.continuous and dtype.kind == 'f':
                mean = float(imp.means_[c])
                if dtype.itemsize == 4 and not float(np.float32(mean)) == mean:
                    refuse(c, 'float32 column whose fitted mean is not a float32: pandas widens the column when it fills')
                kw.update(flags=1, fill=mean)
            if ss is not None and c in ss.columns:
                kw.update(flags=kw['flags'] | 2, min=float(ss.min_[c]), range=float(ss.range_[c]))
            return kw

        gbm = steps.get('gbm_features')                 # its leaf columns are made from the finished blocks, not by the plan
        leaf_names = set(gbm.new_columns) if gbm is not None else set()
        names = [n for n in self.get_categorical_columns() if n not in leaf_names]
        outs = []
        for name in names:
            c = sources.get(name, name)
            dtype = self.fit_dtypes_.get(c)
            if not served_dtype(dtype):
                refuse(c, f'dtype {dtype} at fit')
                outs.append(DeviceOutput(name, c, 'copy'))
            elif name in discrete:
                edges = np.ascontiguousarray(mkbd.edges_[c], dtype=np.float64)
                if np.isnan(edges).any():
                    refuse(c, 'NaN among the quantile edges')
                outs.append(DeviceOutput(name, c, 'bin', edges=edges, **cont_constants(c)))
            elif mle is not None and name in mle.columns:
                if c not in self.raw_keys_:
                    refuse(c, 'no raw keys recorded at fit')
                outs.append(DeviceOutput(name, c, 'lookup', miss=len(mle.maps_[name])))
            elif name == c and dtype.kind in 'biu':
                outs.append(DeviceOutput(name, c, 'copy'))
            else:
                refuse(c, 'a categorical column that is not label-encoded and not an integer')
                outs.append(DeviceOutput(name, c, 'copy'))
        plan.cat = outs if names else None
        if mle is None and names:
            # TableBatches takes the id block through `X[names].values`: one common dtype, which must hold every column exactly
            kinds = [np.dtype('int64') if (n in discrete or not served_dtype(self.fit_dtypes_.get(sources.get(n, n))))
                     else self.fit_dtypes_[sources.get(n, n)] for n in names]
            if any(not served_dtype(self.fit_dtypes_.get(sources.get(n, n))) for n in names) or \
                    np.result_type(*kinds).kind not in 'biu':
                plan.whole = 'auto_encode_label is off and the categorical columns have no common integer dtype'
        for cc in self.continuous_columns or []:
            if leaf_names and set(cc.column_names) <= leaf_names:
                continue
            blk = []
            for c in cc.column_names:
                if not served_dtype(self.fit_dtypes_.get(c)):
                    refuse(c, f'dtype {self.fit_dtypes_.get(c)} at fit')
                    blk.append(DeviceOutput(c, c, 'cont'))
                else:
                    blk.append(DeviceOutput(c, c, 'cont', **cont_constants(c)))
            plan.conts.append(blk)
        seen = []
        for o in plan.outputs():
            if o.source not in seen:
                seen.append(o.source)
        plan.sources = [c for c in self.raw_columns_.values() if c in seen or c in plan.var]
        # LOOKUP tables: the fitted HOST steps on a one-column frame of the raw keys (and one NaN): key -> id is the host's answer
        for o in plan.cat or []:
            if o.op != 'lookup' or o.source in plan.refused:
                continue
            keys = self.raw_keys_[o.source]
            if keys.dtype != self.fit_dtypes_[o.source]:
                refuse(o.source, 'raw keys of another dtype than the column')
                continue
            if keys.dtype.kind == 'f' and not np.isnan(keys).any():
                keys = np.concatenate([keys, np.array([np.nan], dtype=keys.dtype)])
            probe = self._replay_host(pd.DataFrame({o.source: keys}), [o.source])
            from .. import ops
            k64 = ops.prep_keys(keys)
            order = np.argsort(k64, kind='stable')
            o.keys = np.ascontiguousarray(k64[order])
            o.ids = np.ascontiguousarray(probe[o.name].values.astype(np.int64)[order].astype(np.int32))
            if len(o.keys) > 1 and (o.keys[1:] == o.keys[:-1]).any():
                refuse(o.source, 'raw keys that are not distinct')
        plan.host_columns = [c for c in plan.sources if c in plan.refused]
        plan.device_columns = [c for c in plan.sources if c not in plan.refused]
        self._device_plan = plan
        return plan

    GBM_HOST_FITTED = 'a gbm_features step'

    def feed_refusal(self, device, cat_dtype=None, n_rows=None, y_words=0, max_resident_bytes=32 << 30, extra_bytes=0):
        """None when `transform_feed` can take the device path for this call, else the failing condition in words.
        extra_bytes: per-call device bytes besides the feed (fit_feed: the GBM fit's profile); a feed-fitted gbm_features step
        adds its bin matrices and the widened block itself"""
        import torch
        if torch.device(device).type != 'cuda':
            return f'the target device is {torch.device(device)}, not a GPU'
        if getattr(self, 'raw_columns_', None) is None:
            return 'the preprocessor is not fitted'
        if getattr(self, 'fit_dtypes_', None) is None or getattr(self, 'raw_keys_', None) is None:
            return 'the preprocessor was fitted before it recorded fit_dtypes_ and raw_keys_'
        st = self.config.distribute_strategy
        if st is not None and getattr(st, 'world_size', 1) > 1:
            return 'a multi-rank distribute_strategy is active'
        gbm = self.X_transformers.get('gbm_features')
        if gbm is not None and not getattr(gbm, 'feed_fitted_', False):
            return self.GBM_HOST_FITTED                 # (transform_feed spells out that it is the host-fitted kind)
        if cat_dtype is not None and cat_dtype != torch.int32:
            return f'cat_dtype is {cat_dtype}, the kernel writes int32 ids'
        plan = self.device_plan()
        if plan.whole is not None:
            return plan.whole
        if n_rows is not None:
            words = len(plan.cat or []) + sum(len(b) for b in plan.conts) + \
                sum(int(c.max_elements_length) for c in self.var_len_categorical_columns or []) + int(y_words)
            nbytes = 4 * words * int(n_rows) + int(extra_bytes)
            if gbm is not None:
                nbytes += gbm.feed_bytes(n_rows, self.config.gbm_feature_type)[0]
            if nbytes > max_resident_bytes:
                return f'the feed ({nbytes} bytes) would exceed max_resident_bytes={max_resident_bytes}'
        return None

    def feed_blocks(self, X, device, sources=None):
        """The blocks of a feed for the prepared frame X on `device`, by the plan: one upload per raw column, one
        `ops.prep_transform` per id / continuous block; host-served columns go through `_replay_host` and enter as plain
        copies.  A CPU `device` runs the same plan through the numpy branch of ops.prep_transform.
        sources: {raw column: its bytes already on `device`} (fit_feed uploaded them for the profile) are not uploaded again.
        -> (blocks, kinds, host-served raw columns)"""
        import torch
        from .. import ops
        plan = self.device_plan()
        dev_cols, host_cols = plan.partition(X)
        N = len(X)
        with _Phase('upload', device):
            src = {c: sources[c] if sources and c in sources else ops.prep_source(X[c].values, device) for c in dev_cols}
            tabs = plan.resident(device)
        blocks, kinds, var_blocks, host_src = [], [], [], {}
        with _Phase('host_columns', device):
            Xh = self._replay_host(X[host_cols].copy(), host_cols) if host_cols else None
            for o in plan.outputs():            # the host's int64 ids and float64 values, woven in as they are
                if o.source not in src:
                    host_src[o.name] = ops.prep_source(Xh[o.name].values.astype(np.float64 if o.op == 'cont' else np.int64), device)
            for c in self.var_len_categorical_columns or []:            # padded id lists, as training.TableBatches forms them
                arr = np.array(Xh[c.name].tolist())
                var_blocks.append(torch.as_tensor(np.ascontiguousarray(arr).astype(np.int64)).to(torch.int32).to(device))

        def column(o):
            if o.source not in src:
                return ops.PrepColumn(host_src[o.name], 'float64', ops.PREP_CONT) if o.op == 'cont' else \
                    ops.PrepColumn(host_src[o.name], 'int64', ops.PREP_COPY)
            dtype = plan.fit_dtypes[o.source].name
            if o.op == 'lookup':
                return ops.PrepColumn(src[o.source], dtype, ops.PREP_LOOKUP, keys=tabs[o.name, 'keys'], ids=tabs[o.name, 'ids'],
                                      miss=o.miss)
            if o.op == 'bin':
                return ops.PrepColumn(src[o.source], dtype, ops.PREP_BIN, edges=tabs[o.name, 'edges'], fill=o.fill, min=o.min,
                                      range=o.range, flags=o.flags)
            if o.op == 'cont':
                return ops.PrepColumn(src[o.source], dtype, ops.PREP_CONT, fill=o.fill, min=o.min, range=o.range, flags=o.flags)
            return ops.PrepColumn(src[o.source], dtype, ops.PREP_COPY)

        with _Phase('kernel', device):
            if plan.cat is not None:
                blocks.append(ops.prep_transform(N, [column(o) for o in plan.cat], 'cat'))
                kinds.append('cat')
            blocks += var_blocks
            kinds += ['var'] * len(var_blocks)
            for blk in plan.conts:
                blocks.append(ops.prep_transform(N, [column(o) for o in blk], 'cont'))
                kinds.append('cont')
        return blocks, kinds, host_cols

    def transform_feed(self, X, y=None, *, device, task=None, num_classes=None, sample_weight=None, cat_dtype=None, mode='auto',
                       max_resident_bytes=32 << 30, y_encoded=False):
        """A raw frame (and raw y) -> a `training.TableBatches` on `device`, bit for bit
        `TableBatches(self.transform_X(X), self.transform_y(y), ...)`.  On a GPU the numeric columns are uploaded as they are
        and one kernel launch per block writes the resident feed (`feed.transform_path == 'device'`); columns the kernel cannot
        serve — strings, categories, var-len columns, a dtype other than at fit — go through the fitted host steps alone
        (`feed.host_columns`).  mode: 'auto' takes the host construction when the device path refuses the call, True raises
        ValueError naming the condition, False (or DT_AMD_DEVICE_TRANSFORM=0) is the host construction.  y_encoded: y has been
        through `transform_y` already."""
        import torch
        from .. import training
        if mode not in (True, False, 'auto'):
            raise ValueError(f"transform_feed: mode must be True, False or 'auto', got {mode!r}")
        cat_dtype = torch.int32 if cat_dtype is None else cat_dtype
        task = self.task_ if task is None else task
        if num_classes is None:
            num_classes = len(self.labels_) if self.labels_ is not None and len(self.labels_) else 1
        if y is not None and not y_encoded:
            y = self.transform_y(y)
        y_host, y_ndim = training.host_targets(y, task, num_classes, sample_weight)
        if mode is False:
            why = 'mode=False'
        elif os.environ.get('DT_AMD_DEVICE_TRANSFORM', '1') == '0':
            why = 'DT_AMD_DEVICE_TRANSFORM=0'
        else:
            n_rows = X.shape[0] if hasattr(X, 'shape') else len(X)
            y_words = 0 if y_host is None else y_host.numel() // max(1, y_host.shape[0])
            why = self.feed_refusal(device, cat_dtype, n_rows, y_words, max_resident_bytes)
        if why is not None:
            if mode is True:
                if why == self.GBM_HOST_FITTED:
                    why += ' fitted on the host frame (fit_transform); only fit_feed fits the trees on the blocks of a feed'
                raise ValueError(f'transform_feed(mode=True): {why}')
            feed = training.TableBatches(self.transform_X(X), y, self.categorical_columns, self.continuous_columns, device, task,
                                         num_classes, cat_dtype=cat_dtype,
                                         var_len_categorical_columns=self.var_len_categorical_columns,
                                         max_resident_bytes=max_resident_bytes, sample_weight=sample_weight)
            feed.transform_path, feed.host_columns, feed.transform_refusal = 'host', list(self.raw_columns_.values()), why
            return feed
        X = X.copy(deep=False) if isinstance(X, pd.DataFrame) else X
        X = self._prepare_X(X)
        blocks, kinds, host_cols = self.feed_blocks(X, torch.device(device))
        if 'gbm_features' in self.X_transformers:
            with _Phase('gbm', device):
                blocks, kinds = self.X_transformers['gbm_features'].transform_feed(blocks, kinds, self.config.gbm_feature_type)
        feed = training.TableBatches.from_device(blocks, kinds, y=None if y_host is None else y_host.to(device), y_ndim=y_ndim,
                                                 weighted=sample_weight is not None)
        feed.transform_path, feed.host_columns, feed.transform_refusal = 'device', list(host_cols), None
        return feed

    # -- the device path of fit: column profiles (ops.column_profile, csrc/prep_fit.hip), then transform_feed ---------------------
    def device_fit_refusal(self, device):
        """None when `fit_feed` can fit on the device, else the failing condition in words"""
        import torch
        if torch.device(device).type != 'cuda':
            return f'the target device is {torch.device(device)}, not a GPU'
        st = self.config.distribute_strategy
        if st is not None and getattr(st, 'world_size', 1) > 1:
            return 'a multi-rank distribute_strategy is active'
        return None

    def fit_feed(self, X, y, *, device, mode='auto', sample_weight=None, cat_dtype=None, max_resident_bytes=32 << 30):
        """`fit_transform` with the numeric columns' statistics taken on the device, and the training rows turned into a
        resident `training.TableBatches` by `transform_feed` — no transformed pandas frame is made.  Every numeric column
        (`served_dtype`) is uploaded as it is and profiled by `ops.column_profile`: nunique, the distinct values of the columns a
        label encoder sees, min, max, the fixed-order float64 sum behind the mean, and the few order statistics np.quantile's
        formula reads.  Other columns (strings, categories, var-len) are fitted by the host steps on a sub-frame of themselves.
        The fitted state is `fit_transform`'s, attribute for attribute; `means_` is sum / count of the exact-order device sum
        (pandas' own summation order differs by rounding on general data).  mode as `transform_feed`; False, DT_AMD_DEVICE_FIT=0
        or a refusal (`feed.fit_refusal`) take `fit_transform` + `transform_feed`.  -> the feed; `feed.fit_path` says which.
        sample_weight: per-row weights, or a function of the encoded y returning them (class weights need the fitted label
        encoder).  The raw columns are uploaded once and serve the profile and the transform.  max_resident_bytes bounds the
        profile's workspace (16 bytes per numeric element, checked before anything is fitted) and the feed; the feed's size is
        known only after typing, so a feed beyond the bound is refused AFTER the device fit: 'auto' then fits again on the
        host, mode=True raises and leaves the object device-fitted.  `apply_gbm_features`: the trees are fitted on the blocks of
        the feed (`GbmLeavesEncoder.fit_feed`: the id block and the float32 continuous blocks are exactly the columns the host
        fit sees, the continuous ones rounded to float32) and the leaf columns are written into the widened blocks; the bound
        also covers the two bin matrices, the widened block and the profile of the blocks' columns.  A column holding an
        infinite value is a refusal that names it."""
        import torch
        from .. import training
        if mode not in (True, False, 'auto'):
            raise ValueError(f"fit_feed: mode must be True, False or 'auto', got {mode!r}")
        kw = dict(device=device, cat_dtype=cat_dtype, max_resident_bytes=max_resident_bytes)
        if mode is False:
            why = 'mode=False'
        elif os.environ.get('DT_AMD_DEVICE_FIT', '1') == '0':
            why = 'DT_AMD_DEVICE_FIT=0'
        else:
            why = self.device_fit_refusal(device)
        if why is None:
            self._validate_fit_transform(X, y)
            frame = X if isinstance(X, pd.DataFrame) else pd.DataFrame(X)
            numeric = sum(served_dtype(frame[c].dtype) for c in frame.columns)
            if 16 * numeric * len(frame) > max_resident_bytes:          # the sort's two key buffers: 2 x 8 bytes per element
                why = f'the profile workspace ({16 * numeric * len(frame)} bytes) would exceed max_resident_bytes={max_resident_bytes}'
        if why is None:
            y_enc, sources = self._fit_on_device(X, copy.deepcopy(y), device)
            weights = sample_weight(y_enc) if callable(sample_weight) else sample_weight
            num_classes = len(self.labels_) if self.labels_ is not None and len(self.labels_) else 1
            y_host, y_ndim = training.host_targets(y_enc, self.task_, num_classes, weights)
            enc = self._gbm_encoder() if self.config.apply_gbm_features else None
            gbm_bytes = sum(enc.feed_bytes(len(frame), self.config.gbm_feature_type)) if enc is not None else 0
            why = self.feed_refusal(device, cat_dtype, len(frame), y_host.numel() // max(1, y_host.shape[0]), max_resident_bytes,
                                    extra_bytes=gbm_bytes)
            if why is None:
                Xp = self._prepare_X(frame.copy(deep=False))
                blocks, kinds, host_cols = self.feed_blocks(Xp, torch.device(device), sources)
                if enc is not None:
                    try:
                        with _Phase('fit_gbm', device):
                            blocks, kinds = self._apply_gbm_features_feed(enc, blocks, kinds, y_enc)
                    except FeedRefusal as e:            # (a column the in-feed fit does not take: 'auto' fits on the host)
                        why = str(e)
            if why is None:
                feed = training.TableBatches.from_device(blocks, kinds, y=y_host.to(device), y_ndim=y_ndim,
                                                         weighted=weights is not None)
                feed.transform_path, feed.host_columns, feed.transform_refusal = 'device', list(host_cols), None
                feed.fit_path, feed.fit_refusal = 'device', None
                return feed
        if mode is True:
            raise ValueError(f'fit_feed(mode=True): {why}')
        _Xt, y_enc = self.fit_transform(X, y)
        weights = sample_weight(y_enc) if callable(sample_weight) else sample_weight
        feed = self.transform_feed(X, y_enc, y_encoded=True, mode='auto', sample_weight=weights, **kw)
        feed.fit_path, feed.fit_refusal = 'host', why
        return feed

    def _fit_on_device(self, X, y, device):
        """the steps of `fit_transform` in its order; -> (the encoded y, {numeric column: its bytes on `device`})"""
        from .. import ops
        self.reset()
        y = self.fit_transform_y(y)
        X = X.copy(deep=False) if isinstance(X, pd.DataFrame) else pd.DataFrame(X)
        raw = list(X.columns)
        X = self._prepare_X(X)
        self.raw_columns_ = dict(zip(raw, X.columns))
        self.fit_dtypes_ = {c: X[c].dtype for c in X.columns}
        conf, N = self.config, len(X)
        var_names = [v[0] for v in (conf.var_len_categorical_columns or [])]
        dev_cols = [c for c in X.columns if served_dtype(X[c].dtype) and c not in var_names]
        Xh = X[[c for c in X.columns if c not in dev_cols]].copy()            # the host sub-frame, transformed step by step
        prof, at = None, {}
        if dev_cols and N > 0:
            with _Phase('fit_upload', device):
                srcs = [ops.prep_source(X[c].values, device) for c in dev_cols]
            names = [X[c].dtype.name for c in dev_cols]
            cap = max(round(N ** conf.cat_exponent), MultiKBinsDiscretizer([]).max_bins + 1) if conf.cat_exponent < 1 else 0
            with _Phase('fit_kernel', device):
                prof = ops.column_profile(srcs, names, cap=cap)
                prof.host()
            at = {c: j for j, c in enumerate(dev_cols)}
            self.last_profile_passes = list(prof.passes)        # digit passes the sort ran per column (tools/prep_fit_bench.py)
        nuniques = {c: (prof.nunique[at[c]] if c in at else X[c].nunique()) for c in X.columns}
        self._prepare_features(X, nuniques)
        ce = self.X_transformers.get('categorize')
        if ce is not None:
            host_ce = copy.copy(ce)
            host_ce.columns = [c for c in ce.columns if c not in at]
            Xh = host_ce.transform(Xh)
        # the distinct values of the columns a label encoder sees; explicit categoricals above the cap get a second, wider profile
        wanted = [c for c in dev_cols if conf.auto_encode_label and
                  (c in self.get_categorical_columns() or (ce is not None and c in ce.columns))]
        distinct = {c: prof.distinct(at[c]) for c in wanted}
        wide = [c for c in wanted if distinct[c] is None]
        if wide:
            with _Phase('fit_kernel', device):
                p2 = ops.column_profile([srcs[at[c]] for c in wide], [names[at[c]] for c in wide],
                                        cap=int(max(prof.n_distinct[at[c]] for c in wide)))
            distinct.update({c: p2.distinct(j) for j, c in enumerate(wide)})
        self.raw_keys_ = {}
        for c in wanted:
            values = distinct[c][0]
            if prof.nan_count[at[c]]:
                values = np.concatenate([values, np.array([np.nan], dtype=values.dtype)])
            self.raw_keys_[c] = distinct_raw_values(values)
        conts = self.get_continuous_columns()
        dev_conts = [c for c in conts if c in at]
        fill = {}                                       # what a NaN of the column becomes; no entry: it stays
        if conf.auto_imputation:
            cats = self.get_categorical_columns() + self.get_var_len_categorical_columns()
            targets = set() if ce is None else {c + '_cat' if ce.remain_numeric else c for c in ce.columns}
            is_obj = {c: c in targets or str(X[c].dtype).startswith(('obj', 'str')) or str(X[c].dtype) == 'category' for c in cats}
            imp = ColumnImputer(conts, [c for c in cats if is_obj[c]], [c for c in cats if not is_obj[c]])
            for c in dev_conts:
                j = at[c]
                count = N - int(prof.nan_count[j])
                mean = float(prof.sums[j]) / count if count else 0.0
                imp.means_[c] = float(np.float32(mean)) if names[j] == 'float32' else mean
                fill[c] = imp.means_[c]
            Xh = self._fit_host_part(imp, Xh)
            self.X_transformers['imputation'] = imp
        lo_hi = {}
        for c in dev_conts:
            j = at[c]
            lo, hi = prof.minimum(j), prof.maximum(j)
            lo, hi = (float('nan'), float('nan')) if lo is None else (float(lo), float(hi))
            if c in fill and prof.nan_count[j]:
                lo, hi = (fill[c], fill[c]) if lo != lo else (min(lo, fill[c]), max(hi, fill[c]))
            lo_hi[c] = lo, hi
        scale = {}
        if conf.auto_scale:
            ss = MinMaxScalerTransformer(conts)
            for c in dev_conts:
                lo, hi = lo_hi[c]
                ss.min_[c], ss.range_[c] = lo, (hi - lo) if hi > lo else 1.0
                scale[c] = ss.min_[c], ss.range_[c]
            Xh = self._fit_host_part(ss, Xh)
            self.X_transformers['standard_scale'] = ss

        def final(c, values):
            """float64 raw values of continuous column c after imputation and scaling, as the host steps compute them"""
            v = np.asarray(values, dtype=np.float64)
            if c in fill:
                v = np.where(np.isnan(v), fill[c], v)
            return (v - scale[c][0]) / scale[c][1] if c in scale else v

        if conf.auto_encode_label:
            mle = MultiLabelEncoder(self.get_categorical_columns())
            sources = self._output_sources()
            for name in mle.columns:
                c = sources.get(name, name)
                if c in at:                             # the fitted host steps on the one-column frame of distinct raw values
                    probe = self._replay_host(pd.DataFrame({c: self.raw_keys_[c]}), [c])
                    mle.maps_[name] = MultiLabelEncoder([name]).fit(probe).maps_[name]
            Xh = self._fit_host_part(mle, Xh)
            self.X_transformers['label_encoder'] = mle
        if conf.auto_discrete:
            mkbd = MultiKBinsDiscretizer(conts)
            with _Phase('fit_kernel', device):
                stats = self._quantile_edges(prof, at, dev_conts, fill, final, mkbd.max_bins, N) if dev_conts else {}
            host_part = copy.copy(mkbd)
            host_part.columns = [c for c in conts if c not in at]
            host_part.fit(Xh)
            Xh = host_part.transform(Xh)
            host_new = {t[0]: t for t in host_part.new_columns}
            mkbd.new_columns = []
            for c in conts:
                if c in at:
                    mkbd.edges_[c], new = stats[c]
                    mkbd.new_columns.append(new)
                else:
                    mkbd.new_columns.append(host_new[c])
            self._append_categorical_cols([(new_name, bins + 1) for name, new_name, bins in mkbd.new_columns])
            self.X_transformers['discreter'] = mkbd
        var_len = conf.var_len_categorical_columns
        if var_len is not None and len(var_len) > 0:
            self._var_len_encoder(Xh, var_len)
        self.X_transformers['last'] = PassThroughEstimator()
        return y, ({c: srcs[at[c]] for c in dev_cols} if prof is not None else {})

    @staticmethod
    def _fit_host_part(step, Xh):
        """fit `step` (an imputer, scaler or label encoder holding ALL its columns) on those of its columns the host sub-frame
        Xh holds — the fitted dicts are shared with `step` — and transform Xh by it"""
        part = copy.copy(step)
        for attr in ('columns', 'continuous', 'obj_cats', 'num_cats'):
            if hasattr(step, attr):
                setattr(part, attr, [c for c in getattr(step, attr) if c in Xh.columns])
        return part.fit_transform(Xh)

    @staticmethod
    def _quantile_edges(prof, at, columns, fill, final, max_bins, N):
        """{c: (edges_[c], new_columns entry)} of MultiKBinsDiscretizer.fit for profiled columns: np.quantile's 'linear' rule
        (virtual index (n - 1) q, its two neighbours, numpy's lerp) on order statistics read from the device.  The
        imputation and scale maps are monotone, so ranks are taken on raw values and the selected values are mapped here."""
        cols = list(columns)
        bins, ranks, gammas = {}, np.full((len(at), 2 * (max_bins + 1)), -1, dtype=np.int64), {}
        for c in cols:
            j = at[c]
            d = prof.distinct(j)
            if d is None:
                nunique = max_bins + 1                  # more distinct raw values than the cap >= max_bins + 1
            else:
                values = d[0].astype(np.float64)
                if prof.nan_count[j]:
                    values = np.concatenate([values, [np.nan]])
                nunique = pd.Series(final(c, values)).nunique()
            bins[c] = int(max(2, min(max_bins, nunique)))
            q = np.linspace(0, 1, bins[c] + 1)
            virtual = (N - 1) * q
            prev = np.floor(virtual)
            nxt = prev + 1
            above = virtual >= N - 1
            prev[above], nxt[above] = N - 1, N - 1
            gammas[c] = virtual - np.floor(virtual)
            ranks[j, :len(q)] = prev.astype(np.int64)
            ranks[j, len(q):2 * len(q)] = nxt.astype(np.int64)
        fills = np.array([fill.get(c, np.nan) for c in sorted(at, key=at.get)], dtype=np.float64)
        got = prof.order_stats(ranks, fills)
        out = {}
        for c in cols:
            j, n = at[c], bins[c] + 1
            unfilled = c not in fill and prof.nan_count[j] > 0      # np.quantile of a column holding NaN: NaN
            a, b, t = final(c, got[j, :n]), final(c, got[j, n:2 * n]), gammas[c]
            with np.errstate(all='ignore'):
                diff = b - a
                quant = a + diff * t
                quant = np.where(t >= 0.5, b - diff * (1 - t), quant)
            if unfilled:
                quant = np.full(n, np.nan)
            edges = np.unique(quant)
            out[c] = edges[1:-1], (c, c + '_discrete', len(edges) - 1 if len(edges) > 1 else 1)
        return out

    def source_columns(self):
        """{raw column label as given to fit: [the transformed columns computed from it]} — which model inputs change when
        that raw column alone changes (utils/feature_importance.py permutes those instead of transforming again).  Declared
        from the fitted pipeline, not probed: the column itself where the metadata lists it (categorical, var-len or
        continuous), `<c>_cat` of CategorizeEncoder with cat_remain_numeric, `<c>_discrete` of MultiKBinsDiscretizer.  Excluded
        and single-valued columns feed nothing: []."""
        if getattr(self, 'raw_columns_', None) is None:
            raise ValueError('source_columns: the preprocessor is not fitted')
        listed = set(self.get_categorical_columns()) | set(self.get_var_len_categorical_columns()) | \
            set(self.get_continuous_columns())
        derived = {p: ([p] if p in listed else []) for p in self.raw_columns_.values()}
        ce = self.X_transformers.get('categorize')
        if ce is not None:
            for c, new in zip(ce.columns, ce.new_columns):              # (new_columns: only with remain_numeric)
                derived[c].append(new[0])
        mkbd = self.X_transformers.get('discreter')
        if mkbd is not None:
            for c, new, _bins in mkbd.new_columns:
                derived[c].append(new)
        return {raw: derived[p] for raw, p in self.raw_columns_.items()}

    def get_categorical_columns(self):
        return [c.name for c in self.categorical_columns]

    def get_var_len_categorical_columns(self):
        if self.var_len_categorical_columns is not None:
            return [c.name for c in self.var_len_categorical_columns]
        return []

    def get_continuous_columns(self):
        cont_vars = []
        for c in self.continuous_columns:
            cont_vars = cont_vars + c.column_names
        return cont_vars
