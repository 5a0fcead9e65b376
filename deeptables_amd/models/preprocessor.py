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
GBM leaf features (`apply_gbm_features`, needs lightgbm) and the fit cache are not provided.
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
        self.new_columns = []
        if self.remain_numeric:
            for c in self.columns:
                self.new_columns.append((c + '_cat', 'str', int(X[c].nunique())))
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
            raise NotImplementedError('apply_gbm_features needs lightgbm, which this environment does not have')
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
    def _prepare_features(self, X):
        """Column typing, preprocessor.py:267-336."""
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
            nunique = X[c].nunique()
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
            X = ce.fit_transform(X)
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

        names = self.get_categorical_columns()
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

    def feed_refusal(self, device, cat_dtype=None, n_rows=None, y_words=0, max_resident_bytes=32 << 30):
        """None when `transform_feed` can take the device path for this call, else the failing condition in words"""
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
        if cat_dtype is not None and cat_dtype != torch.int32:
            return f'cat_dtype is {cat_dtype}, the kernel writes int32 ids'
        plan = self.device_plan()
        if plan.whole is not None:
            return plan.whole
        if n_rows is not None:
            words = len(plan.cat or []) + sum(len(b) for b in plan.conts) + \
                sum(int(c.max_elements_length) for c in self.var_len_categorical_columns or []) + int(y_words)
            if 4 * words * int(n_rows) > max_resident_bytes:
                return f'the feed ({4 * words * int(n_rows)} bytes) would exceed max_resident_bytes={max_resident_bytes}'
        return None

    def feed_blocks(self, X, device):
        """The blocks of a feed for the prepared frame X on `device`, by the plan: one upload per raw column, one
        `ops.prep_transform` per id / continuous block; host-served columns go through `_replay_host` and enter as plain
        copies.  A CPU `device` runs the same plan through the numpy branch of ops.prep_transform.
        -> (blocks, kinds, host-served raw columns)"""
        import torch
        from .. import ops
        plan = self.device_plan()
        dev_cols, host_cols = plan.partition(X)
        N = len(X)
        with _Phase('upload', device):
            src = {c: ops.prep_source(X[c].values, device) for c in dev_cols}
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
        feed = training.TableBatches.from_device(blocks, kinds, y=None if y_host is None else y_host.to(device), y_ndim=y_ndim,
                                                 weighted=sample_weight is not None)
        feed.transform_path, feed.host_columns, feed.transform_refusal = 'device', list(host_cols), None
        return feed

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
