# -*- coding:utf-8 -*-
"""Drop-in for `deeptables.models.deeptable.DeepTable` (deeptables/models/deeptable.py:30-822):
`DeepTable(config).fit(X_df, y) -> (DeepModel, History)`, `fit_cross_validation`, the model set (`modelset`, `best_model`,
`leaderboard`, `get_model`), `predict` / `predict_proba` / `predict_proba_all` / `evaluate` / `apply` with a `model_selector`,
`save`/`load`.  Cross-validation and prediction over the set live in models/cross_validation.py; GBM features
and the hypernets toolbox are outside the accelerated hot path.  The default preprocessor is
`preprocessor.DefaultPreprocessor` (the TF/hypernets-free restatement of the reference's pipeline);
`SimplePreprocessor` below is a smaller impute + label-encode variant kept for callers that want ids with 0
reserved for unseen values."""
import os
import pickle

import numpy as np
import pandas as pd

from . import cross_validation, deepmodel
from .config import ModelConfig
from .modelset import ModelInfo, ModelSet
from .metainfo import CategoricalColumn, ContinuousColumn
from .preprocessor import DefaultPreprocessor
from ..utils import consts


class SimplePreprocessor:
    """impute -> label-encode categoricals -> pass numerics through (float32)."""

    def __init__(self, config):
        self.config = config
        self.categorical_columns = None
        self.continuous_columns = None
        self.labels_ = None
        self.task_ = None
        self._cat_maps = {}
        self._num_fill = {}
        self._num_scale = {}
        self.pos_label = config.pos_label

    # -- y ----------------------------------------------------------------------------------------
    def _infer_task(self, y):
        if self.config.task != consts.TASK_AUTO:
            task = self.config.task
            labels = sorted(pd.unique(pd.Series(y))) if task != consts.TASK_REGRESSION else []
            return task, list(labels)
        ys = pd.Series(y)
        if ys.dtype.kind == 'f' and ys.nunique() > 20:
            return consts.TASK_REGRESSION, []
        labels = sorted(ys.dropna().unique())
        if len(labels) == 2:
            return consts.TASK_BINARY, list(labels)
        if len(labels) > 2 and (ys.dtype.kind in 'OUSb' or len(labels) <= 100):
            return consts.TASK_MULTICLASS, list(labels)
        return consts.TASK_REGRESSION, []

    def transform_y(self, y):
        if self.task_ == consts.TASK_REGRESSION or not self.config.auto_encode_label:
            return np.asarray(y, dtype=np.float32)
        mapping = {v: i for i, v in enumerate(self.labels_)}
        return pd.Series(y).map(mapping).values.astype(np.float32)

    def inverse_transform_y(self, y_indicator):
        return np.asarray(self.labels_)[np.asarray(y_indicator).astype(np.int64)]

    # -- X ----------------------------------------------------------------------------------------
    def fit_transform(self, X, y):
        X = X.copy()
        X.columns = [str(c) for c in X.columns]
        drop = [c for c in (self.config.exclude_columns or []) if c in X.columns]
        X = X.drop(columns=drop)
        self.task_, self.labels_ = self._infer_task(y)
        if self.pos_label is not None and self.task_ == consts.TASK_BINARY and self.pos_label in self.labels_:
            self.labels_ = [l for l in self.labels_ if l != self.pos_label] + [self.pos_label]
        cc = self.config.categorical_columns
        cat_names = []
        for c in X.columns:
            kind = X[c].dtype.kind
            if (isinstance(cc, (list, tuple)) and c in cc) or kind in 'OUSb' or str(X[c].dtype) == 'category':
                cat_names.append(c)
            elif cc == 'auto' and self.config.auto_categorize and kind in 'iu' and \
                    X[c].nunique() < len(X) ** self.config.cat_exponent:
                cat_names.append(c)
        num_names = [c for c in X.columns if c not in cat_names]
        self.cat_names_, self.num_names_ = cat_names, num_names
        for c in cat_names:
            values = pd.unique(X[c].dropna())
            self._cat_maps[c] = {v: i + 1 for i, v in enumerate(sorted(values, key=lambda t: str(t)))}
        for c in num_names:
            col = pd.to_numeric(X[c], errors='coerce')
            self._num_fill[c] = float(col.mean()) if col.notna().any() else 0.0
            if self.config.auto_scale:
                sd = float(col.std()) or 1.0
                self._num_scale[c] = (float(col.mean()), sd if sd > 0 else 1.0)
        dim = self.config.embeddings_output_dim if self.config.fixed_embedding_dim else 0
        self.categorical_columns = [CategoricalColumn(c, len(self._cat_maps[c]) + 2, dim if dim > 0 else 0)
                                    for c in cat_names]
        self.continuous_columns = [ContinuousColumn(consts.INPUT_PREFIX_NUM + 'all', num_names)] if num_names else []
        return self.transform_X(X, _prepared=True), self.transform_y(y)

    def transform_X(self, X, _prepared=False):
        if not _prepared:
            X = X.copy()
            X.columns = [str(c) for c in X.columns]
        out = pd.DataFrame(index=X.index)
        for c in self.cat_names_:
            out[c] = X[c].map(self._cat_maps[c]).fillna(0).astype(np.int64)     # unseen / NaN -> 0
        for c in self.num_names_:
            col = pd.to_numeric(X[c], errors='coerce').fillna(self._num_fill[c]).astype(np.float32)
            if c in self._num_scale:
                mu, sd = self._num_scale[c]
                col = (col - mu) / sd
            out[c] = col
        return out

    def get_categorical_columns(self):
        return [c.name for c in self.categorical_columns]

    def get_continuous_columns(self):
        return list(self.num_names_)

    def source_columns(self):
        """{column (its label as a string): [the transformed columns computed from it]}: every kept column is its own only
        source (DefaultPreprocessor.source_columns); excluded columns are absent."""
        return {c: [c] for c in list(self.cat_names_) + list(self.num_names_)}


class DeepTable:
    """`DeepTable(config=ModelConfig(nets=deepnets.DeepFM)).fit(df, y)` — deeptable.py:30."""

    def __init__(self, config=None, preprocessor=None):
        self.config = config if config is not None else ModelConfig()
        self.nets = self.config.nets
        self.preprocessor = preprocessor if preprocessor is not None else DefaultPreprocessor(self.config)
        self.model = None               # the current model
        self._models = {}
        metrics = self.config.metrics
        self._modelset = ModelSet(metric=self.config.first_metric_name if metrics else 'loss',
                                  best_mode=consts.MODEL_SELECT_MODE_AUTO)
        self._current_model = None      # its name in the set (None: `model` was set by hand)
        self.last_cv_path = None        # 'device' | 'host' after fit_cross_validation

    @property
    def task(self):
        return self.preprocessor.task_

    @property
    def num_classes(self):
        return len(self.preprocessor.labels_)

    @property
    def classes_(self):
        return self.preprocessor.labels_

    # -- the model set (deeptable.py:281-300, :626-649, :695-712) ------------------------------------------------------
    @property
    def modelset(self):
        return self._modelset

    @property
    def best_model(self):
        return self.get_model(consts.MODEL_SELECTOR_BEST)

    @property
    def leaderboard(self):
        return self._modelset.leaderboard()

    def _push_model(self, type, name, model, history):
        """a fitted model enters the set under `name` and becomes the current one"""
        self._modelset.push(ModelInfo(type, name, model, {}, history=history))
        self._current_model = name
        self.model = model

    def _load_deepmodel(self, filepath):
        pp = self.preprocessor
        return deepmodel.DeepModel(self.task, self.num_classes, self.config, pp.categorical_columns, pp.continuous_columns,
                                   model_file=filepath,
                                   var_categorical_len_columns=getattr(pp, 'var_len_categorical_columns', None))

    def _resolve(self, mi):
        """a ModelInfo's model; a path (a set restored by `load`) is read the first time it is needed"""
        if isinstance(mi.model, str):
            mi.model = self._load_deepmodel(mi.model)
        return mi.model

    def get_model(self, model_selector=consts.MODEL_SELECTOR_CURRENT):
        """'current': the model of the last fit (or fold); 'best': the head of the leaderboard; 'all': every model of the set,
        in the order they were fitted; anything else: the model of that name (ValueError when there is none)"""
        if model_selector == consts.MODEL_SELECTOR_CURRENT:
            self._require_model()
            return self.model
        if model_selector == consts.MODEL_SELECTOR_ALL:
            return [self._resolve(mi) for mi in self._modelset.get_modelinfos()]
        if model_selector == consts.MODEL_SELECTOR_BEST:
            mi = self._modelset.best_model()
        else:
            mi = self._modelset.get_modelinfo(model_selector)
        if mi is None:
            raise ValueError(f'{model_selector} does not exist.')
        return self._resolve(mi)

    def _one_model(self, model_selector):
        model = self.get_model(model_selector)
        if not isinstance(model, deepmodel.DeepModel):
            raise ValueError(f'Wrong model_selector:{model_selector}')
        return model

    # -- fit ------------------------------------------------------------------------------------------------------------
    def fit(self, X=None, y=None, batch_size=128, epochs=1, verbose=1, callbacks=None, validation_split=0.2,
            validation_data=None, shuffle=True, class_weight=None, sample_weight=None, initial_epoch=0,
            steps_per_epoch=None, validation_steps=None, validation_freq=1, max_queue_size=10, workers=1,
            use_multiprocessing=False):
        if X is None or len(X) == 0:
            raise ValueError('X can not be empty.')
        X_t, y_t = self.preprocessor.fit_transform(X, y)
        if validation_data is not None:
            validation_data = (self.preprocessor.transform_X(validation_data[0]),
                               self.preprocessor.transform_y(validation_data[1]))
        if len(self.preprocessor.categorical_columns) == 0 and len(self.preprocessor.continuous_columns) == 0:
            raise ValueError('No valid input columns.')
        model = deepmodel.DeepModel(self.task, self.num_classes, self.config,
                                    self.preprocessor.categorical_columns, self.preprocessor.continuous_columns,
                                    var_categorical_len_columns=getattr(self.preprocessor,
                                                                        'var_len_categorical_columns', None))
        if class_weight is None and self.config.apply_class_weight and self.task != consts.TASK_REGRESSION:
            class_weight = self.get_class_weight(y_t)               # reference deeptable.py:354-355
        history = model.fit(X_t, y_t, batch_size=batch_size, epochs=epochs, verbose=verbose, callbacks=callbacks,
                            validation_split=validation_split, validation_data=validation_data, shuffle=shuffle,
                            class_weight=class_weight, sample_weight=sample_weight,
                            initial_epoch=initial_epoch, steps_per_epoch=steps_per_epoch,
                            validation_steps=validation_steps, validation_freq=validation_freq)
        self._modelset.clear()                                      # reference deeptable.py:369-370, :695-697
        self._push_model('val', '+'.join(self.nets), model, history.history)
        self._models['dt-1'] = model
        return model, history

    def fit_cross_validation(self, X, y, X_eval=None, X_test=None, num_folds=5, stratified=False, iterators=None,
                             batch_size=None, epochs=1, verbose=1, callbacks=None, n_jobs=1, random_state=9527,
                             shuffle=True, class_weight=None, sample_weight=None, initial_epoch=0, steps_per_epoch=None,
                             validation_steps=None, validation_freq=1, max_queue_size=10, workers=1,
                             use_multiprocessing=False, oof_metrics=None, device='auto'):
        """deeptable.py:373-517 -> (oof_proba, eval_proba_mean, test_proba_mean[, oof_scores]).  Every fold's model enters the
        set as '<nets>-kfold-<i>'; the last one is current.  device: 'auto' cuts the folds out of one device-resident feed
        when the model's device, the preprocessor and the feed allow it, True raises and names the condition that fails, False
        is the host loop; `last_cv_path` says which ran (models/cross_validation.py)."""
        return cross_validation.fit_cross_validation(
            self, X, y, X_eval=X_eval, X_test=X_test, num_folds=num_folds, stratified=stratified, iterators=iterators,
            batch_size=batch_size, epochs=epochs, verbose=verbose, callbacks=callbacks, n_jobs=n_jobs,
            random_state=random_state, shuffle=shuffle, class_weight=class_weight, sample_weight=sample_weight,
            initial_epoch=initial_epoch, steps_per_epoch=steps_per_epoch, validation_steps=validation_steps,
            validation_freq=validation_freq, max_queue_size=max_queue_size, workers=workers,
            use_multiprocessing=use_multiprocessing, oof_metrics=oof_metrics, device=device)

    def get_class_weight(self, y):
        """'balanced' class weights n / (classes * count) over the encoded labels (reference deeptable.py:651-668:
        sklearn compute_class_weight('balanced'))."""
        yl = np.asarray(y)
        yl = yl.argmax(-1) if yl.ndim > 1 and yl.shape[-1] > 1 else yl.reshape(-1).astype(np.int64)
        n_cls = len(self.classes_) if self.classes_ is not None else int(yl.max()) + 1
        counts = np.bincount(yl, minlength=n_cls).astype(np.float64)
        return {k: float(len(yl) / (n_cls * c)) if c > 0 else 0.0 for k, c in enumerate(counts)}

    def _require_model(self):
        if self.model is None:
            raise ValueError('DeepTable is not fitted yet.')

    # -- predict (deeptable.py:538-610) ----------------------------------------------------------------------------------
    def predict_proba(self, X, batch_size=128, verbose=0, model_selector=consts.MODEL_SELECTOR_CURRENT,
                      auto_transform_data=True, **kwargs):
        if model_selector == consts.MODEL_SELECTOR_ALL:
            models = self.get_model(model_selector)
            if not models:
                raise ValueError('Model set is empty.')
            return cross_validation.predict_proba_mean(self, X, models, batch_size, auto_transform_data)
        model = self.get_model(model_selector)
        proba = model.predict(self._feed_of(model, X) if auto_transform_data else X, batch_size=batch_size)
        return cross_validation.fix_binary(self, proba)             # fix_binary_predict_proba_result

    def _feed_of(self, model, X, y=None, device=None):
        """The raw frame (and raw y) as the model's input feed: `preprocessor.transform_feed` — on a GPU the numeric columns are
        transformed by one kernel launch per block, on the host otherwise — or, for a preprocessor without it, the frame
        `transform_X` makes (and the encoded y), which `DeepModel` turns into a feed itself"""
        pp = self.preprocessor
        if not callable(getattr(pp, 'transform_feed', None)):
            return pp.transform_X(X) if y is None else (pp.transform_X(X), pp.transform_y(y))
        return pp.transform_feed(X, y, device=model.device if device is None else device, task=model.task,
                                 num_classes=model.num_classes)

    def make_feed(self, X, y=None, device='auto'):
        """A raw frame (and raw y) as a device-resident `training.TableBatches` of the current model's inputs: what `predict`,
        `evaluate` and `DeepModel.fit` / `predict` / `evaluate` take in place of a frame.  device 'auto': the model's.
        `feed.transform_path` says whether the kernel ('device') or pandas ('host') made it."""
        self._require_model()
        model = self._one_model(consts.MODEL_SELECTOR_CURRENT)
        pp = self.preprocessor
        if not callable(getattr(pp, 'transform_feed', None)):
            raise ValueError(f'make_feed: {type(pp).__name__} has no transform_feed')
        return self._feed_of(model, X, y, None if device == 'auto' else device)

    def predict_proba_all(self, X, batch_size=128, verbose=0, auto_transform_data=True):
        """{name: proba} of every model of the set"""
        infos = self._modelset.get_modelinfos()
        if not infos:
            raise ValueError('Model set is empty.')
        return cross_validation.predict_proba_each(self, X, [mi.name for mi in infos], [self._resolve(mi) for mi in infos],
                                                   batch_size, auto_transform_data)

    def predict(self, X, encode_to_label=True, batch_size=128, verbose=0, model_selector=consts.MODEL_SELECTOR_CURRENT,
                auto_transform_data=True, **kwargs):
        proba = self.predict_proba(X, batch_size=batch_size, verbose=verbose, model_selector=model_selector,
                                   auto_transform_data=auto_transform_data)
        if self.task == consts.TASK_REGRESSION:
            return proba.reshape(-1) if proba.shape[-1] == 1 else proba
        idx = proba.argmax(axis=-1)
        if encode_to_label and self.config.auto_encode_label:
            return self.preprocessor.inverse_transform_y(idx)
        return idx

    def proba2predict(self, proba, encode_to_label=True):
        """deeptable.py:581-597: regression outputs as they are; else the argmax of several columns, `> 0.5` of one, turned
        back into labels when asked"""
        if self.task == consts.TASK_REGRESSION:
            return proba
        if proba is None:
            raise ValueError('[proba] can not be none.')
        proba = np.asarray(proba)
        if proba.ndim == 1:
            proba = proba.reshape((-1, 1))
        predict = proba.argmax(axis=-1) if proba.shape[-1] > 1 else \
            (proba > 0.5).astype(consts.DATATYPE_PREDICT_CLASS).reshape(-1)
        return self.preprocessor.inverse_transform_y(predict) if encode_to_label else predict

    def evaluate(self, X_test, y_test, batch_size=256, verbose=0, model_selector=consts.MODEL_SELECTOR_CURRENT, **kwargs):
        model = self._one_model(model_selector)
        feed = self._feed_of(model, X_test, y_test)
        if isinstance(feed, tuple):
            return model.evaluate(feed[0], feed[1], batch_size=batch_size)
        return model.evaluate(feed, batch_size=batch_size)

    def apply(self, X, output_layers, concat_outputs=False, batch_size=128, verbose=0, transformer=None,
              model_selector=consts.MODEL_SELECTOR_CURRENT, auto_transform_data=True):
        model = self._one_model(model_selector)
        return model.apply(self.preprocessor.transform_X(X) if auto_transform_data else X, output_layers, concat_outputs,
                           batch_size, verbose, transformer)

    # -- persistence (deeptable.py:714-822) ------------------------------------------------------------------------------
    def save(self, filepath, deepmodel_basename=None):
        """The current model as '<deepmodel_basename or dt-1>.safetensors', every other model of the set as
        '<its name>.safetensors', and dt.pkl: the config, the preprocessor, 'model_file' (the current model, as before) and
        'modelset' (metric, mode, the current name, and per model its name, type, scores and file)."""
        self._require_model()
        os.makedirs(filepath, exist_ok=True)
        name = deepmodel_basename or 'dt-1'
        self.model.save(os.path.join(filepath, f'{name}.safetensors'))
        entries = []
        for mi in self._modelset.get_modelinfos():
            file = f'{name}.safetensors' if mi.name == self._current_model else f'{mi.name}.safetensors'
            if mi.name != self._current_model:
                self._resolve(mi).save(os.path.join(filepath, file))
            entries.append({'name': mi.name, 'type': mi.type, 'score': dict(mi.score), 'file': file})
        cfg = self.config._replace(distribute_strategy=None)      # strategy is stripped on pickle (deeptable.py:756-771)
        blob = {'config': cfg, 'preprocessor': self.preprocessor, 'model_file': f'{name}.safetensors',
                'modelset': {'metric': self._modelset.metric, 'best_mode': self._modelset.best_mode,
                             'current': self._current_model, 'models': entries}}
        with open(os.path.join(filepath, 'dt.pkl'), 'wb') as f:
            pickle.dump(blob, f, protocol=4)

    @staticmethod
    def load(filepath):
        """The current model is read at once; the other models of a saved set stay paths until `get_model` needs them.  A
        directory without the 'modelset' key (written before there was a set) loads as the one current model."""
        with open(os.path.join(filepath, 'dt.pkl'), 'rb') as f:
            blob = pickle.load(f)
        dt = DeepTable(config=blob['config'], preprocessor=blob['preprocessor'])
        dt.model = dt._load_deepmodel(os.path.join(filepath, blob['model_file']))
        saved = blob.get('modelset')
        if saved:
            dt._modelset = ModelSet(metric=saved['metric'], best_mode=saved['best_mode'])
            for e in saved['models']:
                current = e['name'] == saved['current']
                dt._modelset.push(ModelInfo(e['type'], e['name'], dt.model if current else os.path.join(filepath, e['file']),
                                            e['score']))
            dt._current_model = saved['current']
        return dt
