# -*- coding:utf-8 -*-
"""The models a `DeepTable` holds and how they rank (the interface of deeptables/models/modelset.py): `fit` leaves one model in
the set, `fit_cross_validation` one per fold; `DeepTable.get_model('best')` and `DeepTable.leaderboard` read the ranking.

A `ModelInfo.model` is a `DeepModel`, or the path of its weights file until `DeepTable.get_model` needs the model
(`DeepTable.load` restores a set that way)."""
import pandas as pd

from ..utils import consts

MAX_IS_BEST = ('acc', 'accuracy', 'auc', 'recall', 'precision')     # what best_mode 'auto' maximises; anything else: minimised


def _lower_keys(d):
    return {str(k).lower(): v for k, v in (d or {}).items()}


class ModelInfo:
    """One entry of a ModelSet.  score: {metric: value}, its keys lower-cased; empty (or None) and a `history=` among the meta:
    the last entry of every history key."""

    def __init__(self, type, name, model, score, **meta):
        self.type = type
        self.name = name
        self.model = model
        self.score = _lower_keys(score)
        self.meta = meta
        history = meta.get('history')
        if not self.score and history is not None:
            self.score = {str(k).lower(): history[k][-1] for k in history.keys() if len(history[k]) > 0}

    def get_score(self, metric_name):
        """the value under `metric_name` (any letter case); 0 when the model has no such score"""
        value = self.score.get(str(metric_name).lower())
        return 0 if value is None else value


class ModelSet:
    """An ordered set of ModelInfo with unique names, ranked by `metric` under best_mode 'max' | 'min' | 'auto'."""

    def __init__(self, metric=consts.METRIC_NAME_AUC, best_mode=consts.MODEL_SELECT_MODE_MAX):
        if best_mode not in (consts.MODEL_SELECT_MODE_MAX, consts.MODEL_SELECT_MODE_MIN, consts.MODEL_SELECT_MODE_AUTO):
            raise ValueError(f"best_mode must be 'max', 'min' or 'auto', got {best_mode!r}")
        self.best_mode = best_mode
        self.metric = str(metric).lower()
        self._infos = []

    def clear(self):
        self._infos = []

    def push(self, modelinfo):
        if self.get_modelinfo(modelinfo.name) is not None:
            raise ValueError(f'Duplicate model name is not allowed: a model named "{modelinfo.name}" is in the set already.')
        self._infos.append(modelinfo)

    def get_modelinfo(self, name):
        return next((mi for mi in self._infos if mi.name == name), None)

    def _maximise(self):
        mode = self.best_mode
        if mode == consts.MODEL_SELECT_MODE_AUTO:
            return self.metric in MAX_IS_BEST
        return mode == consts.MODEL_SELECT_MODE_MAX

    def _ranked(self):
        """the entries, best first; equal scores keep the order they were pushed in"""
        return sorted(self._infos, key=lambda mi: mi.get_score(self.metric), reverse=self._maximise())

    def best_model(self):
        if not self._infos:
            raise ValueError('Model set is empty.')
        return self._ranked()[0]

    def get_modelinfos(self, type=None):
        """in the order they were pushed"""
        return [mi for mi in self._infos if type is None or mi.type == type]

    def get_models(self, type=None):
        return [mi.model for mi in self.get_modelinfos(type)]

    def top_n(self, top=0, type=None):
        """the best `top` entries of `type` (top <= 0: all of them), best first"""
        ranked = [mi for mi in self._ranked() if type is None or mi.type == type]
        return ranked if top <= 0 else ranked[:top]

    def leaderboard(self, top=0, type=None):
        """A frame with one row per model, best first: 'model', 'type', then every score; the column of the sort metric is
        named '*<metric>'.  None for an empty set."""
        infos = self.top_n(top, type)
        if not infos:
            return None
        rows = []
        for mi in infos:
            row = {'model': mi.name, 'type': mi.type}
            for k, v in mi.score.items():
                row['*' + k if k == self.metric else k] = v
            rows.append(row)
        return pd.DataFrame(rows)
