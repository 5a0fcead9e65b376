# -*- coding:utf-8 -*-
"""CPU: models/modelset.py — ordering under max, min and auto, the score of a missing metric, duplicate names, scores read
from a history, and the leaderboard's columns and '*' mark."""
import pytest

from deeptables_amd.models.modelset import ModelInfo, ModelSet


def _set(metric, mode, scores):
    ms = ModelSet(metric=metric, best_mode=mode)
    for name, score in scores:
        ms.push(ModelInfo('val', name, object(), score))
    return ms


SCORES = [('a', {'AUC': 0.7, 'loss': 0.5}), ('b', {'auc': 0.9, 'loss': 0.6}), ('c', {'Auc': 0.8, 'loss': 0.4})]


def test_ordering_under_max_min_and_auto():
    assert [m.name for m in _set('AUC', 'max', SCORES).top_n()] == ['b', 'c', 'a']
    assert [m.name for m in _set('AUC', 'min', SCORES).top_n()] == ['a', 'c', 'b']
    assert [m.name for m in _set('auc', 'auto', SCORES).top_n()] == ['b', 'c', 'a']            # auto: auc is maximised
    assert [m.name for m in _set('loss', 'auto', SCORES).top_n()] == ['c', 'a', 'b']           # ... anything else minimised
    for metric in ('acc', 'accuracy', 'AUC', 'recall', 'Precision'):
        ms = _set(metric, 'auto', [('lo', {metric: 0.1}), ('hi', {metric: 0.9})])
        assert ms.best_model().name == 'hi', metric
    for metric in ('loss', 'mse', 'val_auc', 'rmse'):
        ms = _set(metric, 'auto', [('hi', {metric: 0.9}), ('lo', {metric: 0.1})])
        assert ms.best_model().name == 'lo', metric
    ms = _set('AUC', 'max', SCORES)
    assert [m.name for m in ms.top_n(2)] == ['b', 'c'] and [m.name for m in ms.top_n(7)] == ['b', 'c', 'a']
    assert [m.name for m in ms.get_modelinfos()] == ['a', 'b', 'c']                           # pushed order is kept
    assert len(ms.get_models()) == 3 and ms.get_models(type='other') == [] and ms.top_n(type='other') == []
    assert ms.get_modelinfo('b').name == 'b' and ms.get_modelinfo('zz') is None
    with pytest.raises(ValueError):
        ModelSet('auc', 'best')
    ms.clear()
    assert ms.get_modelinfos() == [] and ms.leaderboard() is None
    with pytest.raises(ValueError, match='empty'):
        ms.best_model()


def test_a_missing_metric_scores_zero():
    mi = ModelInfo('val', 'm', None, {'loss': 0.3})
    assert mi.get_score('AUC') == 0 and mi.get_score('LOSS') == 0.3
    ms = _set('auc', 'max', [('none', {'loss': 0.1}), ('neg', {'auc': -0.5}), ('pos', {'auc': 0.2})])
    assert [m.name for m in ms.top_n()] == ['pos', 'none', 'neg']


def test_duplicate_names_are_refused():
    ms = _set('auc', 'max', SCORES)
    with pytest.raises(ValueError, match='Duplicate'):
        ms.push(ModelInfo('val', 'b', None, {'auc': 1.0}))
    assert len(ms.get_modelinfos()) == 3


def test_scores_come_from_the_history():
    history = {'loss': [0.9, 0.5], 'AUC': [0.6, 0.75], 'val_AUC': [0.55, 0.7]}
    mi = ModelInfo('val', 'm', None, {}, history=history)
    assert mi.score == {'loss': 0.5, 'auc': 0.75, 'val_auc': 0.7} and mi.meta['history'] is history
    assert ModelInfo('val', 'm', None, None, history=history).score == mi.score
    assert ModelInfo('val', 'm', None, {'AUC': 1.0}, history=history).score == {'auc': 1.0}    # a given score is kept
    assert ModelInfo('val', 'm', None, {}).score == {} and ModelInfo('val', 'm', None, {}, history=None).score == {}


def test_leaderboard_columns_and_mark():
    board = _set('AUC', 'max', SCORES).leaderboard()
    assert list(board.columns) == ['model', 'type', '*auc', 'loss']
    assert board['model'].tolist() == ['b', 'c', 'a'] and board['type'].tolist() == ['val'] * 3
    assert board['*auc'].tolist() == [0.9, 0.8, 0.7] and board['loss'].tolist() == [0.6, 0.4, 0.5]
    assert _set('AUC', 'max', SCORES).leaderboard(top=1)['model'].tolist() == ['b']
    board = _set('f1', 'max', SCORES).leaderboard()                  # a sort metric no model has: no column is marked
    assert list(board.columns) == ['model', 'type', 'auc', 'loss']
