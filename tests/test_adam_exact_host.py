# -*- coding:utf-8 -*-
"""Host: training.KerasAdam(exact_rows=True) — the catch-up routine's exit rule on a float32 numpy mirror
(tests/adam_exact_reference.py), the bound the constructor checks, and the mode's plumbing through make_optimizer and
hyperparameters().  No GPU: nothing here makes a launch."""
import os
import re

import numpy as np
import pytest

from deeptables_amd import _lib, training
from tests import adam_exact_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STARTS = (1, 2, 28, 1000, 10 ** 5)                   # the step of the first idle step that is owed
GAPS = (1, 8, 9, 200, 2000)
DECADES = tuple(10.0 ** -e for e in range(1, 7))     # m and v over six decades
PS = (0.0, 1e-30, 0.05, -3.0)


@pytest.fixture(scope='module')
def grid():
    """every (start, gap, m, v, p) with both signs of m -> the mirror with and without the early exit and float64, once"""
    S, K, M, V, P = (a.reshape(-1) for a in np.meshgrid(STARTS, GAPS, DECADES, DECADES, PS, indexing='ij'))
    S, K = np.concatenate([S, S]), np.concatenate([K, K])
    M, V, P = np.concatenate([M, -M]), np.concatenate([V, V]), np.concatenate([P, P])
    done = S - 1                                      # the state is current through the step before
    return {'k': K,
            'exit': R.idle_steps_f32(P, M, V, done, K, early_exit=True),
            'full': R.idle_steps_f32(P, M, V, done, K, early_exit=False),
            'f64': R.idle_steps_f64(P, M, V, done, K)}


def test_early_exit_leaves_the_weight_bit_for_bit(grid):
    """the loop that stops at the first step with p unchanged and |term| < 2^-26 |p| gives the float32 p of the loop that
    takes every step, on the whole grid; it is short (the issue's random cases never needed more than 215 trips; the grid's
    p = 0 and p = 1e-30 run until the term underflows)"""
    a, b = grid['exit'], grid['full']
    assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32))
    assert np.array_equal(b[3], grid['k'])            # (the switch is real: the full loop took every step)
    assert a[3].max() < 300 < b[3].max()
    print(f'longest early-exit loop on the grid: {a[3].max()} trips of {b[3].max()}')


def test_mirror_agrees_with_float64_no_worse_than_the_full_loop(grid):
    """against the float64 step-by-step result the early exit is held to the error the float32 FULL loop itself shows on the
    grid: p absolutely (it is the same bits), m and v relative to their value (a decay is a product: the full loop rounds
    once per step, the early exit once per step up to its exit and then a powf and a product), with the float32 denormal
    spacing as the floor of the scale"""
    a, b, r = grid['exit'], grid['full'], grid['f64']
    tiny = 2.0 ** -126
    for i, name in enumerate(('p', 'm', 'v')):
        scale = 1.0 if i == 0 else np.maximum(np.abs(r[i]), tiny)
        err_exit = (np.abs(a[i].astype(np.float64) - r[i]) / scale).max()
        err_full = (np.abs(b[i].astype(np.float64) - r[i]) / scale).max()
        print(f'{name}: early exit {err_exit:.3e}, full loop {err_full:.3e}')
        assert err_exit <= err_full, name
        assert err_full < (2e-6 if i == 0 else 4e-6), name        # (and the full loop is float32 Adam, not something else)


def test_idle_term_ratio_bound():
    """rho = sup_t (lr_{t+1} / lr_t) beta_1 / sqrt(beta_2): Keras' defaults give 0.911 (attained at t = 28); betas for which a
    term may exceed the one before it are refused, and the message names the cause"""
    rho = training.KerasAdam.idle_term_ratio(0.9, 0.999)
    assert 0.91 < rho < 0.92
    t = np.arange(1, 4000, dtype=np.float64)
    lr_t = np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
    ratio = lr_t[1:] / lr_t[:-1]
    assert int(t[ratio.argmax()]) == 28 and abs(rho - ratio.max() * 0.9 / np.sqrt(0.999)) < 1e-12
    assert training.KerasAdam.idle_term_ratio(0.99, 0.9) >= 1
    assert training.KerasAdam.idle_term_ratio(0.0, 0.999) == 0
    with pytest.raises(ValueError, match=r'beta_1 < sqrt\(beta_2\)'):
        training.KerasAdam([], [], beta_1=0.99, beta_2=0.9, exact_rows=True)
    training.KerasAdam([], [], beta_1=0.99, beta_2=0.9)           # the lazy default takes any betas, as before
    with pytest.raises(ValueError, match='exact_rows'):
        training.KerasAdam([], [], exact_rows=1)


class _Layer:
    """what the optimizer touches of a MultiColumnEmbedding at construction"""

    def __init__(self):
        self.sparse_grads = {}
        self.pre_lookup = None


def test_make_optimizer_and_refusals():
    layer = _Layer()
    opt = training.make_optimizer({'class_name': 'Adam', 'config': {'exact_rows': True}}, [], [layer])
    assert isinstance(opt, training.KerasAdam) and opt.exact_rows
    assert callable(layer.pre_lookup)                              # the layers' hook is the optimizer's
    assert not opt.supports_row_segments and not opt.supports_rows_in_step
    lazy = training.make_optimizer('adam', [], [_Layer()])
    assert not lazy.exact_rows and lazy.supports_row_segments and lazy.supports_rows_in_step
    assert lazy.embedding_layers[0].pre_lookup is None
    for extra in ({'weight_decay': 1e-4}, {'use_ema': True}):
        with pytest.raises(ValueError, match='exact_rows'):
            training.KerasAdam([], [], exact_rows=True, **extra)
    training.KerasAdam([], [], exact_rows=True, clipnorm=1.0)      # clipping acts on gradients only
    from deeptables_amd.models.deepmodel import DeepModel
    dm = DeepModel.__new__(DeepModel)                              # (what fit and train_step ask before they start)
    dm.optimizer = opt
    dm._refuse_clipping_under(None)
    with pytest.raises(ValueError, match='exact_rows'):
        dm._refuse_clipping_under(object())
    assert dm.fused_plan() is None


def test_hyperparameters_round_trip():
    opt = training.KerasAdam([], [_Layer()], exact_rows=True, clipvalue=0.5)
    hp = opt.hyperparameters()
    assert hp == {'clipvalue': 0.5, 'exact_rows': True}
    other = training.KerasAdam([], [_Layer()])
    assert other.hyperparameters() == {}                           # (only what is set, as for the clip and the stages)
    other.set_hyperparameters(hp)                                  # what checkpoint.load_model does
    assert other.exact_rows and other.clipvalue == 0.5 and callable(other.embedding_layers[0].pre_lookup)
    assert other.hyperparameters() == hp
    other.set_hyperparameters({'exact_rows': False})
    assert not other.exact_rows and other.embedding_layers[0].pre_lookup is None and other.clipvalue == 0.5
    with pytest.raises(ValueError, match='exact_rows'):
        opt.set_hyperparameters({'use_ema': True})


def test_entry_points_are_declared_bound_and_documented():
    header = open(os.path.join(ROOT, 'include', 'dt_hip.h')).read()
    guide = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in ('dt_adam_exact_supported', 'dt_adam_rows_catchup', 'dt_adam_rows_materialize', 'dt_adam_rows_stamp'):
        assert name in _lib.SIGNATURES and re.search(r'\b' + name + r'\(', header) and name in guide, name
    assert 'deepmodel.py:319-322' in header[header.index('csrc/adam_exact.hip'):]
