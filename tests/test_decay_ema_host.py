# -*- coding:utf-8 -*-
"""CPU: keras.optimizers' `weight_decay` and `use_ema` / `ema_momentum` on the eight optimizer classes — arguments, refusals,
the serialised form, what a checkpoint carries, `exclude_from_weight_decay` — and the float64 restatements of
tests/decay_ema_reference.py against an independent AdamW and against the iterated average.  No kernel is launched."""
import numpy as np
import pytest
import torch

from tests import decay_ema_reference as R

STAGE_KEYS = ('weight_decay', 'use_ema', 'ema_momentum')


def _classes():
    from deeptables_amd import training as T
    return {'Adam': (T.KerasAdam, {}, T.KerasAdam), 'SGD': (T.SGD, {}, T.SGD),
            'MomentumSGD': (T.MomentumSGD, {}, T.MomentumSGD), 'SGD(momentum)': (T.SGD, {'momentum': 0.9}, T.MomentumSGD),
            'Adagrad': (T.Adagrad, {}, T.Adagrad), 'RMSprop': (T.RMSprop, {}, T.RMSprop), 'Adamax': (T.Adamax, {}, T.Adamax),
            'Ftrl': (T.Ftrl, {}, T.Ftrl)}


NAMES = list(_classes())


def _params():
    return [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(4, 2))]


@pytest.mark.parametrize('name', NAMES)
def test_every_class_takes_the_arguments_by_name(name):
    cls, kw, want = _classes()[name]
    off = cls(_params(), [], **kw)
    assert type(off) is want and off.weight_decay is None and off.use_ema is False and off.ema_momentum == 0.99
    assert not off.stages
    on = cls(_params(), [], **dict(kw, weight_decay=0.004, use_ema=True, ema_momentum=0.9))
    assert type(on) is want and on.weight_decay == 0.004 and on.use_ema is True and on.ema_momentum == 0.9 and on.stages
    assert cls(_params(), [], **dict(kw, weight_decay=0)).stages            # 0 is a decay that is set
    assert cls(_params(), [], **dict(kw, use_ema=True)).stages
    # no fused step may apply an un-decayed update
    assert not on.supports_row_segments and not on.supports_rows_in_step
    assert off.supports_row_segments == bool(off._row_segments) and off.supports_rows_in_step == bool(off._rows_in_step)


@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('bad', [dict(weight_decay=-1e-3), dict(weight_decay=float('inf')), dict(weight_decay=float('nan')),
                                 dict(weight_decay='0.1'), dict(weight_decay=True), dict(ema_momentum=-0.1),
                                 dict(ema_momentum=1.5), dict(ema_momentum=float('nan')), dict(ema_momentum=None),
                                 dict(use_ema=1), dict(use_ema=True, ema_overwrite_frequency=10),
                                 dict(ema_overwrite_frequency=1)])
def test_bad_arguments_raise_value_error(name, bad):
    cls, kw, _ = _classes()[name]
    with pytest.raises(ValueError):
        cls(_params(), [], **dict(kw, **bad))


@pytest.mark.parametrize('class_name,extra,want', [('Adam', {}, 'KerasAdam'), ('SGD', {}, 'SGD'),
                                                   ('SGD', {'momentum': 0.5}, 'MomentumSGD'), ('Adagrad', {}, 'Adagrad'),
                                                   ('RMSprop', {}, 'RMSprop'), ('Adamax', {}, 'Adamax'), ('Ftrl', {}, 'Ftrl'),
                                                   ('adam', {'clipnorm': 1.0}, 'KerasAdam')])
def test_the_serialised_form_carries_the_keys(class_name, extra, want):
    from deeptables_amd import training as T
    spec = {'class_name': class_name, 'config': dict(extra, weight_decay=0.004, use_ema=True, ema_momentum=0.5,
                                                     ema_overwrite_frequency=None)}
    opt = T.make_optimizer(spec, _params(), [])
    assert type(opt).__name__ == want and (opt.weight_decay, opt.use_ema, opt.ema_momentum) == (0.004, True, 0.5)
    for key in STAGE_KEYS + ('ema_overwrite_frequency',):
        assert key in T._config_keys(T.OPTIMIZERS[class_name.lower()])
    with pytest.raises(ValueError, match='unknown config keys'):
        T.make_optimizer({'class_name': class_name, 'config': {'weight_decay_rate': 0.1}}, _params(), [])
    with pytest.raises(ValueError, match='ema_overwrite_frequency'):
        T.make_optimizer({'class_name': class_name, 'config': {'ema_overwrite_frequency': 5}}, _params(), [])


@pytest.mark.parametrize('name', NAMES)
def test_hyperparameters_name_the_keys_only_when_set(name):
    cls, kw, _ = _classes()[name]
    off = cls(_params(), [], **kw)
    assert not set(off.hyperparameters()) & set(STAGE_KEYS)
    decay = cls(_params(), [], **dict(kw, weight_decay=0.25))
    assert decay.hyperparameters() == dict(off.hyperparameters(), weight_decay=0.25)
    ema = cls(_params(), [], **dict(kw, use_ema=True, ema_momentum=0.75))
    assert ema.hyperparameters() == dict(off.hyperparameters(), use_ema=True, ema_momentum=0.75)
    both = cls(_params(), [], **dict(kw, weight_decay=0.25, use_ema=True, clipvalue=2.0))
    assert both.hyperparameters() == dict(off.hyperparameters(), weight_decay=0.25, use_ema=True, ema_momentum=0.99,
                                          clipvalue=2.0)
    # what a checkpoint hands back
    fresh = cls(_params(), [], **kw)
    fresh.set_hyperparameters(both.hyperparameters())
    assert fresh.hyperparameters() == both.hyperparameters() and fresh.stages
    assert (fresh.weight_decay, fresh.use_ema, fresh.ema_momentum, fresh.clipvalue) == (0.25, True, 0.99, 2.0)
    before = fresh.hyperparameters()
    for bad in ({'weight_decay': -1.0}, {'ema_momentum': 2.0}):
        with pytest.raises(ValueError):
            fresh.set_hyperparameters(bad)
        assert fresh.hyperparameters() == before                             # a refused update changes nothing
    fresh.set_hyperparameters({'learning_rate': 0.5} if 'learning_rate' in before else {})
    assert fresh.weight_decay == 0.25 and fresh.use_ema                      # keys that are not named stay


def test_exclude_from_weight_decay_by_list_and_by_pattern():
    from deeptables_amd import training as T
    table = torch.nn.Parameter(torch.zeros(10, 4))
    columns = [table.data[0:3], table.data[3:7], table.data[7:10]]
    kernel, bias = torch.nn.Parameter(torch.zeros(4, 2)), torch.nn.Parameter(torch.zeros(2))
    names = {'emb/embeddings_0': columns[0], 'emb/embeddings_1': columns[1], 'emb/embeddings_2': columns[2],
             'dnn_dense_1/kernel': kernel, 'dnn_dense_1/bias': bias}
    opt = T.KerasAdam([table, kernel, bias], [], weight_decay=0.01)
    opt.set_variable_names(lambda: names)
    assert opt.decay_exclusions() == [] and opt._excluded_tensors() == []
    opt.exclude_from_weight_decay(var_list=[columns[1]], var_names=['bias$'])
    opt.exclude_from_weight_decay(var_names=['embeddings_2'])
    got = opt._excluded_tensors()
    assert len(got) == 3 and got[0] is columns[1] and got[1] is columns[2] and got[2] is bias
    skip = [(t.data_ptr(), t.data_ptr() + 4 * t.numel()) for t in got]
    decays = {n: opt._decays(skip, t.data_ptr(), t.numel()) for n, t in names.items()}
    assert decays == {'emb/embeddings_0': True, 'emb/embeddings_1': False, 'emb/embeddings_2': False,
                      'dnn_dense_1/kernel': True, 'dnn_dense_1/bias': False}
    # what a checkpoint stores: the patterns, and the listed tensors by their exact names
    assert opt.decay_exclusions() == ['bias$', 'embeddings_2', '^emb/embeddings_1$']
    # a parameter of var_list covers every variable inside it
    whole = T.SGD([table, kernel], [], weight_decay=0.01)
    whole.set_variable_names(names)
    whole.exclude_from_weight_decay(var_list=[table])
    assert whole.decay_exclusions() == ['^emb/embeddings_0$', '^emb/embeddings_1$', '^emb/embeddings_2$']
    # patterns need names; a bad pattern is refused at once; after the first step the set is closed
    blind = T.Adagrad([kernel], [], weight_decay=0.01)
    blind.exclude_from_weight_decay(var_names=['kernel'])
    with pytest.raises(ValueError, match='names'):
        blind._excluded_tensors()
    with pytest.raises(Exception):
        opt.exclude_from_weight_decay(var_names=['('])
    opt._stage_started = True
    with pytest.raises(ValueError, match='before the first step'):
        opt.exclude_from_weight_decay(var_list=[kernel])


@pytest.mark.parametrize('k', [0, 1, 8, 9, 1000])
def test_the_closed_form_catch_up_is_k_average_steps_on_a_constant_weight(k):
    """float64 round-off of at most a few dozen operations on O(1) values (k = 1000: the iterated average has converged to w
    within 0.99^1000 = 4e-5 of the start, both sides agree on that remainder to its own round-off): 1e-12"""
    rng = np.random.RandomState(k)
    a0, w = rng.randn(64), rng.randn(64)
    for m in (0.0, 0.5, 0.99, 1.0):
        a = a0.copy()
        for t in range(k):
            a = R.ema(a, w, m, t + 2)                   # (never the first step: m_eff = m)
        assert np.abs(R.catch_up(a0, w, m, k) - a).max() <= 1e-12, (m, k)
    assert np.array_equal(R.ema(a0, w, 0.99, 1), w)     # the first step copies the weights whatever the momentum


def test_decay_then_keras_adam_is_adamw():
    """the float64 restatement against torch.optim.AdamW (CPU, float64, eps = 0, non-zero gradients, 5 steps) to 1e-12:
    float64 round-off of a few dozen operations on O(1) values.  Pins the decay's place (before the update, which sees the
    gradient as given) and its plain learning rate."""
    rng = np.random.RandomState(0)
    p0 = rng.randn(257)
    grads = [rng.randn(257) + np.where(rng.rand(257) < 0.5, 2.0, -2.0) for _ in range(5)]
    lr, wd = 1e-2, 0.3
    p = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.AdamW([p], lr=lr, betas=(0.9, 0.999), eps=0.0, weight_decay=wd)
    for g in grads:
        p.grad = torch.from_numpy(g.copy())
        opt.step()
    got = R.adamw_steps(p0, grads, wd, lr=lr, epsilon=0.0)
    err = float(np.abs(got - p.detach().numpy()).max())
    print('largest difference', err)
    assert err <= 1e-12
    # ... and the decay matters at this bar: without it, or with a bias-corrected rate in it, the result is elsewhere
    assert np.abs(R.adamw_steps(p0, grads, 0.0, lr=lr, epsilon=0.0) - p.detach().numpy()).max() > 1e-4


def test_float32_restatements_follow_the_stated_order():
    p = np.array([1.0, -3.0, 1e-30, 0.0, 123456.789], dtype=np.float32)
    wd, lr = 0.004, 1e-3
    want = (p - (p * np.float32(wd)).astype(np.float32) * np.float32(lr)).astype(np.float32)
    assert R.decay32(p, wd, lr).dtype == np.float32 and np.array_equal(R.decay32(p, wd, lr), want)
    a = np.array([0.5, 0.25, -1.0, 2.0, 7.0], dtype=np.float32)
    assert np.array_equal(R.ema32(a, p, 0.99, 1), p)
    m = np.float32(0.99)
    assert np.array_equal(R.ema32(a, p, 0.99, 2), m * a + (np.float32(1) - m) * p)
    assert np.abs(R.ema(a, p, 0.99, 2) - R.ema32(a, p, 0.99, 2)).max() <= 2.0 ** -22 * np.abs(p).max()
