# -*- coding:utf-8 -*-
"""Momentum SGD, Adamax and Ftrl without a GPU: what `make_optimizer` accepts (names and Keras' serialised dict), the refused
hyperparameters, `SGD(momentum=0)` as the class and code path it was, the float64 restatements the GPU tests compare against
(tests/optimizers2_reference.py) pinned on hand-computed cases, and the argument checks of the nine entry points
(csrc/optim_slots.hip)."""
import ctypes
import functools
import math
import os
import re

import pytest
import torch

from tests import optimizers2_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = tuple(f'dt_{k}_{form}_step' for k in ('sgdm', 'adamax', 'ftrl') for form in ('dense', 'multi', 'rows'))


def _w():
    return torch.nn.Parameter(torch.zeros(3))


def test_make_optimizer_takes_the_new_names_with_keras_defaults():
    from deeptables_amd import training as T
    w = _w()
    for name in ('ftrl', 'Ftrl', 'FTRL'):
        opt = T.make_optimizer(name, [w], [])
        assert type(opt) is T.Ftrl and opt._name == 'Ftrl' and opt.hyperparameters() == R.FTRL_DEFAULTS
        assert opt.slot_names == ('accumulator', 'linear') and opt._slot_inits() == (0.1, 0.0)
    for name in ('adamax', 'Adamax'):
        opt = T.make_optimizer(name, [w], [])
        assert type(opt) is T.Adamax and opt._name == 'Adamax' and opt.hyperparameters() == R.ADAMAX_DEFAULTS
        assert opt.slot_names == ('m', 'u') and opt._slot_inits() == (0.0, 0.0)
    for opt in (T.make_optimizer('ftrl', [w], []), T.make_optimizer('adamax', [w], []), T.SGD([w], [], momentum=0.9)):
        assert opt.t == 0 and opt.state == {} and opt.pre_dense_hook is None
        assert not opt.supports_rows_in_step and not opt.supports_row_segments      # the fused plans leave them the update
        assert hasattr(opt, 'register_flat_group') and opt.lr == opt.learning_rate
    with pytest.raises(ValueError, match='Unsupported optimizer') as e:
        T.make_optimizer('nadam', [w], [])
    assert all(repr(n) in str(e.value) for n in ('adam', 'sgd', 'adagrad', 'rmsprop', 'ftrl', 'adamax'))
    assert 'class_name' in str(e.value)


def test_make_optimizer_takes_keras_serialised_dicts():
    from deeptables_amd import training as T
    w = _w()
    opt = T.make_optimizer({'class_name': 'Ftrl', 'config': {'l1_regularization_strength': 1e-4, 'beta': 0.5}}, [w], [])
    assert type(opt) is T.Ftrl
    assert opt.hyperparameters() == dict(R.FTRL_DEFAULTS, l1_regularization_strength=1e-4, beta=0.5)
    opt = T.make_optimizer({'class_name': 'SGD', 'config': {'momentum': 0.9, 'nesterov': True}}, [w], [])
    assert type(opt) is T.MomentumSGD and opt._name == 'SGD'
    assert opt.hyperparameters() == {'learning_rate': 0.01, 'momentum': 0.9, 'nesterov': True}
    assert type(T.make_optimizer({'class_name': 'SGD', 'config': {'learning_rate': 0.1}}, [w], [])) is T.SGD
    assert type(T.make_optimizer({'class_name': 'sgd'}, [w], [])) is T.SGD
    # every optimizer of OPTIMIZERS, with one of its own hyperparameters
    for name, cls, cfg in (('Adam', T.KerasAdam, {'beta_2': 0.99}), ('Adagrad', T.Adagrad, {'initial_accumulator_value': 0.5}),
                           ('RMSprop', T.RMSprop, {'rho': 0.8}), ('Adamax', T.Adamax, {'beta_1': 0.8})):
        opt = T.make_optimizer({'class_name': name, 'config': cfg}, [w], [])
        assert type(opt) is cls
    assert T.make_optimizer({'class_name': 'Adamax', 'config': {'beta_1': 0.8}}, [w], []).beta_1 == 0.8
    assert T.make_optimizer({'class_name': 'Adam', 'config': {'beta_2': 0.99}}, [w], []).b2 == 0.99
    assert set(T.OPTIMIZERS) == {'adam', 'sgd', 'adagrad', 'rmsprop', 'ftrl', 'adamax'}
    for bad in ({'class_name': 'Ftrl', 'config': {'l1': 0.1}}, {'class_name': 'Adamax', 'config': {'amsgrad': True}},
                {'class_name': 'SGD', 'config': {'momentum': 0.9, 'dampening': 0.1}},
                {'class_name': 'Adam', 'config': {'params': []}}):
        with pytest.raises(ValueError, match='unknown config keys'):
            T.make_optimizer(bad, [w], [])
    with pytest.raises(ValueError, match='Unsupported optimizer'):
        T.make_optimizer({'class_name': 'Nadam', 'config': {}}, [w], [])
    # the callable form keeps working
    opt = T.make_optimizer(functools.partial(T.Ftrl, l1_regularization_strength=1e-4), [w], [])
    assert type(opt) is T.Ftrl and opt.l1_regularization_strength == 1e-4


def test_refused_hyperparameters_raise_value_error():
    from deeptables_amd import training as T
    w = _w()
    for kw in ({'initial_accumulator_value': -0.1}, {'learning_rate_power': 0.5}, {'l1_regularization_strength': -1e-3},
               {'l2_regularization_strength': -1e-3}, {'l2_shrinkage_regularization_strength': -1e-3}, {'beta': -0.1}):
        with pytest.raises(ValueError, match=next(iter(kw))):
            T.Ftrl([w], [], **kw)
        with pytest.raises(ValueError, match=next(iter(kw))):
            T.make_optimizer({'class_name': 'Ftrl', 'config': kw}, [w], [])
        opt = T.Ftrl([w], [])
        with pytest.raises(ValueError, match=next(iter(kw))):
            opt.set_hyperparameters(kw)
        assert opt.hyperparameters() == R.FTRL_DEFAULTS                   # a refused update changes nothing
    T.Ftrl([w], [], initial_accumulator_value=0.0, learning_rate_power=0.0)      # the edges are accepted
    for m in (-0.1, 1.5):
        with pytest.raises(ValueError, match='momentum'):
            T.SGD([w], [], momentum=m)
        with pytest.raises(ValueError, match='momentum'):
            T.MomentumSGD([w], [], momentum=m)
    assert type(T.SGD([w], [], momentum=1.0)) is T.MomentumSGD
    opt = T.Adamax([w], [])
    opt.set_hyperparameters({'learning_rate': 0.01, 'beta_2': 0.99})
    assert opt.hyperparameters() == dict(R.ADAMAX_DEFAULTS, learning_rate=0.01, beta_2=0.99)
    with pytest.raises(ValueError, match='unknown hyperparameters'):
        opt.set_hyperparameters({'rho': 0.9})


def test_sgd_without_momentum_is_the_class_and_code_path_it_was():
    from deeptables_amd import training as T
    w = _w()
    for opt in (T.SGD([w], []), T.SGD([w], [], 0.05), T.SGD([w], [], learning_rate=0.05, momentum=0.0, nesterov=True),
                T.make_optimizer('sgd', [w], [])):
        assert type(opt) is T.SGD and opt._name == 'SGD' and not isinstance(opt, T._DeviceOptimizer)
        # no step-driver state: no slots, no device step counter, no flat group
        for attr in ('state', '_dev_state', '_flat', 'slot_names', 'register_flat_group', 'pre_dense_hook', 't'):
            assert not hasattr(opt, attr), attr
        assert opt.params == [w] and opt.embedding_layers == []
        assert opt.hyperparameters()['momentum'] == 0.0
    assert T.SGD([w], [], 0.05).lr == 0.05 and T.SGD([w], []).lr == 0.01
    # its step is the per-tensor launch it was: the dense entry point of the momentum-free kernel, nothing else
    import inspect
    src = inspect.getsource(T.SGD.step)
    assert 'dt_sgd_dense_step' in src and 'dt_sgd_rows_step' in src and 'dt_sgdm' not in src
    m = T.SGD([w], [], momentum=0.5)
    assert isinstance(m, T._DeviceOptimizer) and m._name == 'SGD' and m.slot_names == ('momentum',)


def test_float64_references_reproduce_hand_computed_steps():
    """two elements, w0 = (1, 1), gradients (0.5, -2), then (-2, 0.5)"""
    t = lambda *x: torch.tensor(x, dtype=torch.float64)
    w0, g1, g2 = t(1.0, 1.0), t(0.5, -2.0), t(-2.0, 0.5)
    # SGD, lr 0.01, mu 0.9: m1 = -lr g1; m2 = 0.9 m1 - lr g2
    w, m = R.sgdm_step(w0, g1, t(0.0, 0.0))
    assert torch.allclose(m, t(-0.005, 0.02), atol=1e-17) and torch.allclose(w, t(0.995, 1.02), atol=1e-15)
    w, m = R.sgdm_step(w, g2, m)
    assert torch.allclose(m, t(0.0155, 0.013), atol=1e-17) and torch.allclose(w, t(1.0105, 1.033), atol=1e-15)
    w, m = R.sgdm_step(w0, g1, t(0.0, 0.0), nesterov=True)             # p + mu m - lr g = 1 + 0.9 * (-0.005) - 0.005
    assert torch.allclose(w, t(0.9905, 1.038), atol=1e-15) and torch.allclose(m, t(-0.005, 0.02), atol=1e-17)
    # Adamax at t = 1: m = 0.1 g, u = |g|, 1 - b1 = 0.1: p - lr sign(g) |g| / (|g| + eps)
    w, m, u = R.adamax_step(w0, g1, t(0.0, 0.0), t(0.0, 0.0), 1)
    want = [1.0 - 1e-3 * s * a / (a + 1e-7) for s, a in ((1.0, 0.5), (-1.0, 2.0))]
    assert torch.allclose(w, t(*want), atol=1e-15) and torch.allclose(m, t(0.05, -0.2), atol=1e-16) and u.tolist() == [0.5, 2.0]
    w2, m2, u2 = R.adamax_step(w, g2, m, u, 2)
    assert u2.tolist() == [2.0, 0.999 * 2.0]                            # max(b2 u, |g|)
    assert torch.allclose(m2, t(0.05 + (-2.0 - 0.05) * 0.1, -0.2 + (0.5 + 0.2) * 0.1), atol=1e-16)
    assert abs(w2[0].item() - (want[0] - 1e-3 * m2[0].item() / (0.19 * (2.0 + 1e-7)))) < 1e-15
    # Ftrl, defaults: n 0.1 -> 0.35, linear = g - (sqrt(.35) - sqrt(.1)) / lr * w, w = -linear / (sqrt(.35) / lr)
    w, n, lin = R.ftrl_step(w0[:1], g1[:1], t(0.1), t(0.0))
    lin_want = 0.5 - (math.sqrt(0.35) - math.sqrt(0.1)) / 1e-3
    assert abs(n.item() - 0.35) < 1e-15 and abs(lin.item() - lin_want) < 1e-10
    assert abs(w.item() - (-lin_want / (math.sqrt(0.35) / 1e-3))) < 1e-14 and 0.4 < w.item() < 0.5
    # ... with g = 0 at step 1 the never-trained weight becomes exactly 0: linear = 0 - 0 * w, w = (0 - 0) / q
    w, n, lin = R.ftrl_step(w0, t(0.0, 0.0), t(0.1, 0.1), t(0.0, 0.0))
    assert w.tolist() == [0.0, 0.0] and n.tolist() == [0.1, 0.1] and lin.tolist() == [0.0, 0.0]
    # ... l1 clips: |linear| <= l1 gives exactly 0; beyond it the weight is (sign(linear) l1 - linear) / q
    w, n, lin = R.ftrl_step(t(0.0, 0.0), t(0.01, 2.0), t(0.1, 0.1), t(0.0, 0.0), l1=0.02, l2=0.01, beta=0.1)
    assert lin.tolist() == [0.01, 2.0] and w[0].item() == 0.0
    q = math.sqrt(4.1) / 1e-3 + 2 * (0.01 + 0.1 / 2e-3)
    assert abs(w[1].item() - (0.02 - 2.0) / q) < 1e-15
    # ... shrinkage enters linear, not the accumulator; another power
    w, n, lin = R.ftrl_step(t(1.0), t(0.5), t(0.1), t(0.0), lr_power=-0.7, l2_shrinkage=0.01)
    assert abs(n.item() - 0.35) < 1e-15
    assert abs(lin.item() - (0.5 + 0.02 - (0.35 ** 0.7 - 0.1 ** 0.7) / 1e-3)) < 1e-10
    # ... q == 0 (accumulator 0, gradient 0, no l2): 0, not NaN
    w, n, lin = R.ftrl_step(t(0.0), t(0.0), t(0.0), t(0.0))
    assert w.item() == 0.0 and n.item() == 0.0 and lin.item() == 0.0
    # a sparse gradient: duplicates are summed before the update, skipped lookups (-1) contribute nothing, other rows keep all
    p0 = torch.ones(3, 2, dtype=torch.float64)
    rows = torch.tensor([2, -1, 2, 0])
    vals = torch.tensor([[0.25, 0.0], [9.0, 9.0], [0.25, 1.0], [-2.0, 0.0]], dtype=torch.float64)
    p1, (m1,) = R.rows_step(R.sgdm_step, p0, (torch.zeros_like(p0),), rows, vals)
    assert torch.allclose(m1, t([0.02, 0.0], [0.0, 0.0], [-0.005, -0.01]).reshape(3, 2), atol=1e-17)
    assert torch.equal(p1[1], p0[1]) and abs(p1[2, 0].item() - 0.995) < 1e-15
    p1, (n1, l1) = R.rows_step(R.ftrl_step, p0, (torch.full_like(p0, 0.1), torch.zeros_like(p0)), rows, vals, l2_shrinkage=0.01)
    assert torch.equal(p1[1], p0[1]) and n1[1].tolist() == [0.1, 0.1] and l1[1].tolist() == [0.0, 0.0]   # no shrinkage there
    assert p1[2, 1].item() != 1.0 and p1[0, 1].item() != 1.0            # a touched row's zero-gradient element does move
    p1, (m1, u1) = R.rows_step(R.adamax_step, p0, (torch.zeros_like(p0), torch.zeros_like(p0)), rows, vals, 1)
    assert u1.tolist() == [[2.0, 0.0], [0.0, 0.0], [0.5, 1.0]] and torch.equal(p1[1], p0[1])


def test_header_exports_and_binding_name_the_same_entry_points():
    from deeptables_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'dt_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(dt_(?:sgdm|adamax|ftrl)_[a-z0-9_]+)\s*\(', text))
    assert declared == set(ENTRIES) == {n for n in _lib.SIGNATURES if n.startswith(('dt_sgdm_', 'dt_adamax_', 'dt_ftrl_'))}
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(handle, n) for n in ENTRIES)


HP = {'sgdm': (0.01, 0.9, 0), 'adamax': (1e-3, 0.9, 0.999, 1e-7), 'ftrl': (1e-3, -0.5, 0.0, 0.0, 0.0)}
NSLOTS = {'sgdm': 1, 'adamax': 2, 'ftrl': 2}
P, P2, P3 = 0x10000, 0x20000, 0x30000     # 16-byte aligned, far apart
Q, ODD = 0x10004, 0x10002                 # float aligned only / not even float aligned


def _refused(lib, name, *args):
    assert getattr(lib, name)(*args) != 0, (name, args)
    err = lib.dt_last_error()
    assert name.encode() in err and b'launch failed' not in err, err


@pytest.mark.parametrize('kind', ['sgdm', 'adamax', 'ftrl'])
def test_dense_and_multi_entry_points_check_their_arguments_before_any_launch(kind):
    """Nothing here may reach a launch (the pointers are made up): every refusal must come from the argument checks, and
    the message must name the entry point."""
    from deeptables_amd import _lib
    lib = _lib.lib()
    hp, ns = HP[kind], NSLOTS[kind]
    name = f'dt_{kind}_dense_step'
    f = getattr(lib, name)
    ptrs = [P, P2, P3, 0x40000][:2 + ns]
    nul = [None] * (2 + ns)
    assert f(*nul, 0, *hp, None, 0, None) == 0                          # n = 0: nothing to do, null pointers are fine
    _refused(lib, name, *nul, -1, *hp, None, 0, None)
    _refused(lib, name, *ptrs, 8, *hp, None, 1, None)                   # advance without the device state
    _refused(lib, name, *nul, 0, *hp, None, 1, None)
    for k in range(2 + ns):
        _refused(lib, name, *[None if i == k else x for i, x in enumerate(ptrs)], 8, *hp, P, 0, None)
        _refused(lib, name, *[ODD if i == k else x for i, x in enumerate(ptrs)], 8, *hp, P, 0, None)
    if kind == 'adamax':
        _refused(lib, name, *ptrs, 8, *hp, None, 0, None)               # beta_1^t needs the step number on the device
    if kind == 'ftrl':
        for bad in ((0.0, -0.5, 0, 0, 0), (1e-3, 0.5, 0, 0, 0), (1e-3, -0.5, -1, 0, 0), (1e-3, -0.5, 0, -1, 0),
                    (1e-3, -0.5, 0, 0, -1)):
            _refused(lib, name, *ptrs, 8, *bad, P, 0, None)
    # multi: (count, p[], g[], slot[] .., n[], hyperparameters, state, advance, stream): host arrays
    name = f'dt_{kind}_multi_step'
    f = getattr(lib, name)
    c = lambda a: ctypes.cast(a, ctypes.c_void_p)
    arr = c((ctypes.c_void_p * 2)(P, P))
    bad = c((ctypes.c_void_p * 2)(P, ODD))
    nulp = c((ctypes.c_void_p * 2)(P, None))
    n_ok, neg = c((ctypes.c_int64 * 2)(4, 4)), c((ctypes.c_int64 * 2)(4, -4))
    big, zero = c((ctypes.c_int64 * 2)(4, 1 << 31)), c((ctypes.c_int64 * 2)(0, 0))
    cols = [arr] * (2 + ns)
    assert f(0, *nul, None, *hp, None, 0, None) == 0
    assert f(2, *[nulp] * (2 + ns), zero, *hp, None, 0, None) == 0      # empty tensors: nothing launched
    _refused(lib, name, -1, *nul, None, *hp, None, 0, None)
    _refused(lib, name, 2, *cols, None, *hp, P, 0, None)
    _refused(lib, name, 2, *cols, neg, *hp, P, 0, None)
    _refused(lib, name, 2, *cols, big, *hp, P, 0, None)
    _refused(lib, name, 2, *cols, n_ok, *hp, None, 1, None)
    for k in range(2 + ns):
        _refused(lib, name, 2, *[None if i == k else x for i, x in enumerate(cols)], n_ok, *hp, P, 0, None)
        _refused(lib, name, 2, *[nulp if i == k else x for i, x in enumerate(cols)], n_ok, *hp, P, 0, None)
        _refused(lib, name, 2, *[bad if i == k else x for i, x in enumerate(cols)], n_ok, *hp, P, 0, None)   # the SECOND tensor
    if kind == 'adamax':
        _refused(lib, name, 2, *cols, n_ok, *hp, None, 0, None)


def _rows_args(kind, n=10, D=16, fields=0, table=P, s0=P2, s1=P3, rows=P, values=P, slots=P, n_slots=1024, mark=P, state=P,
               dense_n=0, advance=0, slot_stride=16, hp=None):
    two = NSLOTS[kind] == 2
    head = [table, s0] + ([s1] if two else []) + [rows, values, n, D, fields, slots, n_slots, mark]
    tail = [state, None, None, None] + ([None] if two else []) + [dense_n, advance, slot_stride, None]
    return head + list(hp or HP[kind]) + tail


@pytest.mark.parametrize('kind', ['sgdm', 'adamax', 'ftrl'])
def test_rows_entry_points_check_their_arguments_before_any_launch(kind):
    from deeptables_amd import _lib
    lib = _lib.lib()
    name = f'dt_{kind}_rows_step'
    f = getattr(lib, name)
    mk = functools.partial(_rows_args, kind)
    assert f(*mk(n=0, table=None, s0=None, s1=None, rows=None, values=None, mark=None, slots=None, state=None)) == 0
    _refused(lib, name, *mk(n=-1))
    _refused(lib, name, *mk(D=0))
    _refused(lib, name, *mk(D=-4))
    _refused(lib, name, *mk(fields=-2))                                 # rows applied inside a fused step: Adam only
    _refused(lib, name, *mk(dense_n=-1))
    _refused(lib, name, *mk(dense_n=5))                                 # a dense tail without its arrays
    _refused(lib, name, *mk(slot_stride=8))                             # < D
    _refused(lib, name, *mk(slot_stride=18))                            # D % 4 == 0 needs a 16-byte stride
    keys = ['table', 's0', 'rows', 'values'] + (['s1'] if NSLOTS[kind] == 2 else [])
    for k in keys:
        _refused(lib, name, *mk(**{k: None}))
    for k in [k for k in keys if k != 'rows']:
        _refused(lib, name, *mk(**{k: Q}))                              # D = 16 reads 16-byte pieces
        _refused(lib, name, *mk(D=6, slot_stride=6, **{k: ODD}))
    if NSLOTS[kind] == 2:
        _refused(lib, name, *mk(s1=P2))                                 # the two slots of a row overlap
        _refused(lib, name, *mk(s1=P2 + 32, slot_stride=32))            # ... s1 closer than D floats behind s0
    _refused(lib, name, *mk(rows=Q))
    _refused(lib, name, *mk(mark=None))
    _refused(lib, name, *mk(slots=None))                                # fields = 0 merges through the global hash
    _refused(lib, name, *mk(n_slots=100))
    _refused(lib, name, *mk(n_slots=16))                                # < 2 n
    _refused(lib, name, *mk(advance=1, state=None))
    _refused(lib, name, *mk(n=1 << 31))
    if kind == 'adamax':
        _refused(lib, name, *mk(state=None))
    if kind == 'ftrl':
        _refused(lib, name, *mk(hp=(1e-3, 0.1, 0.0, 0.0, 0.0)))
        _refused(lib, name, *mk(hp=(1e-3, -0.5, -0.1, 0.0, 0.0)))


def test_a_model_compiled_with_the_new_optimizers_builds_on_the_cpu():
    from deeptables_amd import training as T
    from deeptables_amd.models import ModelConfig, DeepModel
    from deeptables_amd.models.metainfo import CategoricalColumn, ContinuousColumn
    sgd = {'class_name': 'SGD', 'config': {'momentum': 0.9, 'nesterov': True}}
    for spec, cls in (('ftrl', T.Ftrl), ('Adamax', T.Adamax), (sgd, T.MomentumSGD),
                      ({'class_name': 'Ftrl', 'config': {'l1_regularization_strength': 1e-4}}, T.Ftrl)):
        conf = ModelConfig(nets=['linear', 'fm_nets', 'dnn_nets'], fixed_embedding_dim=True, embeddings_output_dim=8,
                           optimizer=spec)
        dm = DeepModel('binary', 2, conf, [CategoricalColumn(f'C{i}', 20 + i, 8) for i in range(4)],
                       [ContinuousColumn('input_continuous_all', ['a', 'b'])])
        dm.build('cpu')
        assert type(dm.optimizer) is cls
        assert dm.model_desc.optimizer_info() == cls._name
        tables = [t for layer in dm.optimizer.embedding_layers for t in layer.tables.values()]
        assert tables and all(any(p is t for p in dm.optimizer.params) for t in tables)
