# -*- coding:utf-8 -*-
"""Gradient clipping without a GPU: what the seven optimizer classes and `make_optimizer` accept for `clipnorm` / `clipvalue` /
`global_clipnorm`, the values they refuse, `hyperparameters()` of an unclipped optimizer as it was, the float64 restatement the
GPU tests compare against (tests/gradclip_reference.py) pinned on hand-computed cases, and the argument checks of the entry
points of csrc/gradclip.hip."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import gradclip_reference as R
from tests import optimizers2_reference as R2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('dt_rows_coalesce_chunk', 'dt_rows_coalesce_workspace_bytes', 'dt_rows_coalesce', 'dt_grad_sumsq_workspace_bytes',
           'dt_grad_sumsq', 'dt_rows_field_sumsq', 'dt_grad_clip', 'dt_rows_clip')
NAMES = ('Adam', 'SGD', 'Adagrad', 'RMSprop', 'Adamax', 'Ftrl')
MOMENTUM = {'class_name': 'SGD', 'config': {'momentum': 0.9}}


def _w():
    return torch.nn.Parameter(torch.zeros(3))


def _specs(extra):
    """Keras' serialised form of all seven classes (SGD with momentum is a class of its own) with `extra` in the config"""
    out = [{'class_name': n, 'config': dict(extra)} for n in NAMES]
    return out + [{'class_name': 'SGD', 'config': dict(MOMENTUM['config'], **extra)}]


@pytest.mark.parametrize('key', R.MODES)
def test_make_optimizer_takes_the_three_clip_arguments_for_every_class(key):
    from deeptables_amd import training as T
    classes = set()
    for spec in _specs({key: 1.0}):
        opt = T.make_optimizer(spec, [_w()], [])
        classes.add(type(opt))
        assert getattr(opt, key) == 1.0 and [getattr(opt, k) for k in R.MODES if k != key] == [None, None]
        assert opt.hyperparameters()[key] == 1.0 and not set(opt.hyperparameters()) & (set(R.MODES) - {key})
        # no update inside a fused step while a clip is set
        assert not opt.supports_row_segments and not opt.supports_rows_in_step
        assert opt.last_global_norm is None
    assert classes == {T.KerasAdam, T.SGD, T.MomentumSGD, T.Adagrad, T.RMSprop, T.Adamax, T.Ftrl}
    # ... and the constructors by name
    for cls in (T.KerasAdam, T.SGD, T.MomentumSGD, T.Adagrad, T.RMSprop, T.Adamax, T.Ftrl):
        assert getattr(cls([_w()], [], **{key: 0.5}), key) == 0.5
        assert key in T._config_keys(cls)


def test_two_clip_arguments_together_raise():
    from deeptables_amd import training as T
    pairs = [{'clipnorm': 1.0, 'clipvalue': 1.0}, {'clipnorm': 1.0, 'global_clipnorm': 1.0},
             {'clipvalue': 1.0, 'global_clipnorm': 1.0}, {k: 1.0 for k in R.MODES}]
    for extra in pairs:
        for spec in _specs(extra):
            with pytest.raises(ValueError, match='Only one of'):
                T.make_optimizer(spec, [_w()], [])
    T.make_optimizer({'class_name': 'Adam', 'config': {'clipnorm': 1.0, 'clipvalue': None}}, [_w()], [])      # None is off


@pytest.mark.parametrize('key', R.MODES)
@pytest.mark.parametrize('bad', [0, 0.0, -1.0, float('nan'), float('inf'), -float('inf')])
def test_a_clip_value_that_is_no_finite_positive_number_raises_naming_the_key(key, bad):
    from deeptables_amd import training as T
    for spec in _specs({key: bad}):
        with pytest.raises(ValueError, match=key):
            T.make_optimizer(spec, [_w()], [])
    opt = T.Adamax([_w()], [])
    with pytest.raises(ValueError, match=key):
        opt.set_hyperparameters({key: bad})
    assert opt.hyperparameters() == R2.ADAMAX_DEFAULTS


def test_hyperparameters_of_an_unclipped_optimizer_are_the_dict_they_were():
    from deeptables_amd import training as T
    w = _w()
    assert T.Ftrl([w], []).hyperparameters() == R2.FTRL_DEFAULTS
    assert T.Adamax([w], []).hyperparameters() == R2.ADAMAX_DEFAULTS
    assert T.SGD([w], []).hyperparameters() == {'learning_rate': 0.01, 'momentum': 0.0, 'nesterov': False}
    assert T.SGD([w], [], momentum=0.9).hyperparameters() == {'learning_rate': 0.01, 'momentum': 0.9, 'nesterov': False}
    assert T.Adagrad([w], []).hyperparameters() == {'learning_rate': 1e-3, 'epsilon': 1e-7, 'initial_accumulator_value': 0.1}
    assert T.RMSprop([w], []).hyperparameters() == {'learning_rate': 1e-3, 'epsilon': 1e-7, 'rho': 0.9, 'momentum': 0.0,
                                                    'centered': False}
    assert T.KerasAdam([w], []).hyperparameters() == {}
    for opt in (T.KerasAdam([w], []), T.SGD([w], [], momentum=0.9), T.Ftrl([w], [])):
        assert opt._clip is None and [getattr(opt, k) for k in R.MODES] == [None] * 3
    # the fused plans' switches are what they were
    assert T.KerasAdam([w], []).supports_row_segments and T.KerasAdam([w], []).supports_rows_in_step
    assert not T.Adagrad([w], []).supports_row_segments and not T.Ftrl([w], []).supports_rows_in_step


def test_set_hyperparameters_carries_the_clip_setting():
    """what a checkpoint round trip does: hyperparameters() of one optimizer into set_hyperparameters() of another"""
    from deeptables_amd import training as T
    w = _w()
    for cls, kw in ((T.KerasAdam, {}), (T.Adagrad, {}), (T.RMSprop, {}), (T.Adamax, {}), (T.Ftrl, {}), (T.SGD, {'momentum': 0.5}),
                    (T.SGD, {})):
        src, dst = cls([w], [], global_clipnorm=0.25, **kw), cls([w], [], **kw)
        dst.set_hyperparameters(src.hyperparameters())
        assert dst.global_clipnorm == 0.25 and dst.hyperparameters() == src.hyperparameters()
        assert not dst.supports_row_segments
        other = cls([w], [], clipvalue=2.0, **kw)
        other.set_hyperparameters(src.hyperparameters())          # the setting is replaced as a whole
        assert other.clipvalue is None and other.global_clipnorm == 0.25
        other.set_hyperparameters(cls([w], [], **kw).hyperparameters())       # an unclipped file leaves it alone
        assert other.global_clipnorm == 0.25
        other.set_hyperparameters({'global_clipnorm': None})
        assert other._clip is None


def test_reference_reproduces_hand_computed_cases():
    # 1. clipvalue 1: each element on its own; NaN stays NaN
    out = R.clip_variables('clipvalue', 1.0, [np.array([-3.0, 0.5, 2.0, np.nan, 0.0, -1.0])])[0]
    assert out[:3].tolist() == [-1.0, 0.5, 1.0] and np.isnan(out[3]) and out[4:].tolist() == [0.0, -1.0]
    # 2. clipnorm, per variable: (3, 4) has norm 5 -> (0.6, 0.8) at c = 1 and itself at c = 10; (0, 0) stays; each variable
    #    by its OWN norm: (0.3, 0.4) has norm 0.5 < 1
    a, b, z = R.clip_variables('clipnorm', 1.0, [np.array([3.0, 4.0]), np.array([0.3, 0.4]), np.zeros(2)])
    assert np.allclose(a, [0.6, 0.8], rtol=0, atol=1e-16) and b.tolist() == [0.3, 0.4] and z.tolist() == [0.0, 0.0]
    assert R.clip_variables('clipnorm', 10.0, [np.array([3.0, 4.0])])[0].tolist() == [3.0, 4.0]
    # 3. global_clipnorm: (3) and (4) in two variables have the global norm 5 -> 0.6, 0.8 at c = 1; unchanged at c = 10
    #    (s = 10 * min(1/5, 1/10) = 1); all zeros stay; a non-finite norm makes everything NaN
    a, b = R.clip_variables('global_clipnorm', 1.0, [np.array([3.0]), np.array([4.0])])
    assert abs(a[0] - 0.6) <= 2.0 ** -52 and abs(b[0] - 0.8) <= 2.0 ** -52         # (3 * fl(0.2): one float64 ulp)
    N, s = R.global_scale([9.0, 16.0], 10.0)
    assert N == 5.0 and s == 1.0
    assert R.clip_variables('global_clipnorm', 1.0, [np.zeros(3)])[0].tolist() == [0.0, 0.0, 0.0]
    a, b = R.clip_variables('global_clipnorm', 1.0, [np.array([np.inf, 1.0]), np.array([2.0])])
    assert np.isnan(a).all() and np.isnan(b).all()
    # the sparse gradient: duplicates summed BEFORE the clamp (0.75 + 0.75 = 1.5 -> 1, not 0.75 + 0.75), -1 skipped
    rows, vals = [2, -1, 2, 0], [[0.75, 0.0], [9.0, 9.0], [0.75, 1.0], [-2.0, 0.0]]
    out_rows, out_vals = R.coalesce(rows, vals)
    assert out_rows.tolist() == [0, 2, -1, -1] and out_vals.tolist() == [[-2.0, 0.0], [1.5, 1.0], [0.0, 0.0], [0.0, 0.0]]
    assert R.clip_value(out_vals, 1.0).tolist() == [[-1.0, 0.0], [1.0, 1.0], [0.0, 0.0], [0.0, 0.0]]
    # ... and the fields of a packed table are variables of their own: rows [0, 2) | [2, 3) | [3, 5) (nothing looked up)
    assert R.field_sumsq(out_rows, out_vals, [0, 2, 3], 5) == [4.0, 3.25, 0.0]
    assert R.field_of([0, 1, 2, 4], [0, 2, 3]).tolist() == [0, 0, 1, 2]
    assert R.c32(0.05) == float(np.float32(0.05)) != 0.05


def test_header_exports_and_binding_name_the_same_entry_points():
    from deeptables_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'dt_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(dt_(?:rows_coalesce|grad_sumsq|rows_field_sumsq|grad_clip|rows_clip)[a-z0-9_]*)\s*\(', text))
    assert declared == set(ENTRIES) and all(n in _lib.SIGNATURES for n in ENTRIES)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(handle, n) for n in ENTRIES)
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert all(f'`{n}`' in doc for n in ENTRIES)
    assert (_lib.DT_CLIP_VALUE, _lib.DT_CLIP_NORM, _lib.DT_CLIP_GLOBAL_NORM) == (0, 1, 2)
    assert re.search(rf'#define DT_FIELD_SUMSQ_PARTS {_lib.DT_FIELD_SUMSQ_PARTS}\b', text)
    for name, value in (('DT_CLIP_VALUE', 0), ('DT_CLIP_NORM', 1), ('DT_CLIP_GLOBAL_NORM', 2)):
        assert re.search(rf'#define {name} {value}\b', text)


P, P2, P3, P4 = 0x10000, 0x20000, 0x30000, 0x40000      # 16-byte aligned, far apart; never dereferenced
ODD4, ODD8 = 0x10002, 0x10004                           # not float aligned / float aligned but not 8-byte aligned
TOP = (1 << 32) - 1                                     # the sort key that marks a skipped lookup


def _refused(lib, name, *args):
    assert getattr(lib, name)(*args) != 0, (name, args)
    err = lib.dt_last_error()
    assert name.encode() in err and b'launch failed' not in err, err


def test_workspace_queries_need_no_gpu():
    from deeptables_amd import _lib
    h = _lib.lib()
    T = h.dt_metric_sort_tile()
    assert h.dt_rows_coalesce_chunk() == 512
    sizes = [0, 1, 63, T - 1, T, T + 1, 3 * T + 7]
    got = [h.dt_rows_coalesce_workspace_bytes(n, 16) for n in sizes]
    assert all(b > 0 and b % 256 == 0 for b in got) and got == sorted(got)
    assert all(h.dt_rows_coalesce_workspace_bytes(n, 16) > h.dt_metric_sort_workspace_bytes(n) for n in sizes[1:])
    assert h.dt_rows_coalesce_workspace_bytes(T, 301) > h.dt_rows_coalesce_workspace_bytes(T, 16)
    for n, D in ((-1, 16), (1 << 31, 16), (8, 0), (8, -4)):
        assert h.dt_rows_coalesce_workspace_bytes(n, D) == -1 and b'dt_rows_coalesce_workspace_bytes' in h.dt_last_error()
    n = (ctypes.c_int64 * 3)(1, h.dt_reg_chunk(), 2 * h.dt_reg_chunk() + 1)
    assert h.dt_grad_sumsq_workspace_bytes(3, n) == 8 * (1 + 1 + 3)
    assert h.dt_grad_sumsq_workspace_bytes(0, None) >= 8
    assert h.dt_grad_sumsq_workspace_bytes(-1, n) == -1 and h.dt_grad_sumsq_workspace_bytes(1, None) == -1
    assert h.dt_grad_sumsq_workspace_bytes(1, (ctypes.c_int64 * 1)(-4)) == -1


def test_coalesce_checks_its_arguments_before_any_launch():
    """Nothing here may reach a launch (the pointers are made up): every refusal comes from the argument checks"""
    from deeptables_amd import _lib
    h = _lib.lib()
    name = 'dt_rows_coalesce'

    def args(rows=P, values=P2, n=10, D=16, V=50, out_rows=P3, out_vals=P4, count=P, ws=P2):
        return rows, values, n, D, V, out_rows, out_vals, count, ws, None
    for k in ('rows', 'values', 'out_rows', 'out_vals', 'count'):
        _refused(h, name, *args(**{k: None}))
    _refused(h, name, *args(ws=None))                                   # a null workspace
    _refused(h, name, *args(ws=P2 + 8))                                 # ... a misaligned one
    _refused(h, name, *args(n=-1))
    _refused(h, name, *args(n=1 << 31))
    _refused(h, name, *args(D=0))
    _refused(h, name, *args(D=-4))
    _refused(h, name, *args(V=0))
    _refused(h, name, *args(V=TOP + 1))                                 # a row id >= 2^32 - 1 would be possible
    _refused(h, name, *args(V=1 << 40))
    _refused(h, name, *args(rows=ODD8))
    _refused(h, name, *args(out_rows=ODD8))
    _refused(h, name, *args(count=ODD8))
    _refused(h, name, *args(values=ODD4))
    _refused(h, name, *args(out_vals=ODD4))
    _refused(h, name, *args(n=0, count=None))                           # n = 0 still writes the count


def test_sums_check_their_arguments_before_any_launch():
    from deeptables_amd import _lib
    h = _lib.lib()
    c = lambda a: ctypes.cast(a, ctypes.c_void_p)
    two, nulp, odd = c((ctypes.c_void_p * 2)(P, P2)), c((ctypes.c_void_p * 2)(P, None)), c((ctypes.c_void_p * 2)(P, ODD4))
    n_ok, neg, big = c((ctypes.c_int64 * 2)(4, 4)), c((ctypes.c_int64 * 2)(4, -4)), c((ctypes.c_int64 * 2)(4, 1 << 40))
    name = 'dt_grad_sumsq'
    assert h.dt_grad_sumsq(0, None, None, None, None, None) == 0         # no tensors: nothing to do
    _refused(h, name, -1, two, n_ok, P3, P4, None)
    _refused(h, name, 2, None, n_ok, P3, P4, None)
    _refused(h, name, 2, two, None, P3, P4, None)
    _refused(h, name, 2, two, n_ok, None, P4, None)                     # nowhere to put the sums
    _refused(h, name, 2, two, n_ok, ODD8, P4, None)
    _refused(h, name, 2, nulp, n_ok, P3, P4, None)                      # the SECOND tensor
    _refused(h, name, 2, odd, n_ok, P3, P4, None)
    _refused(h, name, 2, two, neg, P3, P4, None)
    _refused(h, name, 2, two, big, P3, P4, None)
    _refused(h, name, 2, two, n_ok, P3, None, None)                     # a null workspace
    _refused(h, name, 2, two, n_ok, P3, P4 + 4, None)                   # ... a misaligned one
    name = 'dt_rows_field_sumsq'

    def args(out_rows=P, out_vals=P2, n=10, D=16, count=P3, row_offset=P4, F=3, V=50, sums=P, ws=P2):
        return out_rows, out_vals, n, D, count, row_offset, F, V, sums, ws, None
    for k in ('out_rows', 'out_vals', 'count', 'row_offset', 'sums', 'ws'):
        _refused(h, name, *args(**{k: None}))
    for k in ('out_rows', 'count', 'row_offset', 'sums', 'ws'):
        _refused(h, name, *args(**{k: ODD8}))
    _refused(h, name, *args(out_vals=ODD4))
    for bad in (dict(n=-1), dict(n=1 << 31), dict(D=0), dict(F=0), dict(F=-1), dict(V=0), dict(V=TOP + 1)):
        _refused(h, name, *args(**bad))


def test_clips_check_their_arguments_before_any_launch():
    from deeptables_amd import _lib
    h = _lib.lib()
    c = lambda a: ctypes.cast(a, ctypes.c_void_p)
    two, nulp, odd = c((ctypes.c_void_p * 2)(P, P2)), c((ctypes.c_void_p * 2)(P, None)), c((ctypes.c_void_p * 2)(P, ODD4))
    n_ok, neg = c((ctypes.c_int64 * 2)(4, 4)), c((ctypes.c_int64 * 2)(4, -4))
    idx, idx_bad, idx_neg = c((ctypes.c_int * 2)(0, 1)), c((ctypes.c_int * 2)(0, 2)), c((ctypes.c_int * 2)(-1, 0))
    V_, N_, G_ = _lib.DT_CLIP_VALUE, _lib.DT_CLIP_NORM, _lib.DT_CLIP_GLOBAL_NORM
    name = 'dt_grad_clip'
    for mode in (-1, 3):
        _refused(h, name, mode, 1.0, 2, two, n_ok, idx, P3, 2, None, None)
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        for mode in (V_, N_, G_):
            _refused(h, name, mode, bad, 2, two, n_ok, idx, P3, 2, None, None)
    for mode in (V_, N_, G_):
        _refused(h, name, mode, 1.0, -1, two, n_ok, idx, P3, 2, None, None)
        _refused(h, name, mode, 1.0, 2, None, n_ok, idx, P3, 2, None, None)
        _refused(h, name, mode, 1.0, 2, two, None, idx, P3, 2, None, None)
        _refused(h, name, mode, 1.0, 2, nulp, n_ok, idx, P3, 2, None, None)
        _refused(h, name, mode, 1.0, 2, odd, n_ok, idx, P3, 2, None, None)
        _refused(h, name, mode, 1.0, 2, two, neg, idx, P3, 2, None, None)
        _refused(h, name, mode, 1.0, 2, two, n_ok, idx, P3, 2, ODD8, None)      # a misaligned norm_out
        _refused(h, name, mode, 1.0, 2, two, n_ok, idx, P3, -1, None, None)
    for mode in (N_, G_):
        _refused(h, name, mode, 1.0, 2, two, n_ok, idx, None, 2, None, None)    # the sums a norm needs
        _refused(h, name, mode, 1.0, 2, two, n_ok, idx, ODD8, 2, None, None)
    _refused(h, name, N_, 1.0, 2, two, n_ok, None, P3, 2, None, None)
    _refused(h, name, N_, 1.0, 2, two, n_ok, idx_bad, P3, 2, None, None)        # a variable past the end of sums
    _refused(h, name, N_, 1.0, 2, two, n_ok, idx_neg, P3, 2, None, None)
    name = 'dt_rows_clip'

    def args(mode=N_, c=1.0, out_rows=P, out_vals=P2, n=10, D=16, count=P3, row_offset=P4, F=3, V=50, sums=P, sum_base=2,
             n_sums=5, norm_out=None):
        return mode, c, out_rows, out_vals, n, D, count, row_offset, F, V, sums, sum_base, n_sums, norm_out, None
    for mode in (-1, 3):
        _refused(h, name, *args(mode=mode))
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        _refused(h, name, *args(c=bad))
    for mode in (V_, N_, G_):
        for k in ('out_rows', 'out_vals', 'count'):
            _refused(h, name, *args(mode=mode, **{k: None}))
        for k in ('out_rows', 'count', 'norm_out'):
            _refused(h, name, *args(mode=mode, **{k: ODD8}))
        _refused(h, name, *args(mode=mode, out_vals=ODD4))
        for bad in (dict(n=-1), dict(n=1 << 31), dict(D=0), dict(F=0), dict(V=0), dict(V=TOP + 1), dict(sum_base=-1),
                    dict(n_sums=-1)):
            _refused(h, name, *args(mode=mode, **bad))
    for mode in (N_, G_):
        _refused(h, name, *args(mode=mode, sums=None))
        _refused(h, name, *args(mode=mode, sums=ODD8))
    _refused(h, name, *args(row_offset=None))
    _refused(h, name, *args(row_offset=ODD8))
    _refused(h, name, *args(sum_base=3))                                # 3 + F fields > n_sums


def test_clipping_with_a_distribute_strategy_raises():
    from deeptables_amd.models import ModelConfig, DeepModel
    from deeptables_amd.models.metainfo import CategoricalColumn, ContinuousColumn

    class Strategy:                       # what fit asks of a strategy before it looks at anything else
        device = 'cpu'

        def exchange_gradients(self, model, optimizer):
            raise AssertionError('the clip check comes first')

    for key in R.MODES:
        conf = ModelConfig(nets=['linear', 'dnn_nets'], fixed_embedding_dim=True, embeddings_output_dim=8,
                           optimizer={'class_name': 'Adam', 'config': {key: 1.0}}, distribute_strategy=Strategy())
        dm = DeepModel('binary', 2, conf, [CategoricalColumn(f'C{i}', 20 + i, 8) for i in range(4)],
                       [ContinuousColumn('input_continuous_all', ['a', 'b'])])
        dm.build('cpu')
        assert dm.optimizer.hyperparameters() == {key: 1.0} and dm.fused_plan() is None
        with pytest.raises(ValueError, match=key):
            dm.train_step([torch.zeros(2, 4, dtype=torch.int32), torch.zeros(2, 2)], torch.zeros(2, 1))
        with pytest.raises(ValueError, match='distribute_strategy'):
            dm.fit(np.zeros((4, 6)), np.zeros(4), verbose=0)
