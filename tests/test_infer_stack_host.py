# -*- coding:utf-8 -*-
"""CPU: the inference plan for every Add-stacked subset of {'linear', 'fm_nets', 'dnn_nets'} (fused.InferStack,
dt_stack_infer*, csrc/infer_x3.h) — which graphs it takes, what the library's predicate accepts, that the entry points
check their pointers against the net mask before any launch, and which calls `predict` / `evaluate` make with which
tensors.  The plans are built on CPU models and their launches recorded by a stand-in for the library (the recorder of
tests/test_infer_host.py, for the dt_stack_* names): nothing runs on a GPU."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from tests.infer_support import install_recorder
from tests.test_infer_host import CORNERS, PAST, H1, H2, F_, D_, ND_, DEEPFM, DCN, _frame, _model, _names, _decode

LIN, FM, DNN = 1, 2, 4
BITS = {'linear': LIN, 'fm_nets': FM, 'dnn_nets': DNN}
SUBSETS = [list(c) for k in (1, 2) for c in itertools.combinations(BITS, k)]          # the six the new plan takes
ORDERS = [list(p) for s in SUBSETS for p in itertools.permutations(s)]                  # ... in every order: 9
STACK_ENTRIES = ('dt_stack_infer_prepare', 'dt_stack_infer')
OTHER_ENTRIES = ('dt_deepfm_infer_prepare', 'dt_deepfm_infer', 'dt_dcn_infer_prepare', 'dt_dcn_infer')


def _mask(nets):
    return sum(BITS[n] for n in nets)


def test_the_net_bits_are_the_headers():
    from deeptables_amd import _lib
    assert (_lib.DT_NET_LINEAR, _lib.DT_NET_FM, _lib.DT_NET_DNN) == (LIN, FM, DNN)


def test_predicate_accepts_every_corner_and_refuses_the_first_shape_past_each_limit():
    from deeptables_amd import _lib
    lib = _lib.lib()
    for nets in range(1, 8):
        for F, D, Nd in CORNERS:
            for h1, h2 in ((H1, H2), (1, 1), (100, 40)):
                for cells in range(4):
                    assert lib.dt_stack_infer_supported(F, D, Nd, h1, h2, cells, nets) == 1, (F, D, Nd, h1, h2, cells, nets)
            assert lib.dt_stack_infer_workspace_bytes(F, D, Nd, nets) > 0
        for what, (F, D, Nd) in PAST.items():
            assert lib.dt_stack_infer_supported(F, D, Nd, H1, H2, 0, nets) == 0, (what, nets)
            assert lib.dt_stack_infer_workspace_bytes(F, D, Nd, nets) == -1, (what, nets)
        for h1, h2, cells in ((129, 64, 0), (128, 65, 0), (0, 64, 0), (128, 0, 0), (128, 64, 4), (128, 64, -1)):
            # the tower's limits bind exactly when the mask has a tower
            assert lib.dt_stack_infer_supported(26, 16, 13, h1, h2, cells, nets) == (0 if nets & DNN else 1), (h1, h2, cells, nets)
    for nets in (0, 8, -1, 15):
        assert lib.dt_stack_infer_supported(26, 16, 13, H1, H2, 0, nets) == 0
        assert lib.dt_stack_infer_workspace_bytes(26, 16, 13, nets) == -1


def test_workspace_holds_only_what_the_nets_read():
    """head (4 floats) + the linear kernel's CP slab with `linear`; the tower's layouts only with `dnn_nets`; the full mask
    is dt_deepfm_infer's layout"""
    from deeptables_amd import _lib
    lib = _lib.lib()
    F, D, Nd = 26, 16, 13
    CP = (F * D + Nd + 63) // 64 * 64
    wb = {n: lib.dt_stack_infer_workspace_bytes(F, D, Nd, n) for n in range(1, 8)}
    assert wb[FM] == 16 and wb[LIN] == wb[LIN | FM] == 16 + 4 * CP
    assert wb[DNN] == wb[DNN | FM] and wb[DNN | LIN] == wb[7] == wb[DNN] + 4 * CP
    assert wb[7] == lib.dt_deepfm_infer_workspace_bytes(F, D, Nd)
    tower = 4 * (3 * CP * 128 // 2 + 3 * 128 * 64 // 2 + 3 * CP + 3 * 128 + 3 * 64 + 64)
    assert wb[DNN] == tower + 16


def _prepare_args(nets, **over):
    """dt_stack_infer_prepare's arguments with every pointer set to one small host buffer (never read: the checks under
    test return before the launch), then `over` applied by name"""
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    names = ['F', 'D', 'Nd', 'nets', 'w_lin', 'bn_gamma', 'bn_beta', 'bn_mean', 'bn_var', 'bn_eps', 'W1', 'ld1', 'H1', 'b1',
             'W2', 'ld2', 'H2', 'b2', 'cells', 'c1_gamma', 'c1_beta', 'c1_mean', 'c1_var', 'c1_eps', 'c2_gamma', 'c2_beta',
             'c2_mean', 'c2_var', 'c2_eps', 'w3', 'w_out', 'b_out', 'workspace', 'stream']
    ints = {'F': 2, 'D': 4, 'Nd': 1, 'nets': nets, 'ld1': 128, 'H1': 128, 'ld2': 64, 'H2': 64, 'cells': 0}
    vals = {n: ints.get(n, 0.001 if n.endswith('eps') else p) for n in names}
    vals['stream'] = None
    vals.update(over)
    return [vals[n] for n in names], buf


@pytest.mark.parametrize('nets', range(1, 8))
def test_prepare_rejects_null_pointers_the_mask_needs_before_any_launch(nets):
    """w_lin may be null when and only when the mask has no linear, the tower's pointers when and only when it has no
    dnn_nets, w_out only for dnn_nets alone; the refusals come back as DT_REQUIRE errors (-1) naming the entry point.
    The accepted calls are not made here: they would launch."""
    from deeptables_amd import _lib
    lib = _lib.lib()
    needed = {'workspace'}
    if nets & LIN:
        needed.add('w_lin')
    if nets & DNN:
        needed |= {'bn_mean', 'bn_var', 'W1', 'W2', 'w3'}
    if nets != DNN:
        needed.add('w_out')
    for name in sorted(needed):
        args, keep = _prepare_args(nets, **{name: None})
        assert lib.dt_stack_infer_prepare(*args) != 0, (nets, name)
        assert b'dt_stack_infer_prepare' in lib.dt_last_error(), (nets, name)
    if nets & DNN:
        for over in (dict(H1=129), dict(H2=65), dict(cells=4), dict(ld1=100), dict(cells=1, c1_mean=None), dict(cells=2, c2_var=None)):
            args, keep = _prepare_args(nets, **over)
            assert lib.dt_stack_infer_prepare(*args) != 0, (nets, over)
    args, keep = _prepare_args(nets, D=12)
    assert lib.dt_stack_infer_prepare(*args) != 0
    # a workspace that is not 16-byte aligned is the last check before the launch: everything above it passed
    def misaligned(buf):
        a = ctypes.addressof(buf)
        return ctypes.c_void_p(a + (4 - a) % 16)         # = 4 mod 16, inside the 256-byte buffer

    args, keep = _prepare_args(nets)
    args[-2] = misaligned(keep)
    kept_null = {'w_lin': None} if not nets & LIN else {}
    if not nets & DNN:
        kept_null.update(bn_mean=None, bn_var=None, W1=None, W2=None, w3=None, bn_gamma=None, bn_beta=None, H1=0, H2=0)
    if nets == DNN:
        kept_null['w_out'] = None
    args2, keep2 = _prepare_args(nets, **kept_null)
    args2[-2] = misaligned(keep2)
    for a in (args, args2):
        assert lib.dt_stack_infer_prepare(*a) != 0
        assert b'16-byte aligned' in lib.dt_last_error(), lib.dt_last_error()


def test_entry_points_check_their_arguments_before_any_launch():
    from deeptables_amd import _lib
    lib = _lib.lib()
    for nets in range(1, 8):
        assert lib.dt_stack_infer(None, 1, None, None, None, None, 0, 26, 16, 13, nets, None, None, None, None, 0, None) == 0
        assert lib.dt_stack_infer(None, 1, None, None, None, None, 5, 26, 16, 13, nets, None, None, None, None, 0, None) != 0
        assert b'dt_stack_infer' in lib.dt_last_error()
        assert lib.dt_stack_infer(None, 1, None, None, None, None, 0, 26, 16, 13, nets, None, None, None, None, 0x4, None) != 0
        assert lib.dt_stack_infer(None, 7, None, None, None, None, 0, 26, 16, 13, nets, None, None, None, None, 0, None) != 0
        assert lib.dt_stack_infer(None, 1, None, None, None, None, 0, 26, 12, 13, nets, None, None, None, None, 0, None) != 0
    for nets in (0, 8, -1):
        assert lib.dt_stack_infer(None, 1, None, None, None, None, 0, 26, 16, 13, nets, None, None, None, None, 0, None) != 0
        assert b'nets' in lib.dt_last_error()
        args, keep = _prepare_args(nets)
        assert lib.dt_stack_infer_prepare(*args) != 0
        assert b'nets' in lib.dt_last_error()


# ---- routing ------------------------------------------------------------------------------------------------------------
@pytest.fixture
def rec(monkeypatch):
    return install_recorder(monkeypatch, STACK_ENTRIES + OTHER_ENTRIES,
                            ('DT_AMD_FUSED', 'DT_AMD_FUSED_PREDICT', 'DT_AMD_TOWER_DTYPE'))


def _expected_prepare(dm, nets, ld1=100, ld2=40):
    """the decoded dt_stack_infer_prepare arguments: the layers' current parameters by name, NULL / 0 for what the nets lack"""
    L = dm.model.layers_by_name
    mask = _mask(nets)

    def nm(layer, attr):
        return f'{layer.name}.{attr}' if getattr(layer, attr, None) is not None else None

    head = [F_, D_, ND_, mask, 'linear_logit.kernel' if mask & LIN else None]
    if mask & DNN:
        bn, d1, d2 = L['bn_concat_emb_dense'], L['dnn_dense_1'], L['dnn_dense_2']
        mid = [nm(bn, 'gamma'), nm(bn, 'beta'), nm(bn, 'moving_mean'), nm(bn, 'moving_variance'), float(bn.epsilon),
               nm(d1, 'kernel'), ld1, d1.kernel.shape[1], nm(d1, 'bias'), nm(d2, 'kernel'), ld2, d2.kernel.shape[1], nm(d2, 'bias')]
        bits, cellargs = 0, []
        for i in (1, 2):
            b = L.get(f'dnn_bn_{i}')
            if b is None:
                cellargs += [None, None, None, None, 0.0]
            else:
                bits |= 1 << (i - 1)
                cellargs += [nm(b, 'gamma'), nm(b, 'beta'), nm(b, 'moving_mean'), nm(b, 'moving_variance'), float(b.epsilon)]
    else:
        mid, bits, cellargs = [None, None, None, None, 0.0, None, 0, 0, None, None, 0, 0, None], 0, [None, None, None, None, 0.0] * 2
    if mask == DNN:
        w3, wout = 'task_output.kernel', None                  # the tower alone: task_output's [H2, 1] kernel is its vector
    else:
        w3, wout = ('dense_logit_dnn_nets.kernel' if mask & DNN else None), 'task_output.kernel'
    return head + mid + [bits] + cellargs + [w3, wout, nm(L['task_output'], 'bias'), 'ws', None]


def _check_calls(rec, dm, nets, n, b, **ld):
    assert rec.names() == ['dt_stack_infer_prepare'] + ['dt_stack_infer'] * -(-n // b), rec.names()
    names = _names(dm)
    assert _decode(rec.calls[0][1], names) == _expected_prepare(dm, nets, **ld)
    rows = 0
    for _, args in rec.calls[1:]:
        B = args[6]
        assert args[7:11] == (F_, D_, ND_, _mask(nets)) and 0 < B <= b
        assert names.get(args[11].value) == 'ws'
        rows += B
    assert rows == n


@pytest.mark.parametrize('nets', ORDERS, ids='+'.join)
def test_predict_makes_one_prepare_and_one_infer_per_batch(rec, nets):
    from deeptables_amd import _lib, fused
    dm = _model(nets)
    plan = dm.inference_plan()
    assert type(plan) is fused.InferStack and plan.mask == _mask(nets)
    L = dm.model.layers_by_name
    assert ('dense_logit_dnn_nets' in L) == ('dnn_nets' in nets and len(nets) > 1)
    assert tuple(L['task_output'].kernel.shape) == ((40, 1) if nets == ['dnn_nets'] else (1, 1))
    n, b = 100, 32
    out = dm.predict(_frame(n), batch_size=b)
    assert out.shape == (n, 1) and out.dtype == np.float32
    _check_calls(rec, dm, nets, n, b)
    assert not hasattr(dm, '_fused_plan')
    assert rec.calls[1][1][-2] == _lib.DT_INFER_SIGMOID
    # the workspace is the size the library states for this mask
    assert plan.ws.numel() * 4 == _lib.lib().dt_stack_infer_workspace_bytes(F_, D_, ND_, _mask(nets))


@pytest.mark.parametrize('nets', [['dnn_nets'], ['linear', 'dnn_nets'], ['linear', 'fm_nets'], ['fm_nets']], ids='+'.join)
def test_evaluate_routes_through_the_plan(rec, nets, monkeypatch):
    dm = _model(nets)
    n = 50
    y = (np.arange(n) % 3 == 0).astype(np.float32)
    monkeypatch.setattr(torch, 'empty', lambda *a, **k: torch.zeros(*a, **k))     # the recorded launches write nothing
    res = dm.evaluate(_frame(n), y, batch_size=16)
    _check_calls(rec, dm, nets, n, 16)
    assert abs(res['loss'] - float(np.log(2.0))) < 1e-6


def test_the_default_config_takes_the_plan(rec):
    """the bare ModelConfig(): nets ['dnn_nets'], the 128 x 64 tower, one embedding group of width 4, embedding_dropout 0.3"""
    from deeptables_amd import fused
    from deeptables_amd.models import ModelConfig, DeepModel
    from deeptables_amd.models.metainfo import CategoricalColumn, ContinuousColumn
    conf = ModelConfig()
    assert conf.nets == ['dnn_nets']
    dm = DeepModel('binary', 2, conf, [CategoricalColumn(f'C{i}', 20 + i, conf.embeddings_output_dim) for i in range(F_)],
                   [ContinuousColumn('input_continuous_all', ['a', 'b', 'c'])])
    dm.build('cpu')
    assert type(dm.inference_plan()) is fused.InferStack
    dm.predict(_frame(20), batch_size=8)
    assert rec.names() == ['dt_stack_infer_prepare'] + ['dt_stack_infer'] * 3


def test_deepfm_and_dcn_keep_their_plans_and_calls(rec):
    from deeptables_amd import fused
    for net, cls, pre in ((DEEPFM, fused.InferDeepFM, 'deepfm'), (DCN, fused.InferDCN, 'dcn'),
                          (['dnn_nets', 'fm_nets', 'linear'], fused.InferDeepFM, 'deepfm')):
        rec.calls.clear()
        dm = _model(net)
        assert type(dm.inference_plan()) is cls
        assert not fused.InferStack.eligible(dm)
        dm.predict(_frame(20), batch_size=8)
        assert rec.names() == [f'dt_{pre}_infer_prepare'] + [f'dt_{pre}_infer'] * 3


@pytest.mark.parametrize('nets', SUBSETS, ids='+'.join)
@pytest.mark.parametrize('case', ['multiclass', 'concat', 'tanh', 'wide', 'deep', 'sharded', 'env', 'fused_off'])
def test_graphs_and_switches_refused_for_every_subset(rec, monkeypatch, nets, case):
    """multiclass, concat stacking, sharded embeddings and the two switches are refused for every subset; tanh, a 129-wide
    and a three-cell tower wherever a tower is in the graph (a graph without 'dnn_nets' has no tower to refuse)"""
    from deeptables_amd import _lib, fused
    kw = {}
    hidden = ((100, 0, False), (40, 0, False))
    if case == 'multiclass':
        kw['task'] = 'multiclass'
    elif case == 'concat':
        kw['stacking_op'] = 'concat'
    elif case == 'tanh':
        kw['activation'] = 'tanh'
    elif case == 'wide':
        hidden = ((129, 0, False), (40, 0, False))
    elif case == 'deep':
        hidden = ((64, 0, False), (32, 0, False), (16, 0, False))
    dm = _model(nets, hidden, **kw)
    if case == 'env':
        monkeypatch.setenv('DT_AMD_FUSED_PREDICT', '0')
    elif case == 'fused_off':
        monkeypatch.setenv('DT_AMD_FUSED', '0')
    elif case == 'sharded':
        class _Sharded:
            sharded_embeddings, active, world_size = True, True, 1
        dm.config = dm.config._replace(distribute_strategy=_Sharded())
    if case in ('tanh', 'wide', 'deep') and 'dnn_nets' not in nets:
        assert type(fused.make_inference_plan(dm)) is fused.InferStack
        return
    assert fused.make_inference_plan(dm) is None
    with pytest.raises(_lib.DtHipError, match='GPU only'):        # the layer path runs: its first kernel refuses CPU tensors
        dm.predict(_frame(20), batch_size=8)
    assert rec.names() == []


def test_other_refusals(rec):
    """a tower whose last cell has width 1 in a graph of several nets (no dense_logit_dnn_nets; alone, task_output's
    [1, 1] kernel is its vector); a net outside the three; the training plan still refuses ['linear', 'dnn_nets']"""
    from deeptables_amd import fused
    assert fused.make_inference_plan(_model(['linear', 'dnn_nets'], ((100, 0, False), (1, 0, False)))) is None
    assert type(fused.make_inference_plan(_model(['dnn_nets'], ((100, 0, False), (1, 0, False))))) is fused.InferStack
    assert fused.make_inference_plan(_model(['linear', 'cin_nets'])) is None
    dm = _model(['linear', 'dnn_nets'])
    assert dm.fused_plan() is None and type(dm.inference_plan()) is fused.InferStack


@pytest.mark.parametrize('nets', [['dnn_nets'], ['fm_nets', 'dnn_nets']], ids='+'.join)
@pytest.mark.parametrize('hidden', [((100, 0.3, False), (40, 0.1, False)), ((64, 0, True), (32, 0, False)),
                                    ((128, 0.2, True), (64, 0, True))])
def test_dropout_and_batch_norm_cells(rec, nets, hidden):
    dm = _model(nets, hidden)
    dm.predict(_frame(33), batch_size=16)
    _check_calls(rec, dm, nets, 33, 16, ld1=hidden[0][0], ld2=hidden[1][0])
    assert rec.calls[0][1][18] == (1 if hidden[0][2] else 0) | (2 if hidden[1][2] else 0)


@pytest.mark.parametrize('nets', [['dnn_nets'], ['linear', 'fm_nets'], ['linear']], ids='+'.join)
def test_regression_and_output_bias_flags(rec, nets, monkeypatch):
    from deeptables_amd import _lib
    dm = _model(nets, task='regression', output_use_bias=False)
    dm.predict(_frame(10), batch_size=4)
    assert rec.calls[1][1][-2] == 0                     # identity output
    assert rec.calls[0][1][-3] is None                  # no b_out
    rec.calls.clear()
    monkeypatch.setenv('DT_AMD_TOWER_DTYPE', 'bf16')
    dm.predict(_frame(10), batch_size=4)
    assert rec.calls[1][1][-2] == _lib.DT_INFER_TOWER_BF16


def test_building_the_plan_moves_nothing(rec):
    for nets in SUBSETS:
        dm = _model(nets)
        before = {n: p.data_ptr() for n, p in dm.model.named_parameters()}
        assert type(dm.inference_plan()).__name__ == 'InferStack'
        assert not hasattr(dm, '_fused_plan')
        assert {n: p.data_ptr() for n, p in dm.model.named_parameters()} == before
        assert getattr(dm.optimizer, '_flat', None) is None
