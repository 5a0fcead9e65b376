# -*- coding:utf-8 -*-
"""CPU: the fused inference plans (fused.InferDeepFM / InferDCN, csrc/infer_x3.h) — what the library's predicates accept,
and which entry points `predict` / `evaluate` / fit's validation pass call with which tensors.  The plans are built on CPU
models and their launches recorded by a stand-in for the library: nothing runs on a GPU."""
import numpy as np
import pandas as pd
import pytest
import torch

from tests.infer_support import install_recorder

H1, H2 = 128, 64
# (F, D, Nd): the corners of the step's field / width domain (csrc/tile_common.h deepfm_dims)
CORNERS = [(8, 64, 0), (7, 64, 64), (1, 4, 0), (1, 4, 64), (127, 4, 0), (128, 4, 32), (16, 16, 0), (32, 16, 32)]
PAST = {'D = 128': (1, 128, 0), 'D = 12 (3 lanes)': (1, 12, 0), 'D = 0': (1, 0, 0), 'F D / 4 = 129': (129, 4, 0),
        'Nd = 65': (1, 4, 65), 'C = 545': (32, 16, 33), 'F = 0': (0, 4, 4)}


def test_infer_predicates_accept_every_corner_and_refuse_the_first_shape_past_each_limit():
    from deeptables_amd import _lib
    lib = _lib.lib()
    for F, D, Nd in CORNERS:
        for h1, h2 in ((H1, H2), (1, 1), (100, 40)):
            for cells in range(4):
                assert lib.dt_deepfm_infer_supported(F, D, Nd, h1, h2, cells) == 1, (F, D, Nd, h1, h2, cells)
                for L in (1, 8):     # the inference tile holds no backward buffers: every corner fits at L = 8, CP = 576 included
                    assert lib.dt_dcn_infer_supported(F, D, Nd, h1, h2, cells, L) == 1, (F, D, Nd, h1, h2, cells, L)
        assert lib.dt_deepfm_infer_workspace_bytes(F, D, Nd) > 0
        assert lib.dt_dcn_infer_workspace_bytes(F, D, Nd, 8) > lib.dt_dcn_infer_workspace_bytes(F, D, Nd, 1) > 0
        for L in (0, 9):
            assert lib.dt_dcn_infer_supported(F, D, Nd, H1, H2, 0, L) == 0
            assert lib.dt_dcn_infer_workspace_bytes(F, D, Nd, L) == -1
    for what, (F, D, Nd) in PAST.items():
        assert lib.dt_deepfm_infer_supported(F, D, Nd, H1, H2, 0) == 0, what
        assert lib.dt_dcn_infer_supported(F, D, Nd, H1, H2, 0, 2) == 0, what
        assert lib.dt_deepfm_infer_workspace_bytes(F, D, Nd) == -1, what
    for h1, h2, cells in ((129, 64, 0), (128, 65, 0), (0, 64, 0), (128, 0, 0), (128, 64, 4), (128, 64, -1)):
        assert lib.dt_deepfm_infer_supported(26, 16, 13, h1, h2, cells) == 0, (h1, h2, cells)
        assert lib.dt_dcn_infer_supported(26, 16, 13, h1, h2, cells, 2) == 0, (h1, h2, cells)


def test_infer_entry_points_check_their_arguments_before_any_launch():
    from deeptables_amd import _lib
    lib = _lib.lib()
    assert lib.dt_deepfm_infer(None, 1, None, None, None, None, 0, 26, 16, 13, None, None, None, None, 0, None) == 0
    assert lib.dt_deepfm_infer(None, 1, None, None, None, None, 5, 26, 16, 13, None, None, None, None, 0, None) != 0
    assert b'dt_deepfm_infer' in lib.dt_last_error()
    assert lib.dt_deepfm_infer(None, 1, None, None, None, None, 0, 26, 16, 13, None, None, None, None, 0x4, None) != 0
    assert lib.dt_dcn_infer(None, 1, None, None, None, None, 0, 26, 16, 13, 9, None, None, None, None, 0, None) != 0
    assert lib.dt_deepfm_infer(None, 7, None, None, None, None, 0, 26, 16, 13, None, None, None, None, 0, None) != 0


# ---- routing ------------------------------------------------------------------------------------------------------------
DEEPFM = ['linear', 'fm_nets', 'dnn_nets']
DCN = ['dcn_nets']
F_, D_, ND_ = 6, 8, 3
INFER_ENTRIES = ('dt_deepfm_infer_prepare', 'dt_deepfm_infer', 'dt_dcn_infer_prepare', 'dt_dcn_infer')


@pytest.fixture
def rec(monkeypatch):
    return install_recorder(monkeypatch, INFER_ENTRIES, ('DT_AMD_FUSED', 'DT_AMD_FUSED_PREDICT', 'DT_AMD_TOWER_DTYPE'))


def _model(nets, hidden=((100, 0, False), (40, 0, False)), task='binary', **extra):
    from deeptables_amd.models import ModelConfig, DeepModel
    from deeptables_amd.models.metainfo import CategoricalColumn, ContinuousColumn
    if nets == DCN:
        extra.setdefault('cross_params', {'num_cross_layer': 2})
    conf = ModelConfig(nets=nets, fixed_embedding_dim=True, embeddings_output_dim=D_,
                       dnn_params={'hidden_units': hidden, 'activation': extra.pop('activation', 'relu')},
                       **{'embedding_dropout': 0, **extra})
    dm = DeepModel(task, 2 if task != 'multiclass' else 3, conf, [CategoricalColumn(f'C{i}', 20 + i, D_) for i in range(F_)],
                   [ContinuousColumn('input_continuous_all', ['a', 'b', 'c'])])
    dm.build('cpu')
    return dm


def _frame(n, seed=0):
    g = np.random.default_rng(seed)
    df = pd.DataFrame({f'C{i}': g.integers(0, 20, n) for i in range(F_)})
    for k in ('a', 'b', 'c'):
        df[k] = g.standard_normal(n).astype(np.float32)
    return df


def _names(dm):
    """data_ptr -> 'layer.attr' of every parameter / moving statistic a launch may point to, 'ws' for the plan's workspace"""
    named = {}
    for lname, layer in dm.model.layers_by_name.items():
        for attr in ('kernel', 'bias', 'gamma', 'beta', 'moving_mean', 'moving_variance', 'kernel_stack', 'bias_stack'):
            t = getattr(layer, attr, None)
            if isinstance(t, torch.Tensor):
                named.setdefault(t.data_ptr(), []).append(f'{lname}.{attr}')
    named.setdefault(dm.inference_plan().ws.data_ptr(), []).append('ws')
    return {p: '|'.join(sorted(ns)) for p, ns in named.items()}


def _decode(args, names):
    import ctypes
    return [names.get(a.value, f'?{a.value:#x}') if isinstance(a, ctypes.c_void_p) else a for a in args]


def _expected_prepare(dm, net, ld1, ld2):
    """the decoded dt_*_infer_prepare arguments: the layers' current parameters by name"""
    L = dm.model.layers_by_name
    c = 'dnn' if net == DEEPFM else 'dcn'
    bn = L['bn_concat_emb_dense']
    d1, d2 = L[f'{c}_dense_1'], L[f'{c}_dense_2']

    def nm(layer, attr):
        return f'{layer.name}.{attr}' if getattr(layer, attr, None) is not None else None

    head = [F_, D_, ND_] + (['linear_logit.kernel'] if net == DEEPFM else ['dcn_cross_layer.kernel_stack',
                                                                          'dcn_cross_layer.bias_stack', 2])
    mid = [nm(bn, 'gamma'), nm(bn, 'beta'), nm(bn, 'moving_mean'), nm(bn, 'moving_variance'), float(bn.epsilon),
           nm(d1, 'kernel'), ld1, d1.kernel.shape[1], nm(d1, 'bias'), nm(d2, 'kernel'), ld2, d2.kernel.shape[1], nm(d2, 'bias')]
    bits, cellargs = 0, []
    for i in (1, 2):
        b = L.get(f'{c}_bn_{i}')
        if b is None:
            cellargs += [None, None, None, None, 0.0]
        else:
            bits |= 1 << (i - 1)
            cellargs += [nm(b, 'gamma'), nm(b, 'beta'), nm(b, 'moving_mean'), nm(b, 'moving_variance'), float(b.epsilon)]
    tail = (['dense_logit_dnn_nets.kernel', 'task_output.kernel'] if net == DEEPFM else ['task_output.kernel', None]) + \
        [nm(L['task_output'], 'bias'), 'ws', None]
    return head + mid + [bits] + cellargs + tail


def _check_calls(rec, dm, net, n, b, ld1, ld2):
    pre, inf = f'dt_{"deepfm" if net == DEEPFM else "dcn"}_infer_prepare', f'dt_{"deepfm" if net == DEEPFM else "dcn"}_infer'
    assert rec.names() == [pre] + [inf] * -(-n // b), rec.names()
    names = _names(dm)
    assert _decode(rec.calls[0][1], names) == _expected_prepare(dm, net, ld1, ld2)
    rows = 0
    for _, args in rec.calls[1:]:
        B = args[6]
        assert args[7:10] == (F_, D_, ND_) and 0 < B <= b
        k = 10 if net == DEEPFM else 11
        if net == DCN:
            assert args[10] == 2
        assert names.get(args[k].value) == 'ws'
        rows += B
    assert rows == n


@pytest.mark.parametrize('net', [DEEPFM, DCN])
@pytest.mark.parametrize('n,b', [(100, 32), (64, 64), (5, 128), (257, 7)])
def test_predict_makes_one_prepare_and_one_infer_per_batch(rec, net, n, b):
    dm = _model(net)
    out = dm.predict(_frame(n), batch_size=b)
    assert out.shape == (n, 1) and out.dtype == np.float32
    _check_calls(rec, dm, net, n, b, 100, 40)
    assert not hasattr(dm, '_fused_plan')
    flags = rec.calls[1][1][-2]
    from deeptables_amd import _lib
    assert flags == _lib.DT_INFER_SIGMOID


@pytest.mark.parametrize('net', [DEEPFM, DCN])
def test_pointers_follow_the_parameters_after_the_training_plan_rehomed_them(rec, net):
    """before any training plan the tower kernels are contiguous [C, H1] / [H1, H2] (ld = H1 / H2); once fused_plan() moved
    them into its zero-padded [C,128] / [128,64] slabs the same inference plan passes the slab views (ld = 128 / 64) — the
    pointers are read at call time"""
    dm = _model(net)
    plan = dm.inference_plan()
    ptrs = {n: p.data_ptr() for n, p in dm.model.named_parameters()}
    assert not hasattr(dm, '_fused_plan')
    assert {n: p.data_ptr() for n, p in dm.model.named_parameters()} == ptrs     # building the plan moved nothing
    dm.predict(_frame(40), batch_size=16)
    _check_calls(rec, dm, net, 40, 16, 100, 40)
    assert dm.fused_plan() is not None
    moved = {n for n, p in dm.model.named_parameters() if p.data_ptr() != ptrs[n]}
    assert moved, 'the training plan re-homes the tower'
    rec.calls.clear()
    dm.predict(_frame(40), batch_size=16)
    assert dm.inference_plan() is plan
    _check_calls(rec, dm, net, 40, 16, 128, 64)
    L = dm.model.layers_by_name
    c = 'dnn' if net == DEEPFM else 'dcn'
    assert rec.calls[0][1][9 if net == DEEPFM else 11].value == L[f'{c}_dense_1'].kernel.data_ptr()
    assert rec.calls[0][1][13 if net == DEEPFM else 15].value == L[f'{c}_dense_2'].kernel.data_ptr()


@pytest.mark.parametrize('net', [DEEPFM, DCN])
def test_evaluate_and_the_validation_pass_route_through_the_plan(rec, net, monkeypatch):
    dm = _model(net)
    n = 50
    df = _frame(n)
    y = (np.arange(n) % 3 == 0).astype(np.float32)
    # the recorded launches write nothing: the logits are whatever the buffer holds -> give it zeros
    monkeypatch.setattr(torch, 'empty', lambda *a, **k: torch.zeros(*a, **k))
    res = dm.evaluate(df, y, batch_size=16)
    assert 'loss' in res
    _check_calls(rec, dm, net, n, 16, 100, 40)
    assert abs(res['loss'] - float(np.log(2.0))) < 1e-6          # zero logits: BCE = log 2 in every batch


def test_fit_validation_pass_routes_through_the_plan(rec, monkeypatch):
    """fit's per-epoch validation scores the held-out fifth through the inference plan: one prepare, one infer per batch.
    The train steps themselves are not run here (no GPU): train_step is replaced by a no-op."""
    dm = _model(DEEPFM)
    monkeypatch.setattr(type(dm), 'train_step', lambda self, ins, yb, wb=None: (torch.zeros(()), torch.zeros(ins[0].shape[0], 1)))
    n = 100
    y = (np.arange(n) % 2 == 0).astype(np.float32)
    dm.fit(_frame(n), y, batch_size=16, epochs=2, verbose=0, validation_split=0.2, steps_per_execution=1)
    names = rec.names()
    assert names == (['dt_deepfm_infer_prepare'] + ['dt_deepfm_infer'] * 2) * 2, names


@pytest.mark.parametrize('case', ['apply', 'env', 'fused_off', 'multiclass', 'concat', 'sharded', 'tanh', 'wide', 'deep'])
def test_graphs_and_switches_the_plan_refuses_make_no_infer_calls(rec, monkeypatch, case):
    from deeptables_amd import _lib, fused
    kw = {}
    net = DEEPFM
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
    dm = _model(net, hidden, **kw)
    if case == 'env':
        monkeypatch.setenv('DT_AMD_FUSED_PREDICT', '0')
    elif case == 'fused_off':
        monkeypatch.setenv('DT_AMD_FUSED', '0')
    elif case == 'sharded':
        class _Sharded:
            sharded_embeddings, active, world_size = True, True, 1
        dm.config = dm.config._replace(distribute_strategy=_Sharded())
    # the layer path runs instead: on a CPU model its first kernel refuses the CPU tensors
    with pytest.raises(_lib.DtHipError, match='GPU only'):
        if case == 'apply':
            dm.apply(_frame(20), output_layers=['task_output'], batch_size=8)
        else:
            dm.predict(_frame(20), batch_size=8)
    assert not any(n.endswith('_infer') for n in rec.names()), rec.names()
    if case in ('env', 'fused_off'):
        assert dm.inference_plan() is None
    elif case != 'apply':
        assert fused.make_inference_plan(dm) is None


@pytest.mark.parametrize('net', [DEEPFM, DCN])
@pytest.mark.parametrize('hidden', [((100, 0.3, False), (40, 0.1, False)), ((64, 0, True), (32, 0, False)),
                                    ((128, 0.2, True), (64, 0, True))])
def test_dropout_and_batch_norm_cells_are_taken_at_inference_only(rec, net, hidden):
    """the tower cells the training plan refuses — dropout > 0, use_bn — are free at inference: the inference plan takes
    them, with each BN cell's moving statistics in the prepare call, and the training plan still refuses the graph"""
    dm = _model(net, hidden)
    assert dm.fused_plan() is None
    dm.predict(_frame(33), batch_size=16)
    _check_calls(rec, dm, net, 33, 16, hidden[0][0], hidden[1][0])
    bits = rec.calls[0][1][17 if net == DEEPFM else 19]
    assert bits == (1 if hidden[0][2] else 0) | (2 if hidden[1][2] else 0)


def test_regression_and_output_bias_flags(rec):
    from deeptables_amd import _lib
    dm = _model(DEEPFM, task='regression', output_use_bias=False)
    dm.predict(_frame(10), batch_size=4)
    assert rec.calls[1][1][-2] == 0                     # identity output
    assert rec.calls[0][1][-3] is None                  # no b_out
    rec.calls.clear()
    import os
    os.environ['DT_AMD_TOWER_DTYPE'] = 'bf16'
    try:
        dm.predict(_frame(10), batch_size=4)
    finally:
        del os.environ['DT_AMD_TOWER_DTYPE']
    assert rec.calls[1][1][-2] == _lib.DT_INFER_TOWER_BF16


def test_building_the_inference_plan_moves_nothing(rec):
    for net in (DEEPFM, DCN):
        dm = _model(net)
        before = {n: p.data_ptr() for n, p in dm.model.named_parameters()}
        plan = dm.inference_plan()
        assert type(plan).__name__ == ('InferDeepFM' if net == DEEPFM else 'InferDCN')
        assert not hasattr(dm, '_fused_plan')
        assert {n: p.data_ptr() for n, p in dm.model.named_parameters()} == before
        assert getattr(dm.optimizer, '_flat', None) is None
