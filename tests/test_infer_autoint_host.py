# -*- coding:utf-8 -*-
"""CPU: the inference plan for the AutoInt graph (fused.InferAutoInt, dt_autoint_infer*, csrc/autoint.hip) — what the
library's predicate accepts, which graphs take the plan, which calls `predict` makes with which tensors.  The plans are
built on CPU models and their launches recorded by a stand-in for the library (the recorder of
tests/test_infer_xdeepfm_host.py, restated for the dt_autoint_infer* names): nothing runs on a GPU."""
import ctypes

import numpy as np
import pandas as pd
import pytest

from tests.infer_support import install_recorder
from tests.test_infer_host import DEEPFM, DCN, _decode, _names
from tests.test_infer_host import _model as _other_model

F_, D_, ND_ = 6, 16, 3
AI_ENTRIES = ('dt_autoint_infer_prepare', 'dt_autoint_infer')
OTHER_ENTRIES = ('dt_deepfm_infer_prepare', 'dt_deepfm_infer', 'dt_dcn_infer_prepare', 'dt_dcn_infer',
                 'dt_stack_infer_prepare', 'dt_stack_infer', 'dt_xdeepfm_infer_prepare', 'dt_xdeepfm_infer_tower',
                 'dt_xdeepfm_infer_cin', 'dt_xdeepfm_infer_head')
F32, BF16, X2 = 0, 1, 2
AUTOINT = {'num_attention': 2, 'num_heads': 2, 'dropout_rate': 0, 'use_residual': True}


@pytest.fixture
def rec(monkeypatch):
    return install_recorder(monkeypatch, AI_ENTRIES + OTHER_ENTRIES,
                            ('DT_AMD_FUSED', 'DT_AMD_FUSED_PREDICT', 'DT_AMD_AUTOINT_DTYPE'))


def _model(nets=('autoint_nets',), task='binary', D=D_, conts=True, autoint=AUTOINT, **extra):
    from deeptables_amd.models import ModelConfig, DeepModel
    from deeptables_amd.models.metainfo import CategoricalColumn, ContinuousColumn
    conf = ModelConfig(nets=list(nets), fixed_embedding_dim=True, embeddings_output_dim=D, autoint_params=dict(autoint),
                       dnn_params={'hidden_units': ((100, 0, False), (40, 0, False)), 'activation': 'relu'},
                       **{'embedding_dropout': 0, **extra})
    dm = DeepModel(task, 2 if task != 'multiclass' else 3, conf, [CategoricalColumn(f'C{i}', 20 + i, D) for i in range(F_)],
                   [ContinuousColumn('input_continuous_all', ['a', 'b', 'c'])] if conts else [])
    dm.build('cpu')
    return dm


def _frame(n, seed=0, conts=True):
    g = np.random.default_rng(seed)
    df = pd.DataFrame({f'C{i}': g.integers(0, 20, n) for i in range(F_)})
    for k in ('a', 'b', 'c') if conts else ():
        df[k] = g.standard_normal(n).astype(np.float32)
    return df


def _host_ptrs(arg, n):
    return list((ctypes.c_void_p * n).from_address(arg.value))


# ---- the library's predicates (no launch) ---------------------------------------------------------------------------------
def test_the_codes_are_the_headers():
    from deeptables_amd import _lib
    assert (_lib.DT_AI_F32, _lib.DT_AI_BF16, _lib.DT_AI_BF16X2) == (F32, BF16, X2)
    assert (_lib.DT_AUTOINT_INFER_MAX_LAYERS, _lib.DT_AUTOINT_INFER_MAX_BLOCKS) == (8, 256)


def test_predicate_follows_the_layer_kernels_domain_the_modes_and_the_lds_budget():
    from deeptables_amd import _lib
    lib = _lib.lib()
    MAXL = _lib.DT_AUTOINT_INFER_MAX_LAYERS
    for F in (0, 1, 16, 17, 26, 32, 33):
        for D in (8, 16, 32, 64):
            for H in (1, 2, 3, 4, 8):
                want = lib.dt_autoint_supported(F, D, H)
                assert lib.dt_autoint_infer_supported(F, D, H, 1, 1, F32) == want, (F, D, H)
                assert lib.dt_autoint_infer_supported(F, D, H, 3, 0, F32) == want, (F, D, H)
    assert lib.dt_autoint_infer_supported(33, 32, 4, 3, 1, F32) == 0 and lib.dt_autoint_infer_supported(26, 8, 2, 3, 1, F32) == 0
    # the bf16 modes: D = 32 only
    for mode in (BF16, X2):
        assert lib.dt_autoint_infer_supported(26, 32, 4, 3, 1, mode) == 1 and lib.dt_autoint_infer_supported(26, 16, 4, 3, 1, mode) == 0
    assert lib.dt_autoint_infer_supported(26, 32, 4, 3, 1, 3) == 0 and lib.dt_autoint_infer_supported(26, 32, 4, 3, 1, -1) == 0
    assert lib.dt_autoint_infer_supported(26, 32, 4, 3, 2, F32) == 0
    # 1 <= n_layers <= DT_AUTOINT_INFER_MAX_LAYERS
    assert lib.dt_autoint_infer_supported(26, 16, 4, 0, 1, F32) == 0 and lib.dt_autoint_infer_supported(26, 16, 4, MAXL + 1, 1, F32) == 0
    assert lib.dt_autoint_infer_supported(26, 16, 4, MAXL, 1, F32) == 1
    # include/dt_hip.h: at D = 32 five layers' weights and four slabs fit the LDS, six do not
    for mode in (F32, BF16, X2):
        assert lib.dt_autoint_infer_supported(26, 32, 4, 5, 1, mode) == 1 and lib.dt_autoint_infer_supported(26, 32, 4, 6, 1, mode) == 0
    # the workspace is the LDS image: per layer Wcat [D][4 D + 4] | bcat [4 D] | s | t, then the head [32 D] + 4 floats
    assert lib.dt_autoint_infer_workspace_bytes(26, 32, 3) == 4 * (3 * (32 * 132 + 6 * 32) + 32 * 32 + 4)
    assert lib.dt_autoint_infer_workspace_bytes(1, 16, 8) == 4 * (8 * (16 * 68 + 6 * 16) + 32 * 16 + 4)
    for F, D, n in ((26, 32, 5), (32, 16, 1), (1, 32, 1)):
        assert lib.dt_autoint_infer_workspace_bytes(F, D, n) > 0
    for F, D, n in ((26, 32, 6), (33, 32, 3), (0, 16, 1), (26, 8, 3), (26, 16, 0), (26, 16, MAXL + 1)):
        assert lib.dt_autoint_infer_workspace_bytes(F, D, n) == -1, (F, D, n)


def test_entry_points_check_their_arguments_before_any_launch():
    from deeptables_amd import _lib
    lib = _lib.lib()
    none = [None, 1, None, None, None]                 # idx, idx_kind, table, row_offset, vocab
    assert lib.dt_autoint_infer(*none, 0, 26, 32, 4, 3, 4, None, None, None, None, 1, X2, None) == 0            # an empty batch
    assert lib.dt_autoint_infer(*none, 5, 26, 32, 4, 3, 4, None, None, None, None, 1, X2, None) != 0
    assert b'dt_autoint_infer' in lib.dt_last_error()
    assert lib.dt_autoint_infer(*none, 0, 26, 32, 4, 6, 4, None, None, None, None, 0, X2, None) != 0            # six layers
    assert lib.dt_autoint_infer(*none, 0, 26, 32, 4, 3, 2, None, None, None, None, 0, X2, None) != 0            # NP = 2
    assert lib.dt_autoint_infer(*none, 0, 26, 16, 4, 3, 4, None, None, None, None, 0, X2, None) != 0            # bf16x2 at D = 16
    assert lib.dt_autoint_infer(*none, 0, 26, 32, 4, 3, 4, None, None, None, None, 0x2, X2, None) != 0          # an unknown flag
    assert lib.dt_autoint_infer(None, 7, None, None, None, 0, 26, 32, 4, 3, 4, None, None, None, None, 0, X2, None) != 0
    assert lib.dt_autoint_infer(*none, 1 << 31, 26, 32, 4, 3, 4, None, None, None, None, 0, X2, None) != 0
    assert lib.dt_autoint_infer_prepare(26, 32, 3, *([None] * 12), 1e-3, None, None, None, None) != 0
    assert b'dt_autoint_infer_prepare' in lib.dt_last_error()
    assert lib.dt_autoint_infer_prepare(26, 32, 6, *([None] * 12), 1e-3, None, None, None, None) != 0


# ---- routing ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('task', ['binary', 'regression'])
@pytest.mark.parametrize('conts', [True, False])
def test_the_graph_takes_the_plan(rec, task, conts):
    from deeptables_amd import fused
    dm = _model(task=task, conts=conts)
    plan = dm.inference_plan()
    assert type(plan) is fused.InferAutoInt
    assert (plan.F, plan.D, plan.H, plan.n_layers) == (F_, D_, 2, 2)
    assert rec.names() == [] and not hasattr(dm, '_fused_plan')


@pytest.mark.parametrize('task', ['binary', 'regression'])
def test_predict_makes_one_prepare_per_call_and_one_launch_per_batch(rec, task):
    from deeptables_amd import _lib
    dm = _model(task=task)
    plan = dm.inference_plan()
    n, b, nl = 20, 8, 2
    out = dm.predict(_frame(n), batch_size=b)
    assert out.shape == (n, 1) and out.dtype == np.float32
    assert rec.names() == ['dt_autoint_infer_prepare'] + ['dt_autoint_infer'] * 3
    names = _names(dm)
    L = dm.model.layers_by_name
    mha = [L['multihead_attention'], L['multihead_attention_1']]
    for l in mha:
        for sub in (l.dense_Q, l.dense_K, l.dense_V, l.dense_residual):
            names[sub.kernel.data_ptr()] = f'{sub.name}.kernel'
            names[sub.bias.data_ptr()] = f'{sub.name}.bias'
        bn = l.batch_normalize
        for attr in ('gamma', 'beta', 'moving_mean', 'moving_variance'):
            names[getattr(bn, attr).data_ptr()] = f'{bn.name}.{attr}'
    # prepare: F, D, n_layers, the twelve per-layer pointer arrays, eps, task_output's kernel and bias, the workspace, the stream
    pa = rec.calls[0][1]
    assert len(pa) == 20 and pa[:3] == (F_, D_, nl)
    subs = ('q', 'k', 'v', 'residual')
    for j, sub in enumerate(subs):
        assert [names[p] for p in _host_ptrs(pa[3 + j], nl)] == [f'{l.name}_dense_{sub}.kernel' for l in mha]
        assert [names[p] for p in _host_ptrs(pa[7 + j], nl)] == [f'{l.name}_dense_{sub}.bias' for l in mha]
    for j, attr in enumerate(('gamma', 'beta', 'moving_mean', 'moving_variance')):
        assert [names[p] for p in _host_ptrs(pa[11 + j], nl)] == [f'{l.name}_bn.{attr}' for l in mha]
    assert pa[15] == pytest.approx(float(mha[0].batch_normalize.epsilon))
    assert _decode(pa[16:19], names) == ['task_output.kernel', 'task_output.bias', 'ws'] and pa[19] is None
    assert tuple(L['task_output'].kernel.shape) == (F_ * D_, 1)
    assert plan.ws.numel() * 4 == _lib.lib().dt_autoint_infer_workspace_bytes(F_, D_, nl)
    # per batch: the plan's own table / offsets / vocabulary / workspace; B = 8, 8, 4; outputs are slices of one buffer
    emb = L['emb_categorical_vars_all']
    rows, lg0, out0 = 0, None, None
    for i in range(3):
        a = rec.calls[1 + i][1]
        assert len(a) == 18 and a[1] in (_lib.DT_IDX_F32, _lib.DT_IDX_I32)
        assert a[2].value == emb.tables[plan.key].data_ptr()
        assert a[3].value == getattr(emb, f'row_offset_{plan.key}').data_ptr()
        assert a[4].value == getattr(emb, f'vocab_{plan.key}').data_ptr()
        assert a[5] == (8, 8, 4)[i] and a[6:11] == (F_, D_, 2, nl, 4)
        assert a[11].value == plan.ws.data_ptr() and a[14] is None
        assert a[15] == (_lib.DT_INFER_SIGMOID if task == 'binary' else 0) and a[16] == F32 and a[17] is None
        if i == 0:
            lg0, out0 = a[12].value, a[13].value
        assert a[12].value == lg0 + 4 * rows and a[13].value == out0 + 4 * rows
        rows += a[5]
    assert rows == n


def test_no_residual_hands_over_null_entries_and_np_3(rec):
    dm = _model(autoint=dict(AUTOINT, use_residual=False, num_attention=3), output_use_bias=False)
    dm.predict(_frame(10), batch_size=16)
    assert rec.names() == ['dt_autoint_infer_prepare', 'dt_autoint_infer']
    pa = rec.calls[0][1]
    assert pa[2] == 3 and _host_ptrs(pa[6], 3) == [None] * 3 and _host_ptrs(pa[10], 3) == [None] * 3
    assert all(p is not None for j in (3, 4, 5, 7, 8, 9) for p in _host_ptrs(pa[j], 3))
    assert pa[17] is None                                # no output bias: NULL
    assert rec.calls[1][1][10] == 3 and rec.calls[1][1][5] == 10


def test_prepare_reads_the_tensors_and_the_mode_at_call_time(rec):
    """the plan caches no parameter: a kernel re-homed between two predict calls is the one the second prepare names; the
    precision mode is read in prepare"""
    import torch
    dm = _model(D=32, autoint=dict(AUTOINT, num_heads=4))
    plan = dm.inference_plan()
    dm.predict(_frame(10), batch_size=16)
    q0 = dm.model.layers_by_name['multihead_attention'].dense_Q
    before = _host_ptrs(rec.calls[0][1][3], 2)
    assert before[0] == q0.kernel.data_ptr() and rec.calls[1][1][16] == X2          # D = 32: split-bf16 by default
    q0.kernel.data = torch.clone(q0.kernel.data) * 2
    for l in plan.mha:
        l.params['mfma_dtype'] = 'bf16'                  # the layer path reads this key on every call too
    rec.calls.clear()
    dm.predict(_frame(10), batch_size=16)
    after = _host_ptrs(rec.calls[0][1][3], 2)
    assert after[0] == q0.kernel.data_ptr() != before[0] and after[1] == before[1]
    assert rec.calls[1][1][16] == BF16
    plan.mha[0].params['mfma_dtype'] = 'fp8'
    with pytest.raises(ValueError):
        dm.predict(_frame(10), batch_size=16)


@pytest.mark.parametrize('case', ['multiclass', 'with_dnn', 'with_linear', 'concat', 'sharded', 'env', 'fused_off', 'D8'])
def test_graphs_and_switches_refused(rec, monkeypatch, case):
    from deeptables_amd import _lib, fused
    kw = {}
    if case == 'multiclass':
        kw['task'] = 'multiclass'
    elif case == 'with_dnn':
        kw['nets'] = ['autoint_nets', 'dnn_nets']
    elif case == 'with_linear':
        kw['nets'] = ['linear', 'autoint_nets']
    elif case == 'concat':
        kw['stacking_op'] = 'concat'
    elif case == 'D8':
        kw['D'] = 8
    dm = _model(**kw)
    if case == 'env':
        monkeypatch.setenv('DT_AMD_FUSED_PREDICT', '0')
    elif case == 'fused_off':
        monkeypatch.setenv('DT_AMD_FUSED', '0')
    elif case == 'sharded':
        class _Sharded:
            sharded_embeddings, active, world_size = True, True, 1
        dm.config = dm.config._replace(distribute_strategy=_Sharded())
    assert fused.make_inference_plan(dm) is None
    assert not (case not in ('env', 'fused_off') and fused.InferAutoInt.eligible(dm))
    with pytest.raises(_lib.DtHipError, match='GPU only'):        # the layer path runs: its first kernel refuses CPU tensors
        dm.predict(_frame(20), batch_size=8)
    assert rec.names() == []


def test_too_many_layers_and_a_mode_the_size_does_not_take_are_refused(rec):
    from deeptables_amd import fused
    assert type(fused.make_inference_plan(_model(D=32, autoint=dict(AUTOINT, num_attention=5)))) is fused.InferAutoInt
    assert fused.make_inference_plan(_model(D=32, autoint=dict(AUTOINT, num_attention=6))) is None
    assert fused.make_inference_plan(_model(D=16, autoint=dict(AUTOINT, mfma_dtype='bf16x2'))) is None
    assert fused.make_inference_plan(_model(D=16, autoint=dict(AUTOINT, num_heads=8))) is None        # d_h = 2
    assert rec.names() == []


def test_the_other_graphs_keep_their_plans(rec):
    from deeptables_amd import fused
    assert type(_other_model(DEEPFM).inference_plan()) is fused.InferDeepFM
    assert type(_other_model(DCN).inference_plan()) is fused.InferDCN
    assert type(_other_model(['linear', 'dnn_nets']).inference_plan()) is fused.InferStack
    assert type(_other_model(['linear', 'cin_nets', 'dnn_nets'],
                             cin_params={'cross_layer_size': (8, 6), 'direct': False}).inference_plan()) is fused.InferXDeepFM
    for nets in (DEEPFM, DCN, ['dnn_nets']):
        assert not fused.InferAutoInt.eligible(_other_model(nets))
    assert _model().fused_plan() is None                 # the training side has no AutoInt plan


def test_building_the_plan_moves_nothing(rec):
    dm = _model()
    before = {n: p.data_ptr() for n, p in dm.model.named_parameters()}
    assert type(dm.inference_plan()).__name__ == 'InferAutoInt'
    assert {n: p.data_ptr() for n, p in dm.model.named_parameters()} == before
    assert getattr(dm.optimizer, '_flat', None) is None
