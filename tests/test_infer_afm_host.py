# -*- coding:utf-8 -*-
"""CPU: the inference plan for the AFM graphs (fused.InferAFM, dt_afm_infer*, csrc/afm_infer.hip) — what the library's
predicate accepts, which graphs take the plan, which calls `predict` / `evaluate` / fit's validation pass make with which
tensors.  The plans are built on CPU models and their launches recorded by a stand-in for the library (the recorder of
tests/test_infer_autoint_host.py, restated for the dt_afm_infer* names): nothing runs on a GPU."""
import numpy as np
import pandas as pd
import pytest

from tests.infer_support import install_recorder
from tests.test_infer_host import DEEPFM, DCN, _decode, _names
from tests.test_infer_host import _model as _other_model

F_, D_, ND_, H_ = 6, 16, 3, 16
AFM_ENTRIES = ('dt_afm_infer_prepare', 'dt_afm_infer')
OTHER_ENTRIES = ('dt_deepfm_infer_prepare', 'dt_deepfm_infer', 'dt_dcn_infer_prepare', 'dt_dcn_infer',
                 'dt_stack_infer_prepare', 'dt_stack_infer', 'dt_xdeepfm_infer_prepare', 'dt_xdeepfm_infer_tower',
                 'dt_xdeepfm_infer_cin', 'dt_xdeepfm_infer_head', 'dt_autoint_infer_prepare', 'dt_autoint_infer')
LIN, FM, AFM = 0x1, 0x2, 0x8
# the four graphs, each in two orders of config.nets
GRAPHS = [(['afm_nets'], AFM), (['afm_nets'], AFM),
          (['linear', 'afm_nets'], AFM | LIN), (['afm_nets', 'linear'], AFM | LIN),
          (['fm_nets', 'afm_nets'], AFM | FM), (['afm_nets', 'fm_nets'], AFM | FM),
          (['linear', 'fm_nets', 'afm_nets'], AFM | LIN | FM), (['afm_nets', 'fm_nets', 'linear'], AFM | LIN | FM)]


@pytest.fixture
def rec(monkeypatch):
    return install_recorder(monkeypatch, AFM_ENTRIES + OTHER_ENTRIES, ('DT_AMD_FUSED', 'DT_AMD_FUSED_PREDICT'))


def _model(nets=('linear', 'afm_nets'), task='binary', D=D_, F=F_, afm=None, **extra):
    from deeptables_amd.models import ModelConfig, DeepModel
    from deeptables_amd.models.metainfo import CategoricalColumn, ContinuousColumn
    conf = ModelConfig(nets=list(nets), fixed_embedding_dim=True, embeddings_output_dim=D,
                       afm_params=dict(afm or {'hidden_factor': H_, 'dropout_rate': 0}),
                       dnn_params={'hidden_units': ((100, 0, False), (40, 0, False)), 'activation': 'relu'},
                       **{'embedding_dropout': 0, **extra})
    dm = DeepModel(task, 2 if task != 'multiclass' else 3, conf, [CategoricalColumn(f'C{i}', 20 + i, D) for i in range(F)],
                   [ContinuousColumn('input_continuous_all', ['a', 'b', 'c'])])
    dm.build('cpu')
    return dm


def _frame(n, seed=0, F=F_, y=False):
    g = np.random.default_rng(seed)
    df = pd.DataFrame({f'C{i}': g.integers(0, 20, n) for i in range(F)})
    for k in ('a', 'b', 'c'):
        df[k] = g.standard_normal(n).astype(np.float32)
    return (df, g.integers(0, 2, n)) if y else df


def _afm_names(dm):
    names = _names(dm)
    afm = dm.model.layers_by_name['afm_layer']
    names[afm.dense_attention.kernel.data_ptr()] = 'dense_afm_attention.kernel'
    names[afm.dense_attention.bias.data_ptr()] = 'dense_afm_attention.bias'
    names[afm.attention_p.data_ptr()] = 'projection_h'
    names[afm.dense_out.kernel.data_ptr()] = 'afm_layer_dense_out.kernel'
    return names


# ---- the library's predicates (no launch) ---------------------------------------------------------------------------------
def test_the_codes_are_the_headers():
    from deeptables_amd import _lib
    assert (_lib.DT_NET_LINEAR, _lib.DT_NET_FM, _lib.DT_NET_AFM) == (LIN, FM, AFM)
    assert (_lib.DT_AFM_INFER_ROWS, _lib.DT_AFM_INFER_MAX_BLOCKS) == (4, 1024)


def test_predicate_at_and_just_beyond_each_limit():
    from deeptables_amd import _lib
    lib = _lib.lib()
    ok = lib.dt_afm_infer_supported
    RELU = _lib.DT_ACT_RELU
    # at least two fields
    assert ok(1, 16, 0, 16, RELU, AFM) == 0 and ok(2, 16, 0, 16, RELU, AFM) == 1
    # F D <= 512 (128 lookups of 16 bytes)
    assert ok(128, 4, 0, 16, RELU, AFM) == 1 and ok(129, 4, 0, 16, RELU, AFM) == 0
    assert ok(32, 16, 0, 16, RELU, AFM) == 1 and ok(33, 16, 0, 16, RELU, AFM) == 0
    assert ok(8, 64, 0, 16, RELU, AFM) == 1 and ok(9, 64, 0, 16, RELU, AFM) == 0
    # the attention factor
    assert ok(26, 16, 13, 64, RELU, AFM) == 1 and ok(26, 16, 13, 65, RELU, AFM) == 0
    assert ok(26, 16, 13, 1, RELU, AFM) == 1 and ok(26, 16, 13, 0, RELU, AFM) == 0
    # the embedding sizes of deepfm_dims
    for D in (4, 8, 16, 32, 64):
        assert ok(4, D, 0, 16, RELU, AFM | LIN | FM) == 1, D
    for D in (0, 2, 12, 20, 128):
        assert ok(4, D, 0, 16, RELU, AFM) == 0, D
    # every activation dt_afm_fwd takes, none beyond
    for act in range(9):
        assert ok(26, 16, 13, 16, act, AFM | LIN) == 1, act
    assert ok(26, 16, 13, 16, 9, AFM) == 0 and ok(26, 16, 13, 16, -1, AFM) == 0
    # the mask: DT_NET_AFM with or without linear / fm_nets, nothing else
    for nets, want in ((AFM, 1), (AFM | LIN, 1), (AFM | FM, 1), (AFM | LIN | FM, 1), (0, 0), (LIN | FM, 0), (AFM | 0x4, 0),
                       (AFM | 0x10, 0)):
        assert ok(26, 16, 13, 16, RELU, nets) == want, nets
    assert ok(26, 16, 64, 16, RELU, AFM | LIN) == 1 and ok(26, 16, 65, 16, RELU, AFM | LIN) == 0
    # the workspace: stamp [4] | Wa [D][HP] | ba [HP] | h [HP] | w_do [D] | head [4] | w_lin [F + Nd] | the pair table [P16],
    # each region rounded up to four floats; HP = 16 / 32 / 64
    wsb = lib.dt_afm_infer_workspace_bytes
    assert wsb(26, 16, 13, 16, AFM) == 4 * (4 + 16 * 16 + 16 + 16 + 16 + 4 + 336)
    assert wsb(26, 16, 13, 16, AFM | LIN) == 4 * (4 + 16 * 16 + 16 + 16 + 16 + 4 + 40 + 336)
    assert wsb(26, 16, 13, 17, AFM) == 4 * (4 + 16 * 32 + 32 + 32 + 16 + 4 + 336)
    assert wsb(2, 4, 0, 64, AFM | FM) == 4 * (4 + 4 * 64 + 64 + 64 + 4 + 4 + 16)
    for bad in ((1, 16, 0, 16, AFM), (26, 16, 0, 65, AFM), (26, 12, 0, 16, AFM), (26, 16, 0, 16, LIN)):
        assert wsb(*bad) == -1, bad


def test_entry_points_check_their_arguments_before_any_launch():
    from deeptables_amd import _lib
    lib = _lib.lib()
    none = [None, 1, None, None, None, None]            # idx, idx_kind, table, row_offset, vocab, dense
    tail = [None, None, None, None]                     # workspace, logit_out, out, oob_count
    assert lib.dt_afm_infer(*none, 0, 26, 16, 13, 16, AFM | LIN, 1, *tail, 1, None) == 0             # an empty batch
    assert lib.dt_afm_infer(*none, 5, 26, 16, 13, 16, AFM | LIN, 1, *tail, 1, None) != 0
    assert b'dt_afm_infer' in lib.dt_last_error()
    assert lib.dt_afm_infer(*none, 0, 26, 16, 13, 65, AFM, 1, *tail, 0, None) != 0                   # H = 65
    assert lib.dt_afm_infer(*none, 0, 1, 16, 13, 16, AFM, 1, *tail, 0, None) != 0                    # one field
    assert lib.dt_afm_infer(*none, 0, 26, 16, 13, 16, LIN, 1, *tail, 0, None) != 0                   # no DT_NET_AFM
    assert lib.dt_afm_infer(*none, 0, 26, 16, 13, 16, AFM, 9, *tail, 0, None) != 0                   # an unknown activation
    assert lib.dt_afm_infer(*none, 0, 26, 16, 13, 16, AFM, 1, *tail, 0x2, None) != 0                 # an unknown flag
    assert lib.dt_afm_infer(None, 7, None, None, None, None, 0, 26, 16, 13, 16, AFM, 1, *tail, 0, None) != 0
    assert lib.dt_afm_infer(*none, 1 << 31, 26, 16, 13, 16, AFM, 1, *tail, 0, None) != 0
    assert lib.dt_afm_infer_prepare(26, 16, 13, 16, AFM, *([None] * 9)) != 0
    assert b'dt_afm_infer_prepare' in lib.dt_last_error()
    assert lib.dt_afm_infer_prepare(26, 16, 13, 65, AFM, *([None] * 9)) != 0


# ---- routing ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', range(len(GRAPHS)))
def test_each_graph_takes_the_plan_and_predict_makes_its_calls(rec, k):
    """prepare once per call, one launch per batch and no other library call; the pointers are the layers' own tensors"""
    from deeptables_amd import _lib, fused
    nets, mask = GRAPHS[k]
    task = 'regression' if k % 2 else 'binary'
    bias = k not in (2, 5)
    dm = _model(nets=nets, task=task, output_use_bias=bias)
    plan = dm.inference_plan()
    assert type(plan) is fused.InferAFM and plan.mask == mask
    assert (plan.F, plan.D, plan.Nd, plan.H) == (F_, D_, ND_, H_)
    assert rec.names() == [] and not hasattr(dm, '_fused_plan')
    L = dm.model.layers_by_name
    assert tuple(L['task_output'].kernel.shape) == (1, 1) and 'dense_logit_afm_nets' not in L
    n, b = 33, 16
    out = dm.predict(_frame(n), batch_size=b)
    assert out.shape == (n, 1) and out.dtype == np.float32
    assert rec.names() == ['dt_afm_infer_prepare'] + ['dt_afm_infer'] * 3
    names = _afm_names(dm)
    # prepare: F, D, Nd, H, nets, Wa, ba, h, w_do, w_lin, w_out, b_out, the workspace, the stream
    pa = rec.calls[0][1]
    assert len(pa) == 14 and pa[:5] == (F_, D_, ND_, H_, mask)
    assert _decode(pa[5:13], names) == [
        'dense_afm_attention.kernel', 'dense_afm_attention.bias', 'projection_h', 'afm_layer_dense_out.kernel',
        'linear_logit.kernel' if mask & LIN else None, 'task_output.kernel', 'task_output.bias' if bias else None, 'ws']
    assert pa[13] is None
    assert (L['task_output'].bias is None) == (not bias)
    assert plan.ws.numel() * 4 == _lib.lib().dt_afm_infer_workspace_bytes(F_, D_, ND_, H_, mask)
    emb = L['emb_categorical_vars_all']
    rows, lg0, out0 = 0, None, None
    for i in range(3):
        a = rec.calls[1 + i][1]
        assert len(a) == 19 and a[1] in (_lib.DT_IDX_F32, _lib.DT_IDX_I32)
        assert a[2].value == emb.tables[plan.key].data_ptr()
        assert a[3].value == getattr(emb, f'row_offset_{plan.key}').data_ptr()
        assert a[4].value == getattr(emb, f'vocab_{plan.key}').data_ptr()
        assert (a[5] is None) == (not mask & LIN)                 # dense: NULL when `linear` is absent
        assert a[6] == (16, 16, 1)[i] and a[7:12] == (F_, D_, ND_, H_, mask) and a[12] == _lib.DT_ACT_RELU
        assert a[13].value == plan.ws.data_ptr() and a[16] is None
        assert a[17] == (_lib.DT_INFER_SIGMOID if task == 'binary' else 0) and a[18] is None
        if i == 0:
            lg0, out0 = a[14].value, a[15].value
        assert a[14].value == lg0 + 4 * rows and a[15].value == out0 + 4 * rows
        rows += a[6]
    assert rows == n


def test_evaluate_and_fits_validation_pass_make_the_same_family(rec, monkeypatch):
    """evaluate: one prepare, one infer per batch.  fit's per-epoch validation scores the held-out fifth the same way (the
    train steps themselves are not run here, no GPU: train_step is replaced by a no-op)"""
    import torch
    dm = _model()
    n = 40
    y = (np.arange(n) % 3 == 0).astype(np.float32)
    # the recorded launches write nothing: the logits are whatever the buffer holds -> give it zeros
    monkeypatch.setattr(torch, 'empty', lambda *a, **k: torch.zeros(*a, **k))
    res = dm.evaluate(_frame(n), y, batch_size=16)
    assert rec.names() == ['dt_afm_infer_prepare'] + ['dt_afm_infer'] * 3
    assert abs(res['loss'] - float(np.log(2.0))) < 1e-6          # zero logits: BCE = log 2 in every batch
    rec.calls.clear()
    monkeypatch.setattr(type(dm), 'train_step', lambda self, ins, yb, wb=None: (torch.zeros(()), torch.zeros(ins[0].shape[0], 1)))
    n = 100
    y = (np.arange(n) % 2 == 0).astype(np.float32)
    dm.fit(_frame(n), y, batch_size=16, epochs=2, verbose=0, validation_split=0.2, steps_per_execution=1)
    assert rec.names() == (['dt_afm_infer_prepare'] + ['dt_afm_infer'] * 2) * 2


def test_the_activation_code_and_hidden_factor_reach_the_launch(rec):
    from deeptables_amd import _lib
    dm = _model(nets=['afm_nets'], afm={'hidden_factor': 5, 'dropout_rate': 0.3, 'activation': 'tanh'})
    dm.predict(_frame(10), batch_size=16)
    assert rec.names() == ['dt_afm_infer_prepare', 'dt_afm_infer']
    assert rec.calls[0][1][3] == 5 and rec.calls[0][1][9] is None
    a = rec.calls[1][1]
    assert a[5] is None and a[6] == 10 and a[10] == 5 and a[11] == AFM and a[12] == _lib.ACT_CODES['tanh']
    # the activation is read in prepare: the layer path reads the attribute on every call too
    dm.inference_plan().afm.activation_function = 'selu'
    rec.calls.clear()
    dm.predict(_frame(10), batch_size=16)
    assert rec.calls[1][1][12] == _lib.ACT_CODES['selu']


def test_prepare_reads_the_tensors_at_call_time(rec):
    """the plan caches no parameter: a kernel re-homed between two predict calls is the one the second prepare names"""
    import torch
    dm = _model()
    dm.predict(_frame(10), batch_size=16)
    att = dm.model.layers_by_name['afm_layer'].dense_attention
    before = rec.calls[0][1][5].value
    assert before == att.kernel.data_ptr()
    att.kernel.data = torch.clone(att.kernel.data) * 2
    rec.calls.clear()
    dm.predict(_frame(10), batch_size=16)
    assert rec.calls[0][1][5].value == att.kernel.data_ptr() != before


REFUSED = ['multiclass', 'concat', 'sharded', 'fused_off', 'predict_off', 'one_field', 'H65', 'D12', 'afm_twice', 'with_dnn',
           'with_cin', 'unknown_act', 'dropout_1']


@pytest.mark.parametrize('case', REFUSED)
def test_graphs_and_switches_refused(rec, monkeypatch, case):
    from deeptables_amd import _lib, fused
    kw = {}
    if case == 'multiclass':
        kw['task'] = 'multiclass'
    elif case == 'concat':
        kw['stacking_op'] = 'concat'
    elif case == 'one_field':
        kw['F'] = 1
    elif case == 'H65':
        kw['afm'] = {'hidden_factor': 65}
    elif case == 'D12':
        kw['D'] = 12
    elif case == 'with_dnn':
        kw['nets'] = ['afm_nets', 'dnn_nets']
    elif case == 'with_cin':
        kw['nets'] = ['linear', 'afm_nets', 'cin_nets']
        kw['cin_params'] = {'cross_layer_size': (8, 6), 'direct': False}
    dm = _model(**kw)
    # what the model builder itself would refuse is put on the built layer, where the plan reads it
    if case == 'unknown_act':
        dm.model.layers_by_name['afm_layer'].activation_function = 'gelu'
    elif case == 'dropout_1':
        dm.model.layers_by_name['afm_layer'].dropout_rate = 1.0
    if case == 'predict_off':
        monkeypatch.setenv('DT_AMD_FUSED_PREDICT', '0')
    elif case == 'fused_off':
        monkeypatch.setenv('DT_AMD_FUSED', '0')
    elif case == 'afm_twice':
        # ModelConfig drops a repeated name (deepnets.get_nets), so the repetition is put where the plan reads it
        dm.config = dm.config._replace(nets=['afm_nets', 'linear', 'afm_nets'])
    elif case == 'sharded':
        class _Sharded:
            sharded_embeddings, active, world_size = True, True, 1
        dm.config = dm.config._replace(distribute_strategy=_Sharded())
    assert fused.make_inference_plan(dm) is None
    assert not (case not in ('predict_off', 'fused_off') and fused.InferAFM.eligible(dm))
    with pytest.raises(_lib.DtHipError, match='GPU only'):        # the layer path runs: its first kernel refuses CPU tensors
        dm.predict(_frame(20, F=kw.get('F', F_)), batch_size=8)
    assert rec.names() == []


def test_the_other_graphs_keep_their_plans(rec):
    from deeptables_amd import fused
    assert type(_other_model(DEEPFM).inference_plan()) is fused.InferDeepFM
    assert type(_other_model(DCN).inference_plan()) is fused.InferDCN
    assert type(_other_model(['linear', 'dnn_nets']).inference_plan()) is fused.InferStack
    assert type(_other_model(['linear', 'fm_nets']).inference_plan()) is fused.InferStack
    assert type(_other_model(['linear', 'cin_nets', 'dnn_nets'],
                             cin_params={'cross_layer_size': (8, 6), 'direct': False}).inference_plan()) is fused.InferXDeepFM
    from tests.test_infer_autoint_host import _model as _autoint_model
    assert type(_autoint_model().inference_plan()) is fused.InferAutoInt
    assert not fused.InferAFM.eligible(_autoint_model())
    for nets in (DEEPFM, DCN, ['dnn_nets'], ['linear', 'fm_nets']):
        assert not fused.InferAFM.eligible(_other_model(nets))
    assert _model().fused_plan() is None                 # the training side has no AFM plan


def test_building_the_plan_moves_nothing(rec):
    dm = _model(nets=['linear', 'fm_nets', 'afm_nets'])
    before = {n: p.data_ptr() for n, p in dm.model.named_parameters()}
    assert type(dm.inference_plan()).__name__ == 'InferAFM'
    assert {n: p.data_ptr() for n, p in dm.model.named_parameters()} == before
    assert getattr(dm.optimizer, '_flat', None) is None and not hasattr(dm, '_fused_plan')
