# -*- coding:utf-8 -*-
"""CPU: the inference plan for the FiBiNet graph (fused.InferFiBiNet, dt_fibi_infer*, csrc/fibi_infer.hip) — what the
library's predicate accepts, which graphs take the plan, which calls `predict` makes with which tensors.  The plans are built
on CPU models and their launches recorded by a stand-in for the library (tests/infer_support.Recorder): nothing runs on a
GPU."""
import ctypes
import os
import re

import numpy as np
import pandas as pd
import pytest

from tests.infer_support import install_recorder
from tests.test_infer_host import DEEPFM, DCN
from tests.test_infer_host import _model as _other_model

F_, D_, ND_ = 6, 16, 3
P_ = F_ * (F_ - 1) // 2
H1_, H2_ = 100, 40
FIBI_ENTRIES = ('dt_fibi_infer_prepare', 'dt_fibi_infer')
OTHER_ENTRIES = ('dt_deepfm_infer_prepare', 'dt_deepfm_infer', 'dt_dcn_infer_prepare', 'dt_dcn_infer',
                 'dt_stack_infer_prepare', 'dt_stack_infer', 'dt_xdeepfm_infer_prepare', 'dt_xdeepfm_infer_tower',
                 'dt_xdeepfm_infer_cin', 'dt_xdeepfm_infer_head', 'dt_autoint_infer_prepare', 'dt_autoint_infer',
                 'dt_afm_infer_prepare', 'dt_afm_infer', 'dt_pnn_infer_prepare', 'dt_pnn_infer')
INTERACTION, EACH, ALL = 0, 1, 2
MEAN, MAX = 0, 1
TYPES = {'field_interaction': INTERACTION, 'field_each': EACH, 'field_all': ALL}
GRAPHS = [(t, p) for t in TYPES for p in ('mean', 'max')]


@pytest.fixture
def rec(monkeypatch):
    return install_recorder(monkeypatch, FIBI_ENTRIES + OTHER_ENTRIES,
                            ('DT_AMD_FUSED', 'DT_AMD_FUSED_PREDICT', 'DT_AMD_TOWER_DTYPE'))


def _model(nets=('fibi_dnn_nets',), task='binary', D=D_, F=F_, bilinear_type='field_interaction', pool='mean', ratio=3,
           hidden=((H1_, 0, False), (H2_, 0, False)), activation='relu', mfma_dtype=None, **extra):
    from deeptables_amd.models import ModelConfig, DeepModel
    from deeptables_amd.models.metainfo import CategoricalColumn, ContinuousColumn
    dnn = {'hidden_units': hidden, 'activation': activation}
    if mfma_dtype:
        dnn['mfma_dtype'] = mfma_dtype
    conf = ModelConfig(nets=list(nets), fixed_embedding_dim=True, embeddings_output_dim=D,
                       fibinet_params={'senet_pooling_op': pool, 'senet_reduction_ratio': ratio, 'bilinear_type': bilinear_type},
                       dnn_params=dnn, **{'embedding_dropout': 0, **extra})
    dm = DeepModel(task, 2 if task != 'multiclass' else 3, conf, [CategoricalColumn(f'C{i}', 20 + i, D) for i in range(F)],
                   [ContinuousColumn('input_continuous_all', ['a', 'b', 'c'])])
    dm.build('cpu')
    return dm


def _frame(n, seed=0, F=F_):
    g = np.random.default_rng(seed)
    df = pd.DataFrame({f'C{i}': g.integers(0, 20, n) for i in range(F)})
    for k in ('a', 'b', 'c'):
        df[k] = g.standard_normal(n).astype(np.float32)
    return df


def _fibi_layers(dm):
    L = dm.model.layers_by_name
    one = lambda prefix: [l for n, l in L.items() if n.startswith(prefix) and n[len(prefix):].isdigit()]
    (se,), (bs,), (br,) = one('senet_layer_'), one('senet_bilinear_layer_'), one('embedding_bilinear_layer_')
    return se, bs, br


# ---- the library's predicates (no launch) ---------------------------------------------------------------------------------
def test_the_codes_are_the_headers():
    from deeptables_amd import _lib, ops
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'dt_hip.h')).read()
    defines = {k: int(v, 0) for k, v in re.findall(r'#define (DT_(?:BILINEAR|FIBI)_\w+) (\w+)', header)}
    assert defines == {'DT_BILINEAR_FIELD_INTERACTION': _lib.DT_BILINEAR_FIELD_INTERACTION,
                       'DT_BILINEAR_FIELD_EACH': _lib.DT_BILINEAR_FIELD_EACH, 'DT_BILINEAR_FIELD_ALL': _lib.DT_BILINEAR_FIELD_ALL,
                       'DT_FIBI_POOL_MEAN': _lib.DT_FIBI_POOL_MEAN, 'DT_FIBI_POOL_MAX': _lib.DT_FIBI_POOL_MAX,
                       'DT_FIBI_INFER_MAX_BLOCKS': _lib.DT_FIBI_INFER_MAX_BLOCKS}
    assert ops.BILINEAR_TYPES == {'field_interaction': _lib.DT_BILINEAR_FIELD_INTERACTION,
                                  'field_each': _lib.DT_BILINEAR_FIELD_EACH, 'field_all': _lib.DT_BILINEAR_FIELD_ALL} == TYPES
    assert (_lib.DT_FIBI_POOL_MEAN, _lib.DT_FIBI_POOL_MAX) == (MEAN, MAX)


def test_predicate_at_and_just_beyond_each_limit():
    from deeptables_amd import _lib
    ok = _lib.lib().dt_fibi_infer_supported           # (F, D, Nd, H1, H2, cells, bilinear_type, pooling_op, R)
    t = (128, 64, 0, INTERACTION, MEAN, 1)
    # 2 <= F <= 64
    assert ok(1, 8, 1, *t) == 0 and ok(2, 8, 1, *t) == 1 and ok(64, 8, 1, *t) == 1 and ok(65, 8, 1, *t) == 0
    assert ok(65, 4, 1, *t) == 0                       # F = 65 with F D = 260
    # the embedding sizes
    assert ok(2, 2, 1, *t) == 0 and ok(2, 4, 1, *t) == 1 and ok(2, 64, 1, *t) == 1 and ok(2, 128, 1, *t) == 0
    for D in (8, 16, 32):
        assert ok(4, D, 5, *t) == 1, D
    for D in (0, 12, 20):
        assert ok(2, D, 1, *t) == 0, D
    # F D <= 512
    assert ok(32, 16, 1, *t) == 1 and ok(36, 16, 1, *t) == 0          # 512 / 576
    assert ok(8, 64, 1, *t) == 1 and ok(9, 64, 1, *t) == 0            # 512 / 576
    # 1 <= Nd <= 64: the net concatenates the dense input unconditionally
    assert ok(26, 16, 0, *t) == 0 and ok(26, 16, 1, *t) == 1 and ok(26, 16, 64, *t) == 1 and ok(26, 16, 65, *t) == 0
    # R >= 1
    assert ok(26, 16, 13, 128, 64, 0, INTERACTION, MEAN, 0) == 0 and ok(26, 16, 13, 128, 64, 0, INTERACTION, MEAN, 1) == 1
    assert ok(26, 16, 13, 128, 64, 0, INTERACTION, MEAN, 8) == 1
    # the tower of _infer_tower
    for h1, h2, cells, want in ((128, 64, 3, 1), (1, 1, 0, 1), (100, 40, 2, 1), (129, 64, 0, 0), (128, 65, 0, 0), (0, 64, 0, 0),
                                (128, 0, 0, 0), (128, 64, 4, 0), (128, 64, -1, 0)):
        assert ok(26, 16, 13, h1, h2, cells, INTERACTION, MEAN, 8) == want, (h1, h2, cells)
    # the codes
    for bt, want in ((INTERACTION, 1), (EACH, 1), (ALL, 1), (3, 0), (-1, 0)):
        assert ok(26, 16, 13, 128, 64, 0, bt, MAX, 8) == want, bt
    for pool, want in ((MEAN, 1), (MAX, 1), (2, 0), (-1, 0)):
        assert ok(26, 16, 13, 128, 64, 0, EACH, pool, 8) == want, pool


def test_workspace_bytes_follow_the_shape_predicate():
    from deeptables_amd import _lib
    lib = _lib.lib()
    wsb, ok = lib.dt_fibi_infer_workspace_bytes, lib.dt_fibi_infer_supported
    for F, D, Nd, bt, R in ((1, 8, 1, 0, 1), (2, 8, 1, 0, 1), (64, 8, 1, 0, 21), (65, 8, 1, 0, 21), (2, 2, 1, 0, 1), (2, 4, 1, 0, 1),
                            (2, 64, 1, 0, 1), (2, 128, 1, 0, 1), (32, 16, 1, 1, 10), (36, 16, 1, 1, 12), (26, 16, 0, 2, 8),
                            (26, 16, 1, 2, 8), (26, 16, 64, 2, 8), (26, 16, 65, 2, 8), (26, 16, 13, 0, 0), (26, 16, 13, 0, 1),
                            (26, 16, 13, 3, 8), (26, 16, 13, -1, 8), (26, 16, 13, 0, 8), (26, 16, 13, 1, 8)):
        n = wsb(F, D, Nd, bt, R)
        good = ok(F, D, Nd, 128, 64, 0, bt, MEAN, R) == 1
        assert (n == -1) == (not good), (F, D, Nd, bt, R)
        if good:
            K = F * (F - 1) * D + Nd
            KP = -(-K // 128) * 128
            nw = (F * (F - 1) // 2, F - 1, 1)[bt]
            assert n >= 6 * KP * 128 + 2 * 4 * nw * D * D and n % 16 == 0          # the W1 layout and the two bilinear stacks
    assert wsb(26, 16, 13, 0, 8) > 8 * 2 ** 20 > wsb(26, 16, 13, 2, 8) > 10413 * 128 * 6
    assert 24 * 2 ** 20 < wsb(64, 8, 1, 0, 21) < 27 * 2 ** 20
    assert wsb(26, 16, 13, 0, 8) > wsb(26, 16, 13, 1, 8) > wsb(26, 16, 13, 2, 8)


def test_entry_points_check_their_arguments_before_any_launch():
    from deeptables_amd import _lib
    lib = _lib.lib()
    none = [None, 1, None, None, None, None]            # idx, idx_kind, table, row_offset, vocab, dense
    tail = [None, None, None, None]                     # workspace, logit_out, out, oob_count
    shape = (26, 16, 13, INTERACTION, MEAN, 8)
    assert lib.dt_fibi_infer(*none, 0, *shape, *tail, 3, None) == 0                         # an empty batch, every pointer null
    assert lib.dt_fibi_infer(*none, 5, *shape, *tail, 1, None) != 0                         # null pointers with rows to score
    assert b'dt_fibi_infer' in lib.dt_last_error()
    assert lib.dt_fibi_infer(*none, -1, *shape, *tail, 0, None) != 0                        # a negative batch
    assert lib.dt_fibi_infer(*none, 1 << 31, *shape, *tail, 0, None) != 0
    assert lib.dt_fibi_infer(None, 7, None, None, None, None, 0, *shape, *tail, 0, None) != 0      # a bad idx_kind
    assert lib.dt_fibi_infer(*none, 0, *shape, *tail, 0x4, None) != 0                       # an unknown flag
    assert lib.dt_fibi_infer(*none, 0, 1, 16, 13, INTERACTION, MEAN, 8, *tail, 0, None) != 0        # one field
    assert lib.dt_fibi_infer(*none, 0, 26, 16, 0, INTERACTION, MEAN, 8, *tail, 0, None) != 0        # no dense input
    assert lib.dt_fibi_infer(*none, 0, 26, 16, 13, 3, MEAN, 8, *tail, 0, None) != 0                 # an unknown bilinear type
    assert lib.dt_fibi_infer(*none, 0, 26, 16, 13, ALL, 2, 8, *tail, 0, None) != 0                  # an unknown pooling op
    assert lib.dt_fibi_infer(*none, 0, 26, 16, 13, ALL, MAX, 0, *tail, 0, None) != 0                # R = 0

    def prepare(F=26, D=16, Nd=13, bt=INTERACTION, R=8, H1=128, H2=64, cells=0):
        return lib.dt_fibi_infer_prepare(F, D, Nd, bt, R, *([None] * 6), None, 128, H1, None, None, 64, H2, None, cells,
                                         *([None] * 4), 0.0, *([None] * 4), 0.0, None, None, None, None)
    assert prepare() != 0
    assert b'dt_fibi_infer_prepare' in lib.dt_last_error()
    assert prepare(H1=129) != 0 and prepare(F=65, D=8) != 0 and prepare(bt=3) != 0 and prepare(R=0) != 0


# ---- routing ------------------------------------------------------------------------------------------------------------
def _names(dm, plan):
    """data_ptr -> name of every tensor a dt_fibi_infer_prepare call may point to"""
    import torch
    named = {}
    for lname, layer in dm.model.layers_by_name.items():
        for attr in ('kernel', 'bias', 'gamma', 'beta', 'moving_mean', 'moving_variance', 'W'):
            t = getattr(layer, attr, None)
            if isinstance(t, torch.Tensor):
                named[t.data_ptr()] = f'{lname}.{attr}'
    se, _, _ = _fibi_layers(dm)
    for sub in ('dense_att1', 'dense_att2'):
        for attr in ('kernel', 'bias'):
            named[getattr(getattr(se, sub), attr).data_ptr()] = f'{sub}.{attr}'
    named[plan.ws.data_ptr()] = 'ws'
    return named


def _decode(args, names):
    return [names.get(a.value, f'?{a.value:#x}') if isinstance(a, ctypes.c_void_p) else a for a in args]


def _expected_prepare(dm, bt, R, ld1, ld2):
    L = dm.model.layers_by_name
    se, bs, br = _fibi_layers(dm)
    d1, d2 = L['fibi_dnn_dense_1'], L['fibi_dnn_dense_2']

    def nm(layer, attr):
        return f'{layer.name}.{attr}' if getattr(layer, attr, None) is not None else None

    head = [F_, D_, ND_, bt, R, 'dense_att1.kernel', 'dense_att1.bias', 'dense_att2.kernel', 'dense_att2.bias',
            f'{bs.name}.W', f'{br.name}.W']
    mid = [nm(d1, 'kernel'), ld1, d1.kernel.shape[1], nm(d1, 'bias'), nm(d2, 'kernel'), ld2, d2.kernel.shape[1], nm(d2, 'bias')]
    bits, cellargs = 0, []
    for i in (1, 2):
        b = L.get(f'fibi_dnn_bn_{i}')
        if b is None:
            cellargs += [None, None, None, None, 0.0]
        else:
            bits |= 1 << (i - 1)
            cellargs += [nm(b, 'gamma'), nm(b, 'beta'), nm(b, 'moving_mean'), nm(b, 'moving_variance'), float(b.epsilon)]
    return head + mid + [bits] + cellargs + ['task_output.kernel', nm(L['task_output'], 'bias'), 'ws', None]


@pytest.mark.parametrize('k', range(len(GRAPHS)))
def test_each_graph_takes_the_plan_and_predict_makes_its_calls(rec, k):
    """prepare once per call, one launch per batch and no other library call; the pointers are the layers' own tensors —
    SENET's four, the two bilinear stacks, W1 with its leading dimension, task_output's [H2, 1] kernel as w3; no input
    BatchNormalization is named anywhere (the graph has none: the dense values enter the tower raw)"""
    from deeptables_amd import _lib, fused
    bilinear_type, pool = GRAPHS[k]
    task = 'regression' if k % 2 else 'binary'
    bias = k not in (2, 5)
    hidden = ((H1_, 0, k == 1), (H2_, 0.3, k in (1, 4))) if k in (1, 4) else ((H1_, 0, False), (H2_, 0, False))
    ratio = (3, 1, 20)[k % 3]
    R = max(F_ // ratio, 1)
    dm = _model(task=task, bilinear_type=bilinear_type, pool=pool, ratio=ratio, output_use_bias=bias, hidden=hidden)
    plan = dm.inference_plan()
    bt, pc = TYPES[bilinear_type], MAX if pool == 'max' else MEAN
    assert type(plan) is fused.InferFiBiNet and (plan.bt, plan.pool, plan.R) == (bt, pc, R)
    assert (plan.F, plan.D, plan.Nd) == (F_, D_, ND_)
    assert rec.names() == [] and not hasattr(dm, '_fused_plan')
    L = dm.model.layers_by_name
    se, bs, br = _fibi_layers(dm)
    nw = (P_, F_ - 1, 1)[bt]
    assert tuple(L['task_output'].kernel.shape) == (H2_, 1) and 'dense_logit_fibi_dnn_nets' not in L
    assert tuple(L['fibi_dnn_dense_1'].kernel.shape) == (2 * P_ * D_ + ND_, H1_)
    assert tuple(bs.W.shape) == tuple(br.W.shape) == (nw, D_, D_) and bs.W.data_ptr() != br.W.data_ptr()
    assert tuple(se.dense_att1.kernel.shape) == (F_, R) and tuple(se.dense_att2.kernel.shape) == (R, F_)
    n, b = 20, 8
    out = dm.predict(_frame(n), batch_size=b)
    assert out.shape == (n, 1) and out.dtype == np.float32
    assert rec.names() == ['dt_fibi_infer_prepare'] + ['dt_fibi_infer'] * 3
    names = _names(dm, plan)
    pa = rec.calls[0][1]
    assert len(pa) == 34
    decoded = _decode(pa, names)
    assert decoded == _expected_prepare(dm, bt, R, H1_, H2_)
    assert not any(isinstance(v, str) and v.startswith('bn_concat') for v in decoded)
    assert (L['task_output'].bias is None) == (not bias)
    assert plan.ws.numel() * 4 == _lib.lib().dt_fibi_infer_workspace_bytes(F_, D_, ND_, bt, R)
    emb = L['emb_categorical_vars_all']
    done, lg0, out0 = 0, None, None
    for i in range(3):
        a = rec.calls[1 + i][1]
        assert len(a) == 19 and a[1] in (_lib.DT_IDX_F32, _lib.DT_IDX_I32)
        assert a[2].value == emb.tables[plan.key].data_ptr()
        assert a[3].value == getattr(emb, f'row_offset_{plan.key}').data_ptr()
        assert a[4].value == getattr(emb, f'vocab_{plan.key}').data_ptr()
        assert a[5] is not None                                   # dense [B][Nd]
        assert a[6] == (8, 8, 4)[i] and a[7:13] == (F_, D_, ND_, bt, pc, R)
        assert a[13].value == plan.ws.data_ptr() and a[16] is None
        assert a[17] == (_lib.DT_INFER_SIGMOID if task == 'binary' else 0) and a[18] is None
        if i == 0:
            lg0, out0 = a[14].value, a[15].value
        assert a[14].value == lg0 + 4 * done and a[15].value == out0 + 4 * done
        done += a[6]
    assert done == n


def test_the_tower_mode_and_the_layer_codes_are_read_in_prepare(rec):
    from deeptables_amd import _lib
    dm = _model(bilinear_type='field_all', mfma_dtype='bf16')
    dm.predict(_frame(10), batch_size=16)
    assert rec.names() == ['dt_fibi_infer_prepare', 'dt_fibi_infer']
    assert rec.calls[1][1][17] == _lib.DT_INFER_SIGMOID | _lib.DT_INFER_TOWER_BF16
    assert rec.calls[0][1][3] == ALL and rec.calls[1][1][10:12] == (ALL, MEAN)
    dm.config.dnn_params['mfma_dtype'] = 'f32'           # read in prepare: the six-product forward serves the f32 mode too
    se, _, _ = _fibi_layers(dm)
    se.pooling_op = 'max'
    rec.calls.clear()
    dm.predict(_frame(10), batch_size=16)
    assert rec.calls[1][1][17] == _lib.DT_INFER_SIGMOID and rec.calls[1][1][10:12] == (ALL, MAX)


def test_prepare_reads_the_tensors_at_call_time(rec):
    """the plan caches no parameter: a tensor re-homed between two predicts is the one the second prepare names"""
    import torch
    dm = _model()
    dm.predict(_frame(10), batch_size=16)
    L = dm.model.layers_by_name
    se, bs, br = _fibi_layers(dm)
    d1 = L['fibi_dnn_dense_1']
    a0 = rec.calls[0][1]
    assert a0[9].value == bs.W.data_ptr() and a0[10].value == br.W.data_ptr()
    assert a0[11].value == d1.kernel.data_ptr() and a0[12] == H1_
    slab = torch.zeros(d1.kernel.shape[0], 128)
    slab[:, :H1_] = d1.kernel.data
    d1.kernel.data = slab[:, :H1_]
    br.W.data = torch.clone(br.W.data) * 2
    se.dense_att2.kernel.data = torch.clone(se.dense_att2.kernel.data)
    rec.calls.clear()
    dm.predict(_frame(10), batch_size=16)
    assert rec.names() == ['dt_fibi_infer_prepare', 'dt_fibi_infer']
    a1 = rec.calls[0][1]
    assert a1[10].value == br.W.data_ptr() != a0[10].value and a1[9].value == a0[9].value
    assert a1[7].value == se.dense_att2.kernel.data_ptr() != a0[7].value
    assert a1[11].value == slab.data_ptr() != a0[11].value and a1[12] == 128 and a1[13] == H1_


REFUSED = ['with_linear', 'with_dnn', 'fibi_nets', 'concat', 'multiclass', 'tanh_tower', 'three_cells', 'H1_129', 'H2_65',
           'sharded', 'fused_off', 'predict_off', 'D12', 'FD576', 'output_kernel', 'two_senet_layers']


@pytest.mark.parametrize('case', REFUSED)
def test_graphs_and_switches_refused(rec, monkeypatch, case):
    import torch
    from deeptables_amd import _lib, fused
    kw = {}
    if case == 'with_linear':
        kw['nets'] = ['linear', 'fibi_dnn_nets']
    elif case == 'with_dnn':
        kw['nets'] = ['fibi_dnn_nets', 'dnn_nets']
    elif case == 'fibi_nets':
        kw['nets'] = ['fibi_nets']
    elif case == 'concat':
        kw['stacking_op'] = 'concat'
    elif case == 'multiclass':
        kw['task'] = 'multiclass'
    elif case == 'tanh_tower':
        kw['activation'] = 'tanh'
    elif case == 'three_cells':
        kw['hidden'] = ((64, 0, False), (32, 0, False), (16, 0, False))
    elif case == 'H1_129':
        kw['hidden'] = ((129, 0, False), (64, 0, False))
    elif case == 'H2_65':
        kw['hidden'] = ((128, 0, False), (65, 0, False))
    elif case == 'D12':
        kw['D'] = 12
    elif case == 'FD576':
        kw.update(F=9, D=64)
    dm = _model(**kw)
    if case == 'predict_off':
        monkeypatch.setenv('DT_AMD_FUSED_PREDICT', '0')
    elif case == 'fused_off':
        monkeypatch.setenv('DT_AMD_FUSED', '0')
    elif case == 'output_kernel':
        dm.model.layers_by_name['task_output'].kernel.data = torch.zeros(H2_ + 1, 1)
    elif case == 'two_senet_layers':
        from deeptables_amd.models import layers
        dm.model.layers_by_name['senet_layer_99'] = layers.SENET(name='senet_layer_99')
    elif case == 'sharded':
        class _Sharded:
            sharded_embeddings, active, world_size = True, True, 1
        dm.config = dm.config._replace(distribute_strategy=_Sharded())
    assert fused.make_inference_plan(dm) is None
    assert not (case not in ('predict_off', 'fused_off') and fused.InferFiBiNet.eligible(dm))
    if case in ('output_kernel', 'two_senet_layers'):
        return                                   # (the model was tampered with: the layer path is not run)
    with pytest.raises(_lib.DtHipError, match='GPU only'):        # the layer path runs: its first kernel refuses CPU tensors
        dm.predict(_frame(20, F=kw.get('F', F_)), batch_size=8)
    assert rec.names() == []


@pytest.mark.parametrize('case', ['var_len_column', 'two_embedding_groups'])
def test_var_len_columns_and_several_embedding_groups_are_refused(rec, case):
    from deeptables_amd import _lib, fused
    from deeptables_amd.models import ModelConfig, DeepModel
    from deeptables_amd.models.metainfo import CategoricalColumn, ContinuousColumn, VarLenCategoricalColumn
    dnn = {'hidden_units': ((H1_, 0, False), (H2_, 0, False)), 'activation': 'relu'}
    conts = [ContinuousColumn('input_continuous_all', ['a', 'b', 'c'])]
    if case == 'var_len_column':
        conf = ModelConfig(nets=['fibi_dnn_nets'], fixed_embedding_dim=True, embeddings_output_dim=D_, embedding_dropout=0,
                           dnn_params=dnn)
        vl = VarLenCategoricalColumn('g', 12, D_)
        vl.max_elements_length = 5
        dm = DeepModel('binary', 2, conf, [CategoricalColumn(f'C{i}', 20 + i, D_) for i in range(F_)], conts,
                       var_categorical_len_columns=[vl])
    else:
        conf = ModelConfig(nets=['fibi_dnn_nets'], fixed_embedding_dim=False, embedding_dropout=0, dnn_params=dnn)
        dm = DeepModel('binary', 2, conf, [CategoricalColumn(f'C{i}', 20 + i, 16 if i < 3 else 8) for i in range(F_)], conts)
    dm.build('cpu')
    L = dm.model.layers_by_name
    se, bs, br = _fibi_layers(dm)
    assert type(se).__name__ == 'SENET' and type(bs).__name__ == type(br).__name__ == 'BilinearInteraction'
    assert 'fibi_dnn_dense_1' in L and 'fibi_dnn_dense_2' in L
    if case == 'var_len_column':
        assert dm.var_len_categorical_columns and 'emb_g' in L
    else:
        assert len(L['emb_categorical_vars_all'].groups) == 2
    assert fused.make_inference_plan(dm) is None and dm.inference_plan() is None
    assert not fused.InferFiBiNet.eligible(dm)
    if case == 'two_embedding_groups':
        with pytest.raises(_lib.DtHipError, match='GPU only'):    # the layer path runs: its first kernel refuses CPU tensors
            dm.predict(_frame(20), batch_size=8)
    assert rec.names() == []


def test_the_other_graphs_keep_their_plans(rec):
    from deeptables_amd import fused
    assert type(_other_model(DEEPFM).inference_plan()) is fused.InferDeepFM
    assert type(_other_model(DCN).inference_plan()) is fused.InferDCN
    assert type(_other_model(['dnn_nets']).inference_plan()) is fused.InferStack
    assert type(_other_model(['linear', 'fm_nets']).inference_plan()) is fused.InferStack
    from tests.test_infer_afm_host import _model as _afm_model
    from tests.test_infer_pnn_host import _model as _pnn_model
    from tests.test_infer_autoint_host import _model as _autoint_model
    from tests.test_infer_xdeepfm_host import XDEEPFM
    assert type(_afm_model().inference_plan()) is fused.InferAFM
    assert type(_pnn_model().inference_plan()) is fused.InferPNN
    assert type(_autoint_model().inference_plan()) is fused.InferAutoInt
    assert type(_other_model(XDEEPFM).inference_plan()) is fused.InferXDeepFM
    for nets in (DEEPFM, DCN, ['dnn_nets'], ['linear', 'fm_nets']):
        assert not fused.InferFiBiNet.eligible(_other_model(nets))
    assert not fused.InferFiBiNet.eligible(_afm_model()) and not fused.InferFiBiNet.eligible(_pnn_model())
    assert _model().fused_plan() is None                 # the training side has no FiBiNet plan


def test_building_the_plan_moves_nothing(rec):
    dm = _model()
    before = {n: p.data_ptr() for n, p in dm.model.named_parameters()}
    assert type(dm.inference_plan()).__name__ == 'InferFiBiNet'
    assert {n: p.data_ptr() for n, p in dm.model.named_parameters()} == before
    assert getattr(dm.optimizer, '_flat', None) is None and not hasattr(dm, '_fused_plan')
