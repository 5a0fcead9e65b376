# -*- coding:utf-8 -*-
"""CPU: the inference plan for the product nets (fused.InferPNN, dt_pnn_infer*, csrc/pnn_infer.hip) — what the library's
predicate accepts, which graphs take the plan, which calls `predict` / `evaluate` / fit's validation pass make with which
tensors.  The plans are built on CPU models and their launches recorded by a stand-in for the library (the recorder of
tests/test_infer_afm_host.py, restated for the dt_pnn_infer* names): nothing runs on a GPU."""
import numpy as np
import pandas as pd
import pytest

from tests.infer_support import install_recorder
from tests.test_infer_host import DEEPFM, DCN, _decode, _names
from tests.test_infer_host import _model as _other_model

F_, D_, ND_ = 6, 16, 3
P_ = F_ * (F_ - 1) // 2
H1_, H2_ = 100, 40
PNN_ENTRIES = ('dt_pnn_infer_prepare', 'dt_pnn_infer')
OTHER_ENTRIES = ('dt_deepfm_infer_prepare', 'dt_deepfm_infer', 'dt_dcn_infer_prepare', 'dt_dcn_infer',
                 'dt_stack_infer_prepare', 'dt_stack_infer', 'dt_xdeepfm_infer_prepare', 'dt_xdeepfm_infer_tower',
                 'dt_xdeepfm_infer_cin', 'dt_xdeepfm_infer_head', 'dt_autoint_infer_prepare', 'dt_autoint_infer',
                 'dt_afm_infer_prepare', 'dt_afm_infer')
INNER, OUTER = 0x1, 0x2
MAT, VEC, NUM = 0, 1, 2
# net -> (the tower's cell prefix, product mask, inner layer, outer layer)
NETS = {'pnn_nets': ('pnn', INNER | OUTER, 'pnn_inner_product_layer', 'pnn_outer_product_layer'),
        'ipnn_nets': ('ipnn', INNER, 'inner_product_layer', None),
        'opnn_nets': ('opnn', OUTER, None, 'outer_product_layer')}
GRAPHS = [('pnn_nets', 'mat'), ('pnn_nets', 'vec'), ('pnn_nets', 'num'), ('ipnn_nets', 'mat'), ('opnn_nets', 'mat'),
          ('opnn_nets', 'vec'), ('opnn_nets', 'num')]


@pytest.fixture
def rec(monkeypatch):
    return install_recorder(monkeypatch, PNN_ENTRIES + OTHER_ENTRIES,
                            ('DT_AMD_FUSED', 'DT_AMD_FUSED_PREDICT', 'DT_AMD_TOWER_DTYPE'))


def _model(nets=('pnn_nets',), task='binary', D=D_, F=F_, kernel_type='mat', hidden=((H1_, 0, False), (H2_, 0, False)),
           activation='relu', mfma_dtype=None, **extra):
    from deeptables_amd.models import ModelConfig, DeepModel
    from deeptables_amd.models.metainfo import CategoricalColumn, ContinuousColumn
    dnn = {'hidden_units': hidden, 'activation': activation}
    if mfma_dtype:
        dnn['mfma_dtype'] = mfma_dtype
    conf = ModelConfig(nets=list(nets), fixed_embedding_dim=True, embeddings_output_dim=D,
                       pnn_params={'outer_product_kernel_type': kernel_type}, dnn_params=dnn,
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


# ---- the library's predicates (no launch) ---------------------------------------------------------------------------------
def test_the_codes_are_the_headers():
    import os
    import re
    from deeptables_amd import _lib
    assert (_lib.DT_PNN_INNER, _lib.DT_PNN_OUTER) == (INNER, OUTER)
    assert _lib.DT_OP_KERNEL == {'mat': MAT, 'vec': VEC, 'num': NUM}
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'dt_hip.h')).read()
    defines = {k: int(v, 0) for k, v in re.findall(r'#define (DT_PNN_\w+) (\w+)', header)}
    assert defines == {'DT_PNN_INNER': _lib.DT_PNN_INNER, 'DT_PNN_OUTER': _lib.DT_PNN_OUTER,
                       'DT_PNN_INFER_MAX_BLOCKS': _lib.DT_PNN_INFER_MAX_BLOCKS}


def test_predicate_at_and_just_beyond_each_limit():
    from deeptables_amd import _lib
    lib = _lib.lib()
    ok = lib.dt_pnn_infer_supported
    both = INNER | OUTER
    # 2 <= F <= 64
    assert ok(1, 8, 0, 128, 64, 0, both, MAT) == 0 and ok(2, 8, 0, 128, 64, 0, both, MAT) == 1
    assert ok(64, 8, 0, 128, 64, 0, both, MAT) == 1 and ok(65, 8, 0, 128, 64, 0, both, MAT) == 0
    assert ok(65, 4, 0, 128, 64, 0, both, MAT) == 0          # F = 65 with F D = 260
    # F D <= 512
    assert ok(64, 8, 0, 128, 64, 0, INNER, 0) == 1 and ok(65, 8, 0, 128, 64, 0, INNER, 0) == 0        # 512 / 520
    assert ok(32, 16, 0, 128, 64, 0, both, VEC) == 1 and ok(33, 16, 0, 128, 64, 0, both, VEC) == 0
    assert ok(8, 64, 0, 128, 64, 0, OUTER, MAT) == 1 and ok(9, 64, 0, 128, 64, 0, OUTER, MAT) == 0
    # the embedding sizes
    for D in (4, 8, 16, 32, 64):
        assert ok(4, D, 5, 128, 64, 0, both, MAT) == 1, D
    for D in (0, 2, 12, 20, 128):
        assert ok(2, D, 0, 128, 64, 0, both, MAT) == 0, D
    # Nd <= 64
    assert ok(26, 16, 64, 128, 64, 0, both, MAT) == 1 and ok(26, 16, 65, 128, 64, 0, both, MAT) == 0
    assert ok(26, 16, -1, 128, 64, 0, both, MAT) == 0
    # the tower of _infer_tower
    for h1, h2, cells, want in ((128, 64, 3, 1), (1, 1, 0, 1), (100, 40, 2, 1), (129, 64, 0, 0), (128, 65, 0, 0), (0, 64, 0, 0),
                                (128, 0, 0, 0), (128, 64, 4, 0), (128, 64, -1, 0)):
        assert ok(26, 16, 13, h1, h2, cells, both, MAT) == want, (h1, h2, cells)
    # the product mask; the kernel type, ignored without an outer layer
    for products, want in ((0, 0), (INNER, 1), (OUTER, 1), (both, 1), (4, 0), (both | 4, 0), (-1, 0)):
        assert ok(26, 16, 13, 128, 64, 0, products, MAT) == want, products
    for kt, want in ((MAT, 1), (VEC, 1), (NUM, 1), (3, 0), (-1, 0)):
        assert ok(26, 16, 13, 128, 64, 0, both, kt) == want and ok(26, 16, 13, 128, 64, 0, OUTER, kt) == want, kt
        assert ok(26, 16, 13, 128, 64, 0, INNER, kt) == 1, kt
    # the workspace: stamp [4] | W1 3 x [KP][128] bf16 | W2 3 x [128][64] bf16 | BN 3 x [F D + Nd -> 4] | cell 1 [3][128] |
    # cell 2 [3][64] | w3 [64] | head [4] | the outer kernel; KP = the first Dense's rows rounded up to 128
    wsb = lib.dt_pnn_infer_workspace_bytes
    fixed = 4 + 3 * 128 * 64 // 2 + 3 * 128 + 3 * 64 + 64 + 4
    assert wsb(26, 16, 13, both, MAT) == 4 * (fixed + 3 * 1152 * 64 + 3 * 432 + 325 * 256)
    assert wsb(26, 16, 13, both, VEC) == 4 * (fixed + 3 * 1152 * 64 + 3 * 432 + 325 * 16)
    assert wsb(26, 16, 13, OUTER, NUM) == 4 * (fixed + 3 * 768 * 64 + 3 * 432 + 328)
    assert wsb(26, 16, 13, INNER, MAT) == wsb(26, 16, 13, INNER, 7) == 4 * (fixed + 3 * 768 * 64 + 3 * 432)
    assert wsb(2, 4, 0, INNER, 0) == 4 * (fixed + 3 * 128 * 64 + 3 * 8)
    for bad in ((1, 16, 0, both, MAT), (65, 8, 0, both, MAT), (26, 12, 0, both, MAT), (26, 16, 65, both, MAT),
                (26, 16, 0, 0, MAT), (26, 16, 0, both, 3), (33, 16, 0, INNER, 0)):
        assert wsb(*bad) == -1, bad


def test_entry_points_check_their_arguments_before_any_launch():
    from deeptables_amd import _lib
    lib = _lib.lib()
    none = [None, 1, None, None, None, None]            # idx, idx_kind, table, row_offset, vocab, dense
    tail = [None, None, None, None]                     # workspace, logit_out, out, oob_count
    both = INNER | OUTER
    assert lib.dt_pnn_infer(*none, 0, 26, 16, 13, both, MAT, *tail, 3, None) == 0               # an empty batch
    assert lib.dt_pnn_infer(*none, 5, 26, 16, 13, both, MAT, *tail, 1, None) != 0
    assert b'dt_pnn_infer' in lib.dt_last_error()
    assert lib.dt_pnn_infer(*none, 0, 1, 16, 13, both, MAT, *tail, 0, None) != 0                # one field
    assert lib.dt_pnn_infer(*none, 0, 26, 16, 13, 0, MAT, *tail, 0, None) != 0                  # no product layer
    assert lib.dt_pnn_infer(*none, 0, 26, 16, 13, both, 3, *tail, 0, None) != 0                 # an unknown kernel type
    assert lib.dt_pnn_infer(*none, 0, 26, 16, 13, both, MAT, *tail, 0x4, None) != 0             # an unknown flag
    assert lib.dt_pnn_infer(None, 7, None, None, None, None, 0, 26, 16, 13, both, MAT, *tail, 0, None) != 0
    assert lib.dt_pnn_infer(*none, 1 << 31, 26, 16, 13, both, MAT, *tail, 0, None) != 0
    assert lib.dt_pnn_infer(*none, -1, 26, 16, 13, both, MAT, *tail, 0, None) != 0

    def prepare(F=26, D=16, Nd=13, products=both, kt=MAT, H1=128, H2=64, cells=0):
        return lib.dt_pnn_infer_prepare(F, D, Nd, products, kt, *([None] * 5), 1e-3, None, 128, H1, None, None, 64, H2, None,
                                        cells, *([None] * 4), 0.0, *([None] * 4), 0.0, None, None, None, None)
    assert prepare() != 0
    assert b'dt_pnn_infer_prepare' in lib.dt_last_error()
    assert prepare(H1=129) != 0 and prepare(F=65, D=8) != 0 and prepare(products=0) != 0


# ---- routing ------------------------------------------------------------------------------------------------------------
def _expected_prepare(dm, net, kernel_type, ld1, ld2):
    """the decoded dt_pnn_infer_prepare arguments: the layers' current parameters by name"""
    cell, mask, _, outer = NETS[net]
    L = dm.model.layers_by_name
    bn = L['bn_concat_emb_dense']
    d1, d2 = L[f'{cell}_dense_1'], L[f'{cell}_dense_2']

    def nm(layer, attr):
        return f'{layer.name}.{attr}' if getattr(layer, attr, None) is not None else None

    head = [F_, D_, ND_, mask, {'mat': MAT, 'vec': VEC, 'num': NUM}[kernel_type] if outer else 0,
            f'{outer}.kernel' if outer else None]
    mid = [nm(bn, 'gamma'), nm(bn, 'beta'), nm(bn, 'moving_mean'), nm(bn, 'moving_variance'), float(bn.epsilon),
           nm(d1, 'kernel'), ld1, d1.kernel.shape[1], nm(d1, 'bias'), nm(d2, 'kernel'), ld2, d2.kernel.shape[1], nm(d2, 'bias')]
    bits, cellargs = 0, []
    for i in (1, 2):
        b = L.get(f'{cell}_bn_{i}')
        if b is None:
            cellargs += [None, None, None, None, 0.0]
        else:
            bits |= 1 << (i - 1)
            cellargs += [nm(b, 'gamma'), nm(b, 'beta'), nm(b, 'moving_mean'), nm(b, 'moving_variance'), float(b.epsilon)]
    return head + mid + [bits] + cellargs + ['task_output.kernel', nm(L['task_output'], 'bias'), 'ws', None]


@pytest.mark.parametrize('k', range(len(GRAPHS)))
def test_each_graph_takes_the_plan_and_predict_makes_its_calls(rec, k):
    """prepare once per call, one launch per batch and no other library call; the pointers are the layers' own tensors — W1
    with its leading dimension, task_output's [H2, 1] kernel as w3"""
    from deeptables_amd import _lib, fused
    net, kernel_type = GRAPHS[k]
    cell, mask, inner, outer = NETS[net]
    task = 'regression' if k % 2 else 'binary'
    bias = k not in (2, 5)
    hidden = ((H1_, 0, k == 1), (H2_, 0.3, k in (1, 4))) if k in (1, 4) else ((H1_, 0, False), (H2_, 0, False))
    dm = _model(nets=[net], task=task, kernel_type=kernel_type, output_use_bias=bias, hidden=hidden)
    plan = dm.inference_plan()
    kt = _lib.DT_OP_KERNEL[kernel_type] if outer else 0
    assert type(plan) is fused.InferPNN and (plan.products, plan.kt, plan.CELL) == (mask, kt, cell)
    assert (plan.F, plan.D, plan.Nd) == (F_, D_, ND_)
    assert rec.names() == [] and not hasattr(dm, '_fused_plan')
    L = dm.model.layers_by_name
    rows = P_ * (bool(inner) + bool(outer)) + F_ * D_ + ND_
    assert tuple(L['task_output'].kernel.shape) == (H2_, 1) and f'dense_logit_{net}' not in L
    assert tuple(L[f'{cell}_dense_1'].kernel.shape) == (rows, H1_)
    assert (inner in L if inner else True) and (outer in L if outer else True)
    n, b = 33, 16
    out = dm.predict(_frame(n), batch_size=b)
    assert out.shape == (n, 1) and out.dtype == np.float32
    assert rec.names() == ['dt_pnn_infer_prepare'] + ['dt_pnn_infer'] * 3
    names = _names(dm)
    pa = rec.calls[0][1]
    assert len(pa) == 34
    assert _decode(pa, names) == _expected_prepare(dm, net, kernel_type, H1_, H2_)
    assert (L['task_output'].bias is None) == (not bias)
    assert plan.ws.numel() * 4 == _lib.lib().dt_pnn_infer_workspace_bytes(F_, D_, ND_, mask, kt)
    emb = L['emb_categorical_vars_all']
    done, lg0, out0 = 0, None, None
    for i in range(3):
        a = rec.calls[1 + i][1]
        assert len(a) == 18 and a[1] in (_lib.DT_IDX_F32, _lib.DT_IDX_I32)
        assert a[2].value == emb.tables[plan.key].data_ptr()
        assert a[3].value == getattr(emb, f'row_offset_{plan.key}').data_ptr()
        assert a[4].value == getattr(emb, f'vocab_{plan.key}').data_ptr()
        assert a[5] is not None                                   # dense [B][Nd]
        assert a[6] == (16, 16, 1)[i] and a[7:12] == (F_, D_, ND_, mask, kt)
        assert a[12].value == plan.ws.data_ptr() and a[15] is None
        assert a[16] == (_lib.DT_INFER_SIGMOID if task == 'binary' else 0) and a[17] is None
        if i == 0:
            lg0, out0 = a[13].value, a[14].value
        assert a[13].value == lg0 + 4 * done and a[14].value == out0 + 4 * done
        done += a[6]
    assert done == n


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
    assert rec.names() == ['dt_pnn_infer_prepare'] + ['dt_pnn_infer'] * 3
    assert abs(res['loss'] - float(np.log(2.0))) < 1e-6          # zero logits: BCE = log 2 in every batch
    rec.calls.clear()
    monkeypatch.setattr(type(dm), 'train_step', lambda self, ins, yb, wb=None: (torch.zeros(()), torch.zeros(ins[0].shape[0], 1)))
    n = 100
    y = (np.arange(n) % 2 == 0).astype(np.float32)
    dm.fit(_frame(n), y, batch_size=16, epochs=2, verbose=0, validation_split=0.2, steps_per_execution=1)
    assert rec.names() == (['dt_pnn_infer_prepare'] + ['dt_pnn_infer'] * 2) * 2


def test_the_tower_mode_reaches_the_launch(rec):
    from deeptables_amd import _lib
    dm = _model(nets=['opnn_nets'], kernel_type='vec', mfma_dtype='bf16')
    dm.predict(_frame(10), batch_size=16)
    assert rec.names() == ['dt_pnn_infer_prepare', 'dt_pnn_infer']
    assert rec.calls[1][1][16] == _lib.DT_INFER_SIGMOID | _lib.DT_INFER_TOWER_BF16
    dm.config.dnn_params['mfma_dtype'] = 'f32'           # read in prepare: the six-product forward serves the f32 mode too
    rec.calls.clear()
    dm.predict(_frame(10), batch_size=16)
    assert rec.calls[1][1][16] == _lib.DT_INFER_SIGMOID


def test_prepare_reads_the_tensors_at_call_time(rec):
    """the plan caches no parameter: `prepare` is called again on a later predict, and a kernel re-homed between the two calls
    is the one the second prepare names — here W1 as a strided view with another leading dimension"""
    import torch
    dm = _model()
    dm.predict(_frame(10), batch_size=16)
    L = dm.model.layers_by_name
    d1, op = L['pnn_dense_1'], L['pnn_outer_product_layer']
    a0 = rec.calls[0][1]
    assert a0[5].value == op.kernel.data_ptr() and a0[11].value == d1.kernel.data_ptr() and a0[12] == H1_
    slab = torch.zeros(d1.kernel.shape[0], 128)
    slab[:, :H1_] = d1.kernel.data
    d1.kernel.data = slab[:, :H1_]
    op.kernel.data = torch.clone(op.kernel.data) * 2
    rec.calls.clear()
    dm.predict(_frame(10), batch_size=16)
    assert rec.names() == ['dt_pnn_infer_prepare', 'dt_pnn_infer']
    a1 = rec.calls[0][1]
    assert a1[5].value == op.kernel.data_ptr() != a0[5].value
    assert a1[11].value == slab.data_ptr() != a0[11].value and a1[12] == 128 and a1[13] == H1_


REFUSED = ['multiclass', 'concat', 'sharded', 'fused_off', 'predict_off', 'one_field', 'D12', 'F65', 'FD528', 'with_dnn',
           'with_linear', 'two_product_nets', 'pnn_twice', 'H1_129', 'H2_65', 'three_cells', 'tanh_tower', 'output_kernel']


@pytest.mark.parametrize('case', REFUSED)
def test_graphs_and_switches_refused(rec, monkeypatch, case):
    import torch
    from deeptables_amd import _lib, fused
    kw = {}
    if case == 'multiclass':
        kw['task'] = 'multiclass'
    elif case == 'concat':
        kw['stacking_op'] = 'concat'
    elif case == 'one_field':
        # the product net returns None (no layer of its own), and alone it leaves the graph without any net: beside the tower
        kw.update(F=1, nets=['ipnn_nets', 'dnn_nets'])
    elif case == 'D12':
        kw['D'] = 12
    elif case == 'F65':
        kw.update(F=65, D=4)
    elif case == 'FD528':
        kw.update(F=33, D=16)
    elif case == 'with_dnn':
        kw['nets'] = ['pnn_nets', 'dnn_nets']
    elif case == 'with_linear':
        kw['nets'] = ['linear', 'ipnn_nets']
    elif case == 'two_product_nets':
        kw['nets'] = ['ipnn_nets', 'opnn_nets']
    elif case == 'H1_129':
        kw['hidden'] = ((129, 0, False), (64, 0, False))
    elif case == 'H2_65':
        kw['hidden'] = ((128, 0, False), (65, 0, False))
    elif case == 'three_cells':
        kw['hidden'] = ((64, 0, False), (32, 0, False), (16, 0, False))
    elif case == 'tanh_tower':
        kw['activation'] = 'tanh'
    dm = _model(**kw)
    if case == 'one_field':
        assert 'inner_product_layer' not in dm.model.layers_by_name and 'ipnn_dense_1' not in dm.model.layers_by_name
    if case == 'predict_off':
        monkeypatch.setenv('DT_AMD_FUSED_PREDICT', '0')
    elif case == 'fused_off':
        monkeypatch.setenv('DT_AMD_FUSED', '0')
    elif case == 'pnn_twice':
        # ModelConfig drops a repeated name (deepnets.get_nets), so the repetition is put where the plan reads it
        dm.config = dm.config._replace(nets=['pnn_nets', 'pnn_nets'])
    elif case == 'output_kernel':
        out = dm.model.layers_by_name['task_output']
        out.kernel.data = torch.zeros(H2_ + 1, 1)
    elif case == 'sharded':
        class _Sharded:
            sharded_embeddings, active, world_size = True, True, 1
        dm.config = dm.config._replace(distribute_strategy=_Sharded())
    assert fused.make_inference_plan(dm) is None
    assert not (case not in ('predict_off', 'fused_off') and fused.InferPNN.eligible(dm))
    if case == 'output_kernel':
        return                                   # (the layer path itself cannot run a kernel of the wrong shape)
    with pytest.raises(_lib.DtHipError, match='GPU only'):        # the layer path runs: its first kernel refuses CPU tensors
        dm.predict(_frame(20, F=kw.get('F', F_)), batch_size=8)
    assert rec.names() == []


@pytest.mark.parametrize('case', ['var_len_column', 'two_embedding_groups'])
def test_var_len_columns_and_several_embedding_groups_are_refused(rec, case):
    """both graphs build with their product layers (a var-len column is one more field of the pairs; with
    fixed_embedding_dim=False the columns' own sizes make two groups of the embedding layer) and neither takes the plan"""
    from deeptables_amd import _lib, fused
    from deeptables_amd.models import ModelConfig, DeepModel
    from deeptables_amd.models.metainfo import CategoricalColumn, ContinuousColumn, VarLenCategoricalColumn
    dnn = {'hidden_units': ((H1_, 0, False), (H2_, 0, False)), 'activation': 'relu'}
    conts = [ContinuousColumn('input_continuous_all', ['a', 'b', 'c'])]
    if case == 'var_len_column':
        conf = ModelConfig(nets=['pnn_nets'], fixed_embedding_dim=True, embeddings_output_dim=D_, embedding_dropout=0,
                           dnn_params=dnn)
        vl = VarLenCategoricalColumn('g', 12, D_)
        vl.max_elements_length = 5
        dm = DeepModel('binary', 2, conf, [CategoricalColumn(f'C{i}', 20 + i, D_) for i in range(F_)], conts,
                       var_categorical_len_columns=[vl])
    else:
        conf = ModelConfig(nets=['pnn_nets'], fixed_embedding_dim=False, embedding_dropout=0, dnn_params=dnn)
        dm = DeepModel('binary', 2, conf, [CategoricalColumn(f'C{i}', 20 + i, 16 if i < 3 else 8) for i in range(F_)], conts)
    dm.build('cpu')
    L = dm.model.layers_by_name
    assert 'pnn_inner_product_layer' in L and 'pnn_outer_product_layer' in L and 'pnn_dense_1' in L
    if case == 'var_len_column':
        assert dm.var_len_categorical_columns and 'emb_g' in L
    else:
        assert len(L['emb_categorical_vars_all'].groups) == 2
    assert fused.make_inference_plan(dm) is None and dm.inference_plan() is None
    assert not fused.InferPNN.eligible(dm)
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
    assert type(_afm_model().inference_plan()) is fused.InferAFM
    for nets in (DEEPFM, DCN, ['dnn_nets'], ['linear', 'fm_nets']):
        assert not fused.InferPNN.eligible(_other_model(nets))
    assert not fused.InferPNN.eligible(_afm_model())
    assert _model().fused_plan() is None                 # the training side has no PNN plan


def test_building_the_plan_moves_nothing(rec):
    dm = _model(nets=['pnn_nets'])
    before = {n: p.data_ptr() for n, p in dm.model.named_parameters()}
    assert type(dm.inference_plan()).__name__ == 'InferPNN'
    assert {n: p.data_ptr() for n, p in dm.model.named_parameters()} == before
    assert getattr(dm.optimizer, '_flat', None) is None and not hasattr(dm, '_fused_plan')
