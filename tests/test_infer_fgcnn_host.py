# -*- coding:utf-8 -*-
"""CPU: the inference plan for the FGCNN graph (fused.InferFGCNN, dt_fgcnn_infer*, csrc/fgcnn_infer.hip) — what the
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
H1_, H2_ = 100, 40
KEYS = ('fg_filters', 'fg_heights', 'fg_pool_heights', 'fg_new_feat_filters')
DEFAULTS = ((14, 16), (7, 7), (2, 2), (2, 2))
FG_ENTRIES = ('dt_fgcnn_infer_prepare', 'dt_fgcnn_infer_conv', 'dt_fgcnn_infer_recomb', 'dt_fgcnn_infer_tower')
OTHER_ENTRIES = ('dt_deepfm_infer_prepare', 'dt_deepfm_infer', 'dt_dcn_infer_prepare', 'dt_dcn_infer',
                 'dt_stack_infer_prepare', 'dt_stack_infer', 'dt_xdeepfm_infer_prepare', 'dt_xdeepfm_infer_tower',
                 'dt_xdeepfm_infer_cin', 'dt_xdeepfm_infer_head', 'dt_autoint_infer_prepare', 'dt_autoint_infer',
                 'dt_afm_infer_prepare', 'dt_afm_infer', 'dt_pnn_infer_prepare', 'dt_pnn_infer', 'dt_fibi_infer_prepare',
                 'dt_fibi_infer')
# block lists: the defaults; one block; three blocks with a height above the field count and a pool that does not divide
GRAPHS = [DEFAULTS, ((3,), (2,), (3,), (1,)), ((5, 4, 3), (9, 2, 3), (3, 2, 1), (1, 3, 2))]


@pytest.fixture
def rec(monkeypatch):
    return install_recorder(monkeypatch, FG_ENTRIES + OTHER_ENTRIES,
                            ('DT_AMD_FUSED', 'DT_AMD_FUSED_PREDICT', 'DT_AMD_TOWER_DTYPE'))


def _model(nets=('fgcnn_dnn_nets',), task='binary', D=D_, F=F_, fg=DEFAULTS, hidden=((H1_, 0, False), (H2_, 0, False)),
           activation='relu', mfma_dtype=None, dense=True, **extra):
    from deeptables_amd.models import ModelConfig, DeepModel
    from deeptables_amd.models.metainfo import CategoricalColumn, ContinuousColumn
    dnn = {'hidden_units': hidden, 'activation': activation}
    if mfma_dtype:
        dnn['mfma_dtype'] = mfma_dtype
    conf = ModelConfig(nets=list(nets), fixed_embedding_dim=True, embeddings_output_dim=D, fgcnn_params=dict(zip(KEYS, fg)),
                       dnn_params=dnn, **{'embedding_dropout': 0, **extra})
    dm = DeepModel(task, 2 if task != 'multiclass' else 3, conf, [CategoricalColumn(f'C{i}', 20 + i, D) for i in range(F)],
                   [ContinuousColumn('input_continuous_all', ['a', 'b', 'c'])] if dense else [])
    dm.build('cpu')
    return dm


def _frame(n, seed=0, F=F_, dense=True):
    g = np.random.default_rng(seed)
    df = pd.DataFrame({f'C{i}': g.integers(0, 20, n) for i in range(F)})
    if dense:
        for k in ('a', 'b', 'c'):
            df[k] = g.standard_normal(n).astype(np.float32)
    return df


def _blocks(dm):
    return [l for l in dm.model.layers_by_name.values() if type(l).__name__ == 'FGCNN']


def _dims(F, D, fg):
    """per block (F_k, C_k, Fp_k, K_k, N_k)"""
    out, C = [], 1
    for filt, _, pool, nf in zip(*fg):
        Fp = -(-F // pool)
        out.append((F, C, Fp, Fp * D * filt, F * D * nf))
        F, C = Fp, filt
    return out


def _arrs(fg):
    keep = [(ctypes.c_int * len(v))(*v) for v in fg]
    return keep, [ctypes.cast(a, ctypes.c_void_p) for a in keep]


def _ints(p, n):
    return tuple(ctypes.cast(p, ctypes.POINTER(ctypes.c_int))[i] for i in range(n))


def _ptrs(p, n):
    return tuple(ctypes.cast(p, ctypes.POINTER(ctypes.c_void_p))[i] for i in range(n))


# ---- the library's predicates (no launch) ---------------------------------------------------------------------------------
def test_the_constants_are_the_headers():
    from deeptables_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'dt_hip.h')).read()
    defines = {k: int(v, 0) for k, v in re.findall(r'#define (DT_FGCNN_\w+) (\w+)', header)}
    assert defines == {'DT_FGCNN_INFER_MAX_BLOCKS': _lib.DT_FGCNN_INFER_MAX_BLOCKS,
                       'DT_FGCNN_INFER_MAX_DEPTH': _lib.DT_FGCNN_INFER_MAX_DEPTH}
    assert set(FG_ENTRIES) | {'dt_fgcnn_infer_supported', 'dt_fgcnn_infer_workspace_bytes'} == \
        {n for n in _lib.SIGNATURES if n.startswith('dt_fgcnn_')}


def test_predicate_at_and_just_beyond_each_limit():
    from deeptables_amd import _lib
    lib = _lib.lib()

    def ok(F, D, Nd, fg=((3,), (3,), (2,), (1,)), H1=128, H2=64, cells=0, depth=None):
        keep, a = _arrs(fg)
        return lib.dt_fgcnn_infer_supported(F, D, Nd, H1, H2, cells, len(fg[0]) if depth is None else depth, *a)
    # 2 <= F <= 64
    assert ok(1, 8, 1) == 0 and ok(2, 8, 1) == 1 and ok(64, 8, 1) == 1 and ok(65, 8, 1) == 0 and ok(65, 4, 1) == 0
    # the embedding sizes
    assert ok(2, 2, 1) == 0 and ok(2, 4, 1) == 1 and ok(2, 64, 1) == 1 and ok(2, 128, 1) == 0
    for D in (8, 16, 32):
        assert ok(4, D, 5) == 1, D
    for D in (0, 12, 20):
        assert ok(2, D, 1) == 0, D
    # F D <= 512
    assert ok(32, 16, 1) == 1 and ok(36, 16, 1) == 0 and ok(8, 64, 1) == 1 and ok(9, 64, 1) == 0
    # 0 <= Nd <= 64: the net takes no dense input when there is none
    assert ok(26, 16, -1) == 0 and ok(26, 16, 0) == 1 and ok(26, 16, 64) == 1 and ok(26, 16, 65) == 0
    # depth 1 .. 3
    one = ((3,), (3,), (2,), (1,))
    assert ok(26, 16, 13, one, depth=0) == 0
    for depth in (1, 2, 3):
        assert ok(26, 16, 13, tuple(v * depth for v in one)) == 1, depth
    assert ok(26, 16, 13, tuple(v * 4 for v in one)) == 0
    # filters 1 .. 16, heights 1 .. 9 (both parities, above F_k), pool heights 1 .. 3 (not dividing F_k), new filters 1 .. 3
    for filt, want in ((0, 0), (1, 1), (14, 1), (16, 1), (17, 0)):
        assert ok(26, 16, 13, ((filt,), (3,), (2,), (1,))) == want, filt
    for h, want in ((0, 0), (1, 1), (2, 1), (8, 1), (9, 1), (10, 0)):
        assert ok(5, 16, 13, ((3,), (h,), (2,), (1,))) == want, h
    for p, want in ((0, 0), (1, 1), (2, 1), (3, 1), (4, 0)):
        assert ok(5, 16, 13, ((3,), (3,), (p,), (1,))) == want, p
    for nf, want in ((0, 0), (1, 1), (3, 1), (4, 0)):
        assert ok(5, 16, 13, ((3,), (3,), (2,), (nf,))) == want, nf
    assert ok(5, 8, 3, GRAPHS[2]) == 1 and ok(26, 16, 13, DEFAULTS) == 1
    assert ok(26, 16, 13, ((3, 3), (3, 3), (2, 2), (1, 4))) == 0          # the second block out of range
    # the tower of _infer_tower
    for h1, h2, cells, want in ((128, 64, 3, 1), (1, 1, 0, 1), (100, 40, 2, 1), (129, 64, 0, 0), (128, 65, 0, 0), (0, 64, 0, 0),
                                (128, 0, 0, 0), (128, 64, 4, 0), (128, 64, -1, 0)):
        assert ok(26, 16, 13, DEFAULTS, h1, h2, cells) == want, (h1, h2, cells)
    # null arrays
    assert lib.dt_fgcnn_infer_supported(26, 16, 13, 128, 64, 0, 2, None, None, None, None) == 0


def test_workspace_bytes_follow_the_shape_predicate():
    from deeptables_amd import _lib
    lib = _lib.lib()
    for F, D, Nd, fg in ((1, 8, 1, DEFAULTS), (2, 8, 1, DEFAULTS), (64, 8, 64, DEFAULTS), (65, 8, 1, DEFAULTS), (2, 2, 1, DEFAULTS),
                         (26, 16, 13, DEFAULTS), (26, 16, 0, DEFAULTS), (26, 16, 65, DEFAULTS), (5, 8, 3, GRAPHS[2]),
                         (26, 16, 13, ((17,), (3,), (2,), (1,))), (26, 16, 13, ((3,), (10,), (2,), (1,))),
                         (26, 16, 13, ((3,), (3,), (4,), (1,))), (26, 16, 13, ((3,), (3,), (2,), (4,)))):
        keep, a = _arrs(fg)
        n = lib.dt_fgcnn_infer_workspace_bytes(F, D, Nd, len(fg[0]), *a)
        good = lib.dt_fgcnn_infer_supported(F, D, Nd, 128, 64, 0, len(fg[0]), *a) == 1
        assert (n == -1) == (not good), (F, D, Nd, fg)
        if good:
            bd = _dims(F, D, fg)
            KT = sum(d[4] for d in bd) + F * D + Nd
            packed = sum(6 * d[3] * d[4] for d in bd) + 6 * KT * 128     # the three bf16 parts of every GEMM's weight
            assert n >= packed and n % 16 == 0
    keep, a = _arrs(DEFAULTS)
    assert 21 * 2 ** 20 < lib.dt_fgcnn_infer_workspace_bytes(26, 16, 13, 2, *a) < 23 * 2 ** 20


def test_entry_points_check_their_arguments_before_any_launch():
    from deeptables_amd import _lib
    lib = _lib.lib()
    keep, a = _arrs(DEFAULTS)
    gather = [None, 1, None, None, None]                 # idx, idx_kind, table, row_offset, vocab
    shape = (26, 16, 13, 2, *a)

    def conv(B=0, block=0, kind=1, shape=shape):
        return lib.dt_fgcnn_infer_conv(block, None, kind, None, None, None, None, B, *shape, None, None, None)

    def recomb(B=0, block=0, shape=shape):
        return lib.dt_fgcnn_infer_recomb(block, None, B, *shape, None, None, None)

    def tower(B=0, kind=1, flags=0, shape=shape):
        return lib.dt_fgcnn_infer_tower(None, kind, None, None, None, None, None, B, *shape, None, None, None, None, flags, None)
    assert conv() == 0 and recomb() == 0 and tower(flags=3) == 0          # an empty batch, every pointer null
    assert conv(5) != 0 and b'dt_fgcnn_infer_conv' in lib.dt_last_error()
    assert recomb(5) != 0 and b'dt_fgcnn_infer_recomb' in lib.dt_last_error()
    assert tower(5) != 0 and b'dt_fgcnn_infer_tower' in lib.dt_last_error()
    for f in (conv, recomb, tower):
        assert f(-1) != 0 and f(1 << 31) != 0                              # a negative / too large batch
        assert f(shape=(1, 16, 13, 2, *a)) != 0                            # one field
        assert f(shape=(26, 12, 13, 2, *a)) != 0 and f(shape=(26, 16, 13, 4, *a)) != 0 and f(shape=(26, 16, 13, 0, *a)) != 0
        assert f(shape=(26, 16, 13, 2, None, None, None, None)) != 0
    assert conv(block=2) != 0 and conv(block=-1) != 0 and recomb(block=2) != 0
    assert conv(kind=7) != 0 and tower(kind=7) != 0                        # a bad idx_kind
    assert tower(flags=0x4) != 0                                           # an unknown flag

    def prepare(F=26, D=16, Nd=13, depth=2, H1=128, H2=64, cells=0):
        return lib.dt_fgcnn_infer_prepare(F, D, Nd, depth, *a, *([None] * 4), None, 128, H1, None, None, 64, H2, None, cells,
                                          *([None] * 4), 0.0, *([None] * 4), 0.0, None, None, None, None)
    assert prepare() != 0
    assert b'dt_fgcnn_infer_prepare' in lib.dt_last_error()
    assert prepare(H1=129) != 0 and prepare(F=65, D=8) != 0 and prepare(depth=4) != 0 and prepare(cells=4) != 0


# ---- routing ------------------------------------------------------------------------------------------------------------
def _names(dm, plan):
    """data_ptr -> name of every tensor a dt_fgcnn_infer_prepare call may point to"""
    import torch
    named = {}
    for lname, layer in dm.model.layers_by_name.items():
        for attr in ('kernel', 'bias', 'gamma', 'beta', 'moving_mean', 'moving_variance', 'conv_kernel', 'conv_bias'):
            t = getattr(layer, attr, None)
            if isinstance(t, torch.Tensor):
                named[t.data_ptr()] = f'{lname}.{attr}'
    for k, b in enumerate(_blocks(dm)):
        named[b.dense_output.kernel.data_ptr()] = f'block{k}.dense.kernel'
        named[b.dense_output.bias.data_ptr()] = f'block{k}.dense.bias'
    named[plan.ws.data_ptr()] = 'ws'
    return named


def _decode(args, names):
    return [names.get(a.value, f'?{a.value:#x}') if isinstance(a, ctypes.c_void_p) else a for a in args]


@pytest.mark.parametrize('k', range(len(GRAPHS)))
def test_each_graph_takes_the_plan_and_predict_makes_its_calls(rec, k):
    """prepare once per call; per batch one conv and one recomb call per block in block order, then the tower: 2 depth + 1
    launches, and no other library call.  The pointers are the layers' own tensors — per block the convolution's kernel and
    bias and the recombination Dense's, W1 with its leading dimension, task_output's [H2, 1] kernel as w3; no input
    BatchNormalization is named anywhere (the graph has none: the dense values enter the tower raw)"""
    from deeptables_amd import _lib, fused
    fg = GRAPHS[k]
    depth = len(fg[0])
    task = 'regression' if k == 1 else 'binary'
    bias = k != 2
    hidden = ((H1_, 0, True), (H2_, 0.3, k == 2)) if k else ((H1_, 0, False), (H2_, 0, False))
    dm = _model(task=task, fg=fg, output_use_bias=bias, hidden=hidden)
    plan = dm.inference_plan()
    assert type(plan) is fused.InferFGCNN and plan.params == fg and plan.depth == depth
    assert (plan.F, plan.D, plan.Nd) == (F_, D_, ND_)
    assert rec.names() == [] and not hasattr(dm, '_fused_plan')
    L = dm.model.layers_by_name
    blocks, bd = _blocks(dm), _dims(F_, D_, fg)
    assert len(blocks) == depth
    for b, (Fk, Ck, Fp, K, N), filt, h in zip(blocks, bd, fg[0], fg[1]):
        assert tuple(b.conv_kernel.shape) == (h, 1, Ck, filt) and tuple(b.dense_output.kernel.shape) == (K, N)
        assert b.activation == 'tanh'
    SN = sum(d[4] for d in bd)
    assert tuple(L['task_output'].kernel.shape) == (H2_, 1) and 'dense_logit_fgcnn_dnn_nets' not in L
    assert tuple(L['fgcnn_dnn_dense_1'].kernel.shape) == (SN + F_ * D_ + ND_, H1_)
    n, bsz = 20, 8
    out = dm.predict(_frame(n), batch_size=bsz)
    assert out.shape == (n, 1) and out.dtype == np.float32
    per_batch = [x for j in range(depth) for x in ('dt_fgcnn_infer_conv', 'dt_fgcnn_infer_recomb')] + ['dt_fgcnn_infer_tower']
    assert len(per_batch) == 2 * depth + 1
    assert rec.names() == ['dt_fgcnn_infer_prepare'] + per_batch * 3
    names = _names(dm, plan)
    pa = rec.calls[0][1]
    assert len(pa) == 35
    assert pa[:4] == (F_, D_, ND_, depth) and tuple(_ints(p, depth) for p in pa[4:8]) == fg
    host = [[names.get(v) for v in _ptrs(p, depth)] for p in pa[8:12]]
    assert host == [[f'{b.name}.conv_kernel' for b in blocks], [f'{b.name}.conv_bias' for b in blocks],
                    [f'block{j}.dense.kernel' for j in range(depth)], [f'block{j}.dense.bias' for j in range(depth)]]
    d1, d2 = L['fgcnn_dnn_dense_1'], L['fgcnn_dnn_dense_2']

    def nm(layer, attr):
        return f'{layer.name}.{attr}' if getattr(layer, attr, None) is not None else None
    bits, cellargs = 0, []
    for i in (1, 2):
        b = L.get(f'fgcnn_dnn_bn_{i}')
        if b is None:
            cellargs += [None, None, None, None, 0.0]
        else:
            bits |= 1 << (i - 1)
            cellargs += [nm(b, 'gamma'), nm(b, 'beta'), nm(b, 'moving_mean'), nm(b, 'moving_variance'), float(b.epsilon)]
    assert bits == ((1 | (2 if k == 2 else 0)) if k else 0)
    decoded = _decode(pa[12:], names)
    assert decoded == [nm(d1, 'kernel'), H1_, H1_, nm(d1, 'bias'), nm(d2, 'kernel'), H2_, H2_, nm(d2, 'bias'), bits] + \
        cellargs + ['task_output.kernel', nm(L['task_output'], 'bias'), 'ws', None]
    assert not any(isinstance(v, str) and v.startswith('bn_concat') for v in decoded)
    assert (L['task_output'].bias is None) == (not bias)
    keep, a = _arrs(fg)
    assert plan.ws.numel() * 4 == _lib.lib().dt_fgcnn_infer_workspace_bytes(F_, D_, ND_, depth, *a)
    emb = L['emb_categorical_vars_all']
    gather = (emb.tables[plan.key].data_ptr(), getattr(emb, f'row_offset_{plan.key}').data_ptr(),
              getattr(emb, f'vocab_{plan.key}').data_ptr())

    def shape_of(a):
        return a[:4], tuple(_ints(p, depth) for p in a[4:8])
    done, lg0, out0 = 0, None, None
    for i in range(3):
        calls = rec.calls[1 + i * len(per_batch):1 + (i + 1) * len(per_batch)]
        B = (8, 8, 4)[i]
        pooled, feats = [], None
        for j in range(depth):
            c, r = calls[2 * j][1], calls[2 * j + 1][1]
            assert len(c) == 19 and c[0] == j and c[2] in (_lib.DT_IDX_F32, _lib.DT_IDX_I32)
            assert tuple(v.value for v in c[3:6]) == gather and c[7] == B
            assert shape_of(c[8:16]) == ((F_, D_, ND_, depth), fg) and c[16].value == plan.ws.data_ptr() and c[18] is None
            assert (c[6] is None) if j == 0 else (c[6].value == pooled[j - 1])       # the pooled map of the block before
            pooled.append(c[17].value)
            assert len(r) == 14 and r[0] == j and r[1].value == pooled[j] and r[2] == B
            assert shape_of(r[3:11]) == ((F_, D_, ND_, depth), fg) and r[11].value == plan.ws.data_ptr() and r[13] is None
            feats = feats or r[12].value
            assert r[12].value == feats
        assert len(set(pooled)) == depth and feats not in pooled
        t = calls[-1][1]
        assert len(t) == 22 and t[1] in (_lib.DT_IDX_F32, _lib.DT_IDX_I32) and tuple(v.value for v in t[2:5]) == gather
        assert t[5] is not None and t[6].value == feats and t[7] == B
        assert shape_of(t[8:16]) == ((F_, D_, ND_, depth), fg) and t[16].value == plan.ws.data_ptr() and t[19] is None
        assert t[20] == (_lib.DT_INFER_SIGMOID if task == 'binary' else 0) and t[21] is None
        if i == 0:
            lg0, out0 = t[17].value, t[18].value
        assert t[17].value == lg0 + 4 * done and t[18].value == out0 + 4 * done
        done += B
    assert done == n


def test_no_dense_input_is_in_the_domain(rec):
    from deeptables_amd import fused
    dm = _model(dense=False)
    plan = dm.inference_plan()
    assert type(plan) is fused.InferFGCNN and plan.Nd == 0
    dm.predict(_frame(10, dense=False), batch_size=16)
    assert rec.names() == ['dt_fgcnn_infer_prepare'] + ['dt_fgcnn_infer_conv', 'dt_fgcnn_infer_recomb'] * 2 + ['dt_fgcnn_infer_tower']
    t = rec.calls[-1][1]
    assert t[5] is None and t[10] == 0


def test_the_tower_mode_and_the_block_parameters_are_read_in_prepare(rec):
    from deeptables_amd import _lib
    dm = _model(mfma_dtype='bf16')
    dm.predict(_frame(10), batch_size=16)
    assert rec.calls[-1][0] == 'dt_fgcnn_infer_tower'
    assert rec.calls[-1][1][20] == _lib.DT_INFER_SIGMOID | _lib.DT_INFER_TOWER_BF16
    dm.config.dnn_params['mfma_dtype'] = 'f32'           # read in prepare: the six-product forward serves the f32 mode too
    rec.calls.clear()
    dm.predict(_frame(10), batch_size=16)
    assert rec.calls[-1][1][20] == _lib.DT_INFER_SIGMOID
    assert tuple(_ints(p, 2) for p in rec.calls[0][1][4:8]) == DEFAULTS


def test_prepare_reads_the_tensors_at_call_time(rec):
    """the plan caches no parameter: a tensor re-homed between two predicts is the one the second prepare names"""
    import torch
    dm = _model()
    dm.predict(_frame(10), batch_size=16)
    L = dm.model.layers_by_name
    b0, b1 = _blocks(dm)
    d1 = L['fgcnn_dnn_dense_1']
    a0 = rec.calls[0][1]
    assert _ptrs(a0[8], 2) == (b0.conv_kernel.data_ptr(), b1.conv_kernel.data_ptr())
    assert _ptrs(a0[10], 2) == (b0.dense_output.kernel.data_ptr(), b1.dense_output.kernel.data_ptr())
    assert a0[12].value == d1.kernel.data_ptr() and a0[13] == H1_
    old = (b1.conv_kernel.data_ptr(), b0.dense_output.kernel.data_ptr(), d1.kernel.data_ptr())
    slab = torch.zeros(d1.kernel.shape[0], 128)
    slab[:, :H1_] = d1.kernel.data
    d1.kernel.data = slab[:, :H1_]
    b1.conv_kernel.data = torch.clone(b1.conv_kernel.data) * 2
    b0.dense_output.kernel.data = torch.clone(b0.dense_output.kernel.data)
    rec.calls.clear()
    dm.predict(_frame(10), batch_size=16)
    assert rec.names()[0] == 'dt_fgcnn_infer_prepare' and len(rec.names()) == 6
    a1 = rec.calls[0][1]
    assert _ptrs(a1[8], 2) == (b0.conv_kernel.data_ptr(), b1.conv_kernel.data_ptr()) and b1.conv_kernel.data_ptr() != old[0]
    assert _ptrs(a1[10], 2)[0] == b0.dense_output.kernel.data_ptr() != old[1]
    assert a1[12].value == slab.data_ptr() != old[2] and a1[13] == 128 and a1[14] == H1_


REFUSED = ['with_linear', 'with_dnn', 'fg_nets', 'fgcnn_ipnn_nets', 'fgcnn_fm_nets', 'fgcnn_cin_nets', 'fgcnn_afm_nets', 'concat',
           'multiclass', 'tanh_tower', 'three_cells', 'H1_129', 'H2_65', 'sharded', 'fused_off', 'predict_off', 'D12', 'FD576',
           'one_field', 'output_kernel', 'relu_block', 'extra_block', 'four_blocks', 'filters_17', 'height_10', 'pool_4',
           'new_filters_4', 'conv_kernel_shape', 'dense_kernel_shape']


@pytest.mark.parametrize('case', REFUSED)
def test_graphs_and_switches_refused(rec, monkeypatch, case):
    import torch
    from deeptables_amd import _lib, fused
    kw = {}
    if case == 'with_linear':
        kw['nets'] = ['linear', 'fgcnn_dnn_nets']
    elif case == 'with_dnn':
        kw['nets'] = ['fgcnn_dnn_nets', 'dnn_nets']
    elif case in ('fg_nets', 'fgcnn_ipnn_nets', 'fgcnn_fm_nets', 'fgcnn_cin_nets', 'fgcnn_afm_nets'):
        kw['nets'] = [case]
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
    elif case == 'one_field':
        kw['F'] = 1
    elif case == 'four_blocks':
        kw['fg'] = ((3,) * 4, (3,) * 4, (2,) * 4, (1,) * 4)
    elif case == 'filters_17':
        kw['fg'] = ((17,), (3,), (2,), (1,))
    elif case == 'height_10':
        kw['fg'] = ((3,), (10,), (2,), (1,))
    elif case == 'pool_4':
        kw['fg'] = ((3,), (3,), (4,), (1,))
    elif case == 'new_filters_4':
        kw['fg'] = ((3,), (3,), (2,), (4,))
    dm = _model(**kw)
    tampered = ('output_kernel', 'relu_block', 'extra_block', 'conv_kernel_shape', 'dense_kernel_shape')
    if case == 'predict_off':
        monkeypatch.setenv('DT_AMD_FUSED_PREDICT', '0')
    elif case == 'fused_off':
        monkeypatch.setenv('DT_AMD_FUSED', '0')
    elif case == 'output_kernel':
        dm.model.layers_by_name['task_output'].kernel.data = torch.zeros(H2_ + 1, 1)
    elif case == 'sharded':
        class _Sharded:
            sharded_embeddings, active, world_size = True, True, 1
        dm.config = dm.config._replace(distribute_strategy=_Sharded())
    elif case == 'relu_block':
        _blocks(dm)[1].activation = 'relu'
    elif case == 'extra_block':
        from deeptables_amd.models import layers
        dm.model.layers_by_name['fgcnn_99'] = layers.FGCNN(3, 3, 1, 2, name='fgcnn_99')
    elif case == 'conv_kernel_shape':
        b = _blocks(dm)[0]
        b.conv_kernel.data = torch.zeros(5, 1, 1, b.filters)
    elif case == 'dense_kernel_shape':
        b = _blocks(dm)[1]
        b.dense_output.kernel.data = torch.zeros(b.dense_output.kernel.shape[0] + 16, b.dense_output.kernel.shape[1])
    assert fused.make_inference_plan(dm) is None
    assert not (case not in ('predict_off', 'fused_off') and fused.InferFGCNN.eligible(dm))
    if case in tampered:
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
        conf = ModelConfig(nets=['fgcnn_dnn_nets'], fixed_embedding_dim=True, embeddings_output_dim=D_, embedding_dropout=0,
                           dnn_params=dnn)
        vl = VarLenCategoricalColumn('g', 12, D_)
        vl.max_elements_length = 5
        dm = DeepModel('binary', 2, conf, [CategoricalColumn(f'C{i}', 20 + i, D_) for i in range(F_)], conts,
                       var_categorical_len_columns=[vl])
    else:
        conf = ModelConfig(nets=['fgcnn_dnn_nets'], fixed_embedding_dim=False, embedding_dropout=0, dnn_params=dnn)
        dm = DeepModel('binary', 2, conf, [CategoricalColumn(f'C{i}', 20 + i, 16) for i in range(F_)], conts)
    dm.build('cpu')
    L = dm.model.layers_by_name
    if case == 'two_embedding_groups':
        # the net concatenates the fields, so they share one width; the second group is a table re-homed beside the first
        emb = L['emb_categorical_vars_all']
        emb.groups = list(emb.groups) + [emb.groups[0]]
        assert len(emb.groups) == 2
    else:
        assert dm.var_len_categorical_columns and 'emb_g' in L
    assert len(_blocks(dm)) == 2 and 'fgcnn_dnn_dense_1' in L
    assert fused.make_inference_plan(dm) is None and dm.inference_plan() is None
    assert not fused.InferFGCNN.eligible(dm)
    assert rec.names() == []


def test_the_other_graphs_keep_their_plans(rec):
    from deeptables_amd import fused
    assert type(_other_model(DEEPFM).inference_plan()) is fused.InferDeepFM
    assert type(_other_model(DCN).inference_plan()) is fused.InferDCN
    assert type(_other_model(['dnn_nets']).inference_plan()) is fused.InferStack
    from tests.test_infer_afm_host import _model as _afm_model
    from tests.test_infer_pnn_host import _model as _pnn_model
    from tests.test_infer_fibi_host import _model as _fibi_model
    assert type(_afm_model().inference_plan()) is fused.InferAFM
    assert type(_pnn_model().inference_plan()) is fused.InferPNN
    assert type(_fibi_model().inference_plan()) is fused.InferFiBiNet
    for nets in (DEEPFM, DCN, ['dnn_nets'], ['linear', 'fm_nets']):
        assert not fused.InferFGCNN.eligible(_other_model(nets))
    assert not fused.InferFGCNN.eligible(_fibi_model()) and not fused.InferFGCNN.eligible(_pnn_model())
    assert _model().fused_plan() is None                 # the training side has no FGCNN plan


def test_building_the_plan_moves_nothing(rec):
    dm = _model()
    before = {n: p.data_ptr() for n, p in dm.model.named_parameters()}
    assert type(dm.inference_plan()).__name__ == 'InferFGCNN'
    assert {n: p.data_ptr() for n, p in dm.model.named_parameters()} == before
    assert getattr(dm.optimizer, '_flat', None) is None and not hasattr(dm, '_fused_plan')
