# -*- coding:utf-8 -*-
"""CPU: the inference plan for the xDeepFM graph (fused.InferXDeepFM, dt_xdeepfm_infer_*, csrc/infer_x3.h) — which graphs
it takes, what the library's predicates accept, which calls `predict` / `evaluate` make with which tensors.  The plans are
built on CPU models and their launches recorded by a stand-in for the library (the recorder of tests/test_infer_stack_host.py,
restated for the dt_xdeepfm_* names): nothing runs on a GPU."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from tests.infer_support import install_recorder
from tests.test_infer_host import F_, D_, ND_, DEEPFM, DCN, _frame, _model, _names, _decode

XDEEPFM = ['linear', 'cin_nets', 'dnn_nets']
ORDERS = [list(p) for p in itertools.permutations(XDEEPFM)]
XD_BATCH = ('dt_xdeepfm_infer_tower', 'dt_xdeepfm_infer_cin', 'dt_xdeepfm_infer_head')
XD_ENTRIES = ('dt_xdeepfm_infer_prepare',) + XD_BATCH
OTHER_ENTRIES = ('dt_deepfm_infer_prepare', 'dt_deepfm_infer', 'dt_dcn_infer_prepare', 'dt_dcn_infer',
                 'dt_stack_infer_prepare', 'dt_stack_infer', 'dt_cin_pack', 'dt_cin_layer_fwd_packed')
CIN = {'cross_layer_size': (8, 6), 'direct': False}
F32, BF16, X3 = 0, 1, 2


@pytest.fixture
def rec(monkeypatch):
    return install_recorder(monkeypatch, XD_ENTRIES + OTHER_ENTRIES,
                            ('DT_AMD_FUSED', 'DT_AMD_FUSED_PREDICT', 'DT_AMD_TOWER_DTYPE', 'DT_AMD_CIN_DTYPE'))


def _xd(nets=XDEEPFM, hidden=((100, 0, False), (40, 0, False)), cin=CIN, **kw):
    return _model(list(nets), hidden, cin_params=dict(cin), **kw)


def _sizes(n, *v):
    return (ctypes.c_int * n)(*v)


def _host_ints(arg, n):
    return list((ctypes.c_int * n).from_address(arg.value))


def _host_ptrs(arg, n):
    return list((ctypes.c_void_p * n).from_address(arg.value))


def test_the_mode_codes_are_the_headers():
    from deeptables_amd import _lib
    assert (_lib.DT_CIN_F32, _lib.DT_CIN_BF16, _lib.DT_CIN_BF16X3) == (F32, BF16, X3)
    assert _lib.DT_XDEEPFM_MAX_LAYERS == 8


# ---- the library's predicates (no launch) ---------------------------------------------------------------------------------
def test_predicate_follows_the_stack_plans_domain_and_the_cin_kernels():
    from deeptables_amd import _lib
    lib = _lib.lib()

    def ok(F=26, D=16, Nd=13, h1=128, h2=64, cells=0, sizes=(128, 128), direct=0, res=0, red=0, act=1, mode=X3):
        return lib.dt_xdeepfm_infer_supported(F, D, Nd, h1, h2, cells, len(sizes), _sizes(len(sizes), *sizes), direct, res, red,
                                              act, mode)

    for mode in (F32, BF16, X3):
        assert ok(mode=mode) == 1 and ok(mode=mode, direct=1) == 1 and ok(mode=mode, sizes=(64, 32, 16)) == 1
        assert ok(mode=mode, D=4) == 1 and ok(mode=mode, Nd=0) == 1 and ok(mode=mode, cells=3) == 1
    assert ok(F=64, D=8, Nd=0) == 1 and ok(F=65, D=4, Nd=0) == 0                   # F <= 64 (the stack plan alone takes 65)
    assert lib.dt_stack_infer_supported(65, 4, 0, 128, 64, 0, 5) == 1
    # the stack plan's field / tower domain
    assert ok(D=12) == 0 and ok(D=128, F=1) == 0 and ok(Nd=65) == 0 and ok(F=33, D=16, Nd=17) == 0
    assert ok(h1=129) == 0 and ok(h2=65) == 0 and ok(cells=4) == 0 and ok(h1=1, h2=1) == 1
    # the CIN: 1 .. 8 layers, even sizes where direct=False halves them, no residual, no reduce_D, a known mode
    assert ok(sizes=(7, 6)) == 0 and ok(sizes=(8, 7)) == 1 and ok(sizes=(7, 5), direct=1) == 1 and ok(sizes=(6,)) == 1
    assert ok(sizes=()) == 0 and ok(sizes=(8,) * 8) == 1 and ok(sizes=(8,) * 9) == 0 and ok(sizes=(8, 0)) == 0
    assert ok(res=1) == 0 and ok(red=1) == 0 and ok(mode=3) == 0 and ok(mode=-1) == 0
    assert ok(act=3) == 1 and ok(act=99) == 0 and ok(act=-1) == 0
    # the layer kernels' own limits: the bf16 modes take L <= 256 and Hk <= 128, the exact kernel has neither limit
    assert ok(sizes=(258, 8), mode=X3) == 0 and ok(sizes=(258, 8), mode=BF16) == 0 and ok(sizes=(258, 8), mode=F32) == 1
    assert ok(sizes=(256, 8), mode=X3, direct=1) == 0 and ok(sizes=(256, 8), mode=X3, direct=0) == 1    # Hk = 256 / 128
    for mode in (F32, BF16, X3):
        for F0, Hk, L, D, act in ((26, 26, 128, 16, 1), (26, 64, 128, 16, 1), (64, 128, 256, 4, 3), (1, 1, 1, 4, 0)):
            assert lib.dt_cin_fwd_supported(mode, F0, Hk, L, D, act) == 1, (mode, F0, Hk, L, D, act)
        assert lib.dt_cin_fwd_supported(mode, 0, 8, 8, 4, 1) == 0 and lib.dt_cin_fwd_supported(mode, 8, 8, 8, 4, 99) == 0
    assert lib.dt_cin_fwd_supported(3, 8, 8, 8, 4, 1) == 0


def test_workspace_is_the_tower_layouts_the_exfm_vector_and_the_packed_filters():
    from deeptables_amd import _lib
    lib = _lib.lib()
    F, D, Nd, sizes = 26, 16, 13, (128, 128)
    base = lib.dt_stack_infer_workspace_bytes(F, D, Nd, 5)
    hks = (26, 64)
    for mode in (F32, BF16, X3):
        packed = [lib.dt_cin_packed_bytes(mode, F, hk, l) for hk, l in zip(hks, sizes)]
        assert all(p > 0 and p % 16 == 0 for p in packed)
        got = lib.dt_xdeepfm_infer_workspace_bytes(F, D, Nd, 2, _sizes(2, *sizes), 0, mode)
        assert got == base + (64 + 128) * 4 + 16 + sum(packed), mode
    assert lib.dt_cin_packed_bytes(F32, 26, 64, 128) == 26 * 64 * 128 * 4
    assert lib.dt_cin_packed_bytes(BF16, 26, 64, 128) == 2 * 128 * 26 * 64            # W^T [Lp][F0 Hp], one bf16 part
    assert lib.dt_cin_packed_bytes(X3, 26, 26, 128) == 3 * 2 * 128 * 26 * 32          # Hp = Hk rounded up to 8, three parts
    assert lib.dt_cin_packed_bytes(3, 26, 26, 128) == -1 and lib.dt_cin_packed_bytes(X3, 0, 26, 128) == -1
    assert lib.dt_xdeepfm_infer_workspace_bytes(65, 4, 0, 2, _sizes(2, 8, 8), 0, X3) == -1
    assert lib.dt_xdeepfm_infer_workspace_bytes(F, D, Nd, 2, _sizes(2, 7, 8), 0, X3) == -1


def test_entry_points_check_their_arguments_before_any_launch():
    from deeptables_amd import _lib
    lib = _lib.lib()
    sz = _sizes(2, 8, 6)
    none = [None, 1, None, None, None, None]           # idx, idx_kind, table, row_offset, vocab, dense
    assert lib.dt_xdeepfm_infer_tower(*none, 0, 6, 8, 3, None, None, None, None, 0, None) == 0          # an empty batch
    assert lib.dt_xdeepfm_infer_tower(*none, 5, 6, 8, 3, None, None, None, None, 0, None) != 0
    assert b'dt_xdeepfm_infer_tower' in lib.dt_last_error()
    assert lib.dt_xdeepfm_infer_tower(*none, 0, 6, 8, 3, None, None, None, None, 0x1, None) != 0        # no sigmoid here
    assert lib.dt_xdeepfm_infer_cin(0, None, None, None, 1, 0, 6, 8, 3, 2, sz, 0, X3, None, None, None) == 0
    assert lib.dt_xdeepfm_infer_cin(0, None, None, None, 1, 4, 6, 8, 3, 2, sz, 0, X3, None, None, None) != 0
    assert b'dt_xdeepfm_infer_cin' in lib.dt_last_error()
    assert lib.dt_xdeepfm_infer_cin(2, None, None, None, 1, 0, 6, 8, 3, 2, sz, 0, X3, None, None, None) != 0   # layer 2 of 2
    assert lib.dt_xdeepfm_infer_cin(0, None, None, None, 1, 0, 65, 4, 0, 2, sz, 0, X3, None, None, None) != 0
    assert lib.dt_xdeepfm_infer_head(None, None, 0, 6, 8, 3, 2, sz, 0, X3, None, None, None, 1, None) == 0
    assert lib.dt_xdeepfm_infer_head(None, None, 4, 6, 8, 3, 2, sz, 0, X3, None, None, None, 1, None) != 0
    assert b'dt_xdeepfm_infer_head' in lib.dt_last_error()
    assert lib.dt_xdeepfm_infer_head(None, None, 0, 6, 8, 3, 2, sz, 0, X3, None, None, None, 0x2, None) != 0
    assert lib.dt_xdeepfm_infer_head(None, None, 0, 6, 8, 3, 2, _sizes(2, 7, 6), 0, X3, None, None, None, 0, None) != 0
    assert lib.dt_cin_pack(7, None, 6, 6, 8, None, None) != 0 and lib.dt_cin_pack(X3, None, 6, 6, 8, None, None) != 0
    assert lib.dt_cin_layer_fwd_packed(X3, None, None, None, None, 1, 0, 6, 6, 8, 8, 48, 48, None, None) == 0
    assert lib.dt_cin_layer_fwd_packed(X3, None, None, None, None, 1, 2, 6, 6, 8, 8, 48, 48, None, None) != 0
    assert lib.dt_cin_layer_fwd_packed(X3, None, None, None, None, 1, 0, 6, 6, 300, 8, 48, 48, None, None) != 0


# ---- routing ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nets', ORDERS, ids='+'.join)
def test_the_preset_takes_the_plan_in_every_net_order(rec, nets):
    from deeptables_amd import fused
    dm = _xd(nets)
    plan = dm.inference_plan()
    assert type(plan) is fused.InferXDeepFM
    assert plan.n_layers == 2 and list(plan.sizes) == [8, 6] and plan.direct == 0 and plan.cin_mode == X3
    assert not hasattr(dm, '_fused_plan') and rec.names() == []


def _xd_names(dm):
    names = _names(dm)
    cin = dm.inference_plan().cin
    names[cin.exFM_out.kernel.data_ptr()] = 'exFM_out.kernel'
    names[cin.exFM_out.bias.data_ptr()] = 'exFM_out.bias'
    return names


@pytest.mark.parametrize('direct', [False, True])
def test_predict_makes_one_prepare_and_two_plus_n_layers_calls_per_batch(rec, direct):
    from deeptables_amd import _lib
    dm = _xd(cin=dict(CIN, direct=direct), output_use_bias=False)
    plan = dm.inference_plan()
    n, b, nl = 20, 8, 2
    out = dm.predict(_frame(n), batch_size=b)
    assert out.shape == (n, 1) and out.dtype == np.float32
    assert rec.names() == ['dt_xdeepfm_infer_prepare'] + ['dt_xdeepfm_infer_tower'] + ['dt_xdeepfm_infer_cin'] * nl + \
        ['dt_xdeepfm_infer_head'] + (['dt_xdeepfm_infer_tower'] + ['dt_xdeepfm_infer_cin'] * nl + ['dt_xdeepfm_infer_head']) * 2
    assert len(rec.calls) == 1 + 3 * (2 + nl)
    names = _xd_names(dm)
    L = dm.model.layers_by_name
    # prepare: the tower as dt_stack_infer_prepare's, then the head weights, the CIN's shape and mode, its filters, exFM_out
    pa = rec.calls[0][1]
    assert len(pa) == 40 and pa[:3] == (F_, D_, ND_)
    d = _decode(pa, names)
    bn, d1, d2 = L['bn_concat_emb_dense'], L['dnn_dense_1'], L['dnn_dense_2']
    assert d[3:17] == ['linear_logit.kernel', 'bn_concat_emb_dense.gamma', 'bn_concat_emb_dense.beta',
                       'bn_concat_emb_dense.moving_mean', 'bn_concat_emb_dense.moving_variance', float(bn.epsilon),
                       'dnn_dense_1.kernel', 100, 100, 'dnn_dense_1.bias', 'dnn_dense_2.kernel', 40, 40, 'dnn_dense_2.bias']
    assert d[17] == 0 and d[18:28] == [None, None, None, None, 0.0] * 2
    assert d[28:31] == ['dense_logit_dnn_nets.kernel', 'task_output.kernel', None]       # no output bias: NULL
    assert L['task_output'].bias is None
    assert pa[31] == nl and _host_ints(pa[32], nl) == [8, 6] and pa[33] == int(direct) and pa[34] == X3
    assert [p for p in _host_ptrs(pa[35], nl)] == [plan.cin.f_[k].data_ptr() for k in range(nl)]
    assert d[36:40] == ['exFM_out.kernel', 'exFM_out.bias', 'ws', None]
    assert tuple(plan.cin.exFM_out.kernel.shape) == ((14, 1) if direct else (10, 1))
    assert plan.ws.numel() * 4 == _lib.lib().dt_xdeepfm_infer_workspace_bytes(F_, D_, ND_, nl, plan.sizes, int(direct), X3)
    # per batch: the same scratch for every batch of the call; every layer reads x0 and the layer before it
    rows, scratch = 0, None
    for i in range(3):
        tower, c0, c1, head = [a for _, a in rec.calls[1 + 4 * i:5 + 4 * i]]
        B = tower[6]
        assert 0 < B <= b and tower[7:10] == (F_, D_, ND_) and names.get(tower[10].value) == 'ws' and tower[14] == 0
        x0, partial = tower[11].value, tower[12].value
        assert c0[0] == 0 and c0[1].value == x0 and c0[2] is None and c0[3] is None and c0[4] == 1 and c0[5] == B
        assert c1[0] == 1 and c1[1].value == x0 and c1[2].value == c0[14].value and c1[5] == B
        for c in (c0, c1):
            assert c[6:9] == (F_, D_, ND_) and c[9] == nl and _host_ints(c[10], nl) == [8, 6] and c[11:13] == (int(direct), X3)
            assert names.get(c[13].value) == 'ws'
        assert _host_ptrs(head[0], nl) == [c0[14].value, c1[14].value] and head[1].value == partial and head[2] == B
        assert head[3:6] == (F_, D_, ND_) and head[6] == nl and head[8:10] == (int(direct), X3)
        assert names.get(head[10].value) == 'ws' and head[13] == _lib.DT_INFER_SIGMOID
        assert head[11].value is not None and head[12].value is not None
        if scratch is None:
            scratch = (x0, partial, c0[14].value, c1[14].value)
        assert scratch == (x0, partial, c0[14].value, c1[14].value)
        rows += B
    assert rows == n and plan._scratch is None
    assert not hasattr(dm, '_fused_plan')


def test_evaluate_routes_through_the_plan(rec, monkeypatch):
    dm = _xd()
    n = 50
    y = (np.arange(n) % 3 == 0).astype(np.float32)
    monkeypatch.setattr(torch, 'empty', lambda *a, **k: torch.zeros(*a, **k))     # the recorded launches write nothing
    res = dm.evaluate(_frame(n), y, batch_size=16)
    assert rec.names() == ['dt_xdeepfm_infer_prepare'] + list(XD_BATCH[:1] + XD_BATCH[1:2] * 2 + XD_BATCH[2:]) * 4
    assert abs(res['loss'] - float(np.log(2.0))) < 1e-6


def test_prepare_reads_the_modes_the_bias_and_regression_at_call_time(rec, monkeypatch):
    from deeptables_amd import _lib
    dm = _xd(task='regression', cin=dict(CIN, use_bias=True, cross_layer_size=(8, 6, 4)))
    plan = dm.inference_plan()
    dm.predict(_frame(10), batch_size=4)
    assert rec.names() == ['dt_xdeepfm_infer_prepare'] + (['dt_xdeepfm_infer_tower'] + ['dt_xdeepfm_infer_cin'] * 3 +
                                                          ['dt_xdeepfm_infer_head']) * 3
    assert rec.calls[0][1][34] == X3 and rec.calls[1][1][14] == 0
    assert [rec.calls[2 + k][1][3].value for k in range(3)] == [plan.cin.bias[k].data_ptr() for k in range(3)]
    assert rec.calls[5][1][13] == 0                     # identity output
    assert rec.calls[0][1][30] is not None              # task_output's bias
    for mode, code in (('bf16', BF16), ('float32', F32), ('bf16x3', X3)):
        rec.calls.clear()
        plan.cin.mfma_dtype = mode                      # the layer path reads this attribute on every call too
        dm.predict(_frame(10), batch_size=4)
        assert rec.calls[0][1][34] == code and rec.calls[2][1][12] == code and rec.calls[5][1][9] == code
        assert plan.ws.numel() * 4 >= _lib.lib().dt_xdeepfm_infer_workspace_bytes(F_, D_, ND_, 3, plan.sizes, 0, code)
    rec.calls.clear()
    monkeypatch.setenv('DT_AMD_TOWER_DTYPE', 'bf16')
    dm.predict(_frame(10), batch_size=4)
    assert rec.calls[1][1][14] == _lib.DT_INFER_TOWER_BF16 and rec.calls[5][1][13] == 0
    plan.cin.mfma_dtype = 'fp8'
    with pytest.raises(ValueError):
        dm.predict(_frame(10), batch_size=4)


def test_the_cin_dtype_switch_is_read_when_the_layer_is_built(rec, monkeypatch):
    monkeypatch.setenv('DT_AMD_CIN_DTYPE', 'float32')
    assert _xd().inference_plan().cin_mode == F32
    assert _xd(cin=dict(CIN, mfma_dtype='bf16')).inference_plan().cin_mode == BF16           # the config wins over the env


@pytest.mark.parametrize('case', ['multiclass', 'concat', 'tanh', 'wide', 'deep', 'residual', 'reduce_D', 'sharded', 'env',
                                  'fused_off'])
def test_graphs_and_switches_refused(rec, monkeypatch, case):
    from deeptables_amd import _lib, fused
    kw, cin = {}, dict(CIN)
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
    elif case == 'residual':
        cin['use_residual'] = True
    elif case == 'reduce_D':
        cin['reduce_D'] = True
    dm = _xd(hidden=hidden, cin=cin, **kw)
    if case == 'env':
        monkeypatch.setenv('DT_AMD_FUSED_PREDICT', '0')
    elif case == 'fused_off':
        monkeypatch.setenv('DT_AMD_FUSED', '0')
    elif case == 'sharded':
        class _Sharded:
            sharded_embeddings, active, world_size = True, True, 1
        dm.config = dm.config._replace(distribute_strategy=_Sharded())
    assert fused.make_inference_plan(dm) is None
    with pytest.raises(_lib.DtHipError, match='GPU only'):        # the layer path runs: its first kernel refuses CPU tensors
        dm.predict(_frame(20), batch_size=8)
    assert rec.names() == []


def test_other_combinations_with_cin_nets_stay_refused_and_the_other_plans_keep_theirs(rec):
    from deeptables_amd import fused
    for nets in (['linear', 'cin_nets'], ['cin_nets', 'dnn_nets'], ['cin_nets'], ['linear', 'cin_nets', 'dnn_nets', 'fm_nets']):
        assert fused.make_inference_plan(_xd(nets)) is None, nets
    assert not fused.InferXDeepFM.eligible(_model(DEEPFM)) and type(_model(DEEPFM).inference_plan()) is fused.InferDeepFM
    assert type(_model(DCN).inference_plan()) is fused.InferDCN
    assert type(_model(['linear', 'dnn_nets']).inference_plan()) is fused.InferStack
    # a tower whose last cell has width 1 has no dense_logit_dnn_nets: refused as by the other plans
    assert fused.make_inference_plan(_xd(hidden=((100, 0, False), (1, 0, False)))) is None
    # the training side has no xDeepFM plan
    assert _xd().fused_plan() is None


def test_building_the_plan_moves_nothing(rec):
    dm = _xd()
    before = {n: p.data_ptr() for n, p in dm.model.named_parameters()}
    assert type(dm.inference_plan()).__name__ == 'InferXDeepFM'
    assert not hasattr(dm, '_fused_plan')
    assert {n: p.data_ptr() for n, p in dm.model.named_parameters()} == before
    assert getattr(dm.optimizer, '_flat', None) is None
