# -*- coding:utf-8 -*-
"""GPU: the fused inference plan for every Add-stacked subset of {'linear', 'fm_nets', 'dnn_nets'} (fused.InferStack:
one k_infer_prep launch per call, one k_infer — or, without a tower, k_infer_sparse — launch per batch, csrc/infer_x3.h)
against the float64 oracle at inference, held to the tower mode's forward class exactly as tests/test_infer_gpu.py holds
DeepFM and DCN (its helpers are used by import); graphs without a tower are plain fp32 sums and are held to the 'f32'
class.  Then the corners of the accepted domain, odd ids, the head variants, row independence, and end to end through
predict / evaluate and a DeepTable built on the bare default ModelConfig() against the layer-by-layer path."""
import numpy as np
import pytest
import torch

import tests.test_infer_gpu as I
from tests.infer_support import _frame, _train_and_perturb

pytestmark = pytest.mark.gpu

LIN, FM, DNN = 'linear', 'fm_nets', 'dnn_nets'
# all seven subsets; two orders where there are two or three nets
NETS = [[LIN], [FM], [DNN], [LIN, FM], [FM, LIN], [LIN, DNN], [DNN, LIN], [FM, DNN], [DNN, FM], [LIN, FM, DNN], [DNN, FM, LIN]]
NET_MODES = [(n, m) for n in NETS for m in (I.MODES if DNN in n else ['f32'])]


def _id(nets):
    return '+'.join(nets)


def _build(nets, F=26, D=16, Nd=13, vocab=30, hidden=None, **kw):
    import tests.test_fused_gpu as T
    if hidden is not None:
        kw['dnn_params'] = {'hidden_units': hidden, 'activation': 'relu'}
    return T.build(F, Nd, D, vocab=vocab, nets=list(nets), **kw)


def _mode(nets, mode='bf16x3'):
    """the precision class a graph is held to: the tower's mode, 'f32' without a tower"""
    return mode if DNN in nets else 'f32'


@pytest.mark.parametrize('nets,mode', NET_MODES, ids=[f'{_id(n)}-{m}' for n, m in NET_MODES])
def test_every_net_combination_matches_the_oracle_after_training(dev, monkeypatch, nets, mode):
    import tests.test_fused_gpu as T
    from deeptables_amd import fused
    monkeypatch.setenv('DT_AMD_TOWER_DTYPE', mode)
    dm, cats = _build(nets)
    _train_and_perturb(dm, cats, 13, dev)
    plan = dm.inference_plan()
    assert plan is not None, f'{nets} should take a fused inference plan'
    assert type(plan) is (fused.InferDeepFM if len(nets) == 3 else fused.InferStack)
    idx, dense, _ = T.batch(cats, 13, 300, seed=41)
    I._check(dm, idx, dense, dev, mode, f'infer_stack[{_id(nets)},{mode}]')


CORNER_NETS = [[DNN], [LIN, DNN], [LIN, FM]]
CORNER_POINTS = [(n, m, F, D, Nd, I.BATCHES[(i + k) % len(I.BATCHES)])
                 for k, n in enumerate(CORNER_NETS) for m in (['bf16x3', 'bf16'] if DNN in n else ['f32'])
                 for i, (F, D, Nd) in enumerate(I.DEEPFM_CORNERS)]


@pytest.mark.parametrize('nets,mode,F,D,Nd,B', CORNER_POINTS, ids=[f'{_id(p[0])}-{p[1]}-{p[2]}-{p[3]}-{p[4]}-{p[5]}' for p in CORNER_POINTS])
def test_inference_at_the_corners(dev, monkeypatch, nets, mode, F, D, Nd, B):
    """tests/test_infer_gpu.py's DEEPFM_CORNERS (F = 1, F = 127 / 128 at D = 4, D = 64, Nd = 0 / 64, CP = 576) against the
    oracle at its BATCHES (1, 2, 31, 33, 8193)"""
    import tests.test_fused_gpu as T
    monkeypatch.setenv('DT_AMD_TOWER_DTYPE', mode)
    dm, cats = _build(nets, F, D, Nd)
    _train_and_perturb(dm, cats, Nd, dev, steps=1)
    idx, dense, _ = T.batch(cats, Nd, B, seed=B)
    I._check(dm, idx, dense, dev, mode, f'infer_stack_corner[{_id(nets)},{mode},{F},{D},{Nd},{B}]')


@pytest.mark.parametrize('kind', ['int32', 'float32'])
@pytest.mark.parametrize('nets', [[DNN], [LIN, FM], [FM, DNN], [LIN]], ids=_id)
def test_out_of_range_and_fractional_ids(dev, monkeypatch, nets, kind):
    """as tests/test_infer_gpu.py::test_out_of_range_and_fractional_ids: an out-of-range id reads a zero row and is counted,
    a float id is truncated; the oracle gets a zero row appended to each table and the out-of-range ids pointed at it"""
    import tests.test_fused_gpu as T
    from oracle import bridge
    from tests.test_fused_domain_gpu import _odd_ids
    mode = _mode(nets)
    monkeypatch.setenv('DT_AMD_TOWER_DTYPE', mode)
    dm, cats = _build(nets, 26, 16, 13, vocab=60)
    _train_and_perturb(dm, cats, 13, dev, steps=1)
    idx, dense, _ = T.batch(cats, 13, 65, seed=17)
    ids, n_oob = _odd_ids(cats, idx, kind)
    trunc = ids.to(torch.int32).to(torch.int64)
    vocab = torch.tensor([c.vocabulary_size for c in cats])
    bad = (trunc < 0) | (trunc >= vocab)
    assert int(bad.sum()) == n_oob > 0
    ids_o = torch.where(bad, vocab.expand_as(trunc), trunc).to(torch.float32)

    def weights(dtype):
        w = bridge.oracle_weights(dm, dtype)
        w['emb_categorical_vars_all'] = [torch.cat([t, torch.zeros(1, t.shape[1], dtype=t.dtype)])
                                         for t in w['emb_categorical_vars_all']]
        return w
    emb = dm.model.layers_by_name['emb_categorical_vars_all']
    emb.check_oob = True
    emb.oob_count.zero_()
    try:
        I._check(dm, ids, dense, dev, mode, f'infer_stack_ids[{_id(nets)},{kind}]', kind=kind, weights=weights, ids_oracle=ids_o)
        torch.cuda.synchronize()
        assert int(emb.oob_count.item()) == n_oob
    finally:
        emb.check_oob = False


@pytest.mark.parametrize('variant', ['no_output_bias', 'regression'])
@pytest.mark.parametrize('nets', [[DNN], [LIN, DNN], [FM, DNN], [LIN, FM], [LIN], [FM]], ids=_id)
def test_head_variants(dev, monkeypatch, nets, variant):
    """output_use_bias=False; the regression task, whose output is the logit bit for bit (I._check asserts torch.equal)"""
    import tests.test_fused_gpu as T
    mode = _mode(nets)
    monkeypatch.setenv('DT_AMD_TOWER_DTYPE', mode)
    kw = {'no_output_bias': dict(use_bias=False), 'regression': dict(task='regression')}[variant]
    dm, cats = _build(nets, **kw)
    assert (dm.model.layers_by_name['task_output'].bias is None) == (variant == 'no_output_bias')
    _train_and_perturb(dm, cats, 13, dev, steps=2)
    idx, dense, _ = T.batch(cats, 13, 70, seed=8)
    logit, out = I._check(dm, idx, dense, dev, mode, f'infer_stack_head[{_id(nets)},{variant}]')
    if variant == 'regression':
        assert torch.equal(out, logit)


@pytest.mark.parametrize('nets', [[DNN], [LIN, DNN]], ids=_id)
@pytest.mark.parametrize('hidden', [((128, 0.3, False), (64, 0.5, False)), ((64, 0, True), (32, 0, False)),
                                    ((128, 0.2, True), (64, 0, True)), ((3, 0, False), (2, 0, False))])
def test_tower_cells_with_dropout_and_batch_norm(dev, monkeypatch, nets, hidden):
    """dropout is the identity at inference, a use_bn cell is a per-column affine map over its (perturbed) moving
    statistics; a narrow tower; embedding_dropout / dense_dropout > 0 are ignored as well"""
    import tests.test_fused_gpu as T
    monkeypatch.setenv('DT_AMD_TOWER_DTYPE', 'bf16x3')
    dm, cats = _build(nets, hidden=hidden, embedding_dropout=0.3, dense_dropout=0.4)
    _train_and_perturb(dm, cats, 13, dev, steps=2)
    idx, dense, _ = T.batch(cats, 13, 97, seed=3)
    I._check(dm, idx, dense, dev, 'bf16x3', f'infer_stack_tower[{_id(nets)},{hidden}]')


@pytest.mark.parametrize('nets', [[DNN], [LIN, DNN], [LIN, FM], [FM]], ids=_id)
def test_predictions_are_row_independent_and_match_the_layer_path(dev, monkeypatch, nets):
    """predict is bit-identical across batch sizes 7 / 128 / 8192 and across two calls; predict / evaluate agree with the
    layer path (DT_AMD_FUSED_PREDICT=0) at the bars of tests/test_infer_gpu.py::test_fit_predict_evaluate_against_the_layer_path"""
    monkeypatch.setenv('DT_AMD_TOWER_DTYPE', 'bf16x3')
    dm, cats = _build(nets)
    _train_and_perturb(dm, cats, 13, dev)
    df, y = _frame(cats, 13, 9000, 4)
    p1 = dm.predict(df, batch_size=128)
    p2 = dm.predict(df, batch_size=128)
    p7 = dm.predict(df, batch_size=7)
    pbig = dm.predict(df, batch_size=8192)
    assert np.array_equal(p1, p2) and np.array_equal(p1, p7) and np.array_equal(p1, pbig)
    e1 = dm.evaluate(df, y, batch_size=256)
    monkeypatch.setenv('DT_AMD_FUSED_PREDICT', '0')
    assert dm.inference_plan() is None
    q = dm.predict(df, batch_size=128)
    e0 = dm.evaluate(df, y, batch_size=256)
    assert np.abs(p1 - q).max() <= 1e-5, np.abs(p1 - q).max()
    for k in e0:
        assert abs(e1[k] - e0[k]) <= 1e-6 * max(1.0, abs(e0[k])), (k, e1[k], e0[k])


@pytest.mark.parametrize('nets', [None, [LIN, FM]], ids=['default', 'FM'])
def test_the_layer_path_is_not_run(dev, monkeypatch, nets):
    """predict and evaluate with model.forward patched to raise: ModelConfig's default nets (['dnn_nets']) and the FM model"""
    from deeptables_amd.models import ModelConfig
    if nets is None:
        nets = ModelConfig().nets
        assert nets == [DNN]
    dm, cats = _build(nets)
    df, y = _frame(cats, 13, 300, 2)

    def boom(*a, **k):
        raise AssertionError('the layer-by-layer forward ran')
    monkeypatch.setattr(dm.model, 'forward', boom)
    p = dm.predict(df, batch_size=128)
    assert p.shape == (300, 1) and np.isfinite(p).all()
    res = dm.evaluate(df, y, batch_size=64)
    assert np.isfinite(res['loss'])


def test_deeptable_end_to_end_with_the_default_config(dev, monkeypatch):
    """DeepTable(config=ModelConfig()) — the bare default, nothing changed: nets ['dnn_nets'], one embedding group of width
    4, embedding_dropout 0.3 — fit -> predict_proba / predict / evaluate: the inference plan and its DT_AMD_FUSED_PREDICT=0
    twin agree at the bars of tests/test_infer_gpu.py::test_deeptable_end_to_end"""
    import pandas as pd
    from deeptables_amd import fused
    from deeptables_amd.models import DeepTable, ModelConfig
    rng = np.random.default_rng(0)
    n = 3000
    df = pd.DataFrame({'job': rng.choice(['admin', 'tech', 'services', 'retired'], n), 'marital': rng.choice(['m', 's', 'd'], n),
                       'city': rng.choice([f'c{i}' for i in range(40)], n),
                       'age': rng.integers(18, 80, n).astype(np.float32), 'balance': rng.normal(1000, 500, n).astype(np.float32)})
    y = ((df['age'] > 50) ^ (df['job'] == 'tech')).map({True: 'yes', False: 'no'})
    dt = DeepTable(config=ModelConfig())
    dt.fit(df, y, batch_size=128, epochs=2, verbose=0)
    assert dt.model.model is not None
    assert type(dt.model.inference_plan()) is fused.InferStack, 'DeepTable\'s default graph should take the inference plan'
    pr1, pd1, ev1 = dt.predict_proba(df), dt.predict(df), dt.evaluate(df, y)
    monkeypatch.setenv('DT_AMD_FUSED_PREDICT', '0')
    pr0, pd0, ev0 = dt.predict_proba(df), dt.predict(df), dt.evaluate(df, y)
    assert np.abs(pr1 - pr0).max() <= 1e-5
    assert (pd1 == pd0).mean() >= 0.999
    for k in ev0:
        assert abs(ev1[k] - ev0[k]) <= 1e-6 * max(1.0, abs(ev0[k])), (k, ev1[k], ev0[k])


def test_deepfm_and_dcn_keep_their_plans(dev):
    from deeptables_amd import fused
    dm, _ = I._build('DeepFM')
    assert type(dm.inference_plan()) is fused.InferDeepFM
    dm, _ = I._build('DCN')
    assert type(dm.inference_plan()) is fused.InferDCN
