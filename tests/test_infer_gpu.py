# -*- coding:utf-8 -*-
"""GPU: the fused DeepFM / DCN inference plans (fused.InferDeepFM / InferDCN: one k_infer_prep launch per call, one k_infer
launch per batch, csrc/infer_x3.h) against the float64 oracle at inference (moving statistics, no dropout), held to the
tower mode's forward class (tests/precision.py), at the corners of the accepted domain, with odd ids and the tower shapes
only inference takes; and end to end through fit / predict / evaluate against the layer-by-layer path."""
import numpy as np
import pytest
import torch

from tests import precision as P
from tests.infer_support import _frame, _oracle, _train_and_perturb, run_plan

pytestmark = pytest.mark.gpu


def _build(net, F=26, D=16, Nd=13, L=3, vocab=30, hidden=None, **kw):
    import tests.test_fused_gpu as T
    from deeptables_amd.models import deepnets
    if net == 'DCN':
        kw.update(nets=deepnets.DCN, cross_params={'num_cross_layer': L})
    if hidden is not None:
        kw['dnn_params'] = {'hidden_units': hidden, 'activation': 'relu'}
    elif net == 'DCN':
        kw['dnn_params'] = {'hidden_units': ((128, 0, False), (64, 0, False)), 'activation': 'relu'}
    dm, cats = T.build(F, Nd, D, vocab=vocab, **kw)
    if net == 'DCN':
        g = torch.Generator().manual_seed(11)
        with torch.no_grad():
            cr = dm.model.layers_by_name['dcn_cross_layer']
            cr.bias_stack.add_(torch.randn(cr.bias_stack.shape, generator=g).to(cr.bias_stack.device) * 0.05)
    return dm, cats


def _check(dm, idx, dense, dev, mode, label, kind='int32', weights=None, ids_oracle=None):
    logit, out = run_plan(dm, idx, dense, dev, None, kind)
    ids_o = idx if ids_oracle is None else ids_oracle
    w64 = weights(torch.float64) if weights else None
    w32 = weights(torch.float32) if weights else None
    r64 = _oracle(dm, ids_o, dense, torch.float64, w64)
    r32 = _oracle(dm, ids_o, dense, torch.float32, w32)
    figs = {'logit': ('fwd', P.max_rel(logit, r64), P.max_rel(r32, r64))}
    if dm.output_activation == 'sigmoid':
        figs['prob'] = ('fwd', P.max_rel(out, torch.sigmoid(r64)), P.max_rel(torch.sigmoid(r32.double()), torch.sigmoid(r64)))
    else:
        assert torch.equal(out, logit)
    P.check_step(label, 'tower', mode, figs)
    return logit, out


MODES = ['f32', 'bf16x3', 'bf16']


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('net', ['DeepFM', 'DCN'])
def test_inference_matches_the_oracle_after_training(dev, monkeypatch, net, mode):
    import tests.test_fused_gpu as T
    monkeypatch.setenv('DT_AMD_TOWER_DTYPE', mode)
    dm, cats = _build(net)
    _train_and_perturb(dm, cats, 13, dev)
    assert dm.fused_plan() is not None           # the tower lives in the training plan's slabs now (strided views)
    idx, dense, _ = T.batch(cats, 13, 300, seed=41)
    _check(dm, idx, dense, dev, mode, f'infer[{net},{mode}]')


DEEPFM_CORNERS = [(8, 64, 0), (7, 64, 64), (1, 4, 0), (1, 4, 64), (127, 4, 0), (128, 4, 32), (32, 16, 32)]
DCN_CORNERS = [(32, 16, 0, 8), (7, 64, 0, 8), (128, 4, 0, 8), (1, 4, 0, 1), (1, 4, 64, 2), (32, 16, 32, 8)]
BATCHES = [1, 2, 31, 33, 8193]
CORNER_POINTS = ([('DeepFM', F, D, Nd, None, BATCHES[i % len(BATCHES)]) for i, (F, D, Nd) in enumerate(DEEPFM_CORNERS)] +
                 [('DCN', F, D, Nd, L, BATCHES[(i + 2) % len(BATCHES)]) for i, (F, D, Nd, L) in enumerate(DCN_CORNERS)])


@pytest.mark.parametrize('mode', ['bf16x3', 'bf16'])
@pytest.mark.parametrize('net,F,D,Nd,L,B', CORNER_POINTS)
def test_inference_at_the_corners(dev, monkeypatch, mode, net, F, D, Nd, L, B):
    """D = 64, Nd = 0 / 64, F = 1, F = 127 / 128 at D = 4, C = 544 (CP = 576: the split tile serves it at inference), DCN at
    L = 8 up to CP = 576, against the oracle at B in {1, 2, 31, 33, 8193}"""
    import tests.test_fused_gpu as T
    monkeypatch.setenv('DT_AMD_TOWER_DTYPE', mode)
    dm, cats = _build(net, F, D, Nd, L or 1)
    _train_and_perturb(dm, cats, Nd, dev, steps=1)
    idx, dense, _ = T.batch(cats, Nd, B, seed=B)
    _check(dm, idx, dense, dev, mode, f'infer_corner[{mode},{net},{F},{D},{Nd},{L},{B}]')


@pytest.mark.parametrize('kind', ['int32', 'float32'])
@pytest.mark.parametrize('net', ['DeepFM', 'DCN'])
def test_out_of_range_and_fractional_ids(dev, monkeypatch, net, kind):
    """an out-of-range id reads a zero row and is counted; a float id is truncated (layers.py:893-895).  The oracle gets a
    zero row appended to each table and the out-of-range ids pointed at it."""
    import tests.test_fused_gpu as T
    from oracle import bridge
    from tests.test_fused_domain_gpu import _odd_ids
    monkeypatch.setenv('DT_AMD_TOWER_DTYPE', 'bf16x3')
    dm, cats = _build(net, 26, 16, 13, 4, vocab=60)
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
        _check(dm, ids, dense, dev, 'bf16x3', f'infer_ids[{net},{kind}]', kind=kind, weights=weights, ids_oracle=ids_o)
        torch.cuda.synchronize()
        assert int(emb.oob_count.item()) == n_oob
    finally:
        emb.check_oob = False


@pytest.mark.parametrize('net', ['DeepFM', 'DCN'])
@pytest.mark.parametrize('hidden,plan_first', [(((100, 0, False), (40, 0, False)), False),
                                               (((100, 0, False), (40, 0, False)), True),
                                               (((3, 0, False), (2, 0, False)), True),
                                               (((128, 0.3, False), (64, 0.5, False)), False),
                                               (((64, 0, True), (32, 0, False)), False),
                                               (((128, 0.2, True), (64, 0, True)), False)])
def test_tower_shapes(dev, monkeypatch, net, hidden, plan_first):
    """narrow towers, before and after the training plan re-homed them into its slabs; dropout and batch-norm cells (the
    training plan refuses them: trained here on the layer path, the moving statistics of every BN then perturbed)"""
    import tests.test_fused_gpu as T
    monkeypatch.setenv('DT_AMD_TOWER_DTYPE', 'bf16x3')
    dm, cats = _build(net, hidden=hidden)
    if plan_first:
        assert dm.fused_plan() is not None
    _train_and_perturb(dm, cats, 13, dev, steps=2)
    idx, dense, _ = T.batch(cats, 13, 97, seed=3)
    _check(dm, idx, dense, dev, 'bf16x3', f'infer_tower[{net},{hidden},{plan_first}]')


@pytest.mark.parametrize('net', ['DeepFM', 'DCN'])
@pytest.mark.parametrize('variant', ['no_output_bias', 'regression', 'dropouts'])
def test_head_variants_and_ignored_dropouts(dev, monkeypatch, net, variant):
    """output_use_bias=False; the regression task (identity output); embedding_dropout / dense_dropout > 0, which must be
    ignored at inference"""
    import tests.test_fused_gpu as T
    monkeypatch.setenv('DT_AMD_TOWER_DTYPE', 'bf16x3')
    kw = {'no_output_bias': dict(use_bias=False), 'regression': dict(task='regression'),
          'dropouts': dict(embedding_dropout=0.3, dense_dropout=0.4)}[variant]
    dm, cats = _build(net, **kw)
    _train_and_perturb(dm, cats, 13, dev, steps=2)
    idx, dense, _ = T.batch(cats, 13, 70, seed=8)
    _check(dm, idx, dense, dev, 'bf16x3', f'infer_head[{net},{variant}]')


@pytest.mark.parametrize('net', ['DeepFM', 'DCN'])
def test_the_layer_path_is_not_run(dev, monkeypatch, net):
    dm, cats = _build(net)
    df, y = _frame(cats, 13, 300, 2)

    def boom(*a, **k):
        raise AssertionError('the layer-by-layer forward ran')
    monkeypatch.setattr(dm.model, 'forward', boom)
    p = dm.predict(df, batch_size=128)
    assert p.shape == (300, 1) and np.isfinite(p).all()
    res = dm.evaluate(df, y, batch_size=64)
    assert np.isfinite(res['loss'])


@pytest.mark.parametrize('net', ['DeepFM', 'DCN'])
def test_fit_predict_evaluate_against_the_layer_path(dev, monkeypatch, net):
    """DeepModel.fit with a validation split (its validation pass runs the plan), then predict / evaluate with the plan and
    with DT_AMD_FUSED_PREDICT=0 (the layer path) on the same trained model: within the fp32 class, metrics to 1e-6;
    predictions row-independent (two calls and batch sizes 7 / 8192 bit-identical)"""
    monkeypatch.setenv('DT_AMD_TOWER_DTYPE', 'bf16x3')
    dm, cats = _build(net)
    df, y = _frame(cats, 13, 3000, 4)
    hist = dm.fit(df, y, batch_size=256, epochs=2, verbose=0, validation_split=0.2)
    assert 'val_loss' in hist.history
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


def test_deeptable_end_to_end(dev, monkeypatch):
    """DeepTable.fit -> predict_proba / predict / evaluate: the inference plan and its DT_AMD_FUSED_PREDICT=0 twin agree"""
    import pandas as pd
    from deeptables_amd.models import DeepTable, ModelConfig, deepnets
    rng = np.random.default_rng(0)
    n = 3000
    df = pd.DataFrame({'job': rng.choice(['admin', 'tech', 'services', 'retired'], n), 'marital': rng.choice(['m', 's', 'd'], n),
                       'city': rng.choice([f'c{i}' for i in range(40)], n),
                       'age': rng.integers(18, 80, n).astype(np.float32), 'balance': rng.normal(1000, 500, n).astype(np.float32)})
    y = ((df['age'] > 50) ^ (df['job'] == 'tech')).map({True: 'yes', False: 'no'})
    conf = ModelConfig(nets=deepnets.DeepFM, metrics=["AUC", "accuracy"], earlystopping_patience=0, fixed_embedding_dim=True,
                       embeddings_output_dim=8)
    dt = DeepTable(config=conf)
    dt.fit(df, y, batch_size=128, epochs=2, verbose=0)
    assert dt.model.model is not None
    if dt.model.inference_plan() is None:
        pytest.fail('DeepTable\'s DeepFM graph should take the inference plan')
    pr1, pd1, ev1 = dt.predict_proba(df), dt.predict(df), dt.evaluate(df, y)
    monkeypatch.setenv('DT_AMD_FUSED_PREDICT', '0')
    pr0, pd0, ev0 = dt.predict_proba(df), dt.predict(df), dt.evaluate(df, y)
    assert np.abs(pr1 - pr0).max() <= 1e-5
    assert (pd1 == pd0).mean() >= 0.999
    for k in ev0:
        assert abs(ev1[k] - ev0[k]) <= 1e-6 * max(1.0, abs(ev0[k])), (k, ev1[k], ev0[k])
