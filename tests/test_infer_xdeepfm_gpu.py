# -*- coding:utf-8 -*-
"""GPU: the fused xDeepFM inference plan (fused.InferXDeepFM: one prepare call per predict / evaluate, then per batch the
tower launch that also emits x0 and the partial logit, one CIN layer kernel per layer on a filter packed once, the head
launch; csrc/infer_x3.h, csrc/cin_bf16.hip) against the float64 oracle at inference, against the layer-by-layer path on
the same trained model, against the reference code's own xDeepFM fixtures, and for row independence and out-of-range
ids."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import precision as P
from tests.infer_support import _frame, _oracle, _train_and_perturb, run_plan

pytestmark = pytest.mark.gpu

ORDER = {'fp32': 0, 'b17': 1, 'bf16': 2}
CIN_NAME = {'float32': 'float32', 'bf16x3': 'bf16x3', 'bf16': 'bf16'}


def _build(F=26, D=16, Nd=13, cross=(128, 128), direct=False, vocab=30, cin_mode=None, **kw):
    import tests.test_fused_gpu as T
    from deeptables_amd.models import deepnets
    cin = {'cross_layer_size': tuple(cross), 'direct': direct, **kw.pop('cin', {})}
    if cin_mode is not None:
        cin['mfma_dtype'] = cin_mode
    return T.build(F, Nd, D, vocab=vocab, nets=kw.pop('nets', deepnets.xDeepFM), cin_params=cin, **kw)


def _weaker(cin_mode, tower_mode):
    """the (kernel, mode) pair of tests/precision.py CLAIMS whose forward class is the weaker of the CIN's and the tower's:
    the plan's logit is their sum, so it is held to that class"""
    a, b = ('cin', CIN_NAME[cin_mode]), ('tower', tower_mode)
    return a if ORDER[P.bar_of(*a, 'fwd')] >= ORDER[P.bar_of(*b, 'fwd')] else b


def _run_plan(dm, idx, dense, dev, kind='int32'):
    from deeptables_amd import fused
    return run_plan(dm, idx, dense, dev, fused.InferXDeepFM, kind)


def _check(dm, idx, dense, dev, cin_mode, tower_mode, label, kind='int32', weights=None, ids_oracle=None):
    logit, out = _run_plan(dm, idx, dense, dev, kind)
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
    print(label, {k: (g, f) for k, (_, g, f) in figs.items()})
    P.check_step(label, *_weaker(cin_mode, tower_mode), figs)
    return logit, out


@pytest.mark.parametrize('D', [4, 16])
@pytest.mark.parametrize('Nd', [13, 0])
@pytest.mark.parametrize('cross', [(128, 128), (64, 32, 16)], ids=['128x128', '64x32x16'])
@pytest.mark.parametrize('direct', [False, True])
def test_plan_matches_the_oracle_after_training(dev, monkeypatch, direct, cross, Nd, D):
    import tests.test_fused_gpu as T
    monkeypatch.setenv('DT_AMD_TOWER_DTYPE', 'bf16x3')
    dm, cats = _build(D=D, Nd=Nd, cross=cross, direct=direct)
    _train_and_perturb(dm, cats, Nd, dev, steps=2)
    idx, dense, _ = T.batch(cats, Nd, 203, seed=41)
    _check(dm, idx, dense, dev, 'bf16x3', 'bf16x3', f'xdeepfm[{direct},{cross},{Nd},{D}]')


@pytest.mark.parametrize('direct', [False, True])
def test_regression_task(dev, monkeypatch, direct):
    import tests.test_fused_gpu as T
    monkeypatch.setenv('DT_AMD_TOWER_DTYPE', 'bf16x3')
    dm, cats = _build(direct=direct, task='regression')
    _train_and_perturb(dm, cats, 13, dev, steps=2)
    idx, dense, _ = T.batch(cats, 13, 70, seed=8)
    _check(dm, idx, dense, dev, 'bf16x3', 'bf16x3', f'xdeepfm_regression[{direct}]')


@pytest.mark.parametrize('cin_mode,tower_mode', [('float32', 'f32'), ('bf16', 'bf16x3'), ('bf16x3', 'bf16'), ('bf16', 'bf16')])
def test_every_precision_mode_runs_its_own_kernel(dev, monkeypatch, cin_mode, tower_mode):
    """the three CIN modes and the tower's bf16 mode, each held to the class tests/precision.py gives it; a CIN bias, a
    sigmoid CIN activation and no output bias ride along"""
    import tests.test_fused_gpu as T
    monkeypatch.setenv('DT_AMD_TOWER_DTYPE', tower_mode)
    dm, cats = _build(cross=(64, 32, 16), cin_mode=cin_mode, cin={'use_bias': True, 'activation': 'sigmoid'}, use_bias=False)
    _train_and_perturb(dm, cats, 13, dev, steps=2)
    assert dm.inference_plan().cin.mfma_dtype == cin_mode
    idx, dense, _ = T.batch(cats, 13, 130, seed=5)
    _check(dm, idx, dense, dev, cin_mode, tower_mode, f'xdeepfm_modes[{cin_mode},{tower_mode}]')


def test_packed_forward_is_the_layer_kernels_bit_for_bit(dev):
    """dt_cin_pack + dt_cin_layer_fwd_packed against dt_cin_layer_fwd / _bf16 / _bf16x3 (ops.cin_layer) on the same inputs,
    for a narrow and a wide batch (the forward picks its block shape by B D) and a strided x_k"""
    from deeptables_amd import _lib, ops
    from deeptables_amd._lib import check, lib, ptr, stream_ptr
    g = torch.Generator().manual_seed(2)
    F0, Hk, L, D = 26, 64, 128, 16
    W = (torch.randn(F0 * Hk, L, generator=g) * 0.05).to(dev)
    bias = (torch.randn(L, generator=g) * 0.1).to(dev)
    for B in (37, 2100):
        x0 = torch.randn(B, F0, D, generator=g).to(dev)
        prev = torch.randn(B, 2 * Hk, D, generator=g).to(dev)
        xk = prev[:, :Hk]
        for mode, name in ((_lib.DT_CIN_F32, 'float32'), (_lib.DT_CIN_BF16, 'bf16'), (_lib.DT_CIN_BF16X3, 'bf16x3')):
            want = ops.cin_layer(x0, xk, W, bias, 'relu', name)
            packed = torch.empty(lib().dt_cin_packed_bytes(mode, F0, Hk, L) // 4, dtype=torch.float32, device=dev)
            y = torch.empty((B, L, D), dtype=torch.float32, device=dev)
            check(lib().dt_cin_pack(mode, ptr(W), F0, Hk, L, ptr(packed), stream_ptr()), 'dt_cin_pack')
            check(lib().dt_cin_layer_fwd_packed(mode, ptr(x0), ptr(xk), ptr(packed), ptr(bias), _lib.act_code('relu', 'CIN'), B,
                                                F0, Hk, L, D, F0 * D, xk.stride(0), ptr(y), stream_ptr()),
                  'dt_cin_layer_fwd_packed')
            torch.cuda.synchronize()
            assert torch.equal(y, want), (B, name, (y - want).abs().max().item())


@pytest.mark.parametrize('kind', ['int32', 'float32'])
def test_out_of_range_and_fractional_ids(dev, monkeypatch, kind):
    """an out-of-range id reads a zero row in the tower AND in the CIN's x0, and is counted once per lookup.  The oracle gets
    a zero row appended to each table and the out-of-range ids pointed at it."""
    import tests.test_fused_gpu as T
    from oracle import bridge
    from tests.test_fused_domain_gpu import _odd_ids
    monkeypatch.setenv('DT_AMD_TOWER_DTYPE', 'bf16x3')
    dm, cats = _build(vocab=60)
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
        _check(dm, ids, dense, dev, 'bf16x3', 'bf16x3', f'xdeepfm_ids[{kind}]', kind=kind, weights=weights, ids_oracle=ids_o)
        torch.cuda.synchronize()
        assert int(emb.oob_count.item()) == n_oob
    finally:
        emb.check_oob = False


def test_the_layer_path_is_not_run(dev, monkeypatch):
    dm, cats = _build()
    df, y = _frame(cats, 13, 300, 2)

    def boom(*a, **k):
        raise AssertionError('the layer-by-layer forward ran')
    monkeypatch.setattr(dm.model, 'forward', boom)
    p = dm.predict(df, batch_size=128)
    assert p.shape == (300, 1) and np.isfinite(p).all()
    res = dm.evaluate(df, y, batch_size=64)
    assert np.isfinite(res['loss'])


def test_fit_predict_evaluate_against_the_layer_path(dev, monkeypatch):
    """DeepModel.fit with a validation split (its validation pass runs the plan), then predict / evaluate with the plan and
    with DT_AMD_FUSED_PREDICT=0 (the layer path, which runs the same CIN kernels) on the same trained model: 1e-5 on the
    outputs, 1e-6 relative on evaluate's metrics; predictions row-independent (two calls and batch sizes 7 / 128 / 8192
    bit-identical — the 7-row and the ragged last batches run the tile tails)"""
    monkeypatch.setenv('DT_AMD_TOWER_DTYPE', 'bf16x3')
    dm, cats = _build()
    df, y = _frame(cats, 13, 3000, 4)
    hist = dm.fit(df, y, batch_size=256, epochs=2, verbose=0, validation_split=0.2)
    assert 'val_loss' in hist.history
    p1 = dm.predict(df, batch_size=128)
    p2 = dm.predict(df, batch_size=128)
    p7 = dm.predict(df, batch_size=7)
    pbig = dm.predict(df, batch_size=8192)
    assert np.array_equal(p1, p2), 'two calls differ'
    assert np.array_equal(p1, p7), np.abs(p1 - p7).max()
    assert np.array_equal(p1, pbig), np.abs(p1 - pbig).max()
    e1 = dm.evaluate(df, y, batch_size=256)
    monkeypatch.setenv('DT_AMD_FUSED_PREDICT', '0')
    assert dm.inference_plan() is None
    q = dm.predict(df, batch_size=128)
    e0 = dm.evaluate(df, y, batch_size=256)
    print('plan vs layer path: max |dp| =', np.abs(p1 - q).max(), {k: (e1[k], e0[k]) for k in e0})
    assert np.abs(p1 - q).max() <= 1e-5, np.abs(p1 - q).max()
    for k in e0:
        assert abs(e1[k] - e0[k]) <= 1e-6 * max(1.0, abs(e0[k])), (k, e1[k], e0[k])


@pytest.mark.parametrize('direct', [False, True])
def test_row_independence_across_batch_sizes(dev, monkeypatch, direct):
    """logits bit-identical for batch sizes 7, 128 and 8192 over 9000 rows (8192 + a ragged 808-row batch: the CIN forward
    picks its wide blocks there and its narrow ones for the small batches)"""
    dm, cats = _build(direct=direct, cross=(64, 32, 16) if direct else (128, 128))
    _train_and_perturb(dm, cats, 13, dev, steps=1)
    df, _ = _frame(cats, 13, 9000, 6)
    a = dm.predict(df, batch_size=8192)
    b = dm.predict(df, batch_size=128)
    c = dm.predict(df.iloc[:1500], batch_size=7)
    assert np.array_equal(a, b), np.abs(a - b).max()
    assert np.array_equal(a[:1500], c), np.abs(a[:1500] - c).max()


@pytest.mark.parametrize('tag', ['xdeepfm', 'xdeepfm_d16'])
def test_reference_code_fixture(dev, tag):
    """tests/golden/reference_code_model_<tag>.npz: the output of the reference's own xDeepFM graph (deepmodel.py / deepnets.py /
    layers.py imported unmodified, float64).  First the mode of the recorded forward is established: the drop-in model's
    layer path in inference mode on the fixture's weights either reproduces it (an inference-mode recording) or does not.
    It does not: tests/golden/make_reference_golden.py records TRAINING-mode forwards (its BatchNormalization normalises with
    the statistics of the fixture's batch, and the fixture holds no moving statistics).  A training-mode BatchNormalization
    over one batch IS the inference-mode one whose moving mean / variance are that batch's mean / biased variance, so those
    are computed from the fixture's own inputs and embedding tables (float64) and stored as bn_concat_emb_dense's moving
    statistics — the only BatchNormalization of this graph; the tower cells have none.  The plan must then reproduce the
    recorded logit and output at the bar tests/test_reference_models_gpu.py holds the layer path to for this fixture: 1e-4,
    relative to the logit scale above 1."""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_oracle_reference_code import GOLDEN as GOLDEN_DIR, load_model_fixture
    from oracle import bridge          # only its weight loader
    from deeptables_amd import fused
    meta, tensors, want = load_model_fixture(os.path.join(GOLDEN_DIR, f'reference_code_model_{tag}.npz'))
    dm, ids, dense = bridge.model_from_reference_fixture(meta['static'], tensors, dev)
    assert list(dm.config.nets) == ['linear', 'cin_nets', 'dnn_nets']
    assert [n for n, l in dm.model.layers_by_name.items() if hasattr(l, 'moving_mean')] == ['bn_concat_emb_dense']
    tol = 1e-4 * max(1.0, want.abs().max().item())
    inputs = [ids.to(dev)] + ([] if dense is None else [dense.to(dev)])

    def layer_path_eval():
        dm.model.eval()
        with torch.no_grad():
            logit = dm.model(inputs)
            return torch.cat([logit, dm._activate(logit)], -1).double().cpu()

    recorded_in_inference_mode = (layer_path_eval() - want).abs().max().item() < tol
    print(tag, 'recorded in inference mode:', recorded_in_inference_mode)
    if not recorded_in_inference_mode:
        tables = tensors['weights']['emb_categorical_vars_all']
        rows = [torch.as_tensor(t).double()[ids[:, f].long()] for f, t in enumerate(tables)]
        x = torch.cat(rows + ([] if dense is None else [dense.double()]), 1)
        bn = dm.model.layers_by_name['bn_concat_emb_dense']
        with torch.no_grad():
            bn.moving_mean.copy_(x.mean(0).float().to(dev))
            bn.moving_variance.copy_(x.var(0, unbiased=False).float().to(dev))
        err = (layer_path_eval() - want).abs().max().item()
        assert err < tol, f'the inference-mode layer path on the batch statistics: {err:.3e}'
    plan = dm.inference_plan()
    assert type(plan) is fused.InferXDeepFM
    B = ids.shape[0]
    logit = torch.empty((B, 1), dtype=torch.float32, device=dev)
    out = torch.empty_like(logit)
    plan.prepare()
    plan.infer(inputs[0], inputs[1] if len(inputs) > 1 else None, logit, out)
    torch.cuda.synchronize()
    got = torch.cat([logit, out], -1).double().cpu()
    err = (got - want).abs().max().item()
    print(tag, 'plan vs reference code:', err, 'tolerance', tol)
    assert err < tol, f'reference_code_model_{tag}: |plan - reference code| = {err:.3e} (tolerance {tol:.1e})'
