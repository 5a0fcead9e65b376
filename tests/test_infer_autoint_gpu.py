# -*- coding:utf-8 -*-
"""GPU: the fused AutoInt inference plan (fused.InferAutoInt: one dt_autoint_infer_prepare launch per predict / evaluate, one
k_autoint_infer launch per batch — gather, every interacting layer with its inference BatchNormalization, Flatten, task_output,
the activation; csrc/autoint.hip) against the float64 oracle at inference, held to the forward class tests/precision.py gives
the interacting layer's mode; over every (D, d_h) instantiation, both sides of the 16-row tile, one layer and the most the
LDS holds, all three precision modes; the grid stride and its two-deep prefetch; row independence; odd ids; and end to end
through fit / predict / evaluate against the layer-by-layer path."""
import numpy as np
import pytest
import torch

from tests import precision as P
from tests.infer_support import _frame, _oracle, _train_and_perturb, run_plan

pytestmark = pytest.mark.gpu

# the launch's grid is at most DT_AUTOINT_INFER_MAX_BLOCKS = 256 blocks; at D = 32 with three layers a block has 6 waves
# (include/dt_hip.h), so 1536 rows are resident at once.  3203 rows = two full passes of every wave plus a third of 131 waves:
# rows of the second and third pass come out of the prefetch chain (table rows one pass ahead, ids two).
B_BIG = 2 * 256 * 6 + 131


def _build(F=26, D=32, H=4, layers=3, Nd=0, mode=None, residual=True, vocab=30, **kw):
    import tests.test_fused_gpu as T
    from deeptables_amd.models import deepnets
    ap = {'num_attention': layers, 'num_heads': H, 'dropout_rate': 0, 'use_residual': residual}
    if mode is not None:
        ap['mfma_dtype'] = mode
    return T.build(F, Nd, D, vocab=vocab, nets=deepnets.AutoInt, autoint_params=ap, **kw)


def _mode_name(dm, D):
    """the (kernel, mode) name of tests/precision.py CLAIMS for the mode the plan runs"""
    from deeptables_amd import _lib, ops
    code = ops.autoint_mfma_mode(dm.config.autoint_params.get('mfma_dtype'), D)
    return {_lib.DT_AI_F32: 'float32', _lib.DT_AI_BF16X2: 'bf16x2', _lib.DT_AI_BF16: 'bf16'}[code]


def _run_plan(dm, idx, dense, dev, kind='int32'):
    from deeptables_amd import fused
    return run_plan(dm, idx, dense, dev, fused.InferAutoInt, kind)


def _check(dm, idx, dense, dev, label, kind='int32', weights=None, ids_oracle=None):
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
    mode = _mode_name(dm, dm.inference_plan().D)
    print(label, mode, {k: (g, f) for k, (_, g, f) in figs.items()})
    P.check_step(label, 'autoint', mode, figs)
    return logit, out


def _max_layers(D, H, F=26):
    from deeptables_amd import _lib
    lib = _lib.lib()
    return max(n for n in range(1, _lib.DT_AUTOINT_INFER_MAX_LAYERS + 1) if lib.dt_autoint_infer_supported(F, D, H, n, 1, 0))


# every (D, d_h) instantiation; F = one field, both sides of the 16-row MFMA tile (17 with both D), the benchmark's 26, the
# maximum 32; 1 and 3 layers and ('max') the most the predicate accepts at D = 32
PARITY = [(16, 1, 1, 1), (16, 2, 16, 3), (16, 4, 17, 1), (16, 2, 32, 3), (32, 2, 17, 3), (32, 4, 26, 3), (32, 4, 32, 1),
          (32, 2, 16, 'max')]


@pytest.mark.parametrize('D,H,F,layers', PARITY)
def test_plan_matches_the_oracle_after_training(dev, D, H, F, layers):
    import tests.test_fused_gpu as T
    if layers == 'max':
        layers = _max_layers(D, H)
        assert layers == 5                      # include/dt_hip.h: D = 32 takes up to 5 layers
    dm, cats = _build(F=F, D=D, H=H, layers=layers)
    _train_and_perturb(dm, cats, 0, dev, steps=2)
    assert dm.inference_plan().n_layers == layers
    idx, dense, _ = T.batch(cats, 0, 203, seed=41)
    _check(dm, idx, dense, dev, f'autoint_infer[{D},{H},{F},{layers}]')


@pytest.mark.parametrize('mode,variant', [('float32', 'no_residual'), ('bf16x2', 'no_output_bias'), ('bf16', 'plain')])
def test_every_precision_mode_runs_its_own_kernel(dev, mode, variant):
    """D = 32: exact fp32, three-part and two-part split-bf16 projections, each held to its own forward class;
    use_residual=False (NP = 3) rides on the first, no output bias on the second"""
    import tests.test_fused_gpu as T
    from deeptables_amd import _lib
    dm, cats = _build(F=13, D=32, H=4, layers=2, mode=mode, residual=variant != 'no_residual',
                      use_bias=variant != 'no_output_bias')
    _train_and_perturb(dm, cats, 0, dev, steps=2)
    idx, dense, _ = T.batch(cats, 0, 203, seed=5)
    _check(dm, idx, dense, dev, f'autoint_infer_modes[{mode},{variant}]')
    plan = dm.inference_plan()
    assert plan.mode == {'float32': _lib.DT_AI_F32, 'bf16x2': _lib.DT_AI_BF16X2, 'bf16': _lib.DT_AI_BF16}[mode]
    assert plan.NP == (3 if variant == 'no_residual' else 4)
    assert (dm.model.layers_by_name['task_output'].bias is None) == (variant == 'no_output_bias')


def test_regression_task(dev):
    import tests.test_fused_gpu as T
    dm, cats = _build(F=9, D=16, H=2, layers=2, task='regression')
    _train_and_perturb(dm, cats, 0, dev, steps=2)
    idx, dense, _ = T.batch(cats, 0, 70, seed=8)
    logit, out = _check(dm, idx, dense, dev, 'autoint_infer_regression')
    assert torch.equal(out, logit)


@pytest.fixture(scope='module')
def trained(dev):
    """the benchmark's graph (F = 26, D = 32, four heads, three layers) after two steps, with every BN's moving statistics
    moved; the frame of B_BIG rows and the float64 / float32 oracle logits of those rows (computed once, never changed)"""
    import tests.test_fused_gpu as T
    dm, cats = _build()
    _train_and_perturb(dm, cats, 0, dev, steps=2)
    idx, _, _ = T.batch(cats, 0, B_BIG, seed=77)
    r64 = _oracle(dm, idx, None, torch.float64)
    r32 = _oracle(dm, idx, None, torch.float32)
    return dm, cats, idx, r64, r32


@pytest.mark.parametrize('B', [1, 5, B_BIG])
def test_grid_stride(dev, trained, B):
    """one row; a partial block; more rows than the launch has waves (second and third pass, the prefetch chain)"""
    dm, cats, idx, r64, r32 = trained
    logit, out = _run_plan(dm, idx[:B], None, dev)
    figs = {'logit': ('fwd', P.max_rel(logit, r64[:B]), P.max_rel(r32[:B], r64[:B])),
            'prob': ('fwd', P.max_rel(out, torch.sigmoid(r64[:B])),
                     P.max_rel(torch.sigmoid(r32[:B].double()), torch.sigmoid(r64[:B])))}
    print(f'autoint_infer_grid[{B}]', {k: (g, f) for k, (_, g, f) in figs.items()})
    P.check_step(f'autoint_infer_grid[{B}]', 'autoint', 'bf16x2', figs)


def test_row_independence_across_batch_sizes_and_calls(dev, trained):
    dm, cats, idx, _, _ = trained
    import pandas as pd
    df = pd.DataFrame({c.name: idx[:, i].numpy() for i, c in enumerate(cats)})
    big = dm.predict(df, batch_size=B_BIG)
    again = dm.predict(df, batch_size=B_BIG)
    mid = dm.predict(df, batch_size=128)
    small = dm.predict(df.iloc[:700], batch_size=7)
    assert big.shape == (B_BIG, 1)
    assert np.array_equal(big, again), 'two calls differ'
    assert np.array_equal(big, mid), np.abs(big - mid).max()
    assert np.array_equal(big[:700], small), np.abs(big[:700] - small).max()


def test_float_and_int_ids_give_the_same_bits(dev, trained):
    dm, cats, idx, _, _ = trained
    a = _run_plan(dm, idx[:300], None, dev, 'int32')
    b = _run_plan(dm, idx[:300], None, dev, 'float32')
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize('kind', ['int32', 'float32'])
def test_out_of_range_and_fractional_ids(dev, kind):
    """an out-of-range id (negative, equal to vocab, huge) reads a zero row and is counted once per lookup; a float id is
    truncated.  The oracle gets a zero row appended to each table and the out-of-range ids pointed at it; the rows of the
    batch without a bad id keep the bits they have in a batch without any."""
    import tests.test_fused_gpu as T
    from oracle import bridge
    from tests.test_fused_domain_gpu import _odd_ids
    dm, cats = _build(F=17, D=16, H=2, layers=2, vocab=60)
    _train_and_perturb(dm, cats, 0, dev, steps=1)
    idx, dense, _ = T.batch(cats, 0, 65, seed=17)
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
        logit, out = _check(dm, ids, dense, dev, f'autoint_infer_ids[{kind}]', kind=kind, weights=weights, ids_oracle=ids_o)
        torch.cuda.synchronize()
        assert int(emb.oob_count.item()) == n_oob
    finally:
        emb.check_oob = False
    clean = ~bad.any(1)
    assert 0 < int(clean.sum()) < len(clean)
    ref_logit, ref_out = _run_plan(dm, trunc.clamp(min=0).minimum(vocab - 1), dense, dev)
    assert torch.equal(logit[clean.to(dev)], ref_logit[clean.to(dev)]) and torch.equal(out[clean.to(dev)], ref_out[clean.to(dev)])


def test_the_layer_path_is_not_run(dev, monkeypatch):
    dm, cats = _build(F=7, D=16, H=2, layers=2)
    df, y = _frame(cats, 0, 300, 2)

    def boom(*a, **k):
        raise AssertionError('the layer-by-layer forward ran')
    monkeypatch.setattr(dm.model, 'forward', boom)
    p = dm.predict(df, batch_size=128)
    assert p.shape == (300, 1) and np.isfinite(p).all()
    res = dm.evaluate(df, y, batch_size=64)
    assert np.isfinite(res['loss'])


def test_fit_predict_evaluate_against_the_layer_path(dev, monkeypatch):
    """DeepModel.fit with a validation split (its validation pass runs the plan), then predict / evaluate with the plan and
    with DT_AMD_FUSED_PREDICT=0 (the layer path) on the same trained model: both within the mode's class of the oracle,
    evaluate's loss and AUC to 1e-6"""
    dm, cats = _build(F=26, D=32, H=4, layers=3)
    df, y = _frame(cats, 0, 2000, 4)
    hist = dm.fit(df, y, batch_size=256, epochs=2, verbose=0, validation_split=0.2)
    assert 'val_loss' in hist.history
    p1 = dm.predict(df, batch_size=128)
    e1 = dm.evaluate(df, y, batch_size=256)
    monkeypatch.setenv('DT_AMD_FUSED_PREDICT', '0')
    assert dm.inference_plan() is None
    q = dm.predict(df, batch_size=128)
    e0 = dm.evaluate(df, y, batch_size=256)
    idx = torch.as_tensor(df[[c.name for c in cats]].to_numpy())
    r64 = torch.sigmoid(_oracle(dm, idx, None, torch.float64))
    r32 = torch.sigmoid(_oracle(dm, idx, None, torch.float32).double())
    f32 = P.max_rel(r32, r64)
    figs = {'plan': ('fwd', P.max_rel(torch.as_tensor(p1), r64), f32), 'layer_path': ('fwd', P.max_rel(torch.as_tensor(q), r64), f32)}
    print('plan vs layer path: max |dp| =', np.abs(p1 - q).max(), {k: (g, f) for k, (_, g, f) in figs.items()},
          {k: (e1[k], e0[k]) for k in e0})
    P.check_step('autoint_infer_fit', 'autoint', 'bf16x2', figs)
    for k in e0:
        assert abs(e1[k] - e0[k]) <= 1e-6 * max(1.0, abs(e0[k])), (k, e1[k], e0[k])


def test_continuous_columns_are_ignored(dev):
    """the net does not read the continuous columns (deepnets.py:210-224): the same predictions with 13 of them in the frame
    and for the same model called with dense=None"""
    import tests.test_fused_gpu as T
    dm, cats = _build(F=11, D=16, H=4, layers=2, Nd=13)
    _train_and_perturb(dm, cats, 13, dev, steps=1)
    df, _ = _frame(cats, 13, 150, 9)
    p = dm.predict(df, batch_size=64)
    idx, dense, _ = T.batch(cats, 13, 150, seed=9)
    logit, out = _run_plan(dm, idx, None, dev)
    logit_d, out_d = _run_plan(dm, idx, dense, dev)
    assert torch.equal(out, out_d) and torch.equal(logit, logit_d)
    assert np.array_equal(p, out.cpu().numpy())
