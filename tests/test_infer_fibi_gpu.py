# -*- coding:utf-8 -*-
"""GPU: the fused FiBiNet inference plan (fused.InferFiBiNet: one dt_fibi_infer_prepare launch per predict / evaluate, one
k_fibi_infer launch per batch — gather, SENET, both bilinear layers from the raw rows, the tower in K chunks, task_output, the
activation; csrc/fibi_infer.hip) against the float64 oracle at inference, held to the forward class tests/precision.py gives
the tower mode in force (('tower', 'bf16x3') by default, ('tower', 'bf16') with the bf16 flag — the bar
tests/test_infer_pnn_gpu.py holds the PNN plan to): over the shapes at which the kernel takes another path, every bilinear
type and pooling op, tower widths off the tile with every batch-norm combination, the grid stride, row independence, odd ids,
a mismatched workspace, and end to end through DeepTable fit / predict / evaluate against the layer-by-layer path.

Two relu layers can leave SENET's a2 all zero, and then the senet half contributes nothing and cannot be wrong: every
parametrised shape asserts, on the oracle's restatement of SENET over the gathered float64 rows, that at least a quarter of
the (row, field) entries of a2 are strictly positive and that they are not all equal.  `_trained` adds a seeded positive
shift to the two SENET biases so that this holds for every shape and seed used here."""
import numpy as np
import pytest
import torch

from tests import precision as P
from tests.infer_support import _ins, _oracle, _train_and_perturb, run_plan

pytestmark = pytest.mark.gpu

EMB_SCALE = 8.0


def _b_big():
    """more rows than two residencies of the launch (its grid is at most DT_FIBI_INFER_MAX_BLOCKS blocks, each striding over
    32-row tiles), plus an odd remainder: every block scores a third tile or a ragged one"""
    from deeptables_amd import _lib
    return 2 * _lib.DT_FIBI_INFER_MAX_BLOCKS * 32 + 37


def _build(F=26, D=16, Nd=13, bt='field_interaction', pool='mean', ratio=3, hidden=None, mode=None, vocab=30, **kw):
    import tests.test_fused_gpu as T
    dnn = {'hidden_units': hidden or ((128, 0, False), (64, 0, False)), 'activation': 'relu'}
    if mode:
        dnn['mfma_dtype'] = mode
    return T.build(F, Nd, D, vocab=vocab, nets=['fibi_dnn_nets'], dnn_params=dnn,
                   fibinet_params={'senet_pooling_op': pool, 'senet_reduction_ratio': ratio, 'bilinear_type': bt}, **kw)


def _senet(dm):
    (se,) = [l for l in dm.model.layers_by_name.values() if type(l).__name__ == 'SENET']
    return se


def _trained(dm, cats, Nd, dev, steps=2, train=True):
    """two train steps on the layer path (infer_support._train_and_perturb: the moving statistics of every BN then leave
    (0, 1)), then the embedding rows scaled by 8 as in tests/test_infer_pnn_gpu.py, then a seeded positive shift of SENET's
    two biases (the cap of the module docstring).  train=False: a seeded perturbation of every parameter instead of the
    steps, for a shape the layer path itself refuses to train."""
    if train:
        _train_and_perturb(dm, cats, Nd, dev, steps=steps)
    else:
        g = torch.Generator().manual_seed(33)
        with torch.no_grad():
            for _, p in dm.model.named_parameters():
                p.mul_(1.0 + 0.2 * torch.randn(p.shape, generator=g).to(p.device))
            for layer in dm.model.layers_by_name.values():
                if getattr(layer, 'moving_mean', None) is not None:
                    mm, mv = layer.moving_mean, layer.moving_variance
                    mm.add_((torch.randn(mm.shape, generator=g) * 0.2).to(mm.device))
                    mv.mul_((torch.rand(mv.shape, generator=g) + 0.5).to(mv.device))
    g = torch.Generator().manual_seed(55)
    se = _senet(dm)
    with torch.no_grad():
        for t in dm.model.layers_by_name['emb_categorical_vars_all'].tables.values():
            t.mul_(EMB_SCALE)
        for d in (se.dense_att1, se.dense_att2):
            d.bias.add_((0.25 + 0.5 * torch.rand(d.bias.shape, generator=g)).to(d.bias.device))


def _assert_senet_alive(dm, idx):
    """the cap: a2 of these rows, by the oracle's SENET on the gathered float64 rows"""
    from oracle import bridge, reference_layers as R
    w = bridge.oracle_weights(dm, torch.float64)
    x = torch.stack([t[idx[:, f].long()] for f, t in enumerate(w['emb_categorical_vars_all'])], 1)      # [B, F, D]
    (sw,) = w['senet']
    se = _senet(dm)
    v = R.senet(x, sw['att1'], sw['att2'], 'max' if se.pooling_op == 'max' else 'mean')                 # = a2_i x_i
    a2 = (v * x).sum(-1) / (x * x).sum(-1)                                                              # [B, F]
    pos = a2 > 0
    assert float(pos.double().mean()) >= 0.25, float(pos.double().mean())
    assert float(a2[pos].max()) > float(a2[pos].min())
    return a2


def _run_plan(dm, idx, dense, dev, kind='int32'):
    from deeptables_amd import fused
    return run_plan(dm, idx, dense, dev, fused.InferFiBiNet, kind)


def _figs(dm, logit, out, r64, r32):
    figs = {'logit': ('fwd', P.max_rel(logit, r64), P.max_rel(r32, r64))}
    if dm.output_activation == 'sigmoid':
        figs['prob'] = ('fwd', P.max_rel(out, torch.sigmoid(r64)), P.max_rel(torch.sigmoid(r32.double()), torch.sigmoid(r64)))
    else:
        assert torch.equal(out, logit)
    return figs


def _check(dm, idx, dense, dev, label, mode='bf16x3', kind='int32', weights=None, ids_oracle=None):
    logit, out = _run_plan(dm, idx, dense, dev, kind)
    ids_o = idx if ids_oracle is None else ids_oracle
    w64 = weights(torch.float64) if weights else None
    w32 = weights(torch.float32) if weights else None
    r64 = _oracle(dm, ids_o, dense, torch.float64, w64)
    r32 = _oracle(dm, ids_o, dense, torch.float32, w32)
    assert bool(torch.isfinite(r64).all())
    figs = _figs(dm, logit, out, r64, r32)
    print(label, {k: (g, f) for k, (_, g, f) in figs.items()})
    P.check_step(label, 'tower', mode, figs)
    return logit, out


# (F, D, Nd), bilinear type, pooling op, reduction ratio: one pair, R = 1, one dense column, a chunk nearly empty; the
# smallest D, 32 pairs per chunk, the halves meet inside chunk 0; P D = 80, a half boundary that is a multiple of nothing,
# R = F; a ratio above F gives R = 1, P D = 576 = 4.5 chunks: the boundary is mid-chunk; the benchmark shape, 82 chunks, a
# ragged last one; the widest D: one pair is half a chunk; the widest dense block; F D = 512, P = 2016, the most chunks, the
# largest workspace
SHAPES = [((2, 16, 1), 'field_interaction', 'mean', 3), ((3, 4, 2), 'field_each', 'max', 2), ((5, 8, 3), 'field_all', 'mean', 1),
          ((9, 16, 5), 'field_interaction', 'max', 20), ((26, 16, 13), 'field_interaction', 'mean', 3),
          ((8, 64, 3), 'field_each', 'mean', 3), ((16, 32, 64), 'field_all', 'max', 3), ((64, 8, 1), 'field_interaction', 'mean', 3)]


@pytest.mark.parametrize('shape,bt,pool,ratio', SHAPES,
                         ids=lambda v: '-'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_plan_matches_the_oracle_after_training(dev, shape, bt, pool, ratio):
    import tests.test_fused_gpu as T
    from deeptables_amd import _lib, ops
    F, D, Nd = shape
    dm, cats = _build(F=F, D=D, Nd=Nd, bt=bt, pool=pool, ratio=ratio)
    train = True
    try:
        idx, dense, y = T.batch(cats, Nd, 64, seed=20)
        dm.train_step(_ins(idx, dense, dev), y.to(dev))
    except _lib.DtHipError as e:                     # the layer path refuses to train this shape: a backward kernel's domain
        assert '_bwd' in str(e), str(e)
        train = False
    _trained(dm, cats, Nd, dev, train=train, steps=1 if train else 0)
    plan = dm.inference_plan()
    assert (plan.F, plan.D, plan.Nd) == (F, D, Nd)
    assert (plan.bt, plan.R) == (ops.BILINEAR_TYPES[bt], max(F // ratio, 1))
    assert plan.pool == (_lib.DT_FIBI_POOL_MAX if pool == 'max' else _lib.DT_FIBI_POOL_MEAN)
    idx, dense, _ = T.batch(cats, Nd, 203, seed=41)
    _assert_senet_alive(dm, idx)
    _check(dm, idx, dense, dev, f'fibi_infer[{F},{D},{Nd},{bt},{pool},{ratio}]')


@pytest.mark.parametrize('cells', range(4))
def test_tower_widths_off_the_tile_with_every_batch_norm_combination(dev, cells):
    import tests.test_fused_gpu as T
    hidden = ((100, 0.2, bool(cells & 1)), (40, 0, bool(cells & 2)))
    dm, cats = _build(F=9, D=16, Nd=5, hidden=hidden, bt=('field_interaction', 'field_each', 'field_all', 'field_each')[cells])
    _trained(dm, cats, 5, dev)
    L = dm.model.layers_by_name
    assert ('fibi_dnn_bn_1' in L) == bool(cells & 1) and ('fibi_dnn_bn_2' in L) == bool(cells & 2)
    idx, dense, _ = T.batch(cats, 5, 203, seed=9)
    _assert_senet_alive(dm, idx)
    _check(dm, idx, dense, dev, f'fibi_infer_cells[{cells}]')


def test_bf16_tower_mode(dev):
    """the flag acts on the tower; the bar is the ('tower', 'bf16') class"""
    import tests.test_fused_gpu as T
    from deeptables_amd import _lib
    dm, cats = _build(F=11, D=16, Nd=5, mode='bf16')
    _trained(dm, cats, 5, dev)
    idx, dense, _ = T.batch(cats, 5, 203, seed=4)
    _assert_senet_alive(dm, idx)
    _check(dm, idx, dense, dev, 'fibi_infer_bf16', mode='bf16')
    assert dm.inference_plan().flags & _lib.DT_INFER_TOWER_BF16


@pytest.mark.parametrize('variant', ['regression', 'no_output_bias'])
def test_regression_task_and_no_output_bias(dev, variant):
    import tests.test_fused_gpu as T
    dm, cats = _build(F=9, D=16, Nd=3, bt='field_each' if variant == 'regression' else 'field_all', pool='max',
                      task='regression' if variant == 'regression' else 'binary', use_bias=variant != 'no_output_bias')
    _trained(dm, cats, 3, dev)
    assert (dm.model.layers_by_name['task_output'].bias is None) == (variant == 'no_output_bias')
    idx, dense, _ = T.batch(cats, 3, 203, seed=8)
    _assert_senet_alive(dm, idx)
    logit, out = _check(dm, idx, dense, dev, f'fibi_infer[{variant}]')
    if variant == 'regression':
        assert torch.equal(out, logit)


@pytest.fixture(scope='module')
def trained(dev):
    """a small graph after two steps; the frame of B_BIG rows and the float64 / float32 oracle logits of those rows (computed
    once, never changed)"""
    import tests.test_fused_gpu as T
    dm, cats = _build(F=5, D=8, Nd=3)
    _trained(dm, cats, 3, dev)
    idx, dense, _ = T.batch(cats, 3, _b_big(), seed=77)
    r64 = _oracle(dm, idx, dense, torch.float64)
    r32 = _oracle(dm, idx, dense, torch.float32)
    return dm, cats, idx, dense, r64, r32


def test_grid_stride(dev, trained):
    """more rows than two residencies of the capped grid plus an odd remainder, against the oracle"""
    dm, cats, idx, dense, r64, r32 = trained
    B = _b_big()
    logit, out = _run_plan(dm, idx, dense, dev)
    figs = _figs(dm, logit, out, r64, r32)
    print(f'fibi_infer_grid[{B}]', {k: (g, f) for k, (_, g, f) in figs.items()})
    P.check_step(f'fibi_infer_grid[{B}]', 'tower', 'bf16x3', figs)


def test_a_single_row(dev, trained):
    """B = 1: the row's bits are those it has as row 0 of a 203-row batch, which is held to the class bar; the row's own
    error is measured on that batch's scale, as tests/test_infer_pnn_gpu.py explains"""
    dm, cats, idx, dense, r64, r32 = trained
    n = 203
    many = _run_plan(dm, idx[:n], dense[:n], dev)
    P.check_step(f'fibi_infer_grid[{n}]', 'tower', 'bf16x3', _figs(dm, many[0], many[1], r64[:n], r32[:n]))
    one = _run_plan(dm, idx[:1], dense[:1], dev)
    assert one[0].shape == (1, 1) and one[1].shape == (1, 1)

    def row_err(got, ref):
        return float((got.detach().cpu().double() - ref[:1]).abs().max()) / float(ref[:n].abs().max())
    p64, p32 = torch.sigmoid(r64), torch.sigmoid(r32.double())
    figs = {'logit': ('fwd', row_err(one[0], r64), P.max_rel(r32[:n], r64[:n])),
            'prob': ('fwd', row_err(one[1], p64), P.max_rel(p32[:n], p64[:n]))}
    print('fibi_infer_grid[1]', {k: (g, f) for k, (_, g, f) in figs.items()})
    P.check_step('fibi_infer_grid[1]', 'tower', 'bf16x3', figs)
    assert torch.equal(one[0], many[0][:1]) and torch.equal(one[1], many[1][:1])


def test_an_empty_batch_is_accepted(dev, trained):
    """B = 0 returns without an error; the scores of the call after it are unchanged"""
    dm, cats, idx, dense, _, _ = trained
    before = _run_plan(dm, idx[:40], dense[:40], dev)
    plan = dm.inference_plan()
    plan.prepare()
    logit = torch.empty((0, 1), dtype=torch.float32, device=dev)
    plan.infer(idx[:0].to(torch.int32).to(dev), dense[:0].to(dev), logit, torch.empty_like(logit))
    torch.cuda.synchronize()
    after = _run_plan(dm, idx[:40], dense[:40], dev)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])


def test_rows_are_independent_of_their_place_in_the_batch(dev, trained):
    """row r of a 203-row batch equals the same row scored alone, bit for bit; so does a permuted batch"""
    dm, cats, idx, dense, _, _ = trained
    n = 203
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(5))
    a = _run_plan(dm, idx[:n], dense[:n], dev)
    b = _run_plan(dm, idx[:n][perm], dense[:n][perm], dev)
    for x, y in zip(a, b):
        assert torch.equal(x[perm.to(dev)], y)
    for r in (0, 31, 32, 100, 202):
        alone = _run_plan(dm, idx[r:r + 1], dense[r:r + 1], dev)
        assert torch.equal(a[0][r:r + 1], alone[0]) and torch.equal(a[1][r:r + 1], alone[1]), r


def test_float_and_int_ids_give_the_same_bits(dev, trained):
    dm, cats, idx, dense, r64, r32 = trained
    a = _run_plan(dm, idx[:300], dense[:300], dev, 'int32')
    b = _run_plan(dm, idx[:300], dense[:300], dev, 'float32')
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    P.check_step('fibi_infer_float_ids', 'tower', 'bf16x3', _figs(dm, b[0], b[1], r64[:300], r32[:300]))


@pytest.mark.parametrize('kind', ['int32', 'float32'])
def test_out_of_range_and_fractional_ids(dev, kind):
    """an out-of-range id (negative, equal to vocab, huge) reads a zero row and is counted once per lookup; a float id is
    truncated.  The oracle gets a zero row appended to each table and the out-of-range ids pointed at it; the rows of the
    batch without a bad id keep the bits they have in a batch without any."""
    import tests.test_fused_gpu as T
    from oracle import bridge
    from tests.test_fused_domain_gpu import _odd_ids
    dm, cats = _build(F=17, D=16, Nd=3, vocab=60)
    _trained(dm, cats, 3, dev, steps=1)
    idx, dense, _ = T.batch(cats, 3, 65, seed=17)
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
        logit, out = _check(dm, ids, dense, dev, f'fibi_infer_ids[{kind}]', kind=kind, weights=weights, ids_oracle=ids_o)
        torch.cuda.synchronize()
        assert int(emb.oob_count.item()) == n_oob
    finally:
        emb.check_oob = False
    clean = ~bad.any(1)
    assert 0 < int(clean.sum()) < len(clean)
    ref_logit, ref_out = _run_plan(dm, trunc.clamp(min=0).minimum(vocab - 1), dense, dev)
    assert torch.equal(logit[clean.to(dev)], ref_logit[clean.to(dev)]) and torch.equal(out[clean.to(dev)], ref_out[clean.to(dev)])


def test_a_launch_that_does_not_match_the_prepared_workspace_scores_nan(dev):
    """the workspace names the (F, D, Nd, bilinear_type, R) it was prepared for; a launch with another bilinear type or R —
    both inside the domain, both with a layout no larger than the prepared one — reads no weight from where another layout
    put it: every logit and output is NaN, and the next matching call gives the first call's bits"""
    import tests.test_fused_gpu as T
    from deeptables_amd import _lib
    dm, cats = _build(F=7, D=16, Nd=3, ratio=2)
    idx, dense, _ = T.batch(cats, 3, 37, seed=2)
    good = _run_plan(dm, idx, dense, dev)
    assert bool(torch.isfinite(good[0]).all()) and bool(torch.isfinite(good[1]).all())
    plan = dm.inference_plan()
    assert (plan.bt, plan.R) == (_lib.DT_BILINEAR_FIELD_INTERACTION, 3)
    ins = _ins(idx, dense, dev)
    for attr, other in (('bt', _lib.DT_BILINEAR_FIELD_ALL), ('R', 2)):
        keep = getattr(plan, attr)
        plan.prepare()
        setattr(plan, attr, other)
        try:
            assert 0 < _lib.lib().dt_fibi_infer_workspace_bytes(*plan._dims()) <= plan.ws.numel() * 4
            logit = torch.zeros((37, 1), dtype=torch.float32, device=dev)
            out = torch.zeros_like(logit)
            plan.infer(ins[0], ins[1], logit, out)
            torch.cuda.synchronize()
        finally:
            setattr(plan, attr, keep)
        assert bool(torch.isnan(logit).all()) and bool(torch.isnan(out).all()), attr
    again = _run_plan(dm, idx, dense, dev)
    assert torch.equal(again[0], good[0]) and torch.equal(again[1], good[1])


def test_fit_predict_evaluate_against_the_layer_path(dev, monkeypatch):
    """DeepTable end to end with nets=deepnets.FiBiNet at (F, D, Nd) = (26, 16, 13), 300 rows: fit with a validation split (its
    validation pass runs the plan), then predict_proba, predict and evaluate with the plan at batch sizes 128 / 7 / 8192
    (identical) and with DT_AMD_FUSED_PREDICT=0 (the layer path) on the same trained model.  predict_proba's second column is
    held to the class bar through the oracle on both paths."""
    import pandas as pd
    from deeptables_amd.models import DeepTable, ModelConfig, deepnets
    rng = np.random.default_rng(0)
    n, F, Nd = 300, 26, 13
    df = pd.DataFrame({f'c{i:02d}': rng.choice([f'v{k}' for k in range(5 + i % 7)], n) for i in range(F)})
    for j in range(Nd):
        df[f'x{j:02d}'] = rng.normal(0.0, 1.0, n).astype(np.float32)
    y = pd.Series(((df['x03'] > 0) ^ (df['c01'] == 'v1'))).map({True: 'yes', False: 'no'})
    conf = ModelConfig(nets=deepnets.FiBiNet, metrics=['AUC'], earlystopping_patience=0, fixed_embedding_dim=True,
                       embeddings_output_dim=16)
    dt = DeepTable(config=conf)
    _, hist = dt.fit(df, y, batch_size=128, epochs=2, verbose=0, validation_split=0.2)
    assert 'val_loss' in hist.history
    dm = dt.model
    plan = dm.inference_plan()
    assert type(plan).__name__ == 'InferFiBiNet' and (plan.F, plan.D, plan.Nd) == (F, 16, Nd)
    pr1, pd1, ev1 = dt.predict_proba(df, batch_size=128), dt.predict(df, batch_size=128), dt.evaluate(df, y, batch_size=128)
    for b in (7, 8192):
        assert np.array_equal(dt.predict_proba(df, batch_size=b), pr1), b
    monkeypatch.setenv('DT_AMD_FUSED_PREDICT', '0')
    assert dm.inference_plan() is None
    pr0, pd0, ev0 = dt.predict_proba(df, batch_size=128), dt.predict(df, batch_size=128), dt.evaluate(df, y, batch_size=128)
    assert pr1.shape == pr0.shape == (n, 2)
    Xt = dt.preprocessor.transform_X(df)
    idx = torch.as_tensor(Xt[[c.name for c in dm.categorical_columns]].to_numpy())
    dense = torch.as_tensor(Xt[list(dm.continuous_columns[0].column_names)].to_numpy(dtype=np.float32))
    r64 = torch.sigmoid(_oracle(dm, idx, dense, torch.float64))
    r32 = torch.sigmoid(_oracle(dm, idx, dense, torch.float32).double())
    f32 = P.max_rel(r32, r64)
    figs = {'plan': ('fwd', P.max_rel(torch.as_tensor(pr1[:, 1]), r64), f32),
            'layer_path': ('fwd', P.max_rel(torch.as_tensor(pr0[:, 1]), r64), f32)}
    print('plan vs layer path: max |dp| =', np.abs(pr1 - pr0).max(), {k: (g, f) for k, (_, g, f) in figs.items()},
          {k: (ev1[k], ev0[k]) for k in ev0})
    P.check_step('fibi_infer_deeptable', 'tower', 'bf16x3', figs)
    for pr in (pr1, pr0):
        assert np.array_equal(pr[:, 0], 1.0 - pr[:, 1])
    pr = r64.reshape(-1)
    tol = 2 * P.STEP_BAR['fp32'] * max(f32, P.FLOOR) * float(pr.max())
    undecided = ((pr - 0.5).abs() <= tol).numpy()
    assert np.array_equal(np.asarray(pd1)[~undecided], np.asarray(pd0)[~undecided])
    assert set(np.unique(pd1)) <= {'yes', 'no'}
    assert {k.lower() for k in ev0} >= {'loss', 'auc'} and all(np.isfinite(ev1[k]) for k in ev1)
