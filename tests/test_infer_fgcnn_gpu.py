# -*- coding:utf-8 -*-
"""GPU: the fused FGCNN inference plan (fused.InferFGCNN: one dt_fgcnn_infer_prepare launch per predict / evaluate, then per
batch one conv and one recomb launch per block and the tower launch; csrc/fgcnn_infer.hip) against the float64 oracle at
inference, held to the forward class tests/precision.py gives the tower mode in force (('tower', 'bf16x3') by default,
('tower', 'bf16') with the bf16 flag — the bar tests/test_infer_pnn_gpu.py and tests/test_infer_fibi_gpu.py hold their plans
to): over the shapes at which a kernel takes another path, tower widths off the tile with every batch-norm combination, the
grid stride, row independence, odd ids, a mismatched workspace, and end to end through DeepTable fit / predict / evaluate
against the layer-by-layer path.

tanh and the max pooling can hide an error: a saturated unit gives +-1 whatever its input, a nearly linear one would pass
without tanh.  Every parametrised shape therefore asserts, on the oracle's float64 restatement of each block on its actual
input (reference_layers.fgcnn without activation and with pool height 1 for the convolution's pre-activations; the oracle's
pooled map times the recombination kernel for the recombination's), that at most 0.05 of the pre-activations have |z| > 4 and
at least 0.10 have 0.5 <= |z| <= 3.  The embedding rows are overwritten with seeded N(0, 2^2) values for that: rows at the
initialiser's scale leave the convolution in tanh's linear range."""
import numpy as np
import pytest
import torch

from tests import precision as P
from tests.infer_support import _ins, _oracle, _train_and_perturb, run_plan

pytestmark = pytest.mark.gpu

ROW_SCALE = 2.0
KEYS = ('fg_filters', 'fg_heights', 'fg_pool_heights', 'fg_new_feat_filters')
DEFAULTS = ((14, 16), (7, 7), (2, 2), (2, 2))
SMALL = ((5, 4), (3, 2), (2, 2), (2, 1))             # on (5, 8, 3): F_k = 5 -> 3 -> 2, an odd and an even height


def _b_big():
    """more rows than two residencies of the tower launch (its grid is at most DT_FGCNN_INFER_MAX_BLOCKS blocks, each
    striding over 32-row tiles), plus an odd remainder; the conv launches (tiles of at most 32 rows) and the recomb launches
    (64-row tiles) stride as well"""
    from deeptables_amd import _lib
    return 2 * _lib.DT_FGCNN_INFER_MAX_BLOCKS * 32 + 37


def _build(F=26, D=16, Nd=13, fg=DEFAULTS, hidden=None, mode=None, vocab=30, **kw):
    import tests.test_fused_gpu as T
    dnn = {'hidden_units': hidden or ((128, 0, False), (64, 0, False)), 'activation': 'relu'}
    if mode:
        dnn['mfma_dtype'] = mode
    return T.build(F, Nd, D, vocab=vocab, nets=['fgcnn_dnn_nets'], dnn_params=dnn, fgcnn_params=dict(zip(KEYS, fg)), **kw)


def _trained(dm, cats, Nd, dev, steps=2, train=True, row_seed=55, row_scale=ROW_SCALE):
    """train steps on the layer path (infer_support._train_and_perturb: the moving statistics of every BN then leave (0, 1)),
    then the embedding rows overwritten with seeded N(0, row_scale^2) values (the cap of the module docstring).  train=False:
    a seeded perturbation of every parameter instead of the steps, for a shape the layer path itself refuses to train."""
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
    g = torch.Generator().manual_seed(row_seed)
    with torch.no_grad():
        for t in dm.model.layers_by_name['emb_categorical_vars_all'].tables.values():
            t.copy_((torch.randn(t.shape, generator=g) * row_scale).to(t.device))


def _assert_blocks_alive(dm, idx):
    """the cap: per block, the shares of saturated and of mid-range pre-activations of the convolution and of the
    recombination Dense, by the oracle in float64"""
    from oracle import bridge, reference_layers as R
    w = bridge.oracle_weights(dm, torch.float64)
    x = torch.stack([t[idx[:, f].long()] for f, t in enumerate(w['emb_categorical_vars_all'])], 1).unsqueeze(-1)   # [B, F, D, 1]
    plan = dm.inference_plan()
    shares = []
    for k, fw in enumerate(w['fgcnn']):
        _, F, D, C = x.shape
        filt, pool, nf = plan.params[0][k], plan.params[2][k], plan.params[3][k]
        one = torch.zeros(F * D * filt, F * D, dtype=x.dtype)
        zc, _ = R.fgcnn(x, fw['conv_kernel'], fw['conv_bias'], one, torch.zeros(F * D, dtype=x.dtype), 1, 1, activation=None)
        pooled, feats = R.fgcnn(x, fw['conv_kernel'], fw['conv_bias'], fw['dense_kernel'], fw['dense_bias'], pool, nf)
        zr = pooled.reshape(pooled.shape[0], -1) @ fw['dense_kernel'] + fw['dense_bias']
        assert torch.allclose(torch.tanh(zr).reshape(feats.shape), feats)
        for what, z in (('conv', zc), ('recomb', zr)):
            a = z.abs()
            sat, mid = float((a > 4).double().mean()), float(((a >= 0.5) & (a <= 3)).double().mean())
            shares.append((k, what, sat, mid))
            assert sat <= 0.05 and mid >= 0.10, (k, what, sat, mid)
        x = pooled
    return shares


def _run_plan(dm, idx, dense, dev, kind='int32'):
    from deeptables_amd import fused
    return run_plan(dm, idx, dense, dev, fused.InferFGCNN, kind)


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


# ((F, D, Nd); filters; heights; pools; new filters): fewest fields, no dense input, height 1, pool 1; an even height, F_1 = 3
# not divisible by the pool (a one-field last window against the -inf padding), one filter; depth 3, a height above the field
# count, F_k = 5 -> 2 -> 1, a block whose map is one field; odd F, the widest filter count, three new filters; the benchmark
# shape with the default blocks (the largest recombination weight of the defaults); the widest D; F D = 512 with the widest
# dense block.  The third entry is the seed of the model's initialisation: with the builder's default (3) the depth-3 case's
# third block — one field of four tanh outputs into Glorot weights — has 0.006 of its convolution pre-activations in the
# mid range and misses the cap; seed 4 gives 0.25 or more in every block and stage (measured on the CPU oracle).
SHAPES = [((2, 4, 0), ((3,), (1,), (1,), (1,)), 3),
          ((3, 16, 1), ((1,), (2,), (2,), (1,)), 3),
          ((5, 8, 3), ((5, 4, 3), (9, 2, 3), (3, 2, 1), (1, 3, 2)), 4),
          ((13, 16, 5), ((16,), (4,), (2,), (3,)), 3),
          ((26, 16, 13), DEFAULTS, 3),
          ((8, 64, 3), ((4, 4), (3, 3), (2, 2), (2, 2)), 3),
          ((64, 8, 64), ((2,), (7,), (3,), (1,)), 3)]


@pytest.mark.parametrize('shape,fg,seed', SHAPES,
                         ids=lambda v: f's{v}' if isinstance(v, int) else '-'.join(map(str, v)) if isinstance(v[0], int) else f'd{len(v[0])}')
def test_plan_matches_the_oracle_after_training(dev, shape, fg, seed):
    import tests.test_fused_gpu as T
    from deeptables_amd import _lib
    F, D, Nd = shape
    dm, cats = _build(F=F, D=D, Nd=Nd, fg=fg, seed=seed)
    train = True
    try:
        idx, dense, y = T.batch(cats, Nd, 64, seed=20)
        dm.train_step(_ins(idx, dense, dev), y.to(dev))
    except _lib.DtHipError as e:                     # the layer path refuses to train this shape: a kernel's domain
        print('layer path refused the train step:', str(e)[:200])
        train = False
    _trained(dm, cats, Nd, dev, train=train, steps=1 if train else 0)
    plan = dm.inference_plan()
    assert (plan.F, plan.D, plan.Nd) == (F, D, Nd) and plan.params == tuple(tuple(v) for v in fg) and plan.depth == len(fg[0])
    idx, dense, _ = T.batch(cats, Nd, 203, seed=41)
    print('pre-activation shares (block, stage, |z| > 4, 0.5 <= |z| <= 3):', _assert_blocks_alive(dm, idx))
    _check(dm, idx, dense, dev, f'fgcnn_infer[{F},{D},{Nd},{fg}]')


@pytest.mark.parametrize('cells', range(4))
def test_tower_widths_off_the_tile_with_every_batch_norm_combination(dev, cells):
    import tests.test_fused_gpu as T
    hidden = ((100, 0.2, bool(cells & 1)), (40, 0, bool(cells & 2)))
    dm, cats = _build(F=5, D=8, Nd=3, fg=SMALL, hidden=hidden)
    _trained(dm, cats, 3, dev)
    L = dm.model.layers_by_name
    assert ('fgcnn_dnn_bn_1' in L) == bool(cells & 1) and ('fgcnn_dnn_bn_2' in L) == bool(cells & 2)
    idx, dense, _ = T.batch(cats, 3, 203, seed=9)
    _assert_blocks_alive(dm, idx)
    _check(dm, idx, dense, dev, f'fgcnn_infer_cells[{cells}]')


def test_bf16_tower_mode(dev):
    """the flag acts on the tower; the bar is the ('tower', 'bf16') class"""
    import tests.test_fused_gpu as T
    from deeptables_amd import _lib
    dm, cats = _build(F=5, D=8, Nd=3, fg=SMALL, mode='bf16')
    _trained(dm, cats, 3, dev)
    idx, dense, _ = T.batch(cats, 3, 203, seed=4)
    _assert_blocks_alive(dm, idx)
    _check(dm, idx, dense, dev, 'fgcnn_infer_bf16', mode='bf16')
    assert dm.inference_plan().flags & _lib.DT_INFER_TOWER_BF16


@pytest.mark.parametrize('variant', ['regression', 'no_output_bias'])
def test_regression_task_and_no_output_bias(dev, variant):
    import tests.test_fused_gpu as T
    dm, cats = _build(F=5, D=8, Nd=3, fg=SMALL, task='regression' if variant == 'regression' else 'binary',
                      use_bias=variant != 'no_output_bias')
    _trained(dm, cats, 3, dev)
    assert (dm.model.layers_by_name['task_output'].bias is None) == (variant == 'no_output_bias')
    idx, dense, _ = T.batch(cats, 3, 203, seed=8)
    _assert_blocks_alive(dm, idx)
    logit, out = _check(dm, idx, dense, dev, f'fgcnn_infer[{variant}]')
    if variant == 'regression':
        assert torch.equal(out, logit)


@pytest.fixture(scope='module')
def trained(dev):
    """a small graph after two steps; the frame of B_BIG rows and the float64 / float32 oracle logits of those rows (computed
    once, never changed)"""
    import tests.test_fused_gpu as T
    dm, cats = _build(F=5, D=8, Nd=3, fg=SMALL)
    _trained(dm, cats, 3, dev)
    idx, dense, _ = T.batch(cats, 3, _b_big(), seed=77)
    r64 = _oracle(dm, idx, dense, torch.float64)
    r32 = _oracle(dm, idx, dense, torch.float32)
    return dm, cats, idx, dense, r64, r32


def test_grid_stride(dev, trained):
    """more rows than two residencies of the capped grids plus an odd remainder, against the oracle"""
    dm, cats, idx, dense, r64, r32 = trained
    B = _b_big()
    logit, out = _run_plan(dm, idx, dense, dev)
    figs = _figs(dm, logit, out, r64, r32)
    print(f'fgcnn_infer_grid[{B}]', {k: (g, f) for k, (_, g, f) in figs.items()})
    P.check_step(f'fgcnn_infer_grid[{B}]', 'tower', 'bf16x3', figs)


def test_a_single_row(dev, trained):
    """B = 1: the row's bits are those it has as row 0 of a 203-row batch, which is held to the class bar; the row's own
    error is measured on that batch's scale, as tests/test_infer_pnn_gpu.py explains"""
    dm, cats, idx, dense, r64, r32 = trained
    n = 203
    many = _run_plan(dm, idx[:n], dense[:n], dev)
    P.check_step(f'fgcnn_infer_grid[{n}]', 'tower', 'bf16x3', _figs(dm, many[0], many[1], r64[:n], r32[:n]))
    one = _run_plan(dm, idx[:1], dense[:1], dev)
    assert one[0].shape == (1, 1) and one[1].shape == (1, 1)

    def row_err(got, ref):
        return float((got.detach().cpu().double() - ref[:1]).abs().max()) / float(ref[:n].abs().max())
    p64, p32 = torch.sigmoid(r64), torch.sigmoid(r32.double())
    figs = {'logit': ('fwd', row_err(one[0], r64), P.max_rel(r32[:n], r64[:n])),
            'prob': ('fwd', row_err(one[1], p64), P.max_rel(p32[:n], p64[:n]))}
    print('fgcnn_infer_grid[1]', {k: (g, f) for k, (_, g, f) in figs.items()})
    P.check_step('fgcnn_infer_grid[1]', 'tower', 'bf16x3', figs)
    assert torch.equal(one[0], many[0][:1]) and torch.equal(one[1], many[1][:1])


def test_an_empty_batch_is_accepted(dev, trained):
    """B = 0 returns without an error and without a launch; the scores of the call after it are unchanged"""
    from deeptables_amd import fused
    dm, cats, idx, dense, _, _ = trained
    before = _run_plan(dm, idx[:40], dense[:40], dev)
    plan = dm.inference_plan()
    plan.prepare()
    logit = torch.empty((0, 1), dtype=torch.float32, device=dev)
    plan.infer(idx[:0].to(torch.int32).to(dev), dense[:0].to(dev), logit, torch.empty_like(logit))
    # the library's entry points accept B = 0 too, before they look at a pointer
    lib, shape = fused.lib(), plan._dims()
    assert lib.dt_fgcnn_infer_conv(0, None, 1, None, None, None, None, 0, *shape, None, None, None) == 0
    assert lib.dt_fgcnn_infer_recomb(0, None, 0, *shape, None, None, None) == 0
    assert lib.dt_fgcnn_infer_tower(None, 1, None, None, None, None, None, 0, *shape, None, None, None, None, 0, None) == 0
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
    for r in (0, 31, 32, 63, 64, 100, 202):
        alone = _run_plan(dm, idx[r:r + 1], dense[r:r + 1], dev)
        assert torch.equal(a[0][r:r + 1], alone[0]) and torch.equal(a[1][r:r + 1], alone[1]), r


def test_float_and_int_ids_give_the_same_bits(dev, trained):
    dm, cats, idx, dense, r64, r32 = trained
    a = _run_plan(dm, idx[:300], dense[:300], dev, 'int32')
    b = _run_plan(dm, idx[:300], dense[:300], dev, 'float32')
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    P.check_step('fgcnn_infer_float_ids', 'tower', 'bf16x3', _figs(dm, b[0], b[1], r64[:300], r32[:300]))


@pytest.mark.parametrize('kind', ['int32', 'float32'])
def test_out_of_range_and_fractional_ids(dev, kind):
    """an out-of-range id (negative, equal to vocab, huge) reads a zero row — in the first block's gather and in the tower's —
    and is counted once per lookup; a float id is truncated.  The oracle gets a zero row appended to each table and the
    out-of-range ids pointed at it; the rows of the batch without a bad id keep the bits they have in a batch without any."""
    import tests.test_fused_gpu as T
    from oracle import bridge
    from tests.test_fused_domain_gpu import _odd_ids
    dm, cats = _build(F=9, D=16, Nd=3, fg=((4, 3), (3, 2), (2, 2), (2, 1)), vocab=60)
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
        logit, out = _check(dm, ids, dense, dev, f'fgcnn_infer_ids[{kind}]', kind=kind, weights=weights, ids_oracle=ids_o)
        torch.cuda.synchronize()
        assert int(emb.oob_count.item()) == n_oob
    finally:
        emb.check_oob = False
    clean = ~bad.any(1)
    assert 0 < int(clean.sum()) < len(clean)
    ref_logit, ref_out = _run_plan(dm, trunc.clamp(min=0).minimum(vocab - 1), dense, dev)
    assert torch.equal(logit[clean.to(dev)], ref_logit[clean.to(dev)]) and torch.equal(out[clean.to(dev)], ref_out[clean.to(dev)])


def test_a_launch_that_does_not_match_the_prepared_workspace_scores_nan(dev):
    """the workspace names the (F, D, Nd, block parameters) it was prepared for; launches with another height or another
    new-filter count — both inside the domain, both with a layout no larger than the prepared one — read no weight from where
    another layout put it: every logit and output is NaN, and the next matching call gives the first call's bits"""
    import tests.test_fused_gpu as T
    from deeptables_amd import _lib
    fg = ((4, 3), (3, 3), (2, 2), (2, 2))
    dm, cats = _build(F=7, D=16, Nd=3, fg=fg)
    idx, dense, _ = T.batch(cats, 3, 37, seed=2)
    good = _run_plan(dm, idx, dense, dev)
    assert bool(torch.isfinite(good[0]).all()) and bool(torch.isfinite(good[1]).all())
    plan = dm.inference_plan()
    assert plan.params == fg
    ins = _ins(idx, dense, dev)
    for what, other in (('height', (fg[0], (2, 3), fg[2], fg[3])), ('new_filters', (fg[0], fg[1], fg[2], (1, 2)))):
        plan.prepare()
        keep = (plan.params, plan._arrays, plan._shape_args)
        plan.params = other
        plan._arrays, plan._shape_args = plan._host_arrays(other)
        try:
            assert 0 < _lib.lib().dt_fgcnn_infer_workspace_bytes(*plan._dims()) <= plan.ws.numel() * 4
            logit = torch.zeros((37, 1), dtype=torch.float32, device=dev)
            out = torch.zeros_like(logit)
            plan.infer(ins[0], ins[1], logit, out)
            torch.cuda.synchronize()
        finally:
            plan.params, plan._arrays, plan._shape_args = keep
        assert bool(torch.isnan(logit).all()) and bool(torch.isnan(out).all()), what
    again = _run_plan(dm, idx, dense, dev)
    assert torch.equal(again[0], good[0]) and torch.equal(again[1], good[1])


def test_fit_predict_evaluate_against_the_layer_path(dev, monkeypatch):
    """DeepTable end to end with nets=deepnets.FGCNN at (F, D, Nd) = (26, 16, 13), 300 rows: fit with a validation split (its
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
    conf = ModelConfig(nets=deepnets.FGCNN, metrics=['AUC'], earlystopping_patience=0, fixed_embedding_dim=True,
                       embeddings_output_dim=16)
    dt = DeepTable(config=conf)
    _, hist = dt.fit(df, y, batch_size=128, epochs=2, verbose=0, validation_split=0.2)
    assert 'val_loss' in hist.history
    dm = dt.model
    plan = dm.inference_plan()
    assert type(plan).__name__ == 'InferFGCNN' and (plan.F, plan.D, plan.Nd) == (F, 16, Nd) and plan.params == DEFAULTS
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
    P.check_step('fgcnn_infer_deeptable', 'tower', 'bf16x3', figs)
    for pr in (pr1, pr0):
        assert np.array_equal(pr[:, 0], 1.0 - pr[:, 1])
    pr = r64.reshape(-1)
    tol = 2 * P.STEP_BAR['fp32'] * max(f32, P.FLOOR) * float(pr.max())
    undecided = ((pr - 0.5).abs() <= tol).numpy()
    assert np.array_equal(np.asarray(pd1)[~undecided], np.asarray(pd0)[~undecided])
    assert set(np.unique(pd1)) <= {'yes', 'no'}
    assert {k.lower() for k in ev0} >= {'loss', 'auc'} and all(np.isfinite(ev1[k]) for k in ev1)
