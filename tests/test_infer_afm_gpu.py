# -*- coding:utf-8 -*-
"""GPU: the fused AFM inference plan (fused.InferAFM: one dt_afm_infer_prepare launch per predict / evaluate, one k_afm_infer
launch per batch — gather, `linear` / `fm_nets` from the raw rows, the AFM layer on the exact-fp32 matrix core with an online
softmax over the pairs, Add, task_output, the activation; csrc/afm_infer.hip) against the float64 oracle at inference, held
to the forward class tests/precision.py gives the AFM kernel ('afm', 'float32'): over the shapes at which the kernel takes
another path (one pair, P not a multiple of 16, every embedding size, H below / at the compiled widths, the most pairs), all
four net masks, every activation, pair logits beyond +-100, the grid stride, row independence, odd ids, and end to end
through fit / predict / evaluate against the layer-by-layer path."""
import numpy as np
import pytest
import torch

from tests import precision as P
from tests.infer_support import _frame, _ins, _oracle, _train_and_perturb, run_plan

pytestmark = pytest.mark.gpu

AFM, LIN, FM = ['afm_nets'], ['linear', 'afm_nets'], ['afm_nets', 'fm_nets']
ALL = ['linear', 'fm_nets', 'afm_nets']
EMB_SCALE = 8.0


def _b_big():
    """more rows than two residencies of the launch: its grid is at most DT_AFM_INFER_MAX_BLOCKS blocks of DT_AFM_INFER_ROWS
    waves (include/dt_hip.h), one row per wave at a time — so every wave scores a second and 131 a third row, which come out
    of the prefetch chain (table rows one pass ahead, ids two)"""
    from deeptables_amd import _lib
    return 2 * _lib.DT_AFM_INFER_MAX_BLOCKS * _lib.DT_AFM_INFER_ROWS + 131


def _build(F=26, D=16, H=16, nets=LIN, Nd=0, act=None, vocab=30, dropout=0, **kw):
    import tests.test_fused_gpu as T
    ap = {'hidden_factor': H, 'dropout_rate': dropout}
    if act is not None:
        ap['activation'] = act
    return T.build(F, Nd, D, vocab=vocab, nets=list(nets), afm_params=ap, **kw)


def _trained(dm, cats, Nd, dev, steps=2, train=True):
    """tests.test_infer_gpu._train_and_perturb: `steps` train steps on the layer path, then the embedding rows scaled up.
    train=False, for the one shape whose AFM backward lies outside the layer path's own domain (NO_BACKWARD): the parameters
    leave their initial values by a seeded perturbation instead — the plan under test is the same either way.  Every other
    shape trains, and a refusal there is an error."""
    if train:
        _train_and_perturb(dm, cats, Nd, dev, steps=steps)
    else:
        g = torch.Generator().manual_seed(33)
        with torch.no_grad():
            for _, p in dm.model.named_parameters():
                p.mul_(1.0 + 0.2 * torch.randn(p.shape, generator=g).to(p.device))
    # the embedding rows start out at a few hundredths, which leaves the pair products (and with them the whole AFM term) far
    # below the other terms of the logit: scaled up, an error in the attention pooling shows in the figures
    with torch.no_grad():
        for t in dm.model.layers_by_name['emb_categorical_vars_all'].tables.values():
            t.mul_(EMB_SCALE)


def _run_plan(dm, idx, dense, dev, kind='int32'):
    from deeptables_amd import fused
    return run_plan(dm, idx, dense, dev, fused.InferAFM, kind)


def _figs(dm, logit, out, r64, r32):
    figs = {'logit': ('fwd', P.max_rel(logit, r64), P.max_rel(r32, r64))}
    if dm.output_activation == 'sigmoid':
        figs['prob'] = ('fwd', P.max_rel(out, torch.sigmoid(r64)), P.max_rel(torch.sigmoid(r32.double()), torch.sigmoid(r64)))
    else:
        assert torch.equal(out, logit)
    return figs


def _check(dm, idx, dense, dev, label, kind='int32', weights=None, ids_oracle=None):
    logit, out = _run_plan(dm, idx, dense, dev, kind)
    ids_o = idx if ids_oracle is None else ids_oracle
    w64 = weights(torch.float64) if weights else None
    w32 = weights(torch.float32) if weights else None
    r64 = _oracle(dm, ids_o, dense, torch.float64, w64)
    r32 = _oracle(dm, ids_o, dense, torch.float32, w32)
    assert bool(torch.isfinite(r64).all())
    figs = _figs(dm, logit, out, r64, r32)
    print(label, {k: (g, f) for k, (_, g, f) in figs.items()})
    P.check_step(label, 'afm', 'float32', figs)
    return logit, out


# (F, D, H), nets: one pair (the softmax is 1); the smallest D and H; P = 136, neither a multiple of 16 nor of 64; the
# benchmark, P = 325; F D at the limit; D = 32; odd H below the compiled width at D = 64; the most pairs (8128) and widest H
SHAPES = [((2, 16, 16), AFM), ((3, 4, 1), LIN), ((17, 16, 16), FM), ((26, 16, 16), ALL), ((32, 16, 4), AFM),
          ((16, 32, 16), LIN), ((8, 64, 5), ALL), ((128, 4, 64), FM)]
# dt_afm_bwd keeps [P][H] floats in LDS: P = 8128 pairs x 64 is 2 MB, so the layer path cannot train this shape (its forward,
# and with it the DT_AMD_FUSED_PREDICT=0 path, can)
NO_BACKWARD = (128, 4, 64)


@pytest.mark.parametrize('shape,nets', SHAPES, ids=lambda v: '-'.join(map(str, v)))
def test_plan_matches_the_oracle_after_training(dev, shape, nets):
    import tests.test_fused_gpu as T
    F, D, H = shape
    dm, cats = _build(F=F, D=D, H=H, nets=nets)
    if shape == NO_BACKWARD:
        from deeptables_amd import _lib
        idx, dense, y = T.batch(cats, 0, 64, seed=21)
        with pytest.raises(_lib.DtHipError, match='dt_afm_bwd'):
            dm.train_step(_ins(idx, dense, dev), y.to(dev))
    _trained(dm, cats, 0, dev, train=shape != NO_BACKWARD)
    plan = dm.inference_plan()
    assert (plan.F, plan.D, plan.H) == (F, D, H)
    idx, dense, _ = T.batch(cats, 0, 203, seed=41)
    _check(dm, idx, dense, dev, f'afm_infer[{F},{D},{H},{"+".join(nets)}]')


@pytest.mark.parametrize('variant', ['continuous_13', 'no_output_bias'])
def test_continuous_columns_and_no_output_bias(dev, variant):
    import tests.test_fused_gpu as T
    Nd = 13 if variant == 'continuous_13' else 0
    dm, cats = _build(F=11, D=16, H=16, nets=ALL if Nd else LIN, Nd=Nd, use_bias=variant != 'no_output_bias')
    _trained(dm, cats, Nd, dev)
    assert (dm.model.layers_by_name['task_output'].bias is None) == (variant == 'no_output_bias')
    idx, dense, _ = T.batch(cats, Nd, 203, seed=6)
    _check(dm, idx, dense, dev, f'afm_infer[{variant}]')


def test_regression_task(dev):
    import tests.test_fused_gpu as T
    dm, cats = _build(F=9, D=16, H=8, nets=LIN, task='regression')
    _trained(dm, cats, 0, dev)
    idx, dense, _ = T.batch(cats, 0, 70, seed=8)
    logit, out = _check(dm, idx, dense, dev, 'afm_infer_regression')
    assert torch.equal(out, logit)


@pytest.mark.parametrize('act', ['linear', 'sigmoid', 'tanh', 'elu', 'selu', 'softplus', 'softsign', 'exponential'])
def test_every_other_activation(dev, act):
    import tests.test_fused_gpu as T
    from deeptables_amd import _lib
    dm, cats = _build(F=9, D=16, H=8, nets=LIN, act=act, dropout=0.25)
    _trained(dm, cats, 0, dev)
    assert dm.inference_plan().act == _lib.ACT_CODES[act]
    idx, dense, _ = T.batch(cats, 0, 203, seed=12)
    _check(dm, idx, dense, dev, f'afm_infer_act[{act}]')


def test_pair_logits_beyond_plus_minus_100(dev):
    """projection_h is scaled until the float64 oracle's own pair logits l_p = act(bi_p Wa + ba) . h span beyond +-100; the
    oracle stays finite there, and so must the kernel: without the running max e^l overflows"""
    import tests.test_fused_gpu as T
    from oracle import bridge
    dm, cats = _build(F=17, D=16, H=16, nets=AFM)
    _trained(dm, cats, 0, dev)
    idx, dense, _ = T.batch(cats, 0, 203, seed=3)

    def pair_logits():
        w = bridge.oracle_weights(dm, torch.float64)
        a = w['afm'][0]
        x = torch.stack([t[idx[:, f]] for f, t in enumerate(w['emb_categorical_vars_all'])], 1)     # [B, F, D]
        i, j = torch.triu_indices(len(cats), len(cats), 1)
        pre = (x[:, i] * x[:, j]) @ a['att_kernel'] + a['att_bias']
        return (torch.relu(pre) @ a['projection_h']).squeeze(-1)

    l0 = pair_logits()
    assert l0.max() > 0 > l0.min()
    afm = dm.model.layers_by_name['afm_layer']
    with torch.no_grad():
        afm.attention_p.mul_(150.0 / float(min(l0.max(), -l0.min())))
    lp = pair_logits()
    print('pair logits', float(lp.min()), float(lp.max()))
    assert lp.max() > 100 and lp.min() < -100
    logit, out = _check(dm, idx, dense, dev, 'afm_infer_softmax_range')
    assert bool(torch.isfinite(logit).all()) and bool(torch.isfinite(out).all())


@pytest.fixture(scope='module')
def trained(dev):
    """a small graph with all three nets after two steps; the frame of B_BIG rows and the float64 / float32 oracle logits of
    those rows (computed once, never changed)"""
    import tests.test_fused_gpu as T
    dm, cats = _build(F=5, D=8, H=4, nets=ALL, Nd=3)
    _trained(dm, cats, 3, dev)
    idx, dense, _ = T.batch(cats, 3, _b_big(), seed=77)
    r64 = _oracle(dm, idx, dense, torch.float64)
    r32 = _oracle(dm, idx, dense, torch.float32)
    return dm, cats, idx, dense, r64, r32


@pytest.mark.parametrize('B', [1, 5, 'big'])
def test_grid_stride(dev, trained, B):
    """one row; a partial block; more rows than two residencies of the launch"""
    dm, cats, idx, dense, r64, r32 = trained
    B = _b_big() if B == 'big' else B
    logit, out = _run_plan(dm, idx[:B], dense[:B], dev)
    figs = _figs(dm, logit, out, r64[:B], r32[:B])
    print(f'afm_infer_grid[{B}]', {k: (g, f) for k, (_, g, f) in figs.items()})
    P.check_step(f'afm_infer_grid[{B}]', 'afm', 'float32', figs)


def test_rows_are_independent_of_their_place_in_the_batch(dev, trained):
    dm, cats, idx, dense, _, _ = trained
    n = 3000
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(5))
    a = _run_plan(dm, idx[:n], dense[:n], dev)
    b = _run_plan(dm, idx[:n][perm], dense[:n][perm], dev)
    small = _run_plan(dm, idx[:7], dense[:7], dev)
    for x, y, z in zip(a, b, small):
        assert torch.equal(x[perm.to(dev)], y)
        assert torch.equal(x[:7], z)


def test_float_and_int_ids_give_the_same_bits(dev, trained):
    dm, cats, idx, dense, _, _ = trained
    a = _run_plan(dm, idx[:300], dense[:300], dev, 'int32')
    b = _run_plan(dm, idx[:300], dense[:300], dev, 'float32')
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize('kind', ['int32', 'float32'])
def test_out_of_range_and_fractional_ids(dev, kind):
    """an out-of-range id (negative, equal to vocab, huge) reads a zero row and is counted once per lookup; a float id is
    truncated.  The oracle gets a zero row appended to each table and the out-of-range ids pointed at it; the rows of the
    batch without a bad id keep the bits they have in a batch without any."""
    import tests.test_fused_gpu as T
    from oracle import bridge
    from tests.test_fused_domain_gpu import _odd_ids
    dm, cats = _build(F=17, D=16, H=16, nets=ALL, vocab=60)
    _trained(dm, cats, 0, dev, steps=1)
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
        logit, out = _check(dm, ids, dense, dev, f'afm_infer_ids[{kind}]', kind=kind, weights=weights, ids_oracle=ids_o)
        torch.cuda.synchronize()
        assert int(emb.oob_count.item()) == n_oob
    finally:
        emb.check_oob = False
    clean = ~bad.any(1)
    assert 0 < int(clean.sum()) < len(clean)
    ref_logit, ref_out = _run_plan(dm, trunc.clamp(min=0).minimum(vocab - 1), dense, dev)
    assert torch.equal(logit[clean.to(dev)], ref_logit[clean.to(dev)]) and torch.equal(out[clean.to(dev)], ref_out[clean.to(dev)])


def test_the_layer_path_is_not_run(dev, monkeypatch):
    dm, cats = _build(F=7, D=16, H=16, nets=LIN)
    df, y = _frame(cats, 0, 300, 2)

    def boom(*a, **k):
        raise AssertionError('the layer-by-layer forward ran')
    monkeypatch.setattr(dm.model, 'forward', boom)
    p = dm.predict(df, batch_size=128)
    assert p.shape == (300, 1) and np.isfinite(p).all()
    res = dm.evaluate(df, y, batch_size=64)
    assert np.isfinite(res['loss'])


def test_fit_predict_evaluate_against_the_layer_path(dev, monkeypatch):
    """DeepTable end to end at (F, D, H) = (26, 16, 16), 300 rows, batch_size 128: fit with a validation split (its validation
    pass runs the plan), then predict_proba, predict and evaluate with the plan and with DT_AMD_FUSED_PREDICT=0 (the layer
    path) on the same trained model.  predict_proba's second column is held to the class bar through the oracle on both
    paths, not fused against layer path alone.  The metrics then agree to what that bar implies: two probabilities within
    tol = 2 x bar of each other move the mean BCE by at most tol / min(p, 1 - p), the AUC by the share of (positive,
    negative) pairs whose oracle probabilities lie closer than tol, and a label only where the probability is within tol
    of 0.5."""
    import pandas as pd
    from deeptables_amd.models import DeepTable, ModelConfig
    rng = np.random.default_rng(0)
    n, F, Nd = 300, 26, 13
    df = pd.DataFrame({f'c{i:02d}': rng.choice([f'v{k}' for k in range(5 + i % 7)], n) for i in range(F)})
    for j in range(Nd):
        df[f'x{j:02d}'] = rng.normal(0.0, 1.0, n).astype(np.float32)
    y = pd.Series(((df['x03'] > 0) ^ (df['c01'] == 'v1'))).map({True: 'yes', False: 'no'})
    conf = ModelConfig(nets=LIN, metrics=['AUC'], earlystopping_patience=0, fixed_embedding_dim=True, embeddings_output_dim=16,
                       afm_params={'hidden_factor': 16, 'dropout_rate': 0})
    dt = DeepTable(config=conf)
    _, hist = dt.fit(df, y, batch_size=128, epochs=2, verbose=0, validation_split=0.2)
    assert 'val_loss' in hist.history
    dm = dt.model
    plan = dm.inference_plan()
    assert type(plan).__name__ == 'InferAFM' and (plan.F, plan.D, plan.Nd, plan.H) == (F, 16, Nd, 16)
    pr1, pd1, ev1 = dt.predict_proba(df, batch_size=128), dt.predict(df, batch_size=128), dt.evaluate(df, y, batch_size=128)
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
    P.check_step('afm_infer_deeptable', 'afm', 'float32', figs)
    for pr in (pr1, pr0):
        assert np.array_equal(pr[:, 0], 1.0 - pr[:, 1])
    pr = r64.reshape(-1)
    tol = 2 * P.STEP_BAR['fp32'] * max(f32, P.FLOOR) * float(pr.max())
    undecided = ((pr - 0.5).abs() <= tol).numpy()
    assert np.array_equal(np.asarray(pd1)[~undecided], np.asarray(pd0)[~undecided])
    assert set(np.unique(pd1)) <= {'yes', 'no'}
    loss_tol = tol / max(float(torch.minimum(pr, 1 - pr).min()), 1e-7)       # 1e-7: where binary cross-entropy clips p
    yt = torch.as_tensor(dt.preprocessor.transform_y(y))
    pos, neg = pr[yt > 0.5], pr[yt <= 0.5]
    auc_tol = float(((pos[:, None] - neg[None, :]).abs() <= tol).sum()) / max(1, len(pos) * len(neg)) + 1e-7
    assert {k.lower() for k in ev0} >= {'loss', 'auc'}
    for k in ev0:
        bound = auc_tol if k.lower() == 'auc' else loss_tol
        assert abs(ev1[k] - ev0[k]) <= bound + 4 * P.U * abs(ev0[k]), (k, ev1[k], ev0[k], bound)


def test_a_launch_that_does_not_match_the_prepared_workspace_scores_nan(dev):
    """the workspace names the (F, D, Nd, compiled H, nets) it was prepared for; a launch with another compiled width or net
    mask reads no weight from where another layout put it: every logit and output is NaN"""
    import tests.test_fused_gpu as T
    from deeptables_amd import _lib
    dm, cats = _build(F=7, D=16, H=16, nets=LIN, Nd=3)
    idx, dense, _ = T.batch(cats, 3, 37, seed=2)
    good = _run_plan(dm, idx, dense, dev)
    assert bool(torch.isfinite(good[0]).all()) and bool(torch.isfinite(good[1]).all())
    plan = dm.inference_plan()
    ins = _ins(idx, dense, dev)
    for attr, other in (('H', 17), ('mask', _lib.DT_NET_AFM | _lib.DT_NET_LINEAR | _lib.DT_NET_FM)):
        keep = getattr(plan, attr)
        plan.prepare()
        setattr(plan, attr, other)
        try:
            logit = torch.zeros((37, 1), dtype=torch.float32, device=dev)
            out = torch.zeros_like(logit)
            plan.infer(ins[0], ins[1], logit, out)
            torch.cuda.synchronize()
        finally:
            setattr(plan, attr, keep)
        assert bool(torch.isnan(logit).all()) and bool(torch.isnan(out).all()), attr
    again = _run_plan(dm, idx, dense, dev)
    assert torch.equal(again[0], good[0]) and torch.equal(again[1], good[1])
