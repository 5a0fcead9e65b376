# -*- coding:utf-8 -*-
"""GPU: the fused DeepFM / DCN steps at the corners of the domain the library's own predicates accept (csrc/deepfm.hip
deepfm_dims, dt_dcn_supported, step_chains), not only at the handful of shapes the other files use.

Each corner is there for what only it exercises:
  D = 64                the LPR = 16 instance of k_sparse_fwd; 16 pieces per field in rows_epilogue_wave
  Nd = 64               every lane of kernel A's wave carries a continuous value; dwlin / BN vectors at full width
  F = 1                 FM with no pairs, a one-field election, TPR = 1 (64 rows per epilogue pass)
  F = 127 / 128, D = 4  128 fields in the election and in FM; F = 127: an odd TPR > 64, the second half-wave has an idle lane
  F = 16, D = 16        TPR = 64 exactly: parts = 1, rpw = 1, the switch point of the epilogue's lane split
  C = 544 (CP = 576)    the bf16x3 mode runs the exact fp32 tile (the split tile stops at CP = 512): held to the fp32 class
  DCN at CP = 512, L = 8  the split-bf16 DCN tile near the top of its LDS
  B = 1, 2              one partial 32-row tile; BatchNormalization over one row (variance 0)
tests/test_host_api.py asks the library that every corner here is accepted and the first shape past each limit refused."""
import pytest
import torch

from tests import precision as P

pytestmark = pytest.mark.gpu

H1, H2 = 128, 64

# (F, D, Nd): accepted by dt_deepfm_supported
DEEPFM_CORNERS = [(8, 64, 0), (7, 64, 64), (8, 64, 32), (1, 4, 0), (1, 4, 64), (127, 4, 0), (128, 4, 32), (16, 16, 0),
                  (32, 16, 32)]
# (F, D, Nd, L): accepted by dt_dcn_supported
DCN_CORNERS = [(32, 16, 0, 8), (7, 64, 0, 8), (128, 4, 0, 8), (1, 4, 0, 1), (1, 4, 64, 2)]
# accepted by DeepFM, refused by DCN at every L: the tile kernel's LDS (ldsD) passes 160 KB
DCN_REFUSED = [(8, 64, 0), (7, 64, 64)]
# (F, D, Nd): the first shape past each limit of deepfm_dims
DEEPFM_PAST = {'D = 128': (1, 128, 0), 'D = 12 (3 lanes)': (1, 12, 0), 'F D / 4 = 129': (129, 4, 0), 'Nd = 65': (1, 4, 65),
               'C = 545': (32, 16, 33)}
DCN_PAST_L = (0, 9)


def cp_of(F, D, Nd):
    return (F * D + Nd + 63) // 64 * 64


# the batch sizes of each corner in the class check: every corner meets a partial tile, all of B = 1, 2, 33, 65, 129 occur
CLASS_POINTS = ([('DeepFM', F, D, Nd, None, B) for (F, D, Nd), Bs in zip(DEEPFM_CORNERS, [
                    (1, 65), (2, 129), (33, 129), (1, 129), (2, 65), (33, 65), (1, 33), (2, 129), (65, 129)]) for B in Bs] +
                [('DCN', F, D, Nd, L, B) for (F, D, Nd, L), Bs in zip(DCN_CORNERS, [
                    (1, 65), (2, 129), (33, 65), (1, 129), (2, 33)]) for B in Bs])


def _build(net, F, D, Nd, L, vocab=30):
    import tests.test_fused_gpu as T
    from deeptables_amd.models import deepnets
    kw = {}
    if net == 'DCN':
        kw = dict(nets=deepnets.DCN, cross_params={'num_cross_layer': L},
                  dnn_params={'hidden_units': ((H1, 0, False), (H2, 0, False)), 'activation': 'relu'})
    dm, cats = T.build(F, Nd, D, vocab=vocab, **kw)
    if net == 'DCN':                # cross biases start at zero: give them some size
        g = torch.Generator().manual_seed(11)
        with torch.no_grad():
            cr = dm.model.layers_by_name['dcn_cross_layer']
            cr.bias_stack.add_(torch.randn(cr.bias_stack.shape, generator=g).to(cr.bias_stack.device) * 0.05)
    return dm, cats


@pytest.mark.parametrize('mode', ['bf16x3', 'f32', 'bf16'])
@pytest.mark.parametrize('net,F,D,Nd,L,B', CLASS_POINTS)
def test_fused_step_holds_its_class_at_the_corners(dev, monkeypatch, mode, net, F, D, Nd, L, B):
    """logits, loss, every dense gradient and the table gradient row by row against the float64 oracle, measured against the
    float32 oracle's own error (test_precision_gpu.test_fused_step_holds_its_class at the corners).  At CP = 576 the bf16x3
    mode must run the exact tile and its exact weight-gradient GEMMs: it is held to the ('tower', 'f32') class."""
    import tests.test_fused_gpu as T
    from tests.test_precision_gpu import _step_figures
    from deeptables_amd import fused
    monkeypatch.setenv('DT_AMD_TOWER_DTYPE', mode)
    dm, cats = _build(net, F, D, Nd, L)
    plan = dm.fused_plan()
    assert type(plan).__name__ == 'Fused' + net
    assert plan.tower_flag == fused._tower_mfma_flag({'mfma_dtype': mode})
    idx, dense, y = T.batch(cats, Nd, B)
    ins = [idx.int().to(dev)] + ([dense.to(dev)] if Nd else [])
    held = 'f32' if mode == 'bf16x3' and cp_of(F, D, Nd) > 512 else mode
    figs = _step_figures(dm, idx, dense, y, ins, y.to(dev), P.CLAIMS[('tower', held)][0])
    P.check_step(f'corner[{mode},{net},{B},{F},{D},{Nd},{L}]', 'tower', held, figs)


# ---- the step modes at the corners ---------------------------------------------------------------------------------------
ROWS_POINTS = [('DeepFM', 8, 64, 0, None, 129), ('DeepFM', 128, 4, 0, None, 129), ('DeepFM', 1, 4, 0, None, 129),
               ('DeepFM', 7, 64, 64, None, 65), ('DeepFM', 1, 4, 64, None, 65), ('DeepFM', 16, 16, 0, None, 1),
               ('DCN', 7, 64, 0, 8, 129), ('DCN', 128, 4, 0, 8, 129), ('DCN', 1, 4, 0, 1, 129), ('DCN', 1, 4, 64, 2, 65),
               ('DCN', 32, 16, 0, 8, 1), ('DCN', 32, 16, 0, 8, 2)]


@pytest.mark.parametrize('mode', ['bf16x3', 'f32'])
@pytest.mark.parametrize('net,F,D,Nd,L,B', ROWS_POINTS)
def test_rows_in_step_equals_the_separate_optimizer_step_at_the_corners(dev, monkeypatch, mode, net, F, D, Nd, L, B):
    """the in-step Keras Adam (dt_deepfm_train_step_adam / dt_dcn_train_step_adam) against forward_backward + optimizer.step,
    as test_fused_gpu.test_rows_in_step_equals_the_separate_optimizer_step does at the default shape: a first batch from zero
    slots, a second from the slots the first left.  DCN at B = 1: BatchNormalization over one row outputs beta whatever its input,
    and in DCN (no FM, no linear term) every path from the table runs through it — the rows' gradient is exactly zero and
    both paths must leave them where they are."""
    import tests.test_fused_gpu as T
    from deeptables_amd.models import layers as dl
    from oracle import headline
    monkeypatch.setenv('DT_AMD_TOWER_DTYPE', mode)
    monkeypatch.setattr(dl, 'DENSE_GRAD_MAX_ELEMS', 0)
    dm, cats = _build(net, F, D, Nd, L)
    assert type(dm.fused_plan()).__name__ == 'Fused' + net
    for seed in (5, 6):
        idx, dense, y = T.batch(cats, Nd, B, seed=seed)
        dd = dense.to(dev) if Nd else None
        res = headline.check_rows_in_step(dm, (idx.to(torch.int32).to(dev), dd, y.to(dev)), steps=1)
        if net == 'DCN' and B == 1:
            assert res['rows_moved'] == 0 and headline.rows_in_step_ok(dict(res, rows_moved=1.0)), str(sorted(res.items()))
        else:
            assert headline.rows_in_step_ok(res), str(sorted(res.items()))
        dm.train_step([idx.to(torch.int32).to(dev)] + ([dd] if Nd else []), y.to(dev))


@pytest.mark.parametrize('mode', ['bf16x3', 'f32'])
@pytest.mark.parametrize('net,F,D,Nd', [('DeepFM', 8, 64, 0), ('DeepFM', 128, 4, 0), ('DCN', 128, 4, 0)])
def test_chained_steps_at_the_chain_limit(dev, monkeypatch, mode, net, F, D, Nd):
    """B = 8192, the largest batch the chain takes, away from the benchmarked shape: four chained steps leave the weights,
    tables and slots of four plain steps (test_fused_gpu.chained_steps_equal_plain_steps, same bounds).  B = 8193 is not
    chained, and its plain step still agrees with the separate optimizer step."""
    import tests.test_fused_gpu as T
    from deeptables_amd.models import deepnets, layers as dl
    from oracle import headline
    monkeypatch.setenv('DT_AMD_TOWER_DTYPE', mode)
    T.chained_steps_equal_plain_steps(dev, monkeypatch, net, 3000, 8192, mode, F, Nd, D)
    monkeypatch.setattr(dl, 'DENSE_GRAD_MAX_ELEMS', 0)
    kw = dict(nets=deepnets.DCN, cross_params={'num_cross_layer': 5}) if net == 'DCN' else {}
    dm, cats = T.build(F, Nd, D, vocab=3000, **kw)
    plan = dm.fused_plan()
    assert type(plan).__name__ == 'Fused' + net
    assert not plan.can_chain(8193)
    idx, dense, y = T.batch(cats, Nd, 8193, seed=80)
    res = headline.check_rows_in_step(dm, (idx.to(torch.int32).to(dev), dense.to(dev) if Nd else None, y.to(dev)), steps=1)
    assert headline.rows_in_step_ok(res), str(sorted(res.items()))


# ---- out-of-range and fractional ids against the oracle -------------------------------------------------------------------
OOB_FIELD, FRAC_FIELD = 1, 2          # out-of-range ids go to field 1 (and the last field), fractional in-range ids to field 2


def _odd_ids(cats, idx, kind):
    """-> (ids [B, F] int32 or float32 with out-of-range / fractional entries, number of out-of-range lookups).
    In the out-of-range fields no in-range lookup takes the rows a clamped read would hit (id 0 and vocab - 1), so a step that
    read or updated them for an out-of-range id shows."""
    idx = idx.clone()
    last = len(cats) - 1
    for f in (OOB_FIELD, last):
        v = cats[f].vocabulary_size
        col = idx[:, f]
        col[(col == 0) | (col == v - 1)] = 1
    if kind == 'int32':
        for f in (OOB_FIELD, last):
            v = cats[f].vocabulary_size
            idx[0::5, f] = -1
            idx[1::5, f] = v
            idx[2::5, f] = v + 999
        n_oob = int(((idx < 0) | (idx >= torch.tensor([c.vocabulary_size for c in cats]))).sum())
        return idx.to(torch.int32), n_oob
    ids = idx.to(torch.float32)
    v = cats[FRAC_FIELD].vocabulary_size
    ids[0::4, FRAC_FIELD] = 3.999                     # -> 3
    ids[1::4, FRAC_FIELD] = -0.5                      # -> 0 (truncation toward zero: in range)
    ids[2::4, FRAC_FIELD] = v - 0.5                   # -> v - 1, in range
    ids[0::3, OOB_FIELD] = -1.0                       # out of range
    ids[1::3, last] = float(cats[last].vocabulary_size) + 0.25     # -> vocab: out of range
    n_oob = int(ids[0::3, OOB_FIELD].numel() + ids[1::3, last].numel())
    return ids, n_oob


@pytest.mark.parametrize('kind', ['int32', 'float32'])
@pytest.mark.parametrize('mode', ['bf16x3', 'f32'])
@pytest.mark.parametrize('net,F,D,Nd,L', [('DeepFM', 26, 16, 13, None), ('DeepFM', 8, 64, 0, None),
                                          ('DCN', 26, 16, 13, 4), ('DCN', 7, 64, 0, 8)])
def test_out_of_range_and_fractional_ids_against_the_oracle(dev, monkeypatch, kind, mode, net, F, D, Nd, L):
    """TF-GPU's embedding_lookup: an out-of-range id reads a zero row and updates nothing; a float id is truncated
    (layers.py:893-895).  One step against oracle.headline.oracle_train_step (its _RowTable gives the zero row) in float64
    and float32: logits, loss, dense gradients and the merged row gradients of the in-range lookups, held to the mode's
    class; the embedding layer counts the out-of-range lookups; an in-step Adam step touches no row and no m / v slot
    outside the in-range rows."""
    import tests.test_fused_gpu as T
    from deeptables_amd.models import layers as dl
    from oracle import headline
    monkeypatch.setenv('DT_AMD_TOWER_DTYPE', mode)
    monkeypatch.setattr(dl, 'DENSE_GRAD_MAX_ELEMS', 0)
    B = 65
    dm, cats = _build(net, F, D, Nd, L, vocab=60)
    plan = dm.fused_plan()
    assert type(plan).__name__ == 'Fused' + net
    idx, dense, y = T.batch(cats, Nd, B, seed=17)
    ids, n_oob = _odd_ids(cats, idx, kind)
    assert n_oob > 0
    ids_d, dense_d, y_d = ids.to(dev), dense.to(dev) if Nd else None, y.to(dev)
    ins = [ids_d] + ([dense_d] if Nd else [])
    r64 = headline.oracle_train_step(dm, ids, dense, y)
    if r64['relu_units_near_kink']:
        headline.shift_tower_biases(dm)
        r64 = headline.oracle_train_step(dm, ids, dense, y, tables_cpu=r64['tables_cpu'])
    r32 = headline.oracle_train_step(dm, ids, dense, y, dtype=torch.float32, tables_cpu=r64['tables_cpu'])
    assert int((r64['rows'] < 0).sum()) == n_oob
    emb = dm.model.layers_by_name['emb_categorical_vars_all']
    emb.check_oob = True
    emb.oob_count.zero_()
    dm.model.train()
    loss, logit = dm.forward_backward(ins, y_d)
    torch.cuda.synchronize()
    assert int(emb.oob_count.item()) == n_oob
    emb.check_oob = False
    figs = {'logit': ('fwd', P.max_rel(logit, r64['logit']), P.max_rel(r32['logit'], r64['logit'])),
            'loss': ('fwd', abs(float(loss) - r64['loss']), abs(r32['loss'] - r64['loss']))}
    g32 = dict((id(p), g) for p, g in headline.oracle_dense_grads(dm, r32['weights']))
    names = {id(p): n for n, p in dm.model.named_parameters()}
    for p, g in headline.oracle_dense_grads(dm, r64['weights']):
        m = P.row_rel if g.dim() >= 2 else P.max_rel
        figs[names[id(p)]] = ('bwd', m(p.grad.reshape(g.shape), g), m(g32[id(p)].reshape(g.shape), g))
    # the row gradients the step handed the optimizer: exactly the in-range rows, each with the oracle's merged gradient
    key = f'd{D}'
    exp = [s.expanded() if hasattr(s, 'expanded') else (s.rows, s.values) for s in emb.sparse_grads[key]]
    u_got, v_got = headline.merge_rows(torch.cat([r.reshape(-1) for r, _ in exp]).cpu(),
                                       torch.cat([v.reshape(-1, D) for _, v in exp]).double().cpu())
    u64, v64 = headline.merge_rows(r64['rows'], r64['row_grads'].double())
    u32, v32 = headline.merge_rows(r32['rows'], r32['row_grads'].double())
    assert torch.equal(u_got, u64) and torch.equal(u32, u64)
    figs['rows'] = ('bwd', P.row_rel(v_got, v64), P.row_rel(v32, v64))
    P.check_step(f'odd_ids[{kind},{mode},{net},{F},{D},{Nd},{L}]', 'tower', mode, figs)
    # one in-step Adam step: only the in-range rows (and their slots) move
    table = emb.tables[key]
    opt = dm.optimizer
    slots = opt._st(table, rows=True)
    t0, m0, v0 = table.detach().clone(), slots['m'].clone(), slots['v'].clone()
    dm._forward_backward(ins, y_d, apply_rows=True)
    assert getattr(opt, '_applied_in_step', False), 'the step did not take the in-step Adam path'
    opt.step()
    torch.cuda.synchronize()
    for name, before, after in (('table', t0, table.detach()), ('m', m0, slots['m']), ('v', v0, slots['v'])):
        moved = ((after - before) != 0).any(1).nonzero().reshape(-1).cpu()
        assert bool(torch.isin(moved, u64).all()), (name, sorted(set(moved.tolist()) - set(u64.tolist()))[:8])
    assert bool((table.detach()[u64.to(dev)] != t0[u64.to(dev)]).any())
