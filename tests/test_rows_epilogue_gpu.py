# -*- coding:utf-8 -*-
"""GPU: the row epilogue of the weight-gradient launch (csrc/deepfm.hip rows_epilogue_wave) at the smallest shapes at which
its pipelined, work-pulled loop can go wrong.  The fast body (in-step Adam, no embedding dropout, row-major gradient rows)
pulls chunks of kRowsStage = 2 passes and keeps the loads of the next chunk in flight while it finishes the current one;
the generic body (dropout here; field-major rows in tests/test_parallel_gpu.py) pulls chunks of kRowsUB = 4 passes.

Lanes per batch row (F D / 4) and what each shape is there for:
  10   (F = 5,  D = 8)    six rows per pass, four idle lanes, a ragged last pass
  56   (F = 7,  D = 32)   one row per pass, eight idle lanes
  64   (F = 16, D = 16)   exactly one wave per row
  68   (F = 17, D = 16)   two parts of 34 lanes: every wave has idle lanes
  104  (F = 26, D = 16)   the benchmarked shape
  128  (F = 32, D = 16)   the limit: two full half-row waves
Batch sizes: 1 and 31 (one partial tile), 33 (one full tile plus one row), one chunk of the fast body plus one row, and
32 * 256 + 5 (some blocks get two tiles; within a block some waves get no chunk, exactly one, or only a ticket past the end).
Ids: every lookup distinct (all Adam updates), three ids per field (every lookup a segment member: no Adam update once
B >= 31), and a mix with out-of-range ids (-1 and vocab).
Every figure is judged by oracle.headline.rows_in_step_ok / check_in_step_vs_oracle: their bars, none of this file's own."""
import pytest
import torch

import tests.test_fused_gpu as T

pytestmark = pytest.mark.gpu

kTM, kRowsStage = 32, 2                 # csrc/deepfm.hip: batch rows per tile, passes per stage of the fast body
VOCAB = 8300                            # >= the largest batch: a field's lookups can all be distinct
BIG = 32 * 256 + 5

# (F, D, Nd)
SHAPES = [(5, 8, 3), (7, 32, 3), (16, 16, 3), (17, 16, 3), (26, 16, 13), (32, 16, 0)]
ID_MODES = ['distinct', 'segments', 'mixed']


def chunk_plus_one(F, D):
    tpr = F * D // 4
    rpw = 64 // tpr if tpr <= 64 else 1
    return rpw * kRowsStage + 1


def batch_sizes(F, D):
    return [1, 31, 33, chunk_plus_one(F, D), BIG]


# each shape meets every batch size; the id modes rotate so that every (shape, mode) and every (batch size, mode) pair occurs
POINTS = [(F, D, Nd, B, ID_MODES[(si + bi) % 3]) for si, (F, D, Nd) in enumerate(SHAPES)
          for bi, B in enumerate(batch_sizes(F, D))]


def _build(net, F, D, Nd, **extra):
    from deeptables_amd.models import deepnets
    kw = dict(nets=deepnets.DCN, cross_params={'num_cross_layer': 3}) if net == 'DCN' else {}
    dm, cats = T.build(F, Nd, D, vocab=VOCAB, **kw, **extra)
    if net == 'DCN':                    # cross biases start at zero: give them some size
        g = torch.Generator().manual_seed(11)
        with torch.no_grad():
            cr = dm.model.layers_by_name['dcn_cross_layer']
            cr.bias_stack.add_(torch.randn(cr.bias_stack.shape, generator=g).to(cr.bias_stack.device) * 0.05)
    return dm, cats


def _ids(cats, idx, mode, seed):
    """T.batch's ids reshaped to the mode.  Out-of-range ids stay off the first field's -1 and the last field's vocab, so that
    id + row offset is still a row of the table for the checker's snapshot (a neighbouring field's row: unchanged by both paths)."""
    B, F = idx.shape
    g = torch.Generator().manual_seed(100 + seed)
    if mode == 'distinct':
        return torch.stack([torch.randperm(c.vocabulary_size, generator=g)[:B] for c in cats], 1)
    if mode == 'segments':
        return idx % 3
    idx = idx % max(B // 2, 2)           # about half of the lookups share their row with another
    if F > 1:
        idx[0::5, F - 1] = -1
        idx[1::5, 0] = cats[0].vocabulary_size
    return idx


def _two_steps(dev, dm, cats, net, Nd, B, mode):
    from oracle import headline
    for seed in (5, 6):                 # the second step starts from the slots the first one left
        idx, dense, y = T.batch(cats, Nd, B, seed=seed)
        idx = _ids(cats, idx, mode, seed).to(torch.int32).to(dev)
        dd = dense.to(dev) if Nd else None
        res = headline.check_rows_in_step(dm, (idx, dd, y.to(dev)), steps=1)
        print(net, B, mode, seed, sorted(res.items()))
        if net == 'DCN' and B == 1:
            # BatchNormalization over one row outputs beta whatever its input, and in DCN every path from the table runs through
            # it: the rows' gradient is exactly zero and both paths must leave them where they are
            assert res['rows_moved'] == 0 and headline.rows_in_step_ok(dict(res, rows_moved=1.0)), str(sorted(res.items()))
        else:
            assert headline.rows_in_step_ok(res), str((seed, sorted(res.items())))
        dm.train_step([idx] + ([dd] if Nd else []), y.to(dev))     # move on (in-step path)


@pytest.fixture(scope='module')
def models():
    """one model per (net, shape), shared by that shape's batch sizes: its state simply moves on from case to case"""
    cache = {}

    def get(net, F, D, Nd):
        key = (net, F, D, Nd)
        if key not in cache:
            cache[key] = _build(net, F, D, Nd)
        return cache[key]
    return get


@pytest.mark.parametrize('net', ['DeepFM', 'DCN'])
@pytest.mark.parametrize('F,D,Nd,B,mode', POINTS)
def test_fast_body_equals_the_separate_optimizer_step(dev, monkeypatch, models, net, F, D, Nd, B, mode):
    """the in-step row update through the fast body against forward_backward + optimizer.step, two steps in a row"""
    from deeptables_amd.models import layers as dl
    monkeypatch.setattr(dl, 'DENSE_GRAD_MAX_ELEMS', 0)          # row-sparse update also on these small tables
    dm, cats = models(net, F, D, Nd)
    assert type(dm.fused_plan()).__name__ == 'Fused' + net
    _two_steps(dev, dm, cats, net, Nd, B, mode)


@pytest.mark.parametrize('net', ['DeepFM', 'DCN'])
@pytest.mark.parametrize('drop', [0.3, 0.0])
def test_body_selection_with_and_without_embedding_dropout(dev, monkeypatch, net, drop):
    """the same model and batches with embedding dropout 0.3 (generic body: p read from the table, the keep-mask on the
    gradient) and without (fast body), two parts with idle lanes, several tiles per block's share and a ragged last one"""
    from deeptables_amd.models import layers as dl
    monkeypatch.setattr(dl, 'DENSE_GRAD_MAX_ELEMS', 0)
    F, D, Nd = 17, 16, 3
    dm, cats = _build(net, F, D, Nd, embedding_dropout=drop)
    assert type(dm.fused_plan()).__name__ == 'Fused' + net
    _two_steps(dev, dm, cats, net, Nd, 2 * kTM * 8 + 7, 'mixed')


@pytest.mark.parametrize('net', ['DeepFM', 'DCN'])
def test_chained_steps_run_the_election_before_the_matrix_waves_join(dev, monkeypatch, net):
    """chained steps through FusedDeepFM.run(next_ids=..., prepared=...): the matrix waves run the next step's election and
    only then pull chunks of the row epilogue; the result is that of plain steps (test_fused_gpu's body and bounds)"""
    monkeypatch.setenv('DT_AMD_TOWER_DTYPE', 'bf16x3')
    T.chained_steps_equal_plain_steps(dev, monkeypatch, net, 3000, 1029, 'bf16x3', 17, 3, 16)


@pytest.mark.parametrize('net', ['DeepFM', 'DCN'])
def test_fast_body_matches_oracle_adam_over_three_steps(dev, monkeypatch, net):
    """three consecutive steps against the float64 oracle's own Keras Adam and running slots (warm rows from step 2 on) at the
    benchmarked row shape, with a ragged last tile (B = 16 tiles + 5 rows).  The checker's gradient band (g_band = 2e-6 of a
    row's largest |g|) was set at this model: at F = 5, D = 8 (B = 333) the step before this file's change and the step after
    it both miss `upd_tol` by the same figure (rows_p_err 4.75e-3 of a step for both), so smaller models are no case of
    this check."""
    from oracle import headline
    from deeptables_amd.models import deepnets, layers as dl
    monkeypatch.setattr(dl, 'DENSE_GRAD_MAX_ELEMS', 0)
    F, Nd, D, B = 26, 13, 16, 517
    extra = dict(nets=deepnets.DCN, cross_params={'num_cross_layer': 3}) if net == 'DCN' else {}
    dm, cats = T.build(F, Nd, D, vocab=300, **extra)
    batches = []
    for s in range(3):
        idx, dense, y = T.batch(cats, Nd, B, seed=20 + s)
        batches.append((idx.int().to(dev), dense.to(dev), y.to(dev)))
    res = headline.check_in_step_vs_oracle(dm, batches)
    print(net, sorted(res.items()))
    assert res['ok'] and res['steps_counted'] == 3 and res['warm_rows'] > 0, str(sorted(res.items()))
