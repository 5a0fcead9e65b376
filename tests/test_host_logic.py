# -*- coding:utf-8 -*-
"""CPU: host-side logic added in round 2 that needs no kernel — the per-lookup view of a segmented sparse gradient
(ops.SparseRowGrad.expanded), Keras' sample / class weighting of the loss (losses.named_loss), the feed carrying
per-row weights through a shuffle (training.TableBatches), balanced class weights (DeepTable.get_class_weight)."""
import os

import numpy as np
import torch


def test_segmented_sparse_grad_expands_to_one_entry_per_lookup():
    from deeptables_amd.ops import SparseRowGrad
    ids = torch.tensor([5, 9, 5, 2, 9, 9, 7, -1, 2], dtype=torch.int64)
    vals = torch.arange(9 * 4, dtype=torch.float32).reshape(9, 4)
    # rows 5 (lookups 0, 2), 9 (1, 4, 5) and 2 (3, 8) are looked up several times -> segments in 2 regions of capacity 3
    regions, cap = 2, 3
    nseg = torch.tensor([2, 1], dtype=torch.int32)
    seg_row = torch.tensor([5, 2, 0, 9, 0, 0], dtype=torch.int64)
    seg_off = torch.tensor([0, 2, 0, 4, 0, 0], dtype=torch.int32)
    seg_cnt = torch.tensor([2, 2, 0, 3, 0, 0], dtype=torch.int32)
    seg_list = torch.tensor([0, 2, 3, 8, 1, 4, 5, 0, 0], dtype=torch.int32)
    rows = ids.clone()
    rows[[0, 2, 3, 8, 1, 4, 5]] = -1
    sg = SparseRowGrad(rows, vals, fields=-1, segments=(nseg, seg_row, seg_off, seg_cnt, seg_list, regions, cap))
    got_rows, got_vals = sg.expanded()
    assert torch.equal(got_rows, ids) and got_vals is vals
    assert torch.equal(rows[[0, 2]], torch.tensor([-1, -1]))        # the stored rows are untouched
    plain = SparseRowGrad(ids, vals)
    assert plain.expanded()[0] is ids
    empty = SparseRowGrad(ids, vals, segments=(torch.zeros(2, dtype=torch.int32), seg_row, seg_off, seg_cnt, seg_list, 2, 3))
    assert torch.equal(empty.expanded()[0], ids)


def test_weighted_loss_follows_keras_sample_weight_semantics():
    from deeptables_amd import losses
    g = torch.Generator().manual_seed(0)
    z = torch.randn(17, 1, generator=g, dtype=torch.float64)
    y = (torch.rand(17, 1, generator=g) < 0.4).double()
    w = torch.rand(17, generator=g, dtype=torch.float64) * 3
    p = torch.sigmoid(z)
    per = -(y * torch.log(p) + (1 - y) * torch.log(1 - p)).reshape(-1)
    assert abs(float(losses.named_loss('binary_crossentropy', z, y, w)) - float((per * w).sum() / 17)) < 1e-12
    # all-ones weights = the unweighted mean
    assert abs(float(losses.named_loss('binary_crossentropy', z, y, torch.ones(17, dtype=torch.float64))) -
               float(losses.named_loss('binary_crossentropy', z, y))) < 1e-12
    zc = torch.randn(9, 4, generator=g, dtype=torch.float64)
    yc = torch.eye(4, dtype=torch.float64)[torch.randint(0, 4, (9,), generator=g)]
    wc = torch.rand(9, generator=g, dtype=torch.float64)
    per_c = -(torch.log_softmax(zc, -1) * yc).sum(-1)
    assert abs(float(losses.named_loss('categorical_crossentropy', zc, yc, wc)) - float((per_c * wc).sum() / 9)) < 1e-12
    yr = torch.randn(17, 1, generator=g, dtype=torch.float64)
    assert abs(float(losses.named_loss('mse', z, yr, w)) - float((((z - yr) ** 2).reshape(-1) * w).sum() / 17)) < 1e-12


def test_feed_carries_row_weights_through_the_shuffle():
    from deeptables_amd import training
    from deeptables_amd.models.metainfo import CategoricalColumn, ContinuousColumn
    n = 50
    X = {'cat': np.arange(n * 2).reshape(n, 2) % 7, 'input_continuous_all': np.arange(n, dtype=np.float32).reshape(n, 1)}

    class XF:
        def __init__(self, d):
            self.d = d

        def __len__(self):
            return n

        def __getitem__(self, k):
            return self.d[k]
    y = (np.arange(n) % 3 == 0).astype(np.float32)
    w = np.arange(n, dtype=np.float32) + 0.5                        # weight i+0.5 belongs to the row whose dense value is i
    cats = [CategoricalColumn('C0', 7, 4), CategoricalColumn('C1', 7, 4)]
    conts = [ContinuousColumn('input_continuous_all', ['I0'])]
    tb = training.TableBatches(XF(X), y, cats, conts, 'cpu', 'binary', 2, sample_weight=w)
    assert tb.weighted
    seen = 0
    for ins, yb in tb.iterate(16, True, drop_remainder=False):
        dense = ins[-1].reshape(-1)
        assert yb.shape[1] == 2
        assert torch.allclose(yb[:, -1], dense + 0.5)               # the weight travelled with its row
        assert torch.allclose(yb[:, 0], (dense.long() % 3 == 0).float())
        seen += len(dense)
    assert seen == n
    assert not training.TableBatches(XF(X), y, cats, conts, 'cpu', 'binary', 2).weighted


def test_balanced_class_weights():
    from deeptables_amd.models.deeptable import DeepTable

    class Stub:
        classes_ = [0, 1, 2]
    y = np.array([0] * 6 + [1] * 3 + [2] * 1)
    cw = DeepTable.get_class_weight(Stub(), y)
    assert cw == {0: 10 / (3 * 6), 1: 10 / (3 * 3), 2: 10 / (3 * 1)}      # sklearn 'balanced': n / (classes * count)


def _cpu_model(nets, hidden, task='binary', **extra):
    from deeptables_amd.models import ModelConfig, DeepModel
    from deeptables_amd.models.metainfo import CategoricalColumn, ContinuousColumn
    conf = ModelConfig(nets=nets, fixed_embedding_dim=True, embeddings_output_dim=8,
                       dnn_params={'hidden_units': hidden, 'activation': 'relu'}, **{'embedding_dropout': 0, **extra})
    dm = DeepModel(task, 2, conf, [CategoricalColumn(f'C{i}', 20 + i, 8) for i in range(6)],
                   [ContinuousColumn('input_continuous_all', ['a', 'b', 'c'])])
    dm.build('cpu')
    return dm


def test_fused_plan_eligibility_by_tower_shape():
    """which dnn_params the whole-step plans take (fused._tower_widths): two relu cells without dropout / batch norm whose
    widths fit the compiled 128 x 64 tile; everything else falls back to the per-layer kernels (plan None).  Host logic
    only: the plan is constructed on CPU, nothing is launched."""
    from deeptables_amd.fused import FusedDCN, FusedDeepFM, _tower_widths
    assert _tower_widths({'hidden_units': ((128, 0, False), (64, 0, False)), 'activation': 'relu'}) == (128, 64)
    assert _tower_widths({'hidden_units': [[100, 0, False], [40, 0, False]]}) == (100, 40)
    for bad in ({'hidden_units': ((129, 0, False), (64, 0, False))}, {'hidden_units': ((128, 0, False), (65, 0, False))},
                {'hidden_units': ((64, 0, True), (32, 0, False))}, {'hidden_units': ((64, 0.2, False), (32, 0, False))},
                {'hidden_units': ((64, 0, False),)}, {'hidden_units': ((64, 0, False), (32, 0, False), (16, 0, False))},
                {'hidden_units': ((64, 0, False), (32, 0, False)), 'activation': 'tanh'},
                {'hidden_units': ((64, 0, False), (32, 0, False)), 'custom_dnn_fn': lambda x, p, c: x}, {'hidden_units': ()}):
        assert _tower_widths(bad) is None, bad
    assert isinstance(_cpu_model(['linear', 'fm_nets', 'dnn_nets'], ((100, 0, False), (40, 0, False))).fused_plan(), FusedDeepFM)
    assert isinstance(_cpu_model(['dcn_nets'], ((32, 0, False), (64, 0, False)), cross_params={'num_cross_layer': 3}).fused_plan(),
                      FusedDCN)
    assert _cpu_model(['linear', 'fm_nets', 'dnn_nets'], ((256, 0, False), (64, 0, False))).fused_plan() is None
    assert _cpu_model(['linear', 'fm_nets', 'dnn_nets'], ((64, 0, False), (1, 0, False))).fused_plan() is None    # no dense_logit layer
    assert _cpu_model(['linear', 'dnn_nets'], ((128, 0, False), (64, 0, False))).fused_plan() is None             # not DeepFM
    assert _cpu_model(['linear', 'fm_nets', 'dnn_nets'], ((128, 0, False), (64, 0, False)), stacking_op='concat').fused_plan() is None


def test_narrow_tower_parameters_are_views_of_zero_padded_slabs():
    """the plan moves W1 / b1 / W2 / b2 / w3 into [C,128] / [128] / [128,64] / [64] / [64] slabs of its flat parameter
    buffer: values kept, pads zero, the gradient views and the Adam moments laid out the same way"""
    dm = _cpu_model(['linear', 'fm_nets', 'dnn_nets'], ((100, 0, False), (40, 0, False)))
    L = dm.model.layers_by_name
    before = {n: p.detach().clone() for n, p in dm.model.named_parameters()}
    plan = dm.fused_plan()
    for n, p in dm.model.named_parameters():
        assert torch.equal(p.detach(), before[n]), n                      # moving the storage keeps every value
    C = 6 * 8 + 3
    d1, d2, dl = L['dnn_dense_1'], L['dnn_dense_2'], L['dense_logit_dnn_nets']
    assert tuple(d1.kernel.shape) == (C, 100) and d1.kernel.stride() == (128, 1)
    assert tuple(d2.kernel.shape) == (100, 40) and d2.kernel.stride() == (64, 1)
    o, flat = plan.off, plan.flat_params
    lo, hi = flat.data_ptr(), flat.data_ptr() + flat.numel() * 4
    for p, g in plan.grad_views:
        assert lo <= p.data_ptr() < hi and tuple(p.shape) == tuple(g.shape) and p.stride() == g.stride()
        assert (p.data_ptr() - lo) == (g.data_ptr() - plan.accum.data_ptr())          # same offset in both buffers
        st = dm.optimizer.state[id(p)]
        assert tuple(st['m'].shape) == tuple(p.shape) and st['m'].stride() == p.stride()
    W1 = flat[o['dW1']:o['dW1'] + C * 128].view(C, 128)
    W2 = flat[o['dW2']:o['dW2'] + 128 * 64].view(128, 64)
    assert torch.equal(W1[:, :100], d1.kernel.detach()) and W1[:, 100:].abs().sum() == 0
    assert torch.equal(W2[:100, :40], d2.kernel.detach()) and W2[100:].abs().sum() == 0 and W2[:, 40:].abs().sum() == 0
    assert flat[o['db1'] + 100:o['db1'] + 128].abs().sum() == 0 and flat[o['db2'] + 40:o['db2'] + 64].abs().sum() == 0
    assert torch.equal(flat[o['dw3']:o['dw3'] + 40], dl.kernel.detach().reshape(-1)) and flat[o['dw3'] + 40:o['dw3'] + 64].abs().sum() == 0
    with torch.no_grad():                         # writes through the parameter land in the slab (the kernels read the slab)
        d1.kernel[3, 7] = 42.0
    assert W1[3, 7].item() == 42.0


def test_segmented_sparse_grad_expands_for_random_segment_layouts():
    """property: whatever way duplicated rows are split into (region, segment) records — regions of different fill, segments
    in any order inside a region, members in any order inside a segment — `expanded()` restores the row id of every lookup"""
    from hypothesis import given, settings, strategies as st
    from deeptables_amd.ops import SparseRowGrad

    @settings(max_examples=60, deadline=None)
    @given(st.integers(1, 40), st.integers(1, 4), st.integers(1, 6), st.integers(0, 2 ** 31 - 1))
    def check(n, regions, cap, seed):
        rng = np.random.RandomState(seed)
        rows = rng.randint(0, max(2, n // 2), size=n).astype(np.int64)          # many duplicates
        rows[rng.rand(n) < 0.1] = -1                                            # out-of-range lookups stay -1
        reported = rows.copy()
        nseg = np.zeros(regions, np.int32)
        seg_row = np.zeros(regions * cap, np.int64)
        seg_off = np.zeros(regions * cap, np.int32)
        seg_cnt = np.zeros(regions * cap, np.int32)
        seg_list = np.zeros((regions, n), np.int32)
        fill = np.zeros(regions, np.int64)
        for r in rng.permutation(np.unique(rows[rows >= 0])):
            members = np.flatnonzero(rows == r)
            if len(members) < 2:
                continue
            reg = int(rng.randint(regions))
            if nseg[reg] == cap:                                                # region full: the row stays per-lookup
                continue                                                        # (the kernels size cap so this cannot happen)
            k = reg * cap + nseg[reg]
            seg_row[k], seg_off[k], seg_cnt[k] = r, reg * n + fill[reg], len(members)
            seg_list[reg, fill[reg]:fill[reg] + len(members)] = rng.permutation(members)
            fill[reg] += len(members)
            nseg[reg] += 1
            reported[members] = -1
        T = torch.as_tensor
        sg = SparseRowGrad(T(reported), torch.zeros(n, 2), fields=-1,
                           segments=(T(nseg), T(seg_row), T(seg_off), T(seg_cnt), T(seg_list.reshape(-1)), regions, cap))
        got, _ = sg.expanded()
        assert np.array_equal(got.numpy(), rows)
        assert np.array_equal(sg.rows.numpy(), reported)                       # the stored gradient is not modified
    check()


def _run_bench(extra_args, env_extra, timeout=300):
    import subprocess
    import sys as _sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    env.update(env_extra)
    return subprocess.run([_sys.executable, os.path.join(root, 'bench.py')] + extra_args, env=env, capture_output=True,
                          text=True, timeout=timeout)


def test_bench_gpus_flag_spawns_that_many_ranks():
    """`python bench.py --gpus 2` without a launcher must run TWO ranks (re-exec under torch.distributed.run),
    not one rank labelled 2 (reference shape: deeptables/tests/models/run_dt.py:35-44).  The probe mode joins a gloo group
    and leaves before any device is touched, so this runs on CPU."""
    import json
    r = _run_bench(['--gpus', '2', '--steps', '2', '--warmup', '0'], {'DT_BENCH_SPAWN_PROBE': '1'})
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert lines, r.stdout + r.stderr
    assert json.loads(lines[-1]) == {'spawned_ranks': 2, 'world_size': 2}


def test_bench_gpus_flag_must_match_the_launcher():
    """inside a launcher (WORLD_SIZE set) a different --gpus is an error, not a mislabelled line"""
    r = _run_bench(['--gpus', '4'], {'DT_BENCH_SPAWN_PROBE': '1', 'WORLD_SIZE': '2', 'RANK': '0'}, timeout=120)
    assert r.returncode != 0
    assert 'WORLD_SIZE=2' in (r.stderr + r.stdout)


def test_bench_plain_run_has_no_leg_but_the_headline_and_full_has_them_all():
    """bench.select_legs: without --full the parity, extras and CPU-baseline legs are off and no region is repeated, whatever
    --no-* options came along; --full runs them all with five repeats, less what a --no-* option drops; an explicit --repeats
    holds in both."""
    import argparse
    import bench

    def legs(**kw):
        a = dict(full=False, repeats=None, no_parity=False, no_extras=False, no_cpu_baseline=False)
        a.update(kw)
        r = bench.select_legs(argparse.Namespace(**a))
        return (not r.no_parity, not r.no_extras, not r.no_cpu_baseline, r.repeats)
    assert legs() == (False, False, False, 0)
    assert legs(no_parity=True) == (False, False, False, 0)
    assert legs(repeats=3) == (False, False, False, 3)
    assert legs(full=True) == (True, True, True, 5)
    assert legs(full=True, no_cpu_baseline=True) == (True, True, False, 5)
    assert legs(full=True, no_parity=True, no_extras=True, repeats=0) == (False, False, True, 0)


def test_model_peephole_defers_the_interacting_layers_normalisation_only_for_consumers_that_take_it():
    """functional.Model.__init__: an AutoInt interacting layer hands over its output with the BatchNormalization pending when
    that output has ONE consumer which applies it on load — the next interacting layer, or Flatten -> linear Dense(1)
    (deepnets.py:219-224, deepmodel.py:131-143) — and never otherwise (a second consumer, a model output, a wider Dense)."""
    import torch
    from deeptables_amd import functional as K
    from deeptables_amd.models import layers

    def stack(tail):
        inp = K.Input(shape=(6, 32), name='x')
        a = layers.MultiheadAttention(params={'num_heads': 4}, name='att_a')(inp)
        b = layers.MultiheadAttention(params={'num_heads': 4}, name='att_b')(a)
        return inp, a, b, tail(a, b)

    def deferred(model):
        return sorted(n.layer.name for n in model.nodes if id(n) in model._defer_norm)

    inp, a, b, out = stack(lambda a, b: K.Dense(1, name='out')(K.Flatten(name='fl')(b)))
    assert deferred(K.Model(inputs=[inp], outputs=out)) == ['att_a', 'att_b']
    inp, a, b, out = stack(lambda a, b: K.Dense(1, activation='relu', name='out')(K.Flatten(name='fl')(b)))
    assert deferred(K.Model(inputs=[inp], outputs=out)) == ['att_a']                       # a relu unit is not the linear head
    inp, a, b, out = stack(lambda a, b: K.Dense(3, name='out')(K.Flatten(name='fl')(b)))
    assert deferred(K.Model(inputs=[inp], outputs=out)) == ['att_a']                       # neither is a wider Dense
    inp, a, b, out = stack(lambda a, b: K.Add(name='add')([K.Dense(1, name='o1')(K.Flatten(name='f1')(b)),
                                                          K.Dense(1, name='o2')(K.Flatten(name='f2')(a))]))
    assert deferred(K.Model(inputs=[inp], outputs=out)) == ['att_b']                       # att_a's output has two consumers
    inp, a, b, out = stack(lambda a, b: b)
    assert deferred(K.Model(inputs=[inp], outputs=out)) == ['att_a']                       # a model output stays normalised


_STEP_ENTRIES = ('dt_deepfm_train_step', 'dt_deepfm_train_step_adam', 'dt_dcn_train_step', 'dt_dcn_train_step_adam',
                 'dt_deepfm_preelect', 'dt_embedding_bwd_dense')


class _StepRecorder:
    """stand-in for fused.lib(): the step's launches are recorded as (name, args) and return 0; every host-side query goes
    to the real library (dt_deepfm_step_chains is recorded as well, and answered by the library)"""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        if name in _STEP_ENTRIES:
            return lambda *args: self.calls.append((name, args)) or 0
        fn = getattr(self.real, name)
        if name == 'dt_deepfm_step_chains':
            return lambda *args: self.calls.append((name, args)) or fn(*args)
        return fn


def _tensor_names(plan, dm, inputs):
    """data_ptr -> 'name' ('a|b' when several named tensors start at the same address)"""
    import ctypes  # noqa: F401
    L = dm.model.layers_by_name
    emb, opt = plan.emb, dm.optimizer
    table = emb.tables[plan.key]
    named = dict(inputs)
    named.update({'table': table, 'row_offset': getattr(emb, f'row_offset_{plan.key}'),
                  'vocab': getattr(emb, f'vocab_{plan.key}'), 'oob': emb.oob_count,
                  'gamma': plan.bn.gamma, 'beta': plan.bn.beta, 'mean': plan.bn.moving_mean,
                  'var': plan.bn.moving_variance, 'W1': plan.d1.kernel, 'b1': plan.d1.bias, 'W2': plan.d2.kernel,
                  'b2': plan.d2.bias, 'out.kernel': L['task_output'].kernel, 'out.bias': L['task_output'].bias,
                  'accum': plan.accum, 'flat_params': plan.flat_params, 'drop_seed': plan.drop_seed})
    if 'linear_logit' in L:
        named.update({'w_lin': L['linear_logit'].kernel, 'dense_logit.kernel': L['dense_logit_dnn_nets'].kernel})
    else:
        named.update({'cross.kernel': L['dcn_cross_layer'].kernel_stack, 'cross.bias': L['dcn_cross_layer'].bias_stack,
                      'one': plan.one})
    if table.grad is not None:
        named['table.grad'] = table.grad
    if id(table) in opt.state:
        named.update({'adam.m': opt.state[id(table)]['m'], 'adam.v': opt.state[id(table)]['v']})
    if opt._dev_state is not None:
        named['adam.state'] = opt._dev_state
    if opt._flat is not None:
        named.update({'flat.m': opt._flat[2], 'flat.v': opt._flat[3]})
    for key, buf in plan._bufs.items():
        for k, v in buf.items():
            if isinstance(v, torch.Tensor):
                named[k if isinstance(key, int) else f'sharded.{k}'] = v
        for s, sb in buf.get('slots', {}).items():
            for k, v in sb.items():
                if isinstance(v, torch.Tensor):
                    named[f'slot{s}.{k}'] = v
    by_ptr = {}
    for n, t in named.items():
        by_ptr.setdefault(t.data_ptr(), []).append(n)
    return {p: '|'.join(sorted(ns)) for p, ns in by_ptr.items()}


def _decoded(rec, plan, dm, inputs):
    """the recorded calls with every pointer argument replaced by the name of the tensor it points to"""
    import ctypes
    names = _tensor_names(plan, dm, inputs)
    out = []
    for name, args in rec.calls:
        dec = []
        for a in args:
            if isinstance(a, ctypes.c_void_p):
                assert a.value in names, (name, len(dec), a.value)
                a = names[a.value]
            dec.append(a)
        out.append((name, dec))
    rec.calls.clear()
    return out


def test_fused_plans_hand_the_step_entry_points_the_same_arguments(monkeypatch):
    """pins what FusedDeepFM / FusedDCN hand the library in every step mode: the entry point, the argument count, the
    `phases` word, the scalars and which tensor every pointer points to.  The launches are recorded (not run), so the
    plans run on CPU tensors; the sharded split (sharded_core) runs with a one-rank stand-in for the strategy."""
    import pytest
    from deeptables_amd import _lib, fused
    from deeptables_amd.models import layers
    rec = _StepRecorder(_lib.lib())
    monkeypatch.setattr(fused, 'lib', lambda: rec)
    monkeypatch.setattr(fused, 'stream_ptr', lambda: None)
    X3, BF16, MSE = _lib.DT_STEP_TOWER_X3, _lib.DT_STEP_TOWER_BF16, _lib.DT_STEP_LOSS_MSE
    PRE, PREP, STAMPS = _lib.DT_STEP_PREELECTED, _lib.DT_STEP_PREPARED, _lib.DT_STEP_STAMPS
    B, F, D, Nd = 16, 6, 8, 3
    slots_n = _lib.lib().dt_deepfm_dedupe_slots(B, F)
    DEEPFM = ['linear', 'fm_nets', 'dnn_nets']
    DCN = ['dcn_nets']

    def make(nets, task='binary', env=None, **extra):
        for k in ('DT_AMD_FUSED_DEDUPE', 'DT_AMD_TOWER_DTYPE', 'DT_AMD_STEP_STAMPS'):      # read when the plan is built
            monkeypatch.delenv(k, raising=False)
        for k, v in (env or {}).items():
            monkeypatch.setenv(k, v)
        extra = dict(extra)
        if nets == DCN:
            extra.setdefault('cross_params', {'num_cross_layer': 2})
        dm = _cpu_model(nets, ((100, 0, False), (40, 0, False)), task=task, **extra)
        dm.optimizer._dev_state = torch.zeros(68, dtype=torch.int32)     # _state_tensor launches nothing
        plan = dm.fused_plan()
        assert type(plan).__name__ == ('FusedDeepFM' if nets == DEEPFM else 'FusedDCN')
        for k in (env or {}):
            monkeypatch.delenv(k)
        return dm, plan

    g = torch.Generator().manual_seed(0)
    idx = torch.randint(0, 20, (B, F), generator=g, dtype=torch.int32)
    idx2 = torch.randint(0, 20, (B, F), generator=g, dtype=torch.int32)
    dense = torch.randn(B, Nd, generator=g)
    y = (torch.rand(B, 1, generator=g) < 0.5).float()
    sw = torch.rand(B, generator=g)
    logit_out = torch.empty(B, 1)
    idx_f = idx.float()
    inputs = {'idx': idx, 'idx_f': idx_f, 'idx2': idx2, 'dense': dense, 'y': y, 'sw': sw, 'logit_out': logit_out}

    def head(dm, net, ids='idx', rows='rows', dedupe='dedupe', training=True, logit='logit', oob=None,
             kind=_lib.DT_IDX_I32):
        bn = dm.model.layers_by_name['bn_concat_emb_dense']
        common = [ids, kind, 'table', 'row_offset', 'vocab', 'dense', 'y', B, F, D, Nd]
        mid = ['gamma', 'beta', 'mean' if training else None, 'var' if training else None, float(bn.epsilon),
               float(bn.momentum), 'W1|flat_params', 'b1', 'W2', 'b2']
        tail = [logit, rows, 'grad_rows', 'accum', 'ws', oob, dedupe, slots_n]
        if net == DEEPFM:
            return common + ['w_lin'] + mid + ['dense_logit.kernel', 'out.kernel', 'out.bias'] + tail
        return common + ['cross.kernel', 'cross.bias', 2] + mid + ['out.kernel', 'one', 'out.bias'] + tail

    def plain_tail(net, phases, emb_drop=0.0, dense_drop=0.0, w=None):
        return ([1.0, 0] if net == DEEPFM else []) + [phases, emb_drop, 'drop_seed', dense_drop, w, None]

    def adam_tail(dm, plan, phases, whole=True, nxt=(None, None, None), w=None):
        opt = dm.optimizer
        dn = ['W1|flat_params', 'flat.m', 'flat.v', opt._flat[4], float(opt.lr)] if whole else [None, None, None, 0, 0.0]
        return [phases, 0.0, 'drop_seed', 0.0, w, 'adam.m', 'adam.v', 2 * D, 'adam.state', 0.0, opt.b1, opt.b2, opt.eps,
                *dn, *nxt, None]

    def entry(net, adam=False):
        return ('dt_deepfm' if net == DEEPFM else 'dt_dcn') + ('_train_step_adam' if adam else '_train_step')

    def one_call(dm, plan, **kw):
        loss, logit = plan.run(kw.pop('ids', idx), dense, y, **kw)
        calls = _decoded(rec, plan, dm, inputs)
        assert len(calls) == 1, [c[0] for c in calls]
        return calls[0], logit

    def check_call(got, name, want):
        assert got[0] == name
        assert len(got[1]) == len(want), (name, len(got[1]), len(want))
        for i, (a, b) in enumerate(zip(got[1], want)):
            if isinstance(b, float):
                assert a == pytest.approx(b), (name, i, a, b)
            else:
                assert a == b, (name, i, a, b)

    for net in (DEEPFM, DCN):
        # -- dense-gradient tables (the small tables' default): no dedupe, the row gradients densified ---------------
        dm, plan = make(net)
        assert plan.emb.uses_dense_grad(D)
        plan.run(idx, dense, y)
        calls = _decoded(rec, plan, dm, inputs)
        assert [c[0] for c in calls] == [entry(net), 'dt_embedding_bwd_dense']
        check_call(calls[0], entry(net), head(dm, net, dedupe=None) + plain_tail(net, 2 | X3))
        check_call(calls[1], 'dt_embedding_bwd_dense', ['rows', 'grad_rows', B * F, D, 'table.grad', None])
        assert plan.key not in plan.emb.sparse_grads

        monkeypatch.setattr(layers, 'DENSE_GRAD_MAX_ELEMS', 0)          # row-sparse tables: the dedupe paths
        dm, plan = make(net)
        # forward only: no tower / diagnostic bits, no dedupe
        got, logit = one_call(dm, plan, backward=False)
        check_call(got, entry(net), head(dm, net, dedupe=None) + plain_tail(net, 1))
        assert logit is plan._bufs[B]['logit']
        # backward without the optimizer
        got, _ = one_call(dm, plan)
        check_call(got, entry(net), head(dm, net) + plain_tail(net, 2 | X3))
        sg = plan.emb.sparse_grads[plan.key][0]
        assert sg.fields == -1 and sg.segments is not None and sg.rows.data_ptr() == plan._bufs[B]['rows'].data_ptr()
        for p, gv in plan.grad_views:
            assert p.grad is gv
        # the whole optimizer step inside the step
        got, _ = one_call(dm, plan, apply_rows=True)
        check_call(got, entry(net, True), head(dm, net) + adam_tail(dm, plan, 2 | X3))
        assert plan.emb.sparse_grads[plan.key][0].fields == -2 and dm.optimizer._applied_in_step
        dm.optimizer._applied_in_step = False
        monkeypatch.setenv('DT_AMD_STEP_IN_STEP', '0')
        got, _ = one_call(dm, plan, apply_rows=True)
        check_call(got, entry(net, True), head(dm, net) + adam_tail(dm, plan, 2 | X3, whole=False))
        assert not dm.optimizer._applied_in_step
        monkeypatch.delenv('DT_AMD_STEP_IN_STEP')
        monkeypatch.setenv('DT_AMD_ROWS_IN_STEP', '0')
        got, _ = one_call(dm, plan, apply_rows=True)
        check_call(got, entry(net), head(dm, net) + plain_tail(net, 2 | X3))
        assert plan.emb.sparse_grads[plan.key][0].fields == -1
        monkeypatch.delenv('DT_AMD_ROWS_IN_STEP')
        # sample weights, float ids, a caller-owned logit buffer, an out-of-range counter
        plan.emb.check_oob = True
        got, logit = one_call(dm, plan, ids=idx_f, sample_weight=sw, logit_out=logit_out)
        check_call(got, entry(net), head(dm, net, ids='idx_f', logit='logit_out', oob='oob', kind=_lib.DT_IDX_F32) +
                   plain_tail(net, 2 | X3, w='sw'))
        assert logit is logit_out
        plan.emb.check_oob = False
        with pytest.raises(ValueError, match='logit_out must be a contiguous float32'):
            plan.run(idx, dense, y, logit_out=torch.empty(B, 2))
        # pre-elected steps: the ids-only half ran ahead into slot 1's buffers
        plan.preelect(idx, 1)
        check_call(_decoded(rec, plan, dm, inputs)[0], 'dt_deepfm_preelect',
                   ['idx', _lib.DT_IDX_I32, 'row_offset', 'vocab', B, F, 'slot1.rows', 'slot1.dedupe', slots_n, None])
        got, _ = one_call(dm, plan, apply_rows=True, slot=1, preelected=True)
        check_call(got, entry(net, True), head(dm, net, rows='slot1.rows', dedupe='slot1.dedupe') +
                   adam_tail(dm, plan, 2 | X3 | PRE))
        assert plan.emb.sparse_grads[plan.key][0].rows.data_ptr() == plan._bufs[B]['slots'][1]['rows'].data_ptr()
        got, _ = one_call(dm, plan, slot=1, preelected=True)
        check_call(got, entry(net), head(dm, net, rows='slot1.rows', dedupe='slot1.dedupe') + plain_tail(net, 2 | X3 | PRE))
        with pytest.raises(_lib.DtHipError, match='a pre-elected step needs the in-step dedupe'):
            plan.run(idx, dense, y, backward=False, slot=1, preelected=True)
        # chained steps: this step prepares the next one (slot 2) and was prepared by the one before it (slot 1)
        assert plan.can_chain(B)
        got = _decoded(rec, plan, dm, inputs)
        check_call(got[0], 'dt_deepfm_step_chains', [B, F, D, Nd, 2 | X3])
        got, _ = one_call(dm, plan, apply_rows=True, slot=1, next_ids=(idx2, 2), prepared=True)
        check_call(got, entry(net, True), head(dm, net, rows='slot1.rows', dedupe='slot1.dedupe') +
                   adam_tail(dm, plan, 2 | X3 | PREP, nxt=('idx2', 'slot2.rows', 'slot2.dedupe')))
        got, _ = one_call(dm, plan, apply_rows=True, next_ids=(idx2, 2))
        check_call(got, entry(net, True), head(dm, net) +
                   adam_tail(dm, plan, 2 | X3, nxt=('idx2', 'slot2.rows', 'slot2.dedupe')))
        with pytest.raises(_lib.DtHipError, match=r'chained steps need the in-step dedupe and optimizer \(can_chain\)'):
            plan.run(idx, dense, y, slot=1, prepared=True)
        with pytest.raises(_lib.DtHipError, match=r'chained steps need the in-step dedupe and optimizer \(can_chain\)'):
            plan.run(idx, dense, y, next_ids=(idx2, 2))
        for bad in ((idx2, 1), (idx2, 0), (idx2.float(), 2), (idx2[:8], 2), (idx2.t(), 2)):
            with pytest.raises(ValueError, match="next_ids: \\(contiguous ids like this step's, a slot of their own\\)"):
                plan.run(idx, dense, y, apply_rows=True, slot=1, next_ids=bad)
        assert not rec.calls
        # evaluation mode: no running statistics, no dropout
        dm.model.eval()
        got, _ = one_call(dm, plan, backward=False)
        check_call(got, entry(net), head(dm, net, dedupe=None, training=False) + plain_tail(net, 1))
        dm.model.train()

        # DT_AMD_FUSED_DEDUPE=0: no dedupe, so no in-step optimizer and no pre-election
        dm, plan = make(net, env={'DT_AMD_FUSED_DEDUPE': '0'})
        got, _ = one_call(dm, plan, apply_rows=True)
        check_call(got, entry(net), head(dm, net, dedupe=None) + plain_tail(net, 2 | X3))
        assert plan.emb.sparse_grads[plan.key][0].fields is None
        assert not plan.can_chain(B)
        with pytest.raises(_lib.DtHipError, match='a pre-elected step needs the in-step dedupe'):
            plan.run(idx, dense, y, slot=1, preelected=True)
        # the tower's matrix-core mode and the phase stamps
        for mode, bit in (('f32', 0), ('bf16x3', X3), ('bf16', BF16)):
            dm, plan = make(net, env={'DT_AMD_TOWER_DTYPE': mode, 'DT_AMD_STEP_STAMPS': '1'})
            got, _ = one_call(dm, plan)
            check_call(got, entry(net), head(dm, net) + plain_tail(net, 2 | bit | STAMPS))
            got, _ = one_call(dm, plan, apply_rows=True)
            check_call(got, entry(net, True), head(dm, net) + adam_tail(dm, plan, 2 | bit | STAMPS))
            got, _ = one_call(dm, plan, backward=False)
            check_call(got, entry(net), head(dm, net, dedupe=None) + plain_tail(net, 1))
            plan.can_chain(B)
            check_call(_decoded(rec, plan, dm, inputs)[0], 'dt_deepfm_step_chains', [B, F, D, Nd, 2 | bit])
        # dropouts
        dm, plan = make(net, embedding_dropout=0.25, dense_dropout=0.5)
        got, _ = one_call(dm, plan, sample_weight=sw)
        check_call(got, entry(net), head(dm, net) + plain_tail(net, 2 | X3, 0.25, 0.5, w='sw'))
        dm.model.eval()
        got, _ = one_call(dm, plan, backward=False)
        check_call(got, entry(net), head(dm, net, dedupe=None, training=False) + plain_tail(net, 1))
        # regression: the mse loss bit
        dm, plan = make(net, task='regression')
        got, _ = one_call(dm, plan, backward=False)
        check_call(got, entry(net), head(dm, net, dedupe=None) + plain_tail(net, 1 | MSE))
        got, _ = one_call(dm, plan, apply_rows=True)
        check_call(got, entry(net, True), head(dm, net) + adam_tail(dm, plan, 2 | MSE | X3))
        monkeypatch.setattr(layers, 'DENSE_GRAD_MAX_ELEMS', 1 << 22)

    # the sharded split (DeepFM only): the step's kernels on the received rows, one rank
    class OneRank:
        world_size, rank = 1, 0

        @staticmethod
        def field_bounds(F):
            return [(0, F)]
    monkeypatch.setattr(layers, 'DENSE_GRAD_MAX_ELEMS', 0)
    dm, plan = make(DEEPFM, env={'DT_AMD_STEP_STAMPS': '1'})
    bn = plan.bn
    for part, phases in ((0, 2 | X3 | STAMPS), (_lib.DT_STEP_SKIP_FINISH, 2 | _lib.DT_STEP_SKIP_FINISH | X3 | STAMPS),
                         (_lib.DT_STEP_FINISH_ONLY, 2 | _lib.DT_STEP_FINISH_ONLY)):
        plan.sharded_core(B, dense, y, OneRank, sample_weight=sw, part=part)
        got = _decoded(rec, plan, dm, inputs)
        assert len(got) == 1
        check_call(got[0], 'dt_deepfm_train_step',
                   ['sharded.iota', _lib.DT_IDX_I32, 'sharded.emb_T', 'sharded.zero_off', 'sharded.fb_vocab', 'dense', 'y',
                    B, F, D, Nd, 'w_lin', 'gamma', 'beta', 'mean', 'var', float(bn.epsilon), float(bn.momentum),
                    'W1|flat_params', 'b1', 'W2', 'b2', 'dense_logit.kernel', 'out.kernel', 'out.bias', 'logit',
                    'sharded.rows_dummy', 'grad_rows', 'accum', 'ws', None, None, 0, 1.0, 1, phases, 0.0, 'drop_seed', 0.0,
                    'sw', None])
        assert dm.model._dt_sharded_step
