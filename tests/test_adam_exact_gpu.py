# -*- coding:utf-8 -*-
"""GPU: training.KerasAdam(exact_rows=True) — csrc/adam_exact.hip (dt_adam_rows_catchup, dt_adam_rows_materialize,
dt_adam_rows_stamp) against keras.optimizers.Adam applied to the densified gradient, restated in float64
(tests/adam_exact_reference.py), at the kernel level and through DeepModel.  Four lookups per field per step everywhere.

The bar comes from existing code: the library's own dense kernel (dt_adam_dense_step) runs the same 340 steps on a copy of the
table with the densified gradients, and its largest absolute distance from the oracle is d0 — one per quantity (weights, m, v).
The exact mode may be 4 d0 off: both paths share the per-step roundings; a gap adds one running-power chain and one powf per
slot, a few roundings per gap and not per step.  Measured on an MI355X (the tests print every figure; exact rows / d0):
    D = 16: weights 1.733e-7 / 1.733e-7, m 2.392e-7 / 2.541e-7, v 1.478e-5 / 1.478e-5 (the largest errors sit on the filler
            rows both paths update every few steps); row B at the forward of step 340: 7.4e-8
    D = 1:  weights 9.786e-8 / 9.786e-8, m 2.415e-7 / 2.415e-7, v 1.369e-5 / 1.369e-5; row B: 1.6e-8
    lazy rows A and B end 3.8e-3 .. 6.9e-3 from Keras' dense result: 7,000 to 17,500 bars
    an extra sweep after step 13 moves the final weights by 1.5e-8 and no slot at all
    model, 12 steps: exact rows 6.8e-7 from the dense-gradient path, lazy rows 5.7e-3; captured against eager and resumed
    against uninterrupted: 0.0
Duplicate lookups are summed with float atomics in an order that changes from run to run; the scripted gradients sit on a 2^-6
grid, |g| <= 4, so every such sum is exact in float32 (tests/test_optimizers2_gpu.py)."""
import numpy as np
import pandas as pd
import pytest
import torch

from tests import adam_exact_reference as R

pytestmark = pytest.mark.gpu

STEPS, B = 340, 4
VOCABS, OFFS, V = (5, 9, 300), (0, 5, 14), 314
ROW_A, ROW_B, ROW_C, ROW_D = 14 + 7, 14 + 11, 14 + 299, 5 + 3
A_STEPS, B_STEPS = (1, 2, 4, 13, 340), (1, 340)
MARGIN = 4.0


def _script(D):
    """ids [STEPS, B, 3] int32, packed rows (-1: out of range) and gradients [STEPS, B 3, D] on a 2^-6 grid"""
    ids = np.zeros((STEPS, B, 3), dtype=np.int32)
    for s in range(1, STEPS + 1):
        for b in range(B):
            n = 4 * s + b
            ids[s - 1, b] = (n % 5, n % 9, 20 + (n * 7) % 270)      # filler rows cycle; field 2 stays inside ids 20 .. 289
    for s in A_STEPS:
        ids[s - 1, 3, 2] = 7                    # row A: gaps 0, 1, 8 and 326
    for s in B_STEPS:
        ids[s - 1, 2, 2] = 11                   # row B: the first and the last step only
    ids[4, 0, 1] = ids[4, 1, 1] = 3             # row D twice inside one batch at step 5
    ids[6, 0, 0] = 5                            # one id out of range at step 7 (field 0 has 5 rows)
    assert not (ids[:, :, 2] == 299).any()      # row C is never looked up
    ok = (ids >= 0) & (ids < np.array(VOCABS))
    rows = np.where(ok, ids + np.array(OFFS), -1).astype(np.int64)
    rng = np.random.RandomState(11 + D)
    vals = (rng.randint(-256, 257, size=(STEPS, B * 3, D)) / 64.0).astype(np.float32)
    t0 = (0.05 * rng.randn(V, D)).astype(np.float32)
    return ids, rows, vals, t0


class _Emb:
    """MultiColumnEmbedding as the optimizer and the gather see it (tests/test_optimizers2_gpu.py's fake layer, with the
    buffers of the gather and the `pre_lookup` attribute the optimizer sets)"""

    def __init__(self, table, dev):
        D = table.shape[1]
        self.key = f'd{D}'
        self.tables = {self.key: table}
        self.groups = [(D, [0, 1, 2])]
        self.sparse_grads = {}
        self.pre_lookup = None
        setattr(self, f'row_offset_{self.key}', torch.tensor(OFFS, dtype=torch.int64, device=dev))
        setattr(self, f'vocab_{self.key}', torch.tensor(VOCABS, dtype=torch.int32, device=dev))


def _oracle(rows, vals, t0, lazy=False):
    """float64: Keras' dense step over the whole table (lazy=True: the looked-up rows only, the default mode's semantics)
    -> final (p, m, v) and the weights after step 339"""
    p, m, v = t0.astype(np.float64), np.zeros(t0.shape), np.zeros(t0.shape)
    p339 = None
    for s in range(1, STEPS + 1):
        if s == STEPS:
            p339 = p.copy()
        r = rows[s - 1].reshape(-1)
        if lazy:
            touched = np.unique(r[r >= 0])
            q = (p[touched].copy(), m[touched].copy(), v[touched].copy())
            where = {int(x): i for i, x in enumerate(touched)}
            R.dense_adam_step(*q, np.array([where.get(int(x), -1) for x in r]), vals[s - 1], s)
            p[touched], m[touched], v[touched] = q
        else:
            R.dense_adam_step(p, m, v, r, vals[s - 1], s)
    return p, m, v, p339


def _run(dev, D, script, exact, sweep_at=None):
    """the optimizer driven through the fake layer: catch-up hook, (the gather at the last step), sparse gradient, step()"""
    from deeptables_amd import ops, training
    from deeptables_amd.ops import SparseRowGrad
    ids, rows, vals, t0 = script
    table = torch.nn.Parameter(torch.from_numpy(t0).to(dev))
    emb = _Emb(table, dev)
    opt = training.KerasAdam([table], [emb], exact_rows=exact)
    assert (emb.pre_lookup is not None) == exact
    ids_d, rows_d, vals_d = (torch.from_numpy(a).to(dev) for a in (ids, rows, vals))
    seen_b = None
    for s in range(1, STEPS + 1):
        if emb.pre_lookup is not None:
            emb.pre_lookup(emb.key, ids_d[s - 1])
        if s == STEPS:                          # what the forward of the last step reads, before that step's update runs
            with torch.no_grad():
                out, _ = ops.embedding_lookup(ids_d[s - 1], table, getattr(emb, f'row_offset_{emb.key}'),
                                              getattr(emb, f'vocab_{emb.key}'))
            seen_b = out[2, 2].double().cpu().numpy()
        emb.sparse_grads = {emb.key: [SparseRowGrad(rows_d[s - 1].reshape(-1), vals_d[s - 1].clone())]}
        opt.step()
        if s == sweep_at:
            opt.materialize()
    opt.materialize()
    assert opt.t == STEPS
    st = opt.state[id(table)]
    torch.cuda.synchronize()
    return {'p': table.detach().double().cpu().numpy(), 'm': st['m'].double().cpu().numpy(), 'v': st['v'].double().cpu().numpy(),
            'stamp': st['stamp'].cpu().numpy() if 'stamp' in st else None, 'seen_b': seen_b,
            'p32': table.detach().cpu().numpy()}


def _run_dense(dev, D, script):
    """the library's dense kernel (dt_adam_dense_step through KerasAdam's dense update) on the densified gradients"""
    from deeptables_amd import training
    ids, rows, vals, t0 = script
    table = torch.nn.Parameter(torch.from_numpy(t0).to(dev))
    opt = training.KerasAdam([table])
    rows_d, vals_d = torch.from_numpy(rows).to(dev), torch.from_numpy(vals).to(dev)
    for s in range(1, STEPS + 1):
        r = rows_d[s - 1].reshape(-1)
        g = torch.zeros(V, D, device=dev)
        g.index_add_(0, r.clamp(min=0), vals_d[s - 1] * (r >= 0).float()[:, None])      # (exact sums: the 2^-6 grid)
        table.grad = g
        opt.step()
    st = opt.state[id(table)]
    torch.cuda.synchronize()
    return {'p': table.detach().double().cpu().numpy(), 'm': st['m'].double().cpu().numpy(), 'v': st['v'].double().cpu().numpy()}


_BASELINE = {}


def _baseline(dev, D):
    """(script, float64 oracle, d0 per quantity) of the 340 scripted steps, computed once per D and left unchanged"""
    if D not in _BASELINE:
        script = _script(D)
        ref = dict(zip(('p', 'm', 'v', 'p339'), _oracle(script[1], script[2], script[3])))
        dense = _run_dense(dev, D, script)
        _BASELINE[D] = (script, ref, {k: np.abs(dense[k] - ref[k]).max() for k in ('p', 'm', 'v')})
    return _BASELINE[D]


@pytest.fixture(scope='module', params=[16, 1], ids=['D16', 'D1'])
def case(request, dev):
    """the script, the oracle and every run of it, computed once per D (1: the smallest D the scalar path takes)"""
    from deeptables_amd._lib import lib
    D = request.param
    assert lib().dt_adam_exact_supported(D) == 1 and lib().dt_adam_exact_supported(0) == 0
    script, ref, d0 = _baseline(dev, D)
    return {'D': D, 'script': script, 'ref': ref, 'd0': d0, 'exact': _run(dev, D, script, True),
            'lazy': _run(dev, D, script, False), 'swept': _run(dev, D, script, True, sweep_at=13)}


def test_trajectory_matches_keras_dense_adam(case):
    """1. table, m and v after 340 steps and a final materialize() against the float64 oracle, within 4 d0"""
    got, ref, d0 = case['exact'], case['ref'], case['d0']
    for k in ('p', 'm', 'v'):
        err = np.abs(got[k] - ref[k]).max()
        print(f"D={case['D']} {k}: dense kernel d0 = {d0[k]:.3e}, exact rows {err:.3e} ({err / d0[k]:.2f} d0)")
    for k in ('p', 'm', 'v'):
        assert d0[k] > 0
        assert np.abs(got[k] - ref[k]).max() <= MARGIN * d0[k], k
    # row C was never looked up: its weights are the initial bits, its m and v zero, and the sweep moved its stamp
    assert np.array_equal(got['p32'][ROW_C].view(np.int32), case['script'][3][ROW_C].view(np.int32))
    assert not got['m'][ROW_C].any() and not got['v'][ROW_C].any()
    assert (got['stamp'] == STEPS).all()


def test_forward_sees_current_weights(case):
    """2. the gather of step 340 reads row B (idle since step 1) as Keras holds it after step 339"""
    err = np.abs(case['exact']['seen_b'] - case['ref']['p339'][ROW_B]).max()
    print(f"D={case['D']} row B at the forward of step 340: {err:.3e} (bar {MARGIN * case['d0']['p']:.3e})")
    assert err <= MARGIN * case['d0']['p']


def test_default_is_untouched_and_the_deviation_is_real(case):
    """3. exact_rows=False is the lazy update it was — the looked-up rows only, checked against that semantics in float64 —
    and rows A and B end more than 100 bars away from Keras' dense result"""
    ids, rows, vals, t0 = case['script']
    lazy_ref = dict(zip(('p', 'm', 'v'), _oracle(rows, vals, t0, lazy=True)))
    got, d0 = case['lazy'], case['d0']
    assert got['stamp'] is None
    for k in ('p', 'm', 'v'):
        err = np.abs(got[k] - lazy_ref[k]).max()
        print(f"D={case['D']} lazy {k}: {err:.3e} from the lazy oracle (bar {MARGIN * d0[k]:.3e})")
        assert err <= MARGIN * d0[k], k
    assert np.array_equal(got['p32'][ROW_C].view(np.int32), t0[ROW_C].view(np.int32))
    for name, row in (('A', ROW_A), ('B', ROW_B)):
        dev_ = np.abs(got['p'][row] - case['ref']['p'][row]).max()
        print(f"D={case['D']} lazy row {name}: {dev_:.3e} from Keras' dense result ({dev_ / (MARGIN * d0['p']):.0f} bars)")
        assert dev_ > 100 * MARGIN * d0['p'], name


def test_sweep_is_transparent(case):
    """4. an extra materialize() after step 13 splits gaps in two and changes the final state by no more than the bar"""
    for k in ('p', 'm', 'v'):
        diff = np.abs(case['swept'][k] - case['exact'][k]).max()
        print(f"D={case['D']} extra sweep, {k}: {diff:.3e} (bar {MARGIN * case['d0'][k]:.3e})")
        assert diff <= MARGIN * case['d0'][k], k
    assert (case['swept']['stamp'] == STEPS).all()


# ---- through the model ---------------------------------------------------------------------------------------------------
F, ND, D, VOC = 8, 3, 16, 40
EXACT = {'class_name': 'Adam', 'config': {'exact_rows': True}}


def _frame(n, seed=0):
    rng = np.random.RandomState(seed)
    df = pd.DataFrame({f'C{i}': rng.randint(0, VOC + i, n) for i in range(F)})
    for j in range(ND):
        df[f'I{j}'] = rng.randn(n).astype(np.float32)
    return df, (rng.rand(n) < 0.3).astype(np.float32)


def _model(optimizer='auto', seed=4):
    from deeptables_amd import functional
    from deeptables_amd.models import ModelConfig, DeepModel
    from deeptables_amd.models.metainfo import CategoricalColumn, ContinuousColumn
    functional.set_seed(seed)
    conf = ModelConfig(nets=['dnn_nets'], fixed_embedding_dim=True, embeddings_output_dim=D, embedding_dropout=0,
                       dense_dropout=0, metrics=['AUC'], optimizer=optimizer)
    cats = [CategoricalColumn(f'C{i}', VOC + i, D) for i in range(F)]
    conts = [ContinuousColumn('input_continuous_all', [f'I{j}' for j in range(ND)])]
    dm = DeepModel('binary', 2, conf, cats, conts)
    dm.build()
    return dm


def _fit(dm, df, y, spe=1, epochs=1, shuffle=False):
    torch.manual_seed(123)
    torch.cuda.manual_seed_all(123)
    return dm.fit(df, y, batch_size=B, epochs=epochs, verbose=0, validation_split=0, shuffle=shuffle, steps_per_execution=spe)


def _one_step(dm, df, y, lo, dev):
    """one train step outside fit, on rows lo .. lo + B of the frame"""
    ins = [torch.from_numpy(df[[f'C{i}' for i in range(F)]].values[lo:lo + B].astype(np.int32)).to(dev),
           torch.from_numpy(df[[f'I{j}' for j in range(ND)]].values[lo:lo + B].astype(np.float32)).to(dev)]
    dm.model.train()
    dm.train_step(ins, torch.from_numpy(y[lo:lo + B]).to(dev).reshape(-1, 1))


def _distance(a, b):
    return max((p0.detach() - p1.detach()).abs().max().item()
               for (_, p0), (_, p1) in zip(a.model.named_parameters(), b.model.named_parameters()))


@pytest.fixture(scope='module')
def kernel_bar(dev):
    """the weights' bar of case 1 at D = 16, for the model tests that are held to it"""
    return MARGIN * _baseline(dev, 16)[2]['p']


def test_through_the_model(dev, monkeypatch):
    """5. twelve eager steps of a ['dnn_nets'] model on a fixed feed: row-sparse tables with exact_rows against the same
    model on the dense-gradient path (Keras' semantics, existing code); the lazy default is the yardstick: rounding against a
    semantic difference of about lr per idle step, orders of magnitude apart"""
    from deeptables_amd.models import layers as dl
    df, y = _frame(B * 12)
    dense = _model()
    _fit(dense, df, y)
    with monkeypatch.context() as mp:
        mp.setattr(dl, 'DENSE_GRAD_MAX_ELEMS', 0)
        exact, lazy = _model(EXACT), _model()
        assert exact.optimizer.exact_rows and exact.fused_plan() is None
        _fit(exact, df, y)
        _fit(lazy, df, y)
        assert exact.optimizer.t == lazy.optimizer.t == dense.optimizer.t == 12
        d_exact, d_lazy = _distance(exact, dense), _distance(lazy, dense)
        print(f'12 steps: exact rows {d_exact:.3e} from the dense-gradient path, lazy rows {d_lazy:.3e}')
        assert d_exact <= d_lazy / 100
        # rows are pending again after one more step: predict through the inference plan sweeps them first
        _one_step(exact, df, y, 0, dev)
        mp.setenv('DT_AMD_TOWER_DTYPE', 'bf16x3')
        assert exact.optimizer._pending and exact.inference_plan() is not None
        through_plan = exact.predict(df, batch_size=16)
        assert not exact.optimizer._pending
        mp.setenv('DT_AMD_FUSED_PREDICT', '0')
        assert exact.inference_plan() is None
        layer_path = exact.predict(df, batch_size=16)
        err = np.abs(through_plan - layer_path).max()
        print(f'predict through the plan against the layer path: {err:.3e}')
        assert err <= 1e-5


def test_captured_steps(dev, monkeypatch):
    """6. fit(steps_per_execution=4) captures the catch-up and stamp launches with the rest of the layer-path step: same
    weights and loss curve as eager fitting, within the bar of tests/test_compiled_gpu.py's layer-path comparison (5e-6)"""
    from deeptables_amd.models import layers as dl
    monkeypatch.setattr(dl, 'DENSE_GRAD_MAX_ELEMS', 0)
    df, y = _frame(B * 12)
    eager, graphed = _model(EXACT), _model(EXACT)
    h0 = _fit(eager, df, y, 1, epochs=3, shuffle=True)
    h1 = _fit(graphed, df, y, 4, epochs=3, shuffle=True)
    assert eager.compiled_loop is None
    assert graphed.compiled_loop is not None and graphed.compiled_loop.graph is not None and graphed.compiled_loop.k == 4
    assert eager.optimizer.t == graphed.optimizer.t == 36
    d = _distance(eager, graphed)
    print(f'captured against eager, 36 steps: {d:.3e}')
    assert d <= 5e-6
    assert np.allclose(h0.history['loss'], h1.history['loss'], atol=5e-6), (h0.history, h1.history)


def test_checkpoint(dev, monkeypatch, tmp_path, kernel_bar):
    """7. save after an odd number of steps (5), with and without the optimizer; the uninterrupted run goes on for 3 steps.
    With the optimizer: a fresh model loads the file, takes the same 3 steps and ends within the bar of case 1.  Without it
    nothing can be continued (no slots, no step count); what the file must hold is the weights with every idle step paid —
    bit for bit the materialised tables — so that a fresh model that loads it predicts what the trained one predicts."""
    from deeptables_amd import checkpoint
    from deeptables_amd.models import layers as dl
    from safetensors import safe_open
    monkeypatch.setattr(dl, 'DENSE_GRAD_MAX_ELEMS', 0)
    monkeypatch.setenv('DT_AMD_FUSED_PREDICT', '0')
    df, y = _frame(B * 8)
    run = _model(EXACT)
    _fit(run, df.iloc[:B * 4], y[:B * 4])
    _one_step(run, df, y, B * 4, dev)           # (fit ends on a sweep; the fifth step leaves rows pending for the saves)
    assert run.optimizer.t == 5 and run.optimizer._pending
    with_opt, bare = str(tmp_path / 'with.safetensors'), str(tmp_path / 'bare.safetensors')
    run.save(bare, include_optimizer=False)
    run.save(with_opt, include_optimizer=True)
    table = run.model.layers_by_name['emb_categorical_vars_all'].tables['d16']
    assert (run.optimizer.state[id(table)]['stamp'] == 5).all()
    with safe_open(bare, framework='pt', device='cpu') as f:
        assert not any(k.startswith('optimizer/') for k in f.keys())
        for i, e in enumerate(run.model.layers_by_name['emb_categorical_vars_all'].embeddings):
            assert torch.equal(f.get_tensor(f'emb_categorical_vars_all/embeddings_{i}'), e.detach().cpu())
    fresh = _model(EXACT, seed=9)
    checkpoint.load_model(fresh.model, bare, optimizer=None)
    assert np.array_equal(fresh.predict(df, batch_size=16), run.predict(df, batch_size=16))
    resumed = _model('auto', seed=9)            # the file brings the mode with it
    meta = checkpoint.load_model(resumed.model, with_opt, optimizer=resumed.optimizer)
    assert resumed.optimizer.exact_rows and resumed.optimizer.t == 5 and meta['optimizer'] == 'Adam'
    assert resumed.fused_plan() is None
    _fit(run, df.iloc[B * 5:], y[B * 5:])
    _fit(resumed, df.iloc[B * 5:], y[B * 5:])
    assert run.optimizer.t == resumed.optimizer.t == 8
    d = _distance(run, resumed)
    print(f'resumed against uninterrupted, 5 + 3 steps: {d:.3e} (bar {kernel_bar:.3e})')
    assert d <= kernel_bar
