# -*- coding:utf-8 -*-
"""GPU: the Adagrad and RMSprop kernels (csrc/optim_slots.hip dt_adagrad_* / dt_rmsprop_*) and `training.Adagrad` /
`training.RMSprop` against the float64 restatement of Keras' formulas in tests/optim_reference.py.

Bars.  The update is fp32 element-wise arithmetic, the class of Adam's, and is held to the bars tests/test_optim_gpu.py
holds Adam's to, on weights of the same scale (randn dense tensors, 0.05 randn tables):
  * weights: 2e-6 absolute (W_BAR).  One step rounds w - u to half an ulp of w (2.4e-7 at |w| in [2, 4)); the update u
    ~ 1e-3 carries a few 1e-7 of relative error, 1e-9 absolute.
  * slots: 1e-6 of the tensor's largest entry (S_BAR x max(1, max |slot|)); Adam's m stays below 1, so there the same
    bar reads 1e-6 absolute.  acc += g^2 and rms = rho rms + (1 - rho) g^2 round twice or three times per step, 2^-24
    relative each: a few 1e-7 of the entry over three steps.  float(0.9) and 1 - float(0.9) differ from 0.9 and 0.1 by
    2.6e-8 and 2.4e-7 relative, inside the same bar.
  * RMSprop's lazy decay rho^idle: gaps up to 8 steps repeat the dense decay's own multiplications (bit-identical to
    decaying every step in fp32); a longer gap takes one powf: 1.1e-7 of the largest rms entry against float64
    (test_rmsprop_long_gap).  Neither needs more than S_BAR.
The duplicate lookups of a row are summed with float atomics in an order that changes from run to run; so that this does
not blur the check of the update, the sparse gradients here sit on a 2^-6 grid, |g| <= 4: any sum of up to 1000 of them is
exact in fp32."""
import ctypes

import numpy as np
import pytest
import torch

from tests import optim_reference as R

pytestmark = pytest.mark.gpu

W_BAR, S_BAR = 2e-6, 1e-6
KINDS = ('adagrad', 'rmsprop', 'rmsprop_record')       # RMSprop with its stamps in an array of their own / in the slot record


def _make(kind, params, emb_layers=()):
    from deeptables_amd import training as T
    if kind == 'adagrad':
        return T.Adagrad(params, emb_layers)
    opt = T.RMSprop(params, emb_layers)
    opt.stamp_in_record = kind == 'rmsprop_record'
    return opt


def _slot0(kind, like):
    return torch.full_like(like, 0.1 if kind == 'adagrad' else 0.0)


def _dense_ref(kind, p, g, s):
    return R.adagrad_step(p, g, s) if kind == 'adagrad' else R.rmsprop_step(p, g, s)


def _w_close(got, ref, what=''):
    err = (got.detach().double().cpu() - ref).abs().max().item()
    assert err <= W_BAR, (what, err)


def _s_close(got, ref, what=''):
    err = (got.detach().double().cpu() - ref).abs().max().item()
    assert err <= S_BAR * max(1.0, ref.abs().max().item()), (what, err, ref.abs().max().item())


class _FakeEmb:
    """MultiColumnEmbedding as the optimizer sees it (tests/test_optim_gpu.py)"""

    def __init__(self, table, n_fields):
        self.tables = {f'd{table.shape[1]}': table}
        self.groups = [(table.shape[1], list(range(n_fields)))]
        self.sparse_grads = {}


# ---- dense ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['adagrad', 'rmsprop'])
def test_dense_steps_match_keras_formulas(dev, kind):
    """three steps with fresh gradients at the sizes where the launch changes shape: one element, less than a float4, one
    short of / exactly / one past a 256-thread block of scalars, and 3 blocks of float4 pieces plus a scalar tail"""
    g = torch.Generator().manual_seed(0)
    for n in (1, 3, 255, 256, 257, 4 * 256 * 3 + 3):
        p0 = torch.randn(n, generator=g)
        p = torch.nn.Parameter(p0.clone().to(dev))
        opt = _make(kind, [p])
        rp, rs = p0.double(), _slot0(kind, p0).double()
        for t in range(1, 4):
            grad = torch.randn(n, generator=g) * (0.1 if t % 2 else 3.0)
            p.grad = grad.to(dev)
            opt.step()
            rp, rs = _dense_ref(kind, rp, grad.double(), rs)
            assert opt.t == t
            _w_close(p, rp, (n, t))
            _s_close(opt.slot(p), rs, (n, t))


@pytest.mark.parametrize('kind', ['adagrad', 'rmsprop'])
def test_dense_step_takes_float_aligned_pointers(dev, kind):
    """a pointer that is 4-byte but not 16-byte aligned is ACCEPTED: the launch takes the scalar loop instead of the float4
    body, with the same result bit for bit (whichever of p, g and the slot it is)"""
    from deeptables_amd._lib import check, lib, ptr
    g = torch.Generator().manual_seed(1)
    n = 1000
    p0, g0 = torch.randn(n, generator=g), torch.randn(n, generator=g)
    hp = (1e-3, 1e-7) if kind == 'adagrad' else (1e-3, 0.9, 1e-7)
    f = getattr(lib(), f'dt_{kind}_dense_step')
    outs = []
    for odd in (None, 0, 1, 2):
        bufs = [torch.empty(n + 4, device=dev) for _ in range(3)]
        views = [b[1:n + 1] if i == odd else b[:n] for i, b in enumerate(bufs)]
        assert all((v.data_ptr() % 16 == 4) == (i == odd) for i, v in enumerate(views))
        for v, src in zip(views, (p0, g0, _slot0(kind, p0))):
            v.copy_(src)
        check(f(ptr(views[0]), ptr(views[1]), ptr(views[2]), n, *hp, None, 0, None), kind)
        outs.append((views[0].cpu(), views[2].cpu()))
    rp, rs = _dense_ref(kind, p0.double(), g0.double(), _slot0(kind, p0).double())
    _w_close(outs[0][0], rp)
    _s_close(outs[0][1], rs)
    for w, s in outs[1:]:
        assert torch.equal(w, outs[0][0]) and torch.equal(s, outs[0][1])


@pytest.mark.parametrize('kind', ['adagrad', 'rmsprop'])
def test_multi_tensor_launch_equals_single_launches(dev, kind):
    """33 tensors of 1 .. 33 elements (one past the 32-tensor chunk) in one call against 33 dense calls: bit for bit, and
    the call advances the step counter once"""
    from deeptables_amd._lib import check, lib, ptr
    g = torch.Generator().manual_seed(2)
    hp = (1e-3, 1e-7) if kind == 'adagrad' else (1e-3, 0.9, 1e-7)
    ps = [torch.randn(k, generator=g) for k in range(1, 34)]
    gs = [torch.randn(k, generator=g) for k in range(1, 34)]
    one = [[t.clone().to(dev) for t in ps], [t.to(dev) for t in gs], [_slot0(kind, t).to(dev) for t in ps]]
    many = [[t.clone().to(dev) for t in ps], [t.to(dev) for t in gs], [_slot0(kind, t).to(dev) for t in ps]]
    opt = _make(kind, [torch.nn.Parameter(torch.zeros(1, device=dev))])
    state = opt._state_tensor(dev)
    dense = getattr(lib(), f'dt_{kind}_dense_step')
    for step in range(2):
        for p, gr, s in zip(*one):
            check(dense(ptr(p), ptr(gr), ptr(s), p.numel(), *hp, None, 0, None), kind)
        arr = ctypes.c_void_p * 33
        cols = [ctypes.cast(arr(*[t.data_ptr() for t in col]), ctypes.c_void_p) for col in many]
        ns = ctypes.cast((ctypes.c_int64 * 33)(*range(1, 34)), ctypes.c_void_p)
        check(getattr(lib(), f'dt_{kind}_multi_step')(33, *cols, ns, *hp, ptr(state), 1, None), kind)
        assert opt.t == step + 1
    for k in range(33):
        assert torch.equal(one[0][k], many[0][k]) and torch.equal(one[2][k], many[2][k]), k
    assert not torch.equal(one[0][32].cpu(), ps[32])


# ---- rows ----------------------------------------------------------------------------------------------------------------
V = 50


def _lookups(g, n, D, F):
    """n lookups of a 50-row table in shuffled order: row 0 looked up 300 times (fewer where fewer positions exist), three
    rows twice, a few lookups skipped (-1).  F > 0: the [.., F] layout of a packed table — lookup i belongs to field i % F,
    whose rows are [12 f, 12 f + 12); the repeated rows are field 0's, which has n / F positions (250 at n = 1000: row 0
    takes 242 of them)."""
    if F:
        ids = torch.randint(0, 12, (n,), generator=g) + (torch.arange(n) % F) * 12
        pos = torch.arange(0, n, F)
    else:
        ids = torch.randint(0, V, (n,), generator=g)
        pos = torch.arange(n)
    pos = pos[torch.randperm(pos.numel(), generator=g)]
    hot = min(300, max(pos.numel() - 8, pos.numel() // 2))
    if n >= 16:
        ids[pos[:hot]] = 0
        for k in range(3):
            if hot + 2 * k + 1 < pos.numel():
                ids[pos[hot + 2 * k]] = ids[pos[hot + 2 * k + 1]] = 1 + k
        ids[torch.randperm(n, generator=g)[:max(1, n // 50)]] = -1
    vals = (torch.randn(n, D, generator=g) * 64).round().clamp(-256, 256) / 64
    return ids, vals


@pytest.mark.parametrize('D', [4, 6, 16, 24, 32, 64, 301, 1028])
@pytest.mark.parametrize('kind', KINDS)
def test_rows_steps_match_keras_formulas(dev, kind, D):
    """D: float4 pieces with a whole number of rows per block (4, 16, 32, 64) and with idle lanes (24: six pieces a row);
    scalar pieces (6); more pieces than a block has threads (301 scalars, 1028 = 257 float4).  n: one lookup, one short of /
    exactly / one past 64, and 1000 (several blocks; field-local merge at n % 4 == 0, the global hash otherwise).  Three
    steps each (a row looked up at steps 1 and 3 only has a decay pending at step 3), with the `fields` hint 0 and 4."""
    from deeptables_amd.ops import SparseRowGrad
    g = torch.Generator().manual_seed(D)
    for F in (0, 4):
        for n in (1, 63, 64, 65, 1000):
            t0 = torch.randn(V, D, generator=g) * 0.05
            table = torch.nn.Parameter(t0.clone().to(dev))
            emb = _FakeEmb(table, F)
            opt = _make(kind, [table], [emb])
            rp, rs = t0.double(), _slot0(kind, t0).double()
            key = opt.slot_names[0]
            for t in range(1, 4):
                ids, vals = _lookups(g, n, D, F)
                before = table.detach().clone()
                acc_before = None
                if kind == 'adagrad':
                    acc_before = opt.state[id(table)]['acc'].clone() if t > 1 else torch.full((V, D), 0.1, device=dev)
                emb.sparse_grads = {f'd{D}': [SparseRowGrad(ids.to(dev), vals.clone().to(dev))]}
                opt.step()
                assert opt.t == t
                if kind == 'adagrad':
                    rp, rs = R.adagrad_rows_step(rp, rs, ids, vals.double())
                else:
                    rp, rs = R.rmsprop_rows_step(rp, rs, ids, vals.double())
                touched = torch.zeros(V, dtype=torch.bool)
                touched[ids[ids >= 0]] = True
                what = (F, n, t)
                _w_close(table[touched], rp[touched], what)
                assert torch.equal(table.detach()[~touched].cpu(), before[~touched].cpu()), what      # bit for bit
                if acc_before is not None:
                    assert torch.equal(opt.state[id(table)]['acc'][~touched].cpu(), acc_before[~touched].cpu()), what
                _s_close(opt.state[id(table)][key][touched], rs[touched], what)    # (raw: nothing is pending on these)
            _s_close(opt.slot(table), rs, (F, n))
            if 'slots' in opt.state[id(table)]:
                assert int(opt.state[id(table)]['slots'].abs().sum().item()) == 0     # the global hash is left empty


@pytest.mark.parametrize('kind', ['rmsprop', 'rmsprop_record'])
def test_rmsprop_lazy_decay_equals_decaying_every_row(dev, kind):
    """5 steps on 50 rows: rows 0-9 looked up at steps 1 and 4, rows 10-19 at step 3, rows 20-29 at every step, the rest
    never.  After every step the looked-up rows' weights are Keras'; after materialize() rms of ALL rows is Keras' slot;
    a further step equals the reference too."""
    from deeptables_amd.ops import SparseRowGrad
    g = torch.Generator().manual_seed(7)
    D = 16
    when = {1: [0, 20], 2: [20], 3: [10, 20], 4: [0, 20], 5: [20], 6: [0, 10, 20, 30]}
    t0 = torch.randn(V, D, generator=g) * 0.05
    table = torch.nn.Parameter(t0.clone().to(dev))
    emb = _FakeEmb(table, 0)
    opt = _make(kind, [table], [emb])
    rp, rs = t0.double(), torch.zeros(V, D, dtype=torch.float64)
    rho32 = torch.tensor(0.9, dtype=torch.float32)
    raw3 = None

    def step(t):
        nonlocal rp, rs
        ids = torch.cat([torch.arange(s, s + 10) for s in when[t]])
        ids = torch.cat([ids, ids[:3]])[torch.randperm(ids.numel() + 3, generator=g)]          # three rows looked up twice
        vals = (torch.randn(ids.numel(), D, generator=g) * 64).round() / 64
        emb.sparse_grads = {'d16': [SparseRowGrad(ids.to(dev), vals.clone().to(dev))]}
        opt.step()
        rp, rs = R.rmsprop_rows_step(rp, rs, ids, vals.double())
        _w_close(table, rp, t)

    for t in range(1, 6):
        step(t)
        if t == 3:
            raw3 = opt.state[id(table)]['rms'][10:20].cpu().clone()
    st = opt.state[id(table)]
    assert st['stamp'].cpu().tolist() == [4] * 10 + [3] * 10 + [5] * 10 + [0] * 20
    assert torch.equal(st['rms'][10:20].cpu(), raw3)                     # decay is pending on the rows looked up at step 3 only
    rms = opt.slot(table).cpu()                                          # materialize()
    _s_close(rms, rs)
    assert float(rms[30:].abs().max()) == 0.0                            # never looked up: exactly 0
    assert torch.equal(rms[10:20], (raw3 * rho32) * rho32)               # rho^2 of its value, as two dense decays round it
    assert st['stamp'].cpu().tolist() == [5] * V and opt.t == 5
    before = table.detach().clone()
    opt.materialize()                                                    # nothing pending: nothing changes
    assert torch.equal(opt.state[id(table)]['rms'].cpu(), rms) and torch.equal(table.detach(), before)
    step(6)
    _s_close(opt.slot(table), rs)


def test_rmsprop_long_gap(dev):
    """a row that sits out more than 8 steps takes its decay as one powf(rho, idle): rows 0-3 at steps 1 and 13
    (idle = 11).  Measured against float64 on an MI355X: weights 8.0e-9, rms 1.1e-7 of its largest entry."""
    from deeptables_amd.ops import SparseRowGrad
    g = torch.Generator().manual_seed(11)
    D, Vs = 4, 8
    t0 = torch.randn(Vs, D, generator=g) * 0.05
    table = torch.nn.Parameter(t0.clone().to(dev))
    emb = _FakeEmb(table, 0)
    opt = _make('rmsprop', [table], [emb])
    rp, rs = t0.double(), torch.zeros(Vs, D, dtype=torch.float64)
    for t in range(1, 14):
        ids = torch.arange(0, 4) if t in (1, 13) else torch.arange(4, 8)
        vals = (torch.randn(4, D, generator=g) * 64).round() / 64
        emb.sparse_grads = {'d4': [SparseRowGrad(ids.to(dev), vals.clone().to(dev))]}
        opt.step()
        rp, rs = R.rmsprop_rows_step(rp, rs, ids, vals.double())
    print('long gap: w err', (table.detach().double().cpu() - rp).abs().max().item(), 'rms err / max',
          (opt.slot(table).double().cpu() - rs).abs().max().item() / rs.abs().max().item())
    _w_close(table, rp)
    _s_close(opt.slot(table), rs)


# ---- models --------------------------------------------------------------------------------------------------------------
def _real_table_model(optimizer, dev):
    from deeptables_amd import functional
    from deeptables_amd.models import ModelConfig, DeepModel
    from deeptables_amd.models.metainfo import CategoricalColumn, ContinuousColumn
    functional.set_seed(3)
    conf = ModelConfig(nets=['linear', 'fm_nets', 'dnn_nets'], fixed_embedding_dim=True, embeddings_output_dim=16,
                       embedding_dropout=0, optimizer=optimizer)
    vocabs = [300000, 11, 7, 30]
    cats = [CategoricalColumn(f'C{i}', v, 16) for i, v in enumerate(vocabs)]
    dm = DeepModel('binary', 2, conf, cats, [ContinuousColumn('input_continuous_all', ['a', 'b', 'c'])])
    dm.build(dev)
    return dm, vocabs


@pytest.mark.parametrize('optimizer', ['adagrad', 'rmsprop'])
def test_row_sparse_update_of_a_real_table(dev, optimizer):
    """a 300,000-row column (4.8 M floats: above DENSE_GRAD_MAX_ELEMS, so its table keeps a sparse gradient) next to three
    small ones: the weights after every one of three steps are the float64 formula applied to the gradients the step
    handed to the optimizer, and rows that were not looked up do not move"""
    dm, vocabs = _real_table_model(optimizer, dev)
    emb = dm.model.layers_by_name['emb_categorical_vars_all']
    table = emb.tables['d16']
    assert not emb.uses_dense_grad(16)
    g = torch.Generator().manual_seed(5)
    B, Vt = 64, table.shape[0]
    dm.model.train()
    dense_params = [p for p in dm.optimizer.params if p is not table]
    refs = {id(p): (p.detach().double().cpu(), _slot0(optimizer, p.detach().cpu()).double()) for p in dense_params}
    rslot = _slot0(optimizer, torch.empty(Vt, 16)).double()
    sample = torch.randperm(Vt, generator=g)[:1200]
    for t in range(1, 4):
        idx = torch.stack([torch.randint(0, v, (B,), generator=g) for v in vocabs], 1)
        y = (torch.rand(B, 1, generator=g) < 0.3).float()
        dm.forward_backward([idx.int().to(dev), torch.randn(B, 3, generator=g).to(dev)], y.to(dev))
        (sg,) = emb.sparse_grads['d16']
        rows, vals = sg.rows.reshape(-1).cpu(), sg.values.reshape(-1, 16).double().cpu()
        grads = {id(p): p.grad.detach().double().cpu().reshape(p.shape) for p in dense_params if p.grad is not None}
        assert len(grads) >= len(dense_params) - 1
        looked = torch.unique(rows[rows >= 0])
        assert looked.numel() > 64
        before, quiet = table.detach()[looked].double().cpu(), sample[~torch.isin(sample, looked)][:1000]
        quiet_before = table.detach()[quiet].clone()
        dm.optimizer.step()
        assert dm.optimizer.t == t
        for p in dense_params:
            if id(p) in grads:
                refs[id(p)] = _dense_ref(optimizer, refs[id(p)][0], grads[id(p)], refs[id(p)][1])
            _w_close(p, refs[id(p)][0], t)
        gsum = torch.zeros(Vt, 16, dtype=torch.float64).index_add_(0, rows[rows >= 0], vals[rows >= 0])[looked]
        if optimizer == 'rmsprop':
            rslot *= 0.9                                      # Keras: every row's rms decays every step
            rslot[looked] += (1 - 0.9) * gsum * gsum
        else:
            rslot[looked] += gsum * gsum
        _w_close(table.detach()[looked], before - 1e-3 * gsum / (rslot[looked].sqrt() + 1e-7), t)
        assert quiet.numel() == 1000 and torch.equal(table.detach()[quiet], quiet_before)
    _s_close(dm.optimizer.slot(table), rslot)


@pytest.mark.parametrize('tower_mode', ['bf16x3', 'f32'])
def test_fused_forward_backward_with_a_separate_adagrad_update(dev, monkeypatch, tower_mode):
    """DeepFM with optimizer='adagrad': the fused plan runs forward + backward and leaves the WHOLE update to
    optimizer.step() (no rows applied inside the step, no segments); three steps agree with the layer-by-layer path
    (DT_AMD_FUSED=0) to the bar of test_fused_gpu.py's fused-versus-layer comparison of train steps."""
    from tests.test_fused_gpu import batch, build, rel
    from deeptables_amd.models import layers as L
    monkeypatch.setattr(L, 'DENSE_GRAD_MAX_ELEMS', 0)                    # row-sparse table: the rows kernel runs
    monkeypatch.setenv('DT_AMD_TOWER_DTYPE', tower_mode)
    F, Nd, D, B = 26, 13, 16, 256
    dm, cats = build(F, Nd, D, vocab=300, optimizer='adagrad')
    monkeypatch.setenv('DT_AMD_FUSED', '0')
    twin, _ = build(F, Nd, D, vocab=300, optimizer='adagrad')
    assert twin.fused_plan() is None
    monkeypatch.setenv('DT_AMD_FUSED', '1')
    assert dm.fused_plan() is not None
    with torch.no_grad():
        for (n1, p1), (n2, p2) in zip(dm.model.named_parameters(), twin.model.named_parameters()):
            p2.copy_(p1)
    seen = []
    real_step = dm.optimizer.step

    def spy():
        seen.extend((sg.fields, sg.segments) for layer in dm.optimizer.embedding_layers
                    for sgs in layer.sparse_grads.values() for sg in sgs)
        real_step()
    dm.optimizer.step = spy
    dm.model.train(); twin.model.train()
    for step in range(3):
        idx, dense, y = batch(cats, Nd, B, seed=40 + step)
        ins = [idx.int().to(dev), dense.to(dev)]
        l1, _ = dm.train_step(ins, y.to(dev))
        l2, _ = twin.train_step(ins, y.to(dev))
        assert dm._step_used_plan and not twin._step_used_plan
        assert abs(float(l1) - float(l2)) < 2e-5, step
    assert len(seen) == 3 and all(f != -2 and s is None for f, s in seen)
    assert dm.optimizer.t == twin.optimizer.t == 3
    for (n1, p1), (_, p2) in zip(dm.model.named_parameters(), twin.model.named_parameters()):
        assert rel(p1, p2) < (5e-4 if tower_mode == 'f32' else 3e-3), n1      # (test_fused_gpu.py's two bars)


@pytest.mark.parametrize('optimizer', ['adagrad', 'rmsprop'])
def test_checkpoint_round_trip_with_the_slots(dev, tmp_path, monkeypatch, optimizer):
    """two train steps, save(include_optimizer=True), load into a fresh model: weights, slots and step count are bit
    identical, and so are they after one more optimizer step on both.  That step is fed the SAME gradient bits on both
    sides (model A's forward + backward: the batch sums of a backward pass are float atomics, two runs of it differ in
    the last bits) on a batch without repeated ids (the merge of repeated lookups is a float-atomic sum as well).
    RMSprop: decay is pending on rows at save time; the file holds the materialized slot."""
    from tests.test_fused_gpu import batch, build
    from deeptables_amd.models import DeepModel
    from deeptables_amd.models import layers as L
    from deeptables_amd.ops import SparseRowGrad
    from safetensors import safe_open
    monkeypatch.setattr(L, 'DENSE_GRAD_MAX_ELEMS', 0)
    F, Nd, D = 6, 3, 16
    dm, cats = build(F, Nd, D, vocab=80, optimizer=optimizer)
    dm.model.train()
    for step in range(2):
        idx, dense, y = batch(cats, Nd, 48, seed=step)
        dm.train_step([idx.int().to(dev), dense.to(dev)], y.to(dev))
    emb = dm.model.layers_by_name['emb_categorical_vars_all']
    table = emb.tables['d16']
    if optimizer == 'rmsprop':
        assert bool((dm.optimizer.state[id(table)]['stamp'] == 1).any())             # looked up at step 1, not at step 2
    path = str(tmp_path / 'dm.safetensors')
    dm.save(path, include_optimizer=True)
    with safe_open(path, framework='pt', device='cpu') as f:
        slot = dm.optimizer.slot_names[0]
        keys = [k for k in f.keys() if k.startswith('optimizer/')]
        assert keys and all(k.endswith('/' + slot) for k in keys)                       # no key of Adam's (.../m, .../v)
        meta = f.metadata()
    assert meta['optimizer'] == dm.optimizer._name and meta['optimizer_iterations'] == '2'
    assert 'learning_rate' in meta['optimizer_hyperparameters']
    dm2 = DeepModel('binary', 2, dm.config, dm.categorical_columns, dm.continuous_columns, model_file=path)
    assert type(dm2.optimizer) is type(dm.optimizer) and dm2.optimizer.t == 2

    def same(tensors):
        for a, b in zip(tensors(dm.model), tensors(dm2.model)):
            assert torch.equal(a, b)
        for pa, pb in zip(dm.optimizer.params, dm2.optimizer.params):
            sa, sb = dm.optimizer.slot(pa), dm2.optimizer.slot(pb)
            assert (sa is None) == (sb is None) and (sa is None or torch.equal(sa, sb.reshape(sa.shape)))
        assert dm.optimizer.t == dm2.optimizer.t
    same(lambda m: m.state_dict().values())
    g = torch.Generator().manual_seed(9)
    idx = torch.stack([torch.randperm(80, generator=g)[:48] for _ in range(F)], 1)        # no id twice in a column
    _, dense, y = batch(cats, Nd, 48, seed=7)
    dm.forward_backward([idx.int().to(dev), dense.to(dev)], y.to(dev))
    emb2 = dm2.model.layers_by_name['emb_categorical_vars_all']
    dm2.optimizer.zero_grad()
    for pa, pb in zip(dm.optimizer.params, dm2.optimizer.params):
        if pa.grad is not None:
            pb.grad = pa.grad.detach().clone().reshape(pb.shape)
    emb2.sparse_grads = {k: [SparseRowGrad(sg.rows.clone(), sg.values.clone(), fields=sg.fields) for sg in sgs]
                         for k, sgs in emb.sparse_grads.items()}
    assert emb2.sparse_grads
    dm.optimizer.step()
    dm2.optimizer.step()
    assert dm.optimizer.t == 3
    same(lambda m: m.parameters())                  # (the moving statistics of model A saw a forward pass more)
    # an Adam model refuses the file's slots, and says why
    adam = DeepModel('binary', 2, dm.config._replace(optimizer='adam'), dm.categorical_columns, dm.continuous_columns)
    with pytest.raises(ValueError, match=dm.optimizer._name):
        adam._load_model(path)
    # ... and the reverse
    adam.model.train()
    adam.train_step([idx.int().to(dev), dense.to(dev)], y.to(dev))
    adam_path = str(tmp_path / 'adam.safetensors')
    adam.save(adam_path, include_optimizer=True)
    with pytest.raises(ValueError, match='Adam'):
        DeepModel('binary', 2, dm.config, dm.categorical_columns, dm.continuous_columns, model_file=adam_path)


@pytest.mark.parametrize('optimizer', ['adagrad', 'rmsprop'])
def test_graphed_fit_replays_the_new_optimizers(dev, monkeypatch, optimizer):
    """`fit(steps_per_execution=5)` captures the optimizer step with the rest (compiled.py takes any optimizer: the step
    counter and RMSprop's stamps live on the device) and equals the eager fit after one epoch of 13 steps — two replays of
    five and three eager steps — at the bar tests/test_compiled_gpu.py holds the row-sparse Adam fit to."""
    from tests.test_compiled_gpu import _fit, _frame, _model, _same
    from deeptables_amd.models import layers as L
    monkeypatch.setattr(L, 'DENSE_GRAD_MAX_ELEMS', 0)
    df, y = _frame(64 * 13 + 5)
    eager, graphed = _model('DeepFM', optimizer=optimizer), _model('DeepFM', optimizer=optimizer)
    h0 = _fit(eager, df, y, 1, epochs=1)
    h1 = _fit(graphed, df, y, 5, epochs=1)
    assert eager.compiled_loop is None
    loop = graphed.compiled_loop
    assert loop is not None and loop.graph is not None and loop.k == 5 and not loop.chained
    assert eager.optimizer.t == graphed.optimizer.t == 13
    _same(eager, graphed, tol=2e-6)
    assert np.allclose(h0.history['loss'], h1.history['loss'], atol=2e-6), (h0.history, h1.history)


@pytest.mark.parametrize('preset', ['WideDeep', 'DeepFM', 'xDeepFM', 'AutoInt', 'DCN', 'FGCNN', 'FiBiNet', 'PNN', 'AFM'])
def test_every_preset_trains_with_both_optimizers(dev, preset):
    """DeepTable's presets (deepnets.py) compile and train with optimizer='adagrad' / 'rmsprop': two steps each, the loss
    and every weight stay finite, most tensors have moved and every tensor that moved has a slot"""
    from tests.test_fused_gpu import batch, build
    from deeptables_amd.models import deepnets
    F, Nd, D = 9, 4, (32 if preset == 'AutoInt' else 16)
    for optimizer in ('adagrad', 'rmsprop'):
        dm, cats = build(F, Nd, D, vocab=30, nets=getattr(deepnets, preset), optimizer=optimizer)
        dm.model.train()
        start = [p.detach().clone() for p in dm.optimizer.params]
        for step in range(2):
            idx, dense, y = batch(cats, Nd, 64, seed=step)
            loss, _ = dm.train_step([idx.int().to(dev), dense.to(dev)], y.to(dev))
            assert np.isfinite(float(loss))
        assert dm.optimizer.t == 2 and dm.optimizer._name == {'adagrad': 'Adagrad', 'rmsprop': 'RMSprop'}[optimizer]
        moved = [not torch.equal(p.detach(), s) for p, s in zip(dm.optimizer.params, start)]
        assert sum(moved) > len(moved) // 2 and all(bool(torch.isfinite(p).all()) for p in dm.optimizer.params), (preset, moved)
        assert all(dm.optimizer.slot(p) is not None for p, m in zip(dm.optimizer.params, moved) if m)


@pytest.mark.parametrize('kind', ['adagrad', 'rmsprop'])
def test_pre_dense_hook_orders_table_updates_first(dev, kind):
    """the data-parallel strategy's hook (an all-reduce pending on the dense gradients): the table update is launched first,
    the hook runs, then the dense update advances the counter — the same bits as the step without a hook, whose dense
    update rides in the row launch's trailing blocks"""
    from deeptables_amd.ops import SparseRowGrad
    g = torch.Generator().manual_seed(9)
    D, F, B, vocab = 16, 2, 128, 500
    t0 = torch.randn(F * vocab, D, generator=g) * 0.05
    w0, wg = torch.randn(300, generator=g), torch.randn(300, generator=g)
    rows = (torch.randint(0, vocab, (B, F), generator=g) + torch.arange(F) * vocab).reshape(-1)
    vals = (torch.randn(B * F, D, generator=g) * 64).round() / 64
    out = []
    for use_hook in (False, True):
        table = torch.nn.Parameter(t0.clone().to(dev))
        w = torch.nn.Parameter(w0.clone().to(dev))
        emb = _FakeEmb(table, F)
        opt = _make(kind, [table, w], [emb])
        called = []
        for step in range(2):
            w.grad = wg.to(dev) * (0.5 if use_hook else 1.0)
            emb.sparse_grads = {'d16': [SparseRowGrad(rows.to(dev), vals.clone().to(dev))]}
            if use_hook:
                def hook(w=w):
                    called.append(1)
                    w.grad.mul_(2.0)              # what the pending all-reduce would deliver
                opt.pre_dense_hook = hook
            opt.step()
        assert opt.t == 2 and (len(called) == 2) == use_hook and opt.pre_dense_hook is None
        out.append((table.detach().cpu().clone(), w.detach().cpu().clone(), opt.slot(w).cpu().clone()))
    assert all(torch.equal(a, b) for a, b in zip(*out))


def test_flat_dense_parameters_train_like_separate_tensors(dev, monkeypatch, optimizer='adagrad'):
    """DT_AMD_FLAT_PARAMS=1 (`training.flatten_dense_parameters`): every dense parameter, gradient and slot lives in one flat
    buffer and the dense update is ONE launch; two steps agree with the model that keeps them apart.  (Adagrad: its update
    is proportional to the gradient where the accumulator is still near its initial value, so the last bits of a backward
    pass's atomic sums stay last bits; RMSprop and Adam normalise a gradient of pure rounding noise to a full-size step.)"""
    from tests.test_fused_gpu import batch, build
    from deeptables_amd.models import deepnets
    models = []
    for flat in ('0', '1'):
        monkeypatch.setenv('DT_AMD_FLAT_PARAMS', flat)
        dm, cats = build(9, 4, 16, vocab=30, nets=deepnets.AFM, optimizer=optimizer)
        assert (dm.optimizer._flat is not None) == (flat == '1')
        dm.model.train()
        for step in range(2):
            idx, dense, y = batch(cats, 4, 64, seed=step)
            dm.train_step([idx.int().to(dev), dense.to(dev)], y.to(dev))
        models.append(dm)
    for (n0, p0), (_, p1) in zip(models[0].model.named_parameters(), models[1].model.named_parameters()):
        assert (p0 - p1).abs().max().item() <= W_BAR, n0


@pytest.mark.parametrize('kind', ['adam', 'adagrad', 'rmsprop'])
def test_flat_group_paths_equal_independent_tensors(dev, kind):
    """A flat group of three members — [4, 6] (24 elements), [5, 8] (40) as a strided view inside a zero-padded [5, 16] slab,
    [7] — registered once with grad_views=True, against the same parameters held as independent tensors under the same
    optimizer, fed the same gradients.  Two steps each of: the gradients ARE the flat views (one flat launch); the
    gradients are separate tensors (scattered into the flat gradient buffer, one flat launch); only the strided member has
    a gradient (contiguous copies updated on their own and written back).  The update is element-wise, so after every step
    parameters and slots are equal bit for bit (as test_multi_tensor_launch_equals_single_launches holds the multi launch
    to the single ones), and what lies between the members — parameter and slots — keeps exactly its initial value."""
    from deeptables_amd import training as T
    g = torch.Generator().manual_seed(11)
    keys = {'adam': ('m', 'v'), 'adagrad': ('acc',), 'rmsprop': ('rms',)}[kind]
    make = (lambda ps: T.KerasAdam(ps)) if kind == 'adam' else (lambda ps: _make(kind, ps))
    layout = ((5, 8), (16, 1))
    specs = [((4, 6), 0, 24, None), ((5, 8), 64, 40, layout), ((7,), 144, 7, None)]
    n_flat = 192
    flat_p = torch.zeros(n_flat, device=dev)
    flat_g = torch.zeros(n_flat, device=dev)
    between = torch.ones(n_flat, dtype=torch.bool, device=dev)
    members, twins = [], []
    for shape, off, cnt, lay in specs:
        w0 = torch.randn(shape, generator=g)
        view = torch.as_strided(flat_p, lay[0], lay[1], off) if lay else flat_p[off:off + cnt].view(shape)
        view.copy_(w0)
        (torch.as_strided(between, lay[0], lay[1], off) if lay else between[off:off + cnt]).fill_(False)
        p = torch.nn.Parameter(torch.empty(0, device=dev))
        p.data = view
        members.append((p, off, cnt, lay) if lay else (p, off, cnt))
        twins.append(torch.nn.Parameter(w0.clone().to(dev)))
    params = [mb[0] for mb in members]
    assert not params[1].data.is_contiguous() and int(between.sum()) == n_flat - 71
    opt, ref = make(params), make(twins)
    opt.register_flat_group(flat_p, flat_g, members, n_flat, grad_views=True)
    slot_init = [s.clone() for s in opt._flat[2:4] if s is not None]
    for step, how in enumerate(('views', 'views', 'scatter', 'scatter', 'strided only', 'strided only')):
        grads = [torch.randn(p.shape, generator=g).to(dev) * (3.0 if step % 2 else 0.1) for p in params]
        before = [q.detach().clone() for q in twins]
        opt.zero_grad(flat=how == 'views')
        ref.zero_grad()
        for i, (p, q, gr) in enumerate(zip(params, twins, grads)):
            if how == 'strided only' and i != 1:
                continue
            if how == 'views':
                assert p.grad is p._dt_grad_view
                p.grad.copy_(gr)
            else:
                p.grad = gr.clone()
            q.grad = gr.clone()
        opt.step()
        ref.step()
        assert opt.t == ref.t == step + 1
        for i, (p, q) in enumerate(zip(params, twins)):
            assert torch.equal(p.detach(), q.detach()), (how, step, i)
            for k in keys:
                assert torch.equal(opt.state[id(p)][k], ref.state[id(q)][k]), (how, step, i, k)
        assert float(flat_p[between].abs().max()) == 0.0, (how, step)
        for s, s0 in zip([s for s in opt._flat[2:4] if s is not None], slot_init):
            assert torch.equal(s[between], s0[between]), (how, step)
        moved = [not torch.equal(q.detach(), q0) for q, q0 in zip(twins, before)]
        assert moved == ([False, True, False] if how == 'strided only' else [True] * 3), (how, step)
