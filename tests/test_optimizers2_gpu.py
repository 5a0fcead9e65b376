# -*- coding:utf-8 -*-
"""GPU: the momentum SGD, Adamax and Ftrl kernels (csrc/optim_slots.hip dt_sgdm_* / dt_adamax_* / dt_ftrl_*) and
`training.SGD(momentum != 0)` / `training.Adamax` / `training.Ftrl` against the float64 restatement of Keras 3's formulas in
tests/optimizers2_reference.py.

Bars: those of tests/test_optimizers_gpu.py, on weights of the same scale (randn dense tensors, 0.05 randn tables):
  * weights: 2e-6 absolute (W_BAR);
  * slots: 1e-6 of the tensor's largest entry (S_BAR x max(1, max |slot|)).
Measured on an MI355X over the dense test's sizes and steps (the test prints every figure): weights within 3.5e-7 of
float64 for every kind; Ftrl's `linear` within 3.9e-4 at max |linear| 1881 (sqrtf kinds) and, for power -0.7, 1.6e-3 at 6086
and 8.5e-4 at 2180 — 2.6 x under S_BAR at the closest, so the powf kind stays on the project's bars too.  Ftrl's
n'^a - n^a is NOT evaluated as a difference of two float32 powers in the kernel: that cancels to a few bits for a small
gradient (a single element missed the slot bar at step 1 by 12 x: 2.4e-5 at |linear| = 1.88) — DESIGN.md §3.11.
The duplicate lookups of a row are summed with float atomics in an order that changes from run to run; so that this does
not blur the check of the update, the sparse gradients here sit on a 2^-6 grid, |g| <= 4: any sum of up to 1000 of them is
exact in fp32."""
import ctypes

import numpy as np
import pytest
import torch

from tests import optimizers2_reference as R

pytestmark = pytest.mark.gpu

W_BAR, S_BAR = 2e-6, 1e-6
KINDS = ('sgdm', 'sgdm_nesterov', 'adamax', 'ftrl', 'ftrl_reg', 'ftrl_pow')
FTRL_REG = dict(l1=0.02, l2=0.01, l2_shrinkage=0.01, beta=0.1)
FTRL_POW = dict(lr_power=-0.7, l1=0.02)
# kind -> (entry-point family, constructor arguments, slot names, initial values, l1)
CFG = {
    'sgdm': ('sgdm', dict(momentum=0.9), ('momentum',), (0.0,), 0.0),
    'sgdm_nesterov': ('sgdm', dict(momentum=0.9, nesterov=True), ('momentum',), (0.0,), 0.0),
    'adamax': ('adamax', {}, ('m', 'u'), (0.0, 0.0), 0.0),
    'ftrl': ('ftrl', {}, ('accumulator', 'linear'), (0.1, 0.0), 0.0),
    'ftrl_reg': ('ftrl', dict(l1_regularization_strength=0.02, l2_regularization_strength=0.01,
                              l2_shrinkage_regularization_strength=0.01, beta=0.1), ('accumulator', 'linear'), (0.1, 0.0), 0.02),
    'ftrl_pow': ('ftrl', dict(learning_rate_power=-0.7, l1_regularization_strength=0.02), ('accumulator', 'linear'),
                 (0.1, 0.0), 0.02),
}


def _make(kind, params, emb_layers=(), **more):
    from deeptables_amd import training as T
    cls = {'sgdm': T.SGD, 'adamax': T.Adamax, 'ftrl': T.Ftrl}[CFG[kind][0]]
    return cls(params, emb_layers, **dict(CFG[kind][1], **more))


def _slots0(kind, like):
    return tuple(torch.full_like(like, v) for v in CFG[kind][3])


def _ref_step(kind, t):
    """-> f(p, g, *slots) -> (p, *slots) in the dtype of its inputs, at step t (1-based)"""
    if kind.startswith('sgdm'):
        return lambda p, g, m: R.sgdm_step(p, g, m, nesterov=kind == 'sgdm_nesterov')
    if kind == 'adamax':
        return lambda p, g, m, u: R.adamax_step(p, g, m, u, t)
    kw = {'ftrl': {}, 'ftrl_reg': FTRL_REG, 'ftrl_pow': FTRL_POW}[kind]
    return lambda p, g, n, lin: R.ftrl_step(p, g, n, lin, **kw)


def _dense_ref(kind, t, p, g, slots):
    out = _ref_step(kind, t)(p, g, *slots)
    return out[0], tuple(out[1:])


def _w_close(got, ref, what=''):
    err = (got.detach().double().cpu() - ref).abs().max().item()
    assert err <= W_BAR, (what, err)


def _s_close(got, ref, what=''):
    err = (got.detach().double().cpu() - ref).abs().max().item()
    assert err <= S_BAR * max(1.0, ref.abs().max().item()), (what, err, ref.abs().max().item())


def _l1_zeros(kind, got_w, ref_linear, what):
    """Ftrl with l1 > 0: where the reference's |linear| is inside the clip by more than the slot bar, the weight is exactly 0.0
    -> how many such elements there are"""
    l1 = CFG[kind][4]
    if not l1:
        return 0
    inside = ref_linear.abs() < l1 - S_BAR * max(1.0, ref_linear.abs().max().item())
    w = got_w.detach().cpu()
    assert bool((w[inside] == 0.0).all()), (what, int(inside.sum()), w[inside].abs().max().item())
    return int(inside.sum())


class _FakeEmb:
    """MultiColumnEmbedding as the optimizer sees it (tests/test_optim_gpu.py)"""

    def __init__(self, table, n_fields):
        self.tables = {f'd{table.shape[1]}': table}
        self.groups = [(table.shape[1], list(range(n_fields)))]
        self.sparse_grads = {}


# ---- dense ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
def test_dense_steps_match_keras_formulas(dev, kind):
    """three steps with fresh gradients at the sizes where the launch changes shape: one element, less than a float4, one
    short of / exactly / one past a 256-thread block of scalars, and 3 blocks of float4 pieces plus a scalar tail"""
    g = torch.Generator().manual_seed(0)
    for n in (1, 3, 255, 256, 257, 4 * 256 * 3 + 3):
        p0 = torch.randn(n, generator=g)
        p = torch.nn.Parameter(p0.clone().to(dev))
        opt = _make(kind, [p])
        rp, rs = p0.double(), tuple(s.double() for s in _slots0(kind, p0))
        for t in range(1, 4):
            grad = torch.randn(n, generator=g) * (0.1 if t % 2 else 3.0)
            p.grad = grad.to(dev)
            opt.step()
            rp, rs = _dense_ref(kind, t, rp, grad.double(), rs)
            assert opt.t == t
            err_w = (p.detach().double().cpu() - rp).abs().max().item()
            err_s = [(opt.slot(p, k).double().cpu() - r).abs().max().item() for k, r in zip(opt.slot_names, rs)]
            print(kind, 'n', n, 't', t, 'w err', err_w, 'slot err', err_s, 'slot max', [r.abs().max().item() for r in rs])
            _w_close(p, rp, (n, t))
            for k, r in zip(opt.slot_names, rs):
                _s_close(opt.slot(p, k), r, (n, t, k))
            zeros = _l1_zeros(kind, p, rs[-1], (n, t))
            if CFG[kind][4] and n == 4 * 256 * 3 + 3 and t == 1:
                assert zeros >= 1                         # (about 4 % of the elements: the check is never vacuous)


@pytest.mark.parametrize('kind', KINDS)
def test_dense_step_takes_float_aligned_pointers(dev, kind):
    """a pointer that is 4-byte but not 16-byte aligned is ACCEPTED: the launch takes the scalar loop instead of the float4
    body, with the same result bit for bit (whichever of p, g and the slots it is)"""
    from deeptables_amd._lib import check, lib, ptr
    g = torch.Generator().manual_seed(1)
    n = 1000
    p0, g0 = torch.randn(n, generator=g), torch.randn(n, generator=g)
    opt = _make(kind, [torch.nn.Parameter(torch.zeros(1, device=dev))])
    state = opt._state_tensor(dev)
    f = getattr(lib(), f'dt_{CFG[kind][0]}_dense_step')
    ns = len(opt.slot_names)
    outs = []
    for odd in [None] + list(range(2 + ns)):
        bufs = [torch.empty(n + 4, device=dev) for _ in range(2 + ns)]
        views = [b[1:n + 1] if i == odd else b[:n] for i, b in enumerate(bufs)]
        assert all((v.data_ptr() % 16 == 4) == (i == odd) for i, v in enumerate(views))
        for v, src in zip(views, (p0, g0) + _slots0(kind, p0)):
            v.copy_(src)
        check(f(*[ptr(v) for v in views], n, *opt._hpargs(), ptr(state), 0, None), kind)
        outs.append([views[0].cpu()] + [v.cpu() for v in views[2:]])
    assert opt.t == 0
    rp, rs = _dense_ref(kind, 1, p0.double(), g0.double(), tuple(s.double() for s in _slots0(kind, p0)))
    _w_close(outs[0][0], rp)
    for got, r in zip(outs[0][1:], rs):
        _s_close(got, r)
    for out in outs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(out, outs[0]))


@pytest.mark.parametrize('kind', KINDS)
def test_multi_tensor_launch_equals_single_launches(dev, kind):
    """33 tensors of 1 .. 33 elements (one past the 32-tensor chunk) in one call against 33 dense calls: bit for bit, and
    the call advances the step counter once"""
    from deeptables_amd._lib import check, lib, ptr
    g = torch.Generator().manual_seed(2)
    ps = [torch.randn(k, generator=g) for k in range(1, 34)]
    gs = [torch.randn(k, generator=g) for k in range(1, 34)]

    def columns():
        cols = [[t.clone().to(dev) for t in ps], [t.to(dev) for t in gs]]
        return cols + [list(col) for col in zip(*[[s.to(dev) for s in _slots0(kind, t)] for t in ps])]
    one, many = columns(), columns()
    opt = _make(kind, [torch.nn.Parameter(torch.zeros(1, device=dev))])
    hp = opt._hpargs()
    state = opt._state_tensor(dev)
    dense = getattr(lib(), f'dt_{CFG[kind][0]}_dense_step')
    for step in range(2):
        for tensors in zip(*one):
            check(dense(*[ptr(x) for x in tensors], tensors[0].numel(), *hp, ptr(state), 0, None), kind)
        arr = ctypes.c_void_p * 33
        cols = [ctypes.cast(arr(*[t.data_ptr() for t in col]), ctypes.c_void_p) for col in many]
        ns = ctypes.cast((ctypes.c_int64 * 33)(*range(1, 34)), ctypes.c_void_p)
        check(getattr(lib(), f'dt_{CFG[kind][0]}_multi_step')(33, *cols, ns, *hp, ptr(state), 1, None), kind)
        assert opt.t == step + 1
    for k in range(33):
        for c in [0] + list(range(2, len(one))):
            assert torch.equal(one[c][k], many[c][k]), (k, c)
    assert not torch.equal(one[0][32].cpu(), ps[32])


# ---- rows ----------------------------------------------------------------------------------------------------------------
V = 50


def _lookups(g, n, D, F):
    """n lookups of a 50-row table in shuffled order: row 0 looked up 300 times (fewer where fewer positions exist), three
    rows twice, a few lookups skipped (-1).  F > 0: the [.., F] layout of a packed table — lookup i belongs to field i % F,
    whose rows are [12 f, 12 f + 12); the repeated rows are field 0's, which has n / F positions (250 at n = 1000: row 0
    takes 242 of them).  (The recipe of tests/test_optimizers_gpu.py.)"""
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
    steps each, with the `fields` hint 0 and 4.  The touched rows equal the float64 formula on the summed duplicates (for
    ftrl_reg the shrinkage reaches the touched rows only: the documented row-sparse behaviour); the other rows keep the
    table and every slot bit for bit."""
    from deeptables_amd.ops import SparseRowGrad
    g = torch.Generator().manual_seed(D)
    for F in (0, 4):
        for n in (1, 63, 64, 65, 1000):
            t0 = torch.randn(V, D, generator=g) * 0.05
            table = torch.nn.Parameter(t0.clone().to(dev))
            emb = _FakeEmb(table, F)
            opt = _make(kind, [table], [emb])
            names = opt.slot_names
            rp, rs = t0.double(), tuple(s.double() for s in _slots0(kind, t0))
            slots_before = [s.to(dev) for s in _slots0(kind, t0)]
            for t in range(1, 4):
                ids, vals = _lookups(g, n, D, F)
                before = table.detach().clone()
                emb.sparse_grads = {f'd{D}': [SparseRowGrad(ids.to(dev), vals.clone().to(dev))]}
                opt.step()
                assert opt.t == t
                rp, rs = R.rows_step(_ref_step(kind, t), rp, rs, ids, vals.double())
                touched = torch.zeros(V, dtype=torch.bool)
                touched[ids[ids >= 0]] = True
                what = (F, n, t)
                st = opt.state[id(table)]
                if len(names) == 2:                       # one [V, 2, D] record: two random locations per row
                    assert st['rec'].shape == (V, 2, D) and st[names[1]].data_ptr() == st[names[0]].data_ptr() + 4 * D
                _w_close(table[touched], rp[touched], what)
                assert torch.equal(table.detach()[~touched].cpu(), before[~touched].cpu()), what      # bit for bit
                for k, r, sb in zip(names, rs, slots_before):
                    assert torch.equal(st[k][~touched].cpu(), sb[~touched].cpu()), (what, k)
                    _s_close(st[k][touched], r[touched], (what, k))
                _l1_zeros(kind, table[touched], rs[-1][touched], what)
                slots_before = [st[k].clone() for k in names]
            for k, r in zip(names, rs):
                _s_close(opt.slot(table, k), r, (F, n, k))
            if 'slots' in opt.state[id(table)]:
                assert int(opt.state[id(table)]['slots'].abs().sum().item()) == 0     # the global hash is left empty


@pytest.mark.parametrize('kind', KINDS)
def test_pre_dense_hook_orders_table_updates_first(dev, kind):
    """the data-parallel strategy's hook (an all-reduce pending on the dense gradients): the table update is launched first,
    the hook runs, then the dense update advances the counter — the same bits as the step without a hook, whose dense
    update rides in the row launch's trailing blocks (now with two slots)"""
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
        out.append([table.detach().cpu().clone(), w.detach().cpu().clone()] +
                   [opt.slot(w, k).cpu().clone() for k in opt.slot_names] + [opt.slot(table, k).cpu().clone() for k in opt.slot_names])
    assert all(torch.equal(a, b) for a, b in zip(*out))
    # ... and the dense tensor is what the dense call alone makes of it
    ref = torch.nn.Parameter(w0.clone().to(dev))
    alone = _make(kind, [ref])
    for step in range(2):
        ref.grad = wg.to(dev)
        alone.step()
    assert torch.equal(ref.detach().cpu(), out[0][1])
    for i, k in enumerate(alone.slot_names):
        assert torch.equal(alone.slot(ref, k).cpu(), out[0][2 + i]), k
    assert not torch.equal(out[0][1], w0)


# ---- flat groups ---------------------------------------------------------------------------------------------------------
def _flat_group(dev, g):
    """three members — [4, 6] (24 elements), [5, 8] (40) as a strided view inside a zero-padded [5, 16] slab, [7] — in a flat
    buffer of 192 floats -> (flat_p, flat_g, members, twins, between)"""
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
    assert int(between.sum()) == n_flat - 71
    return flat_p, flat_g, members, twins, between


@pytest.mark.parametrize('kind', KINDS)
def test_flat_group_paths_equal_independent_tensors(dev, kind):
    """tests/test_optimizers_gpu.py's check of the same name for the new optimizers: a flat group registered once with
    grad_views=True against the same parameters held as independent tensors, two steps each of: the gradients ARE the flat
    views; the gradients are separate tensors (scattered); only the strided member has a gradient.  Parameters and slots are
    equal bit for bit after every step, and what lies between the members keeps exactly its initial value."""
    g = torch.Generator().manual_seed(11)
    flat_p, flat_g, members, twins, between = _flat_group(dev, g)
    params = [mb[0] for mb in members]
    assert not params[1].data.is_contiguous()
    opt, ref = _make(kind, params), _make(kind, twins)
    keys = opt.slot_names
    opt.register_flat_group(flat_p, flat_g, members, flat_p.numel(), grad_views=True)
    slot_init = [s.clone() for s in opt._flat[2:4] if s is not None]
    assert len(slot_init) == len(keys) and [float(s[0]) for s in slot_init] == [np.float32(v) for v in CFG[kind][3]]
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


@pytest.mark.parametrize('kind', KINDS)
def test_zero_pads_of_a_flat_group_stay_zero(dev, kind):
    """a strided member inside a zero-padded slab (a fused plan's narrow tower): three flat steps leave the pads exactly 0 and
    everything finite.  Ftrl runs with initial_accumulator_value = 0: on a pad n' = 0 and q = 0, where the kernel writes 0
    and Keras' formula NaN."""
    g = torch.Generator().manual_seed(12)
    flat_p, flat_g, members, twins, between = _flat_group(dev, g)
    params = [mb[0] for mb in members]
    opt = _make(kind, params, **({'initial_accumulator_value': 0.0} if kind.startswith('ftrl') else {}))
    opt.register_flat_group(flat_p, flat_g, members, flat_p.numel(), grad_views=True)
    start = flat_p.clone()
    for step in range(3):
        opt.zero_grad()
        for p in params:
            p.grad.copy_(torch.randn(p.shape, generator=g).to(dev))
        assert float(flat_g[between].abs().max()) == 0.0
        opt.step()
        assert float(flat_p[between].abs().max()) == 0.0, step
        assert bool(torch.isfinite(flat_p).all()), step
        for s in opt._flat[2:4]:
            assert s is None or (bool(torch.isfinite(s).all()) and float(s[between].abs().max()) == 0.0), step
    assert opt.t == 3 and not torch.equal(flat_p[~between], start[~between])


# ---- models --------------------------------------------------------------------------------------------------------------
SGDM_SPEC = {'class_name': 'SGD', 'config': {'momentum': 0.9, 'nesterov': True}}
MODEL_SPECS = {'ftrl': 'ftrl', 'adamax': 'adamax', 'sgdm': SGDM_SPEC}
MODEL_NAMES = {'ftrl': 'Ftrl', 'adamax': 'Adamax', 'sgdm': 'SGD'}


@pytest.mark.parametrize('which', ['adamax', 'ftrl', 'sgdm'])
def test_graphed_fit_replays_the_new_optimizers(dev, monkeypatch, which):
    """`fit(steps_per_execution=5)` captures the optimizer step with the rest and equals the eager fit after one epoch of 13
    steps — two replays of five and three eager steps.  Adamax: the replayed launches carry frozen host arguments, so this
    fails if beta_1^t were a host value."""
    from tests.test_compiled_gpu import _fit, _frame, _model
    from deeptables_amd.models import layers as L
    monkeypatch.setattr(L, 'DENSE_GRAD_MAX_ELEMS', 0)
    df, y = _frame(64 * 13 + 5)
    eager, graphed = _model('DeepFM', optimizer=MODEL_SPECS[which]), _model('DeepFM', optimizer=MODEL_SPECS[which])
    h0 = _fit(eager, df, y, 1, epochs=1)
    h1 = _fit(graphed, df, y, 5, epochs=1)
    assert eager.compiled_loop is None
    loop = graphed.compiled_loop
    assert loop is not None and loop.graph is not None and loop.k == 5 and not loop.chained
    assert eager.optimizer.t == graphed.optimizer.t == 13
    assert eager.optimizer._name == MODEL_NAMES[which]
    print(which, 'loss eager', h0.history['loss'], 'graphed', h1.history['loss'], 'max weight difference',
          max((p0 - p1).abs().max().item() for p0, p1 in zip(eager.model.parameters(), graphed.model.parameters())))
    assert np.allclose(h0.history['loss'], h1.history['loss'], atol=2e-6), (h0.history, h1.history)


@pytest.mark.parametrize('preset', ['WideDeep', 'DeepFM', 'xDeepFM', 'AutoInt', 'DCN', 'FGCNN', 'FiBiNet', 'PNN', 'AFM'])
def test_every_preset_trains_with_the_new_optimizers(dev, preset):
    """DeepTable's presets (deepnets.py) compile and train with optimizer='ftrl' / 'adamax' / momentum SGD in Keras'
    serialised form: two steps each, the loss and every weight stay finite, most tensors have moved and every tensor that
    moved has its slots"""
    from tests.test_fused_gpu import batch, build
    from deeptables_amd.models import deepnets
    F, Nd, D = 9, 4, (32 if preset == 'AutoInt' else 16)
    for which, spec in MODEL_SPECS.items():
        dm, cats = build(F, Nd, D, vocab=30, nets=getattr(deepnets, preset), optimizer=spec)
        dm.model.train()
        start = [p.detach().clone() for p in dm.optimizer.params]
        for step in range(2):
            idx, dense, y = batch(cats, Nd, 64, seed=step)
            loss, _ = dm.train_step([idx.int().to(dev), dense.to(dev)], y.to(dev))
            assert np.isfinite(float(loss))
        assert dm.optimizer.t == 2 and dm.optimizer._name == MODEL_NAMES[which]
        moved = [not torch.equal(p.detach(), s) for p, s in zip(dm.optimizer.params, start)]
        assert sum(moved) > len(moved) // 2 and all(bool(torch.isfinite(p).all()) for p in dm.optimizer.params), (preset, moved)
        assert all(dm.optimizer.slot(p, k) is not None for p, m in zip(dm.optimizer.params, moved) if m
                   for k in dm.optimizer.slot_names)


@pytest.mark.parametrize('which', ['ftrl', 'adamax', 'sgdm'])
@pytest.mark.parametrize('tower_mode', ['bf16x3', 'f32'])
def test_fused_forward_backward_with_a_separate_update(dev, monkeypatch, tower_mode, which):
    """DeepFM: the fused plan runs forward + backward and leaves the WHOLE update to optimizer.step() (no rows applied inside
    the step, no segments); three steps agree with the layer-by-layer path (DT_AMD_FUSED=0) to the bar of
    tests/test_optimizers_gpu.py's check of Adagrad."""
    from tests.test_fused_gpu import batch, build, rel
    from deeptables_amd.models import layers as L
    monkeypatch.setattr(L, 'DENSE_GRAD_MAX_ELEMS', 0)                    # row-sparse table: the rows kernel runs
    monkeypatch.setenv('DT_AMD_TOWER_DTYPE', tower_mode)
    F, Nd, D, B = 26, 13, 16, 256
    dm, cats = build(F, Nd, D, vocab=300, optimizer=MODEL_SPECS[which])
    monkeypatch.setenv('DT_AMD_FUSED', '0')
    twin, _ = build(F, Nd, D, vocab=300, optimizer=MODEL_SPECS[which])
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
        print(which, tower_mode, 'step', step, 'loss difference', abs(float(l1) - float(l2)))
        assert abs(float(l1) - float(l2)) < 2e-5, step
    assert len(seen) == 3 and all(f != -2 and s is None for f, s in seen)
    assert dm.optimizer.t == twin.optimizer.t == 3
    worst = max((rel(p1, p2), n1) for (n1, p1), (_, p2) in zip(dm.model.named_parameters(), twin.model.named_parameters()))
    print(which, tower_mode, 'largest relative difference', worst)
    for (n1, p1), (_, p2) in zip(dm.model.named_parameters(), twin.model.named_parameters()):
        assert rel(p1, p2) < (5e-4 if tower_mode == 'f32' else 3e-3), n1      # (test_fused_gpu.py's two bars)


CKPT_SPECS = {
    'ftrl': ({'class_name': 'Ftrl', 'config': {'l1_regularization_strength': 1e-4, 'beta': 0.05}}, 'ftrl'),
    'adamax': ({'class_name': 'Adamax', 'config': {'beta_1': 0.8, 'learning_rate': 2e-3}}, 'adamax'),
    'sgdm': (SGDM_SPEC, {'class_name': 'SGD', 'config': {'momentum': 0.5}}),
}


@pytest.mark.parametrize('which', ['ftrl', 'adamax', 'sgdm'])
def test_checkpoint_round_trip_with_the_slots(dev, tmp_path, monkeypatch, which):
    """two train steps, save(include_optimizer=True), load into a fresh model compiled with the same optimizer at OTHER
    hyperparameters: weights, slots (saved from a [V, 2, D] record for the table), step count and hyperparameters are the
    file's, bit for bit, and so are weights and slots after one more optimizer step on both.  That step is fed the SAME
    gradient bits on both sides, on a batch without repeated ids (tests/test_optimizers_gpu.py has the reasons)."""
    from tests.test_fused_gpu import batch, build
    from deeptables_amd.models import DeepModel
    from deeptables_amd.models import layers as L
    from deeptables_amd.ops import SparseRowGrad
    from safetensors import safe_open
    monkeypatch.setattr(L, 'DENSE_GRAD_MAX_ELEMS', 0)
    F, Nd, D = 6, 3, 16
    spec, other = CKPT_SPECS[which]
    dm, cats = build(F, Nd, D, vocab=80, optimizer=spec)
    dm.model.train()
    for step in range(2):
        idx, dense, y = batch(cats, Nd, 48, seed=step)
        dm.train_step([idx.int().to(dev), dense.to(dev)], y.to(dev))
    emb = dm.model.layers_by_name['emb_categorical_vars_all']
    table = emb.tables['d16']
    names = dm.optimizer.slot_names
    assert ('rec' in dm.optimizer.state[id(table)]) == (len(names) == 2)
    path = str(tmp_path / 'dm.safetensors')
    dm.save(path, include_optimizer=True)
    with safe_open(path, framework='pt', device='cpu') as f:
        keys = [k for k in f.keys() if k.startswith('optimizer/')]
        assert keys and {k.rsplit('/', 1)[1] for k in keys} == set(names)
        meta = f.metadata()
    assert meta['optimizer'] == dm.optimizer._name == MODEL_NAMES[which] and meta['optimizer_iterations'] == '2'
    from deeptables_amd import training
    assert training.make_optimizer(other, [], []).hyperparameters() != dm.optimizer.hyperparameters()
    dm2 = DeepModel('binary', 2, dm.config._replace(optimizer=other), dm.categorical_columns, dm.continuous_columns,
                    model_file=path)
    assert type(dm2.optimizer) is type(dm.optimizer) and dm2.optimizer.t == 2
    assert dm2.optimizer.hyperparameters() == dm.optimizer.hyperparameters()

    def same(tensors):
        for a, b in zip(tensors(dm.model), tensors(dm2.model)):
            assert torch.equal(a, b)
        for pa, pb in zip(dm.optimizer.params, dm2.optimizer.params):
            for k in names:
                sa, sb = dm.optimizer.slot(pa, k), dm2.optimizer.slot(pb, k)
                assert (sa is None) == (sb is None) and (sa is None or torch.equal(sa, sb.reshape(sa.shape))), k
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
    # a model compiled with another optimizer refuses the file's slots, and says why
    adam = DeepModel('binary', 2, dm.config._replace(optimizer='adam'), dm.categorical_columns, dm.continuous_columns)
    with pytest.raises(ValueError, match=dm.optimizer._name):
        adam._load_model(path)
    ada = DeepModel('binary', 2, dm.config._replace(optimizer='adagrad'), dm.categorical_columns, dm.continuous_columns)
    with pytest.raises(ValueError, match=dm.optimizer._name):
        ada._load_model(path)
