# -*- coding:utf-8 -*-
"""GPU: keras.optimizers' `weight_decay` and `use_ema` / `ema_momentum` — csrc/optim_stages.hip (dt_decay_multi, dt_ema_multi,
dt_rows_stage_pre / _post, dt_ema_rows_materialize, the stage's device step count) and the stages around `step()` of the eight
optimizer classes, against tests/decay_ema_reference.py.

Bars: the decay and the one-step average are compared bit for bit with the float32 restatements (the kernels evaluate the
stated operations in the stated order without contraction).  The lazy average of a row-sparse table and the AdamW run are
compared with float64 within W_BAR = 2e-6, tests/test_optimizers2_gpu.py's bar for weights of this scale (|w| < 1: a few
dozen float32 roundings of 6e-8 each).  Sparse gradients sit on a 2^-6 grid, |g| <= 4, so that any sum of them is exact in
float32 whatever its order."""
import ctypes

import numpy as np
import pytest
import torch

from tests import decay_ema_reference as R
from tests.test_optimizers2_gpu import W_BAR

pytestmark = pytest.mark.gpu

WD, LR, MOM = 0.004, 0.01, 0.9


def _h():
    from deeptables_amd import _lib
    return _lib, _lib.lib()


def _host(ptrs, ns):
    T = len(ns)
    cols = [ctypes.cast((ctypes.c_void_p * T)(*col), ctypes.c_void_p) for col in ptrs]
    return cols + [ctypes.cast((ctypes.c_int64 * T)(*ns), ctypes.c_void_p)]


def _values(rng, n):
    """weights of every size: O(1), a few tiny and huge ones, zeros of both signs"""
    x = rng.randn(n).astype(np.float32)
    x[rng.rand(n) < 0.05] *= np.float32(1e-20)        # (every product below stays a normal float32)
    x[rng.rand(n) < 0.05] *= np.float32(1e30)
    x[rng.rand(n) < 0.03] = 0.0
    x[rng.rand(n) < 0.03] = -0.0
    return x


def _same_bits(got, want, what=''):
    """float32 arrays, equal bit for bit up to the sign of a zero"""
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    want = np.asarray(want, dtype=np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), (what, float(np.abs(got.astype(np.float64) - want).max()))


class _Emb:
    """MultiColumnEmbedding as the optimizer sees it: one packed [V, D] table whose columns start at the rows `offs`"""

    def __init__(self, table, offs):
        key = f'd{table.shape[1]}'
        self.tables = {key: table}
        self.groups = [(table.shape[1], list(range(len(offs))))]
        self.input_dims = [hi - lo for lo, hi in zip(offs, list(offs[1:]) + [table.shape[0]])]
        self.sparse_grads = {}
        setattr(self, f'row_offset_{key}', torch.tensor(offs, dtype=torch.int64, device=table.device))
        self.key = key


def _grid(rng, shape):
    g = rng.randint(-256, 257, shape).astype(np.float32) / 64.0
    g[rng.rand(*shape) < 0.1] = 0.0
    return g


# ---- 1. dense decay ----------------------------------------------------------------------------------------------------------
def test_dense_decay_is_the_float32_formula_bit_for_bit(dev):
    _lib, h = _h()
    rng = np.random.RandomState(1)
    sizes = [1, 3, 255, 256, 257, 3075]
    hosts = [_values(rng, n) for n in sizes] + [_values(rng, 3075)]
    bufs = [torch.from_numpy(x).to(dev) for x in hosts[:-1]]
    odd = torch.zeros(3075 + 1, device=dev)               # the same 3075 one float off 16-byte alignment: the scalar path
    odd[1:].copy_(torch.from_numpy(hosts[-1]))
    tensors = bufs + [odd[1:]]
    assert odd[1:].data_ptr() % 16 == 4
    _lib.check(h.dt_decay_multi(len(tensors), *_host([[t.data_ptr() for t in tensors]], [t.numel() for t in tensors]), WD, LR,
                                _lib.stream_ptr()), 'dt_decay_multi')
    for t, x in zip(tensors, hosts):
        _same_bits(t, R.decay32(x, WD, LR), t.numel())
    assert float(odd[0]) == 0.0
    assert not np.array_equal(R.decay32(hosts[5], WD, LR), hosts[5])
    # nothing to do, and the refusals
    assert h.dt_decay_multi(0, None, None, WD, LR, None) == 0
    assert h.dt_decay_multi(1, *_host([[tensors[0].data_ptr()]], [-1]), WD, LR, None) == -1
    assert h.dt_decay_multi(1, *_host([[tensors[0].data_ptr() + 2]], [1]), WD, LR, None) == -1
    assert h.dt_decay_multi(1, *_host([[tensors[0].data_ptr()]], [1]), -1.0, LR, None) == -1
    assert h.dt_decay_multi(1, *_host([[tensors[0].data_ptr()]], [1]), float('nan'), LR, None) == -1


def test_33_tensors_decay_in_one_step_and_the_excluded_ones_do_not(dev):
    """one past the 32-tensor chunk; plain SGD with a zero gradient moves nothing, so what is left is the decay"""
    from deeptables_amd import training as T
    rng = np.random.RandomState(2)
    hosts = [_values(rng, 1 + 37 * i % 300) for i in range(33)]
    params = [torch.nn.Parameter(torch.from_numpy(x).to(dev)) for x in hosts]
    opt = T.SGD(params, [], learning_rate=LR, weight_decay=WD)
    opt.exclude_from_weight_decay(var_list=[params[4], params[32]])
    for p in params:
        p.grad = torch.zeros_like(p)
    opt.step()
    for i, (p, x) in enumerate(zip(params, hosts)):
        if i in (4, 32):
            assert np.array_equal(p.detach().cpu().numpy().view(np.int32), x.view(np.int32)), i      # bitwise untouched
        else:
            _same_bits(p, R.decay32(x, WD, LR), i)
    with pytest.raises(ValueError, match='before the first step'):
        opt.exclude_from_weight_decay(var_list=[params[0]])


def test_one_column_of_a_table_with_a_dense_gradient_is_excluded_by_name(dev):
    """a packed table with a DENSE gradient follows the formula literally, on every row, one region per column"""
    from deeptables_amd import training as T
    rng = np.random.RandomState(5)
    V, D, offs = 30, 6, [0, 9, 20]
    w0, b0 = _values(rng, V * D).reshape(V, D), _values(rng, 5)
    table, bias = torch.nn.Parameter(torch.from_numpy(w0).to(dev)), torch.nn.Parameter(torch.from_numpy(b0).to(dev))
    opt = T.SGD([table, bias], [_Emb(table, offs)], learning_rate=LR, weight_decay=WD)
    opt.set_variable_names({'emb/embeddings_0': table.data[0:9], 'emb/embeddings_1': table.data[9:20],
                            'emb/embeddings_2': table.data[20:], 'dnn_dense_1/bias': bias.data})
    opt.exclude_from_weight_decay(var_names=['embeddings_1$', 'bias'])
    table.grad, bias.grad = torch.zeros_like(table), torch.zeros_like(bias)
    opt.step()
    got = table.detach().cpu().numpy()
    keep = np.zeros(V, dtype=bool)
    keep[9:20] = True
    _same_bits(got[~keep], R.decay32(w0, WD, LR)[~keep])
    assert np.array_equal(got[keep].view(np.int32), w0[keep].view(np.int32))
    assert np.array_equal(bias.detach().cpu().numpy().view(np.int32), b0.view(np.int32))


# ---- 2. row decay ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', [4, 6, 16, 1028])
def test_row_decay_touches_the_looked_up_rows_of_the_included_fields_only(dev, D):
    from tests.test_gradclip_gpu import _coalesce
    _lib, h = _h()
    rng = np.random.RandomState(D)
    V, n = (6, 8) if D == 1028 else (40, 96)
    offs = [0, 1, 3, 4] if V == 6 else [0, 7, 19, 30]                  # four fields; field 2 is excluded
    edges = offs + [V]
    ids = rng.randint(0, V, n).astype(np.int64)
    ids[[1, 5]] = -1
    ids[[2, 3]] = ids[0]                                               # duplicates
    ids[6] = edges[2]                                                  # the excluded field is looked up too
    w0 = _values(rng, V * D).reshape(V, D)
    table = torch.from_numpy(w0).to(dev)
    out_rows, _, count = _coalesce(torch.from_numpy(ids).to(dev), torch.zeros(n, D, device=dev), V)
    on = torch.tensor([1, 1, 0, 1], dtype=torch.int32, device=dev)
    offs_dev = torch.tensor(offs, dtype=torch.int64, device=dev)
    _lib.check(h.dt_rows_stage_pre(_lib.ptr(table), None, None, _lib.ptr(out_rows), n, D, V, _lib.ptr(offs_dev), _lib.ptr(on), 4,
                                   1, WD, LR, 0.0, None, _lib.stream_ptr()), 'dt_rows_stage_pre')
    looked = np.zeros(V, dtype=bool)
    looked[ids[ids >= 0]] = True
    field = np.searchsorted(np.asarray(edges), np.arange(V), side='right') - 1
    moves = looked & (field != 2)
    assert moves.any() and (looked & (field == 2)).any() and (~looked).any() and int(count.item()) == int(looked.sum())
    want = np.where(moves[:, None], R.decay32(w0, WD, LR), w0)
    got = table.cpu().numpy()
    _same_bits(got[moves], want[moves], D)
    assert np.array_equal(got[~moves].view(np.int32), w0[~moves].view(np.int32)), D      # bitwise untouched
    # every field on (no mask), and decay off: nothing moves
    table2 = torch.from_numpy(w0).to(dev)
    _lib.check(h.dt_rows_stage_pre(_lib.ptr(table2), None, None, _lib.ptr(out_rows), n, D, V, _lib.ptr(offs_dev), None, 4, 1, WD,
                                   LR, 0.0, None, _lib.stream_ptr()), 'dt_rows_stage_pre')
    _same_bits(table2.cpu().numpy()[looked], R.decay32(w0, WD, LR)[looked], D)
    assert np.array_equal(table2.cpu().numpy()[~looked].view(np.int32), w0[~looked].view(np.int32)), D


# ---- 3. dense average --------------------------------------------------------------------------------------------------------
def test_dense_average_three_steps_bit_for_bit(dev):
    from deeptables_amd import training as T
    rng = np.random.RandomState(3)
    sizes = [1, 3, 255, 256, 257, 3075]
    params = [torch.nn.Parameter(torch.from_numpy(rng.randn(n).astype(np.float32)).to(dev)) for n in sizes]
    opt = T.SGD(params, [], learning_rate=0.1, use_ema=True, ema_momentum=MOM)
    assert opt.average(params[0]) is None and opt.stage_t == 0
    avg = [None] * len(params)
    for t in (1, 2, 3):
        for p in params:
            p.grad = torch.from_numpy(rng.randn(p.numel()).astype(np.float32)).to(dev)
        opt.step()
        assert opt.stage_t == t
        for i, p in enumerate(params):
            w = p.detach().cpu().numpy()
            avg[i] = R.ema32(np.zeros_like(w) if avg[i] is None else avg[i], w, MOM, t)
            _same_bits(opt.average(p), avg[i], (t, sizes[i]))
            if t == 1:
                assert torch.equal(opt.average(p), p.detach())          # the first step copies the weights
            else:
                assert not torch.equal(opt.average(p), p.detach())
    # pointers one float off 16-byte alignment: the scalar path gives the same bits
    _lib, h = _h()
    w, a = rng.randn(3075).astype(np.float32), rng.randn(3075).astype(np.float32)
    wb, ab = torch.zeros(3076, device=dev), torch.zeros(3076, device=dev)
    wb[1:].copy_(torch.from_numpy(w))
    ab[1:].copy_(torch.from_numpy(a))
    _lib.check(h.dt_ema_multi(1, *_host([[wb[1:].data_ptr()], [ab[1:].data_ptr()]], [3075]), MOM, _lib.ptr(opt._stage_dev),
                              _lib.stream_ptr()), 'dt_ema_multi')
    _same_bits(ab[1:], R.ema32(a, w, MOM, 4), 'misaligned')
    assert float(ab[0]) == 0.0 and np.array_equal(wb[1:].cpu().numpy(), w)


# ---- 4. the lazy average of a row-sparse table -------------------------------------------------------------------------------
# step (1-based) -> rows looked up.  Row 0: every step (sits out 0); row 1: every other step (1); row 2: steps 1 and 10 (8: the
# repeated multiplication's last case); row 3: steps 2 and 12 (9: the first powf); row 4: step 1 only, so 11 steps are
# pending when the average is asked for (its average met its weight at step 1: they must leave it there); rows 5 and 6: never
SCHEDULE = {t: [0] + ([1] if t % 2 else []) + ([2] if t in (1, 10) else []) + ([3] if t in (2, 12) else []) +
            ([4] if t == 1 else []) for t in range(1, 13)}


@pytest.mark.parametrize('D', [4, 6])
@pytest.mark.parametrize('decay', [None, WD])
def test_lazy_row_average_is_the_dense_average_of_the_recorded_weights(dev, D, decay):
    from deeptables_amd import training as T
    from deeptables_amd.ops import SparseRowGrad
    rng = np.random.RandomState(40 + D)
    V = 7
    w0 = (0.05 * rng.randn(V, D)).astype(np.float32)
    table = torch.nn.Parameter(torch.from_numpy(w0).to(dev))
    emb = _Emb(table, [0, 3])
    opt = T.SGD([table], [emb], learning_rate=LR, use_ema=True, ema_momentum=MOM, weight_decay=decay)
    trajectory = []
    for t in range(1, 13):
        rows = SCHEDULE[t] + [SCHEDULE[t][0], -1]                     # a duplicate and a skipped lookup
        ids = np.asarray(rows, dtype=np.int64)[rng.permutation(len(rows))]
        emb.sparse_grads[emb.key] = [SparseRowGrad(torch.from_numpy(ids).to(dev), torch.from_numpy(_grid(rng, (len(rows), D))).to(dev))]
        opt.step()
        trajectory.append(table.detach().cpu().numpy().astype(np.float64))
        assert opt.stage_t == t
        stamp = opt._stamps[id(table)].cpu().numpy()
        assert all(stamp[r] == t for r in SCHEDULE[t]) and stamp[5] == stamp[6] == 0
    assert np.array_equal(trajectory[-1][5:], w0[5:].astype(np.float64))                 # idle rows never moved
    want = R.ema_trajectory(trajectory, MOM)
    pending = opt._averages[id(table)].clone()
    got = opt.average(table)                                                              # materialises
    err = np.abs(got.cpu().numpy().astype(np.float64) - want).max(axis=1)
    print('D', D, 'decay', decay, 'largest error per row', err)
    assert float(err.max()) <= W_BAR, err
    assert not torch.equal(pending[2], got[2])                     # row 2's steps 11 and 12 were pending on its average
    assert torch.equal(pending[4], got[4])                         # (row 4's average met its weight at step 1: 11 steps of nothing)
    assert torch.equal(got[5:].cpu(), torch.from_numpy(w0[5:]))                           # never looked up: exactly the weight
    assert bool((opt._stamps[id(table)] == 12).all())
    # one column's average is a view of the table's
    assert torch.equal(opt.average(table.data[3:]), got[3:])
    opt.finalize_variable_values()
    assert torch.equal(table.detach(), got)


# ---- 5. the whole step -------------------------------------------------------------------------------------------------------
def _classes():
    from deeptables_amd import training as T
    return {'Adam': (T.KerasAdam, {}), 'SGD': (T.SGD, {}), 'MomentumSGD': (T.MomentumSGD, {}),
            'SGD(momentum)': (T.SGD, {'momentum': 0.9}), 'Adagrad': (T.Adagrad, {}), 'RMSprop': (T.RMSprop, {}),
            'Adamax': (T.Adamax, {}), 'Ftrl': (T.Ftrl, {})}


@pytest.mark.parametrize('clip', [None, 'clipvalue', 'global_clipnorm'])
@pytest.mark.parametrize('name', list(_classes()))
def test_a_step_is_the_decay_then_the_plain_step_then_the_average(dev, name, clip):
    """three steps: the weights and every slot equal, bit for bit, those of a twin without the arguments whose weights were
    decayed by the float32 restatement and which is given the same (clipped) gradients, the table's as coalesced rows"""
    from deeptables_amd.ops import SparseRowGrad
    cls, kw = _classes()[name]
    extra = {} if clip is None else {clip: 0.5}
    V, offs = 30, [0, 9, 20]
    for D in (4, 6):
        g = torch.Generator().manual_seed(D)
        rng = np.random.RandomState(50 + D)
        start = [torch.randn(5, generator=g), torch.randn(1027, generator=g), 0.05 * torch.randn(V, D, generator=g)]
        params = [torch.nn.Parameter(w.clone().to(dev)) for w in start]
        twins = [torch.nn.Parameter(w.clone().to(dev)) for w in start]
        emb, emb2 = _Emb(params[2], offs), _Emb(twins[2], offs)
        opt = cls(params, [emb], **dict(kw, weight_decay=WD, use_ema=True, ema_momentum=MOM, **extra))
        ref = cls(twins, [emb2], **kw)
        lr = float(opt.lr)
        seen = {}
        before = opt._stages_before

        def spy():
            ctx = before()
            seen['dense'] = [p.grad.detach().clone() for p in params[:2]]
            (sg,) = emb.sparse_grads[emb.key]
            seen['sparse'] = (sg.rows.clone(), sg.values.clone(), sg.fields)
            return ctx
        opt._stages_before = spy
        avg = [None, None]
        for step in (1, 2, 3):
            ids = rng.randint(0, V, 37).astype(np.int64)
            ids[[3, 17]] = -1
            ids[[5, 6, 7]] = ids[4]
            dense = [torch.randn(w.shape, generator=g).to(dev) for w in start[:2]]
            for p, x in zip(params, dense):
                p.grad = x.clone()
            emb.sparse_grads[emb.key] = [SparseRowGrad(torch.from_numpy(ids[:20]).to(dev), torch.from_numpy(_grid(rng, (20, D))).to(dev)),
                                         SparseRowGrad(torch.from_numpy(ids[20:]).to(dev), torch.from_numpy(_grid(rng, (17, D))).to(dev))]
            opt.step()
            what = (name, clip, D, step)
            rows_c, vals_c, fields = seen['sparse']
            assert fields == -1 and np.array_equal(rows_c.cpu().numpy()[:np.unique(ids[ids >= 0]).size], np.unique(ids[ids >= 0]))
            # the twin: decayed by the restatement, then its plain step
            looked = np.zeros(V, dtype=bool)
            looked[ids[ids >= 0]] = True
            for q in twins[:2]:
                q.data.copy_(torch.from_numpy(R.decay32(q.detach().cpu().numpy(), WD, lr)))
            w = twins[2].detach().cpu().numpy()
            twins[2].data.copy_(torch.from_numpy(np.where(looked[:, None], R.decay32(w, WD, lr), w)))
            for q, gq in zip(twins, seen['dense']):
                q.grad = gq.clone()
            emb2.sparse_grads[emb2.key] = [SparseRowGrad(rows_c.clone(), vals_c.clone(), fields=-1)]
            ref.step()
            for i, (p, q) in enumerate(zip(params, twins)):
                assert torch.equal(p.detach(), q.detach()), (what, i)
                for k in getattr(opt, 'slot_names', ()):
                    assert torch.equal(opt.state[id(p)][k], ref.state[id(q)][k]), (what, i, k)
            if hasattr(opt, 't'):
                assert opt.t == ref.t == step
            assert opt.stage_t == step and not emb.sparse_grads
            # the average behind the update
            for i, p in enumerate(params[:2]):
                wi = p.detach().cpu().numpy()
                avg[i] = R.ema32(np.zeros_like(wi) if avg[i] is None else avg[i], wi, MOM, step)
                _same_bits(opt.average(p), avg[i], (what, i))
        assert not torch.equal(params[2].detach().cpu(), start[2])


# ---- 6. flat groups ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['sgdm', 'adamax', 'ftrl'])
def test_zero_pads_of_a_flat_group_stay_zero_with_both_arguments(dev, kind):
    from tests.test_optimizers2_gpu import _flat_group, _make
    g = torch.Generator().manual_seed(12)
    flat_p, flat_g, members, twins, between = _flat_group(dev, g)
    params = [mb[0] for mb in members]
    opt = _make(kind, params, **dict({'initial_accumulator_value': 0.0} if kind.startswith('ftrl') else {}, weight_decay=0.1,
                                     use_ema=True, ema_momentum=MOM))
    opt.register_flat_group(flat_p, flat_g, members, flat_p.numel(), grad_views=True)
    start = flat_p.clone()
    for step in range(3):
        opt.zero_grad()
        for p in params:
            p.grad.copy_(torch.randn(p.shape, generator=g).to(dev))
        opt.step()
        flat_a = opt._averages['flat']
        assert float(flat_p[between].abs().max()) == 0.0 and float(flat_a[between].abs().max()) == 0.0, step
        assert bool(torch.isfinite(flat_p).all()) and bool(torch.isfinite(flat_a).all()), step
        for p in params:                                   # the members' averages are views of the one flat buffer
            a = opt.average(p)
            assert a.shape == p.shape and flat_a.data_ptr() <= a.data_ptr() < flat_a.data_ptr() + 4 * flat_a.numel()
            assert a.data_ptr() - flat_a.data_ptr() == p.data.data_ptr() - flat_p.data_ptr() and a.stride() == p.data.stride()
            if step == 0:
                assert torch.equal(a, p.detach())
    assert opt.t == 3 and opt.stage_t == 3 and not torch.equal(flat_p[~between], start[~between])
    assert not torch.equal(opt._averages['flat'], flat_p)


# ---- 7. through fit ----------------------------------------------------------------------------------------------------------
def _spec(**config):
    return {'class_name': 'Adam', 'config': config}


def test_no_fused_train_plan_with_either_argument_and_the_same_inference_plan(dev):
    from tests.test_compiled_gpu import _model
    plain = _model('DeepFM', optimizer='adam')
    for config in (dict(weight_decay=WD), dict(use_ema=True), dict(weight_decay=0.0)):
        dm = _model('DeepFM', optimizer=_spec(**config))
        assert dm.fused_plan() is None and not hasattr(dm, '_fused_plan')
        assert not dm.optimizer.supports_row_segments and not dm.optimizer.supports_rows_in_step
        assert type(dm.inference_plan()) is type(plain.inference_plan()) and dm.inference_plan() is not None
    assert plain.fused_plan() is not None


def test_fit_ends_on_the_averages_and_the_graphed_fit_replays_the_stages(dev, monkeypatch):
    """`fit(steps_per_execution=4)` over 13 steps equals the eager fit's loss history within 2e-6 (the bar of
    test_graphed_fit_replays_the_new_optimizers); after `fit` the weights ARE the averages — of both runs within the weight
    bar, which fails if a replayed launch took the stage's step count from the host"""
    from tests.test_compiled_gpu import _fit, _frame, _model
    from deeptables_amd.models import layers as L
    monkeypatch.setattr(L, 'DENSE_GRAD_MAX_ELEMS', 0)
    df, y = _frame(64 * 13 + 5)
    spec = _spec(weight_decay=WD, use_ema=True, ema_momentum=MOM)
    eager, graphed = _model('DeepFM', optimizer=spec), _model('DeepFM', optimizer=spec)
    h0 = _fit(eager, df, y, 1, epochs=1)
    h1 = _fit(graphed, df, y, 4, epochs=1)
    assert eager.compiled_loop is None and eager.fused_plan() is None and graphed.fused_plan() is None
    loop = graphed.compiled_loop
    assert loop is not None and loop.graph is not None and loop.k == 4
    print('loss eager', h0.history['loss'], 'graphed', h1.history['loss'])
    assert np.allclose(h0.history['loss'], h1.history['loss'], atol=2e-6), (h0.history, h1.history)
    for dm in (eager, graphed):
        assert dm.optimizer.t == dm.optimizer.stage_t == 13
        for p in dm.optimizer.params:
            a = dm.optimizer.average(p)
            assert a is not None and torch.equal(p.detach(), a)
    worst = 0.0
    for (n0, p0), (n1, p1) in zip(eager.model.named_parameters(), graphed.model.named_parameters()):
        worst = max(worst, float((p0.detach() - p1.detach()).abs().max()))
    print('largest difference of the averaged weights', worst)
    assert worst <= W_BAR


# ---- 8. checkpoint -----------------------------------------------------------------------------------------------------------
def _grid_step(dm, rng, dev):
    """one optimizer step on gradients of the 2^-6 grid: dense ones for every dense parameter, lookups with duplicates for the
    row-sparse table"""
    from deeptables_amd.ops import SparseRowGrad
    opt = dm.optimizer
    layer = opt.embedding_layers[0]
    (key, table), = layer.tables.items()
    opt.zero_grad()
    for p in opt.params:
        if p is table:
            continue
        x = torch.from_numpy(_grid(rng, tuple(p.shape)) / 64.0).to(dev)
        if p.grad is not None:
            p.grad.copy_(x)
        else:
            p.grad = x
    ids = rng.randint(0, table.shape[0], 40).astype(np.int64)
    ids[[5, 6]] = ids[4]
    layer.sparse_grads[key] = [SparseRowGrad(torch.from_numpy(ids).to(dev), torch.from_numpy(_grid(rng, (40, table.shape[1])) / 64.0).to(dev))]
    opt.step()
    return table


@pytest.mark.parametrize('class_name', ['Adam', 'SGD', 'RMSprop'])
def test_checkpoint_round_trip_continues_bit_for_bit(dev, tmp_path, monkeypatch, class_name):
    from tests.test_fused_gpu import build
    from deeptables_amd.models import DeepModel
    from deeptables_amd.models import layers as L
    monkeypatch.setattr(L, 'DENSE_GRAD_MAX_ELEMS', 0)
    spec = {'class_name': class_name, 'config': dict(weight_decay=WD, use_ema=True, ema_momentum=MOM, learning_rate=0.01)}
    dm, cats = build(6, 3, 16, vocab=80, optimizer=spec)
    dm.optimizer.exclude_from_weight_decay(var_names=['bias', 'embeddings_1$'])
    rng = np.random.RandomState(8)
    for _ in range(4):
        _grid_step(dm, rng, dev)
    path = str(tmp_path / f'{class_name}.safetensors')
    dm.save(path, include_optimizer=True)
    other = {'class_name': class_name, 'config': dict(learning_rate=0.01)}
    dm2 = DeepModel('binary', 2, dm.config._replace(optimizer=other), dm.categorical_columns, dm.continuous_columns,
                    model_file=path)
    o1, o2 = dm.optimizer, dm2.optimizer
    assert o2.hyperparameters() == o1.hyperparameters() and o2.stages and dm2.fused_plan() is None
    assert (o2.weight_decay, o2.use_ema, o2.ema_momentum, o2.stage_t) == (WD, True, MOM, 4)
    assert o2.decay_exclusions() == o1.decay_exclusions() == ['bias', 'embeddings_1$']
    state = rng.get_state()
    for run, d in enumerate((dm, dm2)):
        rng.set_state(state)
        for _ in range(3):
            _grid_step(d, rng, dev)
    t1 = o1.embedding_layers[0].tables['d16']
    t2 = o2.embedding_layers[0].tables['d16']
    assert torch.equal(o1._stamps[id(t1)], o2._stamps[id(t2)]) and int(o1._stamps[id(t1)].max()) == 7
    assert torch.equal(o1._averages[id(t1)], o2._averages[id(t2)])               # as they stand, with what is pending
    for p, q in zip(o1.params, o2.params):
        assert torch.equal(p.detach(), q.detach())
        assert torch.equal(o1.average(p), o2.average(q))
        for k in getattr(o1, 'slot_names', ()):
            assert torch.equal(o1.state[id(p)][k], o2.state[id(q)][k]), k
    assert o1.stage_t == o2.stage_t == 7
    assert not torch.equal(o1.average(t1), t1.detach())


# ---- 9. AdamW ----------------------------------------------------------------------------------------------------------------
def test_adam_with_weight_decay_is_adamw_through_the_model(dev, monkeypatch):
    """tiny DeepFM, {'class_name': 'Adam', 'config': {'weight_decay': 0.004}}, 5 train steps: every weight against the float64
    restatement fed the step's own gradients (decay with the plain learning rate, then Keras' Adam; the table's rows lazily, as
    KerasAdam updates them), within W_BAR"""
    from tests.test_fused_gpu import batch, build
    from deeptables_amd.models import layers as L
    monkeypatch.setattr(L, 'DENSE_GRAD_MAX_ELEMS', 0)
    dm, cats = build(6, 3, 16, vocab=80, optimizer={'class_name': 'Adam', 'config': {'weight_decay': 0.004}})
    opt = dm.optimizer
    assert dm.fused_plan() is None and opt.weight_decay == 0.004 and not opt.use_ema
    layer = opt.embedding_layers[0]
    table = layer.tables['d16']
    dense = [p for p in opt.params if p is not table]
    ref = {id(p): [p.detach().cpu().numpy().astype(np.float64)] for p in opt.params}
    for r in ref.values():
        r += [np.zeros_like(r[0]), np.zeros_like(r[0])]
    plain = {id(p): [x.copy() for x in ref[id(p)]] for p in dense}         # the same replay without the decay
    seen = {}
    before = opt._stages_before

    def spy():
        ctx = before()
        seen['dense'] = {id(p): p.grad.detach().cpu().numpy().astype(np.float64) for p in dense if p.grad is not None}
        (sg,) = layer.sparse_grads['d16']
        seen['sparse'] = (sg.rows.cpu().numpy(), sg.values.cpu().numpy().astype(np.float64))
        return ctx
    opt._stages_before = spy
    dm.model.train()
    for t in range(1, 6):
        idx, x, y = batch(cats, 3, 48, seed=t)
        dm.train_step([idx.int().to(dev), x.to(dev)], y.to(dev))
        for p in dense:
            if id(p) in seen['dense']:
                w, m, v = ref[id(p)]
                ref[id(p)] = list(R.adam_step(R.decay(w, 0.004, 1e-3), seen['dense'][id(p)], m, v, t))
                plain[id(p)] = list(R.adam_step(plain[id(p)][0], seen['dense'][id(p)], *plain[id(p)][1:], t))
        rows, vals = seen['sparse']
        w, m, v = ref[id(table)]
        k = int((rows >= 0).sum())
        r = rows[:k]
        w[r], m[r], v[r] = R.adam_step(R.decay(w[r], 0.004, 1e-3), vals[:k], m[r], v[r], t)
    assert opt.t == 5
    worst = 0.0
    for p in opt.params:
        err = float(np.abs(p.detach().cpu().numpy().astype(np.float64) - ref[id(p)][0]).max())
        worst = max(worst, err)
        assert err <= W_BAR, (tuple(p.shape), err)
    # the decay is visible at this bar: the same replay without it is elsewhere
    off = max(float(np.abs(p.detach().cpu().numpy().astype(np.float64) - plain[id(p)][0]).max()) for p in dense)
    print('largest |weight - float64 AdamW|', worst, '; against plain Adam', off)
    assert off > W_BAR
