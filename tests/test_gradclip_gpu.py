# -*- coding:utf-8 -*-
"""GPU: gradient clipping — csrc/gradclip.hip (dt_rows_coalesce, dt_grad_sumsq, dt_rows_field_sumsq, dt_grad_clip,
dt_rows_clip) and `clipnorm` / `clipvalue` / `global_clipnorm` of the seven optimizer classes against the float64 restatement
in tests/gradclip_reference.py.

Bars, with u = 2^-24:
  * a coalesced row's sum: (m - 1) u sum|v| over its m lookups — the bound of any float32 summation order;
  * sum of squares: n 2^-53 relative to numpy's float64 sum (squares are exact in float64, only the order differs);
  * clipvalue: bit-exact (no arithmetic);
  * clipnorm: 4 u relative per element — three float32 roundings (n_v, g c, the quotient);
  * global_clipnorm: 5 u relative per element — four roundings (N, 1 / N, c min(..), g s).
Where a check is about the clip and not about the coalesced sum, the sparse gradients sit on a 2^-6 grid, |g| <= 4: any sum
of up to 1000 of them is exact in float32 (tests/test_optimizers2_gpu.py does the same)."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import gradclip_reference as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
BAR = {'clipvalue': 0.0, 'clipnorm': 4 * U, 'global_clipnorm': 5 * U}


def _h():
    from deeptables_amd import _lib
    return _lib, _lib.lib()


def _mode(name):
    from deeptables_amd import _lib
    return {'clipvalue': _lib.DT_CLIP_VALUE, 'clipnorm': _lib.DT_CLIP_NORM, 'global_clipnorm': _lib.DT_CLIP_GLOBAL_NORM}[name]


def _close(got, ref, bar, what=''):
    """|got - ref| <= bar |ref| per element (NaN where the reference is NaN); bar 0: the float32 rounding of ref, bit for bit"""
    got = got.detach().cpu().numpy().astype(np.float64).reshape(-1)
    ref = np.asarray(ref, dtype=np.float64).reshape(-1)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), what
    if bar == 0.0:
        assert np.array_equal(got[~nan].astype(np.float32), ref[~nan].astype(np.float32)), what
        return 0.0
    err = np.abs(got[~nan] - ref[~nan])
    worst = float((err / np.maximum(np.abs(ref[~nan]), 1e-300)).max()) if err.size else 0.0
    assert bool((err <= bar * np.abs(ref[~nan])).all()), (what, worst / U)
    return worst


# ---- coalesce ----------------------------------------------------------------------------------------------------------------
def _coalesce(rows, vals, V):
    _lib, h = _h()
    n, D = rows.numel(), vals.shape[1]
    dev = rows.device
    out_rows = torch.full((max(n, 1),), -7, dtype=torch.int64, device=dev)[:n]
    out_vals = torch.full((max(n, 1), D), float('nan'), device=dev)[:n]
    count = torch.full((1,), -7, dtype=torch.int64, device=dev)
    ws = torch.empty(int(h.dt_rows_coalesce_workspace_bytes(n, D)), dtype=torch.uint8, device=dev)
    _lib.check(h.dt_rows_coalesce(_lib.ptr(rows), _lib.ptr(vals), n, D, V, _lib.ptr(out_rows), _lib.ptr(out_vals), _lib.ptr(count),
                                  _lib.ptr(ws), _lib.stream_ptr()), 'dt_rows_coalesce')
    return out_rows, out_vals, count


def _patterns(n, rng):
    """name -> (ids int64 [n], V)"""
    top = (1 << 31) + 5
    hot = rng.permutation(n).astype(np.int64) + 10
    hot[rng.permutation(n)[:(n + 1) // 2]] = 3                    # one row holds half of the lookups, the others are distinct
    gaps = rng.randint(0, max(n // 3, 1), n).astype(np.int64)
    gaps[::3] = -1
    return {
        'distinct': (rng.permutation(n).astype(np.int64), n + 3),
        'one row': (np.full(n, 7, dtype=np.int64), 8),
        'hot row': (hot, n + 10),
        'skipped interleaved': (gaps, max(n // 3, 1)),
        'all skipped': (np.full(n, -1, dtype=np.int64), 5),
        'top digit': (top - 4 + rng.randint(0, 9, n).astype(np.int64), (1 << 32) - 1),
    }


@pytest.mark.parametrize('D', [1, 4, 6, 16, 301])
def test_coalesce_sums_duplicates_in_a_fixed_order(dev, D):
    _lib, h = _h()
    T = h.dt_metric_sort_tile()
    rng = np.random.RandomState(D)
    worst = 0.0
    for n in (1, 2, 63, 64, 65, T - 1, T, T + 1, 3 * T + 7):
        vals_h = rng.randn(n, D).astype(np.float32)
        vals = torch.from_numpy(vals_h).to(dev)
        for name, (ids, V) in _patterns(n, rng).items():
            rows = torch.from_numpy(ids).to(dev)
            out_rows, out_vals, count = _coalesce(rows, vals, V)
            again = _coalesce(rows.clone(), vals.clone(), V)
            what = (name, n, D)
            assert torch.equal(rows.cpu(), torch.from_numpy(ids)) and torch.equal(vals.cpu(), torch.from_numpy(vals_h)), what
            ref_rows, ref_vals = R.coalesce(ids, vals_h)
            k = int((ref_rows >= 0).sum())
            assert int(count.item()) == k == np.unique(ids[ids >= 0]).size, what
            assert np.array_equal(out_rows.cpu().numpy(), ref_rows), what
            got = out_vals.cpu().numpy()
            assert not got[k:].any() and not np.signbit(got[k:]).any(), what          # the tail is exactly +0
            # (m - 1) u sum|v| per distinct row and column
            valid = ids >= 0
            _, inverse, m = np.unique(ids[valid], return_inverse=True, return_counts=True)
            mass = np.zeros((k, D))
            np.add.at(mass, inverse, np.abs(vals_h[valid].astype(np.float64)))
            err = np.abs(got[:k].astype(np.float64) - ref_vals[:k])
            bound = (m - 1)[:, None] * U * mass
            assert bool((err <= bound).all()), (what, float((err - bound).max()))
            if bound.any():
                worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
            assert all(torch.equal(a, b) for a, b in zip((out_rows, out_vals, count), again)), what     # the same bits
    print('D', D, 'largest error / bound', worst)


def test_coalesce_with_nothing_to_do_writes_the_count(dev):
    _lib, h = _h()
    count = torch.full((1,), -7, dtype=torch.int64, device=dev)
    _lib.check(h.dt_rows_coalesce(None, None, 0, 16, 50, None, None, _lib.ptr(count), None, _lib.stream_ptr()), 'dt_rows_coalesce')
    assert int(count.item()) == 0
    # an id outside [0, V) is a skipped lookup
    rows = torch.tensor([4, 50, 2, -3, 4, 1 << 40], dtype=torch.int64, device=dev)
    vals = torch.ones(6, 4, device=dev)
    out_rows, out_vals, count = _coalesce(rows, vals, 50)
    assert out_rows.tolist() == [2, 4, -1, -1, -1, -1] and int(count.item()) == 2
    assert out_vals[:, 0].tolist() == [1.0, 2.0, 0.0, 0.0, 0.0, 0.0]


# ---- sums and clips ------------------------------------------------------------------------------------------------------------
SIZES = (1, 3, 255, 256, 257, 4 * 256 * 3 + 3)


def _magnitudes(rng, n, lo, hi):
    """exact zeros (one in eight), or magnitudes log-uniform in [lo, hi] with a random sign"""
    x = np.exp(rng.uniform(np.log(lo), np.log(hi), n)) * rng.choice([-1.0, 1.0], n)
    x[rng.rand(n) < 0.125] = 0.0
    return x.astype(np.float32)


def _tensors(dev, seed=0):
    """33 tensors, every size of SIZES at least five times (two launches of 32 and 1): (host arrays, device tensors).  Every
    third tensor is small throughout (its norm is below 1), tensor 4 is all zeros, tensor 7 an unaligned view"""
    rng = np.random.RandomState(seed)
    host = []
    for t in range(33):
        n = SIZES[t % len(SIZES)]
        x = _magnitudes(rng, n, 1e-6, 1e-4) if t % 3 == 0 else _magnitudes(rng, n, 1e-6, 1e3)
        host.append(np.zeros(n, dtype=np.float32) if t == 4 else x)
    device = [torch.from_numpy(x).to(dev) for x in host]
    pad = torch.zeros(host[7].size + 1, device=dev)
    pad[1:].copy_(device[7])
    device[7] = pad[1:]
    assert device[7].data_ptr() % 16 == 4
    return host, device


def _arrays(tensors):
    T = len(tensors)
    gs = ctypes.cast((ctypes.c_void_p * T)(*[t.data_ptr() for t in tensors]), ctypes.c_void_p)
    ns = ctypes.cast((ctypes.c_int64 * T)(*[t.numel() for t in tensors]), ctypes.c_void_p)
    idx = ctypes.cast((ctypes.c_int * T)(*range(T)), ctypes.c_void_p)
    return gs, ns, idx


def _sumsq(tensors):
    _lib, h = _h()
    T, dev = len(tensors), tensors[0].device
    gs, ns, _ = _arrays(tensors)
    sums = torch.full((T,), float('nan'), dtype=torch.float64, device=dev)
    ws = torch.empty(int(h.dt_grad_sumsq_workspace_bytes(T, ns)) // 8, dtype=torch.float64, device=dev)
    _lib.check(h.dt_grad_sumsq(T, gs, ns, _lib.ptr(sums), _lib.ptr(ws), _lib.stream_ptr()), 'dt_grad_sumsq')
    return sums


def test_sum_of_squares_per_tensor(dev):
    host, device = _tensors(dev)
    got = _sumsq(device).cpu().numpy()
    again = _sumsq(device).cpu().numpy()
    for t, x in enumerate(host):
        ref = R.sumsq(x)
        assert abs(got[t] - ref) <= x.size * 2.0 ** -53 * ref, (t, x.size, got[t], ref)
    assert got[4] == 0.0 and np.array_equal(got, again)
    # one tensor, more than one chunk and not a multiple of four, against the same bar
    x = _magnitudes(np.random.RandomState(5), 3 * 4096 + 1027, 1e-6, 1e3)
    one = float(_sumsq([torch.from_numpy(x).to(dev)])[0])
    assert abs(one - R.sumsq(x)) <= x.size * 2.0 ** -53 * R.sumsq(x)


@pytest.mark.parametrize('D', [6, 16])
def test_sum_of_squares_per_field_of_a_coalesced_table(dev, D):
    """five fields over 1000 rows — one of a single row, one nobody looks up — at 3 T + 7 lookups, so that a field's range is
    cut into slices of more than one float4; against the float64 sum of the coalesced float32 values"""
    _lib, h = _h()
    n, Vt, offs = 3 * h.dt_metric_sort_tile() + 7, 1000, (0, 100, 101, 500, 900)
    rng = np.random.RandomState(D)
    ids = rng.randint(0, 500, n).astype(np.int64)                 # nothing at or above row 500 ...
    ids[rng.rand(n) < 0.3] = rng.randint(900, Vt)                 # ... but one row of the last field, often
    ids[::11] = -1
    vals = torch.from_numpy(_magnitudes(rng, n * D, 1e-6, 1e3).reshape(n, D)).to(dev)
    out_rows, out_vals, count = _coalesce(torch.from_numpy(ids).to(dev), vals, Vt)
    row_offset = torch.tensor(offs, dtype=torch.int64, device=dev)
    sums = torch.full((len(offs),), float('nan'), dtype=torch.float64, device=dev)
    ws = torch.empty(len(offs) * _lib.DT_FIELD_SUMSQ_PARTS, dtype=torch.float64, device=dev)
    for _ in range(2):
        _lib.check(h.dt_rows_field_sumsq(_lib.ptr(out_rows), _lib.ptr(out_vals), n, D, _lib.ptr(count), _lib.ptr(row_offset),
                                         len(offs), Vt, _lib.ptr(sums), _lib.ptr(ws), _lib.stream_ptr()), 'dt_rows_field_sumsq')
        got = sums.cpu().numpy()
        ref = R.field_sumsq(out_rows.cpu().numpy(), out_vals.cpu().numpy(), offs, Vt)
        rows_h = out_rows.cpu().numpy()
        edges = offs + (Vt,)
        for f, (g, r) in enumerate(zip(got, ref)):
            elems = int(((rows_h >= edges[f]) & (rows_h < edges[f + 1])).sum()) * D
            assert abs(g - r) <= elems * 2.0 ** -53 * r, (f, g, r, elems)
        assert got[3] == 0.0 and ref[3] == 0.0 and all(r > 0 for i, r in enumerate(ref) if i != 3)
        first = got if _ == 0 else first
    assert np.array_equal(first, got)


@pytest.mark.parametrize('mode', R.MODES)
def test_dense_clip_matches_the_formulas(dev, mode):
    _lib, h = _h()
    host, device = _tensors(dev, seed=1)
    if mode == 'clipvalue':
        host[2][1] = np.nan
        device[2][1] = float('nan')
    T = len(host)
    gs, ns, idx = _arrays(device)
    for c in ((1.0,) if mode != 'global_clipnorm' else (1.0, 1e6)):
        work = [t.clone() for t in device]
        pad = torch.zeros(host[7].size + 1, device=dev)
        pad[1:].copy_(device[7])
        work[7] = pad[1:]                                  # (still the unaligned one)
        gs, ns, idx = _arrays(work)
        sums = _sumsq(work) if mode != 'clipvalue' else None
        norm = torch.full((), float('nan'), dtype=torch.float64, device=dev)
        _lib.check(h.dt_grad_clip(_mode(mode), c, T, gs, ns, idx, _lib.ptr(sums), T if sums is not None else 0, _lib.ptr(norm),
                                  _lib.stream_ptr()), 'dt_grad_clip')
        ref = R.clip_variables(mode, c, host)
        worst = max(_close(g, r, BAR[mode], (mode, c, t)) for t, (g, r) in enumerate(zip(work, ref)))
        S = [R.sumsq(x) for x in host]
        if mode == 'clipvalue':
            assert float(norm) == 0.0
            assert any((np.abs(x[~np.isnan(x)]) > c).any() for x in host) and any((np.abs(x[~np.isnan(x)]) < c).all() for x in host)
        elif mode == 'clipnorm':
            norms = np.sqrt(S)
            assert (norms > c).any() and ((norms < c) & (norms > 0)).any() and (norms == 0).any()      # clipped, kept, zero
            assert all(torch.equal(w, d) for w, d, nv in zip(work, device, norms) if nv == 0)
        else:
            N = float(np.sqrt(np.sum(S)))
            assert (N > c) == (c == 1.0)                                                # both sides of c occur
            assert abs(float(norm) - N) <= 1e-12 * N
        print(mode, 'c', c, 'largest relative error / u', worst / U)


def test_global_clipnorm_with_a_non_finite_norm_makes_every_gradient_nan(dev):
    _lib, h = _h()
    a, b = torch.tensor([1.0, float('inf'), 0.0], device=dev), torch.tensor([2.0, 0.0], device=dev)
    gs, ns, idx = _arrays([a, b])
    sums = _sumsq([a, b])
    _lib.check(h.dt_grad_clip(_mode('global_clipnorm'), 1.0, 2, gs, ns, idx, _lib.ptr(sums), 2, None, _lib.stream_ptr()),
               'dt_grad_clip')
    assert bool(torch.isnan(a).all()) and bool(torch.isnan(b).all())
    z = torch.zeros(5, device=dev)                                                      # N = 0: unchanged
    gs, ns, idx = _arrays([z])
    sums = _sumsq([z])
    _lib.check(h.dt_grad_clip(_mode('global_clipnorm'), 1.0, 1, gs, ns, idx, _lib.ptr(sums), 1, None, _lib.stream_ptr()),
               'dt_grad_clip')
    assert z.tolist() == [0.0] * 5


# ---- one packed table, three fields ----------------------------------------------------------------------------------------
V, OFFS = 50, (0, 20, 35)


class _Emb:
    """MultiColumnEmbedding as the optimizer sees it: one packed [V, D] table of three columns"""

    def __init__(self, table):
        key = f'd{table.shape[1]}'
        self.tables = {key: table}
        self.groups = [(table.shape[1], [0, 1, 2])]
        self.sparse_grads = {}
        setattr(self, f'row_offset_{key}', torch.tensor(OFFS, dtype=torch.int64, device=table.device))
        self.key = key


def _lookups(rng, D, fields=(0, 2)):
    """37 lookups with duplicates and -1, in the given fields only; values on a 2^-6 grid, |g| <= 4"""
    edges = OFFS + (V,)
    ids = np.concatenate([rng.randint(edges[f], edges[f + 1], 37) for f in fields])[rng.permutation(37 * len(fields))[:37]]
    ids[[3, 17, 30]] = -1
    ids[[5, 6, 7]] = ids[4]
    vals = rng.randint(-256, 257, (37, D)).astype(np.float32) / 64.0
    vals[rng.rand(37, D) < 0.1] = 0.0
    return ids.astype(np.int64), vals


def _sparse_reference(mode, c, ids, vals, other_sums=()):
    """(out_rows, clipped out_vals float64, per-field sums) of one table; other_sums: the other variables' (global mode)"""
    out_rows, out_vals = R.coalesce(ids, vals)
    S = R.field_sumsq(out_rows, out_vals, OFFS, V)
    k = int((out_rows >= 0).sum())
    if mode == 'clipvalue':
        return out_rows, R.clip_value(out_vals, c), S
    if mode == 'clipnorm':
        per_row = np.ones(out_rows.size)
        per_row[:k] = np.asarray(S)[R.field_of(out_rows[:k], OFFS)]
        return out_rows, R.clip_norm(out_vals, per_row[:, None], c), S
    return out_rows, out_vals * R.global_scale(list(S) + list(other_sums), c)[1], S


@pytest.mark.parametrize('D', [4, 6])
def test_clipnorm_scales_each_field_of_a_packed_table_by_its_own_norm(dev, D):
    from deeptables_amd import training as T
    from deeptables_amd.ops import SparseRowGrad
    rng = np.random.RandomState(D)
    ids, vals = _lookups(rng, D)
    # field 0 small (kept), field 2 large (clipped), field 1 without a lookup
    vals[(ids >= 0) & (ids < OFFS[1])] /= 64.0
    c = 1.0
    out_rows, ref_vals, S = _sparse_reference('clipnorm', c, ids, vals)
    assert 0 < S[0] < c * c < S[2] and S[1] == 0.0
    # the row-sparse route
    table = torch.nn.Parameter(torch.zeros(V, D, device=dev))
    emb = _Emb(table)
    opt = T.SGD([table], [emb], clipnorm=c)
    emb.sparse_grads[emb.key] = [SparseRowGrad(torch.from_numpy(ids[:20]).to(dev), torch.from_numpy(vals[:20]).to(dev)),
                                 SparseRowGrad(torch.from_numpy(ids[20:]).to(dev), torch.from_numpy(vals[20:]).to(dev))]
    opt.clip_gradients()
    (g,) = emb.sparse_grads[emb.key]
    assert g.fields == -1 and g.segments is None and np.array_equal(g.rows.cpu().numpy(), out_rows)
    worst = _close(g.values, ref_vals, BAR['clipnorm'], 'sparse')
    k = int((out_rows >= 0).sum())
    small = out_rows[:k] < OFFS[1]
    assert np.array_equal(g.values.cpu().numpy()[:k][small], R.coalesce(ids, vals)[1][:k][small].astype(np.float32))   # g c / c
    # the dense-gradient route of the same table: the same gradient, densified
    dense = np.zeros((V, D), dtype=np.float32)
    dense[out_rows[:k]] = R.coalesce(ids, vals)[1][:k]
    emb.sparse_grads.clear()
    table.grad = torch.from_numpy(dense).to(dev)
    opt.clip_gradients()
    ref_dense = np.zeros((V, D))
    ref_dense[out_rows[:k]] = ref_vals[:k]
    worst = max(worst, _close(table.grad, ref_dense, BAR['clipnorm'], 'dense'))
    assert not table.grad[OFFS[1]:OFFS[2]].any()
    print('D', D, 'largest relative error / u', worst / U)


# ---- through the optimizers -------------------------------------------------------------------------------------------------
def _classes():
    from deeptables_amd import training as T
    return {'Adam': (T.KerasAdam, {}), 'SGD': (T.SGD, {}), 'MomentumSGD': (T.SGD, {'momentum': 0.9}), 'Adagrad': (T.Adagrad, {}),
            'RMSprop': (T.RMSprop, {}), 'Adamax': (T.Adamax, {}), 'Ftrl': (T.Ftrl, {})}


@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('name', ['Adam', 'SGD', 'MomentumSGD', 'Adagrad', 'RMSprop', 'Adamax', 'Ftrl'])
def test_clipped_step_is_the_clip_stage_then_the_unclipped_step(dev, name, mode):
    """three steps: (a) after the clip stage alone the gradients meet the bars of the kernel tests; (b) the step equals, bit
    for bit, the step of an unclipped twin given those clipped gradients (the table's as coalesced rows with fields = -1):
    weights, every slot and t"""
    from deeptables_amd.ops import SparseRowGrad
    cls, kw = _classes()[name]
    c = {'clipvalue': 0.5, 'clipnorm': 1.0, 'global_clipnorm': 1.0}[mode]
    for D in (4, 6):
        g = torch.Generator().manual_seed(D)
        rng = np.random.RandomState(100 + D)
        start = [torch.randn(5, generator=g), torch.randn(1027, generator=g), 0.05 * torch.randn(V, D, generator=g)]
        sides = []
        for clipped in (True, False):
            params = [torch.nn.Parameter(w.clone().to(dev)) for w in start]
            emb = _Emb(params[2])
            sides.append((params, emb, cls(params, [emb], **dict(kw, **({mode: c} if clipped else {})))))
        (params, emb, opt), (twins, emb2, ref) = sides
        assert type(opt) is type(ref) and opt._clip == (mode, c) and ref._clip is None
        seen = {}
        stage = opt.clip_gradients

        def spy():
            stage()
            seen['dense'] = [p.grad.detach().clone() for p in params[:2]]
            (sg,) = emb.sparse_grads[emb.key]
            seen['sparse'] = (sg.rows.clone(), sg.values.clone(), sg.fields)
        opt.clip_gradients = spy
        for step in range(3):
            scale = (3.0, 0.01, 1.0)[step]                 # above c, below c, in between
            dense = [(torch.randn(w.shape, generator=g) * scale).numpy() for w in start[:2]]
            ids, vals = _lookups(rng, D, fields=(0, 1, 2) if step == 1 else (0, 2))
            vals = (vals * (1.0 if step == 0 else 2.0 ** -6)).astype(np.float32)
            opt.zero_grad()
            ref.zero_grad()
            for p, x in zip(params, dense):
                p.grad = torch.from_numpy(x).to(dev)
            emb.sparse_grads[emb.key] = [SparseRowGrad(torch.from_numpy(ids).to(dev), torch.from_numpy(vals).to(dev))]
            opt.step()
            # (a)
            S_dense = [R.sumsq(x) for x in dense]
            out_rows, ref_vals, S_fields = _sparse_reference(mode, c, ids, vals, other_sums=S_dense)
            if mode == 'global_clipnorm':
                s = R.global_scale(S_dense + list(S_fields), c)[1]
                ref_dense = [x.astype(np.float64) * s for x in dense]
                N = float(np.sqrt(sum(S_dense) + sum(S_fields)))
                assert abs(float(opt.last_global_norm) - N) <= 1e-12 * N
            else:
                ref_dense = R.clip_variables(mode, c, dense)
            what = (name, mode, D, step)
            for got, want in zip(seen['dense'], ref_dense):
                _close(got, want, BAR[mode], what)
            rows_c, vals_c, fields = seen['sparse']
            assert fields == -1 and np.array_equal(rows_c.cpu().numpy(), out_rows), what
            _close(vals_c, ref_vals, BAR[mode], what)
            # (b)
            for q, gq in zip(twins, seen['dense']):
                q.grad = gq.clone()
            emb2.sparse_grads[emb2.key] = [SparseRowGrad(rows_c.clone(), vals_c.clone(), fields=-1)]
            ref.step()
            for i, (p, q) in enumerate(zip(params, twins)):
                assert torch.equal(p.detach(), q.detach()), (what, i)
                for k in getattr(opt, 'slot_names', ()):
                    assert torch.equal(opt.state[id(p)][k], ref.state[id(q)][k]), (what, i, k)
            if hasattr(opt, 't'):
                assert opt.t == ref.t == step + 1
            assert not emb.sparse_grads and not emb2.sparse_grads
        assert all(not torch.equal(p.detach().cpu(), w) for p, w in zip(params, start))


@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('kind', ['sgdm', 'sgdm_nesterov', 'adamax', 'ftrl', 'ftrl_reg', 'ftrl_pow'])
def test_zero_pads_of_a_flat_group_stay_zero_with_a_clip(dev, kind, mode):
    """tests/test_optimizers2_gpu.py's test_zero_pads_of_a_flat_group_stay_zero with each clip set: the members are clipped as
    regions of the flat gradient (the strided member with the pads its slab encloses), the pads have gradient 0 and stay 0"""
    from tests.test_optimizers2_gpu import _flat_group, _make
    g = torch.Generator().manual_seed(12)
    flat_p, flat_g, members, twins, between = _flat_group(dev, g)
    params = [mb[0] for mb in members]
    opt = _make(kind, params, **dict({'initial_accumulator_value': 0.0} if kind.startswith('ftrl') else {}, **{mode: 0.5}))
    opt.register_flat_group(flat_p, flat_g, members, flat_p.numel(), grad_views=True)
    start = flat_p.clone()
    for step in range(3):
        opt.zero_grad()
        grads = [torch.randn(p.shape, generator=g) for p in params]
        for p, x in zip(params, grads):
            p.grad.copy_(x.to(dev))
        assert float(flat_g[between].abs().max()) == 0.0
        opt.step()
        # the stage ran on the flat gradient: each member by its own norm / all by the global one
        want = R.clip_variables(mode, 0.5, [x.numpy() for x in grads])
        for p, w in zip(params, want):
            _close(opt._flat_grad_view(p), w, BAR[mode], (kind, mode, step))
        assert float(flat_g[between].abs().max()) == 0.0 and float(flat_p[between].abs().max()) == 0.0, step
        assert bool(torch.isfinite(flat_p).all()), step
        for s in opt._flat[2:4]:
            assert s is None or (bool(torch.isfinite(s).all()) and float(s[between].abs().max()) == 0.0), step
    assert opt.t == 3 and not torch.equal(flat_p[~between], start[~between])


# ---- through fit -------------------------------------------------------------------------------------------------------------
def _sgd(c):
    return {'class_name': 'SGD', 'config': {'learning_rate': 1.0, 'global_clipnorm': c}}


@pytest.mark.parametrize('c', [0.05, 1e9])
def test_one_sgd_step_moves_the_weights_by_the_clipped_norm(dev, monkeypatch, c):
    """plain SGD, learning rate 1: |delta theta| over ALL parameters is lr min(N, c), N the global norm the step reports"""
    from tests.test_compiled_gpu import _frame, _model
    from deeptables_amd import training
    from deeptables_amd.models import layers as L
    monkeypatch.setattr(L, 'DENSE_GRAD_MAX_ELEMS', 0)
    dm = _model('DeepFM', optimizer=_sgd(c))
    assert dm.fused_plan() is None and not hasattr(dm, '_fused_plan') and dm.optimizer.global_clipnorm == c
    df, y = _frame(64)
    feed = training.TableBatches(df, y, dm.categorical_columns, dm.continuous_columns, dm.device, dm.task, dm.num_classes)
    ins, yb = next(iter(feed.iterate(64, False, True)))
    dm.model.train()
    before = [p.detach().double().cpu() for p in dm.model.parameters()]
    dm.train_step(ins, yb)
    after = [p.detach().double().cpu() for p in dm.model.parameters()]
    moved = math.sqrt(sum(float(((a - b) ** 2).sum()) for a, b in zip(after, before)))
    theta = math.sqrt(sum(float((b ** 2).sum()) for b in before))
    N = float(dm.optimizer.last_global_norm)
    lr = 1.0
    tol = 2.0 ** -23 * theta + 8 * U * lr * min(c, N)
    print('c', c, 'N', N, '|delta theta|', moved, 'tolerance', tol)
    assert (N > c) == (c == 0.05) and N > 0
    assert abs(moved - lr * min(N, c)) <= tol, (moved, lr * min(N, c), tol)


def test_a_clip_that_never_bites_trains_like_the_unclipped_layer_by_layer_fit(dev, monkeypatch):
    from tests.test_compiled_gpu import _fit, _frame, _model
    from deeptables_amd.models import layers as L
    monkeypatch.setattr(L, 'DENSE_GRAD_MAX_ELEMS', 0)
    df, y = _frame(64 * 13 + 5)
    clipped = _model('DeepFM', optimizer={'class_name': 'Adam', 'config': {'clipvalue': 1e9}})
    h1 = _fit(clipped, df, y, 1, epochs=1)
    monkeypatch.setenv('DT_AMD_FUSED', '0')
    plain = _model('DeepFM', optimizer='adam')
    assert plain.fused_plan() is None and clipped.fused_plan() is None
    h0 = _fit(plain, df, y, 1, epochs=1)
    assert clipped.optimizer.t == plain.optimizer.t == 13
    print('loss clipped', h1.history['loss'], 'unclipped', h0.history['loss'])
    assert np.allclose(h0.history['loss'], h1.history['loss'], atol=2e-6), (h0.history, h1.history)


def test_graphed_fit_replays_the_clip_stage(dev, monkeypatch):
    """`fit(steps_per_execution=5)` over 13 steps — two replays of five and three eager steps — equals the eager fit: the
    replayed clip launches read their sums, counts and scale from device memory"""
    from tests.test_compiled_gpu import _fit, _frame, _model
    from deeptables_amd.models import layers as L
    monkeypatch.setattr(L, 'DENSE_GRAD_MAX_ELEMS', 0)
    df, y = _frame(64 * 13 + 5)
    spec = {'class_name': 'Adam', 'config': {'global_clipnorm': 0.05}}
    eager, graphed = _model('DeepFM', optimizer=spec), _model('DeepFM', optimizer=spec)
    h0 = _fit(eager, df, y, 1, epochs=1)
    h1 = _fit(graphed, df, y, 5, epochs=1)
    assert eager.compiled_loop is None and eager.fused_plan() is None and graphed.fused_plan() is None
    loop = graphed.compiled_loop
    assert loop is not None and loop.graph is not None and loop.k == 5 and not loop.chained
    assert eager.optimizer.t == graphed.optimizer.t == 13
    n0, n1 = float(eager.optimizer.last_global_norm), float(graphed.optimizer.last_global_norm)
    print('loss eager', h0.history['loss'], 'graphed', h1.history['loss'], 'last global norm', n0, n1)
    assert n0 > 0.05                                                                  # the clip was biting
    assert np.allclose(h0.history['loss'], h1.history['loss'], atol=2e-6), (h0.history, h1.history)


def test_checkpoint_round_trip_restores_the_clip_setting(dev, tmp_path, monkeypatch):
    from tests.test_fused_gpu import batch, build
    from deeptables_amd.models import DeepModel
    from deeptables_amd.models import layers as L
    monkeypatch.setattr(L, 'DENSE_GRAD_MAX_ELEMS', 0)
    for spec, other in (({'class_name': 'Adam', 'config': {'clipnorm': 0.5}}, 'adam'),
                        ({'class_name': 'Adagrad', 'config': {'global_clipnorm': 0.25}},
                         {'class_name': 'Adagrad', 'config': {'clipvalue': 3.0}})):
        dm, cats = build(6, 3, 16, vocab=80, optimizer=spec)
        dm.model.train()
        idx, dense, y = batch(cats, 3, 48, seed=0)
        dm.train_step([idx.int().to(dev), dense.to(dev)], y.to(dev))
        path = str(tmp_path / f"{spec['class_name']}.safetensors")
        dm.save(path, include_optimizer=True)
        dm2 = DeepModel('binary', 2, dm.config._replace(optimizer=other), dm.categorical_columns, dm.continuous_columns,
                        model_file=path)
        assert dm2.optimizer._clip == dm.optimizer._clip is not None and dm2.optimizer.t == 1
        assert dm2.optimizer.hyperparameters() == dm.optimizer.hyperparameters()
        assert dm2.fused_plan() is None
