# -*- coding:utf-8 -*-
"""GPU: the Keras L1 / L2 regularizers — csrc/regularizer.hip (dt_reg_penalty, dt_reg_grad) against the float64 restatement
of tests/regularizer_reference.py, ops.regularization_penalty through autograd, and the five knobs of the reference
(`embeddings_regularizer`, `embeddings_activity_regularizer`, dnn_params' `kernel_regularizer` / `activity_regularizer`,
afm_params' `kernel_regularizer`) through train_step, fit, evaluate, predict, checkpoints and the data-parallel step.

Model level: model A has no regularizer, model B carries the ones under test, both start from the same weights; the graph
is tiny (three categorical columns with vocabularies 7, 9 and 11, D = 4, one continuous column, tower 8 -> 4, batch 16) and
every column has a row no sample of the batch looks up."""
import ctypes
import math
import os
import socket

import numpy as np
import pytest
import torch

from tests import precision as P
from tests import regularizer_reference as RR

pytestmark = pytest.mark.gpu

U24, U23 = 2.0 ** -24, 2.0 ** -23


# ===========================================================================================================================
# kernels
# ===========================================================================================================================
def _chunk():
    from deeptables_amd import _lib
    return int(_lib.lib().dt_reg_chunk())


def _lengths():
    c = _chunk()
    return [1, 3, 4, 5, 255, 256, 257, c - 1, c, c + 1, 2 * c + 5]


def _values(n, seed):
    """float32 [n]: normal values with +0.0, -0.0, a negative and an exact power of two planted (as many as fit)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g)
    for pos, v in zip(range(n - 1, -1, -1), (0.0, -0.0, -1.75, 0.5)):
        x[pos] = v
    return x


def _on(dev, x, offset):
    """x on the device, as a fresh tensor or as a view one float into a larger one (not 16-byte aligned)"""
    if not offset:
        t = x.to(dev)
        assert t.data_ptr() % 16 == 0
        return t
    buf = torch.empty(x.numel() + 1, dtype=torch.float32, device=dev)
    t = buf[1:]
    t.copy_(x)
    assert t.data_ptr() % 16 == 4
    return t


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _check_penalty(p64, p32, ref):
    p64, p32 = float(p64), float(p32)
    print(f'penalty: f64 {p64!r} f32 {p32!r} ref {ref!r} rel32 {abs(p32 - ref) / max(abs(ref), 1e-300):.3e}')
    assert abs(p64 - ref) <= 1e-12 * abs(ref), (p64, ref)
    assert abs(p32 - ref) <= U23 * abs(ref), (p32, ref)           # one float32 rounding of a double-accumulated sum


COEFFS = [(0.01, 0.0), (0.0, 0.01), (1e-3, 2.5e-4)]             # l1 only, l2 only, both


@pytest.mark.parametrize('l1,l2', COEFFS)
@pytest.mark.parametrize('offset', [False, True])
def test_single_tensor_penalty_and_gradient(dev, l1, l2, offset):
    from deeptables_amd import ops
    for k, n in enumerate(_lengths()):
        x = _values(n, seed=100 + k)
        xd = _on(dev, x, offset)
        p64, p32 = ops.reg_penalty_raw([xd], [(l1, l2)])
        _check_penalty(p64, p32, RR.penalty(x.numpy(), l1, l2))
        q64, q32 = ops.reg_penalty_raw([xd], [(l1, l2)])           # determinism: the same bits again
        assert _bits(p64.reshape(1).view(torch.float32)).equal(_bits(q64.reshape(1).view(torch.float32)))
        assert _bits(p32.reshape(1)).equal(_bits(q32.reshape(1)))
        for go in (1.0, 0.5):
            god = torch.tensor([go], dtype=torch.float32, device=dev)
            want = torch.from_numpy(RR.grad_f32(x.numpy(), l1, l2, go))
            out = _on(dev, torch.full((n,), 7.0), offset)            # the float4 body needs both pointers at the same phase
            ops.reg_grad_raw([xd], [out], [(l1, l2)], god)
            assert _bits(out).equal(_bits(want)), (n, go, 'write')
            mixed = torch.full((n,), 7.0, device=dev) if offset else _on(dev, torch.full((n,), 7.0), True)
            ops.reg_grad_raw([xd], [mixed], [(l1, l2)], god)         # pointers that disagree: the scalar route, same bits
            assert _bits(mixed).equal(_bits(want)), (n, go, 'mixed alignment')
            g0 = torch.randn(n, generator=torch.Generator().manual_seed(7 + k))
            acc = _on(dev, g0, offset)
            ops.reg_grad_raw([xd], [acc], [(l1, l2)], god, accumulate=True)
            assert _bits(acc).equal(_bits(torch.from_numpy(RR.grad_f32(x.numpy(), l1, l2, go, into=g0.numpy())))), (n, go, 'acc')
            again = _on(dev, torch.zeros(n), offset)
            ops.reg_grad_raw([xd], [again], [(l1, l2)], god)
            assert _bits(again).equal(_bits(out))
        # the sign of zero is zero: with l1 alone both zeros get an exact zero
        if l2 == 0.0 and n >= 2:
            assert out[n - 1].item() == 0.0 and out[n - 2].item() == 0.0


@pytest.mark.parametrize('count', [1, 32, 33])
def test_many_tensors_in_one_call_equal_single_calls(dev, count):
    """1, 32 and 33 tensors cross the descriptor-chunk boundary; mixed lengths and coefficients, one empty member, every
    third tensor an unaligned view"""
    from deeptables_amd import ops
    c = _chunk()
    pool = [5, 257, c + 1, 3, 2 * c + 5, 64, c - 1, 1, c]
    xs, cf, host = [], [], []
    for t in range(count):
        n = 0 if t == 1 else pool[t % len(pool)]
        x = _values(n, seed=300 + t) if n else torch.empty(0)
        host.append(x)
        xs.append(_on(dev, x, offset=(t % 3 == 2)) if n else torch.empty(0, device=dev))
        cf.append(COEFFS[t % 3] if t % 4 else (2e-3 * (t + 1), 1e-3))
    p64, p32 = ops.reg_penalty_raw(xs, cf)
    singles = [ops.reg_penalty_raw([x], [k])[0].item() for x, k in zip(xs, cf)]
    total = math.fsum(singles)
    ref = RR.total_penalty([h.numpy() for h in host], cf)
    _check_penalty(p64, p32, ref)
    assert abs(float(p32) - total) <= U23 * abs(total)
    if count > 1:
        assert singles[1] == 0.0                                    # the n = 0 member contributes nothing
    q64, q32 = ops.reg_penalty_raw(xs, cf)
    assert p64.item() == q64.item() and _bits(p32.reshape(1)).equal(_bits(q32.reshape(1)))
    for go, accumulate in ((1.0, False), (0.5, False), (0.5, True)):
        god = torch.tensor([go], dtype=torch.float32, device=dev)
        start = [torch.randn(x.numel(), generator=torch.Generator().manual_seed(9 + i)) for i, x in enumerate(xs)]
        outs = [_on(dev, s, offset=(i % 3 == 2)) if s.numel() else torch.empty(0, device=dev) for i, s in enumerate(start)]
        ops.reg_grad_raw(xs, outs, cf, god, accumulate=accumulate)
        for i, (x, o, k, s, h) in enumerate(zip(xs, outs, cf, start, host)):
            if not x.numel():
                continue
            one = _on(dev, s, offset=(i % 3 == 2))
            ops.reg_grad_raw([x], [one], [k], god, accumulate=accumulate)
            assert _bits(o).equal(_bits(one)), (i, go, accumulate)
            want = RR.grad_f32(h.numpy(), k[0], k[1], go, into=s.numpy() if accumulate else None)
            assert _bits(o).equal(_bits(torch.from_numpy(want))), (i, go, accumulate)


def test_nan_and_inf_propagate(dev):
    from deeptables_amd import ops
    god = torch.ones(1, device=dev)
    x = torch.tensor([1.0, float('nan'), -2.0, 3.0, 0.5], device=dev)
    p64, p32 = ops.reg_penalty_raw([x], [(0.01, 0.01)])
    assert math.isnan(p64.item()) and math.isnan(p32.item())
    out = torch.zeros(5, device=dev)
    ops.reg_grad_raw([x], [out], [(0.01, 0.01)], god)
    assert math.isnan(out[1].item()) and bool(torch.isfinite(out[[0, 2, 3, 4]]).all())
    y = torch.tensor([1.0, float('inf'), -2.0], device=dev)
    assert ops.reg_penalty_raw([y], [(0.0, 0.01)])[1].item() == float('inf')
    assert ops.reg_penalty_raw([-y], [(0.01, 0.0)])[0].item() == float('inf')
    ops.reg_grad_raw([-y], [out[:3]], [(0.01, 0.01)], god)
    assert out[1].item() == float('-inf')


def test_argument_errors_return_the_code_and_launch_nothing(dev):
    from deeptables_amd import _lib
    h = _lib.lib()
    x = torch.ones(8, device=dev)
    out = torch.full((8,), 5.0, device=dev)
    tot = torch.full((2,), 5.0, dtype=torch.float64, device=dev)
    ws = torch.zeros(4, dtype=torch.float64, device=dev)
    go = torch.ones(1, device=dev)
    px, po, null = (ctypes.c_void_p * 1)(x.data_ptr()), (ctypes.c_void_p * 1)(out.data_ptr()), (ctypes.c_void_p * 1)(None)
    n8, neg = (ctypes.c_int64 * 1)(8), (ctypes.c_int64 * 1)(-8)
    d, f = (ctypes.c_double * 1)(0.5), (ctypes.c_float * 1)(0.5)
    P_ = lambda t: ctypes.c_void_p(t.data_ptr())
    st = _lib.stream_ptr()
    bad = [h.dt_reg_penalty(1, null, n8, d, d, P_(ws), P_(tot), P_(tot[1:]), st),
           h.dt_reg_penalty(1, px, neg, d, d, P_(ws), P_(tot), P_(tot[1:]), st),
           h.dt_reg_penalty(-1, px, n8, d, d, P_(ws), P_(tot), P_(tot[1:]), st),
           h.dt_reg_penalty(1, px, n8, d, d, None, P_(tot), P_(tot[1:]), st),
           h.dt_reg_grad(1, null, po, n8, f, f, P_(go), 0, st),
           h.dt_reg_grad(1, px, null, n8, f, f, P_(go), 0, st),
           h.dt_reg_grad(1, px, po, neg, f, f, P_(go), 1, st),
           h.dt_reg_grad(-1, px, po, n8, f, f, P_(go), 0, st),
           h.dt_reg_grad(1, px, po, n8, f, f, None, 0, st)]
    assert bad == [-1] * len(bad), bad
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()) and bool((tot == 5.0).all())       # nothing ran
    assert h.dt_reg_penalty(0, None, None, None, None, None, P_(tot), P_(tot[1:]), st) == 0      # no tensors: the sum is 0
    torch.cuda.synchronize()
    assert tot[0].item() == 0.0


# ===========================================================================================================================
# autograd
# ===========================================================================================================================
def test_autograd_function_over_weights_and_an_activation(dev):
    from deeptables_amd import ops
    g = torch.Generator().manual_seed(1)
    w1h, w2h, w3h = torch.randn(9, 5, generator=g), torch.randn(_chunk() + 3, generator=g), torch.randn(6, 4, generator=g)
    cf = [(0.01, 0.0), (0.0, 0.01), (1e-3, 5e-4)]
    for scale in (1.0, 2.0):
        w1, w2, w3 = (t.clone().to(dev).requires_grad_(True) for t in (w1h, w2h, w3h))
        act = w3 * 2.0                                    # a non-leaf input: its gradient flows on to w3, doubled exactly
        pen = ops.regularization_penalty([w1, w2, act], cf)
        assert pen.shape == () and pen.dtype == torch.float32 and pen.requires_grad
        ref = RR.total_penalty([w1h.numpy(), w2h.numpy(), (w3h * 2.0).numpy()], cf)
        assert abs(pen.item() - ref) <= U23 * abs(ref)
        (pen * scale).backward()
        for w, h, k, mul in ((w1, w1h, cf[0], 1.0), (w2, w2h, cf[1], 1.0), (w3, w3h * 2.0, cf[2], 2.0)):
            want = RR.grad_f32(h.numpy(), k[0], k[1], go=scale) * np.float32(mul)
            assert _bits(w.grad).equal(_bits(torch.from_numpy(want).reshape(w.shape)))
            ref64 = RR.grad(h.numpy(), k[0], k[1], go=scale) * mul
            assert np.abs(w.grad.cpu().numpy().astype(np.float64) - ref64.reshape(w.shape)).max() <= 3 * U24 * np.abs(ref64).max()
    frozen = w1h.clone().to(dev)                          # an input that needs no gradient gets none
    w = w2h.clone().to(dev).requires_grad_(True)
    ops.regularization_penalty([frozen, w], cf[:2]).backward()
    assert frozen.grad is None and w.grad is not None


# ===========================================================================================================================
# models
# ===========================================================================================================================
VOCABS, D, B, LR = (7, 9, 11), 4, 16, 0.01
TOWER = ((8, 0, False), (4, 0, False))


def _build(nets=('dnn_nets',), optimizer='sgd', dnn=None, var_len=False, strategy=None, **extra):
    from deeptables_amd import functional
    from deeptables_amd.models import ModelConfig, DeepModel
    from deeptables_amd.models.metainfo import CategoricalColumn, ContinuousColumn, VarLenCategoricalColumn
    functional.set_seed(21)
    conf = ModelConfig(nets=list(nets), fixed_embedding_dim=True, embeddings_output_dim=D, embedding_dropout=0, dense_dropout=0,
                       metrics=['AUC'], optimizer=optimizer, distribute_strategy=strategy,
                       dnn_params={'hidden_units': TOWER, 'activation': 'relu', **(dnn or {})}, **extra)
    cats = [CategoricalColumn(f'C{i}', v, D) for i, v in enumerate(VOCABS)]
    conts = [ContinuousColumn('input_continuous_all', ['I0'])]
    vl = None
    if var_len:
        vl = [VarLenCategoricalColumn('V0', 13, D)]
        vl[0].max_elements_length = 5
    dm = DeepModel('binary', 2, conf, cats, conts, var_categorical_len_columns=vl)
    dm.build()
    dm.model.train()
    return dm


def _pair(reg, **common):
    """(A without regularizers, B with `reg`), same weights"""
    a, b = _build(**common), _build(**{**common, **reg, 'dnn': {**common.get('dnn', {}), **reg.get('dnn', {})}})
    sa, sb = a.model.state_dict(), b.model.state_dict()
    assert list(sa) == list(sb)
    b.model.load_state_dict(sa)
    assert not a.model.has_regularizers() and b.model.has_regularizers()
    return a, b


def _batch(dev, var_len=False, seed=5):
    """ids b % (vocab - 1): the last row of every column is never looked up, every other row at least once, most twice"""
    g = torch.Generator().manual_seed(seed)
    idx = torch.stack([torch.arange(B) % (v - 1) for v in VOCABS], 1).int()
    dense = torch.randn(B, 1, generator=g)
    y = (torch.rand(B, 1, generator=g) < 0.4).float()
    ins = [idx.to(dev)]
    if var_len:
        ins.append(torch.randint(0, 13, (B, 5), generator=g).int().to(dev))
    ins.append(dense.to(dev))
    return ins, y.to(dev), idx


def _table(dm):
    return dm.model.layers_by_name['emb_categorical_vars_all'].tables[f'd{D}']


def _f64(t):
    return t.detach().cpu().double().numpy()


def _loss_bar(la, lb):
    return U24 * (abs(la) + abs(lb))            # one rounding of the penalty and one of the sum, at the two losses' size


def _step_pair(a, b, ins, y):
    """forward_backward on both, keep the gradients, then the optimizer step -> per model (loss, {name: (w, grad, w')})"""
    out = []
    for dm in (a, b):
        loss, _ = dm.forward_backward(ins, y)
        named = dict(dm.model.named_parameters())
        before = {n: (p.detach().clone(), None if p.grad is None else p.grad.detach().clone()) for n, p in named.items()}
        dm.optimizer.step()
        torch.cuda.synchronize()
        out.append((float(loss), {n: (before[n][0], before[n][1], named[n].detach().clone()) for n in named}))
    return out


def _check_weight_update(ra, rb, name, l1, l2):
    """w_B' - w_A' = -lr (l1 sign(w) + 2 l2 w) within 4 x 2^-24 x max(|w|, lr |g|): two float32 roundings in each step"""
    w, _ga, wa = ra[name]
    _, gb, wb = rb[name]
    want = -LR * RR.grad(_f64(w), l1, l2)
    got = _f64(wb) - _f64(wa)
    bar = 4 * U24 * np.maximum(np.abs(_f64(w)), LR * np.abs(_f64(gb)))
    worst = float((np.abs(got - want) / np.maximum(bar, 1e-300)).max())
    print(f'{name}: max |got - want| / bar = {worst:.3f}')
    assert (np.abs(got - want) <= bar).all(), (name, worst)
    return got


def _check_unregularised(ra, rb, skip):
    for name in ra:
        if name in skip:
            continue
        err = P.max_rel(rb[name][2], ra[name][2])
        assert err <= P.STEP_BAR['fp32'] * P.U, (name, err)


def test_sgd_step_with_weight_penalties_on_tables_and_kernels(dev):
    reg = dict(embeddings_regularizer={'class_name': 'L1L2', 'config': {'l1': 1e-3, 'l2': 0.01}}, dnn={'kernel_regularizer': 'l1'})
    a, b = _pair(reg)
    ins, y, idx = _batch(dev)
    (la, ra), (lb, rb) = _step_pair(a, b, ins, y)
    tname = [n for n in ra if 'tables' in n][0]
    kernels = [n for n in ra if n.endswith('kernel') and any(a.model.layers[int(n.split('.')[1])].name == d
                                                             for d in ('dnn_dense_1', 'dnn_dense_2'))]
    assert len(kernels) == 2
    pen = RR.penalty(_f64(ra[tname][0]), 1e-3, 0.01) + sum(RR.penalty(_f64(ra[k][0]), 0.01, 0.0) for k in kernels)
    print(f'loss A {la!r} B {lb!r} penalty {pen!r}')
    assert abs((lb - la) - pen) <= _loss_bar(la, lb), (la, lb, pen)
    moved = _check_weight_update(ra, rb, tname, 1e-3, 0.01)
    # rows the batch never looked up decay too: the last row of every column (A leaves them where they were)
    last = np.cumsum(VOCABS) - 1
    w0, _, wa = ra[tname]
    assert torch.equal(w0[last], wa[last]) and (np.abs(moved[last]) > 0).all()
    assert not any(int(v) - 1 in set(idx[:, i].tolist()) for i, v in enumerate(VOCABS))
    for k in kernels:
        _check_weight_update(ra, rb, k, 0.01, 0.0)
    _check_unregularised(ra, rb, skip=[tname] + kernels)


def test_adam_two_steps_with_l2_on_the_table(dev):
    """the whole table against the float64 regularised-Adam reference at the bar tests/test_optim_gpu.py holds the dense Adam
    kernel to (2e-6); the data gradient of each step comes from an unregularised twin holding B's weights"""
    a, b = _pair(dict(embeddings_regularizer='l2'), optimizer='adam')
    w = _f64(_table(b))
    m, v = np.zeros_like(w), np.zeros_like(w)
    for t in (1, 2):
        ins, y, _ = _batch(dev, seed=5 + t)
        a.model.load_state_dict(b.model.state_dict())
        a.forward_backward(ins, y)
        data_grad = _f64(_table(a).grad)
        b.train_step(ins, y)
        torch.cuda.synchronize()
        w, m, v = RR.adam_step(w, data_grad, m, v, t, l2=0.01)
        err = np.abs(_f64(_table(b)) - w).max()
        print(f'adam step {t}: max |table - ref| = {err:.3e}')
        assert err < 2e-6, (t, err)
    assert b.optimizer.t == 2


def test_embeddings_activity_regularizer_stays_on_the_looked_up_rows(dev):
    from deeptables_amd import regularizers as R
    a, b = _pair(dict(embeddings_activity_regularizer=R.L2(1e-3)))
    ins, y, idx = _batch(dev)
    (la, ra), (lb, rb) = _step_pair(a, b, ins, y)
    tname = [n for n in ra if 'tables' in n][0]
    w0 = _f64(ra[tname][0])
    offs = np.concatenate([[0], np.cumsum(VOCABS)[:-1]])
    rows = idx.numpy().astype(np.int64) + offs[None, :]                   # [B, F] packed rows
    pen = 1e-3 * float(np.square(w0[rows]).sum())                        # 1e-3 * sum out^2 over the looked-up [B, F, D] block
    print(f'loss A {la!r} B {lb!r} penalty {pen!r}')
    assert abs((lb - la) - pen) <= _loss_bar(la, lb)
    cnt = np.bincount(rows.reshape(-1), minlength=w0.shape[0]).astype(np.float64)
    assert (cnt == 0).sum() == 3 and (cnt == 1).any() and (cnt == 2).any() and (cnt == 3).any()
    got = _f64(rb[tname][2]) - _f64(ra[tname][2])
    want = -LR * cnt[:, None] * 2.0 * 1e-3 * w0                          # a row looked up twice gets twice the term
    gb = _f64(rb[tname][1])
    # two roundings per step as for a weight penalty, and one more per extra occurrence summed into the row's gradient
    bar = (4 + cnt[:, None]) * U24 * np.maximum(np.abs(w0), LR * np.abs(gb))
    assert (np.abs(got - want) <= bar).all(), float((np.abs(got - want) / np.maximum(bar, 1e-300)).max())
    untouched = cnt == 0
    assert torch.equal(rb[tname][2][untouched], rb[tname][0][untouched])  # untouched rows do NOT move
    assert (np.abs(got[cnt > 0]) > 0).any()
    _check_unregularised(ra, rb, skip=[tname])


def _hook_outputs(dm, names):
    seen, handles = {}, []
    for n in names:
        handles.append(dm.model.layers_by_name[n].register_forward_hook(
            lambda _m, _i, out, n=n: seen.__setitem__(n, out.detach().cpu().double().numpy())))
    return seen, handles


@pytest.mark.parametrize('custom', [False, True])
def test_dnn_kernel_and_activity_regularizers(dev, custom):
    """dnn_params' kernel_regularizer='l1' and activity_regularizer='l2': `dnn` penalises the Dense output before the
    Activation layer, `custom_dnn_D_A_D_B` the output after the Dense's own relu"""
    from deeptables_amd.models import deepnets
    base = {'custom_dnn_fn': deepnets.custom_dnn_D_A_D_B} if custom else {}
    prefix = 'dnn_custom' if custom else 'dnn'
    dense_names = [f'{prefix}_dense_1', f'{prefix}_dense_2']
    # kernel regularizer alone: loss difference and the kernels' update
    a, b = _pair(dict(dnn={'kernel_regularizer': 'l1'}), dnn=base)
    ins, y, _ = _batch(dev)
    (la, ra), (lb, rb) = _step_pair(a, b, ins, y)
    kernels = [n for n in ra if n.endswith('kernel') and a.model.layers[int(n.split('.')[1])].name in dense_names]
    assert len(kernels) == 2
    pen = sum(RR.penalty(_f64(ra[k][0]), 0.01, 0.0) for k in kernels)
    assert abs((lb - la) - pen) <= _loss_bar(la, lb), (la, lb, pen)
    for k in kernels:
        _check_weight_update(ra, rb, k, 0.01, 0.0)
    _check_unregularised(ra, rb, skip=kernels)
    # both: the loss difference is the kernels' penalty plus l2 * sum out^2 of the two Dense outputs
    a, b = _pair(dict(dnn={'kernel_regularizer': 'l1', 'activity_regularizer': 'l2'}), dnn=base)
    seen, handles = _hook_outputs(b, dense_names)
    la, _ = a.forward_backward(ins, y)
    lb, _ = b.forward_backward(ins, y)
    for h in handles:
        h.remove()
    la, lb = float(la), float(lb)
    named = dict(b.model.named_parameters())
    pen = sum(RR.penalty(_f64(named[k]), 0.01, 0.0) for k in kernels) + sum(RR.penalty(seen[n], 0.0, 0.01) for n in dense_names)
    print(f'loss A {la!r} B {lb!r} penalty {pen!r}')
    assert abs((lb - la) - pen) <= _loss_bar(la, lb), (la, lb, pen)
    for n in dense_names:
        assert seen[n].shape == (B, dict(zip(dense_names, (8, 4)))[n])
        if custom:
            assert seen[n].min() == 0.0                   # post-activation: relu has clipped
        else:
            assert seen[n].min() < 0.0                    # pre-activation
    # the activity penalty's gradient reaches the layers below: the first kernel's gradient differs from kernel-penalty-only
    assert not torch.equal(named[kernels[0]].grad, rb[kernels[0]][1])


def test_afm_kernel_regularizer(dev):
    from deeptables_amd import regularizers as R
    afm = {'hidden_factor': 4, 'dropout_rate': 0}
    a, b = _pair(dict(afm_params={**afm, 'kernel_regularizer': R.L1L2(1e-3, 0.01)}), nets=['afm_nets'], afm_params=afm)
    ins, y, _ = _batch(dev)
    (la, ra), (lb, rb) = _step_pair(a, b, ins, y)
    name = [n for n in ra if n.endswith('dense_attention.kernel')]
    assert len(name) == 1
    pen = RR.penalty(_f64(ra[name[0]][0]), 1e-3, 0.01)
    assert pen > 0 and abs((lb - la) - pen) <= _loss_bar(la, lb), (la, lb, pen)
    _check_weight_update(ra, rb, name[0], 1e-3, 0.01)
    _check_unregularised(ra, rb, skip=name)


def test_var_len_column_with_both_embedding_regularizers(dev):
    from deeptables_amd import regularizers as R
    a, b = _pair(dict(embeddings_regularizer='l2', embeddings_activity_regularizer=R.L1(1e-3)), var_len=True)
    ins, y, idx = _batch(dev, var_len=True)
    (la, ra), (lb, rb) = _step_pair(a, b, ins, y)
    tname = [n for n in ra if 'tables' in n][0]
    vname = [n for n in ra if n.endswith('embeddings') and 'tables' not in n]
    assert len(vname) == 1
    w0, v0 = _f64(ra[tname][0]), _f64(ra[vname[0]][0])
    offs = np.concatenate([[0], np.cumsum(VOCABS)[:-1]])
    rows = idx.numpy().astype(np.int64) + offs[None, :]
    seq = ins[1].cpu().numpy().astype(np.int64)
    pen = RR.penalty(w0, 0.0, 0.01) + RR.penalty(v0, 0.0, 0.01) + RR.penalty(w0[rows], 1e-3, 0.0) + RR.penalty(v0[seq], 1e-3, 0.0)
    print(f'loss A {la!r} B {lb!r} penalty {pen!r}')
    assert abs((lb - la) - pen) <= _loss_bar(la, lb), (la, lb, pen)


def test_nothing_of_the_step_stays_allocated(dev):
    """the activations the model collected are gone after the step, without a collector run: the weakref is dead and the
    device memory in use is what it was before the step"""
    import gc
    import weakref
    from deeptables_amd import regularizers as R
    _, b = _pair(dict(embeddings_activity_regularizer=R.L2(1e-3), dnn={'activity_regularizer': 'l2'}))
    ins, y, _ = _batch(dev)
    b.train_step(ins, y)                                   # (allocator warm-up, lazy state)
    torch.cuda.synchronize()
    gc.collect()
    gc.disable()
    try:
        base = torch.cuda.memory_allocated()
        b.model(ins)
        assert len(b.model._activity) == 3                 # the packed [B, F, D] block in one piece + two Dense outputs
        refs = [weakref.ref(t) for t, _ in b.model._activity]
        assert b.model._activity[0][0].shape == (B, 3, D)
        b.train_step(ins, y)
        torch.cuda.synchronize()
        assert b.model._activity is None and all(r() is None for r in refs)
        b.optimizer.zero_grad()
        assert torch.cuda.memory_allocated() <= base
    finally:
        gc.enable()


def _frame(n, seed=0):
    import pandas as pd
    rng = np.random.RandomState(seed)
    df = pd.DataFrame({f'C{i}': rng.randint(0, v - 1, n) for i, v in enumerate(VOCABS)})
    df['I0'] = rng.randn(n).astype(np.float32)
    return df, (rng.rand(n) < 0.4).astype(np.float32)


def test_evaluate_carries_the_penalties_and_predict_does_not_change(dev, monkeypatch):
    """evaluate's loss, Keras' mean over batches with the penalties in every batch's loss:
        loss = sum_b n_b (data_b + activity_b) / sum_b n_b + weight penalty
    (the weight penalty is the same in every batch, so it is added once; activity_b = the batch-summed activity penalty of
    batch b, not divided by n_b).  predict: B's output equals A's bit for bit, on the inference plan in every case.  A model
    with an activity regularizer evaluates on the layer path; its twin A is put there too (DT_AMD_FUSED_PREDICT=0) so that
    the two data losses are the same kernels' and the difference is the penalties alone."""
    from deeptables_amd import regularizers as R
    df, y = _frame(40)
    a, b = _pair(dict(embeddings_regularizer='l2'))
    la, lb = a.evaluate(df, y, batch_size=16)['loss'], b.evaluate(df, y, batch_size=16)['loss']
    wpen = RR.penalty(_f64(_table(a)), 0.0, 0.01)
    assert abs((lb - la) - wpen) <= _loss_bar(la, lb) + U24 * wpen, (la, lb, wpen)
    assert np.array_equal(a.predict(df, batch_size=16), b.predict(df, batch_size=16))
    a, b = _pair(dict(embeddings_regularizer='l2', embeddings_activity_regularizer=R.L2(1e-3)))
    assert np.array_equal(a.predict(df, batch_size=16), b.predict(df, batch_size=16))
    assert (a.inference_plan() is None) == (b.inference_plan() is None)
    monkeypatch.setenv('DT_AMD_FUSED_PREDICT', '0')
    la, lb = a.evaluate(df, y, batch_size=16)['loss'], b.evaluate(df, y, batch_size=16)['loss']
    w0 = _f64(_table(a))
    offs = np.concatenate([[0], np.cumsum(VOCABS)[:-1]])
    rows = df[[f'C{i}' for i in range(3)]].to_numpy().astype(np.int64) + offs[None, :]
    act = [1e-3 * float(np.square(w0[rows[s:s + 16]]).sum()) for s in range(0, 40, 16)]
    sizes = [16, 16, 8]
    want = sum(n * p for n, p in zip(sizes, act)) / 40.0 + wpen
    print(f'evaluate: A {la!r} B {lb!r} want diff {want!r}')
    assert abs((lb - la) - want) <= 4 * _loss_bar(la, lb), (la, lb, want)      # (three batches' sums and the weighted mean)
    assert b.model._activity is None and not b.model.collect_eval_activity


def test_graphed_fit_equals_eager_fit(dev):
    """`fit(steps_per_execution=2)` on a regularised model captures the layer path, penalty included, and equals the eager
    fit after one epoch of 13 steps — the comparison and bars of test_graphed_fit_replays_the_new_optimizers"""
    from tests.test_compiled_gpu import _fit, _frame as frame, _model, _same
    from deeptables_amd import regularizers as R
    df, y = frame(64 * 13 + 5)
    reg = dict(embeddings_regularizer='l2', embeddings_activity_regularizer=R.L2(1e-3),
               dnn_params={'hidden_units': ((128, 0, False), (64, 0, False)), 'kernel_regularizer': R.L1L2(1e-4, 1e-3),
                           'activity_regularizer': R.L2(1e-4)})
    eager, graphed = _model('DeepFM', **reg), _model('DeepFM', **reg)
    assert eager.model.has_regularizers() and eager.fused_plan() is None
    h0 = _fit(eager, df, y, 1, epochs=1)
    h1 = _fit(graphed, df, y, 2, epochs=1)
    assert eager.compiled_loop is None
    loop = graphed.compiled_loop
    assert loop is not None and loop.graph is not None and loop.k == 2
    assert eager.optimizer.t == graphed.optimizer.t == 13
    _same(eager, graphed, tol=2e-6)
    assert np.allclose(h0.history['loss'], h1.history['loss'], atol=2e-6), (h0.history, h1.history)
    plain = _model('DeepFM')
    assert h0.history['loss'][0] > _fit(plain, df, y, 1, epochs=1).history['loss'][0]      # the logged loss carries the penalty


def test_checkpoint_round_trip_trains_on_with_the_same_penalties(dev, tmp_path):
    from deeptables_amd import regularizers as R
    from deeptables_amd.models import DeepModel
    _, b = _pair(dict(embeddings_regularizer='l2', embeddings_activity_regularizer=R.L2(1e-3),
                      dnn={'kernel_regularizer': 'l1', 'activity_regularizer': 'l2'}), optimizer='adam')
    ins, y, _ = _batch(dev)
    b.train_step(ins, y)
    path = str(tmp_path / 'reg.safetensors')
    b.save(path, include_optimizer=True)
    b2 = DeepModel('binary', 2, b.config, b.categorical_columns, b.continuous_columns, model_file=path)
    b2.model.train()
    assert b2.model.has_regularizers() and [c for _, c in b2.model.weight_penalties()] == [c for _, c in b.model.weight_penalties()]
    for t1, t2 in zip(b.model.state_dict().values(), b2.model.state_dict().values()):
        assert torch.equal(t1, t2)
    # one more step on a batch without repeated ids (the table's dense gradient is a float-atomic scatter: with repeats
    # its last bits depend on the order, as in the existing checkpoint tests): the same bits with and without the save / load
    g = torch.Generator().manual_seed(8)
    idx = torch.stack([torch.randperm(v, generator=g)[:6] for v in VOCABS], 1).int()
    ins = [idx.to(dev), torch.randn(6, 1, generator=g).to(dev)]
    y = torch.tensor([[1.0], [0.0], [0.0], [1.0], [0.0], [1.0]], device=dev)
    l1, _ = b.train_step(ins, y)
    l2, _ = b2.train_step(ins, y)
    assert float(l1) == float(l2)
    for (n1, p1), (n2, p2) in zip(b.model.named_parameters(), b2.model.named_parameters()):
        assert torch.equal(p1, p2), n1


def test_data_parallel_step_equals_the_single_process_step(dev):
    """world size 1 through RCCL with the collectives forced: every rank adds the full weight penalty's gradient before the
    exchange (sum, then / W: W identical terms stay that term) — the bars of test_fused_gpu's data-parallel tests"""
    import torch.distributed as dist
    from deeptables_amd import regularizers as R
    from deeptables_amd.parallel import DataParallelStrategy
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK='0', WORLD_SIZE='1', LOCAL_RANK='0')
    st = DataParallelStrategy.from_env('nccl')
    st.force_dp = True
    st.force_collectives = True
    try:
        reg = dict(embeddings_regularizer='l2', embeddings_activity_regularizer=R.L2(1e-3), optimizer='adam',
                   dnn={'kernel_regularizer': 'l1', 'activity_regularizer': 'l2'})
        models = [_build(**reg), _build(strategy=st, **reg)]
        models[1].model.load_state_dict(models[0].model.state_dict())
        losses = [[], []]
        for step in range(3):
            ins, y, _ = _batch(dev, seed=20 + step)
            for k, dm in enumerate(models):
                l, _ = dm.train_step(ins, y)
                losses[k].append(float(l))
        assert np.allclose(losses[0], losses[1], atol=1e-6), losses
        for (n0, p0), (n1, p1) in zip(models[0].model.named_parameters(), models[1].model.named_parameters()):
            assert (p0 - p1).abs().max().item() < 2e-6, n0
    finally:
        dist.destroy_process_group()
