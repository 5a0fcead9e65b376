# -*- coding:utf-8 -*-
"""GPU: the tower-cell kernels of csrc/cell.hip (dt_cell_fwd / dt_cell_bwd) against the float64 restatements of
tests/cell_reference.py, the layers that route through them (Activation, Dropout, Dense with an activation of its own, the
third peephole of functional.Model) and DeepModel towers with every activation name.

Bar: yardstick B of tests/precision.py — err_gpu <= STEP_BAR['fp32'] x max(err_f32, FLOOR), err_f32 the error of the same
restatement evaluated in float32 on the CPU — in two metrics for out and dx: max_rel, and the largest element-wise relative
error over the elements whose reference is at least 1e-30 in magnitude.  Every ratio goes through precision.record.

Geometry of csrc/cell.hip that the shapes walk: 256 threads, one 16-byte vector (4 floats) per thread and step when N C >= 4
and every base address is 16-byte aligned, one float otherwise; at most 2048 blocks, so one grid pass of the vector path
covers dt_cell_pass_elems() = 2048 * 256 * 4 elements; the N C % 4 elements behind the last vector go to block 0.

Random inputs cover each activation's useful range, RANGES below.  For the activations whose derivative is read off the saved
OUTPUT the range ends where that output still determines the derivative to fp32: y + 1 = e^x of elu / selu and 1 - e^-y of
softplus lose the digits of e^x to the rounding of y (an amplification of 1 / e^x, held to 3.5 by x >= -1.25), (1 - |y|)^2 of
softsign those of 1 / (1 + |x|) (2 |y| / (1 - |y|), held to 6 by |x| <= 3) — while torch's float32 backward of these four
starts from the input; sigmoid and tanh lose the digits in torch's own backward in the same way.
The structured set adds +-0, +-1e-30, +-80, +-100, the activation's own kinks (0; 6; +-3) with their two neighbouring floats,
a NaN and an inf."""
import math

import pytest
import torch

from tests import cell_reference as CR
from tests import precision as P

pytestmark = pytest.mark.gpu

BAR, FLOOR = P.STEP_BAR['fp32'], P.FLOOR
TINY = 1e-30
RANGES = {'elu': (-1.25, 6.0), 'selu': (-1.25, 6.0), 'softplus': (-1.25, 6.0), 'softsign': (-3.0, 3.0),
          'exponential': (-10.0, 10.0), 'relu6': (-3.0, 9.0)}
DEFAULT_RANGE = (-6.0, 6.0)


def _structured(name):
    """the hard inputs and the positions of the NaN and the inf among them"""
    vals = [0.0, -0.0, 1e-30, -1e-30, 80.0, -80.0, 100.0, -100.0]
    for k in sorted(CR.KINKS.get(name, {})):
        t = torch.tensor(k)
        vals += [k, torch.nextafter(t, torch.tensor(math.inf)).item(), torch.nextafter(t, torch.tensor(-math.inf)).item()]
    nan_at, inf_at = len(vals), len(vals) + 1
    return torch.tensor(vals + [math.nan, math.inf]), nan_at, inf_at


def _draw(name, N, C, seed=0):
    """x, g float32 [N, C]; the structured set leads the tensor when it fits -> (x, g, nan position, inf position) (flat, or None)"""
    gen = torch.Generator().manual_seed(7919 * seed + 31 * N + C)
    lo, hi = RANGES.get(name, DEFAULT_RANGE)
    x = torch.rand(N * C, generator=gen) * (hi - lo) + lo
    g = (torch.rand(N * C, generator=gen) + 0.5) * (torch.randint(0, 2, (N * C,), generator=gen) * 2 - 1).float()
    s, nan_at, inf_at = _structured(name)
    if N * C < 4 * s.numel():
        return x.reshape(N, C), g.reshape(N, C), None, None
    x[:s.numel()] = s
    return x.reshape(N, C), g.reshape(N, C), nan_at, inf_at


def _dev_view(t, dev, offset):
    """`t` on the device, `offset` floats into a 16-byte aligned buffer (offset 1: every base address is 4 bytes off)"""
    buf = torch.full((t.numel() + 4,), float('nan'), dtype=torch.float32, device=dev)
    v = buf[offset:offset + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * offset
    return v


def _seed_word(dev, value):
    return torch.tensor([value], dtype=torch.int32, device=dev)


def _kernel(dev, name, x, g, rate=0.0, seed=None, salt=0, offset=0):
    """dt_cell_fwd and dt_cell_bwd through ctypes on NaN-poisoned outputs -> (out, dx) on the host.  The backward is handed what
    ops.cell saves: the input for the input kinds and under a mask, else the forward's output."""
    from deeptables_amd import _lib, ops
    h = _lib.lib()
    code = _lib.CELL_ACT_CODES[name]
    N, C = x.shape
    xd, gd = _dev_view(x, dev, offset), _dev_view(g, dev, offset)
    out = _dev_view(torch.full_like(x, float('nan')), dev, offset)
    dx = _dev_view(torch.full_like(x, float('nan')), dev, offset)
    ops.cell_fwd_launch(xd, code, rate, seed, salt, out)
    by_input = bool(h.dt_cell_saves_input(code)) or 0.0 < rate < 1.0
    ops.cell_bwd_launch(gd, xd if by_input else out, by_input, code, rate, seed, salt, dx)
    torch.cuda.synchronize()
    return out.cpu(), dx.cpu()


def _elem_rel(got, ref, live):
    """largest element-wise relative error over the live elements with |ref| >= 1e-30"""
    got, ref = got.double().reshape(-1), ref.double().reshape(-1)
    m = live.reshape(-1) & (ref.abs() >= TINY)
    if not bool(m.any()):
        return 0.0
    return ((got[m] - ref[m]).abs() / ref[m].abs()).max().item()


def _max_rel(got, ref, live):
    m = live.reshape(-1)
    return P.max_rel(got.reshape(-1)[m], ref.reshape(-1)[m])


def _check(test, dev, name, x, g, nan_at, inf_at, rate=0.0, seed=None, salt=0, offset=0, what=''):
    """yardstick B in both metrics for out and dx, the NaN / inf positions, nothing left unwritten -> (out, dx) of the kernel"""
    N, C = x.shape
    keep = None
    if rate > 0:
        from deeptables_amd import ops
        keep = ops.cell_dropout_keep(seed, salt, N, C, rate)
    r_out, r_dx = CR.value_and_grad(name, x, g, keep, torch.float64)
    f_out, f_dx = CR.value_and_grad(name, x, g, keep, torch.float32)
    out, dx = _kernel(dev, name, x, g, rate, seed, salt, offset)
    # elements that are compared as numbers: a finite input whose reference is finite in float32, in both directions
    live = torch.isfinite(x) & torch.isfinite(r_out.float()) & torch.isfinite(r_dx.float())
    if keep is not None:                   # ... before the mask too: 0 * exponential(100) is 0 * inf in float32, as in torch
        a_out, a_dx = CR.value_and_grad(name, x, g, None, torch.float64)
        live &= torch.isfinite(a_out.float()) & torch.isfinite(a_dx.float())
    assert torch.isfinite(out[live]).all() and torch.isfinite(dx[live]).all(), (name, what)
    if nan_at is not None:
        assert math.isnan(out.reshape(-1)[nan_at]) and math.isnan(dx.reshape(-1)[nan_at]), (name, 'NaN in gives NaN out')
        o, r = out.reshape(-1)[inf_at].item(), r_out.float().reshape(-1)[inf_at].item()      # the limit, or NaN where it is inf * 0
        assert (math.isnan(o) and math.isnan(r)) or o == r, (name, 'inf', o, r)
    over = torch.isfinite(x) & ~torch.isfinite(r_out.float()) & torch.isfinite(r_out)       # exponential(100): inf in float32
    assert torch.equal(out[over], r_out.float()[over])
    figures = {}
    for key, got, ref, f32 in (('out', out, r_out, f_out), ('dx', dx, r_dx, f_dx)):
        for metric, fn in (('max_rel', _max_rel), ('elem_rel', _elem_rel)):
            e_g, e_f = fn(got, ref, live), fn(f32, ref, live)
            figures[f'{key}_{metric}'] = (e_g / max(e_f, FLOOR), e_g, e_f)
    P.record(test, name=name, what=str(what), **{k: v[0] for k, v in figures.items()})
    print(test, name, what, {k: (round(v[0], 2), f'{v[1]:.2e}', f'{v[2]:.2e}') for k, v in figures.items()})
    bad = {k: v for k, v in figures.items() if not (math.isfinite(v[0]) and v[0] <= BAR)}
    assert not bad, (name, what, 'ratio, err_gpu, err_f32', bad)
    return out, dx


# ===========================================================================================================================
# kernel level
# ===========================================================================================================================
SHAPES = [(1, 1), (3, 5), (7, 128), (33, 129), (257, 64)]


@pytest.mark.parametrize('name', CR.NAMES)
def test_every_activation_at_every_shape(dev, name):
    for N, C in SHAPES:
        x, g, nan_at, inf_at = _draw(name, N, C)
        _check('cell_shapes', dev, name, x, g, nan_at, inf_at, what=(N, C))


def _past_one_pass():
    """[N, C] just past one full grid pass of the 16-byte path, N C not a multiple of 4"""
    from deeptables_amd import _lib
    one_pass = _lib.lib().dt_cell_pass_elems()
    assert one_pass == 2048 * 256 * 4
    C = 129
    N = one_pass // C + 3
    assert one_pass < N * C < one_pass + 4 * C and (N * C) % 4 != 0
    return N, C


@pytest.mark.parametrize('name', ['tanh', 'gelu', 'relu6'])
def test_the_grid_stride_loop_and_its_tail(dev, name):
    """one output kind, one input kind, one with kinks: every thread of the grid takes a second vector or none, block 0 the tail;
    with a mask the (row, column) of the second pass comes from the stride's (rows, columns)"""
    N, C = _past_one_pass()
    x, g, nan_at, inf_at = _draw(name, N, C)
    _check('cell_past_one_pass', dev, name, x, g, nan_at, inf_at, what=(N, C))
    seed = _seed_word(dev, 20240229)
    _check('cell_past_one_pass', dev, name, x, g, nan_at, inf_at, rate=0.5, seed=seed, salt=77, what=(N, C, 'rate 0.5'))


@pytest.mark.parametrize('name', CR.NAMES)
def test_a_base_address_off_by_four_bytes_takes_the_scalar_path(dev, name):
    for N, C in ((33, 129), (257, 64)):
        x, g, nan_at, inf_at = _draw(name, N, C, seed=1)
        a = _check('cell_scalar_path', dev, name, x, g, nan_at, inf_at, offset=1, what=(N, C, 'offset 4 bytes'))
        b = _kernel(dev, name, x, g)
        for u, v in zip(a, b):                                       # the same element code on both paths
            assert torch.equal(torch.nan_to_num(u, nan=7.0), torch.nan_to_num(v, nan=7.0)), name


@pytest.mark.parametrize('name', sorted(CR.KINKS))
def test_kink_derivatives_are_torch_s(dev, name):
    """AT each kink dx is g times the exact value torch's CPU autograd takes there (test_cell_host.py holds the table to torch)"""
    pts = sorted(CR.KINKS[name])
    x = torch.tensor(pts * 8).reshape(8, len(pts))
    g = torch.linspace(-2.0, 3.0, x.numel()).reshape(x.shape) + 0.0625
    for offset in (0, 1):
        _, dx = _kernel(dev, name, x, g, offset=offset)
        want = g * torch.tensor([CR.KINKS[name][p] for p in pts], dtype=torch.float32)
        assert torch.equal(dx, want), (name, offset, dx[0].tolist(), want[0].tolist())
    seed = _seed_word(dev, 5)
    _, dx = _kernel(dev, name, x, g, rate=0.5, seed=seed, salt=1)     # under a mask the derivative comes from the saved input
    from deeptables_amd import ops
    keep = ops.cell_dropout_keep(seed, 1, 8, len(pts), 0.5)
    assert torch.equal(dx, (g * keep) * torch.tensor([CR.KINKS[name][p] for p in pts], dtype=torch.float32))
    assert 0 < int((keep > 0).sum()) < keep.numel()


@pytest.mark.parametrize('name', CR.NAMES)
def test_dropout_mask_is_the_mirror_s(dev, name):
    """rate > 0: out = act(x) * keep with keep from ops.cell_dropout_keep, to the rounding of one fp32 product (bit-equal to the
    rate-0 output times keep); dx exactly zero where dropped; rates 0 and 1; two seeds and two salts give different masks"""
    from deeptables_amd import ops
    N, C = 33, 129
    x, g, nan_at, inf_at = _draw(name, N, C, seed=2)
    seed, salt = _seed_word(dev, -123456789), ops.cell_salt('dnn_dropout_1')
    out0, dx0 = _check('cell_dropout', dev, name, x, g, nan_at, inf_at, what='rate 0')
    finite = torch.isfinite(out0) & torch.isfinite(dx0)
    for rate in (0.25, 0.9):
        out, dx = _check('cell_dropout', dev, name, x, g, nan_at, inf_at, rate=rate, seed=seed, salt=salt, what=f'rate {rate}')
        keep = ops.cell_dropout_keep(seed, salt, N, C, rate)
        assert torch.equal(out[finite], (out0 * keep)[finite])
        dropped = finite & (keep == 0)
        assert int(dropped.sum()) > 0 and bool((dx[dropped] == 0).all()) and bool((out[dropped] == 0).all())
    out1, dx1 = _kernel(dev, name, x, g, rate=1.0)                      # no seed word needed, no inf scale
    assert bool((out1[finite] == 0).all()) and bool((dx1[finite] == 0).all())
    masks = [(_kernel(dev, 'linear', torch.ones(N, C), torch.ones(N, C), 0.5, _seed_word(dev, s), t)[0] > 0)
             for s, t in ((11, 3), (12, 3), (11, 4))]
    for m, (s, t) in zip(masks, ((11, 3), (12, 3), (11, 4))):
        assert torch.equal(m, ops.cell_dropout_keep(s, t, N, C, 0.5) > 0)
    assert not torch.equal(masks[0], masks[1]) and not torch.equal(masks[0], masks[2])


def test_ops_cell_saves_one_tensor_and_the_seed_word(dev):
    from deeptables_amd import ops
    x = torch.randn(9, 20, device=dev, requires_grad=True)
    seed = _seed_word(dev, 99)
    for name, rate, saved_is in (('tanh', 0.0, 'out'), ('gelu', 0.0, 'x'), ('tanh', 0.3, 'x')):
        y = ops.cell(x, name, rate, seed, 5)
        saved = y.grad_fn.saved_tensors
        assert len(saved) == 2 and (saved[1] is None) == (rate == 0.0)
        assert saved[0].data_ptr() == (y if saved_is == 'out' else x).data_ptr(), (name, rate)
        r_out, r_dx = CR.value_and_grad(name, x, torch.ones(9, 20), ops.cell_dropout_keep(seed, 5, 9, 20, rate))
        (dx,) = torch.autograd.grad(y.sum(), x)
        assert P.max_rel(y, r_out) <= 1e-6 and P.max_rel(dx, r_dx) <= 1e-6
    with pytest.raises(ValueError, match='cell activation'):
        ops.cell(x, 'softmax')
    y3 = ops.cell(torch.randn(4, 3, 8, device=dev), 'relu6')            # rows = every leading dimension
    assert y3.shape == (4, 3, 8)


# ===========================================================================================================================
# layer chains: Input -> Dense(16) -> BN -> Activation -> Dropout(0.25) -> Dense(1), and the D_A_D_B order, 37 rows
# ===========================================================================================================================
ROWS, K_IN, UNITS, RATE, SEED = 37, 9, 16, 0.25, 1234567


def _chain_model(dev, name, order):
    from deeptables_amd import functional as Fn
    Fn.reset_uids()
    Fn.set_seed(17)
    x = Fn.Input((K_IN,), name='cell_in')
    if order == 'dnn':
        h = Fn.Dense(UNITS, use_bias=False, name='d1')(x)
        h = Fn.BatchNormalization(name='bn')(h)
        h = Fn.Activation(name, name='act')(h)
        h = Fn.Dropout(RATE, name='drop')(h)
    else:
        h = Fn.Dense(UNITS, activation=name, name='d1')(x)
        h = Fn.Dropout(RATE, name='drop')(h)
        h = Fn.BatchNormalization(name='bn')(h)
    m = Fn.Model(x, Fn.Dense(1, name='d2')(h)).to(dev)
    m.train()
    return m


@pytest.mark.parametrize('order', ['dnn', 'dadb'])
@pytest.mark.parametrize('name', ['tanh', 'gelu', 'relu6', 'mish', 'relu', 'sigmoid'])
def test_layer_chain_is_one_launch_each_way(dev, monkeypatch, name, order):
    from deeptables_amd import ops
    monkeypatch.setattr(ops, 'draw_cell_seed', lambda device: torch.tensor([SEED], dtype=torch.int32, device=device))
    calls = {'fwd': 0, 'bwd': 0}
    fwd, bwd = ops.cell_fwd_launch, ops.cell_bwd_launch
    monkeypatch.setattr(ops, 'cell_fwd_launch', lambda *a: (calls.__setitem__('fwd', calls['fwd'] + 1), fwd(*a))[1])
    monkeypatch.setattr(ops, 'cell_bwd_launch', lambda *a: (calls.__setitem__('bwd', calls['bwd'] + 1), bwd(*a))[1])

    def no_torch_dropout(*a, **k):
        raise AssertionError('torch.nn.functional.dropout reached')
    monkeypatch.setattr(torch.nn.functional, 'dropout', no_torch_dropout)
    m = _chain_model(dev, name, order)
    if name == 'relu' and order == 'dadb':
        assert not m._cell_fused                      # a Dense's own relu stays in its GEMM; the Dropout is a cell of its own
    else:
        assert len(m._cell_fused) == 1 and len(m._cell_passthrough) == 1
    L = m.layers_by_name
    g = torch.Generator().manual_seed(3)
    x = torch.randn(ROWS, K_IN, generator=g)
    up = torch.randn(ROWS, 1, generator=g)
    with torch.no_grad():                             # weights that make every tensor of the chain non-trivial
        L['bn'].gamma.copy_(torch.rand(UNITS, generator=g) + 0.5)
        L['bn'].beta.copy_(torch.randn(UNITS, generator=g) * 0.3)
        L['d2'].bias.fill_(0.25)
        if order == 'dadb':
            L['d1'].bias.copy_(torch.randn(UNITS, generator=g) * 0.3)
    out = m(x.to(dev))
    (out * up.to(dev)).sum().backward()
    torch.cuda.synchronize()
    assert calls == {'fwd': 1, 'bwd': 1}, calls
    p = {'W1': L['d1'].kernel, 'b1': L['d1'].bias, 'gamma': L['bn'].gamma, 'beta': L['bn'].beta, 'W2': L['d2'].kernel,
         'b2': L['d2'].bias}
    keep = ops.cell_dropout_keep(SEED, L['drop'].salt, ROWS, UNITS, RATE)
    assert 0 < int((keep > 0).sum()) < keep.numel()
    figures = {}
    legs = {}
    for dtype in (torch.float64, torch.float32):
        o, leaf = CR.chain(x, p, name, keep, order, dtype)
        (o * up.to(dtype)).sum().backward()
        legs[dtype] = {'out': o.detach(), **{k: v.grad for k, v in leaf.items()}}
    got = {'out': out.detach(), **{k: v.grad for k, v in p.items() if v is not None}}
    for k, ref in legs[torch.float64].items():
        e_g, e_f = P.max_rel(got[k], ref), P.max_rel(legs[torch.float32][k], ref)
        figures[k] = (e_g / max(e_f, FLOOR), e_g, e_f)
    P.record('cell_chain', name=name, order=order, **{k: v[0] for k, v in figures.items()})
    print('cell_chain', name, order, {k: (round(v[0], 2), f'{v[1]:.2e}', f'{v[2]:.2e}') for k, v in figures.items()})
    bad = {k: v for k, v in figures.items() if not (math.isfinite(v[0]) and v[0] <= BAR)}
    assert not bad, (name, order, bad)
    # inference: the dropout is the identity, the activation alone is one launch
    calls.update(fwd=0, bwd=0)
    m.eval()
    with torch.no_grad():
        m(x.to(dev))
    assert calls == {'fwd': 0 if (name == 'relu' and order == 'dadb') else 1, 'bwd': 0}


def test_the_off_switch_restores_the_torch_ops(dev, monkeypatch):
    from deeptables_amd import ops
    calls = []
    fwd = ops.cell_fwd_launch
    monkeypatch.setattr(ops, 'cell_fwd_launch', lambda *a: (calls.append(1), fwd(*a))[1])
    drops, dropout = [], torch.nn.functional.dropout
    monkeypatch.setattr(torch.nn.functional, 'dropout', lambda *a, **k: (drops.append(1), dropout(*a, **k))[1])
    m = _chain_model(dev, 'tanh', 'dnn')
    x = torch.randn(ROWS, K_IN).to(dev)
    monkeypatch.setenv('DT_AMD_CELL', '0')
    m(x)
    assert not calls and len(drops) == 1
    monkeypatch.setenv('DT_AMD_CELL', '1')                 # read at every call
    m(x)
    assert len(calls) == 1 and len(drops) == 1


# ===========================================================================================================================
# through the model: ['dnn_nets'], 3 categorical + 2 dense columns, B = 64
# ===========================================================================================================================
VOCABS, D, B = (7, 9, 11), 4, 64
TOWER = ((16, 0.25, True), (8, 0.5, False))


def _model(activation, tower=TOWER, seed=33):
    from deeptables_amd import functional
    from deeptables_amd.models import ModelConfig, DeepModel
    from deeptables_amd.models.metainfo import CategoricalColumn, ContinuousColumn
    functional.set_seed(seed)
    conf = ModelConfig(nets=['dnn_nets'], fixed_embedding_dim=True, embeddings_output_dim=D, embedding_dropout=0,
                       dense_dropout=0, metrics=[], optimizer='sgd', dnn_params={'hidden_units': tower, 'activation': activation})
    cats = [CategoricalColumn(f'C{i}', v, D) for i, v in enumerate(VOCABS)]
    conts = [ContinuousColumn('input_continuous_all', ['I0', 'I1'])]
    dm = DeepModel('binary', 2, conf, cats, conts)
    dm.build()
    dm.model.train()
    return dm


def _batch(dev, n=B, seed=0):
    g = torch.Generator().manual_seed(seed)
    idx = torch.stack([torch.randint(0, v, (n,), generator=g) for v in VOCABS], 1).int()
    dense = torch.randn(n, 2, generator=g)
    y = (torch.rand(n, 1, generator=g) < 0.4).float()
    return [idx.to(dev), dense.to(dev)], y.to(dev)


@pytest.mark.parametrize('name', CR.NAMES[1:])
def test_a_tower_with_every_activation_name_trains(dev, name):
    """((16, 0.25, True), (8, 0.5, False)): train_step runs, the loss is finite, the tower's weights move and stay finite"""
    dm = _model(name)
    assert len(dm.model._cell_fused) == (1 if name == 'relu' else 2)      # relu without BN stays in its GEMM (first peephole)
    ins, y = _batch(dev)
    L = dm.model.layers_by_name
    watch = {'dnn_dense_1.kernel': L['dnn_dense_1'].kernel, 'dnn_bn_1.gamma': L['dnn_bn_1'].gamma, 'dnn_bn_1.beta': L['dnn_bn_1'].beta,
             'dnn_dense_2.kernel': L['dnn_dense_2'].kernel, 'dnn_dense_2.bias': L['dnn_dense_2'].bias,
             'task_output.kernel': L['task_output'].kernel}
    before = {k: v.detach().clone() for k, v in watch.items()}
    loss, logit = dm.train_step(ins, y)       # one step: an exponential tower under plain SGD overflows float32 by its second
    assert math.isfinite(float(loss)) and torch.isfinite(logit).all()
    still = [k for k, v in watch.items() if torch.equal(v, before[k]) or not torch.isfinite(v).all()]
    assert not still, still


@pytest.mark.parametrize('name', ['tanh', 'relu', 'gelu', 'mish', 'hard_silu', 'relu6', 'elu'])
def test_rate_zero_tower_agrees_with_the_torch_path(dev, monkeypatch, name):
    """rate 0: the logits and the tower's parameter gradients of the cell run and of the DT_AMD_CELL=0 run of the same model,
    each against the float64 chain from the tower's input: the cell run within yardstick B of the torch run's error"""
    tower = ((16, 0, True), (8, 0, False))
    ins, _ = _batch(dev, seed=5)
    up = torch.randn(B, 1, generator=torch.Generator().manual_seed(9))
    legs, x0 = {}, []
    start = _model(name, tower).model.state_dict()
    for leg in ('cell', 'torch'):
        monkeypatch.setenv('DT_AMD_CELL', '1' if leg == 'cell' else '0')
        dm = _model(name, tower)
        dm.model.load_state_dict(start)
        L = dm.model.layers_by_name
        hook = L['dnn_dense_1'].register_forward_hook(lambda mod, args, out: x0.append(args[0].detach().cpu()))
        logit = dm.model(ins)
        hook.remove()
        (logit * up.to(dev)).sum().backward()
        P_ = {'W1': L['dnn_dense_1'].kernel, 'gamma': L['dnn_bn_1'].gamma, 'beta': L['dnn_bn_1'].beta,
              'W2': L['dnn_dense_2'].kernel, 'b2': L['dnn_dense_2'].bias, 'W3': L['task_output'].kernel}
        legs[leg] = {'logit': logit.detach().cpu(), **{k: v.grad.detach().cpu() for k, v in P_.items()}}
        params = {k: v.detach().cpu() for k, v in P_.items()}
        bias3 = L['task_output'].bias
    assert torch.equal(x0[0], x0[1])
    leaf = {k: v.double().requires_grad_(True) for k, v in params.items()}
    h = CR.act(name, CR.batchnorm(x0[0].double() @ leaf['W1'], leaf['gamma'], leaf['beta']))
    h = CR.act(name, h @ leaf['W2'] + leaf['b2'])
    ref_logit = h @ leaf['W3'] + (0.0 if bias3 is None else bias3.detach().cpu().double())
    (ref_logit * up.double()).sum().backward()
    ref = {'logit': ref_logit.detach(), **{k: v.grad for k, v in leaf.items()}}
    figures = {k: (P.max_rel(legs['cell'][k], r) / max(P.max_rel(legs['torch'][k], r), FLOOR)) for k, r in ref.items()}
    P.record('cell_model_rate0', name=name, **figures)
    print('cell_model_rate0', name, {k: round(v, 2) for k, v in figures.items()})
    bad = {k: v for k, v in figures.items() if not (math.isfinite(v) and v <= BAR)}
    assert not bad, (name, bad)


def test_replayed_steps_draw_fresh_masks(dev, monkeypatch):
    """fit(steps_per_execution=2) on a resident feed with a dropout tower: the two steps of a replay read different seed words,
    and the next replay of the SAME captured graph different ones again — the draw is part of the graph, not a host integer
    frozen into it"""
    from deeptables_amd import ops
    from deeptables_amd.training import TableBatches
    words = []
    draw = ops.draw_cell_seed

    def recording(device):
        w = draw(device)
        words.append(w)
        return w
    monkeypatch.setattr(ops, 'draw_cell_seed', recording)
    g = torch.Generator().manual_seed(1)
    n = B * 4
    idx = torch.stack([torch.randint(0, v, (n,), generator=g) for v in VOCABS], 1).int().to(dev)
    dense = torch.randn(n, 2, generator=g).to(dev)
    y = (torch.rand(n, 1, generator=g) < 0.3).float().to(dev)
    feed = TableBatches.from_device([idx, dense], ['cat', 'cont'], y, y_ndim=2)
    dm = _model('tanh')
    torch.manual_seed(77)
    dm.fit(feed, batch_size=B, epochs=1, verbose=0, steps_per_execution=2)
    assert dm.compiled_loop is not None and dm.compiled_loop.graph is not None
    torch.cuda.synchronize()
    drawn = len(words)
    assert drawn >= 2
    first = [int(w.item()) for w in words[-2:]]               # the captured graph's two draws, as its last replay left them
    dm.fit(feed, batch_size=B, epochs=1, verbose=0, steps_per_execution=2)
    torch.cuda.synchronize()
    assert len(words) == drawn                                # replays only: no Python ran
    second = [int(w.item()) for w in words[-2:]]
    assert len(set(first + second)) == 4, (first, second)


def test_manual_seed_reproduces_a_run(dev, monkeypatch):
    """torch.manual_seed fixes the seed words, hence the masks: the same words, and the first step's loss and logits bit for bit"""
    from deeptables_amd import ops
    runs = []
    draw = ops.draw_cell_seed
    for _ in range(2):
        words = []
        monkeypatch.setattr(ops, 'draw_cell_seed', lambda device: (words.append(draw(device)), words[-1])[1])
        dm = _model('silu')
        ins, y = _batch(dev, seed=3)
        torch.manual_seed(2024)
        steps = [dm.train_step(ins, y) for _ in range(3)]
        runs.append(([int(w.item()) for w in words], steps[0][0].cpu(), steps[0][1].cpu()))
    assert len(runs[0][0]) == 3 and len(set(runs[0][0])) == 3             # one draw per forward, shared by the two cells
    assert runs[0][0] == runs[1][0]
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])
