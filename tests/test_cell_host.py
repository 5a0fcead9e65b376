# -*- coding:utf-8 -*-
"""CPU: the host side of the tower cell (csrc/cell.hip, ops.cell): the new activation names against their float64
definitions, the kink derivatives, the dropout hash and its Python mirror (bit-equal, and sound as a random bit), the entry
points' argument validation, and which chains Model.__init__'s third peephole folds."""
import ctypes
import math

import pytest
import torch

from tests import cell_reference as CR


# ---- activations ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', CR.NEW_NAMES)
def test_new_activation_names_follow_their_definitions(name):
    """relu6, leaky_relu, silu, mish, hard_sigmoid, hard_silu / hard_swish raised `Unknown activation` before"""
    from deeptables_amd import functional as Fn
    fn = Fn.get_activation(name)
    x = torch.cat([torch.linspace(-9, 9, 721), torch.tensor([0.0, -0.0, 3.0, -3.0, 6.0, 1e-30, -1e-30, 30.0, -30.0])])
    x64 = x.double()
    ref = {'relu6': x64.clamp(0, 6), 'leaky_relu': torch.where(x64 > 0, x64, 0.2 * x64), 'silu': x64 / (1 + torch.exp(-x64)),
           'mish': x64 * torch.tanh(torch.log1p(torch.exp(x64))), 'hard_sigmoid': (x64 + 3).clamp(0, 6) / 6,
           'hard_silu': x64 * (x64 + 3).clamp(0, 6) / 6, 'hard_swish': x64 * (x64 + 3).clamp(0, 6) / 6}[name]
    got = fn(x).double()
    assert (got - ref).abs().max().item() <= 4 * 2.0 ** -24 * max(1.0, ref.abs().max().item())
    assert torch.equal(CR.act(name, x64), fn(x64))                    # the tests' restatement IS the registered definition
    layer = Fn.Dense(3, activation=name, name=f'cell_host_dense_{name}')
    assert layer.get_config()['activation'] == name and layer.cell_activation == name


def test_aliases_and_unknown_names():
    from deeptables_amd import functional as Fn, _lib, ops
    assert Fn.get_activation('silu') is Fn.get_activation('swish')
    assert Fn.get_activation('hard_silu') is Fn.get_activation('hard_swish')
    with pytest.raises(ValueError, match='Unknown activation'):
        Fn.get_activation('relu7')
    T = _lib.CELL_ACT_CODES
    assert T['silu'] == T['swish'] and T['hard_silu'] == T['hard_swish'] and 'softmax' not in T
    assert all(T[k] == v for k, v in _lib.ACT_CODES.items()) and max(T.values()) == _lib.DT_CELL_ACT_COUNT - 1
    assert sorted(set(T.values())) == list(range(_lib.DT_CELL_ACT_COUNT))
    # the CIN / AFM table and its message are what they were
    assert 'relu6' not in _lib.ACT_CODES and len(_lib.ACT_CODES) == 10
    with pytest.raises(ValueError, match='the HIP kernels fuse'):
        _lib.act_code('relu6', 'CIN')
    h = _lib.lib()
    for name, code in T.items():
        assert h.dt_cell_saves_input(code) == int(name in CR.INPUT_KINDS), name
        assert (code in ops._CELL_INPUT_KINDS) == (name in CR.INPUT_KINDS), name


@pytest.mark.parametrize('name', sorted(CR.KINKS))
def test_kink_derivatives_are_exact_values(name):
    """the derivative torch's CPU autograd takes AT each kink for the registered definition: the values csrc/cell.hip returns
    there (test_cell_gpu.py compares the kernel with the same table), in float32 and float64"""
    from deeptables_amd import functional as Fn
    for dtype in (torch.float32, torch.float64):
        for at, want in CR.KINKS[name].items():
            # (the registered torch ops are held to float32: F.hardsigmoid's backward multiplies by float32(1 / 6) in float64 too)
            for fn in (Fn.get_activation(name), lambda t: CR.act(name, t)) if dtype == torch.float32 else (lambda t: CR.act(name, t),):
                x = torch.tensor([at], dtype=dtype, requires_grad=True)
                (d,) = torch.autograd.grad(fn(x).sum(), x)
                assert d.item() == torch.tensor(want, dtype=dtype).item(), (name, at, dtype, d.item(), want)


# ---- the dropout hash -----------------------------------------------------------------------------------------------------
def test_the_mirror_is_the_library_s_hash_bit_for_bit():
    from deeptables_amd import _lib, ops
    h = _lib.lib()
    g = torch.Generator().manual_seed(5)
    n = 4096
    big = torch.randint(0, 2 ** 32, (n, 4), generator=g, dtype=torch.int64)
    big[: n // 4, 2:] = torch.randint(0, 2 ** 16, (n // 4, 2), generator=g)                 # small rows and columns
    big[n // 4: n // 2, 2:] = torch.randint(2 ** 16, 2 ** 20, (n // 4, 2), generator=g)      # >= 2^16
    edge = torch.tensor([[0, 0, 0, 0], [2 ** 32 - 1] * 4, [0, 0, 2 ** 31 - 1, 2 ** 31 - 1], [1, 0, 65536, 65536],
                         [0, 1, 0, 2 ** 32 - 1], [7, 9, 2 ** 31, 0]], dtype=torch.int64)
    s = torch.cat([big, edge])
    for seed, salt in {(int(a), int(b)) for a, b in s[:64, :2].tolist()} | {(0, 0), (2 ** 32 - 1, 2 ** 32 - 1)}:
        rows, cols = s[:, 2], s[:, 3]
        got = ops.cell_dropout_hash(seed, salt, rows, cols)
        want = [h.dt_cell_dropout_hash(seed, salt, int(r), int(c)) for r, c in zip(rows.tolist(), cols.tolist())][:512]
        assert got[:512].tolist() == want
    got = [int(ops.cell_dropout_hash(int(a), int(b), torch.tensor(int(r)), torch.tensor(int(c)))) for a, b, r, c in s[-40:].tolist()]
    assert got == [h.dt_cell_dropout_hash(int(a), int(b), int(r), int(c)) for a, b, r, c in s[-40:].tolist()]
    # a seed word drawn as int32 (negative values) is the same 32 bits
    assert int(ops.cell_dropout_hash(torch.tensor([-5], dtype=torch.int32), 3, torch.tensor(1), torch.tensor(2))) == \
        h.dt_cell_dropout_hash(2 ** 32 - 5, 3, 1, 2)
    # thr = rate * 2^32 saturated, at its edges
    for rate in (0.0, 1e-12, 2.0 ** -32, 2.0 ** -31, 0.1, 0.25, 0.5, 0.9, 1.0 - 2.0 ** -24, 1.0):
        assert ops.cell_dropout_threshold(rate) == h.dt_cell_dropout_threshold(rate), rate
    assert h.dt_cell_dropout_threshold(0.0) == 0 and h.dt_cell_dropout_threshold(1.0) == 2 ** 32 - 1
    assert h.dt_cell_dropout_threshold(0.5) == 2 ** 31 and h.dt_cell_dropout_threshold(2.0 ** -32) == 1
    # the keep-scale: the hash against the threshold, times fl(1 / (1 - rate))
    k = ops.cell_dropout_keep(77, 12345, 9, 7, 0.25)
    assert k.shape == (9, 7) and set(k.unique().tolist()) == {0.0, (torch.tensor(1.0) / torch.tensor(0.75)).item()}
    for r in range(9):
        for c in range(7):
            assert (h.dt_cell_dropout_hash(77, 12345, r, c) >= h.dt_cell_dropout_threshold(0.25)) == bool(k[r, c] > 0)
    assert torch.equal(ops.cell_dropout_keep(1, 2, 3, 4, 0.0), torch.ones(3, 4))
    assert torch.equal(ops.cell_dropout_keep(1, 2, 3, 4, 1.0), torch.zeros(3, 4))


@pytest.mark.parametrize('rate', [0.1, 0.5, 0.9])
def test_the_hash_is_a_sound_random_bit(rate):
    """n = 2^20 elements ([8192, 128]): the kept share, and the joint-kept share of row neighbours, column neighbours, the seeds
    s and s + 1 and two salts, each within 5 sigma of its binomial expectation (neighbours as DISJOINT pairs, so that every
    count is a sum of independent draws): a sound hash fails one of the 15 checks with a chance below 1e-5"""
    from deeptables_amd import ops
    N, C, seed, salt = 8192, 128, 20260117, ops.cell_salt('dnn_dropout_1')
    p = 1.0 - rate

    def kept(s, t):
        return ops.cell_dropout_keep(s, t, N, C, rate) > 0

    def check(what, hits, n, q):
        sigma = math.sqrt(q * (1.0 - q) / n)
        share = float(hits) / n
        print(f'rate {rate} {what}: share {share:.6f} expected {q:.6f} ({(share - q) / sigma:+.2f} sigma)')
        assert abs(share - q) <= 5.0 * sigma, (what, rate, share, q, sigma)

    a = kept(seed, salt)
    check('kept', a.sum().item(), N * C, p)
    check('row neighbours', (a[0::2] & a[1::2]).sum().item(), N * C // 2, p * p)
    check('column neighbours', (a[:, 0::2] & a[:, 1::2]).sum().item(), N * C // 2, p * p)
    check('seeds s, s + 1', (a & kept(seed + 1, salt)).sum().item(), N * C, p * p)
    check('two salts', (a & kept(seed, ops.cell_salt('dnn_dropout_2'))).sum().item(), N * C, p * p)


def test_argument_validation_returns_error_codes():
    from deeptables_amd import _lib
    h = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    seed = ctypes.cast((ctypes.c_uint32 * 1)(7), ctypes.c_void_p)
    bad = _lib.DT_CELL_ACT_COUNT
    # forward: null tensors, N <= 0, C <= 0, an unknown code, a rate outside [0, 1], a mask without its seed word, misalignment
    assert h.dt_cell_fwd(None, 4, 4, 1, 0.0, None, 0, p, None) == -1 and b'dt_cell_fwd' in h.dt_last_error()
    assert h.dt_cell_fwd(p, 4, 4, 1, 0.0, None, 0, None, None) == -1
    assert h.dt_cell_fwd(p, 0, 4, 1, 0.0, None, 0, p, None) == -1 and h.dt_cell_fwd(p, -3, 4, 1, 0.0, None, 0, p, None) == -1
    assert h.dt_cell_fwd(p, 2 ** 31, 1, 1, 0.0, None, 0, p, None) == -1 and h.dt_cell_fwd(p, 4, 0, 1, 0.0, None, 0, p, None) == -1
    assert h.dt_cell_fwd(p, 2 ** 30, 2 ** 10, 1, 0.0, None, 0, p, None) == -1                # N C = 2^40
    assert h.dt_cell_fwd(p, 4, 4, bad, 0.0, None, 0, p, None) == -1 and b'unknown activation code' in h.dt_last_error()
    assert h.dt_cell_fwd(p, 4, 4, -1, 0.0, None, 0, p, None) == -1
    assert h.dt_cell_fwd(p, 4, 4, 1, 1.5, seed, 0, p, None) == -1 and h.dt_cell_fwd(p, 4, 4, 1, -0.1, seed, 0, p, None) == -1
    assert h.dt_cell_fwd(p, 4, 4, 1, float('nan'), seed, 0, p, None) == -1
    assert h.dt_cell_fwd(p, 4, 4, 1, 0.5, None, 0, p, None) == -1 and b'seed' in h.dt_last_error()
    assert h.dt_cell_fwd(ctypes.c_void_p(p.value + 2), 4, 4, 1, 0.0, None, 0, p, None) == -1
    # backward: the same, plus which tensor was saved
    assert h.dt_cell_bwd(None, p, 0, 4, 4, 1, 0.0, None, 0, p, None) == -1 and b'dt_cell_bwd' in h.dt_last_error()
    assert h.dt_cell_bwd(p, None, 0, 4, 4, 1, 0.0, None, 0, p, None) == -1
    assert h.dt_cell_bwd(p, p, 0, 4, 4, 1, 0.0, None, 0, None, None) == -1
    assert h.dt_cell_bwd(p, p, 0, 0, 4, 1, 0.0, None, 0, p, None) == -1
    assert h.dt_cell_bwd(p, p, 0, 4, 4, bad, 0.0, None, 0, p, None) == -1
    assert h.dt_cell_bwd(p, p, 0, 4, 4, _lib.DT_CELL_ACT_GELU, 0.0, None, 0, p, None) == -1      # gelu' needs the input
    assert h.dt_cell_bwd(p, p, 0, 4, 4, 1, 0.5, seed, 0, p, None) == -1                          # a mask: the input is saved
    assert h.dt_cell_bwd(p, p, 1, 4, 4, 1, 0.5, None, 0, p, None) == -1                          # ... and the seed word is needed
    assert h.dt_cell_saves_input(bad) == -1 and h.dt_cell_saves_input(-1) == -1
    assert h.dt_cell_pass_elems() == 2048 * 256 * 4


# ---- the execution plan ---------------------------------------------------------------------------------------------------
def _tower(cells, activation, custom=False, outputs_mid=False, **params):
    from deeptables_amd import functional as Fn
    from deeptables_amd.models import deepnets
    Fn.reset_uids()
    x = Fn.Input((5,), name='cell_host_in')
    p = {'hidden_units': cells, 'activation': activation, **params}
    if custom:
        p['custom_dnn_fn'] = deepnets.custom_dnn_D_A_D_B
    h = deepnets.dnn(x, p)
    out = Fn.Dense(1, name='cell_host_out')(h)
    m = Fn.Model(x, out)
    return m, {type(n.layer).__name__ + ':' + n.layer.name: n for n in m.nodes}


def _folded(m):
    by_id = {id(n): n for n in m.nodes}
    return sorted((by_id[k].layer.name, d.name) for k, d in m._cell_fused.items())


def test_the_third_peephole_folds_activation_and_dropout():
    from deeptables_amd import functional as Fn
    # dnn cells: Dense -> (BN) -> Activation -> (Dropout)
    m, _ = _tower(((8, 0.3, True), (4, 0.5, False)), 'tanh')
    assert _folded(m) == [('dnn_activation_1', 'dnn_dropout_1'), ('dnn_activation_2', 'dnn_dropout_2')]
    assert len(m._cell_passthrough) == 2 and not m._fused_relu and not m._passthrough
    m, _ = _tower(((8, 0, True), (4, 0, False)), 'gelu')                      # no Dropout layer: nothing to fold
    assert not m._cell_fused and not m._cell_passthrough
    # relu: with BN the Activation is a launch of its own and takes its Dropout; without BN the relu stays in the GEMM (first
    # peephole, as before) and the Dropout runs alone
    m, _ = _tower(((8, 0.3, True), (4, 0.5, False)), 'relu')
    assert _folded(m) == [('dnn_activation_1', 'dnn_dropout_1')]
    assert len(m._fused_relu) == 1 and len(m._passthrough) == 1
    m, _ = _tower(((8, 0, False), (4, 0, False)), 'relu')
    assert len(m._fused_relu) == 2 and len(m._passthrough) == 2 and not m._cell_fused
    # D_A_D_B cells: Dense(activation) -> (Dropout) -> (BN)
    m, _ = _tower(((8, 0.3, True), (4, 0.5, False), (4, 0, True)), 'mish', custom=True)
    assert _folded(m) == [('dnn_custom_dense_1', 'dnn_custom_dropout_1'), ('dnn_custom_dense_2', 'dnn_custom_dropout_2')]
    m, _ = _tower(((8, 0.3, False),), 'relu', custom=True)                     # a Dense's own relu stays in its GEMM
    assert not m._cell_fused
    m, _ = _tower(((8, 0.3, False),), 'softmax', custom=True)                  # a row operation: not the cell's
    assert not m._cell_fused
    # an activity-regularised Dense keeps its own output
    m, _ = _tower(((8, 0.3, False),), 'tanh', custom=True, activity_regularizer='l2')
    assert not m._cell_fused and not m._cell_passthrough
    m, _ = _tower(((8, 0.3, False),), 'tanh', custom=True, activity_regularizer={'class_name': 'L2', 'config': {'l2': 0.0}})
    assert len(m._cell_fused) == 1
    # an intermediate that is a model output, or that feeds a second consumer, is not folded
    Fn.reset_uids()
    x = Fn.Input((5,), name='cell_host_in2')
    a = Fn.Activation('tanh', name='a')(Fn.Dense(4, name='d')(x))
    d = Fn.Dropout(0.5, name='p')(a)
    assert not Fn.Model(x, [Fn.Dense(1, name='o')(d), a])._cell_fused
    assert not Fn.Model(x, Fn.Add(name='s')([d, a]))._cell_fused
    assert len(Fn.Model(x, Fn.Dense(1, name='o2')(d))._cell_fused) == 1
    assert len(Fn.Model(x, d)._cell_fused) == 1                                # the Dropout's own output may be the model's
    sd = Fn.SpatialDropout1D(0.5, name='sp')(a)                                # overrides call: stays as it is
    assert not Fn.Model(x, sd)._cell_fused
    # a callable is never taken for the name it happens to carry
    assert Fn.Dense(3, activation=torch.tanh, name='d_callable').cell_activation is None


def test_cpu_models_run_the_torch_definitions(monkeypatch):
    """CPU tensors: the folded chain computes act then dropout with torch ops, the same layers one by one; eval mode drops nothing"""
    from deeptables_amd import functional as Fn
    m, nodes = _tower(((8, 0.5, False), (4, 0.25, False)), 'mish')        # (BatchNormalization has no CPU path)
    x = torch.randn(16, 5)
    m.eval()
    with torch.no_grad():
        y = m(x)
        h = x
        for node in m.nodes:
            h = node.layer(h)
    assert torch.equal(y, h)
    m.train()
    torch.manual_seed(3)
    y1 = m(x)
    torch.manual_seed(3)
    y2 = m(x)
    assert torch.equal(y1, y2) and not torch.equal(y1, y)
    y1.sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
