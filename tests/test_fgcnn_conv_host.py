# -*- coding:utf-8 -*-
"""CPU: the FGCNN convolution + pooling entry points (csrc/fgcnn_train.hip) — their shape predicate at every edge of the
domain, the workspace query, the argument validation, and which path layers.FGCNN takes.  No launch happens here."""
import pytest
import torch

LINEAR, RELU, SIGMOID, TANH = 0, 1, 2, 3
BLOCK1 = (26, 16, 1, 14, 7, 2)          # (F, D, C, filters, h, pool) of the benchmark preset
BLOCK2 = (13, 16, 14, 16, 7, 2)


def lds_bytes(F, D, C, h):
    """the header's rule: the kernel padded to 16 filters and to a multiple of four channels, the bias, one batch row's
    map with the channel stride C | 1, and its dz at 20 floats per (f, d)"""
    return 64 * h * ((C + 3) // 4 * 4) + 64 + F * D * (4 * (C | 1) + 80)


def supported(h_, F, D, C, filters, h, pool, act=TANH):
    return h_.dt_fg_conv_pool_supported(F, D, C, filters, h, pool, act)


def test_the_training_entry_points_are_those_of_the_header():
    """the dt_fg_conv_ names are these five; the dt_fgcnn_ prefix stays the inference family's alone, as
    tests/test_infer_fgcnn_host.py pins it"""
    from deeptables_amd import _lib
    assert {n for n in _lib.SIGNATURES if n.startswith('dt_fg_conv_')} == {
        'dt_fg_conv_pool_supported', 'dt_fg_conv_pool_workspace_bytes', 'dt_fg_conv_pool_geometry', 'dt_fg_conv_pool_fwd',
        'dt_fg_conv_pool_bwd'}
    assert all(n.startswith('dt_fgcnn_infer') for n in _lib.SIGNATURES if n.startswith('dt_fgcnn_'))


def test_geometry_query():
    """tile rows and grid cap of both launches: inside the domain only, the backward's consistent with the workspace query,
    the forward's tile at least the backward's (it keeps no dz in LDS), either output pointer optional"""
    import ctypes
    from deeptables_amd import _lib
    h_ = _lib.lib()
    for shape in (BLOCK1, BLOCK2, (3, 4, 1, 2, 3, 2), (1, 1, 1, 1, 1, 1), (3, 4, 16, 16, 16, 8)):
        F, D, C, filters, h, pool = shape
        got = {}
        for backward in (0, 1):
            rows, cap = ctypes.c_int(-1), ctypes.c_int(-1)
            assert h_.dt_fg_conv_pool_geometry(*shape, backward, ctypes.byref(rows), ctypes.byref(cap)) == 0
            got[backward] = (rows.value, cap.value)
            assert 1 <= rows.value <= 32 and cap.value == 512
            assert lds_bytes(F, D, C, h) + (rows.value - 1) * F * D * (4 * (C | 1) + (80 if backward else 0)) <= 65536
        assert got[0][0] >= got[1][0]
        rows, cap = got[1]
        per_block = 4 * (h * C * filters + filters)
        blocks = lambda B: h_.dt_fg_conv_pool_workspace_bytes(B, *shape) // per_block
        assert blocks(rows) == 1 and blocks(rows + 1) == 2 and blocks(rows * cap + 1) == cap
        assert h_.dt_fg_conv_pool_geometry(*shape, 0, None, None) == 0
    assert h_.dt_fg_conv_pool_geometry(3, 4, 17, 4, 3, 2, 0, None, None) == -2
    assert b'dt_fg_conv_pool_geometry' in h_.dt_last_error()
    rows = ctypes.c_int(0)
    assert h_.dt_fg_conv_pool_geometry(*BLOCK2, 0, ctypes.byref(rows), None) == 0 and rows.value == 3
    assert h_.dt_fg_conv_pool_geometry(*BLOCK2, 1, ctypes.byref(rows), None) == 0 and rows.value == 2


def test_predicate_at_every_edge_of_the_domain():
    from deeptables_amd import _lib
    h_ = _lib.lib()
    assert supported(h_, *BLOCK1) == 1 and supported(h_, *BLOCK2) == 1
    assert supported(h_, 1, 1, 1, 1, 1, 1) == 1
    assert supported(h_, 3, 4, 16, 16, 16, 8) == 1                      # every limit at once
    assert supported(h_, 5, 6, 2, 4, 3, 2) == 1                         # D is no power of two
    # C / filters / h at 16 and 17, pool at 8 and 9
    assert supported(h_, 3, 4, 16, 4, 3, 2) == 1 and supported(h_, 3, 4, 17, 4, 3, 2) == 0
    assert supported(h_, 3, 4, 2, 16, 3, 2) == 1 and supported(h_, 3, 4, 2, 17, 3, 2) == 0
    assert supported(h_, 3, 4, 2, 4, 16, 2) == 1 and supported(h_, 3, 4, 2, 4, 17, 2) == 0
    assert supported(h_, 3, 4, 2, 4, 3, 8) == 1 and supported(h_, 3, 4, 2, 4, 3, 9) == 0
    # zeros and negatives, one argument at a time
    good = [3, 4, 2, 4, 3, 2]
    for k in range(6):
        for bad in (0, -1):
            shape = list(good)
            shape[k] = bad
            assert supported(h_, *shape) == 0, shape
    # the activation codes: linear, relu, sigmoid, tanh are fused, every other DT_ACT_* code and junk are not
    for act in range(-1, 12):
        assert supported(h_, *good, act=act) == (1 if act in (LINEAR, RELU, SIGMOID, TANH) else 0), act


@pytest.mark.parametrize('D,C,h', [(16, 1, 7), (16, 14, 7), (6, 3, 16), (1, 16, 16), (7, 5, 1)])
def test_predicate_follows_the_lds_rule_to_the_byte(D, C, h):
    """the largest F the rule admits is accepted, the next one refused"""
    from deeptables_amd import _lib
    h_ = _lib.lib()
    F = 1
    while lds_bytes(F + 1, D, C, h) <= 65536:
        F += 1
    assert lds_bytes(F, D, C, h) <= 65536 < lds_bytes(F + 1, D, C, h)
    assert supported(h_, F, D, C, 4, h, 2) == 1
    assert supported(h_, F + 1, D, C, 4, h, 2) == 0
    assert supported(h_, 1 << 30, D, C, 4, h, 2) == 0 and supported(h_, F, 1 << 30, C, 4, h, 2) == 0     # no overflow


def test_workspace_bytes_is_minus_one_exactly_where_the_predicate_is_zero():
    from deeptables_amd import _lib
    h_ = _lib.lib()
    shapes = [BLOCK1, BLOCK2, (1, 1, 1, 1, 1, 1), (3, 4, 16, 16, 16, 8), (3, 4, 17, 4, 3, 2), (3, 4, 2, 17, 3, 2),
              (3, 4, 2, 4, 17, 2), (3, 4, 2, 4, 3, 9), (0, 4, 2, 4, 3, 2), (3, 0, 2, 4, 3, 2), (3, 4, 0, 4, 3, 2),
              (3, 4, 2, 0, 3, 2), (3, 4, 2, 4, 0, 2), (3, 4, 2, 4, 3, 0), (2000, 16, 1, 4, 3, 2)]
    for shape in shapes:
        ok = supported(h_, *shape)
        for B in (1, 40, 8192, 1 << 33):
            n = h_.dt_fg_conv_pool_workspace_bytes(B, *shape)
            assert (n == -1) == (ok == 0), (shape, B, n)
            if ok:
                F, D, C, filters, h, pool = shape
                per_block = 4 * (h * C * filters + filters)
                assert n > 0 and n % per_block == 0
    assert h_.dt_fg_conv_pool_workspace_bytes(0, *BLOCK2) == 0
    assert h_.dt_fg_conv_pool_workspace_bytes(-1, *BLOCK2) == -1
    # the partials are per block, and the grid is capped: the size stops growing with the batch
    per_block = 4 * (7 * 14 * 16 + 16)
    sizes = [h_.dt_fg_conv_pool_workspace_bytes(B, *BLOCK2) // per_block for B in (1, 2, 3, 100, 8192, 1 << 20, 1 << 40)]
    assert sizes == sorted(sizes) and sizes[0] == 1 and sizes[-1] == sizes[-2]


def test_argument_validation_without_a_gpu():
    """a shape outside the domain, a negative batch and null pointers are refused before any launch"""
    from deeptables_amd import _lib
    h_ = _lib.lib()
    one = torch.zeros(64)
    p = _lib.ptr(one)
    fwd, bwd = h_.dt_fg_conv_pool_fwd, h_.dt_fg_conv_pool_bwd
    good = (3, 4, 2, 4, 3, 2)
    for shape in [(3, 4, 17, 4, 3, 2), (3, 4, 2, 17, 3, 2), (3, 4, 2, 4, 17, 2), (3, 4, 2, 4, 3, 9), (0, 4, 2, 4, 3, 2),
                  (2000, 16, 1, 4, 3, 2)]:
        assert fwd(p, p, p, 4, *shape, TANH, p, p, None) == -2, shape
        assert b'dt_fg_conv_pool_fwd' in h_.dt_last_error()
        assert bwd(p, p, p, p, p, 4, *shape, TANH, p, p, p, p, None) == -2, shape
        assert b'dt_fg_conv_pool_bwd' in h_.dt_last_error()
    assert fwd(p, p, p, 4, *good, 5, p, p, None) == -2                  # selu is not fused
    assert bwd(p, p, p, p, p, 4, *good, 9, p, p, p, p, None) == -2
    assert fwd(p, p, p, -1, *good, TANH, p, p, None) == -1
    assert bwd(p, p, p, p, p, -1, *good, TANH, p, p, p, p, None) == -1
    # null pointers: x, kernel, pooled are required forward (bias and sel are optional) ...
    for args in [(None, p, p, 4, *good, TANH, p, p, None), (p, None, p, 4, *good, TANH, p, p, None),
                 (p, p, p, 4, *good, TANH, None, p, None)]:
        assert fwd(*args) == -1
        assert b'null' in h_.dt_last_error()
    # ... and everything but grad_x and grad_bias backward
    full = [p, p, p, p, p, 4, *good, TANH, p, p, p, p, None]
    for k in (0, 1, 2, 3, 4, 14, 16):
        args = list(full)
        args[k] = None
        assert bwd(*args) == -1, k
        assert b'null' in h_.dt_last_error()


def test_an_empty_batch_is_a_no_op_with_every_pointer_null():
    from deeptables_amd import _lib
    h_ = _lib.lib()
    assert h_.dt_fg_conv_pool_fwd(None, None, None, 0, *BLOCK2, TANH, None, None, None) == 0
    assert h_.dt_fg_conv_pool_bwd(None, None, None, None, None, 0, *BLOCK2, TANH, None, None, None, None, None) == 0


def test_ops_wrappers_refuse_cpu_tensors():
    from deeptables_amd import _lib, ops
    x = torch.zeros(2, 3, 4, 2)
    k = torch.zeros(3, 1, 2, 4)
    assert ops.fgcnn_conv_pool_supported(x, k, 'tanh', 2) is False
    with pytest.raises(_lib.DtHipError):
        ops.fgcnn_conv_pool(x, k, None, 'tanh', 2)


# ---------------------------------------------------------------------------------------------
# layers.FGCNN: which path it takes
# ---------------------------------------------------------------------------------------------
def _layer(activation, F=5, D=6, C=2, filters=4, h=3, pool=2, nf=2):
    from deeptables_amd import functional
    from deeptables_amd.models import layers
    functional.set_seed(3)
    layer = layers.FGCNN(filters=filters, kernel_height=h, new_filters=nf, pool_height=pool, activation=activation)
    layer.build((None, F, D, C))
    with torch.no_grad():
        layer.conv_bias.add_(torch.linspace(-0.2, 0.3, filters))
    x = torch.randn(7, F, D, C, generator=torch.Generator().manual_seed(4))
    return layer, x


def _oracle(layer, x, activation, pool, nf):
    from oracle import reference_layers as R
    ws = [t.detach().double() for t in (layer.conv_kernel, layer.conv_bias, layer.dense_output.kernel,
                                        layer.dense_output.bias)]
    return R.fgcnn(x.double(), ws[0], ws[1], ws[2], ws[3], pool, nf, activation)


class _Spy:
    """stands in for ops.fgcnn_conv_pool: counts the calls and answers with the oracle's pooled map"""

    def __init__(self):
        self.calls = 0

    def __call__(self, x, kernel, bias, activation, pool_height):
        from oracle import reference_layers as R
        self.calls += 1
        filters = kernel.shape[3]
        n = x.shape[1] * x.shape[2] * 2
        pooled, _ = R.fgcnn(x.detach(), kernel.detach(), bias.detach(), torch.zeros(pooled_k(x, kernel, pool_height), n),
                            torch.zeros(n), pool_height, 2, activation)
        assert pooled.shape[3] == filters
        return pooled


def pooled_k(x, kernel, pool):
    return -(-x.shape[1] // pool) * x.shape[2] * kernel.shape[3]


def test_layer_on_cpu_tensors_keeps_the_present_path(monkeypatch):
    from deeptables_amd import ops
    monkeypatch.delenv('DT_AMD_FGCNN_CONV', raising=False)
    spy = _Spy()
    monkeypatch.setattr(ops, 'fgcnn_conv_pool', spy)
    layer, x = _layer('tanh')
    pooled, newf = layer(x)
    rp, rn = _oracle(layer, x, 'tanh', 2, 2)
    assert spy.calls == 0
    assert tuple(pooled.shape) == (7, 3, 6, 4) and tuple(newf.shape) == (7, 10, 6)
    assert (pooled.double() - rp).abs().max().item() < 1e-5 and (newf.double() - rn).abs().max().item() < 1e-5


def test_switch_and_unsupported_activation_route_to_the_present_path(monkeypatch):
    """with the shape predicate patched to accept, the layer takes the kernels — unless DT_AMD_FGCNN_CONV=0 (read per
    call) or the activation is one the kernels do not fuse"""
    from deeptables_amd import ops
    spy = _Spy()
    monkeypatch.setattr(ops, 'fgcnn_conv_pool', spy)
    monkeypatch.setattr(ops, 'fgcnn_conv_pool_supported', lambda *a: True)
    monkeypatch.delenv('DT_AMD_FGCNN_CONV', raising=False)
    layer, x = _layer('tanh')
    rp, rn = _oracle(layer, x, 'tanh', 2, 2)
    pooled, newf = layer(x)                                             # the control: this is how the kernels are reached
    assert spy.calls == 1
    assert (pooled.double() - rp).abs().max().item() < 1e-5 and (newf.double() - rn).abs().max().item() < 1e-5
    monkeypatch.setenv('DT_AMD_FGCNN_CONV', '0')
    pooled, newf = layer(x)
    assert spy.calls == 1
    assert (pooled.double() - rp).abs().max().item() < 1e-5 and (newf.double() - rn).abs().max().item() < 1e-5
    monkeypatch.setenv('DT_AMD_FGCNN_CONV', '1')
    layer(x)
    assert spy.calls == 2
    monkeypatch.delenv('DT_AMD_FGCNN_CONV')
    layer, x = _layer('selu')
    pooled, newf = layer(x)
    rp, rn = _oracle(layer, x, 'selu', 2, 2)
    assert spy.calls == 2
    assert (pooled.double() - rp).abs().max().item() < 1e-5 and (newf.double() - rn).abs().max().item() < 1e-5
