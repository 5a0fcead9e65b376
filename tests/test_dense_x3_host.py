# -*- coding:utf-8 -*-
"""CPU: the entry points of csrc/dense_tiled_x3.hip — their predicate, argument validation and geometry query — and the host
side of the Dense precision modes: which kernel family ops.dense sends a shape to in each mode, that nothing moves while no
mode is set, and who wins between the layer's argument, DT_AMD_DENSE_DTYPE and the builders' 'dense_mfma_dtype' key.  No
launch happens here: a Recorder stands in for the library."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import dense_x3_support as S
from tests import precision as P
from tests.infer_support import Recorder
from tests.test_dense_tiled_host import _FakeCuda

FWD = ['dt_dense_fwd', 'dt_dense_tiled_fwd', 'dt_dense_x3_fwd']
BWD = ['dt_dense_bwd', 'dt_dense_tiled_bwd', 'dt_dense_x3_bwd']
NEW = ['dt_dense_x3_supported', 'dt_dense_x3_workspace_bytes', 'dt_dense_x3_geometry', 'dt_dense_x3_fwd', 'dt_dense_x3_bwd']


# ---------------------------------------------------------------------------------------------------------------------
# predicate, validation, names
# ---------------------------------------------------------------------------------------------------------------------
def test_the_new_names_agree_between_header_export_and_binding():
    from deeptables_amd import _lib
    from tests.test_host_api import header_functions
    names = header_functions()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert n in names and n in _lib.SIGNATURES and hasattr(handle, n), n
    root = os.path.dirname(os.path.dirname(os.path.abspath(_lib.LIB_PATH)))
    header = open(os.path.join(root, 'include', 'dt_hip.h')).read()
    assert f'#define DT_DENSE_X3 {_lib.DT_DENSE_X3}\n' in header and f'#define DT_DENSE_BF16 {_lib.DT_DENSE_BF16}\n' in header
    assert _lib.DT_DENSE_X3 != _lib.DT_DENSE_BF16 and 0 not in (_lib.DT_DENSE_X3, _lib.DT_DENSE_BF16)


def test_predicate_at_its_edges():
    from deeptables_amd import _lib
    h = _lib.lib()
    for mode in (_lib.DT_DENSE_X3, _lib.DT_DENSE_BF16):
        for shape in [(1, 1, 2), (70, 10413, 128), (40, 64, 1300), (8192, 2912, 832), (212992, 10413, 128)]:
            assert h.dt_dense_x3_supported(*shape, mode) == 1, shape
            assert h.dt_dense_x3_workspace_bytes(*shape, mode) >= 0
        for shape in [(5, 7, 1), (8192, 429, 1), (0, 4, 4), (-1, 4, 4), (4, 0, 4), (4, -3, 4), (4, 4, 0), (4, 4, -2)]:
            assert h.dt_dense_x3_supported(*shape, mode) == 0, shape
    for mode in (0, 3, -1, 0x200):
        assert h.dt_dense_x3_supported(70, 10413, 128, mode) == 0, mode


def test_argument_validation_without_a_gpu():
    """the order and the codes of dt_dense_tiled_*: sizes, activation, (mode,) empty batch, null pointers, domain"""
    from deeptables_amd import _lib
    h = _lib.lib()
    X3, RELU, LIN = _lib.DT_DENSE_X3, _lib.DT_ACT_RELU, _lib.DT_ACT_LINEAR
    for N, K, M in [(-1, 4, 4), (4, 0, 4), (4, 4, 0), (4, -2, 4)]:
        assert h.dt_dense_x3_fwd(None, None, None, RELU, N, K, M, None, X3, None, None) == -1, (N, K, M)
        assert b'dt_dense_x3_fwd' in h.dt_last_error() and b'sizes' in h.dt_last_error()
        assert h.dt_dense_x3_bwd(None, None, None, None, RELU, N, K, M, None, None, None, X3, None, None) == -1
        assert b'dt_dense_x3_bwd' in h.dt_last_error() and b'sizes' in h.dt_last_error()
    assert h.dt_dense_x3_fwd(None, None, None, 7, 4, 4, 4, None, X3, None, None) == -1              # act
    assert b'act' in h.dt_last_error()
    assert h.dt_dense_x3_bwd(None, None, None, None, 2, 4, 4, 4, None, None, None, X3, None, None) == -1
    assert b'act' in h.dt_last_error()
    for mode in (0, 3, -1):                                                                         # mode, N = 0 included
        for N in (4, 0):
            assert h.dt_dense_x3_fwd(None, None, None, RELU, N, 4, 4, None, mode, None, None) == -1
            assert b'mode' in h.dt_last_error()
            assert h.dt_dense_x3_bwd(None, None, None, None, RELU, N, 4, 4, None, None, None, mode, None, None) == -1
            assert b'mode' in h.dt_last_error()
    for mode in (_lib.DT_DENSE_X3, _lib.DT_DENSE_BF16):
        assert h.dt_dense_x3_fwd(None, None, None, RELU, 4, 4, 4, None, mode, None, None) == -1      # null pointers
        assert b'null' in h.dt_last_error()
        assert h.dt_dense_x3_bwd(None, None, None, None, LIN, 4, 4, 4, None, None, None, mode, None, None) == -1
        assert b'null' in h.dt_last_error()
        # an empty batch is a no-op, and M == 1 belongs to the GEMV kernels of dt_dense_*
        assert h.dt_dense_x3_fwd(None, None, None, RELU, 0, 4, 4, None, mode, None, None) == 0
        assert h.dt_dense_x3_bwd(None, None, None, None, RELU, 0, 4, 4, None, None, None, mode, None, None) == 0
        p = _lib.ptr(torch.zeros(4))
        assert h.dt_dense_x3_fwd(p, p, None, LIN, 4, 1, 1, p, mode, None, None) == -2
        assert h.dt_dense_x3_bwd(p, p, p, p, LIN, 4, 1, 1, None, p, None, mode, None, None) == -2


def test_geometry_argument_validation():
    from deeptables_amd import _lib
    h = _lib.lib()
    X3 = _lib.DT_DENSE_X3
    assert h.dt_dense_x3_geometry(70, 1204, 132, X3, 0, None, None, None, None) == 0          # NULL outputs
    rows = ctypes.c_int(-1)
    assert h.dt_dense_x3_geometry(70, 1204, 132, X3, 2, ctypes.byref(rows), None, None, None) == 0 and rows.value == 64
    for shape in [(5, 7, 1), (0, 4, 4), (4, -3, 4), (4, 4, 0)]:
        rows = ctypes.c_int(-1)
        assert h.dt_dense_x3_geometry(*shape, X3, 0, ctypes.byref(rows), None, None, None) == -2, shape
        assert b'dt_dense_x3_geometry' in h.dt_last_error() and rows.value == -1
    for product in (-1, 3):
        assert h.dt_dense_x3_geometry(70, 1204, 132, X3, product, None, None, None, None) == -1
        assert b'product' in h.dt_last_error()
    assert h.dt_dense_x3_geometry(70, 1204, 132, 0, 0, None, None, None, None) == -1
    assert b'mode' in h.dt_last_error()


def _cdiv(a, b):
    return -(-a // b)


@pytest.mark.parametrize('mode', ['bf16x3', 'bf16'])
def test_the_gpu_cases_reach_the_paths_they_are_there_for(mode):
    """tests/test_dense_x3_gpu.py's shapes, asked through dt_dense_x3_geometry: every one refused by the LDS-slab kernels;
    each product once on the 128 x 128 tile with an even and with an odd row length, everything else on 64 x 64; contractions
    that are no multiple of the step and below one step in every product; ragged last tiles in both directions; grad_W
    split over the batch with a partial last step"""
    from deeptables_amd import _lib
    h = _lib.lib()
    geo = {c[:3]: tuple(S.geometry(*c[:3], mode, p) for p in (S.FWD, S.GRAD_X, S.GRAD_W)) for c in S.CASES}
    for (N, K, M), g in geo.items():
        assert h.dt_dense_supported(N, K, M) == 0, (N, K, M)
        assert all(t[0] == t[1] and t[0] in (64, 128) for t in g)
        assert g[S.FWD][2:] == (1, _cdiv(K, S.STEP)) and g[S.GRAD_X][2:] == (1, _cdiv(M, S.STEP))
        splits, per = g[S.GRAD_W][2:]
        assert (splits - 1) * per < _cdiv(N, S.STEP) <= splits * per               # every step owned once, no empty split
    for product in (S.FWD, S.GRAD_X, S.GRAD_W):
        big = [s for s, g in geo.items() if g[product][0] == 128]
        rowlen = lambda s: (s[1] if product != S.GRAD_X else s[2])               # x's / grad_y's row length
        assert {rowlen(s) % 2 for s in big} == {0, 1}, (product, big)
        assert any(g[product][0] == 64 for g in geo.values())
    contraction = {S.FWD: lambda s: s[1], S.GRAD_X: lambda s: s[2], S.GRAD_W: lambda s: s[0]}
    outputs = {S.FWD: lambda s: (s[0], s[2]), S.GRAD_X: lambda s: (s[0], s[1]), S.GRAD_W: lambda s: (s[1], s[2])}
    for product in (S.FWD, S.GRAD_X, S.GRAD_W):
        ks = [contraction[product](s) for s in geo]
        assert any(k < S.STEP for k in ks) and any(k > S.STEP and k % S.STEP for k in ks) and any(k % S.STEP == 0 for k in ks)
        for axis in (0, 1):
            assert any(outputs[product](s)[axis] % g[product][axis] for s, g in geo.items())        # a ragged last tile
            assert any(outputs[product](s)[axis] > g[product][axis] for s, g in geo.items())        # more than one tile
    for N, K, M in S.SPLIT_CASES:
        assert h.dt_dense_supported(N, K, M) == 0
        splits, per = S.geometry(N, K, M, mode, S.GRAD_W)[2:]
        assert splits > 1 and (N - (splits - 1) * per * S.STEP) % S.STEP != 0


def test_geometry_walks_a_grid_of_shapes():
    """every (tile, split) the query returns covers its output and its contraction exactly once, N K > 2^31 included"""
    for N in (1, 31, 257, 5000, 212992, 300000):
        for K in (1, 33, 1204, 10413):
            for M in (2, 65, 832, 1300):
                for product in (S.FWD, S.GRAD_X, S.GRAD_W):
                    tr, tc, splits, per = S.geometry(N, K, M, 'bf16x3', product)
                    assert S.geometry(N, K, M, 'bf16', product) == (tr, tc, splits, per)
                    Kc = (K, M, N)[product]
                    assert tr == tc and tr in (64, 128) and splits >= 1
                    assert (splits - 1) * per < _cdiv(Kc, S.STEP) <= splits * per
                    assert splits == 1 or product == S.GRAD_W


# ---------------------------------------------------------------------------------------------------------------------
# routing
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def rec(monkeypatch):
    from deeptables_amd import _lib, ops
    r = Recorder(_lib.lib(), FWD + BWD)
    monkeypatch.setattr(ops, 'lib', lambda: r)
    monkeypatch.setattr(ops, 'stream_ptr', lambda: None)
    monkeypatch.setattr(ops, 'require_cuda', lambda *a: None)
    monkeypatch.delenv('DT_AMD_DENSE_DTYPE', raising=False)
    return r


def _run(ops, N, K, M, **kw):
    x = torch.zeros(N, K, requires_grad=True)
    W = torch.zeros(K, M, requires_grad=True)
    b = torch.zeros(M, requires_grad=True)
    y = ops.dense(x, W, b, 'relu', **kw)
    assert y.shape == (N, M)
    y.sum().backward()
    assert x.grad.shape == (N, K) and W.grad.shape == (K, M) and b.grad.shape == (M,)


@pytest.mark.parametrize('mfma_dtype,const', [('bf16x3', 'DT_DENSE_X3'), ('bf16', 'DT_DENSE_BF16'), ('bfloat16', 'DT_DENSE_BF16')])
@pytest.mark.parametrize('N,K,M,tiled', [(33, 429, 128, False), (64, 39, 1, False), (257, 600, 64, True),
                                         (70, 2912, 832, True), (45, 10413, 128, True), (40, 64, 1300, True)])
def test_a_mode_moves_the_tiled_shapes_and_only_them(rec, N, K, M, tiled, mfma_dtype, const):
    from deeptables_amd import _lib, ops
    assert bool(_lib.lib().dt_dense_supported(N, K, M)) == (not tiled)
    _run(ops, N, K, M, mfma_dtype=mfma_dtype)
    if not tiled:
        assert rec.names() == ['dt_dense_fwd', 'dt_dense_bwd']        # the LDS-slab kernels, exact fp32, in every mode
        return
    assert rec.names() == ['dt_dense_x3_fwd', 'dt_dense_x3_bwd']
    (_, f), (_, b) = rec.calls
    mode = getattr(_lib, const)
    assert f[3:7] == (_lib.DT_ACT_RELU, N, K, M) and f[8] == mode and len(f) == len(_lib.SIGNATURES['dt_dense_x3_fwd'][1])
    assert b[4:8] == (_lib.DT_ACT_RELU, N, K, M) and b[11] == mode and len(b) == len(_lib.SIGNATURES['dt_dense_x3_bwd'][1])


@pytest.mark.parametrize('mfma_dtype', [None, 'float32', 'f32', 'fp32'])
@pytest.mark.parametrize('N,K,M,tiled', [(33, 429, 128, False), (257, 600, 64, True), (45, 10413, 128, True)])
def test_without_a_mode_ops_dense_makes_the_calls_it_made(rec, N, K, M, tiled, mfma_dtype):
    from deeptables_amd import _lib, ops
    _run(ops, N, K, M, **({} if mfma_dtype is None else {'mfma_dtype': mfma_dtype}))
    name = 'dt_dense_tiled' if tiled else 'dt_dense'
    assert rec.names() == [name + '_fwd', name + '_bwd']
    (_, f), (_, b) = rec.calls
    assert len(f) == len(_lib.SIGNATURES[name + '_fwd'][1]) and f[3:7] == (_lib.DT_ACT_RELU, N, K, M)
    assert len(b) == len(_lib.SIGNATURES[name + '_bwd'][1]) and b[4:8] == (_lib.DT_ACT_RELU, N, K, M)


@pytest.mark.parametrize('bad', ['fp16', 'bf16x2', 'BF16', 1, ''])
def test_a_bad_mode_raises(rec, bad):
    from deeptables_amd import functional, ops
    with pytest.raises(ValueError, match='mfma_dtype'):
        _run(ops, 45, 10413, 128, mfma_dtype=bad)
    with pytest.raises(ValueError, match='mfma_dtype'):
        functional.Dense(4, mfma_dtype=bad)
    assert rec.calls == []


# ---------------------------------------------------------------------------------------------------------------------
# the layer, the environment variable and the builders
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def all_cuda(monkeypatch):
    """every tensor says it lives on the GPU: the layers take their kernel paths, and the Recorder makes no launch"""
    monkeypatch.setattr(torch.Tensor, 'is_cuda', property(lambda self: True), raising=False)


def _dense_layer(K, M, **kw):
    from deeptables_amd import functional
    layer = functional.Dense(M, **kw)
    layer.build((None, K))
    return layer


def _modes(rec):
    """per recorded forward: None for the fp32 families, the mode constant for dt_dense_x3_fwd"""
    return [(n, a[8] if n == 'dt_dense_x3_fwd' else None) for n, a in rec.calls if n.endswith('_fwd')]


def test_layer_argument_beats_the_environment_which_is_read_per_call(rec, all_cuda, monkeypatch):
    from deeptables_amd import _lib
    x = torch.zeros(45, 1443)
    plain, pinned, exact = _dense_layer(1443, 128), _dense_layer(1443, 128, mfma_dtype='bf16'), \
        _dense_layer(1443, 128, mfma_dtype='float32')
    with torch.no_grad():
        plain(x), pinned(x), exact(x)
        monkeypatch.setenv('DT_AMD_DENSE_DTYPE', 'bf16x3')
        plain(x), pinned(x), exact(x)
        monkeypatch.setenv('DT_AMD_DENSE_DTYPE', 'bf16')
        plain(x)
        monkeypatch.delenv('DT_AMD_DENSE_DTYPE')
        plain(x)
        monkeypatch.setenv('DT_AMD_DENSE_DTYPE', 'int8')
        with pytest.raises(ValueError, match='mfma_dtype'):
            plain(x)
        pinned(x)
    T, X = 'dt_dense_tiled_fwd', 'dt_dense_x3_fwd'
    assert _modes(rec) == [(T, None), (X, _lib.DT_DENSE_BF16), (T, None),
                           (X, _lib.DT_DENSE_X3), (X, _lib.DT_DENSE_BF16), (T, None),
                           (X, _lib.DT_DENSE_BF16), (T, None), (X, _lib.DT_DENSE_BF16)]
    assert 'mfma_dtype' not in pinned.get_config() and set(pinned.get_config()) == set(plain.get_config())


def _tower(params, K, builder=None):
    from deeptables_amd import functional
    from deeptables_amd.models import deepnets
    inp = functional.Input((K,))
    out = (builder or deepnets.dnn)(inp, params, cellname='t')
    return functional.Model(inp, out)


@pytest.mark.parametrize('builder', ['dnn', 'custom_dnn_D_A_D_B'])
def test_the_builders_key_reaches_every_tower_cell_and_the_fused_towers_key_none(rec, all_cuda, builder):
    from deeptables_amd import _lib
    from deeptables_amd.models import deepnets
    cells = ((1400, 0, False), (128, 0, False), (64, 0, False))      # at N = 45: tiled, tiled, slab
    fn = getattr(deepnets, builder)
    x = torch.zeros(45, 1443)
    expect = {None: [('dt_dense_tiled_fwd', None)] * 2 + [('dt_dense_fwd', None)],
              'bf16x3': [('dt_dense_x3_fwd', _lib.DT_DENSE_X3)] * 2 + [('dt_dense_fwd', None)]}
    for params, want in (({}, None), ({'mfma_dtype': 'bf16x3'}, None), ({'mfma_dtype': 'bf16'}, None),
                         ({'dense_mfma_dtype': 'bf16x3'}, 'bf16x3'), ({'dense_mfma_dtype': 'float32'}, None)):
        model = _tower({'hidden_units': cells, **params}, 1443, fn)
        dense = [l for l in model.modules() if l.__class__.__name__ == 'Dense']
        assert len(dense) == 3 and all(l.mfma_dtype == params.get('dense_mfma_dtype') for l in dense)
        del rec.calls[:]
        with torch.no_grad():
            model(x)
        assert _modes(rec) == expect[want], params
    with pytest.raises(ValueError, match='mfma_dtype'):
        _tower({'hidden_units': cells, 'dense_mfma_dtype': 'fp8'}, 1443, fn)


def test_fgcnn_passes_its_key_to_the_recombination_dense(rec, all_cuda):
    from deeptables_amd import _lib
    from deeptables_amd.models import layers
    x = torch.zeros(70, 13 * 16 * 14)
    want = {None: ('dt_dense_tiled_fwd', None), 'bf16x3': ('dt_dense_x3_fwd', _lib.DT_DENSE_X3),
            'bf16': ('dt_dense_x3_fwd', _lib.DT_DENSE_BF16)}
    for mode, call in want.items():
        layer = layers.FGCNN(filters=14, kernel_height=7, new_filters=2, pool_height=2,
                             **({} if mode is None else {'dense_mfma_dtype': mode}))
        layer.build((None, 26, 16, 1))
        assert tuple(layer.dense_output.kernel.shape) == (2912, 832) and layer.dense_output.mfma_dtype == mode
        del rec.calls[:]
        with torch.no_grad():
            layer.dense_output(x)
        assert _modes(rec) == [call]


def test_the_fgcnn_preset_reads_both_keys_and_only_when_they_are_set():
    from deeptables_amd import functional
    from deeptables_amd.models import ModelConfig, DeepModel
    from deeptables_amd.models.metainfo import CategoricalColumn, ContinuousColumn

    def build(dnn_params, fgcnn_params):
        functional.set_seed(3)
        conf = ModelConfig(nets=['fgcnn_dnn_nets'], fixed_embedding_dim=True, embeddings_output_dim=16, embedding_dropout=0,
                           dense_dropout=0, metrics=['AUC'], dnn_params=dnn_params, fgcnn_params=fgcnn_params)
        cats = [CategoricalColumn(f'C{i}', 20 + i, 16) for i in range(6)]
        dm = DeepModel('binary', 2, conf, cats, [ContinuousColumn('input_continuous_all', ['I0', 'I1'])])
        dm.build(torch.device('cpu'))
        tower = [l.mfma_dtype for l in dm.model.modules() if l.__class__.__name__ == 'Dense' and 'dnn_dense' in l.name]
        recomb = [l.dense_output.mfma_dtype for l in dm.model.modules() if l.__class__.__name__ == 'FGCNN']
        assert len(tower) == 2 and len(recomb) == 2
        return set(tower), set(recomb)

    cells = {'hidden_units': ((128, 0, False), (64, 0, False)), 'activation': 'relu'}
    fg = {'fg_filters': (14, 16), 'fg_heights': (7, 7), 'fg_pool_heights': (2, 2), 'fg_new_feat_filters': (2, 2)}
    assert build(cells, fg) == ({None}, {None})
    assert build({**cells, 'mfma_dtype': 'bf16'}, fg) == ({None}, {None})
    assert build({**cells, 'dense_mfma_dtype': 'bf16x3'}, fg) == ({'bf16x3'}, {None})
    assert build(cells, {**fg, 'dense_mfma_dtype': 'bf16'}) == ({None}, {'bf16'})


# ---------------------------------------------------------------------------------------------------------------------
# the arithmetic the GPU test of the two modes relies on, on the numpy emulation of tests/test_split_bf16_arithmetic.py
# ---------------------------------------------------------------------------------------------------------------------
def test_the_emulated_products_separate_the_classes_at_the_shape_the_gpu_test_uses():
    from tests.test_split_bf16_arithmetic import split
    r = S.reference_for('bf16x3', 33, 1201, 128, 'relu', True)
    x, W, G = (r[k].numpy().astype(np.float32) for k in ('x', 'W', 'up'))

    def fig(a, b, parts, order):
        pa, pb = split(a, parts)[0], split(b, parts)[0]
        got = sum(pa[p].astype(np.float64) @ pb[q].astype(np.float64) for p in range(parts) for q in range(parts)
                  if p + q <= order)
        exact, scale = a.astype(np.float64) @ b.astype(np.float64), np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64)
        live = scale > 0
        return float(np.sqrt(np.mean(((got - exact)[live] / scale[live]) ** 2)))

    assert fig(x, W, 3, 2) <= P.COND_BAR['fp32'] / 10                     # six products at K = 1,201
    assert fig(x, W, 1, 0) > 4 * P.COND_BAR['b17']                        # one product: far over the three-product bar
    for a, b in ((G, W.T.copy()), (x.T.copy(), G)):                       # grad_x (contraction 128), grad_W (contraction 33)
        assert 2 * P.COND_BAR['fp32'] < fig(a, b, 2, 1) <= P.COND_BAR['b17'] / 4
        assert fig(a, b, 1, 0) > 4 * P.COND_BAR['b17']
