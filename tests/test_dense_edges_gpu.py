# -*- coding:utf-8 -*-
"""GPU: csrc/dense.hip — the LDS-slab MFMA Dense, its weight gradient and the Dense(1) kernels — at every launch path, against
the float64 reference on inputs float32 holds exactly (yardstick A of tests/precision.py, bar COND_BAR['fp32'], the claim
('dense', 'float32')).  Everything runs through the C ABI except the last test, so that the pointers, their alignment and what
lies around them are the test's to choose.  The geometry each named case of tests/dense_support.py is there to reach is
asserted through dt_dense_geometry before it runs (and without a GPU in tests/test_dense_host.py).

Which case reaches which branch (forward = k_dense_mfma<false> over Kd = K, Mo = M; grad_x = k_dense_mfma<true> over Kd = M,
Mo = K with the relu mask applied while staging; every case runs both, then k_dense_wgrad):

  k_dense_mfma                         | forward                                 | grad_x (masked)
  staging, 16-byte (Kd % 4 == 0)       | f1_n128 f2_n63 f2_n65 f2_vec f4_n32     | f1_n128 f1_n129 f2_n64 f2_vec f4_n32
  staging, 4-byte, Kd even (KS = Kd+1) | f2_n64 f2_n1 lim4 lim2 lim1             | f1_n127 f1_n1 g2_n1 lim1 lim4_gx
  staging, 4-byte, Kd odd (zero pad)   | f1_n127 f1_n129 f4_n31 f4_n33 f4_n1     | f2_n63 f2_n65 f4_n31 f4_n33 g4_n1 lim4 lim2
  staging, 16-byte shape, moved off    | test_a_misaligned_operand_changes_no_bit: f2_vec f4_n32 (x; grad_y; y)
  NBW = 1, block of 128 rows           | f1_n127 f1_n128 f1_n129 f1_n1 (N = 127, 128, 129, 1); M = 2 and 32
  NBW = 2, block of 64 rows            | f2_n63 f2_n64 f2_n65 f2_n1 (N = 63, 64, 65, 1); M = 33 (second block: one live column),
                                       | 96, 65 (three column blocks on two waves)
  NBW = 4, block of 32 rows            | f4_n31 f4_n32 f4_n33 f4_n1 (N = 31, 32, 33, 1); M = 97, 128, 129 (five blocks on four waves)
  the same block heights for grad_x    | NBW 1: f1_n127 f1_n128 g1_n129 f1_n1;  NBW 2: f2_n63 f2_n64 f2_n65 g2_n1;
                                       | NBW 4: f4_n31 f4_n32 f4_n33 g4_n1
  nch = 0 (no pipeline)                | f1_n127 (K = 31: 15 steps + the odd one), f1_n1 f2_n1 f4_n1 (K = 3, 2, 1)
  nch = 1 (has1 = has2 = false)        | f1_n128 (K = 32), f1_n129 (K = 33: chunk + the odd-tail step)
  nch = 2 (has1, no has2)              | f2_n63 f2_vec (K = 64), f2_n64 (K = 66: + one full remainder step)
  nch = 3 (second trip: no has1)       | f2_n65 (K = 96), f4_n31 (K = 97); grad_x of f2_n64 f2_vec (M = 96), f4_n31 (M = 97)
  nch = 4 (has2, then has1 only)       | f4_n32 (K = 128); grad_x of f4_n32 (M = 128), f4_n33 (M = 129)
  nch odd >= 5                         | f4_n33 (K = 161: nch = 5), lim4 (nch = 37), lim1 (nch = 9); grad_x of lim4_gx (37)
  nch even >= 6                        | lim2 (K = 598: nch = 18)
  dynamic LDS at the 150 KB limit      | lim4 (K = 1198, M = 97), lim2 (K = 598, M = 33), lim1 (K = 298, M = 2); lim4_gx (grad_x's slab)

  k_dense_wgrad                        |
  splits = 1, an empty last wave       | w_n5 (rows 2, 2, 1, 0), f1_n1 f2_n1 f4_n1 g2_n1 g4_n1 (N = 1)
  splits = 1, one full chunk per wave  | w_n128 f1_n128
  splits = 1, full chunks + a guarded  | w_n200 (50 rows per wave), f1_n129 g1_n129 lim4 lim1 (34 rows per wave)
  splits = 2, two full chunks per wave | w_n512
  splits = 2, rounded-up split         | w_n513 (264 rows per split; the last wave has 51)
  the halving loop stops at 4          | w_n1030 (two tiles: 512 -> 4)
  edge tiles (K, M no multiple of 32)  | w_n5 w_n200 w_n1030 and most of the MFMA cases
  grad_b = NULL                        | w_nogb
  grad_x = NULL, ws = NULL, linear,    | w_autoint (ops.py's AutoInt projection call)
  W and y aliased to grad_y            |
  grad_b only from kb == 0             | every case with K > 32

  Dense(1) forward                     |
  K < 64 (idle lanes), 64, 65, 129     | d1_n1_k5 d1_n33_k4 ..., d1_n3_k64, d1_n4_k65, d1_n5_k129
  N = 1, 3, 4, 5                       | d1_n1_k5 d1_n3_k64 d1_n4_k65 d1_n5_k129 (a block's waves beyond N idle)
  grid-stride loop, second trip        | d1_n16385_k8 (also d1_n32769_k8, d1_n65537_k5)
  with / without bias, relu / linear   | d1_n3_k64 d1_n98_k1028 d1_n2050_k3 d1_n65537_k5 have no bias; LINEAR_TOO

  Dense(1) backward                    |
  blocks 1, 2, 4, 5, 61, 64, 65, 129   | d1_n1_k5.., d1_n33_k4 d1_n64_k8, d1_n98_k1028, d1_n131_k63, d1_n1925_k1 (group 0 alone
                                       | takes the `i + 60 < blocks` trip), d1_n2048_k2, d1_n2050_k3, d1_n4100_k257
  last block of 1, 2, 3, 32 rows on    | d1_n33_k4 (1), d1_n98_k1028 (2), d1_n3_k64 (3), d1_n64_k8 (32): the unrolled-by-4 loop
  the 16-byte path                     | and its 1 to 3 row tail
  rows per block 33, 64                | d1_n32769_k8 (every block: 8 trips + a one-row tail), d1_n65537_k5
  16-byte path, K = 4, 8, 1028         | d1_n33_k4, d1_n64_k8 d1_n16385_k8 d1_n32769_k8, d1_n98_k1028 (second trip of the column loop)
  scalar path, K = 1, 2, 3, 5, 257     | d1_n1925_k1, d1_n2048_k2, d1_n2050_k3, d1_n1_k5 d1_n65537_k5, d1_n4100_k257 (second trip)
  scalar path by alignment alone       | test_a_misaligned_operand_changes_no_bit: d1_n64_k8 d1_n98_k1028 (x; W; grad_x; ws)
  bias column: lane 63 / own block     | d1_n131_k63 (K = 63) / d1_n3_k64 (K = 64: reduce block 1, lane 0)
  grad_x = NULL, grad_b = NULL         | d1_nogx, d1_nogb

The Dense(1) weight gradient is summed in a different order on its two column paths (four rows at a time as
(x0 g0 + x1 g1) + (x2 g2 + x3 g3) on the 16-byte path, row by row on the scalar one): where the alignment test swaps the path
it holds grad_w / grad_b to the bar and only y and grad_x to the bit.

Measured on the MI355X, cond_rms / 2^-24 over every run of this file (the bar is 2): MFMA family y <= 0.92 (g4_n1, one row),
grad_x <= 0.73, grad_W <= 0.59, grad_b <= 0.43; Dense(1) y <= 0.56, grad_x <= 0.48, grad_w <= 0.65, grad_b <= 0.56."""
import pytest
import torch

from tests import precision as P
from tests.dense_support import (ACCUMULATE, D1, D1_BWD, D1_FWD, FWD, GRAD_W, GRAD_X, GUARDED, LINEAR_TOO, MFMA, MISALIGNED,
                                 REPEATED, WGRAD, case, geometry)
from tests.test_dense_tiled_edges_gpu import (MARGIN, NAN, PATTERN, _act, _bits, _cond, _explicit, _hold_where_finite, _place,
                                              _prefill, _ref)
from tests.test_dense_tiled_gpu import _rnd

pytestmark = pytest.mark.gpu

INF = float('inf')
OUT = ('y', 'gx', 'gW', 'gb')


def _geometry_of(name):
    """the case's geometry as the query has it now, in the layout of tests/dense_support.py"""
    (N, K, M, _), _ = case(name)
    products = (D1_FWD, D1_BWD) if M == 1 else (FWD, GRAD_X, GRAD_W)
    return tuple(geometry(N, K, M, p) for p in products)


def _want(name):
    for table in (MFMA, WGRAD, D1):
        if name in table:
            return table[name][1:]


def _alloc(dev, r, off=None, margin=0, prefill=None, gx=True, gb=True, ws=True, beyond=None):
    """the operands of one forward + backward on the GPU.  off: {operand: floats past the 16-byte boundary};  margin: floats
    around every buffer (inputs' margins NaN; outputs' and the workspace's margins PATTERN);  prefill: (grad_W, grad_b) to
    accumulate onto, zeros otherwise;  beyond: a value for the first floats after x, W and grad_y (the row after the last)
    -> the tensors, the allocations they sit in, and a copy of the allocations"""
    from deeptables_amd import _lib
    off = off or {}
    N, K = r['x'].shape
    M = r['W'].shape[1]
    t, whole = {}, {}
    for name, src in (('x', r['x']), ('W', r['W']), ('b', r['b']), ('gy', r['up'])):
        t[name], whole[name] = (None, None) if src is None else _place(src, dev, off.get(name, 0), margin)
        if beyond is not None and src is not None and name != 'b':
            assert margin > 0
            first = margin + off.get(name, 0) + src.numel()
            whole[name][first:first + min(margin, src.shape[1])] = beyond
    pre_W, pre_b = prefill if prefill is not None else (torch.zeros(K, M), torch.zeros(M))
    words = (_lib.lib().dt_dense_workspace_bytes(N, K, M) + 3) // 4
    for name, src in (('y', torch.full((N, M), NAN)), ('gx', torch.full((N, K), NAN) if gx else None), ('gW', pre_W),
                      ('gb', pre_b if gb else None), ('ws', torch.full((words,), NAN) if ws else None)):
        t[name], whole[name] = (None, None) if src is None else _place(src, dev, off.get(name, 0), margin, PATTERN)
    before = {k: v.clone() for k, v in whole.items() if v is not None}
    return t, whole, before


def _fwd(t, act):
    from deeptables_amd._lib import check, lib, ptr, stream_ptr
    N, K = t['x'].shape
    M = t['W'].shape[1]
    check(lib().dt_dense_fwd(ptr(t['x']), ptr(t['W']), ptr(t['b']), _act(act), N, K, M, ptr(t['y']), stream_ptr()),
          'dt_dense_fwd')


def _bwd(t, act, gx=True, gb=True, autoint=False):
    """dt_dense_bwd on the tensors of `t`; gx / gb False: NULL in their place;  autoint: ops.py's AutoInt call — W and y
    aliased to grad_y, grad_x = NULL, ws = NULL (the caller passes act = linear)"""
    from deeptables_amd._lib import check, lib, ptr, stream_ptr
    N, K = t['x'].shape
    M = t['W'].shape[1]
    if autoint:
        assert act != 'relu'
        W = y = t['gy']
        grad_x = ws = None
    else:
        W, y, grad_x, ws = t['W'], t['y'], t['gx'] if gx else None, t['ws']
    check(lib().dt_dense_bwd(ptr(t['x']), ptr(W), ptr(y), ptr(t['gy']), _act(act), N, K, M, ptr(grad_x), ptr(t['gW']),
                             ptr(t['gb'] if gb else None), ptr(ws), stream_ptr()), 'dt_dense_bwd')
    torch.cuda.synchronize()


def _run(dev, r, act, y_edit=None, autoint=False, **kw):
    """dt_dense_fwd, then dt_dense_bwd with the upstream gradient r['up'], through ctypes (arguments: _alloc);  y_edit: applied
    to y between the two calls"""
    if autoint:
        kw = dict(kw, gx=False, ws=False)
    t, whole, before = _alloc(dev, r, **kw)
    _fwd(t, act)
    if y_edit is not None:
        y_edit(t['y'])
    _bwd(t, act, autoint=autoint)
    return t, whole, before


def _figures(r, t, prefill=None):
    """cond_rms of y, grad_x, grad_W, grad_b (those that were asked for); with a prefill the increment got - prefill on the
    scale |A| |B| + |prefill| (one more fp32 rounding of the sum, tests/test_dense_tiled_gpu.py)"""
    pre_W, pre_b = (p.double() for p in prefill) if prefill is not None else (0, 0)
    figs = {'y': ('fwd', _cond(t['y'], r['y'], r['s_y'])),
            'dW': ('bwd', _cond(t['gW'].double().cpu() - pre_W, r['dW'], r['s_W'] + abs(pre_W)))}
    if t['gx'] is not None:
        figs['dx'] = ('bwd', _cond(t['gx'], r['dx'], r['s_x']))
    if t['gb'] is not None:
        figs['db'] = ('bwd', _cond(t['gb'].double().cpu() - pre_b, r['db'], r['s_b'] + abs(pre_b)))
    return figs


def _hold(test, r, t, prefill=None):
    for name in OUT:
        assert t[name] is None or bool(torch.isfinite(t[name]).all()), name
    figs = _figures(r, t, prefill)
    print(f'{test} cond_rms / 2^-24:', {k: round(v / P.U, 3) for k, (_, v) in figs.items()})
    P.check_cond(test, 'dense', 'float32', figs)


def _acts(name):
    (_, _, _, _), opt = case(name)
    if opt.get('autoint'):
        return [None]
    return ['relu', None] if name in LINEAR_TOO else ['relu']


def _options(name):
    opt = case(name)[1]
    return {k: v for k, v in opt.items() if k in ('gx', 'gb', 'autoint')}


# ---------------------------------------------------------------------------------------------------------------------
# (a) every named case
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,act', [(n, a) for n in list(MFMA) + list(WGRAD) + list(D1) for a in _acts(n)])
def test_named_case(dev, name, act):
    assert _geometry_of(name) == _want(name)
    (N, K, M, bias), _ = case(name)
    r = _ref(N, K, M, act, bias)
    t, _, _ = _run(dev, r, act, **_options(name))
    assert all(v is None or v.data_ptr() % 16 == 0 for v in t.values())     # fresh allocations: the row length decides
    _hold(f'dense_edges[{name},{act}]', r, t)


# ---------------------------------------------------------------------------------------------------------------------
# (b) guard bands
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', GUARDED)
def test_nothing_outside_the_buffers_is_used_or_written(dev, name):
    """Every buffer sits between 64-float margins: NaN around the inputs (a clamp that lets a neighbour into a sum shows), a
    bit pattern around the outputs and around the workspace's declared size (a store past an edge shows); y and grad_x start
    as NaN (overwritten)"""
    (N, K, M, bias), _ = case(name)
    r = _ref(N, K, M, 'relu', bias)
    t, whole, before = _run(dev, r, 'relu', margin=MARGIN)
    _hold(f'dense_edges[guarded,{name}]', r, t)
    for k in ('x', 'W', 'b', 'gy'):
        assert whole[k] is None or torch.equal(_bits(whole[k]), _bits(before[k])), k
    for k in OUT + ('ws',):
        n = t[k].numel()
        for sl in (slice(0, MARGIN), slice(MARGIN + n, None)):
            assert whole[k][sl].numel() >= MARGIN
            assert bool((_bits(whole[k][sl]) == PATTERN).all()), k


# ---------------------------------------------------------------------------------------------------------------------
# (c) the accumulate / overwrite contract
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ACCUMULATE)
def test_weight_gradients_accumulate_onto_a_prefill(dev, name):
    """grad_W / grad_b = prefill + gradient (one `+=` in k_dense1_reduce, float atomics in k_dense_wgrad); then grad_x = NULL,
    grad_b = NULL once more onto the same grad_W, which leaves grad_b's bits alone"""
    (N, K, M, bias), _ = case(name)
    r = _ref(N, K, M, 'relu', bias)
    prefill = _prefill(K, M)
    t, _, _ = _run(dev, r, 'relu', prefill=prefill)
    _hold(f'dense_edges[prefilled,{name}]', r, t, prefill)
    first, gb, gx = t['gW'].clone(), t['gb'].clone(), t['gx'].clone()
    _bwd(t, 'relu', gx=False, gb=False)
    fig = P.cond_rms(t['gW'].double().cpu() - first.double().cpu(), r['dW'], r['s_W'] + first.double().cpu().abs())
    print(f'dense_edges[prefilled,{name}] second call dW cond_rms / 2^-24: {fig / P.U:.3f}')
    P.check_cond(f'dense_edges[prefilled again,{name}]', 'dense', 'float32', {'dW': ('bwd', fig)})
    assert torch.equal(_bits(t['gb']), _bits(gb)) and torch.equal(_bits(t['gx']), _bits(gx))


# ---------------------------------------------------------------------------------------------------------------------
# (d) alignment: an operand 4 bytes past its 16-byte boundary is read with 4-byte loads, and nothing else changes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', MISALIGNED)
def test_a_misaligned_operand_changes_no_bit(dev, name):
    """The load width changes how the slab is filled (k_dense_mfma) or how the columns are dealt to the threads (k_dense1_bwd),
    not the values: y and grad_x are bit-identical to the aligned run.  The MFMA family's grad_W / grad_b never depend on the
    alignment (unsplit: one atomic add onto zero per element) and are bit-identical too; Dense(1)'s grad_w / grad_b change
    their summation order with the column path and are held to the bar."""
    (N, K, M, bias), _ = case(name)
    assert K % 4 == 0 and (M % 4 == 0 or M == 1)
    if M == 1:
        operands = ('x', 'W', 'y', 'gy', 'gx', 'ws')
        same = ('y', 'gx')
    else:
        assert geometry(N, K, M, FWD)[6] == 1 and geometry(N, K, M, GRAD_X)[6] == 1 and geometry(N, K, M, GRAD_W)[1] == 1
        operands = ('x', 'W', 'y', 'gy')
        same = OUT
    r = _ref(N, K, M, 'relu', bias)
    base, _, _ = _run(dev, r, 'relu')
    _hold(f'dense_edges[aligned,{name}]', r, base)
    for moved in [(k,) for k in operands] + [operands]:
        t, _, _ = _run(dev, r, 'relu', off={k: 1 for k in moved})
        assert all(t[k].data_ptr() % 16 == 4 for k in moved)
        _hold(f'dense_edges[offset {"+".join(moved)},{name}]', r, t)
        for k in same:
            assert torch.equal(_bits(t[k]), _bits(base[k])), (moved, k)


# ---------------------------------------------------------------------------------------------------------------------
# (e) reproducibility
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', REPEATED)
def test_a_second_call_on_the_same_buffers_gives_the_same_bits(dev, name):
    """forward, grad_x, unsplit grad_W / grad_b (one atomic add onto zero per address) and all of Dense(1) (no atomics at all)
    are the same bits twice; a split grad_W's atomic order is free: held to the bar only"""
    (N, K, M, bias), _ = case(name)
    split = M > 1 and geometry(N, K, M, GRAD_W)[1] > 1
    r = _ref(N, K, M, 'relu', bias)
    t, _, _ = _run(dev, r, 'relu')
    _hold(f'dense_edges[first call,{name}]', r, t)
    first = {k: t[k].clone() for k in OUT}
    t['y'].fill_(NAN), t['gx'].fill_(NAN), t['gW'].zero_(), t['gb'].zero_()
    _fwd(t, 'relu')
    _bwd(t, 'relu')
    _hold(f'dense_edges[second call,{name}]', r, t)
    for k in OUT:
        if not (split and k in ('gW', 'gb')):
            assert torch.equal(_bits(t[k]), _bits(first[k])), k
    assert split == (name == 'w_n513')


# ---------------------------------------------------------------------------------------------------------------------
# (f) a single product
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('act', [None, 'relu'])
@pytest.mark.parametrize('N,M', [(1, 2), (129, 65), (5, 1), (131, 1)])
def test_a_single_product_is_exact(dev, N, M, act):
    """K = 1: y = act(x w (+ b)).  Without a bias that is one product, which the exact-fp32 MFMA and the Dense(1) wave both
    round once: equal to the float64 reference rounded to fp32, bit for bit.  With a bias the kernels add it to the rounded
    product — fl(fl(x w) + b), one rounding more than the reference's fl(x w + b) — so there the bits are held to that
    two-step fp32 evaluation."""
    for bias in (False, True):
        r = _ref(N, 1, M, act, bias)
        t, _, _ = _run(dev, r, act)
        got = t['y'].cpu()
        if not bias:
            assert torch.equal(got, r['y'].float())
        else:
            two_step = r['x'].float() * r['W'].float() + r['b'].float()
            two_step = torch.relu(two_step) if act == 'relu' else two_step
            print(f'K=1 [{N},{M},{act}] elements off the once-rounded reference:', int((got != r['y'].float()).sum()))
            assert torch.equal(got, two_step)


# ---------------------------------------------------------------------------------------------------------------------
# (g) hard inputs
# ---------------------------------------------------------------------------------------------------------------------
HARD = [MFMA['f4_n33'][0][:3], (131, 8, 1), (131, 63, 1)]       # NBW = 4 with a one-column last block; Dense(1) on both paths


def _hard_inputs(N, K, M):
    g = torch.Generator().manual_seed(99 + K)
    return _rnd(g, (N, K)), _rnd(g, (K, M), K ** -0.5), _rnd(g, (M,), 0.3), _rnd(g, (N, M))


@pytest.mark.parametrize('N,K,M', HARD)
def test_relu_at_exactly_zero(dev, N, K, M):
    """A row of x that is all (signed) zeros under a zero bias: the pre-activation is exactly 0.0, y is 0 there, and that row
    of grad_x is exactly 0 whether y reads +0.0 or -0.0 (the MFMA mask while staging, Dense(1)'s gs[])"""
    row = N - 2
    x, W, b, up = _hard_inputs(N, K, M)
    x[row] = 0.0
    x[row, ::2] = -0.0
    b = torch.zeros(M, dtype=torch.float64)
    b[1::2] = -0.0
    r = _explicit(x, W, b, up, 'relu')
    assert bool((r['up'][row] != 0).all())             # the upstream gradient is there; the unit is what stops it

    def negative_zeros(y):
        assert bool((y[row] == 0).all())
        y[row, ::3] = -0.0

    t, _, _ = _run(dev, r, 'relu', y_edit=negative_zeros)
    _hold(f'dense_edges[zero row,{N},{K},{M}]', r, t)
    assert bool((t['gx'][row] == 0).all())
    others = [i for i in range(N) if i != row]
    assert bool((t['gx'][others] != 0).any(1).any())


@pytest.mark.parametrize('N,K,M', HARD)
def test_a_negative_zero_or_nan_in_y_passes_no_gradient(dev, N, K, M):
    """-0.0 and NaN written over two live units of y between the two calls: `!(y > 0)` stops their gradient, as if the
    upstream gradient were zero there"""
    x, W, b, up = _hard_inputs(N, K, M)
    r0 = _explicit(x, W, b, up, 'relu')
    live = torch.nonzero((r0['y'] > 0) & (r0['up'] != 0))
    (n0, m0), (n1, m1) = live[0].tolist(), live[-1].tolist()
    assert n0 != n1
    up2 = r0['up'].clone()
    up2[n0, m0] = up2[n1, m1] = 0.0
    r = _explicit(x, W, b, up2, 'relu')
    assert not torch.equal(r['dx'], r0['dx']) and not torch.equal(r['dW'], r0['dW'])
    kept = {}

    def edit(y):
        kept['y'] = y.clone()
        y[n0, m0] = -0.0
        y[n1, m1] = NAN

    t, _, _ = _run(dev, dict(r, up=r0['up']), 'relu', y_edit=edit)
    assert torch.isnan(t['y'][n1, m1]) and t['y'][n0, m0] == 0
    t['y'] = kept['y']
    _hold(f'dense_edges[-0.0 and NaN in y,{N},{K},{M}]', r, t)


@pytest.mark.parametrize('N,K,M', HARD)
def test_an_infinite_input_stays_in_its_row(dev, N, K, M):
    """+inf in x[r, K - 1]: row r of y, and row K - 1 of grad_W (inf x G, NaN where G is 0), are all it reaches; the rows
    staged next to it in LDS, the zero pad column and the other lanes of its MFMA step stay finite"""
    row, k = N - 3, K - 1
    x, W, b, up = _hard_inputs(N, K, M)
    x[row, k] = INF
    r = _explicit(x, W, b, up, 'relu')
    assert bool(torch.isfinite(r['dx']).all()) and bool(torch.isfinite(r['db']).all())
    t, _, _ = _run(dev, r, 'relu')
    reach_y, reach_W = torch.zeros(N, M, dtype=torch.bool), torch.zeros(K, M, dtype=torch.bool)
    reach_y[row], reach_W[k] = True, True
    _hold_where_finite(f'dense_edges[inf in x,{N},{K},{M}]', r, t, {'y': reach_y, 'dW': reach_W})
    got = t['y'][row].double().cpu()
    assert torch.equal(torch.isfinite(got), torch.isfinite(r['y'][row])) and torch.equal(got, r['y'][row])


@pytest.mark.parametrize('m', [0, 128])
def test_a_nan_weight_stays_in_its_column(dev, m):
    """NaN in W[k, m]: column m of y and, through grad_x = G W^T, column k of grad_x (0 x NaN) are all it reaches; grad_W's
    column m is exactly 0 (a NaN pre-activation passes no gradient).  m = 128 is the one live column of the last 32-column
    block; m = 0 is the column that block's 31 dead lanes read in its place"""
    N, K, M = HARD[0]
    assert M == 129
    k = K - 1
    x, W, b, up = _hard_inputs(N, K, M)
    W[k, m] = NAN
    r = _explicit(x, W, b, up, 'relu')
    assert bool(torch.isfinite(r['dW']).all()) and bool((r['dW'][:, m] == 0).all())
    t, _, _ = _run(dev, r, 'relu')
    reach_y, reach_x = torch.zeros(N, M, dtype=torch.bool), torch.zeros(N, K, dtype=torch.bool)
    reach_y[:, m], reach_x[:, k] = True, True
    _hold_where_finite(f'dense_edges[nan in W column {m}]', r, t, {'y': reach_y, 'dx': reach_x})
    assert bool((t['gW'][:, m] == 0).all())


@pytest.mark.parametrize('N,K,M', HARD)
def test_an_infinity_after_the_last_row_reaches_nothing(dev, N, K, M):
    """+inf where row N of x, W and grad_y would be (inside the NaN margin): the slab's rows past N are zeros, not loads"""
    r = _explicit(*_hard_inputs(N, K, M), 'relu')
    t, whole, before = _run(dev, r, 'relu', margin=MARGIN, beyond=INF)
    assert bool(torch.isinf(whole['x'][MARGIN + N * K]))
    _hold(f'dense_edges[inf after the last row,{N},{K},{M}]', r, t)
    for k in OUT + ('ws',):
        n = t[k].numel()
        assert bool((_bits(whole[k][:MARGIN]) == PATTERN).all()) and bool((_bits(whole[k][MARGIN + n:]) == PATTERN).all()), k


# ---------------------------------------------------------------------------------------------------------------------
# (h) through ops.dense
# ---------------------------------------------------------------------------------------------------------------------
class _Spy:
    """deeptables_amd.ops' library with every dt_dense* call noted as (name, args) on its way through"""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if not name.startswith('dt_dense'):
            return fn

        def noted(*args):
            self.calls.append((name, args))
            return fn(*args)
        return noted

    def launches(self):
        return [(n, a) for n, a in self.calls if n.endswith('_fwd') or n.endswith('_bwd')]


@pytest.mark.parametrize('name,split', [('f2_n65', (5, 13)), ('d1_n64_k8', (8, 8))])
def test_ops_dense_runs_these_kernels(dev, monkeypatch, name, split):
    """ops.dense at a named case, through autograd: a 3-D input is flattened to [B * F, K], dt_dense_fwd / dt_dense_bwd are
    what runs, and an input that needs no gradient passes grad_x = NULL"""
    from deeptables_amd import _lib, ops
    (N, K, M, bias), _ = case(name)
    assert split[0] * split[1] == N and bias
    assert _geometry_of(name) == _want(name)
    spy = _Spy(_lib.lib())
    monkeypatch.setattr(ops, 'lib', lambda: spy)
    r = _ref(N, K, M, 'relu', bias)
    up = r['up'].float().to(dev).reshape(*split, M)
    for need_x in (True, False):
        spy.calls.clear()
        xd = r['x'].float().to(dev).reshape(*split, K).requires_grad_(need_x)
        Wd, bd = r['W'].float().to(dev).requires_grad_(True), r['b'].float().to(dev).requires_grad_(True)
        out = ops.dense(xd, Wd, bd, 'relu')
        assert out.shape == up.shape
        (out * up).sum().backward()
        torch.cuda.synchronize()
        (f, fa), (b, ba) = spy.launches()
        assert (f, b) == ('dt_dense_fwd', 'dt_dense_bwd')
        assert tuple(fa[4:7]) == (N, K, M) and tuple(ba[5:8]) == (N, K, M)
        assert (ba[8] is not None) == need_x                                   # grad_x
        assert (xd.grad is not None) == need_x and Wd.grad.shape == (K, M) and bd.grad.shape == (M,)
        t = {'y': out.detach().reshape(N, M), 'gx': xd.grad.reshape(N, K) if need_x else None, 'gW': Wd.grad, 'gb': bd.grad}
        _hold(f'dense_edges[ops.dense {name}, grad_x {need_x}]', r, t)
