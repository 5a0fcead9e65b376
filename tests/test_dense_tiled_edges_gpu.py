# -*- coding:utf-8 -*-
"""GPU: csrc/dense_tiled.hip at every staging path, tile size and batch split, against the float64 reference on inputs float32
holds exactly (yardstick A of tests/precision.py, bar COND_BAR['fp32']).  Everything runs through the C ABI except the last
test, so that the pointers, their alignment and what lies around them are the test's to choose.

k_dense_tiled stages each operand through one of 16 Panel paths: tile (64 | 128) x source layout (KC contraction-contiguous |
OC output-contiguous) x load width (16-byte | 4-byte) x relu mask (on | off).  Which named case of
tests/dense_tiled_support.py reaches which, always under relu — the tile is asserted through dt_dense_tiled_geometry, the
load width through the row lengths (K, M both multiples of 4, or neither) and the 16-byte alignment of every pointer:

  path                      | tile 128                | tile 64
  KC 16-byte unmasked       | fwd128_vec A = x        | gx128_vec forward A = x;  fwd128_vec grad_x B = W
  KC 16-byte masked         | gx128_vec A = grad_y,y  | fwd128_vec grad_x A = grad_y,y
  KC  4-byte unmasked       | fwd128_scalar A = x     | gx128_scalar forward A = x
  KC  4-byte masked         | gx128_scalar A          | fwd128_scalar grad_x A
  OC 16-byte unmasked       | fwd128_vec B = W;       | gx128_vec forward B = W, grad_W A = x
                            | gw128_vec A = x         |
  OC 16-byte masked         | gw128_vec B = grad_y,y  | fwd128_vec / gx128_vec grad_W B = grad_y,y
  OC  4-byte unmasked       | fwd128_scalar B;        | gx128_scalar forward B, grad_W A
                            | gw128_scalar A          |
  OC  4-byte masked         | gw128_scalar B          | fwd128_scalar / gx128_scalar grad_W B
  (KC unmasked is also grad_x's B = W read transposed: gx128_* at tile 128.)

The alignment test then moves one operand at a time off its 16-byte boundary (row lengths still multiples of 4), which swaps
that operand's 16-byte path for the 4-byte one and must not change one bit of the result."""
import functools

import pytest
import torch

from tests import precision as P
from tests.dense_tiled_support import DEGENERATE, FWD, GRAD_W, GRAD_X, ONE_BIG_TILE, SMALL_TILE, SPLIT, geometry
from tests.test_dense_tiled_gpu import _call_bwd, _reference, _rnd

pytestmark = pytest.mark.gpu

BAR = P.COND_BAR['fp32']
NAN = float('nan')
MARGIN = 64                   # floats on each side of a guarded buffer
PATTERN = 0x7FA5C3E1          # the bits of an output margin: a NaN payload no arithmetic produces


def _act(act):
    from deeptables_amd import _lib
    return _lib.DT_ACT_RELU if act == 'relu' else _lib.DT_ACT_LINEAR


@functools.lru_cache(maxsize=None)
def _ref(N, K, M, act, bias):
    """_reference of tests/test_dense_tiled_gpu.py, once per shape, with grad_b's reference also where the forward has no
    bias (the C ABI computes it either way).  Shared between tests: nobody writes to it."""
    r = _reference(torch.Generator().manual_seed(7 * N + K + M), N, K, M, act, bias)
    if r['db'] is None:
        G = r['up'] * (r['y'] > 0) if act == 'relu' else r['up']
        r['db'], r['s_b'] = G.sum(0), G.abs().sum(0)
    return r


def _explicit(x, W, b, up, act):
    """the same float64 reference written out product by product, for inputs with zeros and non-finite values:
    G = up where the pre-activation is > 0 (a NaN or zero pre-activation passes no gradient, as tl_dact has it)"""
    pre, s_y = x @ W + b, x.abs() @ W.abs() + b.abs()
    up = P.kink_mask(pre, s_y, up, act, 'fp32')
    G = torch.where(pre > 0, up, torch.zeros_like(up)) if act == 'relu' else up
    return dict(x=x, W=W, b=b, up=up, y=torch.relu(pre) if act == 'relu' else pre, dx=G @ W.t(), dW=x.t() @ G, db=G.sum(0),
                s_y=s_y, s_x=G.abs() @ W.abs().t(), s_W=x.abs().t() @ G.abs(), s_b=G.abs().sum(0))


def _place(t, dev, off=0, margin=0, bits=None):
    """float32 copy of `t` on the GPU, `off` floats past a 16-byte boundary inside a larger allocation whose other floats are
    NaN (bits = None) or the bit pattern `bits` -> (the tensor, the whole allocation)"""
    assert margin % 4 == 0
    n = t.numel()
    whole = torch.empty(2 * margin + n + 4, dtype=torch.float32, device=dev)
    if bits is None:
        whole.fill_(NAN)
    else:
        whole.view(torch.int32).fill_(bits)
    assert whole.data_ptr() % 16 == 0
    view = whole[margin + off:margin + off + n].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 * off and view.is_contiguous()
    return view, whole


def _bits(t):
    return t.view(torch.int32)


def _run(dev, r, act, off=None, margin=0, prefill=None, y_edit=None):
    """dt_dense_tiled_fwd, then dt_dense_tiled_bwd with the upstream gradient r['up'], through ctypes.
    off: {operand: floats past the 16-byte boundary} for x, W, y, gy;  margin: floats around every buffer (inputs' margins NaN,
    outputs' margins PATTERN, and the two overwritten outputs NaN before the launch);  prefill: (grad_W, grad_b) to accumulate
    onto, zeros otherwise;  y_edit: applied to y between the two calls.  -> the tensors, and the allocations they sit in"""
    from deeptables_amd import _lib
    from deeptables_amd._lib import check, ptr, stream_ptr
    h, off = _lib.lib(), off or {}
    N, K = r['x'].shape
    M = r['W'].shape[1]
    t, whole = {}, {}
    for name, src in (('x', r['x']), ('W', r['W']), ('b', r['b']), ('gy', r['up'])):
        t[name], whole[name] = (None, None) if src is None else _place(src, dev, off.get(name, 0), margin)
    pre_W, pre_b = prefill if prefill is not None else (torch.zeros(K, M), torch.zeros(M))
    for name, src in (('y', torch.full((N, M), NAN)), ('gx', torch.full((N, K), NAN)), ('gW', pre_W), ('gb', pre_b)):
        t[name], whole[name] = _place(src, dev, off.get(name, 0), margin, PATTERN)
    before = {k: v.clone() for k, v in whole.items() if v is not None}
    check(h.dt_dense_tiled_fwd(ptr(t['x']), ptr(t['W']), ptr(t['b']), _act(act), N, K, M, ptr(t['y']), stream_ptr()),
          'dt_dense_tiled_fwd')
    if y_edit is not None:
        y_edit(t['y'])
    _call_bwd(h, t['x'], t['W'], t['y'], t['gy'], _act(act), t['gx'], t['gW'], t['gb'])
    return t, whole, before


def _cond(got, ref, scale):
    """P.cond_rms; a scale that is zero everywhere (no live relu unit in a degenerate shape: every term of every sum is zero)
    asks for exact zeros instead"""
    if not bool((scale > 0).any()):
        assert bool((P._d(got) == 0).all()) and bool((ref == 0).all())
        return 0.0
    return P.cond_rms(got, ref, scale)


def _figures(r, t, prefill=None):
    """cond_rms of y, grad_x, grad_W, grad_b; with a prefill the increment got - prefill on the scale |A| |B| + |prefill| (one
    more fp32 rounding of the sum, tests/test_dense_tiled_gpu.py)"""
    pre_W, pre_b = (p.double() for p in prefill) if prefill is not None else (0, 0)
    return {'y': ('fwd', _cond(t['y'], r['y'], r['s_y'])),
            'dx': ('bwd', _cond(t['gx'], r['dx'], r['s_x'])),
            'dW': ('bwd', _cond(t['gW'].double().cpu() - pre_W, r['dW'], r['s_W'] + abs(pre_W))),
            'db': ('bwd', _cond(t['gb'].double().cpu() - pre_b, r['db'], r['s_b'] + abs(pre_b)))}


def _hold(test, r, t, prefill=None):
    for name in ('y', 'gx', 'gW', 'gb'):
        assert bool(torch.isfinite(t[name]).all()), name
    figs = _figures(r, t, prefill)
    print(f'{test} cond_rms / 2^-24:', {k: round(v / P.U, 3) for k, (_, v) in figs.items()})
    P.check_cond(test, 'dense', 'float32', figs)


def _prefill(K, M, seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((K, M), generator=g), torch.randn((M,), generator=g)


# ---------------------------------------------------------------------------------------------------------------------
# (a) one product at 128 x 128 at a time, both load widths, relu
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', sorted(ONE_BIG_TILE))
def test_one_product_on_the_big_tile(dev, case):
    (N, K, M, bias), want = ONE_BIG_TILE[case]
    assert tuple(geometry(N, K, M, p) for p in (FWD, GRAD_X, GRAD_W)) == want
    vec = case.endswith('_vec')
    assert (K % 4 == 0 and M % 4 == 0) if vec else (K % 4 != 0 and M % 4 != 0)
    r = _ref(N, K, M, 'relu', bias)
    t, _, _ = _run(dev, r, 'relu')
    assert all(v is None or v.data_ptr() % 16 == 0 for v in t.values())     # fresh allocations: the row length decides
    _hold(f'dense_tiled_edges[{case}]', r, t)


# ---------------------------------------------------------------------------------------------------------------------
# (b) alignment: an operand 4 bytes past its 16-byte boundary is staged with 4-byte loads, and nothing else changes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,K,M,bias', [(70, 1204, 132, True), ONE_BIG_TILE['gx128_vec'][0]])
def test_a_misaligned_operand_changes_no_bit(dev, N, K, M, bias):
    """The load width changes how a panel is filled, not the values in it nor the order of the MFMA chain: y, grad_x, and
    grad_W / grad_b where the batch is not split (one `+=` / one atomic add onto zero), are bit-identical to the aligned run."""
    assert K % 4 == 0 and M % 4 == 0
    if (N, K, M) in SMALL_TILE:
        assert tuple(geometry(N, K, M, p) for p in (FWD, GRAD_X, GRAD_W)) == SMALL_TILE[(N, K, M)]
    else:
        assert geometry(N, K, M, GRAD_X)[0] == 128
    unsplit = geometry(N, K, M, GRAD_W)[1] == 1
    r = _ref(N, K, M, 'relu', bias)
    base, _, _ = _run(dev, r, 'relu')
    _hold(f'dense_tiled_edges[aligned,{N},{K},{M}]', r, base)
    same = ('y', 'gx') + (('gW', 'gb') if unsplit else ())
    for moved in (('x',), ('W',), ('y',), ('gy',), ('x', 'W', 'y', 'gy')):
        t, _, _ = _run(dev, r, 'relu', off={name: 1 for name in moved})
        _hold(f'dense_tiled_edges[offset {"+".join(moved)},{N},{K},{M}]', r, t)
        for name in same:
            assert torch.equal(_bits(t[name]), _bits(base[name])), (moved, name)


# ---------------------------------------------------------------------------------------------------------------------
# (c) the atomic batch split, onto a non-zero grad_W / grad_b
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,K,M', sorted(SPLIT))
def test_split_batch_accumulates_onto_a_prefill(dev, N, K, M):
    """grad_W / grad_b = prefill + gradient through float atomics over blockIdx.z; then grad_x = NULL, grad_b = NULL once more
    onto the same grad_W.  The order of an atomic sum is free: nothing here is compared bit for bit between runs."""
    from deeptables_amd._lib import lib
    splits, per, last_rows = SPLIT[(N, K, M)]
    assert geometry(N, K, M, GRAD_W)[1:] == (splits, per) and splits > 1
    assert N - (splits - 1) * per * 32 == last_rows and 0 < last_rows <= per * 32
    r = _ref(N, K, M, 'relu', True)
    prefill = _prefill(K, M)
    t, _, _ = _run(dev, r, 'relu', prefill=prefill)
    _hold(f'dense_tiled_edges[split {splits},{N},{K},{M}]', r, t, prefill)
    first, gb = t['gW'].clone(), t['gb'].clone()
    _call_bwd(lib(), t['x'], t['W'], t['y'], t['gy'], _act('relu'), None, t['gW'], None)
    fig = P.cond_rms(t['gW'].double().cpu() - first.double().cpu(), r['dW'], r['s_W'] + first.double().cpu().abs())
    print(f'dense_tiled_edges[split {splits},{N},{K},{M}] second call dW cond_rms / 2^-24: {fig / P.U:.3f}')
    P.check_cond(f'dense_tiled_edges[split {splits} again,{N},{K},{M}]', 'dense', 'float32', {'dW': ('bwd', fig)})
    assert torch.equal(_bits(t['gb']), _bits(gb))


# ---------------------------------------------------------------------------------------------------------------------
# (d) guard bands
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,K,M', [(67, 133, 69), (70, 1204, 132), ONE_BIG_TILE['gw128_scalar'][0][:3]])
def test_nothing_outside_the_matrices_is_used_or_written(dev, N, K, M):
    """Every buffer sits between 64-float margins: NaN around the inputs (a clamp that lets a neighbour into the sum shows),
    a bit pattern around the outputs (a store past an edge tile shows); y and grad_x start as NaN (overwritten)"""
    r = _ref(N, K, M, 'relu', True)
    t, whole, before = _run(dev, r, 'relu', margin=MARGIN)
    _hold(f'dense_tiled_edges[guarded,{N},{K},{M}]', r, t)
    for name in ('x', 'W', 'b', 'gy'):
        assert torch.equal(_bits(whole[name]), _bits(before[name])), name
    for name in ('y', 'gx', 'gW', 'gb'):
        n = t[name].numel()
        for sl in (slice(0, MARGIN), slice(MARGIN + n, None)):
            assert whole[name][sl].numel() >= MARGIN
            assert bool((_bits(whole[name][sl]) == PATTERN).all()), name


# ---------------------------------------------------------------------------------------------------------------------
# (e) degenerate extents
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('act', [None, 'relu'])
@pytest.mark.parametrize('N,K,M', DEGENERATE)
def test_degenerate_extents(dev, N, K, M, act):
    from deeptables_amd._lib import lib
    assert lib().dt_dense_tiled_supported(N, K, M) == 1
    r = _ref(N, K, M, act, True)
    t, _, _ = _run(dev, r, act, margin=MARGIN)
    _hold(f'dense_tiled_edges[{N},{K},{M},{act}]', r, t)


@pytest.mark.parametrize('act', [None, 'relu'])
@pytest.mark.parametrize('N,M', [(1, 2), (129, 65)])
def test_a_single_product_is_exact(dev, N, M, act):
    """K = 1: y = act(x w (+ b)).  Without a bias that is one product, which the exact-fp32 MFMA rounds once: equal to the
    float64 reference rounded to fp32, bit for bit.  With a bias the kernel adds it to the rounded product — fl(fl(x w) + b),
    one rounding more than the reference's fl(x w + b) — so there the bits are held to that two-step fp32 evaluation."""
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
# (f) special values
# ---------------------------------------------------------------------------------------------------------------------
SP = (70, 1204, 132)


def _special_inputs():
    N, K, M = SP
    g = torch.Generator().manual_seed(99)
    return _rnd(g, (N, K)), _rnd(g, (K, M), K ** -0.5), _rnd(g, (M,), 0.3), _rnd(g, (N, M))


def test_relu_at_exactly_zero(dev):
    """A row of x that is all (signed) zeros under a zero bias: y is 0 there, that row of grad_x is exactly 0 whether y reads
    +0.0 or -0.0, and grad_W / grad_b are those of the batch without the row"""
    N, K, M = SP
    row = 37
    x, W, b, up = _special_inputs()
    x[row] = 0.0
    x[row, ::2] = -0.0
    b = torch.zeros(M, dtype=torch.float64)
    b[1::2] = -0.0
    r = _explicit(x, W, b, up, 'relu')

    def negative_zeros(y):
        assert bool((y[row] == 0).all())
        y[row, ::3] = -0.0

    t, _, _ = _run(dev, r, 'relu', y_edit=negative_zeros)
    _hold('dense_tiled_edges[zero row]', r, t)
    assert bool((t['gx'][row] == 0).all())
    keep = [i for i in range(N) if i != row]
    r1 = _explicit(x[keep], W, b, up[keep], 'relu')
    assert torch.equal(r1['dW'], r['dW']) or P.cond_rms(r1['dW'], r['dW'], r['s_W']) < 2.0 ** -50    # the reference agrees
    t1, _, _ = _run(dev, r1, 'relu')
    _hold('dense_tiled_edges[zero row removed]', r1, t1)
    # grad_W (unsplit: plain +=) is one fmaf chain over the batch index per element: an exact-zero term leaves the accumulator
    # as it is, and taking it out moves the later terms up without reordering them -> the same bits.  grad_b's column sum is
    # kept as two partial sums (even and odd batch rows of each step), which the missing row re-deals: there the two runs
    # are two fp32 evaluations of one sum, within the class of each other.
    assert geometry(N, K, M, GRAD_W)[1] == 1
    assert torch.equal(_bits(t['gW']), _bits(t1['gW']))
    assert P.cond_rms(t['gb'], t1['gb'], r['s_b']) <= BAR


def _hold_where_finite(test, r, t, allowed):
    """allowed: {figure: bool mask of the elements the special value may reach}.  Outside it the kernel is finite wherever the
    reference is, and those elements meet the bar; the kernel is non-finite nowhere but inside it or where the reference is"""
    figs = {}
    for name, got, ref, scale, d in (('y', t['y'], r['y'], r['s_y'], 'fwd'), ('dx', t['gx'], r['dx'], r['s_x'], 'bwd'),
                                     ('dW', t['gW'], r['dW'], r['s_W'], 'bwd'), ('db', t['gb'], r['db'], r['s_b'], 'bwd')):
        got = got.double().cpu()
        reach = allowed.get(name, torch.zeros_like(ref, dtype=torch.bool)) | ~torch.isfinite(ref)
        assert bool(torch.isfinite(got[~reach]).all()), name
        live = ~reach & torch.isfinite(scale)
        zero = torch.zeros_like(ref)
        figs[name] = (d, P.cond_rms(torch.where(live, got, zero), torch.where(live, ref, zero), torch.where(live, scale, zero)))
    print(f'{test} cond_rms / 2^-24:', {k: round(v / P.U, 3) for k, (_, v) in figs.items()})
    P.check_cond(test, 'dense', 'float32', figs)


def test_an_infinite_input_stays_in_its_row(dev):
    """+inf in x[r, k]: row r of y, and row k of grad_W (inf x G, NaN where G is 0), are all it reaches; the zero padding of
    the edge tiles multiplies it only into columns that are never stored"""
    N, K, M = SP
    row, k = 41, 1203
    x, W, b, up = _special_inputs()
    x[row, k] = float('inf')
    r = _explicit(x, W, b, up, 'relu')
    assert bool(torch.isfinite(r['dx']).all()) and bool(torch.isfinite(r['db']).all())
    t, _, _ = _run(dev, r, 'relu')
    reach_y, reach_W = torch.zeros(N, M, dtype=torch.bool), torch.zeros(K, M, dtype=torch.bool)
    reach_y[row], reach_W[k] = True, True
    _hold_where_finite('dense_tiled_edges[inf in x]', r, t, {'y': reach_y, 'dW': reach_W})
    # where the reference of row r is finite (relu of -inf = 0) the kernel has the same 0; elsewhere it is +inf as well
    got = t['y'][row].double().cpu()
    assert torch.equal(torch.isfinite(got), torch.isfinite(r['y'][row])) and torch.equal(got, r['y'][row])


def test_a_nan_weight_stays_in_its_column(dev):
    """NaN in W[k, m]: column m of y and, through grad_x = G W^T, column k of grad_x (0 x NaN) are all it reaches; grad_W's
    column m is the reference's exact 0 (a NaN pre-activation passes no gradient)"""
    N, K, M = SP
    k, m = 1201, 131
    x, W, b, up = _special_inputs()
    W[k, m] = NAN
    r = _explicit(x, W, b, up, 'relu')
    assert bool(torch.isfinite(r['dW']).all()) and bool((r['dW'][:, m] == 0).all())
    t, _, _ = _run(dev, r, 'relu')
    reach_y, reach_x = torch.zeros(N, M, dtype=torch.bool), torch.zeros(N, K, dtype=torch.bool)
    reach_y[:, m], reach_x[:, k] = True, True
    _hold_where_finite('dense_tiled_edges[nan in W]', r, t, {'y': reach_y, 'dx': reach_x})
    assert bool((t['gW'][:, m] == 0).all())


# ---------------------------------------------------------------------------------------------------------------------
# (g) through ops.dense
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('how', ['3d', 'transposed'])
def test_ops_dense_flattens_and_packs_before_the_tiled_kernel(dev, how):
    from deeptables_amd import ops
    from deeptables_amd._lib import lib
    N, K, M = SP
    assert lib().dt_dense_supported(N, K, M) == 0 and lib().dt_dense_tiled_supported(N, K, M) == 1
    r = _ref(N, K, M, 'relu', True)
    if how == '3d':
        xd = r['x'].float().to(dev).reshape(7, 10, K).requires_grad_(True)
        up = r['up'].float().to(dev).reshape(7, 10, M)
    else:
        xd = r['x'].float().t().contiguous().to(dev).t().requires_grad_(True)
        assert not xd.is_contiguous() and xd.shape == (N, K)
        up = r['up'].float().to(dev)
    Wd, bd = r['W'].float().to(dev).requires_grad_(True), r['b'].float().to(dev).requires_grad_(True)
    out = ops.dense(xd, Wd, bd, 'relu')
    assert out.shape == up.shape
    (out * up).sum().backward()
    assert xd.grad.shape == xd.shape and Wd.grad.shape == (K, M) and bd.grad.shape == (M,)
    t = {'y': out.detach().reshape(N, M), 'gx': xd.grad.reshape(N, K), 'gW': Wd.grad, 'gb': bd.grad}
    _hold(f'dense_tiled_edges[ops.dense {how}]', r, t)
