# -*- coding:utf-8 -*-
"""GPU: the tiled Dense on the bf16 matrix cores (csrc/dense_tiled_x3.hip) held to the classes its two modes claim
(tests/dense_x3_support.CLAIM: 'bf16x3' -> fp32 forward, b17 backward; 'bf16' -> bf16 both; grad_b fp32 in both), to
dt_dense_bwd's overwrite / accumulate contract through the C ABI with guard bands around every buffer, to the fp32
kernel's reach of a non-finite operand, and told apart from each other by the bars of the neighbouring class.

Yardstick A as tests/test_dense_tiled_gpu.py::_reference builds it; the kink mask has the width of the forward's class, and
the share of units it zeroes is capped on the reference before any kernel runs (dense_x3_support.MASK_CAP)."""
import pytest
import torch

from tests import dense_x3_support as S
from tests import precision as P

pytestmark = pytest.mark.gpu

MODES = ['bf16x3', 'bf16']


def _figures(mode, r, y, dx, dW, db):
    figs = {'y': (P.cond_rms(y, r['y'], r['s_y']), S.CLAIM[mode][0]),
            'dx': (P.cond_rms(dx, r['dx'], r['s_x']), S.CLAIM[mode][1]),
            'dW': (P.cond_rms(dW, r['dW'], r['s_W']), S.CLAIM[mode][1])}
    if db is not None:
        figs['db'] = (P.cond_rms(db, r['db'], r['s_b']), S.GRAD_B_CLASS)
    return figs


def _hold(tag, figs):
    print(f'{tag} cond_rms / 2^-24:', {k: round(v / P.U, 3) for k, (v, _) in figs.items()})
    bad = {k: (v / P.U, P.COND_BAR[c] / P.U) for k, (v, c) in figs.items() if not v <= P.COND_BAR[c]}
    assert not bad, f'{tag}: cond_rms in units of 2^-24 (measured, bar): {bad}'


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('N,K,M,act,bias', S.CASES)
def test_dense_x3_holds_the_class_of_its_mode(dev, N, K, M, act, bias, mode):
    from deeptables_amd import ops
    from deeptables_amd._lib import lib
    assert lib().dt_dense_supported(N, K, M) == 0          # the LDS-slab kernels cannot be what answers
    assert lib().dt_dense_x3_supported(N, K, M, S.mode_code(mode)) == 1
    act = S.act_in_mode(mode, K, act)
    r = S.reference_for(mode, N, K, M, act, bias)
    assert r['masked'] <= S.MASK_CAP[mode], (mode, r['masked'])
    xd, Wd = r['x'].float().to(dev).requires_grad_(True), r['W'].float().to(dev).requires_grad_(True)
    bd = r['b'].float().to(dev).requires_grad_(True) if bias else None
    out = ops.dense(xd, Wd, bd, act, mfma_dtype=mode)
    (out * r['up'].float().to(dev)).sum().backward()
    _hold(f'dense_x3[{mode},{N},{K},{M},{act},{bias}]', _figures(mode, r, out, xd.grad, Wd.grad, bd.grad if bias else None))


# ---------------------------------------------------------------------------------------------------------------------
# the contract through the C ABI, with 64-float guard bands: NaN around the inputs, a bit pattern around the outputs
# ---------------------------------------------------------------------------------------------------------------------
BAND = 64
PATTERN = 0x5A5AA5A5


def _banded(t, dev, output):
    """`t` inside a buffer with BAND floats on either side -> (buffer, view of the middle)"""
    buf = torch.empty(t.numel() + 2 * BAND, dtype=torch.float32, device=dev)
    if output:
        buf.view(torch.int32).fill_(PATTERN)
    else:
        buf.fill_(float('nan'))
    mid = buf[BAND:BAND + t.numel()].view(t.shape)
    mid.copy_(t)
    return buf, mid


def _bands_intact(buf, output):
    ends = torch.cat([buf[:BAND], buf[-BAND:]])
    if output:
        return bool((ends.view(torch.int32) == PATTERN).all())
    return bool(torch.isnan(ends).all())


def _fwd(h, mode, x, W, b, y, act):
    from deeptables_amd._lib import check, ptr, stream_ptr
    N, K = x.shape
    check(h.dt_dense_x3_fwd(ptr(x), ptr(W), ptr(b), act, N, K, W.shape[1], ptr(y), S.mode_code(mode), None, stream_ptr()),
          'dt_dense_x3_fwd')


def _bwd(h, mode, x, W, y, gy, act, gx, gW, gb):
    from deeptables_amd._lib import check, ptr, stream_ptr
    N, K = x.shape
    M = W.shape[1]
    nbytes = h.dt_dense_x3_workspace_bytes(N, K, M, S.mode_code(mode))
    ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=x.device) if nbytes > 0 else None
    check(h.dt_dense_x3_bwd(ptr(x), ptr(W), ptr(y), ptr(gy), act, N, K, M, ptr(gx), ptr(gW), ptr(gb), S.mode_code(mode),
                            ptr(ws), stream_ptr()), 'dt_dense_x3_bwd')
    torch.cuda.synchronize()


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('N,K,M', [(40, 301, 5), (33, 1201, 128)] + S.SPLIT_CASES)
def test_bwd_overwrites_grad_x_accumulates_the_weight_gradients_and_stays_inside_its_buffers(dev, N, K, M, mode):
    """grad_W / grad_b come back as prefill + gradient (for the split cases: merged with atomics onto a random prefill, and a
    second time onto the result), a NaN-filled grad_x comes back finite, grad_x = NULL / grad_b = NULL are accepted, and
    no guard band is touched"""
    from deeptables_amd import _lib
    h = _lib.lib()
    if (N, K, M) in S.SPLIT_CASES:
        assert S.geometry(N, K, M, mode, S.GRAD_W)[2] > 1
    fc, bc = S.CLAIM[mode]
    r = S.reference_for(mode, N, K, M, 'relu', True)
    assert r['masked'] <= S.MASK_CAP[mode]
    ins = {k: _banded(r[k].float(), dev, False) for k in ('x', 'W', 'b', 'up')}
    x, W, b, gy = (ins[k][1] for k in ('x', 'W', 'b', 'up'))
    ybuf, y = _banded(torch.zeros(N, M), dev, True)
    _fwd(h, mode, x, W, b, y, _lib.DT_ACT_RELU)
    g = torch.Generator().manual_seed(3)
    pre_W, pre_b = torch.randn((K, M), generator=g), torch.randn((M,), generator=g)
    gxbuf, gx = _banded(torch.full((N, K), float('nan')), dev, True)
    gWbuf, gW = _banded(pre_W, dev, True)
    gbbuf, gb = _banded(pre_b, dev, True)
    _bwd(h, mode, x, W, y, gy, _lib.DT_ACT_RELU, gx, gW, gb)
    assert bool(torch.isfinite(gx).all())
    assert P.cond_rms(y, r['y'], r['s_y']) <= P.COND_BAR[fc]
    assert P.cond_rms(gx, r['dx'], r['s_x']) <= P.COND_BAR[bc]
    # the sum adds one fp32 rounding of at most 2^-24 (|prefill| + |gradient|) to the gradient's own error: on the scale
    # |prefill| + |A| |B| the root mean square stays inside the class
    for got, pre, ref, scale, cls in ((gW, pre_W, r['dW'], r['s_W'], bc), (gb, pre_b, r['db'], r['s_b'], S.GRAD_B_CLASS)):
        pre = pre.double()
        fig = P.cond_rms(got.double().cpu() - pre, ref, scale + pre.abs())
        print(f'dense_x3 contract[{mode},{N},{K},{M}] prefill + gradient / 2^-24: {fig / P.U:.3f}')
        assert fig <= P.COND_BAR[cls]
    # grad_x = NULL and grad_b = NULL: the weight gradient alone, accumulated once more onto the same buffer
    first = gW.double().cpu()
    _bwd(h, mode, x, W, y, gy, _lib.DT_ACT_RELU, None, gW, None)
    assert P.cond_rms(gW.double().cpu() - first, r['dW'], r['s_W'] + first.abs()) <= P.COND_BAR[bc]
    for name, (buf, _) in ins.items():
        assert _bands_intact(buf, False), name
    for name, buf in (('y', ybuf), ('grad_x', gxbuf), ('grad_W', gWbuf), ('grad_b', gbbuf)):
        assert _bands_intact(buf, True), name


# ---------------------------------------------------------------------------------------------------------------------
# special values: a non-finite operand reaches what the fp32 kernel's would, and nothing else
# ---------------------------------------------------------------------------------------------------------------------
SPECIAL = (70, 1204, 132)      # 64 x 64 tiles in all three products, no split


def _keep(t, row=None, col=None):
    t = t.detach().double().cpu()
    if row is not None:
        t = torch.cat([t[:row], t[row + 1:]], 0)
    if col is not None:
        t = torch.cat([t[:, :col], t[:, col + 1:]], 1)
    return t


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('which', ['inf_in_x', 'nan_in_W'])
def test_a_non_finite_operand_poisons_one_row_or_column_only(dev, which, mode):
    from deeptables_amd import _lib
    N, K, M = SPECIAL
    assert S.geometry(N, K, M, mode, S.FWD)[:2] == (64, 64)
    h = _lib.lib()
    fc, bc = S.CLAIM[mode]
    r = S.reference_for(mode, N, K, M, None, True)
    x, W, b, gy = (r[k].float().to(dev).contiguous() for k in ('x', 'W', 'b', 'up'))
    rr, kk, mm = 37, 1001, 70                  # the second row / column tile, a contraction index past the 31st step
    if which == 'inf_in_x':
        x[rr, kk] = float('inf')
    else:
        W[kk, mm] = float('nan')
    y = torch.empty((N, M), dtype=torch.float32, device=dev)
    _fwd(h, mode, x, W, b, y, _lib.DT_ACT_LINEAR)
    gx = torch.empty((N, K), dtype=torch.float32, device=dev)
    gW, gb = torch.zeros((K, M), device=dev), torch.zeros((M,), device=dev)
    _bwd(h, mode, x, W, y, gy, _lib.DT_ACT_LINEAR, gx, gW, gb)
    if which == 'inf_in_x':        # row rr of y, row kk of grad_W
        assert not bool(torch.isfinite(y[rr]).any()) and not bool(torch.isfinite(gW[kk]).any())
        cut = dict(y=dict(row=rr), dx={}, dW=dict(row=kk))
    else:                          # column mm of y, column kk of grad_x
        assert bool(torch.isnan(y[:, mm]).all()) and bool(torch.isnan(gx[:, kk]).all())
        cut = dict(y=dict(col=mm), dx=dict(col=kk), dW={})
    figs = {}
    for name, got, ref, scale, cls in (('y', y, 'y', 's_y', fc), ('dx', gx, 'dx', 's_x', bc), ('dW', gW, 'dW', 's_W', bc)):
        rest = _keep(got, **cut[name])
        assert bool(torch.isfinite(rest).all()), f'{name}: a finite neighbour became non-finite'
        figs[name] = (P.cond_rms(rest, _keep(r[ref], **cut[name]), _keep(r[scale], **cut[name])), cls)
    assert bool(torch.isfinite(gb).all())
    figs['db'] = (P.cond_rms(gb, r['db'], r['s_b']), S.GRAD_B_CLASS)
    _hold(f'dense_x3 special[{mode},{which}]', figs)


# ---------------------------------------------------------------------------------------------------------------------
# the modes are told apart: a kernel that ran another number of products than its mode says fails here
# ---------------------------------------------------------------------------------------------------------------------
def test_the_two_modes_are_told_apart_by_the_neighbouring_bars(dev):
    """(33, 1201, 128): the numpy emulation of tests/test_split_bf16_arithmetic.py gives, in units of 2^-24, 0.004 (six
    products) / 3.3 (three) / 1781 (one) for the forward at K = 1,201, and 10 / 5438 (grad_x, contraction 128) and 20 / 10607
    (grad_W, contraction 33) for three / one products (tests/test_dense_x3_host.py repeats it on the CPU)"""
    from deeptables_amd import ops
    N, K, M = 33, 1201, 128
    figs = {}
    for mode in MODES:
        r = S.reference_for(mode, N, K, M, 'relu', True)
        xd, Wd = r['x'].float().to(dev).requires_grad_(True), r['W'].float().to(dev).requires_grad_(True)
        bd = r['b'].float().to(dev).requires_grad_(True)
        out = ops.dense(xd, Wd, bd, 'relu', mfma_dtype=mode)
        (out * r['up'].float().to(dev)).sum().backward()
        figs[mode] = {k: v for k, (v, _) in _figures(mode, r, out, xd.grad, Wd.grad, bd.grad).items()}
        print(f'dense_x3 apart[{mode}] / 2^-24:', {k: round(v / P.U, 3) for k, v in figs[mode].items()})
    assert figs['bf16']['y'] > P.COND_BAR['b17']                  # one product, not three or six
    assert figs['bf16x3']['y'] <= P.COND_BAR['fp32']              # six products forward ...
    assert min(figs['bf16x3']['dx'], figs['bf16x3']['dW']) > P.COND_BAR['fp32']      # ... three backward, not six
    assert max(figs['bf16x3']['dx'], figs['bf16x3']['dW']) <= P.COND_BAR['b17']      # ... and not one
