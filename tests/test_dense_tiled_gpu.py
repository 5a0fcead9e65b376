# -*- coding:utf-8 -*-
"""GPU: the tiled Dense kernels (csrc/dense_tiled.hip) held to the fp32 class of tests/precision.py on shapes the LDS-slab
kernels of csrc/dense.hip refuse, and to dt_dense_bwd's overwrite / accumulate contract through the C ABI.

Shapes: the smallest just past each limit of dt_dense_supported, the real K / M of the FiBiNet and FGCNN presets at a small
N, and two squares of ~1930 — the smallest at which all three products (N x M, N x K, K x M outputs) have the 256 tiles of
128 x 128 that switch the kernel from its 64 x 64 to its 128 x 128 block, one with K % 4 == 0 and M odd, one the other way
round (16-byte and 4-byte staging loads of either operand)."""
import numpy as np
import pytest
import torch

from tests import precision as P

pytestmark = pytest.mark.gpu

CASES = [(33, 1201, 128, 'relu', True), (257, 600, 64, 'relu', True), (37, 301, 2, None, True),
         (40, 64, 1300, 'relu', False), (5, 1203, 3, None, True), (70, 2912, 832, None, True),
         (45, 10413, 128, 'relu', False), (129, 1443, 128, 'relu', True),
         (1930, 1932, 1929, 'relu', True), (1929, 1929, 1932, None, False)]


def _rnd(g, shape, scale=1.0):
    """float64 values that float32 holds exactly: the kernel and the reference see the same inputs"""
    return (torch.randn(shape, generator=g, dtype=torch.float64) * scale).float().double()


def _reference(g, N, K, M, act, bias):
    """float64 forward / backward of one Dense and the |A| |B| scales of yardstick A (tests/test_precision_gpu.py)"""
    x, W = _rnd(g, (N, K)), _rnd(g, (K, M), 1.0 / np.sqrt(K))
    b = _rnd(g, (M,), 0.3) if bias else None
    lin = lambda x_, W_, b_: x_ @ W_ + (b_ if b_ is not None else 0)
    pre = lin(x, W, b)
    up = P.kink_mask(pre, P.abs_forward(lin, (x, W, b)), _rnd(g, (N, M)), act, 'fp32')
    xr, Wr = x.clone().requires_grad_(True), W.clone().requires_grad_(True)
    br = b.clone().requires_grad_(True) if bias else None
    ref = xr @ Wr + (br if bias else 0)
    ref = torch.relu(ref) if act == 'relu' else ref
    (ref * up).sum().backward()
    upl = up * (pre > 0) if act == 'relu' else up
    s_out, (s_x, s_W, s_b) = P.abs_scale(lin, (x, W, b), upl)
    return dict(x=x, W=W, b=b, up=up, y=ref.detach(), dx=xr.grad, dW=Wr.grad, db=br.grad if bias else None,
                s_y=s_out, s_x=s_x, s_W=s_W, s_b=s_b)


@pytest.mark.parametrize('N,K,M,act,bias', CASES)
def test_tiled_dense_is_fp32_class(dev, N, K, M, act, bias):
    from deeptables_amd import ops
    from deeptables_amd._lib import lib
    assert lib().dt_dense_supported(N, K, M) == 0          # the LDS-slab kernels cannot be what answers
    assert lib().dt_dense_tiled_supported(N, K, M) == 1
    r = _reference(torch.Generator().manual_seed(7 * N + K + M), N, K, M, act, bias)
    xd, Wd = r['x'].float().to(dev).requires_grad_(True), r['W'].float().to(dev).requires_grad_(True)
    bd = r['b'].float().to(dev).requires_grad_(True) if bias else None
    out = ops.dense(xd, Wd, bd, act)
    (out * r['up'].float().to(dev)).sum().backward()
    figs = {'y': ('fwd', P.cond_rms(out, r['y'], r['s_y'])), 'dx': ('bwd', P.cond_rms(xd.grad, r['dx'], r['s_x'])),
            'dW': ('bwd', P.cond_rms(Wd.grad, r['dW'], r['s_W']))}
    if bias:
        figs['db'] = ('bwd', P.cond_rms(bd.grad, r['db'], r['s_b']))
    print(f'dense_tiled[{N},{K},{M},{act},{bias}] cond_rms / 2^-24:', {k: round(v / P.U, 3) for k, (_, v) in figs.items()})
    P.check_cond(f'dense_tiled[{N},{K},{M},{act},{bias}]', 'dense', 'float32', figs)


def _call_bwd(h, x, W, y, gy, act, gx, gW, gb):
    from deeptables_amd._lib import check, ptr, stream_ptr
    N, K = x.shape
    M = W.shape[1]
    nbytes = h.dt_dense_tiled_workspace_bytes(N, K, M)
    ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=x.device) if nbytes > 0 else None
    check(h.dt_dense_tiled_bwd(ptr(x), ptr(W), ptr(y), ptr(gy), act, N, K, M, ptr(gx), ptr(gW), ptr(gb), ptr(ws),
                               stream_ptr()), 'dt_dense_tiled_bwd')
    torch.cuda.synchronize()


@pytest.mark.parametrize('N,K,M', [(40, 301, 5), (33, 1201, 128)])
def test_tiled_bwd_overwrites_grad_x_and_accumulates_the_weight_gradients(dev, N, K, M):
    """dt_dense_bwd's contract through ctypes: grad_W / grad_b come back as prefill + gradient, a NaN-filled grad_x comes back
    overwritten and finite, and grad_x = NULL / grad_b = NULL are accepted"""
    from deeptables_amd import _lib
    from deeptables_amd._lib import check, ptr, stream_ptr
    h = _lib.lib()
    r = _reference(torch.Generator().manual_seed(N + K + M), N, K, M, 'relu', True)
    x, W, b, gy = (r[k].float().to(dev).contiguous() for k in ('x', 'W', 'b', 'up'))
    y = torch.empty((N, M), dtype=torch.float32, device=dev)
    check(h.dt_dense_tiled_fwd(ptr(x), ptr(W), ptr(b), _lib.DT_ACT_RELU, N, K, M, ptr(y), stream_ptr()), 'dt_dense_tiled_fwd')
    g = torch.Generator().manual_seed(3)
    pre_W, pre_b = torch.randn((K, M), generator=g).to(dev), torch.randn((M,), generator=g).to(dev)
    gx = torch.full((N, K), float('nan'), dtype=torch.float32, device=dev)
    gW, gb = pre_W.clone(), pre_b.clone()
    _call_bwd(h, x, W, y, gy, _lib.DT_ACT_RELU, gx, gW, gb)
    assert bool(torch.isfinite(gx).all())
    # the sum adds one fp32 rounding of at most 2^-24 (|prefill| + |gradient|) to the gradient's own error: on the scale
    # |prefill| + |A| |B| the root mean square stays inside the fp32 class
    for got, pre, ref, scale in ((gW, pre_W, r['dW'], r['s_W']), (gb, pre_b, r['db'], r['s_b'])):
        pre = pre.double().cpu()
        assert P.cond_rms(got.double().cpu() - pre, ref, scale + pre.abs()) <= P.COND_BAR['fp32']
    assert P.cond_rms(gx, r['dx'], r['s_x']) <= P.COND_BAR['fp32']
    # grad_x = NULL and grad_b = NULL: the weight gradient alone, accumulated once more onto the same buffer
    gW2 = gW.clone()
    _call_bwd(h, x, W, y, gy, _lib.DT_ACT_RELU, None, gW2, None)
    first = gW.double().cpu()
    assert P.cond_rms(gW2.double().cpu() - first, r['dW'], r['s_W'] + first.abs()) <= P.COND_BAR['fp32']


def test_tiled_fwd_on_a_shape_both_families_accept(dev):
    """(64, 128, 64) runs on the tiled kernel when asked for directly: the same yardstick, not bitwise the other family"""
    from deeptables_amd import _lib
    from deeptables_amd._lib import check, ptr, stream_ptr
    h = _lib.lib()
    N, K, M = 64, 128, 64
    assert h.dt_dense_supported(N, K, M) == 1 and h.dt_dense_tiled_supported(N, K, M) == 1
    r = _reference(torch.Generator().manual_seed(11), N, K, M, 'relu', True)
    x, W, b = (r[k].float().to(dev).contiguous() for k in ('x', 'W', 'b'))
    y = torch.full((N, M), float('nan'), dtype=torch.float32, device=dev)
    check(h.dt_dense_tiled_fwd(ptr(x), ptr(W), ptr(b), _lib.DT_ACT_RELU, N, K, M, ptr(y), stream_ptr()), 'dt_dense_tiled_fwd')
    torch.cuda.synchronize()
    assert P.cond_rms(y, r['y'], r['s_y']) <= P.COND_BAR['fp32']
