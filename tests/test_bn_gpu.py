# -*- coding:utf-8 -*-
"""GPU: csrc/bn.hip (Keras BatchNormalization) against the float64 restatement of tests/bn_reference.py on the same
float32-rounded inputs, at every launch path of its two kernel families and on columns whose statistics are hard.

Paths (test_paths, one id per row): bn_vec4 takes the 16-byte family for C % 4 == 0, C <= 1024 and 16-byte aligned pointers,
the scalar one otherwise (test_alignment: one pointer at a time 4 bytes past a 16-byte boundary); bn_chunks gives
ceil(N / 32) chunks up to 512, so past N = 16384 trailing chunks are empty; RS = 256 / CW rows of a chunk are summed side by
side, 4x unrolled in k_bn_stats_v4 and 2x in k_bn_bwd_stats_v4 with a tail loop each; the element-wise passes stride over a
grid capped at 4096 blocks of 256 threads.

Bars (tests/precision.py, yardstick B, nothing of it changed): y, dx, the inference output (row_rel) and the moving
statistics (max_rel) within STEP_BAR['fp32'] = 12 x max(error of the float32 CPU reference, FLOOR).  dgamma, dbeta and the
sums of dt_bn_train_bwd_stats are column sums of N signed terms: per column |err| / sum_n |term| (precision.col_cond), the
kernel within 12 x max(the float32 CPU reference's figure in that metric, U).

MI355X, the largest err_gpu / max(err_f32, 2^-24) per figure over the cases of each test (bar 12; DT_PRECISION_LOG):
  test                  y     dx    infer  mov.mean  mov.var  dgamma  dbeta
  paths                 1.17  2.11  1.32   1.05      1.15     1.61    1.39
  affine                1.57  1.18  1.44   1.22      1.19     0.76    0.66
  alignment             1.11  0.95  1.00   0.56      1.00     0.99    0.39
  rank3                 1.11  2.23  0.72   0.62      0.75     1.63    0.59
  noncontiguous_x       1.95  1.00  0.92   1.00      0.85     0.92    0.66
  hard                  2.24  2.94  1.40   4.23      1.07     2.57    1.23
  constant              0     0.89  1.00   0         0.16     0       1.01
  outlier               1.00  1.83  0.90   1.57      1.19     2.61    1.11
  moving (two steps)    y 2.21, infer 1.00; after step 1: mean 0.90, var 1.07; after step 2: mean 1.29, var 2.35
  stride0               dgamma 0.54, dbeta exact;   bwd_stats: sum_g 0.75, sum_gx 0.57
Before these tests the kernels measured 16.4 on the moving mean wherever it starts at zero (the decay was 1.f - 0.99f, 9.5e-7 off
Keras's float(1.0 - 0.99)), 20.9 on the moving variance at (mean 1e4, std 1) (chunk means rounded to 1e-3 before Chan's delta^2)
and 18 .. 30 on y, dx, both moving statistics and dgamma when a 1e6 outlier was a chunk's shift; bn.hip now takes the decay from
the caller's double, shifts by a median of three rows and merges the variance from means relative to a column reference."""
import pytest
import torch

from tests import bn_reference as B
from tests import precision as P

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32


def _rnd(g, shape, scale=1.0, shift=0.0):
    """float64 values that float32 holds exactly: the kernel and the reference see the same inputs"""
    return (torch.randn(shape, generator=g, dtype=F64) * scale + shift).float().double()


def _mild(seed, shape, affine=(True, True)):
    g = torch.Generator().manual_seed(seed)
    C = shape[-1]
    x = _rnd(g, shape, 2.0, 3.0)
    gamma, beta = _rnd(g, (C,)), _rnd(g, (C,))
    return x, (gamma if affine[0] else None), (beta if affine[1] else None), _rnd(g, shape)


def _opt(t, dt):
    return None if t is None else t.to(dt)


def _reference(x, gamma, beta, up, mm0, mv0, eps, momentum):
    """{dtype: figures} of one training step, its backward for the upstream gradient `up`, and inference on the moving
    statistics that step leaves — each dtype on its own chain"""
    refs = {}
    for dt in (F64, F32):
        xs = [None if t is None else t.to(dt).clone().requires_grad_(True) for t in (x, gamma, beta)]
        r = B.keras_batchnorm(xs[0], xs[1], xs[2], mm0.to(dt), mv0.to(dt), True, eps, momentum, gy=up.to(dt))
        r.y.backward(up.to(dt))
        ri = B.keras_batchnorm(x.to(dt), _opt(gamma, dt), _opt(beta, dt), r.moving_mean, r.moving_var, False, eps)
        refs[dt] = dict(y=r.y.detach(), dx=xs[0].grad, dgamma=None if gamma is None else xs[1].grad,
                        dbeta=None if beta is None else xs[2].grad, mm=r.moving_mean, mv=r.moving_var, yi=ri.y.detach(),
                        sum_g=r.sum_g, sum_gx=r.sum_gx)
    return refs


def _place(t, dev, misalign=False):
    """float32 copy on the device, 16-byte aligned, or 4 bytes past a 16-byte boundary the way a parameter is that
    training.flatten_dense_parameters made a view of the model's flat buffer"""
    if t is None:
        return None
    if not misalign:
        v = t.float().to(dev)
        assert v.data_ptr() % 16 == 0
        return v
    buf = torch.empty(t.numel() + 1, dtype=F32, device=dev)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _gpu(x, gamma, beta, up, mm0, mv0, eps, momentum, dev, misalign=()):
    from deeptables_amd import ops
    xd, gd, bd = (None if t is None else _place(t, dev, n in misalign).requires_grad_(True)
                  for n, t in (('x', x), ('gamma', gamma), ('beta', beta)))
    upd = _place(up, dev, 'up' in misalign)
    mm, mv = mm0.float().to(dev), mv0.float().to(dev)
    y = ops.batchnorm_train(xd, gd, bd, mm, mv, eps, momentum)
    y.backward(upd)
    yi = ops.batchnorm_infer(xd.detach(), None if gd is None else gd.detach(), None if bd is None else bd.detach(), mm, mv,
                             eps)
    assert y.shape == x.shape and yi.shape == x.shape and xd.grad.shape == x.shape
    return dict(y=y.detach(), dx=xd.grad, dgamma=None if gd is None else gd.grad, dbeta=None if bd is None else bd.grad,
                mm=mm, mv=mv, yi=yi)


def _figures(got, refs, x, up, eps, keys=('y', 'dx', 'yi', 'mm', 'mv', 'dgamma', 'dbeta')):
    r64, r32 = refs[F64], refs[F32]
    s_g, s_gx = B.sum_scales(x, up, eps)
    figs = {}
    for k in keys:
        if r64.get(k) is None:
            assert got.get(k) is None
            continue
        assert got[k].shape == r64[k].shape and bool(torch.isfinite(got[k]).all())
        if k in ('dgamma', 'sum_gx', 'dbeta', 'sum_g'):
            s = s_gx if k in ('dgamma', 'sum_gx') else s_g
            figs[k] = ('bwd', P.col_cond(got[k], r64[k], s), P.col_cond(r32[k], r64[k], s))
        else:
            m = P.row_rel if r64[k].dim() >= 2 else P.max_rel
            figs[k] = ('fwd' if k in ('y', 'yi', 'mm', 'mv') else 'bwd', m(got[k], r64[k]), m(r32[k], r64[k]))
    return figs


def _check(test, x, gamma, beta, up, dev, eps=1e-3, momentum=0.99, mm0=None, mv0=None, misalign=()):
    C = x.shape[-1]
    mm0 = torch.zeros(C, dtype=F64) if mm0 is None else mm0
    mv0 = torch.ones(C, dtype=F64) if mv0 is None else mv0
    refs = _reference(x, gamma, beta, up, mm0, mv0, eps, momentum)
    got = _gpu(x, gamma, beta, up, mm0, mv0, eps, momentum, dev, misalign)
    P.check_step(test, 'bn', 'float32', _figures(got, refs, x, up, eps))
    return got, refs


# ---- section 2: every launch path ------------------------------------------------------------------------------------------
PATHS = [
    pytest.param(1, 5, id='N1-scalar-y_is_beta-dx_is_0'),
    pytest.param(1, 8, id='N1-v4-y_is_beta-dx_is_0'),
    pytest.param(32, 1, id='C1-CW1-RS256-one_chunk'),
    pytest.param(33, 1, id='C1-CW1-RS256-two_chunks_17+16'),
    pytest.param(40, 256, id='C256-v4-CW4_64'),
    pytest.param(40, 257, id='C257-scalar-two_column_passes-second_one_live_column'),
    pytest.param(39, 1024, id='C1024-v4-RS1-four_unrolled_then_3_row_tail'),
    pytest.param(39, 1028, id='C1028-mult_of_4_past_1024-scalar_fallback-five_column_passes'),
    pytest.param(1000, 256, id='N1000-C256-v4-RS4-last_chunk_8_rows_tail_only'),
    pytest.param(16385, 5, id='N16385-scalar-512_chunks_15_empty'),
    pytest.param(16385, 8, id='N16385-v4-512_chunks_15_empty'),
    pytest.param(16385, 256, id='N16385-C256-v4-empty_chunks-unrolled_rpc33_RS4-second_grid_stride_trip_v4'),
    pytest.param(16385, 65, id='N16385-C65-scalar-second_grid_stride_trip_apply_and_infer'),
]


@pytest.mark.parametrize('N,C', PATHS)
def test_paths(dev, N, C):
    x, gamma, beta, up = _mild(1000 * C + N, (N, C))
    got, _ = _check(f'paths[{N},{C}]', x, gamma, beta, up, dev)
    if N == 1:                                                           # mean = x and var = 0, exactly
        assert torch.equal(got['y'].cpu(), beta.float().expand(1, C))
        assert torch.equal(got['dx'].cpu(), torch.zeros(1, C))
        assert torch.equal(got['mv'].cpu(), torch.full((C,), 0.99)) and torch.equal(got['dgamma'].cpu(), torch.zeros(C))
        assert torch.equal(got['dbeta'].cpu(), up.float().reshape(C))


@pytest.mark.parametrize('has_gamma,has_beta', [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize('N,C', [(33, 8), (33, 5)])
def test_affine_present_or_none(dev, N, C, has_gamma, has_beta):
    """scale=False / center=False: gamma = 1 and beta = 0 in all six element-wise kernels, and no gradient for them"""
    from deeptables_amd import ops
    x, gamma, beta, up = _mild(7 * N + C, (N, C), (has_gamma, has_beta))
    _check(f'affine[{N},{C},{has_gamma},{has_beta}]', x, gamma, beta, up, dev)
    xd, gd, bd = (None if t is None else t.float().to(dev).requires_grad_(True) for t in (x, gamma, beta))
    y = ops.batchnorm_train(xd, gd, bd, torch.zeros(C, device=dev), torch.ones(C, device=dev))
    grads = ops._BatchNormTrain.backward(y.grad_fn, up.float().to(dev))
    assert len(grads) == 7 and grads[0].shape == (N, C) and all(t is None for t in grads[3:])
    assert (grads[1] is not None) == has_gamma and (grads[2] is not None) == has_beta


@pytest.mark.parametrize('which', ['none', 'x', 'gamma', 'beta', 'up'])
def test_alignment(dev, which):
    """C = 32 with one pointer 4 bytes past a 16-byte boundary: bn_vec4 must send every launch that reads it to the
    scalar family (x, gamma: forward and backward; beta: forward; the upstream gradient: backward).  _place asserts
    data_ptr() % 16 == 4, so the case cannot quietly become the aligned one."""
    x, gamma, beta, up = _mild(5, (100, 32))
    _check(f'alignment[{which}]', x, gamma, beta, up, dev, misalign=() if which == 'none' else (which,))


def test_rank3(dev):
    """x[B, F, D] normalised over B * F rows: the BatchNormalization that closes an AutoInt attention layer"""
    x, gamma, beta, up = _mild(11, (7, 5, 16))
    _check('rank3[7,5,16]', x, gamma, beta, up, dev)


@pytest.mark.parametrize('N,C', [(33, 8), (33, 5)])
def test_stride0_upstream_gradient(dev, N, C):
    """y.sum().backward(): the gradient arrives expanded from one element.  dx is ~0 by cancellation, so it is held
    bit for bit to the run with the same gradient materialised, and to the size its own terms allow."""
    from deeptables_amd import ops
    x, gamma, beta, _ = _mild(13 * N + C, (N, C))
    up = torch.ones(N, C, dtype=F64)
    refs = _reference(x, gamma, beta, up, torch.zeros(C, dtype=F64), torch.ones(C, dtype=F64), 1e-3, 0.99)
    runs = []
    for expanded in (True, False):
        xd, gd, bd = (t.float().to(dev).requires_grad_(True) for t in (x, gamma, beta))
        y = ops.batchnorm_train(xd, gd, bd, torch.zeros(C, device=dev), torch.ones(C, device=dev))
        if expanded:
            y.sum().backward()
        else:
            y.backward(torch.ones(N, C, device=dev))
        runs.append(dict(dx=xd.grad, dgamma=gd.grad, dbeta=bd.grad))
    for k in ('dx', 'dgamma', 'dbeta'):
        assert torch.equal(runs[0][k], runs[1][k]), k
    assert torch.equal(runs[0]['dbeta'].cpu(), torch.full((C,), float(N)))          # N ones: exact
    P.check_step(f'stride0[{N},{C}]', 'bn', 'float32', _figures(runs[0], refs, x, up, 1e-3, keys=('dgamma', 'dbeta')))
    # dx = gamma rstd (1 - sum_g / N - xhat sum_gx / N): 1 - N * fl(1 / N) is within one rounding, and sum_gx = sum xhat,
    # whose true value is 0, within the dgamma bar of sum |xhat|
    r = refs[F64]
    mean = x.mean(0)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(0) + 1e-3)
    xhat = (x - mean) * rstd
    bound = P.STEP_BAR['fp32'] * P.U * gamma.abs() * rstd * (1.0 + xhat.abs() * xhat.abs().mean(0))
    assert bool(((runs[0]['dx'].double().cpu() - r['dx']).abs() <= bound).all())


def test_noncontiguous_x(dev):
    from deeptables_amd import ops
    N, C = 33, 8
    x, gamma, beta, up = _mild(17, (N, C))
    refs = _reference(x, gamma, beta, up, torch.zeros(C, dtype=F64), torch.ones(C, dtype=F64), 1e-3, 0.99)
    base = torch.full((N, 2 * C), 1e6, device=dev)
    base[:, ::2] = x.float().to(dev)
    base.requires_grad_(True)
    xs = base[:, ::2]
    assert not xs.is_contiguous()
    gd, bd = gamma.float().to(dev).requires_grad_(True), beta.float().to(dev).requires_grad_(True)
    mm, mv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    y = ops.batchnorm_train(xs, gd, bd, mm, mv)
    y.backward(up.float().to(dev))
    yi = ops.batchnorm_infer(xs.detach(), gd.detach(), bd.detach(), mm, mv)
    assert torch.equal(base.grad[:, 1::2], torch.zeros(N, C, device=dev))
    got = dict(y=y.detach(), dx=base.grad[:, ::2], dgamma=gd.grad, dbeta=bd.grad, mm=mm, mv=mv, yi=yi)
    P.check_step('noncontiguous_x[33,8]', 'bn', 'float32', _figures(got, refs, x, up, 1e-3))


@pytest.mark.parametrize('eps,momentum', [(1e-3, 0.99), (1e-5, 0.9), (1e-1, 0.0)])
@pytest.mark.parametrize('N,C', [(33, 8), (33, 5)])
def test_moving_statistics_two_steps_in_place(dev, N, C, eps, momentum):
    """random initial moving statistics, two training steps on two batches updating them in place, then inference"""
    from deeptables_amd import ops
    g = torch.Generator().manual_seed(19 * N + C)
    x1, x2 = _rnd(g, (N, C), 2.0, 3.0), _rnd(g, (N, C), 0.5, -1.0)
    gamma, beta, up = _rnd(g, (C,)), _rnd(g, (C,)), _rnd(g, (N, C))
    mm0, mv0 = _rnd(g, (C,)), (torch.rand(C, generator=g, dtype=F64) + 0.5).float().double()
    refs = {}
    for dt in (F64, F32):
        r1 = B.keras_batchnorm(x1.to(dt), gamma.to(dt), beta.to(dt), mm0.to(dt), mv0.to(dt), True, eps, momentum)
        r2 = B.keras_batchnorm(x2.to(dt), gamma.to(dt), beta.to(dt), r1.moving_mean, r1.moving_var, True, eps, momentum)
        ri = B.keras_batchnorm(x1.to(dt), gamma.to(dt), beta.to(dt), r2.moving_mean, r2.moving_var, False, eps)
        refs[dt] = dict(mm1=r1.moving_mean, mv1=r1.moving_var, y=r2.y, mm=r2.moving_mean, mv=r2.moving_var, yi=ri.y)
    gd, bd = gamma.float().to(dev), beta.float().to(dev)
    mm, mv = mm0.float().to(dev), mv0.float().to(dev)
    where = (mm.data_ptr(), mv.data_ptr())
    ops.batchnorm_train(x1.float().to(dev), gd, bd, mm, mv, eps, momentum)
    got = dict(mm1=mm.clone(), mv1=mv.clone())
    got['y'] = ops.batchnorm_train(x2.float().to(dev), gd, bd, mm, mv, eps, momentum)
    assert where == (mm.data_ptr(), mv.data_ptr())
    got.update(mm=mm, mv=mv, yi=ops.batchnorm_infer(x1.float().to(dev), gd, bd, mm, mv, eps))
    figs = {}
    for k in ('mm1', 'mv1', 'y', 'mm', 'mv', 'yi'):
        m = P.row_rel if refs[F64][k].dim() >= 2 else P.max_rel
        figs[k] = ('fwd', m(got[k], refs[F64][k]), m(refs[F32][k], refs[F64][k]))
    P.check_step(f'moving[{N},{C},{eps},{momentum}]', 'bn', 'float32', figs)


# ---- dt_bn_train_bwd_stats, the entry point dt_autoint_bwd builds on --------------------------------------------------------
CANARY = 64


def _ws(N, C, dev):
    """the workspace dt_bn_workspace_bytes asks for, and CANARY floats past it that no kernel may touch"""
    from deeptables_amd import _lib
    nbytes = _lib.lib().dt_bn_workspace_bytes(N, C)
    assert nbytes == 4 * (512 * 3 * C + 2 * C)
    return torch.full((nbytes // 4 + CANARY,), -7.0, dtype=F32, device=dev)


@pytest.mark.parametrize('N,C', [(33, 5), (1000, 32), (16385, 8)])
def test_bwd_stats_entry_point(dev, N, C):
    from deeptables_amd import _lib
    from deeptables_amd._lib import check, ptr, stream_ptr
    L = _lib.lib()
    x, gamma, _, up = _mild(23 * N + C, (N, C))
    refs = _reference(x, gamma, None, up, torch.zeros(C, dtype=F64), torch.ones(C, dtype=F64), 1e-3, 0.99)
    xd, ud, gd = (t.float().to(dev) for t in (x, up, gamma))
    y, mean, rstd = torch.empty_like(xd), torch.empty(C, device=dev), torch.empty(C, device=dev)
    ws = _ws(N, C, dev)
    # no moving statistics: null pointers are allowed, and nothing is updated
    check(L.dt_bn_train_fwd(ptr(xd), N, C, None, None, 1e-3, 0.99, 1.0 - 0.99, None, None, ptr(y), ptr(mean), ptr(rstd), ptr(ws),
                            stream_ptr()), 'dt_bn_train_fwd')
    assert all(t.data_ptr() % 16 == 0 for t in (xd, ud, gd, y, mean, rstd, ws))
    out = {}
    for given in (True, False):
        sums = torch.full((2 * C + CANARY,), -7.0, device=dev)
        gg, gb = (torch.full((C,), -7.0, device=dev), torch.full((C,), -7.0, device=dev)) if given else (None, None)
        ws = _ws(N, C, dev)
        check(L.dt_bn_train_bwd_stats(ptr(xd), ptr(ud), N, C, ptr(mean), ptr(rstd), ptr(sums), ptr(gg), ptr(gb), ptr(ws),
                                      stream_ptr()), 'dt_bn_train_bwd_stats')
        assert torch.equal(sums[2 * C:], torch.full((CANARY,), -7.0, device=dev))
        assert torch.equal(ws[-CANARY:], torch.full((CANARY,), -7.0, device=dev))
        out[given] = dict(sum_g=sums[:C], sum_gx=sums[C:2 * C], gg=gg, gb=gb)
        P.check_step(f'bwd_stats[{N},{C},{"given" if given else "null"}]', 'bn', 'float32',
                     _figures(out[given], refs, x, up, 1e-3, keys=('sum_g', 'sum_gx')))
    assert torch.equal(out[True]['gb'], out[True]['sum_g']) and torch.equal(out[True]['gg'], out[True]['sum_gx'])
    assert torch.equal(out[False]['sum_g'], out[True]['sum_g']) and torch.equal(out[False]['sum_gx'], out[True]['sum_gx'])
    # dt_bn_train_bwd runs the same two reduction kernels with the same launch on aligned inputs: bit for bit
    gx, gg, gb, ws = torch.empty_like(xd), torch.empty(C, device=dev), torch.empty(C, device=dev), _ws(N, C, dev)
    check(L.dt_bn_train_bwd(ptr(xd), ptr(ud), N, C, ptr(gd), ptr(mean), ptr(rstd), ptr(gx), ptr(gg), ptr(gb), ptr(ws),
                            stream_ptr()), 'dt_bn_train_bwd')
    assert torch.equal(ws[-CANARY:], torch.full((CANARY,), -7.0, device=dev))
    assert torch.equal(gb, out[True]['gb']) and torch.equal(gg, out[True]['gg'])
    assert P.row_rel(gx, refs[F64]['dx']) <= P.STEP_BAR['fp32'] * max(P.row_rel(refs[F32]['dx'], refs[F64]['dx']), P.FLOOR)


@pytest.mark.parametrize('N,C', [(16385, 8), (1000, 256)])
def test_deterministic(dev, N, C):
    """nothing in bn.hip uses a float atomic: two runs agree bit for bit"""
    x, gamma, beta, up = _mild(29 * N + C, (N, C))
    z, o = torch.zeros(C, dtype=F64), torch.ones(C, dtype=F64)
    a = _gpu(x, gamma, beta, up, z, o, 1e-3, 0.99, dev)
    b = _gpu(x, gamma, beta, up, z, o, 1e-3, 0.99, dev)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_empty_batch_contract(dev):
    from deeptables_amd import ops
    from deeptables_amd._lib import DtHipError
    C = 8
    gamma, beta = torch.ones(C, device=dev), torch.zeros(C, device=dev)
    mm, mv = torch.full((C,), 0.25, device=dev), torch.full((C,), 2.0, device=dev)
    for shape in ((0, C), (0, 5, C)):
        y = ops.batchnorm_infer(torch.empty(shape, device=dev), gamma, beta, mm, mv)
        assert y.shape == shape and y.dtype == F32
        assert ops.batchnorm_infer(torch.empty(shape, device=dev), None, None, mm, mv).shape == shape
    with pytest.raises(DtHipError, match='dt_bn_train_fwd'):
        ops.batchnorm_train(torch.empty((0, C), device=dev), gamma, beta, mm, mv)
    torch.cuda.synchronize()
    assert torch.equal(mm.cpu(), torch.full((C,), 0.25)) and torch.equal(mv.cpu(), torch.full((C,), 2.0))


# ---- section 3: hard statistics -------------------------------------------------------------------------------------------
TIERS = [(0.0, 1.0), (100.0, 1.0), (1e4, 1.0), (-3e3, 1e-2), (1e6, 1.0), (0.25, 1e-4)]
SIZES = [33, 1000, 16385]


@pytest.mark.parametrize('C', [16, 15], ids=['v4', 'scalar'])
@pytest.mark.parametrize('N', SIZES)
@pytest.mark.parametrize('mean,std', TIERS)
def test_hard_statistics(dev, mean, std, N, C):
    """one tier per tensor, every column the same (mean, std): columns whose mean dwarfs their spread are what the shifted
    chunk sums are for.  The reference is float64 on the float32-rounded x: the kernel's arithmetic is on trial, not the
    rounding of its input."""
    g = torch.Generator().manual_seed(N + C + int(abs(mean)) % 977)
    x = _rnd(g, (N, C), std, mean)
    gamma, beta, up = _rnd(g, (C,)), _rnd(g, (C,)), _rnd(g, (N, C))
    _check(f'hard[{mean:g},{std:g},{N},{C}]', x, gamma, beta, up, dev)


@pytest.mark.parametrize('C', [16, 15], ids=['v4', 'scalar'])
@pytest.mark.parametrize('N', SIZES)
def test_constant_columns(dev, N, C):
    """exactly constant columns: y = beta, and dx as it works out with rstd = 1 / sqrt(eps).  The Chan merge need not hand a
    constant back bit for bit, so the bar is the yardstick with its floor; the variance is finite and not negative."""
    g = torch.Generator().manual_seed(N + C)
    x = torch.tensor([5.0, 0.1, -3e3, 1e6], dtype=F32).double().repeat(4)[:C].expand(N, C).contiguous()
    gamma, beta, up = _rnd(g, (C,)), _rnd(g, (C,)), _rnd(g, (N, C))
    got, refs = _check(f'constant[{N},{C}]', x, gamma, beta, up, dev)
    assert torch.equal(refs[F64]['y'], beta.expand(N, C)) and torch.equal(refs[F64]['mv'], torch.full((C,), 0.99, dtype=F64))
    # moving_var = 1 * 0.99 + var * 0.01: a negative or non-finite batch variance shows
    assert bool(torch.isfinite(got['mv']).all()) and bool((got['mv'].cpu() >= torch.tensor(0.99, dtype=F32)).all())


@pytest.mark.parametrize('C', [16, 15], ids=['v4', 'scalar'])
@pytest.mark.parametrize('N', [33, 1000])
def test_outlier_is_the_shift(dev, N, C):
    """randn columns, each with one row at 1e6 that is the first of its chunk (32 rows at N = 1000, 17 at N = 33) and so
    becomes the shift K of that chunk: every other row of the chunk is summed as x - 1e6"""
    g = torch.Generator().manual_seed(3 * N + C)
    x = _rnd(g, (N, C))
    chunks = (N + 31) // 32
    rpc = (N + chunks - 1) // chunks                                     # bn_chunks and rows_per_chunk of csrc/bn.hip
    for c in range(C):
        x[(c % chunks) * rpc, c] = 1e6
    gamma, beta, up = _rnd(g, (C,)), _rnd(g, (C,)), _rnd(g, (N, C))
    _check(f'outlier[{N},{C}]', x, gamma, beta, up, dev)
