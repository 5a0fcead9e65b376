# -*- coding:utf-8 -*-
"""GPU: the kernels of csrc/loss_reg.hip — Keras' regression losses (dt_loss_reg) and GHM-C (dt_ghmc) — against the float64
restatement of tests/loss_reg_reference.py and oracle.reference_layers.ghmc_loss, the autograd functions over them in a
captured graph, and the losses through DeepModel's train_step and fit.

Bars.  The five kinds: yardstick B of tests/precision.py — the kernel's error is at most STEP_BAR['fp32'] x max(err_f32,
FLOOR), err_f32 the error of the same restatement in float32 on the CPU; relative error for the loss, max_rel for dz — and
the outer caps of tests/test_losses_gpu._bars (1e-4 for the loss, 2e-4 for dz).  GHM-C: `acc_sum` within 1e-6 relative, the
loss within 1e-5 absolute, dz within yardstick B.

Kinks.  Every drawn case keeps its elements at least 1e-3 from its kind's kink (|e| = 0 for MAPE, p = eps for MSLE, p + eps = 0
for Poisson) and, for GHM-C, every float64 gradient length at least 1e-5 from every bin edge, so that all precisions put the
elements into the same bins; the margin is asserted on the float64 reference before the kernel runs and nothing is masked
out of a comparison.  For GHM-C the elements that a draw leaves inside the margin are drawn again on the CPU until none is:
with 256 bins and 5000 elements a whole draw without one does not exist (5e-3 of the unit interval lies inside the margin)."""
import math

import numpy as np
import pytest
import torch

from tests import loss_reg_reference as LRR
from tests import precision as P
from tests.test_losses_gpu import B, _bars, _fit_first_loss, _frame, _inputs, _model, _weights

pytestmark = pytest.mark.gpu

BAR, FLOOR = P.STEP_BAR['fp32'], P.FLOOR
MARGIN = 1e-3
GHMC_MARGIN = 1e-5
F64 = torch.float64


# ===========================================================================================================================
# dt_loss_reg
# ===========================================================================================================================
def _kernel(dev, kind, z, t, w=None, delta=1.0, grad=True):
    """dt_loss_reg through ctypes on poisoned outputs and workspace -> (loss [1], dz or None) on the host"""
    from deeptables_amd import _lib
    from deeptables_amd._lib import check, ptr, stream_ptr
    h = _lib.lib()
    assert z.dtype == torch.float32 and t.dtype == torch.float32 and z.shape == t.shape
    zd, td = z.to(dev).contiguous(), t.to(dev).contiguous()
    wd = None if w is None else w.to(dev).contiguous()
    rows, classes = z.shape
    need = h.dt_loss_reg_workspace_bytes(rows, classes)
    assert need == 8 * ((rows * classes + 2047) // 2048)
    ws = torch.full((need // 8,), float('nan'), dtype=torch.float64, device=dev)
    loss = torch.full((1,), float('nan'), dtype=torch.float32, device=dev)
    dz = torch.full_like(zd, float('nan')) if grad else None
    check(h.dt_loss_reg(LRR.kind_code(kind), ptr(zd), ptr(td), ptr(wd), rows, classes, delta, ptr(loss), ptr(dz), ptr(ws),
                        stream_ptr()), 'dt_loss_reg')
    torch.cuda.synchronize()
    return loss.cpu(), (None if dz is None else dz.cpu())


def _check(name, dev, kind, z, t, w=None, delta=1.0, what=''):
    margin = LRR.kink_margin(kind, z, t)
    assert margin >= MARGIN, (name, kind, what, 'an element lies within 1e-3 of a kink', margin)
    ref = LRR.value_and_grad(kind, z, t, w, delta, torch.float64)
    f32 = LRR.value_and_grad(kind, z, t, w, delta, torch.float32)
    got = _kernel(dev, kind, z, t, w, delta)
    value_only, none = _kernel(dev, kind, z, t, w, delta, grad=False)
    assert none is None and torch.equal(value_only, got[0]), (name, kind, what, 'the loss differs without dz')
    _bars(name, kind, ref, f32, got, what)
    return got


def _draw(kind, rows, classes, seed, clamped=False):
    """(p, t) float32 off every kink by construction: Poisson and MSLE predictions in [0.05, 5] (`clamped`: every flat index
    = 1 mod 3 at <= -1e-3 instead), MAPE targets with |t| >= 0.1 and |e| >= 2e-3"""
    g = torch.Generator().manual_seed(1000 * seed + 7 * rows + classes)
    if kind in ('msle', 'poisson'):
        p = torch.rand(rows, classes, generator=g) * 4.95 + 0.05
        t = torch.rand(rows, classes, generator=g) * 5.0
        if clamped:
            low = (torch.arange(rows * classes) % 3 == 1).reshape(rows, classes)
            p = torch.where(low, -(1e-3 + torch.rand(rows, classes, generator=g)), p)
        return p, t
    if kind == 'mape':
        sign = torch.where(torch.rand(rows, classes, generator=g) < 0.5, -1.0, 1.0)
        t = sign * (0.1 + torch.rand(rows, classes, generator=g) * 3.0)
        e = torch.randn(rows, classes, generator=g)
        e = torch.where(e >= 0, e + 2e-3, e - 2e-3)
        return t + e, t
    return torch.randn(rows, classes, generator=g) * 2.0, torch.randn(rows, classes, generator=g)


# 2048 elements per block: one element, a partial block, exactly one block, two blocks + the total kernel (by rows and by
# rows x classes), and rows of 70 classes whose elements straddle block boundaries
SHAPES = [(1, 1), (7, 3), (2048, 1), (2049, 1), (683, 3), (300, 70)]


@pytest.mark.parametrize('kind', LRR.KINDS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_kinds_at_every_launch_path(dev, kind, shape):
    rows, classes = shape
    p, t = _draw(kind, rows, classes, 1)
    for delta in ((1.0, 0.5) if kind == 'huber' else (1.0,)):
        _check('reg', dev, kind, p, t, None, delta, what=(rows, classes, 'unweighted', delta))
        _check('reg', dev, kind, p, t, _weights(rows, 3), delta, what=(rows, classes, 'weighted', delta))


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_msle_on_the_clamped_side(dev, shape):
    """a third of the predictions at <= -1e-3: max(p, eps) = eps there, and the gradient is exactly 0"""
    rows, classes = shape
    p, t = _draw('msle', rows, classes, 2, clamped=True)
    for w in (None, _weights(rows, 5)):
        _, dz = _check('reg_clamped', dev, 'msle', p, t, w, what=(rows, classes, 'weighted' if w is not None else 'unweighted'))
        assert bool((dz[p < 0] == 0).all()) and (rows * classes < 2 or int((p < 0).sum()) >= rows * classes // 3)


@pytest.mark.parametrize('kind,shape', [('huber', (2049, 1)), ('log_cosh', (683, 3)), ('msle', (300, 70)), ('mape', (7, 3)),
                                        ('poisson', (2048, 1))])
def test_same_bits_on_every_call_and_without_dz(dev, kind, shape):
    p, t = _draw(kind, *shape, 5)
    w = _weights(shape[0], 6)
    l1, d1 = _kernel(dev, kind, p, t, w)
    l2, d2 = _kernel(dev, kind, p, t, w)
    l3, d3 = _kernel(dev, kind, p, t, w, grad=False)
    assert torch.equal(l1, l2) and torch.equal(d1, d2) and torch.equal(l1, l3) and d3 is None
    assert torch.isfinite(l1).all() and torch.isfinite(d1).all()


def test_hard_values(dev):
    # Huber at |e| = delta exactly: both branches give delta^2 / 2 and +-delta
    delta = 0.5
    p = torch.tensor([[0.5, -0.5, 1.0, 0.25]])
    t = torch.zeros(1, 4)
    l, dz = _kernel(dev, 'huber', p, t, None, delta)
    assert abs(float(l) - (0.125 + 0.125 + (0.5 - 0.125) + 0.03125) / 4) <= 1e-7
    assert dz.tolist() == [[0.125, -0.125, 0.125, 0.0625]]
    # e = 0: value and gradient 0 (MAPE: sign(0) = 0); Poisson has its own value there and the gradient eps / (p + eps)
    same = torch.tensor([[0.5, 1.0, 2.0]])
    for kind in ('huber', 'log_cosh', 'msle', 'mape'):
        l, dz = _kernel(dev, kind, same, same.clone())
        assert float(l) == 0.0 and dz.tolist() == [[0.0, 0.0, 0.0]], kind
    l, dz = _kernel(dev, 'poisson', same, same.clone())
    rl, rd = LRR.value_and_grad('poisson', same, same)
    assert abs(float(l) - float(rl)) <= 1e-6 and float((dz.double() - rd).abs().max()) <= 1e-7
    # a Poisson prediction of -1: log of a negative number, NaN as in Keras
    l, _ = _kernel(dev, 'poisson', torch.tensor([[2.0, -1.0]]), torch.tensor([[1.0, 1.0]]))
    assert math.isnan(float(l))
    # log-cosh at |e| = 50 stays finite: |e| - ln 2, gradient +-1
    l, dz = _kernel(dev, 'log_cosh', torch.tensor([[50.0, -50.0]]), torch.zeros(1, 2))
    assert abs(float(l) - (50.0 - math.log(2.0))) <= 1e-5 and dz.tolist() == [[0.5, -0.5]]
    # and for small e it is e^2 / 2, where Keras' float32 form holds ~1e-7 absolute
    e = 1e-4
    l, dz = _kernel(dev, 'log_cosh', torch.tensor([[e]]), torch.zeros(1, 1))
    assert abs(float(l) - e * e / 2) <= 1e-6 * e * e / 2 and abs(float(dz) - e) <= 1e-6 * e


# ===========================================================================================================================
# dt_ghmc
# ===========================================================================================================================
def _ghmc_kernel(dev, z, t, mask, bins, momentum, acc, grad=True):
    """dt_ghmc on poisoned outputs and workspace; `acc` (device tensor or None) is updated in place -> (loss [1], dz) on the host"""
    from deeptables_amd import _lib
    from deeptables_amd._lib import check, ptr, stream_ptr
    h = _lib.lib()
    zd, td = z.to(dev).contiguous(), t.to(dev).contiguous()
    md = None if mask is None else mask.to(dev).contiguous()
    n = z.numel()
    need = h.dt_ghmc_workspace_bytes(n, bins)
    assert need > 0 and need % 8 == 0
    ws = torch.full((need // 8,), float('nan'), dtype=torch.float64, device=dev)
    loss = torch.full((1,), float('nan'), dtype=torch.float32, device=dev)
    dz = torch.full_like(zd, float('nan')) if grad else None
    check(h.dt_ghmc(ptr(zd), ptr(td), ptr(md), n, bins, momentum, 1.0 - momentum, ptr(acc), ptr(loss), ptr(dz), ptr(ws),
                    stream_ptr()), 'dt_ghmc')
    torch.cuda.synchronize()
    return loss.cpu(), (None if dz is None else dz.cpu())


def _ghmc_draw(shape, bins, seed, ignored=False):
    """(z, t, mask) float32 with every float64 gradient length at least GHMC_MARGIN from every bin edge: the elements a draw
    leaves inside the margin are drawn again.  ignored: every 7th target is -1 (in no bin)."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(shape, generator=g) * 2.0
    t = (torch.rand(shape, generator=g) < 0.4).float()
    if ignored:
        t.reshape(-1)[::7] = -1.0
    mask = (torch.rand(shape, generator=g) < 0.7).float()
    left, right = LRR.ghmc_edges(bins, torch.float32)
    edges = torch.cat([left, right[-1:]]).double().reshape(1, -1)
    for _ in range(200):
        gl = (torch.sigmoid(z.double()) - t.double()).abs().reshape(-1, 1)
        near = ((gl - edges).abs().min(1).values < 2 * GHMC_MARGIN).reshape(shape)
        if not bool(near.any()):
            break
        z = torch.where(near, torch.randn(shape, generator=g) * 2.0, z)
    return z, t, mask


GHMC_SHAPES = {1: (1, 1), 200: (200, 1), 2048: (2048, 1), 2049: (2049, 1), 5000: (1000, 5)}
GHMC_PAIRS = [(10, 0.75), (7, 0.0), (256, 0.5)]


def _ghmc_reference(z, t, mask, acc, bins, momentum, dtype):
    """(loss, dz, acc_sum) of one call in `dtype` on the CPU, as float64"""
    from oracle import reference_layers as R
    zz = z.to(dtype).clone().requires_grad_(True)
    if mask is None:
        loss, acc2 = R.ghmc_loss(zz, t.to(dtype), acc.to(dtype), bins=bins, momentum=momentum)
    else:
        loss, acc2 = LRR.ghmc(zz, t.to(dtype), acc.to(dtype), bins=bins, momentum=momentum, mask=mask.to(dtype))
    (dz,) = torch.autograd.grad(loss, zz)
    return loss.detach().double(), dz.double(), acc2.detach().double()


@pytest.mark.parametrize('masked', (False, True), ids=('nomask', 'mask'))
@pytest.mark.parametrize('pair', GHMC_PAIRS, ids=lambda p: f'bins{p[0]}_m{p[1]}')
@pytest.mark.parametrize('n', list(GHMC_SHAPES))
def test_ghmc_three_consecutive_calls(dev, n, pair, masked):
    bins, mmt = pair
    shape = GHMC_SHAPES[n]
    acc_dev = torch.zeros(bins, dtype=torch.float32, device=dev) if mmt > 0 else None
    acc64, acc32 = torch.zeros(bins, dtype=F64), torch.zeros(bins)
    for call in range(3):
        z, t, mask = _ghmc_draw(shape, bins, 100 * n + 10 * bins + call, ignored=(call == 1 and n > 1))
        mask = mask if masked else None
        if masked and n == 1:
            mask = torch.ones(shape)                      # (everything masked out is the NaN case, tested on its own)
        margin = LRR.kink_margin('ghmc', z, t, bins)
        assert margin >= GHMC_MARGIN, (n, pair, call, 'a gradient length lies within 1e-5 of a bin edge', margin)
        rl, rd, acc64 = _ghmc_reference(z, t, mask, acc64, bins, mmt, F64)
        fl, fd, a32 = _ghmc_reference(z, t, mask, acc32, bins, mmt, torch.float32)
        acc32 = a32.float()
        gl, gd = _ghmc_kernel(dev, z, t, mask, bins, mmt, acc_dev)
        assert torch.isfinite(gl).all() and torch.isfinite(gd).all()
        e_d, f_d = P.max_rel(gd, rd), P.max_rel(fd, rd)
        ratio = e_d / max(f_d, FLOOR)
        e_l = abs(float(gl) - float(rl))
        P.record('ghmc', n=n, bins=bins, momentum=mmt, masked=masked, call=call, dz_ratio=ratio, dz_err=e_d, dz_f32=f_d,
                 loss_err=e_l, loss_f32=abs(float(fl) - float(rl)))
        print(f'ghmc n {n} bins {bins} m {mmt} mask {masked} call {call}: loss err {e_l:.2e}  dz err {e_d:.2e} '
              f'(f32 {f_d:.2e}, ratio {ratio:.2f})')
        assert e_l <= 1e-5, (gl, rl)
        assert ratio <= BAR, (ratio, e_d, f_d)
        dead = (t == -1) if mask is None else ((t == -1) | ~(mask > 0))
        assert bool((gd[dead] == 0).all())
        if mmt > 0:
            got_acc = acc_dev.cpu().double()
            assert float((got_acc - acc64).abs().max()) <= 1e-6 * float(acc64.abs().max()), (got_acc, acc64)
            if call == 0:                                  # integer counts: (1 - m) count_b to float32 rounding
                counts = LRR.ghmc_counts(z, t, bins, mask)
                assert int(counts.sum()) == int((~dead).sum())
                assert torch.equal(acc_dev.cpu(), torch.tensor(1.0 - mmt, dtype=torch.float32) * counts.float())


def test_ghmc_same_bits_and_value_without_dz(dev):
    """two runs from the same state give the same bits in loss, dz and acc_sum; dz = NULL gives the loss' bits"""
    z, t, mask = _ghmc_draw((1000, 5), 10, 77)
    start = torch.rand(10) * 100
    outs = []
    for grad in (True, True, False):
        acc = start.to(dev)
        l, d = _ghmc_kernel(dev, z, t, mask, 10, 0.75, acc, grad=grad)
        outs.append((l, d, acc.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][2], outs[1][2])
    assert torch.equal(outs[0][0], outs[2][0]) and outs[2][1] is None and torch.equal(outs[0][2], outs[2][2])


def test_ghmc_everything_masked_out_is_nan(dev):
    from deeptables_amd.models.layers import GHMCLoss
    z, t, _ = _ghmc_draw((50, 1), 10, 78)
    acc = torch.ones(10, device=dev)
    l, _ = _ghmc_kernel(dev, z, t, torch.zeros(50, 1), 10, 0.75, acc)
    assert math.isnan(float(l)) and torch.equal(acc.cpu(), torch.ones(10))          # no bin is non-empty: the state stays
    assert math.isnan(float(GHMCLoss(10, 0.75).calc(z, t, torch.zeros(50, 1), True)))   # the torch body on the CPU agrees


def test_ghmc_calc_dispatches_to_the_device_and_keeps_one_acc_sum(dev, monkeypatch):
    from deeptables_amd.models.layers import GHMCLoss
    z, t, mask = _ghmc_draw((300, 3), 10, 79)
    ghm, twin = GHMCLoss(10, 0.75), GHMCLoss(10, 0.75)
    zd = z.to(dev).requires_grad_(True)
    loss = ghm.calc(zd, t.to(dev))
    assert type(loss.grad_fn).__name__ == '_DeviceGhmcBackward' and loss.dim() == 0
    acc = ghm.acc_sum
    assert acc.is_cuda and acc.dtype == torch.float32
    loss2 = ghm.calc(zd, t.to(dev), mask.to(dev), True)
    assert ghm.acc_sum.data_ptr() == acc.data_ptr()                                  # updated in place
    loss2.backward()
    monkeypatch.setenv('DT_AMD_DEVICE_LOSS', '0')
    zt = z.to(dev).requires_grad_(True)
    want = twin.calc(zt, t.to(dev))
    assert type(want.grad_fn).__name__ != '_DeviceGhmcBackward'
    want2 = twin.calc(zt, t.to(dev), mask.to(dev), True)
    want2.backward()
    assert abs(float(loss.detach()) - float(want.detach())) <= 1e-5 and abs(float(loss2.detach()) - float(want2.detach())) <= 1e-5
    assert torch.allclose(ghm.acc_sum, twin.acc_sum.to(dev), rtol=1e-6, atol=0)
    assert P.max_rel(zd.grad, zt.grad) <= 1e-5


# ===========================================================================================================================
# captured graphs
# ===========================================================================================================================
def _capture(dev, static_z, step):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                # warm-up off the default stream, as torch asks
        for _ in range(2):
            step(static_z)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss, grad = step(static_z)
    return graph, loss, grad


def test_huber_loss_and_backward_replay_from_a_captured_graph(dev):
    from deeptables_amd import losses
    za, t = _draw('huber', 2049, 1, 9)
    zb, _ = _draw('huber', 2049, 1, 10)
    td, unit = t.to(dev), losses.unit_grad(dev)

    def step(zz):
        loss = losses.named_loss('huber', zz, td, None, 0.5)
        assert type(loss.grad_fn).__name__ == '_DeviceRegLossBackward'
        (g,) = torch.autograd.grad(loss, zz, unit)
        return loss, g

    def eager(zv):
        loss, g = step(zv.to(dev).requires_grad_(True))
        return loss.detach().clone(), g.clone()
    want_a, want_b = eager(za), eager(zb)
    static_z = za.to(dev).requires_grad_(True)
    graph, loss, grad = _capture(dev, static_z, step)
    for zv, want in ((zb, want_b), (za, want_a)):
        with torch.no_grad():
            static_z.copy_(zv.to(dev))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss.detach(), want[0]) and torch.equal(grad, want[1])


def test_ghmc_replays_update_acc_sum_like_eager_calls(dev):
    from deeptables_amd import losses
    from deeptables_amd.models.layers import GHMCLoss
    shape = (1000, 5)
    draws = [_ghmc_draw(shape, 10, 90 + i) for i in range(3)]
    td, unit = draws[0][1].to(dev), losses.unit_grad(dev)
    eager_ghm, ghm = GHMCLoss(10, 0.75), GHMCLoss(10, 0.75)

    def make(obj):
        def step(zz):
            loss = obj.calc(zz, td)
            (g,) = torch.autograd.grad(loss, zz, unit)
            return loss, g
        return step
    want = []
    for z, _, _ in draws:
        l, g = make(eager_ghm)(z.to(dev).requires_grad_(True))
        want.append((l.detach().clone(), g.clone(), eager_ghm.acc_sum.clone()))
    static_z = draws[0][0].to(dev).requires_grad_(True)
    graph, loss, grad = _capture(dev, static_z, make(ghm))
    acc = ghm.acc_sum
    acc.zero_()                                                   # (the warm-up calls moved it)
    for (z, _, _), (wl, wg, wacc) in zip(draws, want):
        with torch.no_grad():
            static_z.copy_(z.to(dev))
        graph.replay()
        torch.cuda.synchronize()
        assert ghm.acc_sum.data_ptr() == acc.data_ptr()
        assert torch.equal(loss.detach(), wl) and torch.equal(grad, wg) and torch.equal(acc, wacc)
    assert float(acc.sum()) > 0


# ===========================================================================================================================
# through the model: ['dnn_nets'], 3 categorical + 2 dense columns, hidden (8, 4), B = 64
# ===========================================================================================================================
MODEL_NAMES = {'huber': 'huber', 'log_cosh': 'log_cosh', 'msle': 'msle', 'mape': 'mape', 'poisson': 'poisson'}


def _regression_model(loss):
    """the regression model with its output moved to about 3, inside the domain of MSLE and Poisson"""
    dm = _model('regression', 1, loss)
    with torch.no_grad():
        dm.model.layers_by_name['task_output'].bias.fill_(3.0)
    return dm


def _dense_grads(dm):
    return {k: p.grad.detach().clone() for k, p in dm.model.named_parameters() if p.grad is not None and not p.grad.is_sparse}


@pytest.mark.parametrize('name', list(MODEL_NAMES))
def test_train_step_device_loss_against_torch_loss(dev, monkeypatch, name):
    """The loss and the parameter gradients of one step (forward_backward, the body of train_step before the optimizer) from
    identical state with DT_AMD_DEVICE_LOSS=1, with =0, and with the float64 restatement's dz (rounded to float32) pushed
    through the same backward kernels: the kernel leg's loss and every dense parameter gradient are within yardstick B of
    the reference leg, the torch leg being the float32 class.  The gradients themselves are compared, not the parameters an
    SGD step leaves: MSLE's gradients are small enough that a step of 0.01 moves a weight by a few hundred of its own
    roundings, and one flipped rounding of the stored weight then measures the weight's resolution instead of the loss."""
    kind = MODEL_NAMES[name]
    df, rng = _frame(B, 1)
    ins = _inputs(df, dev)
    y = torch.as_tensor((rng.rand(B, 1) * 3 + 0.1).astype(np.float32))
    yd = y.to(dev)
    legs = {}
    start = _regression_model(name).model.state_dict()
    for leg in ('kernel', 'torch', 'reference'):
        dm = _regression_model(name)
        dm.model.load_state_dict(start)
        monkeypatch.setenv('DT_AMD_DEVICE_LOSS', '0' if leg == 'torch' else '1')
        if leg == 'kernel':
            dm.model.train()
            probe = dm._loss(dm.model(ins), yd)
            assert type(probe.grad_fn).__name__ == '_DeviceRegLossBackward'
            dm = _regression_model(name)                          # (the probe's forward moved the batch-norm statistics)
            dm.model.load_state_dict(start)
        if leg == 'reference':                                    # (every leg's forward gives the kernel leg's logits, bit for bit)
            z = legs['kernel'][1].reshape(B, -1)
            assert LRR.kink_margin(kind, z, y) >= MARGIN and float(z.min()) >= 0.05
            ref_l, ref_dz = LRR.value_and_grad(kind, z, y.reshape(B, -1))
            dzr = ref_dz.float().to(dev)
            dm._loss = lambda logit, yy, sw=None: (logit.reshape(B, -1) * dzr).sum()
        l, logit = dm.forward_backward(ins, yd)
        legs[leg] = (l.detach().cpu().double(), logit.detach().cpu(), _dense_grads(dm))
    assert torch.equal(legs['kernel'][1], legs['torch'][1]) and torch.equal(legs['kernel'][1], legs['reference'][1])
    rl = float(ref_l)
    e_l, f_l = abs(float(legs['kernel'][0]) - rl) / abs(rl), abs(float(legs['torch'][0]) - rl) / abs(rl)
    figures = {'loss': e_l / max(f_l, FLOOR)}
    moved = 0
    for k, gr in legs['reference'][2].items():
        gk, gt = legs['kernel'][2][k], legs['torch'][2][k]
        if float(gr.abs().max()) == 0.0:
            assert torch.equal(gk, gr) and torch.equal(gt, gr), k
            continue
        moved += 1
        figures[k] = P.max_rel(gk, gr) / max(P.max_rel(gt, gr), FLOOR)
    P.record('train_step_reg', case=name, **figures)
    print(name, {k: round(v, 3) for k, v in figures.items()})
    assert moved >= 6, sorted(legs['reference'][2])
    bad = {k: v for k, v in figures.items() if not v <= BAR}
    assert not bad, bad
    assert abs(float(legs['kernel'][0]) - rl) <= 1e-4 * max(1.0, abs(rl))


def _first_step(dev, twin, df, y, w, delta):
    twin.model.train()
    with torch.no_grad():
        z = twin.model(_inputs(df.iloc[:B], dev)).cpu().reshape(B, -1)
    t = y.reshape(B, -1)
    ref = float(LRR.total('huber', z.double(), t.double(), None if w is None else w.double(), delta))
    f32 = float(LRR.total('huber', z, t, w, delta))
    return ref, f32


def test_fit_with_huber_by_name_and_in_the_serialised_form(dev):
    """fit(loss='huber') and fit(loss={'class_name': 'Huber', 'config': {'delta': 0.5}}, sample_weight=...) run, and their
    first-step loss is the restatement's.  Without the feature: 'Unsupported loss: huber'."""
    df, rng = _frame(B, 3)
    y = rng.randn(B).astype(np.float32) * 2
    w = (rng.rand(B) * 2 + 0.25).astype(np.float32)
    for loss, delta, sw in (('huber', 1.0, None), ({'class_name': 'Huber', 'config': {'delta': 0.5}}, 0.5, w)):
        twin, dm = (_model('regression', 1, loss) for _ in range(2))
        dm.model.load_state_dict(twin.model.state_dict())
        assert dm.loss_name == 'huber' and dm.fused_plan() is None
        ref, f32 = _first_step(dev, twin, df, torch.as_tensor(y), None if sw is None else torch.as_tensor(sw), delta)
        got = _fit_first_loss(dm, df, y, **({} if sw is None else {'sample_weight': sw}))
        ratio = abs(got - ref) / abs(ref) / max(abs(f32 - ref) / abs(ref), FLOOR)
        P.record('fit_first_loss', case=f'huber_{delta}', ratio=ratio)
        print('huber', delta, 'fit', got, 'ref', ref, 'ratio', ratio)
        assert ratio <= BAR and abs(got - ref) <= 1e-4 * max(1.0, abs(ref))


@pytest.mark.parametrize('spe', (1, 4), ids=('eager', 'steps_per_execution_4'))
def test_fit_with_ghmc_loss_on_a_binary_task(dev, spe):
    """fit(loss=GHMCLoss(bins=10, momentum=0.75)) trains a separable toy set — eagerly and with four steps per captured
    graph — with a decreasing loss and a non-zero acc_sum on the device.  Without the feature: TypeError."""
    from deeptables_amd.models.layers import GHMCLoss
    df, rng = _frame(4 * B, 6)
    labels = (df['I0'].to_numpy() + 0.5 * df['I1'].to_numpy() > 0).astype(np.int64)
    ghm = GHMCLoss(bins=10, momentum=0.75)
    dm = _model('binary', 2, ghm)
    assert dm.loss_name == 'GHMCLoss'
    h = dm.fit(df, labels, batch_size=B, epochs=8, verbose=0, validation_split=0, shuffle=False, steps_per_execution=spe)
    losses = [float(v) for v in h.history['loss']]
    print('ghmc fit', spe, losses, ghm.acc_sum)
    assert all(math.isfinite(v) for v in losses) and losses[-1] < losses[0]
    assert ghm.acc_sum.is_cuda and ghm.acc_sum.dtype == torch.float32 and float(ghm.acc_sum.sum()) > 0
    with pytest.raises(ValueError, match='GHMCLoss'):
        dm.train_step(_inputs(df.iloc[:B], dev), torch.as_tensor(labels[:B]).float().reshape(B, 1).to(dev),
                      torch.ones(B, device=dev))
