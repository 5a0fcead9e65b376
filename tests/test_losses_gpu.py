# -*- coding:utf-8 -*-
"""GPU: the loss kernels of csrc/loss.hip (dt_loss) against the float64 restatement of tests/loss_reference.py, the autograd
function over them (losses.device_loss), and the losses through DeepModel's train_step, fit and evaluate.

Bars, both from the project: yardstick B of tests/precision.py — the kernel's error is at most STEP_BAR['fp32'] x
max(err_f32, FLOOR), err_f32 the error of the same restatement evaluated in float32 on the CPU; relative error for the
loss, max_rel for dz — and, as an outer cap, the blanket bars of DESIGN §1: the loss within 1e-4 of max(1, |ref|), dz within
2e-4 of its largest entry.  Every measured ratio goes through precision.record.

Geometry of csrc/loss.hip that the shapes walk: the element-wise kinds take 2048 elements per block (one launch up to 2048
elements); the categorical kinds take one wave per row, 4 rows per block, classes <= 64 in registers and a loop above, and one
launch while rows <= 64 and rows x classes <= 16384.

Clamp boundary of the focal losses: no element of any focal case lies within 1e-3 of a bound (|z| = 16.1181 for the binary
loss, log p = ln eps or ln(1 - eps) for the categorical one); `_check` asserts it on the float64 reference before the kernel
runs, and nothing is masked out of a comparison.  One consequence for the categorical focal loss: a row with one logit 80
above the rest puts its top class at log p = 0, 1e-7 from ln(1 - eps), so that row cannot be part of its set — the focal set
has a row with one logit 80 BELOW the rest, rows whose two largest logits tie at 88 and at 0, and a row with one logit 5
above the rest instead; CCE, which has no clamp, gets the row as stated."""
import math
import os

import numpy as np
import pytest
import torch

from tests import loss_reference as LR
from tests import precision as P

pytestmark = pytest.mark.gpu

BAR, FLOOR = P.STEP_BAR['fp32'], P.FLOOR
MARGIN = 1e-3


# ===========================================================================================================================
# kernel level
# ===========================================================================================================================
def _kernel(dev, kind, z, t, w=None, gamma=2.0, alpha=0.25, grad=True):
    """dt_loss through ctypes on poisoned outputs and workspace -> (loss [1], dz or None) on the host"""
    from deeptables_amd import _lib
    from deeptables_amd._lib import check, ptr, stream_ptr
    h = _lib.lib()
    assert z.dtype == torch.float32 and t.dtype == torch.float32 and z.shape == t.shape
    zd, td = z.to(dev).contiguous(), t.to(dev).contiguous()
    wd = None if w is None else w.to(dev).contiguous()
    rows, classes = z.shape
    need = h.dt_loss_workspace_bytes(rows, classes)
    assert need >= 8 and need % 8 == 0
    ws = torch.full((need // 8,), float('nan'), dtype=torch.float64, device=dev)
    loss = torch.full((1,), float('nan'), dtype=torch.float32, device=dev)
    dz = torch.full_like(zd, float('nan')) if grad else None
    check(h.dt_loss(LR.kind_code(kind), ptr(zd), ptr(td), ptr(wd), rows, classes, gamma, alpha, ptr(loss), ptr(dz), ptr(ws),
                    stream_ptr()), 'dt_loss')
    torch.cuda.synchronize()
    return loss.cpu(), (None if dz is None else dz.cpu())


def _bars(name, kind, ref, f32, got, what):
    """yardstick B and the blanket cap for (loss, dz) triples; returns the two ratios"""
    (rl, rd), (fl, fd), (gl, gd) = ref, f32, got
    assert torch.isfinite(gl).all() and torch.isfinite(gd).all(), (name, what)
    rl, fl, gl = float(rl), float(fl), float(gl)
    assert rl != 0.0 and float(rd.abs().max()) > 0.0, (name, what, 'a degenerate case measures nothing')
    e_l, f_l = abs(gl - rl) / abs(rl), abs(fl - rl) / abs(rl)
    e_d, f_d = P.max_rel(gd, rd), P.max_rel(fd, rd)
    r_l, r_d = e_l / max(f_l, FLOOR), e_d / max(f_d, FLOOR)
    P.record(name, kind=kind, what=str(what), loss_ratio=r_l, dz_ratio=r_d, loss_err=e_l, dz_err=e_d, loss_f32=f_l, dz_f32=f_d)
    print(f'{name} {kind} {what}: loss err {e_l:.2e} (f32 {f_l:.2e}, ratio {r_l:.2f})  dz err {e_d:.2e} (f32 {f_d:.2e}, '
          f'ratio {r_d:.2f})')
    assert r_l <= BAR and r_d <= BAR, (name, kind, what, r_l, r_d, e_l, f_l, e_d, f_d)
    assert abs(gl - rl) <= 1e-4 * max(1.0, abs(rl)), (name, kind, what, gl, rl)
    assert e_d <= 2e-4, (name, kind, what, e_d)
    return r_l, r_d


def _check(name, dev, kind, z, t, w=None, gamma=2.0, alpha=0.25, what=''):
    margin = LR.clamp_margin(kind, z)
    assert margin >= MARGIN, (name, kind, what, 'an element lies within 1e-3 of a clamp bound', margin)
    ref = LR.value_and_grad(kind, z, t, w, gamma, alpha, torch.float64)
    f32 = LR.value_and_grad(kind, z, t, w, gamma, alpha, torch.float32)
    got = _kernel(dev, kind, z, t, w, gamma, alpha)
    return _bars(name, kind, ref, f32, got, what)


def _draw(kind, B, C, seed):
    """(z, t) float32: logits at a scale that keeps the focal losses off their clamp bounds (asserted by _check), targets
    0 / 1 for the binary kinds, real for mse / mae, one-hot for the categorical kinds"""
    g = torch.Generator().manual_seed(1000 * seed + 7 * B + C)
    scale = {'bce': 3.0, 'binary_focal': 3.0, 'mse': 1.0, 'mae': 1.0, 'cce': 2.0, 'categorical_focal': 1.0}[kind]
    z = torch.randn(B, C, generator=g) * scale
    if kind in ('bce', 'binary_focal'):
        t = (torch.rand(B, C, generator=g) < 0.4).float()
    elif kind in ('mse', 'mae'):
        t = torch.randn(B, C, generator=g)
    else:
        t = torch.eye(C)[torch.randint(0, C, (B,), generator=g)]
    return z, t


def _weights(B, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.rand(B, generator=g) * 2 + 0.25
    if B > 2:
        w[0] = 0.0
    return w


ELEM_SHAPES = [(B, C) for C in (1, 3) for B in (1, 63, 64, 65, 1000)] + \
    [(2047, 1), (2048, 1), (2049, 1), (683, 3), (4096, 1), (4097, 1), (1366, 3)]       # 2048 elements per block, +-1
CAT_SHAPES = [(B, C) for C in (2, 3, 63, 64, 65, 200) for B in (1, 63, 64, 65, 1000)] + \
    [(5, 4096),                                   # the class limit
     (3, 3), (4, 3), (5, 3), (66, 3), (67, 3),    # rows per wave of the one-block path; 4 rows per block, +-1 and +-2
     (64, 256), (64, 257), (63, 261)]             # 16384 elements: the last one-launch shape, and the first two past it


@pytest.mark.parametrize('kind', LR.ELEMENTWISE)
@pytest.mark.parametrize('shape', ELEM_SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_elementwise_kinds_at_every_launch_path(dev, kind, shape):
    B, C = shape
    z, t = _draw(kind, B, C, 1)
    _check('elementwise', dev, kind, z, t, None, 2.0, 0.25, what=(B, C, 'unweighted'))
    if kind != 'binary_focal':
        _check('elementwise', dev, kind, z, t, _weights(B, 3), what=(B, C, 'weighted'))


@pytest.mark.parametrize('kind', LR.CATEGORICAL)
@pytest.mark.parametrize('shape', CAT_SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_categorical_kinds_at_every_launch_path(dev, kind, shape):
    B, C = shape
    assert B * C <= 300000
    z, t = _draw(kind, B, C, 2)
    _check('categorical', dev, kind, z, t, None, 2.0, 0.25, what=(B, C, 'unweighted'))
    _check('categorical', dev, kind, z, t, _weights(B, 4), what=(B, C, 'weighted'))


HARD_LOGITS = (0.0, 16.0, -16.0, 16.3, -16.3, 30.0, -30.0, 88.0, -88.0)


def _hard_elementwise():
    """every hard logit against the targets 0, 1 and 0.5 -> z, t [9, 3]; weights with 0 and 1e3"""
    z = torch.tensor(HARD_LOGITS).repeat_interleave(3).reshape(9, 3)
    t = torch.tensor([0.0, 1.0, 0.5]).repeat(9).reshape(9, 3)
    w = torch.tensor([1.0, 0.0, 1e3, 0.5, 2.0, 1.0, 0.0, 1e3, 1.0])
    return z, t, w


@pytest.mark.parametrize('kind', LR.ELEMENTWISE)
def test_elementwise_kinds_on_hard_inputs(dev, kind):
    """logits 0, +-16.0, +-16.3, +-30, +-88 against targets 0, 1 and 0.5 (the binary focal loss: both constants, no gradient),
    an element with z == t == 0 (sign(0) = 0), weights 0 and 1e3, gamma 0 / 0.5 / 2 / 5"""
    z, t, w = _hard_elementwise()
    gammas = (0.0, 0.5, 2.0, 5.0) if kind == 'binary_focal' else (2.0,)
    for gamma in gammas:
        for alpha in (0.25, 0.6):
            _check('hard', dev, kind, z, t, None, gamma, alpha, what=('gamma', gamma, 'alpha', alpha))
            if kind != 'binary_focal':
                _check('hard', dev, kind, z, t, w, gamma, alpha, what=('weighted',))
            if kind != 'binary_focal':
                break


def _hard_cce():
    z = torch.tensor([[2.0, 2.0, 2.0, 2.0, 2.0],                 # equal logits
                      [83.0, 3.0, 3.0, 3.0, 3.0],                # one logit 80 above the rest
                      [0.0, 16.0, -16.0, 16.3, -16.3],
                      [30.0, -30.0, 88.0, -88.0, 0.0],
                      [30.0, -30.0, 88.0, -88.0, 0.0],
                      [-1.0, 0.5, 0.25, 2.0, -3.0],
                      [-1.0, 0.5, 0.25, 2.0, -3.0],
                      [83.0, 3.0, 3.0, 3.0, 3.0]])
    t = torch.eye(5)[[0, 0, 2, 3, 2, 1, 4, 1]]                   # row 3: the class at log p = -176; row 7: at log p = -80
    t[5] = torch.tensor([0.2, 0.1, 0.0, 0.3, 0.1])               # soft, sums to 0.7
    t[6] = torch.tensor([0.9, 0.8, 0.0, 0.0, 0.5])               # soft, sums to 2.2
    w = torch.tensor([1.0, 1e3, 0.0, 1.0, 2.0, 1e3, 0.5, 0.0])
    return z, t, w


def _hard_categorical_focal():
    z = torch.tensor([[2.0, 2.0, 2.0, 2.0, 2.0],                 # equal logits
                      [88.0, 88.0, 30.0, -30.0, -88.0],          # the two largest tie: log p = -0.69, the rest clamped
                      [88.0, 88.0, 30.0, -30.0, -88.0],
                      [16.3, 16.0, 0.0, -16.0, -16.3],
                      [16.3, 16.0, 0.0, -16.0, -16.3],
                      [0.0, 0.0, -16.0, -16.3, -30.0],
                      [0.0, 0.0, 0.0, 0.0, -80.0],               # one logit 80 below the rest
                      [5.0, 0.0, 0.0, 0.0, 0.0],                 # one logit 5 above the rest
                      [-1.0, 0.5, 0.25, 2.0, -3.0]])
    t = torch.eye(5)[[0, 0, 4, 1, 4, 2, 4, 0, 1]]                # rows 2, 4, 5, 6: the target sits on a clamped class
    t[8] = torch.tensor([0.2, 0.1, 0.0, 0.3, 0.1])
    w = torch.tensor([1.0, 1e3, 0.0, 1.0, 2.0, 1e3, 0.5, 1.0, 0.0])
    return z, t, w


def test_cce_on_hard_inputs(dev):
    z, t, w = _hard_cce()
    _check('hard', dev, 'cce', z, t, None, what=('unweighted',))
    _check('hard', dev, 'cce', z, t, w, what=('weighted',))


@pytest.mark.parametrize('gamma', (0.0, 0.5, 2.0, 5.0))
def test_categorical_focal_on_hard_inputs(dev, gamma):
    z, t, w = _hard_categorical_focal()
    for alpha in (0.25, 0.6):
        _check('hard', dev, 'categorical_focal', z, t, None, gamma, alpha, what=('gamma', gamma, 'alpha', alpha))
        _check('hard', dev, 'categorical_focal', z, t, w, gamma, alpha, what=('gamma', gamma, 'alpha', alpha, 'weighted'))


@pytest.mark.parametrize('kind,shape', [('bce', (65, 3)), ('bce', (1000, 3)), ('mae', (2049, 1)), ('binary_focal', (1000, 3)),
                                        ('cce', (64, 3)), ('cce', (1000, 200)), ('categorical_focal', (5, 4096)),
                                        ('categorical_focal', (67, 65))])
def test_same_bits_on_every_call_and_without_dz(dev, kind, shape):
    z, t = _draw(kind, *shape, 5)
    w = None if kind == 'binary_focal' else _weights(shape[0], 6)
    l1, d1 = _kernel(dev, kind, z, t, w)
    l2, d2 = _kernel(dev, kind, z, t, w)
    l3, d3 = _kernel(dev, kind, z, t, w, grad=False)
    assert torch.equal(l1, l2) and torch.equal(d1, d2) and torch.equal(l1, l3) and d3 is None
    assert torch.isfinite(l1).all() and torch.isfinite(d1).all()


def test_autograd_unit_gradient_and_scaled_gradient(dev):
    """backward returns the saved dz ITSELF for losses.unit_grad (no launch) and dz * g for any other scalar"""
    from deeptables_amd import _lib, losses
    z0, t = _draw('cce', 65, 3, 7)
    z = z0.to(dev).requires_grad_(True)
    loss = losses.device_loss(_lib.DT_LOSS_CCE, z, t.to(dev), _weights(65, 8).to(dev))
    assert type(loss.grad_fn).__name__ == '_DeviceLossBackward' and loss.dim() == 0 and loss.dtype == torch.float32
    saved = loss.grad_fn.saved_tensors[0]
    (g1,) = torch.autograd.grad(loss, z, losses.unit_grad(dev), retain_graph=True)
    assert g1.data_ptr() == saved.data_ptr() and torch.equal(g1, saved)
    s = torch.tensor(0.375, device=dev)
    (g2,) = torch.autograd.grad(loss, z, s)
    assert g2.data_ptr() != saved.data_ptr() and torch.equal(g2, saved * s)
    kl, kd = _kernel(dev, 'cce', z0, t, _weights(65, 8))
    assert torch.equal(loss.detach().cpu().reshape(1), kl) and torch.equal(saved.cpu(), kd)
    with torch.no_grad():                                        # evaluate: the value only, the same bits
        lv = losses.device_loss(_lib.DT_LOSS_CCE, z, t.to(dev), _weights(65, 8).to(dev))
    assert lv.grad_fn is None and torch.equal(lv.cpu().reshape(1), kl)


def test_loss_and_backward_replay_from_a_captured_graph(dev):
    """CCE, B = 64, C = 3: one capture of loss + backward, replayed on new logits in the static buffers = the eager bits"""
    from deeptables_amd import _lib, losses
    za, t = _draw('cce', 64, 3, 9)
    zb, _ = _draw('cce', 64, 3, 10)
    td = t.to(dev)
    unit = losses.unit_grad(dev)

    def eager(zv):
        zz = zv.to(dev).requires_grad_(True)
        loss = losses.device_loss(_lib.DT_LOSS_CCE, zz, td)
        (g,) = torch.autograd.grad(loss, zz, unit)
        return loss.detach().clone(), g.clone()
    want_a, want_b = eager(za), eager(zb)
    static_z = za.to(dev).requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                # warm-up off the default stream, as torch asks
        for _ in range(2):
            loss = losses.device_loss(_lib.DT_LOSS_CCE, static_z, td)
            torch.autograd.grad(loss, static_z, unit)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = losses.device_loss(_lib.DT_LOSS_CCE, static_z, td)
        (grad,) = torch.autograd.grad(loss, static_z, unit)
    for zv, want in ((zb, want_b), (za, want_a)):
        with torch.no_grad():
            static_z.copy_(zv.to(dev))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss.detach(), want[0]) and torch.equal(grad, want[1])


# ===========================================================================================================================
# through the model: ['dnn_nets'], 3 categorical + 2 dense columns, B = 64
# ===========================================================================================================================
VOCABS, D, B = (7, 9, 11), 4, 64
TOWER = ((8, 0, False), (4, 0, False))


def _model(task, num_classes, loss):
    from deeptables_amd import functional
    from deeptables_amd.models import ModelConfig, DeepModel
    from deeptables_amd.models.metainfo import CategoricalColumn, ContinuousColumn
    functional.set_seed(33)
    conf = ModelConfig(nets=['dnn_nets'], fixed_embedding_dim=True, embeddings_output_dim=D, embedding_dropout=0,
                       dense_dropout=0, metrics=[], optimizer='sgd', loss=loss,
                       dnn_params={'hidden_units': TOWER, 'activation': 'relu'})
    cats = [CategoricalColumn(f'C{i}', v, D) for i, v in enumerate(VOCABS)]
    conts = [ContinuousColumn('input_continuous_all', ['I0', 'I1'])]
    dm = DeepModel(task, num_classes, conf, cats, conts)
    dm.build()
    dm.model.train()
    return dm


def _frame(n, seed=0):
    import pandas as pd
    rng = np.random.RandomState(seed)
    df = pd.DataFrame({f'C{i}': rng.randint(0, v, n) for i, v in enumerate(VOCABS)})
    df['I0'] = rng.randn(n).astype(np.float32)
    df['I1'] = rng.randn(n).astype(np.float32)
    return df, rng


def _inputs(df, dev):
    idx = torch.as_tensor(df[[f'C{i}' for i in range(3)]].to_numpy().astype(np.int32))
    dense = torch.as_tensor(df[['I0', 'I1']].to_numpy().astype(np.float32))
    return [idx.to(dev), dense.to(dev)]


def _floats(dm):
    return {k: v.detach().clone() for k, v in dm.model.state_dict().items() if v.is_floating_point()}


STEP_CASES = {
    'multiclass': ('multiclass', 3, 'auto', 'cce'),
    'regression_mae': ('regression', 1, 'mae', 'mae'),
    'multilabel_class_weight': ('multilabel', 3, 'auto', 'bce'),
}


@pytest.mark.parametrize('case', list(STEP_CASES))
def test_train_step_device_loss_against_torch_loss(dev, monkeypatch, case):
    """One SGD train_step from identical state with DT_AMD_DEVICE_LOSS=1, with =0, and with the float64 restatement's dz
    (rounded to float32) pushed through the same backward kernels: the kernel leg's loss and every updated parameter are
    within yardstick B of the reference leg, the torch leg being the float32 class.  (SGD: the update is linear in dz.)"""
    from deeptables_amd import training
    task, nc, loss, kind = STEP_CASES[case]
    df, rng = _frame(B, 1)
    ins = _inputs(df, dev)
    w = None
    if task == 'multiclass':
        y = torch.eye(3)[torch.as_tensor(rng.randint(0, 3, B))]
    elif task == 'regression':
        y = torch.as_tensor(rng.randn(B, 1).astype(np.float32))
    else:
        y = torch.as_tensor((rng.rand(B, 3) < 0.4).astype(np.float32))
        cw = {0: 0.5, 1: 3.0, 2: 1.5}                             # fit's mapping: the weight of a row's argmax label
        w = torch.tensor([cw[int(k)] for k in y.argmax(-1)])
    yd, wd = y.to(dev), (None if w is None else w.to(dev))
    legs = {}
    base = _model(task, nc, loss)
    start = base.model.state_dict()
    before = _floats(base)
    for leg in ('kernel', 'torch', 'reference'):
        dm = _model(task, nc, loss)
        dm.model.load_state_dict(start)
        monkeypatch.setenv('DT_AMD_DEVICE_LOSS', '0' if leg == 'torch' else '1')
        if leg == 'kernel':
            dm.model.train()
            probe = dm._loss(dm.model(ins), yd, wd)
            assert type(probe.grad_fn).__name__ == '_DeviceLossBackward'
            dm = _model(task, nc, loss)                           # (the probe's forward moved the batch-norm statistics)
            dm.model.load_state_dict(start)
        if leg == 'reference':                                    # (every leg's forward gives the kernel leg's logits, bit for bit)
            ref_l, ref_dz = LR.value_and_grad(kind, legs['kernel'][1].reshape(B, -1), y.reshape(B, -1), w)
            dzr = ref_dz.float().to(dev)
            dm._loss = lambda logit, yy, sw=None: (logit.reshape(B, -1) * dzr).sum()
        l, logit = dm.train_step(ins, yd, wd)
        legs[leg] = (l.detach().cpu().double(), logit.detach().cpu(), _floats(dm))
    assert torch.equal(legs['kernel'][1], legs['torch'][1]) and torch.equal(legs['kernel'][1], legs['reference'][1])
    rl = float(ref_l)
    e_l, f_l = abs(float(legs['kernel'][0]) - rl) / abs(rl), abs(float(legs['torch'][0]) - rl) / abs(rl)
    figures = {'loss': e_l / max(f_l, FLOOR)}
    moved = 0
    for k, p0 in before.items():
        ur, uk, ut = (legs[leg][2][k].double().cpu() - p0.double().cpu() for leg in ('reference', 'kernel', 'torch'))
        if float(ur.abs().max()) == 0.0:
            assert torch.equal(uk, ur) and torch.equal(ut, ur), k
            continue
        moved += 1
        figures[k] = P.max_rel(uk, ur) / max(P.max_rel(ut, ur), FLOOR)
    P.record('train_step', case=case, **figures)
    print(case, {k: round(v, 3) for k, v in figures.items()})
    assert moved >= 6, sorted(before)
    bad = {k: v for k, v in figures.items() if not v <= BAR}
    assert not bad, bad
    assert abs(float(legs['kernel'][0]) - rl) <= 1e-4 * max(1.0, abs(rl))


def _first_step_loss(dev, dm_twin, df, y, w, kind, gamma=2.0, alpha=0.25):
    """(float64 restatement, float32 restatement) of the first step's loss: the twin's training-mode logits of rows 0 .. B-1"""
    dm_twin.model.train()
    with torch.no_grad():
        logit = dm_twin.model(_inputs(df.iloc[:B], dev)).cpu()
    z = logit.reshape(B, -1)
    ref = float(LR.total(kind, z.double(), y.double().reshape(B, -1), None if w is None else w.double(), gamma, alpha))
    f32 = float(LR.total(kind, z, y.reshape(B, -1), w, gamma, alpha))
    return ref, f32


def _fit_first_loss(dm, df, labels, **kw):
    h = dm.fit(df, labels, batch_size=B, epochs=1, verbose=0, validation_split=0, shuffle=False, **kw)
    return float(h.history['loss'][0])


def test_fit_with_categorical_focal_loss_and_class_weight(dev):
    """fit(loss=CategoricalFocalLoss(), class_weight=...) — the imbalanced-data case — runs, on the kernel, and its first-step
    loss is the restatement's.  Without the feature losses.named_loss raises ValueError for this loss."""
    from deeptables_amd.models.layers import CategoricalFocalLoss
    df, rng = _frame(B, 2)
    labels = rng.randint(0, 3, B)
    cw = {0: 0.5, 1: 4.0, 2: 1.0}
    w = torch.tensor([cw[int(k)] for k in labels])
    twin, dm = (_model('multiclass', 3, CategoricalFocalLoss(gamma=1.5, alpha=0.4)) for _ in range(2))
    dm.model.load_state_dict(twin.model.state_dict())
    ref, f32 = _first_step_loss(dev, twin, df, torch.eye(3)[torch.as_tensor(labels)], w, 'categorical_focal', 1.5, 0.4)
    got = _fit_first_loss(dm, df, labels, class_weight=cw)
    ratio = abs(got - ref) / abs(ref) / max(abs(f32 - ref) / abs(ref), FLOOR)
    P.record('fit_first_loss', case='categorical_focal_class_weight', ratio=ratio)
    print('categorical focal + class_weight: fit', got, 'ref', ref, 'ratio', ratio)
    assert ratio <= BAR and abs(got - ref) <= 1e-4 * max(1.0, abs(ref))


def test_fit_with_mae_loss(dev):
    """fit(loss='mae') runs and its first-step loss is the restatement's.  Without the feature: 'Unsupported loss: mae'."""
    df, rng = _frame(B, 3)
    y = rng.randn(B).astype(np.float32)
    twin, dm = (_model('regression', 1, 'mae') for _ in range(2))
    dm.model.load_state_dict(twin.model.state_dict())
    ref, f32 = _first_step_loss(dev, twin, df, torch.as_tensor(y).reshape(B, 1), None, 'mae')
    got = _fit_first_loss(dm, df, y)
    ratio = abs(got - ref) / abs(ref) / max(abs(f32 - ref) / abs(ref), FLOOR)
    P.record('fit_first_loss', case='mae', ratio=ratio)
    print('mae: fit', got, 'ref', ref, 'ratio', ratio)
    assert ratio <= BAR and abs(got - ref) <= 1e-4 * max(1.0, abs(ref))
    dm2 = _model('regression', 1, 'mean_absolute_error')
    dm2.model.load_state_dict(twin.model.state_dict())
    assert _fit_first_loss(dm2, df, y) == got


def test_binary_focal_loss_with_sample_weight_raises(dev):
    from deeptables_amd.models.layers import BinaryFocalLoss
    df, rng = _frame(B, 4)
    y = torch.as_tensor((rng.rand(B, 1) < 0.4).astype(np.float32)).to(dev)
    dm = _model('binary', 2, BinaryFocalLoss())
    l, _ = dm.train_step(_inputs(df, dev), y)                    # unweighted: the kernel
    assert math.isfinite(float(l))
    with pytest.raises(ValueError, match='BinaryFocalLoss'):
        dm.train_step(_inputs(df, dev), y, torch.ones(B, device=dev))


def test_evaluate_loss_is_the_weighted_mean_of_the_batch_losses(dev):
    """evaluate on 40 rows in batches of 16, 16 and 8: its loss = sum_b n_b L_b / 40, L_b the kernel's value (dz = NULL) on
    batch b's logits"""
    from deeptables_amd import _lib, losses
    df, rng = _frame(40, 5)
    labels = rng.randint(0, 3, 40)
    dm = _model('multiclass', 3, 'auto')
    got = float(dm.evaluate(df, labels, batch_size=16)['loss'])
    logits = torch.as_tensor(dm._predict(dm.model, df, batch_size=16, activate=False)).to(dev)
    t = torch.eye(3)[torch.as_tensor(labels)].to(dev)
    want, per = 0.0, []
    for s, n in ((0, 16), (16, 16), (32, 8)):
        with torch.no_grad():
            lb = losses.device_loss(_lib.DT_LOSS_CCE, logits[s:s + n], t[s:s + n])
        assert lb is not None and lb.grad_fn is None
        per.append(float(lb))
        want += n * float(lb)
    want /= 40.0
    ref = float(LR.total('cce', logits.cpu().double(), t.cpu().double()))
    print('evaluate', got, 'batches', per, 'weighted mean', want, 'float64 restatement', ref)
    assert abs(got - want) <= 8 * 2.0 ** -24 * max(1.0, abs(want))
    assert abs(got - ref) <= 1e-4 * max(1.0, abs(ref))
