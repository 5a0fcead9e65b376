# -*- coding:utf-8 -*-
"""CPU: the float64 restatement of the losses (tests/loss_reference.py) against the recorded fixtures of the reference's own
code, the host-side dispatch of losses.device_loss / DeepModel._loss with a stubbed library call, the errors, dt_loss'
argument validation (before any launch, so it runs without a GPU) and the ctypes signatures against the header."""
import json
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import loss_reference as LR
from tests import loss_reg_reference as LRR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _logit(p):
    p = torch.as_tensor(np.asarray(p, dtype=np.float64))
    return torch.log(p) - torch.log1p(-p)


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------
def test_restatement_reproduces_the_reference_code_fixtures():
    """the fixtures hold PROBABILITIES; their logits are log(p / (1 - p)) (sigmoid) and log p (softmax, which also restates the
    reference's renormalisation p / sum p)"""
    g = np.load(os.path.join(GOLDEN, 'reference_code_binary_focal_loss.npz'))
    st = json.loads(str(g['meta']))['static']
    got = LR.total('binary_focal', _logit(g['arg:y_pred']), torch.as_tensor(g['arg:y_true']), None, st['gamma'], st['alpha'])
    assert abs(float(got) - float(g['out'])) <= 1e-12 * abs(float(g['out']))
    g = np.load(os.path.join(GOLDEN, 'reference_code_categorical_focal_loss.npz'))
    z = torch.log(torch.as_tensor(g['arg:y_pred']))
    got = LR.per_row('categorical_focal', z, torch.as_tensor(g['arg:y_true']))
    assert np.allclose(got.numpy(), g['out'], rtol=1e-12, atol=0)
    w = torch.linspace(0.0, 3.0, 7, dtype=torch.float64)
    assert abs(float(LR.total('categorical_focal', z, torch.as_tensor(g['arg:y_true']), w)) -
               float((torch.as_tensor(g['out']) * w).sum() / 7)) <= 1e-14
    g = np.load(os.path.join(GOLDEN, 'layer_losses.npz'))
    got = LR.total('binary_focal', _logit(g['pb'].astype(np.float64)), torch.as_tensor(g['yb'].astype(np.float64)))
    assert abs(float(got) - float(g['binary_focal'])) <= 1e-9 * abs(float(g['binary_focal']))
    got = LR.per_row('categorical_focal', torch.log(torch.as_tensor(g['pc'].astype(np.float64))),
                     torch.as_tensor(g['yc'].astype(np.float64)))
    assert np.allclose(got.numpy(), g['categorical_focal'], rtol=1e-9, atol=1e-12)


def test_restatement_closed_forms_and_gradients():
    """bce = the oracle's stable form, with the gradient (sigmoid(z) - t) / C also at z = 0; cce with soft labels that do not sum
    to 1: (sum_k t_k) p - t; mae: sign(0) = 0; weights scale rows"""
    from oracle import reference_layers as R
    z = torch.tensor([0.0, 16.0, -16.3, 30.0, -88.0, 1.3, -0.2, 700.0, -700.0], dtype=torch.float64).repeat_interleave(3).reshape(9, 3)
    t = torch.tensor([0.0, 1.0, 0.5], dtype=torch.float64).repeat(9).reshape(9, 3)
    assert abs(float(LR.total('bce', z, t)) - float(R.binary_crossentropy_from_logits(z, t))) <= 1e-12
    _, dz = LR.value_and_grad('bce', z, t)
    assert float((dz * 27 - (torch.sigmoid(z) - t)).abs().max()) <= 1e-15
    w = torch.linspace(0.0, 4.0, 9, dtype=torch.float64)
    _, dzw = LR.value_and_grad('bce', z, t, w)
    assert torch.allclose(dzw, dz * w[:, None], rtol=1e-14, atol=0)
    zc = torch.tensor([[1.0, -2.0, 0.5], [80.0, 0.0, 0.0]], dtype=torch.float64)
    tc = torch.tensor([[0.2, 0.1, 0.3], [0.9, 0.8, 0.5]], dtype=torch.float64)
    _, dzc = LR.value_and_grad('cce', zc, tc)
    assert torch.allclose(dzc * 2, tc.sum(-1, keepdim=True) * torch.softmax(zc, -1) - tc, rtol=1e-12, atol=1e-18)
    zm = torch.tensor([[1.0, 2.0, 3.0]], dtype=torch.float64)
    _, dzm = LR.value_and_grad('mae', zm, torch.tensor([[1.0, 5.0, 0.0]], dtype=torch.float64))
    assert dzm.tolist() == [[0.0, -1.0 / 3, 1.0 / 3]]
    with pytest.raises(ValueError):
        LR.total('binary_focal', z, t, w)


def test_cpu_paths_keep_their_values():
    """losses.* on CPU tensors (and so with DT_AMD_DEVICE_LOSS=0): the restatement's values in float64"""
    from deeptables_amd import losses
    from deeptables_amd.models.layers import BinaryFocalLoss, CategoricalFocalLoss
    g = torch.Generator().manual_seed(3)
    z = torch.randn(11, 4, generator=g, dtype=torch.float64)
    y = torch.randn(11, 4, generator=g, dtype=torch.float64)
    t = torch.eye(4, dtype=torch.float64)[torch.randint(0, 4, (11,), generator=g)]
    w = torch.rand(11, generator=g, dtype=torch.float64)
    # predictions and targets of the regression names in [1, 1.25]: inside the domain of MSLE and Poisson, and MAPE's value (a
    # percentage) stays below 16, where the absolute bars below are still several float64 ulp
    p, q = (torch.rand(11, 4, generator=g, dtype=torch.float64) * 0.25 + 1.0 for _ in range(2))
    targets = {'bce': (y > 0).double(), 'cce': t, 'mse': y, 'mae': y}
    for name, code in losses.LOSS_KINDS.items():
        if name in losses.REG_LOSS_KINDS:
            kind = next(k for k in LRR.KINDS if LRR.kind_code(k) == code)
            ref, zz, tt = LRR.total, p, q
        else:
            kind = next(k for k in LR.KINDS if LR.kind_code(k) == code)
            ref, zz, tt = LR.total, z, targets[kind]
        for ww, bar in ((None, 1e-14), (w, 1e-12)):
            got, want = float(losses.named_loss(name, zz, tt, ww)), float(ref(kind, zz, tt, ww))
            print(name, 'weighted' if ww is not None else 'unweighted', got, want, abs(got - want))
            assert abs(got - want) <= bar, name
    soft = lambda q: torch.softmax(q, dim=-1)
    cf = CategoricalFocalLoss(gamma=1.5, alpha=0.4)
    assert abs(float(losses.focal_from_logits(5, cf, z, t, w, soft)) - float(LR.total('categorical_focal', z, t, w, 1.5, 0.4))) <= 1e-14
    assert abs(float(losses.focal_from_logits(5, cf, z, t, None, soft)) - float(LR.total('categorical_focal', z, t, None, 1.5, 0.4))) <= 1e-14
    bf = BinaryFocalLoss(gamma=0.5, alpha=0.3)
    tb = (y > 0).double()
    assert abs(float(losses.focal_from_logits(4, bf, z, tb, None, torch.sigmoid)) - float(LR.total('binary_focal', z, tb, None, 0.5, 0.3))) <= 1e-14
    with pytest.raises(ValueError):
        losses.named_loss('hinge', z, y, w)


# ---------------------------------------------------------------------------------------------------------------------------
# dispatch
# ---------------------------------------------------------------------------------------------------------------------------
class _Recorder:
    """stands in for the library handle: records dt_loss calls, launches nothing"""

    def __init__(self):
        self.calls = []

    def dt_loss_workspace_bytes(self, rows, classes):
        return 8 * max(1, (rows + 3) // 4)

    def dt_loss(self, kind, z, t, w, rows, classes, gamma, alpha, loss, dz, ws, stream):
        self.calls.append(dict(kind=kind, w=w is not None, dz=dz is not None, rows=rows, classes=classes, gamma=gamma, alpha=alpha))
        return 0

    def __getattr__(self, name):
        raise AssertionError(f'unexpected library call {name}')


def _fake_model(loss_name, custom=None, activation='softmax'):
    from deeptables_amd.models.deepmodel import DeepModel
    fake = types.SimpleNamespace(loss_name=loss_name, output_activation=activation)
    if custom is not None:
        fake._custom_loss = custom
    fake._activate = lambda logit: DeepModel._activate(fake, logit)
    return lambda logit, y, w=None: DeepModel._loss(fake, logit, y, w)


def test_dispatch_table(monkeypatch):
    """which loss and weight combination goes to dt_loss, with which kind, and which keeps its torch path; tensors are made to
    look device resident and the library call is a recorder.  DT_AMD_DEVICE_LOSS=0: nothing reaches the library."""
    from deeptables_amd import _lib, losses
    from deeptables_amd.models.layers import BinaryFocalLoss, CategoricalFocalLoss
    rec = _Recorder()
    monkeypatch.setattr(losses, 'lib', lambda: rec)
    monkeypatch.setattr(losses, 'stream_ptr', lambda: None)
    monkeypatch.setattr(losses, '_on_device', lambda t: torch.is_tensor(t))
    g = torch.Generator().manual_seed(1)
    z = torch.randn(6, 3, generator=g).requires_grad_(True)
    z1 = torch.randn(6, 1, generator=g).requires_grad_(True)
    onehot = torch.eye(3)[torch.tensor([0, 1, 2, 2, 1, 0])]
    y1 = (torch.rand(6, 1, generator=g) < 0.5).float()
    w = torch.rand(6, generator=g)
    bf, cf = BinaryFocalLoss(gamma=1.5, alpha=0.3), CategoricalFocalLoss(gamma=0.5, alpha=0.6)
    K = _lib
    table = [   # (loss name, custom object, logits, targets, weights) -> DT_LOSS_* kind, or None: not through dt_loss
        ('binary_crossentropy', None, z1, y1, None, None),          # unweighted BCE keeps dt_bce_logits (CPU here: torch)
        ('binary_crossentropy', None, z1, y1, w, K.DT_LOSS_BCE),
        ('binary_crossentropy', None, z, onehot, w, K.DT_LOSS_BCE),  # multilabel
        ('categorical_crossentropy', None, z, onehot, None, K.DT_LOSS_CCE),
        ('categorical_crossentropy', None, z, onehot, w, K.DT_LOSS_CCE),
        ('mse', None, z1, y1, None, K.DT_LOSS_MSE),
        ('mean_squared_error', None, z1, y1, w, K.DT_LOSS_MSE),
        ('mae', None, z1, y1, None, K.DT_LOSS_MAE),
        ('mean_absolute_error', None, z1, y1, w, K.DT_LOSS_MAE),
        ('focal_loss', bf, z1, y1, None, K.DT_LOSS_BINARY_FOCAL),
        ('focal_loss', cf, z, onehot, None, K.DT_LOSS_CATEGORICAL_FOCAL),
        ('focal_loss', cf, z, onehot, w, K.DT_LOSS_CATEGORICAL_FOCAL),
        ('focal_loss', BinaryFocalLoss(reduction='sum'), z1, y1, None, None),
        ('focal_loss', CategoricalFocalLoss(reduction='sum'), z, onehot, None, None),
        ('custom', lambda yt, yp: ((yt - yp) ** 2).mean(), z1, y1, None, None),
        ('categorical_crossentropy', None, z[:, :1], onehot[:, :1], None, None),      # classes = 1: outside the domain
    ]
    for name, custom, zz, yy, ww, kind in table:
        for env in ('1', '0'):
            monkeypatch.setenv('DT_AMD_DEVICE_LOSS', env)
            rec.calls.clear()
            act = 'sigmoid' if zz.shape[1] == 1 else 'softmax'
            loss = _fake_model(name, custom, act)(zz, yy, ww)
            assert loss.dim() == 0
            if kind is None or env == '0':
                assert rec.calls == [], (name, env, rec.calls)
                assert type(loss.grad_fn).__name__ != '_DeviceLossBackward'
                continue
            assert len(rec.calls) == 1, (name, rec.calls)
            c = rec.calls[0]
            assert (c['kind'], c['w'], c['dz'], c['rows'], c['classes']) == (kind, ww is not None, True, 6, zz.shape[1]), (name, c)
            assert type(loss.grad_fn).__name__ == '_DeviceLossBackward'
            if custom is not None:
                assert (c['gamma'], c['alpha']) == (custom.gamma, custom.alpha)
    # evaluate runs under no_grad: the value only
    monkeypatch.setenv('DT_AMD_DEVICE_LOSS', '1')
    rec.calls.clear()
    with torch.no_grad():
        _fake_model('mae')(z1, y1, None)
    assert [c['dz'] for c in rec.calls] == [False]
    # outside the kernel's domain the host keeps its torch path: too many classes, float64 logits
    rec.calls.clear()
    wide = torch.randn(2, _lib.DT_LOSS_MAX_CLASSES + 1)
    assert losses.device_loss(_lib.DT_LOSS_MSE, wide, wide) is None
    assert losses.device_loss(_lib.DT_LOSS_MSE, z1.double(), y1.double()) is None
    assert losses.device_loss(_lib.DT_LOSS_BINARY_FOCAL, z1, y1, w) is None
    assert rec.calls == []
    float(losses.named_loss('mse', wide, wide))


def test_unit_gradient_is_handed_out_without_a_multiply(monkeypatch):
    from deeptables_amd import _lib, losses
    import ctypes

    class Filling(_Recorder):
        def dt_loss(self, kind, z, t, w, rows, classes, gamma, alpha, loss, dz, ws, stream):
            out = (ctypes.c_float * (rows * classes)).from_address(dz.value)
            out[:] = [float(i) for i in range(rows * classes)]
            return 0
    rec = Filling()
    monkeypatch.setattr(losses, 'lib', lambda: rec)
    monkeypatch.setattr(losses, 'stream_ptr', lambda: None)
    monkeypatch.setattr(losses, '_on_device', lambda t: torch.is_tensor(t))
    z = torch.randn(5, 3).requires_grad_(True)
    loss = losses.device_loss(_lib.DT_LOSS_CCE, z, torch.eye(3)[[0, 1, 2, 0, 1]])
    saved = loss.grad_fn.saved_tensors[0]
    assert torch.equal(saved, torch.arange(15.0).reshape(5, 3))
    (g1,) = torch.autograd.grad(loss, z, losses.unit_grad('cpu'), retain_graph=True)
    assert g1.data_ptr() == saved.data_ptr()
    (g2,) = torch.autograd.grad(loss, z, torch.tensor(0.5))
    assert g2.data_ptr() != saved.data_ptr() and torch.equal(g2, saved * 0.5)


# ---------------------------------------------------------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------------------------------------------------------
def test_errors_and_mae_compiles():
    from deeptables_amd.models import ModelConfig, DeepModel
    from deeptables_amd.models.layers import BinaryFocalLoss, CategoricalFocalLoss
    from deeptables_amd.models.metainfo import CategoricalColumn, ContinuousColumn
    z1, y1, w = torch.randn(4, 1), torch.ones(4, 1), torch.ones(4)
    with pytest.raises(ValueError, match='BinaryFocalLoss.*per-row weight'):
        _fake_model('focal_loss', BinaryFocalLoss(), 'sigmoid')(z1, y1, w)
    with pytest.raises(ValueError, match='sample / class weights'):
        _fake_model('focal_loss', CategoricalFocalLoss(reduction='sum'))(torch.randn(4, 3), torch.eye(3)[[0, 1, 2, 0]], w)
    with pytest.raises(ValueError, match='sample / class weights'):
        _fake_model('custom', lambda a, b: (a - b).mean(), 'sigmoid')(z1, y1, w)
    for bad in ('hinge', 'MAE '):
        with pytest.raises(ValueError, match='Unsupported loss'):
            _fake_model(bad)(z1, y1)
        with pytest.raises(ValueError, match='Unsupported loss'):
            _fake_model(bad)(z1, y1, w)
    for name in ('mae', 'mean_absolute_error'):
        conf = ModelConfig(nets=['dnn_nets'], loss=name, embedding_dropout=0,
                           dnn_params={'hidden_units': ((8, 0, False), (4, 0, False)), 'activation': 'relu'})
        dm = DeepModel('regression', 1, conf, [CategoricalColumn('C0', 5, 4)], [ContinuousColumn('input_continuous_all', ['a'])])
        dm.build('cpu')
        assert dm.loss_name == name and dm.model_desc.loss == name
        assert abs(float(dm._loss(z1, y1)) - float((z1 - y1).abs().mean())) <= 1e-7
        assert abs(float(dm._loss(z1, y1, 2 * w)) - 2 * float((z1 - y1).abs().mean())) <= 1e-6


# ---------------------------------------------------------------------------------------------------------------------------
# the C entry points
# ---------------------------------------------------------------------------------------------------------------------------
def test_argument_validation_without_a_gpu():
    """dt_loss refuses a bad kind, classes of 0 or 4097, rows of 0, a categorical kind with one class, null pointers, a
    misaligned workspace, a weight with the binary focal loss and a negative gamma — all before any launch"""
    from deeptables_amd import _lib
    h = _lib.lib()
    buf = torch.zeros(64)
    p = _lib.ptr(buf)
    ok = dict(kind=_lib.DT_LOSS_MSE, z=p, t=p, w=None, rows=4, classes=3, gamma=2.0, alpha=0.25, loss=p, dz=p, ws=p)

    def call(**kw):
        a = {**ok, **kw}
        return h.dt_loss(a['kind'], a['z'], a['t'], a['w'], a['rows'], a['classes'], a['gamma'], a['alpha'], a['loss'], a['dz'],
                         a['ws'], None)
    for kind in (-1, 6, 99):
        assert call(kind=kind) == -1 and b'kind' in h.dt_last_error()
    for classes in (0, -3, _lib.DT_LOSS_MAX_CLASSES + 1):
        assert call(classes=classes) == -1 and b'classes' in h.dt_last_error()
        assert h.dt_loss_workspace_bytes(4, classes) == -1
    for rows in (0, -1, 1 << 31):
        assert call(rows=rows) == -1 and b'rows' in h.dt_last_error()
        assert h.dt_loss_workspace_bytes(rows, 3) == -1
    for kind in (_lib.DT_LOSS_CCE, _lib.DT_LOSS_CATEGORICAL_FOCAL):
        assert call(kind=kind, classes=1) == -1 and b'classes >= 2' in h.dt_last_error()
    for name in ('z', 't', 'loss', 'ws'):
        assert call(**{name: None}) == -1 and b'null' in h.dt_last_error(), name
    assert call(ws=_lib.ptr(buf[1:])) == -1 and b'workspace' in h.dt_last_error()
    assert call(kind=_lib.DT_LOSS_BINARY_FOCAL, w=p) == -1 and b'per-row weight' in h.dt_last_error()
    assert call(kind=_lib.DT_LOSS_CATEGORICAL_FOCAL, gamma=-1.0) == -1 and b'gamma' in h.dt_last_error()
    assert call(kind=_lib.DT_LOSS_BINARY_FOCAL, alpha=float('nan')) == -1
    assert h.dt_loss_workspace_bytes(1, 1) == 8 and h.dt_loss_workspace_bytes(64, 3) == 8
    assert h.dt_loss_workspace_bytes(65, 3) == 8 * 17                     # 4 rows per block
    assert h.dt_loss_workspace_bytes(4097, 1) == 8 * 1025                 # rows / 4 outweighs elements / 2048
    assert h.dt_loss_workspace_bytes(5, 4096) == 8 * 10                   # 20480 elements / 2048


def test_ctypes_signatures_follow_the_header():
    from deeptables_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'dt_hip.h')).read()
    ctype = {'int': _lib._c_int, 'int64_t': _lib._c_i64, 'float': _lib._c_f32}
    for name in ('dt_loss_workspace_bytes', 'dt_loss'):
        m = re.search(r'^(\w+) ' + name + r'\(([^;]*)\);', header, re.M | re.S)
        assert m, name
        res, args = _lib.SIGNATURES[name]
        assert res is ctype[m.group(1)]
        want = []
        for arg in m.group(2).split(','):
            arg = arg.strip()
            want.append(_lib._ptr if '*' in arg else ctype[arg.split()[-2]])
        assert args == want, (name, args, want)
    for k in ('BCE', 'CCE', 'MSE', 'MAE', 'BINARY_FOCAL', 'CATEGORICAL_FOCAL', 'MAX_CLASSES'):
        m = re.search(r'^#define DT_LOSS_' + k + r' (\d+)$', header, re.M)
        assert m and int(m.group(1)) == getattr(_lib, 'DT_LOSS_' + k), k
