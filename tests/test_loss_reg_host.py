# -*- coding:utf-8 -*-
"""CPU: the restatement of Keras' regression losses and of GHM-C with a mask (tests/loss_reg_reference.py) against closed
forms, the resolution of loss names and of the serialised form, DeepModel._loss on the CPU for the new names and for a
GHMCLoss, the errors, and the argument validation of dt_loss_reg / dt_ghmc (before any launch, so it runs without a GPU)."""
import math
import os
import re

import pytest
import torch

from tests import loss_reg_reference as LRR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


def _one(kind, p, t, delta=1.0):
    return float(LRR.per_element(kind, torch.tensor([[p]], dtype=F64), torch.tensor([[t]], dtype=F64), delta))


def _grad(kind, p, t, delta=1.0):
    _, dz = LRR.value_and_grad(kind, torch.tensor([[p]]), torch.tensor([[t]]), None, delta)
    return float(dz)


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------
def test_restatement_closed_forms_on_hand_values():
    # Huber, delta = 2: quadratic at |e| = 1.5 and exactly at |e| = delta, linear at |e| = 3
    assert _one('huber', 1.5, 0.0, 2.0) == 0.5 * 1.5 ** 2 and _grad('huber', 1.5, 0.0, 2.0) == 1.5
    assert _one('huber', 2.0, 0.0, 2.0) == 2.0 and _grad('huber', -2.0, 0.0, 2.0) == -2.0
    assert _one('huber', -3.0, 0.0, 2.0) == 2.0 * 3.0 - 2.0 and _grad('huber', -3.0, 0.0, 2.0) == -2.0
    assert _one('huber', 0.25, 0.25) == 0.0 and _grad('huber', 0.25, 0.25) == 0.0
    # log-cosh: e^2 / 2 - e^4 / 12 for small e; |e| - ln 2 for large e; tanh e
    e = 1e-4
    assert abs(_one('log_cosh', e, 0.0) - (e * e / 2 - e ** 4 / 12)) <= 1e-15 * e * e
    assert abs(_one('log_cosh', 50.0, 0.0) - (50.0 - math.log(2.0))) <= 1e-13
    assert abs(_one('log_cosh', 0.75, 0.25) - math.log(math.cosh(0.5))) <= 1e-15
    assert abs(_grad('log_cosh', 0.75, 0.25) - math.tanh(0.5)) <= 1e-7
    # the float32 restatement is Keras' own form and agrees with the float64 one to float32's resolution at e = O(1)
    k32 = float(LRR.per_element('log_cosh', torch.tensor([[0.75]]), torch.tensor([[0.25]])))
    assert abs(k32 - math.log(math.cosh(0.5))) <= 2e-7
    # MSLE: the clamp at eps, gradient 0 below it
    assert abs(_one('msle', 3.0, 1.0) - (math.log(4.0) - math.log(2.0)) ** 2) <= 1e-15
    assert abs(_one('msle', -5.0, 1.0) - (math.log1p(1e-7) - math.log(2.0)) ** 2) <= 1e-15
    assert _grad('msle', -5.0, 1.0) == 0.0
    assert abs(_grad('msle', 3.0, 1.0) - 2 * (math.log(4.0) - math.log(2.0)) / 4.0) <= 1e-6
    # MAPE: 100 |e| / |t|, sign(0) = 0, |t| below eps is clamped
    assert abs(_one('mape', 1.5, 2.0) - 25.0) <= 1e-13 and _one('mape', 2.0, 2.0) == 0.0
    assert _grad('mape', 2.0, 2.0) == 0.0 and abs(_grad('mape', 1.5, 2.0) + 50.0) <= 1e-5
    assert abs(_one('mape', 1e-3, 0.0) - 100 * 1e-3 / 1e-7) <= 1e-6
    # Poisson: p - t log(p + eps); NaN for p + eps < 0
    assert abs(_one('poisson', 2.0, 3.0) - (2.0 - 3.0 * math.log(2.0 + 1e-7))) <= 1e-15
    assert abs(_grad('poisson', 2.0, 3.0) - (1.0 - 3.0 / 2.0)) <= 1e-6
    assert math.isnan(_one('poisson', -1.0, 3.0))


def test_restatement_totals_weights_and_margins():
    g = torch.Generator().manual_seed(1)
    p, t = torch.rand(7, 3, generator=g, dtype=F64) + 0.1, torch.rand(7, 3, generator=g, dtype=F64) + 0.1
    w = torch.linspace(0.0, 3.0, 7, dtype=F64)
    for kind in LRR.KINDS:
        per = LRR.per_element(kind, p, t).mean(-1)
        assert abs(float(LRR.total(kind, p, t)) - float(per.mean())) <= 1e-15
        assert abs(float(LRR.total(kind, p, t, w)) - float((per * w).sum() / 7)) <= 1e-15
        _, dz = LRR.value_and_grad(kind, p, t)
        _, dzw = LRR.value_and_grad(kind, p, t, w)
        assert torch.allclose(dzw, dz * w[:, None], rtol=1e-13, atol=0)
    assert LRR.kink_margin('huber', p, t) == math.inf
    assert abs(LRR.kink_margin('mape', torch.tensor([[1.0, 2.0]]), torch.tensor([[1.5, 2.25]])) - 0.25) <= 1e-15
    assert abs(LRR.kink_margin('msle', torch.tensor([[0.5, -0.25]]), p[:1, :2]) - (0.25 + 1e-7)) <= 1e-12
    assert abs(LRR.kink_margin('poisson', torch.tensor([[0.5, -0.25]]), p[:1, :2]) - (0.25 - 1e-7)) <= 1e-12
    # GHM-C: g = |sigmoid(0) - 0.25| = 0.25 against the edges of 10 bins: 0.05 from 0.2 and from 0.3
    m = LRR.kink_margin('ghmc', torch.zeros(1, 1), torch.full((1, 1), 0.25), bins=10)
    assert abs(m - 0.05) <= 1e-7


def test_ghmc_restatement_with_a_mask_and_without():
    """without a mask it is the oracle's; with one, the masked-out elements drop out of the counts and of tot"""
    from oracle import reference_layers as R
    g = torch.Generator().manual_seed(2)
    z = torch.randn(40, 3, generator=g, dtype=F64) * 2
    t = (torch.rand(40, 3, generator=g) < 0.4).double()
    acc = torch.rand(10, generator=g, dtype=F64) * 5
    for mmt in (0.75, 0.0):
        l0, a0 = R.ghmc_loss(z, t, acc, bins=10, momentum=mmt)
        l1, a1 = LRR.ghmc(z, t, acc, bins=10, momentum=mmt)
        assert float(l0) == float(l1) and torch.equal(a0, a1)
        l2, a2 = LRR.ghmc(z, t, acc, bins=10, momentum=mmt, mask=torch.ones(40, 3))
        assert float(l2) == float(l1) and torch.equal(a2, a1)
    mask = (torch.rand(40, 3, generator=g) < 0.6).double()
    keep = mask.reshape(-1) > 0
    lm, am = LRR.ghmc(z, t, torch.zeros(10, dtype=F64), bins=10, momentum=0.5, mask=mask)
    lk, ak = LRR.ghmc(z.reshape(-1)[keep].reshape(-1, 1), t.reshape(-1)[keep].reshape(-1, 1), torch.zeros(10, dtype=F64),
                      bins=10, momentum=0.5)
    assert abs(float(lm) - float(lk)) <= 1e-14 and torch.equal(am, ak)
    counts = LRR.ghmc_counts(z, t, 10, mask)
    assert int(counts.sum()) == int(keep.sum()) and torch.equal(am, 0.5 * counts.double())


# ---------------------------------------------------------------------------------------------------------------------------
# names, the serialised form, DeepModel
# ---------------------------------------------------------------------------------------------------------------------------
NAMES = {'huber': 'huber', 'log_cosh': 'log_cosh', 'logcosh': 'log_cosh', 'msle': 'msle',
         'mean_squared_logarithmic_error': 'msle', 'mape': 'mape', 'mean_absolute_percentage_error': 'mape',
         'poisson': 'poisson'}


def _build(task, num_classes, loss):
    from deeptables_amd.models import ModelConfig, DeepModel
    from deeptables_amd.models.metainfo import CategoricalColumn, ContinuousColumn
    conf = ModelConfig(nets=['dnn_nets'], loss=loss, embedding_dropout=0,
                       dnn_params={'hidden_units': ((8, 0, False), (4, 0, False)), 'activation': 'relu'})
    dm = DeepModel(task, num_classes, conf, [CategoricalColumn('C0', 5, 4)], [ContinuousColumn('input_continuous_all', ['a'])])
    dm.build('cpu')
    return dm


def test_names_resolve_and_cpu_model_loss_is_the_restatement():
    from deeptables_amd import _lib, losses
    assert {n: losses.LOSS_KINDS[n] for n in NAMES} == {n: LRR.kind_code(k) for n, k in NAMES.items()}
    assert set(NAMES) <= set(losses.LOSS_NAMES)
    for bad in ('hinge', 'MAE ', 'Huber', 'huber '):
        assert bad not in losses.LOSS_NAMES
    g = torch.Generator().manual_seed(4)
    z = torch.rand(9, 1, generator=g) * 3 + 0.2
    y = torch.rand(9, 1, generator=g) * 3 + 0.2
    w = torch.rand(9, generator=g) * 2
    for name, kind in NAMES.items():
        dm = _build('regression', 1, name)
        assert dm.loss_name == name and dm.model_desc.loss == name
        for ww in (None, w):
            got = float(dm._loss(z, y, ww))
            want = float(LRR.total(kind, z, y, ww))
            assert abs(got - want) <= 2e-6 * max(1.0, abs(want)), (name, got, want)
            ref = float(LRR.total(kind, z.double(), y.double(), None if ww is None else ww.double()))
            assert abs(float(dm._loss(z.double(), y.double(), ww)) - ref) <= 1e-9 * max(1.0, abs(ref)), name
    # a task with an activation: the loss sees the activated output
    dm = _build('binary', 2, 'huber')
    assert abs(float(dm._loss(z, (y > 1.5).float())) - float(LRR.total('huber', torch.sigmoid(z), (y > 1.5).float()))) <= 1e-6
    assert _lib.DT_LOSS_HUBER > _lib.DT_LOSS_CATEGORICAL_FOCAL


def test_serialised_form():
    from deeptables_amd import losses
    r = losses.resolve_loss
    assert r({'class_name': 'Huber', 'config': {'delta': 2.0}}) == ('huber', {'delta': 2.0})
    assert r({'class_name': 'Huber'}) == ('huber', {})
    assert r({'class_name': 'LogCosh', 'config': {'name': 'lc', 'reduction': 'sum_over_batch_size'}}) == ('log_cosh', {})
    assert r({'class_name': 'MeanSquaredLogarithmicError', 'config': {}})[0] == 'mean_squared_logarithmic_error'
    assert r({'class_name': 'MeanAbsolutePercentageError', 'config': None})[0] == 'mean_absolute_percentage_error'
    assert r({'class_name': 'Poisson', 'config': {'reduction': 'auto'}})[0] == 'poisson'
    assert r({'class_name': 'BinaryCrossentropy', 'config': {'from_logits': False, 'label_smoothing': 0.0}})[0] == \
        'binary_crossentropy'
    assert r({'class_name': 'CategoricalCrossentropy'})[0] == 'categorical_crossentropy'
    assert r({'class_name': 'MeanSquaredError'})[0] == 'mean_squared_error'
    assert r({'class_name': 'MeanAbsoluteError'})[0] == 'mean_absolute_error'
    for bad in ({'class_name': 'Hinge'}, {'class_name': 'huber'}, {'config': {}},
                {'class_name': 'Huber', 'config': {'delta': 0.0}}, {'class_name': 'Huber', 'config': {'delta': -1.0}},
                {'class_name': 'Huber', 'config': {'delta': float('nan')}}, {'class_name': 'Huber', 'config': {'delta': float('inf')}},
                {'class_name': 'Huber', 'config': {'axis': -1}}, {'class_name': 'LogCosh', 'config': {'delta': 1.0}},
                {'class_name': 'Poisson', 'config': {'reduction': 'sum'}}, {'class_name': 'Poisson', 'config': {'reduction': 'none'}},
                {'class_name': 'BinaryCrossentropy', 'config': {'from_logits': True}},
                {'class_name': 'CategoricalCrossentropy', 'config': {'label_smoothing': 0.1}}):
        with pytest.raises(ValueError):
            r(bad)
    # through the model: compiled at build, delta carried into the loss
    z, y = torch.tensor([[3.0], [0.5]]), torch.tensor([[0.0], [0.0]])
    dm = _build('regression', 1, {'class_name': 'Huber', 'config': {'delta': 2.0}})
    assert dm.loss_name == 'huber' and dm.loss_delta == 2.0
    assert abs(float(dm._loss(z, y)) - (2.0 * 3.0 - 2.0 + 0.125) / 2) <= 1e-6
    assert abs(float(dm._loss(z, y, torch.tensor([2.0, 0.0]))) - (2.0 * 3.0 - 2.0)) <= 1e-6
    assert _build('regression', 1, 'huber').loss_delta == 1.0
    with pytest.raises(ValueError, match='unknown config keys'):
        _build('regression', 1, {'class_name': 'Huber', 'config': {'delta': 2.0, 'axis': -1}})
    with pytest.raises(ValueError, match='delta'):
        _build('regression', 1, {'class_name': 'Huber', 'config': {'delta': 0}})
    dm = _build('regression', 1, 'hinge')                       # an unknown string still fails at the first step
    with pytest.raises(ValueError, match='Unsupported loss'):
        dm._loss(z, y)


def test_ghmc_through_a_cpu_model():
    from deeptables_amd.models.layers import GHMCLoss
    g = torch.Generator().manual_seed(5)
    z = torch.randn(12, 1, generator=g)
    y = (torch.rand(12, 1, generator=g) < 0.5).float()
    dm = _build('binary', 2, GHMCLoss(bins=10, momentum=0.75))
    assert dm.loss_name == 'GHMCLoss' and dm.model_desc.loss == 'GHMCLoss'
    twin = GHMCLoss(bins=10, momentum=0.75)
    for _ in range(2):                                          # the state carries from call to call
        got, want = dm._loss(z, y), twin.calc(z, y)
        assert float(got) == float(want)
    assert torch.equal(dm._custom_loss.acc_sum, twin.acc_sum) and float(twin.acc_sum.sum()) > 0
    zg = z.clone().requires_grad_(True)
    dm._loss(zg, y.reshape(-1)).backward()                     # (a flat target is reshaped to the logits)
    assert zg.grad is not None and float(zg.grad.abs().sum()) > 0
    with pytest.raises(ValueError, match='GHMCLoss'):
        dm._loss(z, y, torch.ones(12))
    zm = torch.randn(12, 3, generator=g)
    ym = (torch.rand(12, 3, generator=g) < 0.5).float()
    dmm = _build('multilabel', 3, GHMCLoss(bins=7, momentum=0))
    assert float(dmm._loss(zm, ym)) == float(GHMCLoss(bins=7, momentum=0).calc(zm, ym))
    for task, nc in (('multiclass', 3), ('regression', 1)):
        with pytest.raises(ValueError, match='GHMCLoss'):
            _build(task, nc, GHMCLoss())


# ---------------------------------------------------------------------------------------------------------------------------
# the C entry points
# ---------------------------------------------------------------------------------------------------------------------------
def test_argument_validation_without_a_gpu():
    from deeptables_amd import _lib
    h = _lib.lib()
    buf = torch.zeros(64)
    p = _lib.ptr(buf)
    ok = dict(kind=_lib.DT_LOSS_HUBER, p=p, t=p, w=None, rows=4, classes=3, delta=1.0, loss=p, dz=p, ws=p)

    def call(**kw):
        a = {**ok, **kw}
        return h.dt_loss_reg(a['kind'], a['p'], a['t'], a['w'], a['rows'], a['classes'], a['delta'], a['loss'], a['dz'], a['ws'],
                             None)
    for kind in (-1, 0, 5, 11):                                  # dt_loss' own kinds are not dt_loss_reg's
        assert call(kind=kind) == -1 and b'kind' in h.dt_last_error()
    for classes in (0, _lib.DT_LOSS_MAX_CLASSES + 1):
        assert call(classes=classes) == -1 and b'classes' in h.dt_last_error()
        assert h.dt_loss_reg_workspace_bytes(4, classes) == -1
    for rows in (0, -1, 1 << 31):
        assert call(rows=rows) == -1 and b'rows' in h.dt_last_error()
        assert h.dt_loss_reg_workspace_bytes(rows, 3) == -1
    for name in ('p', 't', 'loss', 'ws'):
        assert call(**{name: None}) == -1 and b'null' in h.dt_last_error(), name
    assert call(ws=_lib.ptr(buf[1:])) == -1 and b'workspace' in h.dt_last_error()
    for delta in (0.0, -1.0, float('nan'), float('inf')):
        assert call(delta=delta) == -1 and b'delta' in h.dt_last_error()
    assert h.dt_loss_reg_workspace_bytes(2048, 1) == 8 and h.dt_loss_reg_workspace_bytes(2049, 1) == 16
    assert h.dt_loss(_lib.DT_LOSS_HUBER, p, p, None, 4, 3, 2.0, 0.25, p, p, p, None) == -1      # and the other way round

    okg = dict(z=p, t=p, mask=None, n=12, bins=10, m=0.75, m1=0.25, acc=p, loss=p, dz=p, ws=p)

    def ghmc(**kw):
        a = {**okg, **kw}
        return h.dt_ghmc(a['z'], a['t'], a['mask'], a['n'], a['bins'], a['m'], a['m1'], a['acc'], a['loss'], a['dz'], a['ws'], None)
    for bins in (0, -1, _lib.DT_GHMC_MAX_BINS + 1):
        assert ghmc(bins=bins) == -1 and b'bins' in h.dt_last_error()
        assert h.dt_ghmc_workspace_bytes(12, bins) == -1
    for n in (0, -5, 1 << 40):
        assert ghmc(n=n) == -1 and h.dt_ghmc_workspace_bytes(n, 10) == -1
    for name in ('z', 't', 'loss', 'ws'):
        assert ghmc(**{name: None}) == -1 and b'null' in h.dt_last_error(), name
    for m in (-0.1, 1.0, float('nan')):
        assert ghmc(m=m) == -1 and b'momentum' in h.dt_last_error()
    assert ghmc(acc=None) == -1 and b'acc_sum' in h.dt_last_error()
    assert ghmc(m1=0.0) == -1
    assert ghmc(ws=_lib.ptr(buf[1:])) == -1 and b'workspace' in h.dt_last_error()
    one, two = h.dt_ghmc_workspace_bytes(2048, 10), h.dt_ghmc_workspace_bytes(2049, 10)
    # per block a double and 11 counts, the counts' region padded to 8 bytes: (16 + 88) - (8 + 48)
    assert one % 8 == 0 and two % 8 == 0 and two - one == 48


def test_header_bindings_and_documents_name_the_new_symbols():
    from deeptables_amd import _lib
    from tests import test_host_api as T
    T.test_library_loads_and_exports_every_declared_symbol()
    T.test_ctypes_signatures_follow_the_header_prototypes()
    T.test_header_constants_equal_the_binding_s()
    header = open(os.path.join(ROOT, 'include', 'dt_hip.h')).read()
    guide = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in ('dt_loss_reg_workspace_bytes', 'dt_loss_reg', 'dt_ghmc_workspace_bytes', 'dt_ghmc'):
        assert name in _lib.SIGNATURES and re.search(r'\b' + name + r'\(', header) and name in guide, name
    for k, v in (('HUBER', 6), ('LOG_COSH', 7), ('MSLE', 8), ('MAPE', 9), ('POISSON', 10)):
        m = re.search(r'^#define DT_LOSS_' + k + r' (\d+)$', header, re.M)
        assert m and int(m.group(1)) == getattr(_lib, 'DT_LOSS_' + k) == v, k
    m = re.search(r'^#define DT_GHMC_MAX_BINS (\d+)$', header, re.M)
    assert m and int(m.group(1)) == _lib.DT_GHMC_MAX_BINS
