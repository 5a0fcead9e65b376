# -*- coding:utf-8 -*-
"""CPU: the host side of the Keras L1 / L2 regularizers — `deeptables_amd.regularizers` (get / serialize / defaults), the way
`ModelConfig`, `dnn_params` and `afm_params` values reach the layers, what the layers serialise, which models keep a fused
train plan, the refusal of a weight penalty on a row-sparse table, the C-ABI of csrc/regularizer.hip, and that the model keeps
no activation of a step alive.  Models are built on the CPU; nothing is launched."""
import ctypes
import os
import re
import weakref

import numpy as np
import pytest
import torch

from tests import regularizer_reference as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REG_ENTRIES = ('dt_reg_chunk', 'dt_reg_penalty_workspace_bytes', 'dt_reg_penalty', 'dt_reg_grad')


# ---- regularizers.get / serialize -----------------------------------------------------------------------------------------
class _KerasLike:
    """what a real keras.regularizers.L1L2 looks like from outside: a callable with numeric l1 / l2 attributes"""

    def __init__(self, l1, l2):
        self.l1, self.l2 = np.float32(l1), l2

    def __call__(self, x):
        raise AssertionError('never called: the penalty runs in the HIP kernels')


class OrthogonalRegularizer:
    def __init__(self):
        self.factor, self.mode = 0.01, 'rows'

    def __call__(self, x):
        return 0.0


def test_get_accepts_every_keras_form_with_keras_defaults():
    from deeptables_amd import regularizers as R
    assert R.get(None) is None
    assert R.get('l1').coefficients() == (RR.KERAS_DEFAULT, 0.0)
    assert R.get('l2').coefficients() == (0.0, RR.KERAS_DEFAULT)
    assert R.get('l1_l2').coefficients() == (RR.KERAS_DEFAULT, RR.KERAS_DEFAULT)
    assert R.L1().coefficients() == (0.01, 0.0) and R.L2().coefficients() == (0.0, 0.01)
    assert R.L1L2().coefficients() == (0.0, 0.0)
    assert R.get({'class_name': 'L1', 'config': {'l1': 0.5}}).coefficients() == (0.5, 0.0)
    assert R.get({'class_name': 'L2', 'config': {'l2': 0.25}}).coefficients() == (0.0, 0.25)
    assert R.get({'class_name': 'L1L2', 'config': {'l1': 0.5, 'l2': 0.125}}).coefficients() == (0.5, 0.125)
    assert R.get({'class_name': 'L2', 'config': {}}).coefficients() == (0.0, 0.01)
    inst = R.L1L2(l1=1e-3, l2=2e-3)
    assert R.get(inst) is inst
    for cls, args in ((R.L1, (0.3,)), (R.L2, (0.4,)), (R.L1L2, (0.1, 0.2))):
        assert isinstance(R.get(cls(*args)), cls)
    k = R.get(_KerasLike(0.5, 0.25))
    assert isinstance(k, R.L1L2) and k.coefficients() == (0.5, 0.25)

    class OnlyL2:
        l2 = 0.125
    assert R.get(OnlyL2()).coefficients() == (0.0, 0.125)


@pytest.mark.parametrize('bad', ['orthogonal_regularizer', 'L2', 'l3', '', lambda w: 0.0, OrthogonalRegularizer(), 0.01,
                                 {'class_name': 'OrthogonalRegularizer', 'config': {'factor': 0.01}},
                                 {'class_name': 'L2', 'config': {'l1': 0.1}}, {'config': {'l2': 0.1}},
                                 {'class_name': 'L2', 'config': {'l2': 'much'}}])
def test_get_refuses_everything_else_and_names_the_knob(bad):
    from deeptables_amd import regularizers as R
    with pytest.raises(ValueError, match='embeddings_regularizer'):
        R.get(bad, 'embeddings_regularizer')


def test_serialize_round_trip():
    from deeptables_amd import regularizers as R
    assert R.serialize(None) is None
    for reg in (R.L1(0.3), R.L2(), R.L1L2(1e-4, 2e-5), R.get('l1_l2'), R.get(_KerasLike(0.5, 0.25))):
        s = R.serialize(reg)
        assert set(s) == {'class_name', 'config'} and s['class_name'] == type(reg).__name__
        back = R.get(s)
        assert type(back) is type(reg) and back.coefficients() == reg.coefficients() and back == reg
    assert R.serialize('l2') == {'class_name': 'L2', 'config': {'l2': 0.01}}
    assert R.serialize(R.L1L2(0.5, 0.25)) == {'class_name': 'L1L2', 'config': {'l1': 0.5, 'l2': 0.25}}


def test_reference_penalty_and_gradient_restate_keras():
    x = np.array([[-2.0, 0.0, -0.0], [0.5, 3.0, -1.0]])
    assert RR.penalty(x, l1=0.5) == 0.5 * 6.5 and RR.penalty(x, l2=0.25) == 0.25 * 14.25
    assert RR.penalty(x, 0.5, 0.25) == 0.5 * 6.5 + 0.25 * 14.25 and RR.penalty(x) == 0.0
    assert RR.penalty(np.array([np.inf]), l1=0.0, l2=0.0) == 0.0           # a zero coefficient forms no term
    g = RR.grad(x, 0.5, 0.25, go=2.0)
    assert np.array_equal(g, 2.0 * (0.5 * np.sign(x) + 0.5 * x)) and g[0, 1] == 0.0 and g[0, 2] == 0.0
    g32 = RR.grad_f32(x.astype(np.float32), 0.5, 0.25, go=2.0)
    assert g32.dtype == np.float32 and np.array_equal(g32.astype(np.float64), g)       # exact at these values
    assert np.array_equal(RR.grad_f32(x, 0.5, 0.25, 2.0, into=np.ones_like(x)), (1.0 + g).astype(np.float32))
    w = np.array([1.0, -1.0, 0.0])
    assert np.allclose(RR.sgd_step(w, np.array([0.1, 0.1, 0.1]), l1=0.5, l2=0.25, lr=0.1),
                       w - 0.1 * (0.1 + np.array([1.0, -1.0, 0.0])))
    # Adam, step 1: m = 0.1 g, v = 0.001 g^2, alpha = lr sqrt(1 - b2) / (1 - b1) -> w - lr g / (|g| + eps sqrt(1 - b2)) ~ -lr sign(g)
    w1, m, v = RR.adam_step(w, np.zeros(3), np.zeros(3), np.zeros(3), 1, l2=0.5)
    assert np.allclose(w1, w - 1e-3 * np.sign(w), atol=1e-8) and np.allclose(m, 0.1 * w)


# ---- layers ---------------------------------------------------------------------------------------------------------------
def test_dense_stores_serialises_and_records_its_regularizers():
    from deeptables_amd import functional as Fn, regularizers as R
    d = Fn.Dense(4, kernel_regularizer='l1', activity_regularizer=R.L2(1e-3), name='reg_host_dense')
    d.build((None, 3))
    c = d.get_config()
    assert c['kernel_regularizer'] == {'class_name': 'L1', 'config': {'l1': 0.01}}
    assert c['activity_regularizer'] == {'class_name': 'L2', 'config': {'l2': 1e-3}}
    pens = d.weight_penalties()
    assert len(pens) == 1 and pens[0][0] is d.kernel and pens[0][1] == (0.01, 0.0)          # the kernel, not the bias
    plain = Fn.Dense(4, name='reg_host_dense_plain')
    plain.build((None, 3))
    assert plain.weight_penalties() == [] and plain.get_config()['kernel_regularizer'] is None
    assert plain.get_config()['activity_regularizer'] is None
    with pytest.raises(ValueError, match='kernel_regularizer'):
        Fn.Dense(4, kernel_regularizer='orthogonal_regularizer')
    with pytest.raises(ValueError, match='activity_regularizer'):
        Fn.Dense(4, activity_regularizer=lambda x: 0.0)
    # Layer.add_weight(regularizer=) records (parameter, regularizer) for any layer
    lay = Fn.Layer(name='reg_host_layer')
    p = lay.add_weight('w', (2, 2), 'ones', regularizer=R.L1L2(0.5, 0.25))
    q = lay.add_weight('v', (2,), 'ones')
    assert [(t is p, c) for t, c in lay.weight_penalties()] == [(True, (0.5, 0.25))] and q is not None
    with pytest.raises(ValueError, match='regularizer'):
        lay.add_weight('u', (2,), 'ones', regularizer='nope')


def test_an_activity_regularised_dense_keeps_its_own_output():
    """no folded relu (Model.__init__'s peephole) and no rank-one AutoInt head: the penalty needs the pre-activation output"""
    from deeptables_amd import functional as Fn
    for reg, folded in ((None, True), ('l2', False)):
        Fn.reset_uids()
        x = Fn.Input((3,))
        h = Fn.Dense(4, activity_regularizer=reg, name='d')(x)
        out = Fn.Dense(1, name='o')(Fn.Activation('relu', name='a')(h))
        m = Fn.Model(x, out)
        assert bool(m._fused_relu) is folded and bool(m._passthrough) is folded
    assert Fn.Dense(1).accepts_pending_norm and not Fn.Dense(1, activity_regularizer='l2').accepts_pending_norm
    assert Fn.Dense(1, activity_regularizer={'class_name': 'L2', 'config': {'l2': 0.0}}).accepts_pending_norm


def test_multi_column_embedding_stores_and_serialises_both(monkeypatch):
    from deeptables_amd.models import layers as L
    from deeptables_amd import regularizers as R
    e = L.MultiColumnEmbedding([7, 9, 11], [4, 4, 4], embeddings_regularizer='l2', activity_regularizer=R.L1(1e-3),
                               name='reg_host_emb')
    e.build((None, 3))
    c = e.get_config()
    assert c['embeddings_regularizer'] == {'class_name': 'L2', 'config': {'l2': 0.01}}
    assert c['activity_regularizer'] == {'class_name': 'L1', 'config': {'l1': 1e-3}}
    pens = e.weight_penalties()
    assert len(pens) == 1 and pens[0][0] is e.tables['d4'] and pens[0][1] == (0.0, 0.01) and pens[0][0].shape == (27, 4)
    two = L.MultiColumnEmbedding([7, 9, 11], [4, 8, 4], embeddings_regularizer='l1', name='reg_host_emb2')
    two.build((None, 3))
    assert [tuple(t.shape) for t, _ in two.weight_penalties()] == [(18, 4), (9, 8)]          # every packed table once
    plain = L.MultiColumnEmbedding([7, 9], [4, 4], name='reg_host_emb3')
    plain.build((None, 2))
    assert plain.weight_penalties() == [] and plain.get_config()['embeddings_regularizer'] is None
    with pytest.raises(ValueError, match='embeddings_regularizer'):
        L.MultiColumnEmbedding([7], [4], embeddings_regularizer='orthogonal_regularizer')
    v = L.VarLenColumnEmbedding(13, 4, embeddings_regularizer='l2', activity_regularizer='l1', name='reg_host_var')
    v.build((None, 5))
    assert [(t is v.embeddings, c) for t, c in v.weight_penalties()] == [(True, (0.0, 0.01))]
    assert v.get_config()['activity_regularizer'] == {'class_name': 'L1', 'config': {'l1': 0.01}}


# ---- config -> layers -----------------------------------------------------------------------------------------------------
def _model(nets=('dnn_nets',), var_len=False, dnn=None, **extra):
    from deeptables_amd import functional
    from deeptables_amd.models import ModelConfig, DeepModel
    from deeptables_amd.models.metainfo import CategoricalColumn, ContinuousColumn, VarLenCategoricalColumn
    functional.set_seed(11)
    conf = ModelConfig(nets=list(nets), fixed_embedding_dim=True, embeddings_output_dim=4, embedding_dropout=0,
                       dnn_params={'hidden_units': ((8, 0, False), (4, 0, False)), 'activation': 'relu', **(dnn or {})}, **extra)
    cats = [CategoricalColumn(f'C{i}', v, 4) for i, v in enumerate((7, 9, 11))]
    conts = [ContinuousColumn('input_continuous_all', ['a'])]
    vl = None
    if var_len:
        vl = [VarLenCategoricalColumn('V0', 13, 4)]
        vl[0].max_elements_length = 5
    dm = DeepModel('binary', 2, conf, cats, conts, var_categorical_len_columns=vl)
    dm.build('cpu')
    return dm


def test_config_values_reach_the_layers():
    from deeptables_amd import regularizers as R
    dm = _model(nets=['dnn_nets'], var_len=True, embeddings_regularizer='l2', embeddings_activity_regularizer=R.L2(1e-3),
                dnn={'kernel_regularizer': 'l1', 'activity_regularizer': {'class_name': 'L2', 'config': {'l2': 0.5}}})
    L = dm.model.layers_by_name
    emb = L['emb_categorical_vars_all']
    assert emb.embeddings_regularizer.coefficients() == (0.0, 0.01) and emb.activity_regularizer.coefficients() == (0.0, 1e-3)
    var = L['emb_V0']
    assert var.embeddings_regularizer.coefficients() == (0.0, 0.01) and var.activity_regularizer.coefficients() == (0.0, 1e-3)
    for name in ('dnn_dense_1', 'dnn_dense_2'):
        assert L[name].kernel_regularizer.coefficients() == (0.01, 0.0) and L[name].activity_regularizer.coefficients() == (0.0, 0.5)
    assert L['task_output'].kernel_regularizer is None and L['task_output'].activity_regularizer is None
    got = {id(t): c for t, c in dm.model.weight_penalties()}
    want = {id(emb.tables['d4']): (0.0, 0.01), id(var.embeddings): (0.0, 0.01), id(L['dnn_dense_1'].kernel): (0.01, 0.0),
            id(L['dnn_dense_2'].kernel): (0.01, 0.0)}
    assert got == want
    assert {l.name for l in dm.model.activity_layers()} == {'emb_categorical_vars_all', 'emb_V0', 'dnn_dense_1', 'dnn_dense_2'}
    assert dm.model.has_regularizers()
    # the tower's relu is no longer folded into the activity-regularised Dense layers
    assert not dm.model._fused_relu
    # afm_params['kernel_regularizer'] reaches AFM.dense_attention (a layer nested in the AFM layer), and only it
    afm = _model(nets=['afm_nets'], afm_params={'hidden_factor': 4, 'dropout_rate': 0, 'kernel_regularizer': R.L1L2(0.25, 0.125)})
    lay = afm.model.layers_by_name['afm_layer']
    assert lay.dense_attention.kernel_regularizer.coefficients() == (0.25, 0.125) and lay.dense_out.kernel_regularizer is None
    assert [(t is lay.dense_attention.kernel, c) for t, c in afm.model.weight_penalties()] == [(True, (0.25, 0.125))]
    assert afm.model.activity_layers() == []


def test_custom_dnn_passes_both_params_on():
    from deeptables_amd.models import deepnets
    dm = _model(dnn={'custom_dnn_fn': deepnets.custom_dnn_D_A_D_B, 'kernel_regularizer': 'l2', 'activity_regularizer': 'l1'})
    d1 = dm.model.layers_by_name['dnn_custom_dense_1']
    assert d1.kernel_regularizer.coefficients() == (0.0, 0.01) and d1.activity_regularizer.coefficients() == (0.01, 0.0)
    assert d1.activation_name == 'relu'         # its output, the penalised tensor, is post-activation


def test_unsupported_regularizers_raise_at_build_naming_the_knob():
    with pytest.raises(ValueError, match='embeddings_regularizer'):
        _model(embeddings_regularizer='orthogonal_regularizer')
    with pytest.raises(ValueError, match='embeddings_activity_regularizer'):
        _model(embeddings_activity_regularizer=lambda x: 0.0)
    with pytest.raises(ValueError, match='kernel_regularizer'):
        _model(dnn={'kernel_regularizer': OrthogonalRegularizer()})
    with pytest.raises(ValueError, match='afm_params'):
        _model(nets=['afm_nets'], afm_params={'kernel_regularizer': 'l3'})


def test_a_model_without_regularizers_has_no_regularization_loss():
    dm = _model()
    assert dm.model.weight_penalties() == [] and dm.model.activity_layers() == [] and not dm.model.has_regularizers()
    assert dm.model.regularization_loss() is None
    assert dm.model._fused_relu            # and its execution plan is the one it always had: relu folded into the tower


def test_zero_coefficients_are_no_regularizer():
    from deeptables_amd import regularizers as R
    dm = _model(embeddings_regularizer=R.L2(0.0), dnn={'activity_regularizer': R.L1L2(0.0, 0.0)})
    assert not dm.model.has_regularizers() and dm.model.regularization_loss() is None and dm.model._fused_relu


def test_weight_penalty_on_a_row_sparse_table_is_refused(monkeypatch):
    from deeptables_amd.models import layers as L
    monkeypatch.setattr(L, 'DENSE_GRAD_MAX_ELEMS', 100)            # the packed table has (7 + 9 + 11) * 4 = 108 elements
    with pytest.raises(ValueError) as e:
        _model(embeddings_regularizer='l2')
    msg = str(e.value)
    assert '108' in msg and '100' in msg and 'embeddings_activity_regularizer' in msg and 'row-sparse' in msg
    dm = _model(embeddings_activity_regularizer='l2')               # the penalty that stays row-sparse builds
    assert not dm.model.layers_by_name['emb_categorical_vars_all'].uses_dense_grad(4) and dm.model.has_regularizers()
    monkeypatch.setattr(L, 'DENSE_GRAD_MAX_ELEMS', 108)            # at the limit: Keras' exact result, dense gradient
    assert _model(embeddings_regularizer='l2').model.has_regularizers()


def test_a_regularised_model_has_no_fused_train_plan(monkeypatch):
    from deeptables_amd import fused
    from deeptables_amd.models import deepnets
    monkeypatch.delenv('DT_AMD_FUSED', raising=False)
    built = []
    monkeypatch.setattr(fused.FusedDeepFM, '__init__', lambda self, dm: built.append(dm))
    kw = dict(nets=deepnets.DeepFM, dnn={'hidden_units': ((128, 0, False), (64, 0, False))})
    plain = _model(**kw)
    assert fused.FusedDeepFM.eligible(plain)
    assert isinstance(fused.make_fused_plan(plain), fused.FusedDeepFM) and built == [plain]         # unchanged without one
    for extra in (dict(embeddings_regularizer='l2'), dict(embeddings_activity_regularizer='l1'),
                  dict(dnn={**kw['dnn'], 'kernel_regularizer': 'l2'}), dict(dnn={**kw['dnn'], 'activity_regularizer': 'l2'})):
        dm = _model(**{**kw, **extra})
        assert fused.FusedDeepFM.eligible(dm), 'the graph itself is still the DeepFM graph'
        assert fused.make_fused_plan(dm) is None and dm.fused_plan() is None, extra
    assert built == [plain]
    # 'auto' steps_per_execution then resolves to eager through the existing rule
    from deeptables_amd import compiled

    class Feed:
        weighted = False
        n = 64 * 20
    assert compiled.resolve_steps_per_execution(dm, 'auto', Feed(), 64, 20) == 1


# ---- C-ABI ----------------------------------------------------------------------------------------------------------------
def _header():
    text = open(os.path.join(ROOT, 'include', 'dt_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return re.sub(r'//[^\n]*', '', text)


def test_entry_points_header_binding_and_library_agree():
    from deeptables_amd import _lib
    protos = dict(re.findall(r'\b(dt_reg_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;', _header()))
    assert sorted(protos) == sorted(REG_ENTRIES) == sorted(n for n in _lib.SIGNATURES if n.startswith('dt_reg_'))
    handle = ctypes.CDLL(_lib.LIB_PATH)

    def kind(decl):
        if '*' in decl:
            return 'ptr'
        words = decl.replace('const', ' ').split()
        return {'int': 'int', 'int64_t': 'i64', 'float': 'f32', 'double': 'f64'}[' '.join(words[:-1]) if len(words) > 1 else words[0]]

    of_ctype = {ctypes.c_void_p: 'ptr', ctypes.c_int: 'int', ctypes.c_int64: 'i64', ctypes.c_float: 'f32'}
    for name, params in protos.items():
        assert hasattr(handle, name), f'{name} declared in include/dt_hip.h but not exported'
        decls = [p.strip() for p in params.split(',') if p.strip() and p.strip() != 'void']
        assert [kind(d) for d in decls] == [of_ctype[a] for a in _lib.SIGNATURES[name][1]], name
    ret = dict((n, r) for r, n in re.findall(r'\b(int|int64_t)\s+(dt_reg_[a-z0-9_]+)\s*\(', _header()))
    assert {n: {'int': ctypes.c_int, 'int64_t': ctypes.c_int64}[r] for n, r in ret.items()} == \
        {n: _lib.SIGNATURES[n][0] for n in REG_ENTRIES}


def test_argument_errors_need_no_gpu():
    """validation comes before the first launch: exercisable without a device"""
    from deeptables_amd import _lib
    h = _lib.lib()
    chunk = h.dt_reg_chunk()
    assert chunk > 0 and chunk % 4 == 0
    n = (ctypes.c_int64 * 3)(1, chunk, 2 * chunk + 5)
    assert h.dt_reg_penalty_workspace_bytes(3, n) == 8 * (1 + 1 + 3)
    assert h.dt_reg_penalty_workspace_bytes(0, None) >= 8
    assert h.dt_reg_penalty_workspace_bytes(-1, n) == -1 and h.dt_reg_penalty_workspace_bytes(1, (ctypes.c_int64 * 1)(-4)) == -1
    one = (ctypes.c_int64 * 1)(5)
    null = (ctypes.c_void_p * 1)(None)
    fake = (ctypes.c_void_p * 1)(4096)
    d1, f1 = (ctypes.c_double * 1)(0.5), (ctypes.c_float * 1)(0.5)
    out = ctypes.c_void_p(4096)
    assert h.dt_reg_penalty(1, null, one, d1, d1, out, out, out, None) == -1          # null pointer with n > 0
    assert b'dt_reg_penalty' in h.dt_last_error()
    assert h.dt_reg_penalty(1, fake, (ctypes.c_int64 * 1)(-1), d1, d1, out, out, out, None) == -1      # negative n
    assert h.dt_reg_penalty(-1, fake, one, d1, d1, out, out, out, None) == -1         # negative count
    assert h.dt_reg_penalty(1, fake, one, d1, d1, None, out, out, None) == -1         # no workspace
    assert h.dt_reg_penalty(1, fake, one, d1, d1, out, None, out, None) == -1         # no output
    assert h.dt_reg_grad(1, null, fake, one, f1, f1, out, 0, None) == -1
    assert b'dt_reg_grad' in h.dt_last_error()
    assert h.dt_reg_grad(1, fake, null, one, f1, f1, out, 0, None) == -1
    assert h.dt_reg_grad(1, fake, fake, (ctypes.c_int64 * 1)(-1), f1, f1, out, 1, None) == -1
    assert h.dt_reg_grad(-2, fake, fake, one, f1, f1, out, 0, None) == -1
    assert h.dt_reg_grad(1, fake, fake, one, f1, f1, None, 0, None) == -1             # go is a device pointer, never null


def test_ops_reject_cpu_tensors_loudly():
    from deeptables_amd import ops
    from deeptables_amd._lib import DtHipError
    with pytest.raises(DtHipError):
        ops.regularization_penalty([torch.zeros(3, requires_grad=True)], [(0.0, 0.01)])
    with pytest.raises(ValueError):
        ops.regularization_penalty([torch.zeros(3)], [])


# ---- nothing of a step stays alive ------------------------------------------------------------------------------------------
def test_no_activity_tensor_survives_the_step(monkeypatch):
    """Model collects the penalised activations of a forward and hands them over to regularization_loss(): after the step's
    backward nothing references them (no cycle for the cyclic collector to find, ADVICE.md: the weakref is dead WITHOUT
    gc.collect()).  The kernels' call is restated with torch ops here: the test is about the bookkeeping, on the CPU."""
    import gc
    from deeptables_amd import functional as Fn, ops
    seen = []

    def torch_penalty(tensors, coeffs):
        seen.append([weakref.ref(t) for t in tensors])
        return sum(l1 * t.abs().sum() + l2 * (t * t).sum() for t, (l1, l2) in zip(tensors, coeffs))

    monkeypatch.setattr(ops, 'regularization_penalty', torch_penalty)
    Fn.reset_uids()
    x = Fn.Input((3,))
    h = Fn.Dense(4, activity_regularizer='l2', kernel_regularizer='l1', name='d')(x)
    out = Fn.Dense(1, name='o')(Fn.Activation('relu', name='a')(h))
    m = Fn.Model(x, out)
    m.train()
    gc.disable()
    try:
        y = m([torch.randn(5, 3)])
        assert len(m._activity) == 1 and m._activity[0][1] == (0.0, 0.01) and m._activity[0][0].shape == (5, 4)
        loss = y.sum() + m.regularization_loss()
        assert m._activity is None and all(l._activity_sink is None for l in m.layers)
        loss.backward()
        refs = seen[0]
        assert len(refs) == 2
        del y, loss
        assert refs[0]() is not None                      # the kernel (a parameter) lives on ...
        assert refs[1]() is None                          # ... the activation does not
        # a forward nobody takes the penalties of: the next forward (or eval mode) drops the list
        m([torch.randn(5, 3)])
        r = weakref.ref(m._activity[0][0])
        m.eval()
        m([torch.randn(5, 3)])
        assert m._activity is None and r() is None
    finally:
        gc.enable()
