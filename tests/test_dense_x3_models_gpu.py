# -*- coding:utf-8 -*-
"""GPU: FiBiNet (F = 10, D = 16, Nd = 3) and FGCNN at the benchmark shape train one step at B = 64 with the Dense precision
modes switched on through the builders' key ('dense_mfma_dtype' in dnn_params, for FGCNN in fgcnn_params as well), against
oracle.bridge as tests/test_dense_tiled_models_gpu.py does:
  bf16x3  logits 1e-4 absolute, gradients 2e-4 max-rel: the project's fp32 bars
  bf16    logits 1e-2 absolute.  Both towers are relu towers whose first, widest Dense now runs one bf16 product: units flip
          that no bias shift clears, and by the note of tests/precision.py on plain-bf16 forwards inside a whole step only the
          forward figure is held there; the gradients' relative L2 errors are printed against the 2e-2 of the AutoInt bf16 mode
          (measured on the MI355X: logits 7.5e-4 / 8.4e-4, gradients 1.0e-2 .. 7.7e-2 in relative L2).
A spy on the library shows the wide layers went through dt_dense_x3_* and none through dt_dense_tiled_*; with the mode off the
model computes bit for bit what a model built without the key computes."""
import pytest
import torch

from tests import precision as P

pytestmark = pytest.mark.gpu

B = 64
MODELS = {
    # name: (nets, F, Nd, wide Dense layers (K, M) that dt_dense_supported refuses at this batch size)
    'FiBiNet': ('fibi_dnn_nets', 10, 3, [(1443, 128)]),
    'FGCNN': ('fgcnn_dnn_nets', 26, 13, [(2912, 832), (1792, 416), (1677, 128)]),
}
DENSE = ['dt_dense_fwd', 'dt_dense_bwd', 'dt_dense_tiled_fwd', 'dt_dense_tiled_bwd', 'dt_dense_x3_fwd', 'dt_dense_x3_bwd']


class _Spy:
    """the library with the Dense entry points recorded as (name, args) on their way through"""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if name not in DENSE:
            return fn

        def call(*args):
            self.calls.append((name, args))
            return fn(*args)
        return call


def _build(name, mode, D=16, vocab=20, seed=3):
    from deeptables_amd import functional
    from deeptables_amd.models import ModelConfig, DeepModel
    from deeptables_amd.models.metainfo import CategoricalColumn, ContinuousColumn
    nets, F, Nd, _ = MODELS[name]
    functional.set_seed(seed)
    key = {} if mode is None else {'dense_mfma_dtype': mode}
    conf = ModelConfig(nets=[nets], fixed_embedding_dim=True, embeddings_output_dim=D, embedding_dropout=0, dense_dropout=0,
                       metrics=['AUC'],
                       dnn_params={'hidden_units': ((128, 0, False), (64, 0, False)), 'activation': 'relu', **key},
                       fgcnn_params={'fg_filters': (14, 16), 'fg_heights': (7, 7), 'fg_pool_heights': (2, 2),
                                     'fg_new_feat_filters': (2, 2), **key})
    cats = [CategoricalColumn(f'C{i}', vocab + i, D) for i in range(F)]       # small vocabularies: dense table gradient
    conts = [ContinuousColumn('input_continuous_all', [f'I{j}' for j in range(Nd)])]
    dm = DeepModel('binary', 2, conf, cats, conts)
    dm.build()
    return dm, cats, Nd


def _step(dm, idx, dense, y, dev, monkeypatch):
    from deeptables_amd import _lib, ops
    spy = _Spy(_lib.lib())
    monkeypatch.setattr(ops, 'lib', lambda: spy)
    dm.model.train()
    dm.optimizer.zero_grad()
    logit = dm.model([idx.int().to(dev), dense.to(dev)])
    dm._loss(logit, y.to(dev)).backward()
    torch.cuda.synchronize()
    monkeypatch.undo()
    return logit.detach(), spy.calls


def _wide(calls, kind):
    """(K, M) of the recorded calls of one direction that dt_dense_supported refuses"""
    from deeptables_amd._lib import lib
    at = 4 if kind == 'fwd' else 5
    return {n: sorted((a[at + 1], a[at + 2]) for m, a in calls if m == n and not lib().dt_dense_supported(*a[at:at + 3]))
            for n in DENSE if n.endswith(kind)}


@pytest.mark.parametrize('mode', ['bf16x3', 'bf16'])
@pytest.mark.parametrize('name', list(MODELS))
def test_preset_trains_in_a_dense_mode_and_matches_the_oracle(dev, monkeypatch, name, mode):
    from deeptables_amd import _lib
    from oracle import bridge, reference_layers as R
    from tests.test_models_gpu import batch
    monkeypatch.delenv('DT_AMD_DENSE_DTYPE', raising=False)
    dm, cats, Nd = _build(name, mode)
    idx, dense, y = batch(cats, Nd, B, dev)
    w = bridge.oracle_weights(dm, requires_grad=True)
    ref_logit, _ = bridge.oracle_forward(dm, idx, dense, training=True, weights=w)
    R.binary_crossentropy_from_logits(ref_logit, y.double()).backward()
    logit, calls = _step(dm, idx, dense, y, dev, monkeypatch)

    # the wide layers, and only they, on the new kernels; none on the fp32 tiled ones
    want = sorted(MODELS[name][3])
    code = {'bf16x3': _lib.DT_DENSE_X3, 'bf16': _lib.DT_DENSE_BF16}[mode]
    for kind, at in (('fwd', 8), ('bwd', 11)):
        wide = _wide(calls, kind)
        assert wide['dt_dense_x3_' + kind] == want and wide['dt_dense_tiled_' + kind] == [] and wide['dt_dense_' + kind] == []
        assert all(a[at] == code for n, a in calls if n == 'dt_dense_x3_' + kind)
    assert all(n.startswith('dt_dense_x3') or _lib.lib().dt_dense_supported(*a[4 if n.endswith('fwd') else 5:][:3])
               for n, a in calls)

    def rel(a, b):
        b = torch.as_tensor(b).double()
        return (a.detach().double().cpu().reshape(b.shape) - b).abs().max().item() / max(b.abs().max().item(), 1e-12)

    err = (logit.double().cpu() - ref_logit.detach()).abs().max().item()
    pairs = [(f'grad[{i}]{tuple(p.shape)}', p.grad, wt.grad) for i, (p, wt) in enumerate(bridge.param_pairs(dm, w))]
    table = dm.model.layers_by_name['emb_categorical_vars_all'].tables['d16']
    pairs.append(('grad[table]', table.grad, torch.cat([t.grad for t in w['emb_categorical_vars_all']], 0)))
    assert all(g is not None and r is not None and bool(torch.isfinite(g).all()) for _, g, r in pairs)
    maxrel = {k: rel(g, r) for k, g, r in pairs}
    l2 = {k: P.l2_rel(g, torch.as_tensor(r).reshape(g.shape)) for k, g, r in pairs}
    print(f'{name}/{mode}: logit {err:.2e}; max-rel ' + ', '.join(f'{k} {v:.2e}' for k, v in maxrel.items()))
    print(f'{name}/{mode}: l2-rel ' + ', '.join(f'{k} {v:.2e}' for k, v in l2.items()))
    if mode == 'bf16x3':
        assert err < 1e-4, f'{name}: logit error {err}'
        bad = {k: v for k, v in maxrel.items() if not v < 2e-4}
        assert not bad, f'{name}: gradient max-rel over 2e-4: {bad}'
    else:
        assert err < 1e-2, f'{name}: logit error {err}'


@pytest.mark.parametrize('name', list(MODELS))
def test_mode_off_is_bit_identical_to_a_model_without_the_key(dev, monkeypatch, name):
    """'float32' through the key, and no key at all: the same calls, the same bits (at B = 64 no product splits its batch, so
    no float atomics reorder a sum in the Dense layers; the embedding table's gradient, merged with atomics over duplicate
    rows, is left out)"""
    from tests.test_models_gpu import batch
    monkeypatch.delenv('DT_AMD_DENSE_DTYPE', raising=False)
    got = []
    for mode in (None, 'float32'):
        dm, cats, Nd = _build(name, mode)
        idx, dense, y = batch(cats, Nd, B, dev)
        logit, calls = _step(dm, idx, dense, y, dev, monkeypatch)
        table = dm.model.layers_by_name['emb_categorical_vars_all'].tables['d16']
        grads = [p.grad.clone() for p in dm.model.parameters() if p is not table and p.grad is not None]
        got.append((logit.clone(), grads, [(n, a[3:7] if n.endswith('fwd') else a[4:8]) for n, a in calls]))
    (la, ga, ca), (lb, gb, cb) = got
    assert ca == cb and not any('x3' in n for n, _ in ca)
    assert torch.equal(la, lb)
    assert len(ga) == len(gb) > 4 and all(torch.equal(a, b) for a, b in zip(ga, gb))
