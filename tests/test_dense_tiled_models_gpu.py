# -*- coding:utf-8 -*-
"""GPU: the two presets whose widest Dense layers lie outside csrc/dense.hip's LDS slab — FiBiNet (tower input K = 1443 here,
10,413 at the benchmark shape) and FGCNN at the benchmark shape (recombination 2,912 -> 832 and 1,792 -> 416, tower input
1,677) — train one step on the library's own kernels: no product goes to the vendor GEMM, and logits and gradients match
the oracle within the bars of tests/test_models_gpu.py (logits 1e-4 absolute, gradients 2e-4 max-rel)."""
import logging

import pytest
import torch

pytestmark = pytest.mark.gpu

B = 64
MODELS = {
    # name: (nets, F, Nd, [(layer, K, M)]: Dense layers that dt_dense_supported refuses at this batch size)
    'FiBiNet': ('fibi_dnn_nets', 10, 3, [('fibi_dnn_dense_1', 1443, 128)]),
    'FGCNN': ('fgcnn_dnn_nets', 26, 13, [('fgcnn_dnn_dense_1', 1677, 128)]),
}


def _build(name, D=16, vocab=20, seed=3):
    from deeptables_amd import functional
    from deeptables_amd.models import ModelConfig, DeepModel
    from deeptables_amd.models.metainfo import CategoricalColumn, ContinuousColumn
    nets, F, Nd, _ = MODELS[name]
    functional.set_seed(seed)
    conf = ModelConfig(nets=[nets], fixed_embedding_dim=True, embeddings_output_dim=D, embedding_dropout=0, dense_dropout=0,
                       metrics=['AUC'])
    cats = [CategoricalColumn(f'C{i}', vocab + i, D) for i in range(F)]       # small vocabularies: dense table gradient
    conts = [ContinuousColumn('input_continuous_all', [f'I{j}' for j in range(Nd)])]
    dm = DeepModel('binary', 2, conf, cats, conts)
    dm.build()
    return dm, cats, Nd


class _Records(logging.Handler):
    def __init__(self):
        super().__init__(level=logging.DEBUG)
        self.messages = []

    def emit(self, record):
        self.messages.append(record.getMessage())


@pytest.mark.parametrize('name', list(MODELS))
def test_preset_trains_without_the_vendor_gemm_and_matches_the_oracle(dev, name):
    from deeptables_amd import functional
    from deeptables_amd._lib import lib
    from oracle import bridge, reference_layers as R
    from tests.test_models_gpu import batch
    dm, cats, Nd = _build(name)
    L = dm.model.layers_by_name
    for layer, K, M in MODELS[name][3]:
        assert tuple(L[layer].kernel.shape) == (K, M)
        assert lib().dt_dense_supported(B, K, M) == 0       # the shapes this file is about
    if name == 'FGCNN':
        recomb = sorted(tuple(l.dense_output.kernel.shape) for l in dm.model.layers if l.__class__.__name__ == 'FGCNN')
        assert recomb == [(1792, 416), (2912, 832)]
        assert all(lib().dt_dense_supported(B, K, M) == 0 for K, M in recomb)
    idx, dense, y = batch(cats, Nd, B, dev)
    w = bridge.oracle_weights(dm, requires_grad=True)
    ref_logit, _ = bridge.oracle_forward(dm, idx, dense, training=True, weights=w)
    R.binary_crossentropy_from_logits(ref_logit, y.double()).backward()

    noted = set(functional._VENDOR_GEMM_NOTED)
    handler = _Records()
    logger = logging.getLogger('deeptables_amd')
    logger.addHandler(handler)
    try:
        dm.model.train()
        dm.optimizer.zero_grad()
        logit = dm.model([idx.int().to(dev), dense.to(dev)])
        dm._loss(logit, y.to(dev)).backward()
        torch.cuda.synchronize()
    finally:
        logger.removeHandler(handler)

    def rel(a, b):
        b = torch.as_tensor(b).double()
        return (a.detach().double().cpu().reshape(b.shape) - b).abs().max().item() / max(b.abs().max().item(), 1e-12)

    err = (logit.detach().double().cpu() - ref_logit.detach()).abs().max().item()
    figures = {'logit': err}
    for i, (p, wt) in enumerate(bridge.param_pairs(dm, w)):
        assert p.grad is not None and wt.grad is not None, f'{name}: pair {i} of shape {tuple(p.shape)} got no gradient'
        figures[f'grad[{i}]{tuple(p.shape)}'] = rel(p.grad, wt.grad)
    table = L['emb_categorical_vars_all'].tables['d16']
    assert table.grad is not None
    figures['grad[table]'] = rel(table.grad, torch.cat([t.grad for t in w['emb_categorical_vars_all']], 0))
    print(f'{name}: ' + ', '.join(f'{k} {v:.2e}' for k, v in figures.items()))
    # the figures are printed first: the same body, run where these products still go to the vendor GEMM, shows its figures
    assert set(functional._VENDOR_GEMM_NOTED) == noted, set(functional._VENDOR_GEMM_NOTED) - noted
    assert not [m for m in handler.messages if 'vendor GEMM' in m], handler.messages
    assert err < 1e-4, f'{name}: logit error {err}'
    bad = {k: v for k, v in figures.items() if k != 'logit' and not v < 2e-4}
    assert not bad, f'{name}: gradient max-rel over 2e-4: {bad}'
