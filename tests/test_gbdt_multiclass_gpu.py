# -*- coding:utf-8 -*-
"""GPU: softmax boosting behind apply_gbm_features on a multiclass task (csrc/gbdt.hip dt_gbdt_grad_softmax, dt_gbdt_mc_*): the K
class trees of a round grown in lock-step are EQUAL, class by class, to the numpy grower of tests/test_gbdt_gpu.py."""
import numpy as np
import pandas as pd
import pytest
import torch

from tests import precision as P
from tests.test_gbdt_gpu import PARAMS, assert_same_tree, draw, grow_numpy

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('L', [2, 31])
@pytest.mark.parametrize('Pf', [1, 9])                  # 9: one feature past a block's feature group
@pytest.mark.parametrize('N', [40, 257, 5000])          # two children of 20; 5000: two histogram chunks, three partition chunks
@pytest.mark.parametrize('K', [3, 5])
def test_batched_growth_equals_the_numpy_grower_class_by_class(dev, K, N, Pf, L):
    """one bin matrix, every class its own gradients; class 1's are constant powers of two — every gain is exactly 0, so its
    tree has no node and its launches idle while the other classes grow on"""
    from deeptables_amd import ops
    bins = draw(N, Pf, 100 * N + Pf)[0]
    grads = [draw(N, Pf, 100 * N + Pf + c)[1:] for c in range(K)]
    grads[1] = (np.full(N, 1 << 20, np.int32), np.full(N, 1 << 22, np.int32))
    qg, qh = np.stack([g for g, _ in grads]), np.stack([h for _, h in grads])
    p = dict(PARAMS, num_leaves=L)
    refs = [grow_numpy(bins, qg[c], qh[c], p) for c in range(K)]
    n0 = int(refs[0]['n_nodes'][0])
    assert int(refs[1]['n_nodes'][0]) == 0 and n0 >= 1 and (N < 5000 or n0 == L - 1)
    scores = torch.zeros((K, N), dtype=torch.float32, device=dev)
    out = ops.gbdt_grow_trees(torch.from_numpy(bins).to(dev), torch.from_numpy(qg).to(dev), torch.from_numpy(qh).to(dev), p, scores=scores)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert got['n_nodes'].shape == (K,) and got['node_child'].shape == (K, L - 1, 2) and got['row_leaf'].shape == (K, N)
    for c in range(K):
        tree = {k: (v[c:c + 1] if k == 'n_nodes' else v[c]) for k, v in got.items()}
        assert_same_tree(tree, refs[c])
        want = np.float32(0) + tree['leaf_value'][tree['row_leaf']]
        assert np.array_equal(scores[c].cpu().numpy().view(np.uint32), want.view(np.uint32)), c


@pytest.mark.parametrize('N', [1, 257, 5000])
@pytest.mark.parametrize('K', [3, 64])
def test_softmax_gradients_against_float64(dev, K, N):
    """each quantised value within one quantum plus precision.py's fp32 bar (STEP_BAR x FLOOR of the largest reference value),
    scaled by 2^S — test_gradients_against_float64's bound; scores of +-80 saturate the softmax, one label is K, one is NaN"""
    from deeptables_amd import ops
    g = torch.Generator().manual_seed(100 * K + N)
    bar = P.STEP_BAR['fp32'] * P.FLOOR
    s = torch.randn((K, N), generator=g) * 3
    s[0, ::5], s[1, ::7] = 80.0, -80.0
    y = torch.randint(0, K, (N,), generator=g).float()
    y[N // 2], y[-1] = K, float('nan')
    qg, qh, sexp = (t.cpu().numpy() for t in ops.gbdt_gradients_softmax(s.to(dev), y.to(dev), K))
    sd = s.double().numpy()
    e = np.exp(sd - sd.max(0))
    p = e / e.sum(0)
    hit = y.numpy()[None, :] == np.arange(K, dtype=np.float32)[:, None]
    assert hit.sum() == max(N - 2, 0)                                       # the two odd labels name no class
    h = K / (K - 1) * (p * (1 - p))
    assert sexp.tolist() == [23, 25]
    assert np.abs(qg - (p - hit) * 2.0 ** 23).max() <= 1 + bar * 2.0 ** 23
    assert np.abs(qh - h * 2.0 ** 25).max() <= 1 + bar * h.max() * 2.0 ** 25
    assert np.abs(qg).max() < 2 ** 24 and np.abs(qh).max() < 2 ** 24


@pytest.mark.parametrize('K', [2, 65])
def test_softmax_gradients_refuse_class_counts_outside_the_domain(dev, K):
    from deeptables_amd import ops
    from deeptables_amd._lib import DtHipError
    with pytest.raises(DtHipError, match='outside'):
        ops.gbdt_gradients_softmax(torch.zeros((K, 4), device=dev), torch.zeros(4, device=dev), K)


@pytest.mark.parametrize('kind', ['embedding', 'dense'])
def test_deeptable_with_gbm_features_on_three_classes(dev, kind, tmp_path):
    """labels follow one categorical column (10 % noise).  The numpy restatement of three rounds (num_leaves 7, learning rate
    0.5) on this frame gives a training log loss of 0.305 against the prior's entropy 1.099: the margin below is wide."""
    from deeptables_amd import functional
    from deeptables_amd.models import DeepTable, ModelConfig, deepnets
    from deeptables_amd.models.preprocessor import DefaultPreprocessor
    g = np.random.default_rng(11)
    N = 3000
    df = pd.DataFrame({f'c{i}': g.integers(0, 6 + 2 * i, N).astype(str) for i in range(3)})
    df['x0'], df['x1'] = g.normal(0, 1, N), g.normal(0, 1, N)
    y = np.where(g.random(N) < 0.1, g.integers(0, 3, N), df['c0'].astype(int) % 3)
    conf = ModelConfig(nets=deepnets.DeepFM, metrics=['accuracy'], earlystopping_patience=0, task='multiclass', apply_gbm_features=True,
                       gbm_params={'n_estimators': 3, 'num_leaves': 7, 'learning_rate': 0.5}, gbm_feature_type=kind, embedding_dropout=0)
    functional.set_seed(3)
    dt = DeepTable(config=conf)
    dt.fit(df.copy(), y, batch_size=256, epochs=1, verbose=0)
    proba = dt.predict_proba(df.copy())
    assert proba.shape == (N, 3) and np.allclose(proba.sum(1), 1.0, atol=1e-5)
    pp = dt.preprocessor
    enc = pp.X_transformers['gbm_features']
    names = [f'gbm_leaf_{j}' for j in range(9)]
    assert enc.new_columns == names and enc.init_score_.shape == (3,) and enc.leaf_value_.shape == (9, 7)
    leaves = pp.transform_X(df.copy())[names].values.astype(np.int64)
    Xf, yt = DefaultPreprocessor(conf).fit_transform(df.copy(), y)
    assert np.array_equal(Xf[names].values.astype(np.int64), leaves)       # the training rows get the leaves of a fit
    s = enc.raw_scores(leaves)
    want = np.tile(enc.init_score_, (N, 1))
    for j in range(9):
        want[:, j % 3] = want[:, j % 3] + enc.leaf_value_[j][leaves[:, j]]
    assert s.shape == (N, 3) and s.dtype == np.float32 and np.array_equal(s, want)
    z = s.astype(np.float64)
    loss = np.mean(np.log(np.exp(z - z.max(1, keepdims=True)).sum(1)) + z.max(1) - z[np.arange(N), yt])
    prior = np.bincount(yt, minlength=3) / N
    assert loss < -(prior * np.log(prior)).sum()
    before = dt.predict(df.copy())
    dt.save(str(tmp_path))
    assert np.array_equal(DeepTable.load(str(tmp_path)).predict(df.copy()), before)
