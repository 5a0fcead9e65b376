# -*- coding:utf-8 -*-
"""GPU: the GBM leaf features inside a resident feed (csrc/gbdt_feed.hip: dt_gbdt_bin_feed, dt_gbdt_leaves_feed; the edges from the
device profile; GbmLeavesEncoder.fit_feed / transform_feed behind DefaultPreprocessor.fit_feed).  Everything is EQUAL to its
numpy statement: bins to searchsorted, edges to gbm_bin_edges, leaves to a walk, the first tree to test_gbdt_gpu.grow_numpy."""
import numpy as np
import pandas as pd
import pytest
import torch

from tests.test_gbdt_gpu import grow_numpy

pytestmark = pytest.mark.gpu

R = 256                                                     # DT_GBDT_FEED_ROWS; a block takes a second tile beyond 256 R rows
LAYOUTS = {'ids': (8, []), 'floats': (0, [9]), 'mixed': (3, [4, 2]), 'two_groups': (5, [60, 8])}       # P = 8, 9, 9, 73 > 64


def walk(bins, feat, thr, child, nn):
    """leaf ids int32 [N, T] of feature-major bins [P, N] by the trees' node arrays"""
    out = np.zeros((bins.shape[1], len(nn)), np.int32)
    for t in range(len(nn)):
        for r in range(bins.shape[1]):
            c = 0 if nn[t] else -1
            while c >= 0:
                c = child[t, c, int(bins[feat[t, c], r] > thr[t, c])]
            out[r, t] = ~c
    return out


@pytest.mark.parametrize('layout', list(LAYOUTS))
@pytest.mark.parametrize('N', [1, R - 1, R, R + 1, 256 * R + 1])
def test_bin_feed_equals_searchsorted(dev, N, layout):
    from deeptables_amd import ops
    F, widths = LAYOUTS[layout]
    P = F + sum(widths)
    g = np.random.default_rng(N + P)
    # feature 0: no edge (a constant column), feature 1: 255 edges, the rest 1 .. 254; edges are float32 values and small integers,
    # so that values EQUAL to an edge occur in both kinds of block; 0.0 is an edge of every list that has one
    edges = [np.zeros(0)]
    for n in [255] + list(g.integers(1, 255, P - 2)):
        pool = np.unique(np.concatenate([np.arange(-40.0, 40.0), g.normal(0, 20, n).astype(np.float32)]))
        edges.append(np.sort(np.append(g.choice(pool[pool != 0], n - 1, replace=False), 0.0)))
    ids = g.integers(-40, 40, (N, F)).astype(np.int32) if F else None
    conts = []
    for b, w in enumerate(widths):
        first = F + sum(widths[:b])
        x = g.normal(0, 20, (N, w)).astype(np.float32)
        for j in range(w):
            e = edges[first + j]
            hit = g.random(N) < 0.3
            x[hit, j] = g.choice(e, hit.sum()) if len(e) else 1.0
        x[g.random((N, w)) < 0.1] = np.nan
        x[g.random((N, w)) < 0.1] = -0.0
        conts.append(x)
    up = lambda a: torch.from_numpy(a).to(dev)
    bins, packed = ops.gbdt_bin_feed(None if ids is None else up(ids), [up(x) for x in conts], edges)
    values = np.concatenate(([ids] if F else []) + conts, 1).astype(np.float64)
    ref = np.stack([np.where(np.isnan(values[:, f]), len(edges[f]), np.searchsorted(edges[f], values[:, f], side='right'))
                    for f in range(P)]).astype(np.uint8)
    P8 = (P + 7) // 8 * 8
    assert tuple(packed.shape) == (N, P8)
    assert np.array_equal(bins.cpu().numpy(), ref)
    assert np.array_equal(packed.cpu().numpy()[:, :P], ref.T) and not packed.cpu().numpy()[:, P:].any()


@pytest.mark.parametrize('max_bin', [255, 16])
def test_feed_edges_equal_gbm_bin_edges(dev, max_bin):
    from deeptables_amd.models.preprocessor import FeedRefusal, gbm_bin_edges, gbm_feed_edges
    g = np.random.default_rng(max_bin)
    N = 3001
    # the last column: max_bin distinct values, max_bin + 1 distinct keys (-0.0 and +0.0 are one value to np.unique)
    x = np.stack([g.normal(0, 1, N), g.integers(0, 12, N), np.exp(g.normal(0, 3, N)), np.full(N, 2.5),
                  g.integers(-(max_bin // 2), (max_bin - 1) // 2 + 1, N)], 1).astype(np.float32)
    x[::7, :3] = np.nan
    x[x[:, 4] == 0, 4] = np.where(g.random((x[:, 4] == 0).sum()) < 0.5, -0.0, 0.0)
    assert len(np.unique(x[:, 4])) == max_bin and np.signbit(x[x[:, 4] == 0, 4]).any() and not np.signbit(x[x[:, 4] == 0, 4]).all()
    ids = np.stack([g.integers(0, 1000, N), g.integers(0, 3, N)], 1).astype(np.int32)
    blocks = [torch.from_numpy(ids).to(dev), torch.from_numpy(x).to(dev)]
    names = ['a', 'b', 'wide', 'few', 'skew', 'const', 'both_zeros']
    got = gbm_feed_edges(blocks, names, max_bin)
    cols = list(ids.T) + list(x.T)
    assert len(np.unique(cols[2][::2])) > max_bin >= len(np.unique(cols[1]))          # both rules are taken
    for name, c, e in zip(names, cols, got):
        ref = gbm_bin_edges(c, max_bin)
        assert e.dtype == np.float64 and np.array_equal(e, ref), (name, len(e), len(ref))
    x[5, 2] = np.inf
    with pytest.raises(FeedRefusal, match="'skew'"):
        gbm_feed_edges([blocks[0], torch.from_numpy(x).to(dev)], names, max_bin)


def random_trees(g, T, L, P):
    """T trees in the grower's layout: node k splits an existing leaf l into l and the next free id; tree 0 has no node"""
    feat, thr = g.integers(0, P, (T, L - 1)).astype(np.int32), g.integers(0, 255, (T, L - 1)).astype(np.int32)
    child, nn = np.full((T, L - 1, 2), -1, np.int32), g.integers(1, L, T).astype(np.int32)
    nn[0] = 0
    for t in range(T):
        where = {0: -1}
        for k in range(nn[t]):
            l, new = int(g.choice(list(where))), len(where)
            child[t, k] = (~l, ~new)
            if where[l] >= 0:
                child[t].reshape(-1)[where[l]] = k
            where[l], where[new] = 2 * k, 2 * k + 1
    return feat, thr, child, nn


@pytest.mark.parametrize('mode', ['embedding', 'dense'])
@pytest.mark.parametrize('T', [1, 102])                     # 31 leaves: 101 trees are one LDS tile
def test_leaves_feed_equals_a_numpy_walk(dev, T, mode):
    from deeptables_amd import ops
    N, P, L, F = 3 * 64 + 7, 9, 31, 4
    g = np.random.default_rng(T)
    bins = g.integers(0, 256, (P, N)).astype(np.uint8)
    feat, thr, child, nn = random_trees(g, T, L, P)
    trees = {k: torch.from_numpy(v).to(dev) for k, v in dict(node_feat=feat, node_bin=thr, node_child=child, n_nodes=nn).items()}
    ids = torch.from_numpy(g.integers(0, 99, (N, F)).astype(np.int32)).to(dev)
    packed = ops.gbdt_pack(torch.from_numpy(bins).to(dev))
    got = ops.gbdt_leaves_feed(packed, trees, L, mode, ids=ids).cpu().numpy()
    ref = walk(bins, feat, thr, child, nn)
    assert (ref[:, 0] == 0).all() and (T == 1 or ref.max() > 0)
    if mode == 'embedding':
        assert got.dtype == np.int32 and np.array_equal(got[:, :F], ids.cpu().numpy()) and np.array_equal(got[:, F:], ref)
    else:
        assert got.dtype == np.float32 and np.array_equal(got, ref.astype(np.float32))


def frame(task, N=300):
    g = np.random.default_rng(4)
    df = pd.DataFrame({'s0': g.integers(0, 5, N).astype(str), 'c1': g.integers(0, 9, N), 'x0': g.normal(0, 1, N),
                       'x1': g.normal(0, 1, N).astype(np.float32), 'x2': np.exp(g.normal(0, 2, N))})
    df.loc[::11, 'x0'] = np.nan
    z = df['x1'] * 1.5 - np.log(df['x2']) + (df['s0'] == '1') * 2.0 + g.normal(0, 0.5, N)
    return df, (z > 0).astype(int).values if task == 'binary' else np.digitize(z, np.quantile(z, [0.33, 0.66]))


GBM = dict(n_estimators=4, num_leaves=7, min_child_samples=5)


def config(task, kind, **kw):
    from deeptables_amd.models import ModelConfig, deepnets
    return ModelConfig(nets=deepnets.DeepFM, metrics=['accuracy'], earlystopping_patience=0, task=task, apply_gbm_features=True,
                       gbm_params=GBM, gbm_feature_type=kind, embedding_dropout=0, **kw)


@pytest.mark.parametrize('kind', ['embedding', 'dense'])
@pytest.mark.parametrize('task', ['binary', 'multiclass'])
def test_fit_feed_with_gbm_features(dev, task, kind):
    from deeptables_amd import ops, training
    from deeptables_amd.models.preprocessor import DefaultPreprocessor
    df, y = frame(task)
    pp = DefaultPreprocessor(config(task, kind))
    feed = pp.fit_feed(df, y, device=dev, mode=True)
    assert feed.fit_path == 'device'
    enc = pp.X_transformers['gbm_features']
    K = 3 if task == 'multiclass' else 1
    T, F = GBM['n_estimators'] * K, len(enc.cat_vars)
    assert enc.feed_fitted_ and list(pp.X_transformers)[-2:] == ['gbm_features', 'last'] and len(enc.n_nodes_) == T
    # the features the trees saw, the leaf columns they made
    ids = feed.cat[:, :F].contiguous()
    conts = feed.conts if kind == 'embedding' else feed.conts[:-1]
    leaves = (feed.cat[:, F:] if kind == 'embedding' else feed.conts[-1]).cpu().numpy()
    bins = ops.gbdt_bin_feed(ids, conts, enc.edges_)[0]
    yd = torch.from_numpy(pp.transform_y(y).astype(np.float32)).to(dev)
    init = torch.from_numpy(np.atleast_1d(enc.init_score_)).to(dev)[:, None].expand(K, len(df)).contiguous()
    qg, qh, _ = ops.gbdt_gradients_softmax(init, yd, K) if K > 1 else ops.gbdt_gradients(init[0], yd, 'binary')
    p = dict(GBM, reg_lambda=0.0, min_split_gain=0.0, learning_rate=0.1, sexp=(23, 25))
    ref = grow_numpy(bins.cpu().numpy(), qg.reshape(K, -1)[0].cpu().numpy(), qh.reshape(K, -1)[0].cpu().numpy(), p)
    n = int(ref['n_nodes'][0])
    assert n == enc.n_nodes_[0] and n > 0
    for k in ('node_feat', 'node_bin', 'node_child'):
        assert np.array_equal(getattr(enc, k + '_')[0][:n], ref[k][:n]), k
    assert np.array_equal(enc.leaf_value_[0].view(np.uint32), ref['leaf_value'].view(np.uint32))
    assert np.array_equal(leaves, walk(bins.cpu().numpy(), enc.node_feat_, enc.node_bin_, enc.node_child_, enc.n_nodes_))
    names = [f'gbm_leaf_{t}' for t in range(T)]
    if kind == 'embedding':
        vocab = {c.name: c.vocabulary_size for c in pp.categorical_columns}
        assert [vocab[nm] for nm in names] == (leaves.max(0) + 1).tolist() == (enc.n_nodes_ + 1).tolist()
    else:
        assert pp.continuous_columns[-1].name == 'input_continuous_gbm_leaves' and pp.continuous_columns[-1].column_names == names
    # transform_feed reproduces the fit's blocks, and both are the host construction bit for bit
    again = pp.transform_feed(df, device=dev, mode=True)
    host = training.TableBatches(pp.transform_X(df.copy()), None, pp.categorical_columns, pp.continuous_columns, dev)
    assert again.transform_path == 'device' and again.kinds == feed.kinds == host.kinds
    for a, b, c in zip(feed.blocks, again.blocks, host.blocks):
        assert a.dtype == b.dtype == c.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert torch.equal(a.view(torch.int32), c.view(torch.int32))


def test_host_fitted_gbm_step_still_refuses(dev):
    from deeptables_amd.models.preprocessor import DefaultPreprocessor
    df, y = frame('binary')
    pp = DefaultPreprocessor(config('binary', 'embedding'))
    pp.fit_transform(df.copy(), y)
    with pytest.raises(ValueError, match='fitted on the host'):
        pp.transform_feed(df, device=dev, mode=True)
    assert pp.transform_feed(df, device=dev).transform_path == 'host'


@pytest.mark.parametrize('kind', ['embedding', 'dense'])
def test_deeptable_fit_feed_with_gbm_features(dev, kind, tmp_path):
    from deeptables_amd import functional
    from deeptables_amd.models import DeepTable
    df, y = frame('binary')
    functional.set_seed(3)
    dt = DeepTable(config=config('binary', kind))
    dt.fit_feed(df, y, batch_size=64, epochs=1, verbose=0, mode=True)
    assert dt.fit_path == 'device'
    proba = dt.predict_proba(df)
    assert proba.shape == (len(df), 2) and np.isfinite(proba).all()
    assert dt.make_feed(df).transform_path == 'device'
    dt.save(str(tmp_path))
    assert np.array_equal(DeepTable.load(str(tmp_path)).predict_proba(df), proba)
