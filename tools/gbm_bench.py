# -*- coding:utf-8 -*-
"""GBM leaf features on the benchmark's column layout: 26 int64 categoricals (1000 values) + 13 float32 columns, 1,048,576 rows,
100 trees of 31 leaves (GbmLeavesEncoder, csrc/gbdt.hip).  Writes profiles/gbm_features.jsonl:
  fit            wall seconds of GbmLeavesEncoder.fit_transform (binning, the boosting loop, the read-back), warmed up by a short
                 fit, the median of `--repeats` fits with min and max, the device drained at the end
  fit_kernels    a fit of its own with the device drained around every entry-point call: seconds per kernel role
  predict        GbmLeavesEncoder.transform on the same rows (upload, bin, pack, walk, read-back) and the walk's launch alone
  sklearn        the yardstick: sklearn.ensemble.HistGradientBoostingClassifier at the same sizes (max_iter = trees,
                 max_leaf_nodes = leaves, no early stopping) on 16 CPU threads; fit and `apply`-free predict_proba seconds
A different implementation and not the same trees: both times are recorded, no ratio is asserted.
--classes K (3 .. 64): a K-class target, softmax boosting with K trees per round (`trees` rounds), and one more record:
  growth         the boosting loop alone on the same bins, per round: one ops.gbdt_grow_trees call (the K class trees in
                 lock-step) against K ops.gbdt_grow_tree calls on the same K gradient sets (the one-class-at-a-time fit); both
                 give the same scores to the bit (asserted); the median of `--repeats` loops after a warm-up, and a per-role
                 split of each from a loop of its own with the device drained around every call
scikit-learn's multiclass hessian has no K / (K - 1) factor: its line is informational.
--feed: one record of its own ('bench': 'gbm_features_feed') instead — the encoder inside a resident feed against the host
encoder on the same rows in the same run.  The columns are put on the device once as a feed holds them (the int32 id block
[N, 26], the float32 block [N, 13]); then, alternating, the median of `--repeats` after a warm-up, with min and max:
  host           GbmLeavesEncoder.fit_transform / transform on the frame (as above)
  feed           GbmLeavesEncoder.fit_feed / transform_feed on the blocks (profile and edges, one binning launch, the boosting
                 loop, one leaf launch; only the fitted trees come back), and `roles`: a fit of its own with the device drained
                 between profile_edges, bin_launch, boosting_loop, state_readback and leaf_launch
The frame's continuous columns are float32, so both fits see the same values: the same trees are asserted.
    python tools/gbm_bench.py [--rows N] [--trees T] [--classes K] [--repeats R] [--feed] [--no-sklearn] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def frame(rows, seed=0, classes=0):
    g = np.random.default_rng(seed)
    df = pd.DataFrame({f'C{i}': g.integers(0, 1000, rows) for i in range(26)})
    for j in range(13):
        df[f'I{j}'] = g.normal(0, 1, rows).astype(np.float32)
    z = df['I0'] * 1.2 - df['I1'] + (df['C0'] % 7 == 0) * 1.5 + (df['C1'] > 500) * 0.7 + g.normal(0, 1, rows)
    if classes:                                             # K equally frequent classes along the same signal
        return df, np.searchsorted(np.quantile(z, np.arange(1, classes) / classes), z).astype(np.int64)
    return df, (z > 0).astype(np.int64).values


def log_loss(scores, y):
    """the mean log loss of raw scores: [N] logits of a binary target or [N, K] of a K-class one"""
    s = scores.astype(np.float64)
    if s.ndim == 1:
        return float(np.mean(np.logaddexp(0, s) - y * s))
    m = s.max(1)
    return float(np.mean(np.log(np.exp(s - m[:, None]).sum(1)) + m - s[np.arange(len(y)), y]))


def growth(ops, torch, enc, df, y, a, timed, stats):
    """`trees` softmax rounds on the encoder's bins: one gbdt_grow_trees call per round against K gbdt_grow_tree calls"""
    dev, K, L, N = torch.device('cuda', 0), a.classes, a.leaves, len(y)
    bins = ops.gbdt_bin(enc._upload(df, dev), enc.edges_)
    yd = torch.from_numpy(y.astype(np.float32)).to(dev)
    init = torch.from_numpy(enc.init_score_).to(dev)
    grow = {k: enc.params[k] for k in ('num_leaves', 'min_child_samples', 'reg_lambda', 'min_split_gain', 'learning_rate')}
    ws = {True: ops.GbdtWorkspace(bins, L, num_classes=K), False: ops.GbdtWorkspace(bins, L)}
    i32 = dict(dtype=torch.int32, device=dev)
    out = {'node_feat': torch.empty((K, L - 1), **i32), 'node_bin': torch.empty((K, L - 1), **i32),
           'node_child': torch.empty((K, L - 1, 2), **i32), 'n_nodes': torch.empty(K, **i32),
           'leaf_value': torch.empty((K, L), dtype=torch.float32, device=dev), 'row_leaf': torch.empty((K, N), **i32)}
    grads = (torch.empty((K, N), **i32), torch.empty((K, N), **i32), torch.empty(2, **i32))

    def loop(batched, rounds, timings=None):
        scores = init[:, None].expand(K, N).contiguous()
        for _ in range(rounds):
            if timings is not None:
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
            qg, qh, s = ops.gbdt_gradients_softmax(scores, yd, K, out=grads)
            if timings is not None:
                torch.cuda.synchronize(dev)
                timings['gradients'] = timings.get('gradients', 0.0) + time.perf_counter() - t0
            if batched:
                ops.gbdt_grow_trees(bins, qg, qh, dict(grow, sexp=s), workspace=ws[True], scores=scores, out=out, timings=timings)
            else:
                for c in range(K):
                    one = {k: (v[c:c + 1] if k == 'n_nodes' else v[c]) for k, v in out.items()}
                    ops.gbdt_grow_tree(bins, qg[c], qh[c], dict(grow, sexp=s), workspace=ws[False], scores=scores[c], out=one,
                                       timings=timings)
        return scores

    modes = ((True, 'grow_trees'), (False, 'grow_tree_x_K'))
    rec, final, ts = {'rounds': a.trees, 'classes': K}, {}, {name: [] for _, name in modes}
    for batched, _ in modes:
        loop(batched, 2)                                                                                     # warm-up
    for _ in range(a.repeats):                              # the two loops alternate, so a busy host slows both alike
        for batched, name in modes:
            t, final[name] = timed(lambda: loop(batched, a.trees))
            ts[name].append(t)
    for batched, name in modes:
        roles = {}
        t_roles, _ = timed(lambda: loop(batched, a.trees, roles))
        rec[name] = dict(stats(ts[name]), per_round_s=stats(ts[name])['median_s'] / a.trees, roles=dict(roles, total_s=t_roles))
    assert torch.equal(final['grow_trees'], final['grow_tree_x_K']), 'both loops must give the same scores to the bit'
    return rec


def feed_leg(torch, enc_cls, df, y, a, task, kw, cats, conts, timed, stats, dev):
    """--feed: the in-feed fit and transform against the host ones, alternating"""
    from deeptables_amd.utils import consts
    blocks = [torch.from_numpy(np.ascontiguousarray(df[cats].values, dtype=np.int32)).to(dev),
              torch.from_numpy(np.ascontiguousarray(df[conts].values, dtype=np.float32)).to(dev)]
    kinds = ['cat', 'cont']
    enc_cls(cats, conts, n_estimators=3, num_leaves=a.leaves, **task).fit_transform(df, y)                     # warm-up
    enc_cls(cats, conts, n_estimators=3, num_leaves=a.leaves, **task).fit_feed(blocks, kinds, y)
    t = {k: [] for k in ('host_fit', 'feed_fit', 'host_transform', 'feed_transform')}
    for _ in range(a.repeats):
        host, feed = enc_cls(cats, conts, **task, **kw), enc_cls(cats, conts, **task, **kw)
        t['host_fit'].append(timed(lambda: host.fit_transform(df, y))[0])
        s, (wide, _kinds) = timed(lambda: feed.fit_feed(blocks, kinds, y, consts.GBM_FEATURE_TYPE_EMB))
        t['feed_fit'].append(s)
    for k in ('node_feat_', 'node_bin_', 'node_child_', 'n_nodes_', 'leaf_value_'):
        assert np.array_equal(getattr(host, k), getattr(feed, k)), f'the two fits must grow the same trees: {k}'
    for i in range(a.repeats + 1):                          # the first transform of each warms up
        s_host, Xp = timed(lambda: host.transform(df))
        s_feed, (again, _kinds) = timed(lambda: feed.transform_feed(blocks, kinds, consts.GBM_FEATURE_TYPE_EMB))
        if i:
            t['host_transform'].append(s_host)
            t['feed_transform'].append(s_feed)
    assert torch.equal(again[0], wide[0]), 'transform_feed must reproduce the blocks of the fit'
    assert np.array_equal(Xp[host.new_columns].values, wide[0][:, len(cats):].cpu().numpy()), 'feed and host leaves must be equal'
    roles = {}
    timed_enc = enc_cls(cats, conts, **task, **kw)
    timed_enc.timings = roles
    t_roles, _ = timed(lambda: timed_enc.fit_feed(blocks, kinds, y))
    return {'host': {'fit_transform': stats(t['host_fit']), 'transform': stats(t['host_transform'])},
            'feed': {'fit_feed': stats(t['feed_fit']), 'transform_feed': stats(t['feed_transform']),
                     'roles': dict(roles, total_s=t_roles, note='device drained between roles')},
            'same_trees': True, 'nodes': int(feed.n_nodes_.sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=1 << 20)
    ap.add_argument('--trees', type=int, default=100)
    ap.add_argument('--leaves', type=int, default=31)
    ap.add_argument('--classes', type=int, default=0, help='0: the binary target; 3 .. 64: a K-class target, K trees per round')
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--no-sklearn', action='store_true')
    ap.add_argument('--feed', action='store_true', help='the in-feed fit / transform against the host ones; a record of its own')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gbm_features.jsonl'))
    a = ap.parse_args()
    import torch
    import __graft_entry__ as entry
    assert torch.cuda.is_available(), 'gbm_bench measures on the GPU; there is no CPU figure'
    from deeptables_amd import ops
    from deeptables_amd.models.preprocessor import GbmLeavesEncoder
    df, y = frame(a.rows, classes=a.classes)
    task = dict(task='multiclass', num_classes=a.classes) if a.classes else dict(task='binary')
    cats, conts = [f'C{i}' for i in range(26)], [f'I{j}' for j in range(13)]
    kw = dict(n_estimators=a.trees, num_leaves=a.leaves)
    dev = torch.device('cuda', 0)

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, out

    def stats(ts):
        return {'median_s': statistics.median(ts), 'min_s': min(ts), 'max_s': max(ts), 'repeats': len(ts)}

    if a.feed:
        rec = dict({'bench': 'gbm_features_feed', 'rows': a.rows, 'columns': {'categorical': 26, 'continuous': 13}, 'trees': a.trees,
                    'leaves': a.leaves, 'classes': a.classes, 'source_hash': entry.source_hash(),
                    'device': torch.cuda.get_device_name(0)},
                   **feed_leg(torch, GbmLeavesEncoder, df, y, a, task, kw, cats, conts, timed, stats, dev))
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            f.write(json.dumps(rec) + '\n')
        print(json.dumps(rec))
        return
    GbmLeavesEncoder(cats, conts, n_estimators=3, num_leaves=a.leaves, **task).fit_transform(df, y)           # warm-up
    fits = []
    for _ in range(a.repeats):
        enc = GbmLeavesEncoder(cats, conts, **task, **kw)
        t, Xt = timed(lambda: enc.fit_transform(df, y))
        fits.append(t)
    names = enc.new_columns
    leaves = Xt[names].values
    loss = log_loss(enc.raw_scores(leaves), y)
    roles = {}
    enc_k = GbmLeavesEncoder(cats, conts, **task, **kw)
    enc_k.timings = roles
    t_roles, _ = timed(lambda: enc_k.fit_transform(df, y))
    preds = []
    for _ in range(a.repeats + 1):
        t, Xp = timed(lambda: enc.transform(df))
        preds.append(t)
    assert np.array_equal(Xp[names].values, leaves), 'the training rows must get the leaves of the fit'
    packed = ops.gbdt_pack(ops.gbdt_bin(enc._upload(df, dev), enc.edges_))
    trees = {k: torch.from_numpy(getattr(enc, k + '_')).to(dev) for k in ('node_feat', 'node_bin', 'node_child', 'n_nodes')}
    walks = [timed(lambda: ops.gbdt_predict_leaves(packed, trees, a.leaves))[0] for _ in range(a.repeats + 1)]
    rec = {'bench': 'gbm_features', 'rows': a.rows, 'columns': {'categorical': 26, 'continuous': 13}, 'trees': a.trees,
           'leaves': a.leaves, 'source_hash': entry.source_hash(), 'device': torch.cuda.get_device_name(0),
           'fit': stats(fits), 'train_log_loss': loss, 'nodes': int(enc.n_nodes_.sum()),
           'fit_kernels': dict(roles, total_s=t_roles, note='device drained around every call: slower than fit'),
           'predict': {'transform': stats(preds[1:]), 'walk_launch': stats(walks[1:])}}
    if a.classes:
        rec['classes'] = a.classes
        rec['growth'] = growth(ops, torch, enc, df, y, a, timed, stats)
    if not a.no_sklearn:
        from sklearn.ensemble import HistGradientBoostingClassifier
        from threadpoolctl import threadpool_limits
        with threadpool_limits(limits=16):
            clf = HistGradientBoostingClassifier(max_iter=a.trees, max_leaf_nodes=a.leaves, learning_rate=0.1, max_bins=255,
                                                 early_stopping=False, min_samples_leaf=20)
            t0 = time.perf_counter()
            clf.fit(df.values, y)
            t_fit = time.perf_counter() - t0
            t0 = time.perf_counter()
            p = clf.predict_proba(df.values)
            t_pred = time.perf_counter() - t0
        if a.classes:
            sk_loss = float(-np.mean(np.log(np.clip(p[np.arange(len(y)), y], 1e-15, 1.0))))
        else:
            p = np.clip(p[:, 1], 1e-15, 1 - 1e-15)
            sk_loss = float(-np.mean(y * np.log(p) + (1 - y) * np.log(1 - p)))
        rec['sklearn'] = {'fit_s': t_fit, 'predict_proba_s': t_pred, 'threads': 16, 'repeats': 1, 'train_log_loss': sk_loss}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'a') as f:
        f.write(json.dumps(rec) + '\n')
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
