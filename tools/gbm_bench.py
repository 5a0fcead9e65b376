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
    python tools/gbm_bench.py [--rows N] [--trees T] [--repeats R] [--no-sklearn] [--out FILE]"""
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


def frame(rows, seed=0):
    g = np.random.default_rng(seed)
    df = pd.DataFrame({f'C{i}': g.integers(0, 1000, rows) for i in range(26)})
    for j in range(13):
        df[f'I{j}'] = g.normal(0, 1, rows).astype(np.float32)
    z = df['I0'] * 1.2 - df['I1'] + (df['C0'] % 7 == 0) * 1.5 + (df['C1'] > 500) * 0.7 + g.normal(0, 1, rows)
    return df, (z > 0).astype(np.int64).values


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=1 << 20)
    ap.add_argument('--trees', type=int, default=100)
    ap.add_argument('--leaves', type=int, default=31)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--no-sklearn', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gbm_features.jsonl'))
    a = ap.parse_args()
    import torch
    import __graft_entry__ as entry
    assert torch.cuda.is_available(), 'gbm_bench measures on the GPU; there is no CPU figure'
    from deeptables_amd import ops
    from deeptables_amd.models.preprocessor import GbmLeavesEncoder
    df, y = frame(a.rows)
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

    GbmLeavesEncoder(cats, conts, 'binary', n_estimators=3, num_leaves=a.leaves).fit_transform(df, y)           # warm-up
    fits = []
    for _ in range(a.repeats):
        enc = GbmLeavesEncoder(cats, conts, 'binary', **kw)
        t, Xt = timed(lambda: enc.fit_transform(df, y))
        fits.append(t)
    names = enc.new_columns
    leaves = Xt[names].values
    s = enc.raw_scores(leaves).astype(np.float64)
    loss = float(np.mean(np.logaddexp(0, s) - y * s))
    roles = {}
    enc_k = GbmLeavesEncoder(cats, conts, 'binary', **kw)
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
            p = clf.predict_proba(df.values)[:, 1]
            t_pred = time.perf_counter() - t0
        p = np.clip(p, 1e-15, 1 - 1e-15)
        rec['sklearn'] = {'fit_s': t_fit, 'predict_proba_s': t_pred, 'threads': 16, 'repeats': 1,
                          'train_log_loss': float(-np.mean(y * np.log(p) + (1 - y) * np.log(1 - p)))}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'a') as f:
        f.write(json.dumps(rec) + '\n')
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
