# -*- coding:utf-8 -*-
"""Times the way from a raw frame to a fitted preprocessor and its resident feed both ways (GPU, not a test): (i) the host
yardstick `TableBatches(*pp.fit_transform(X, y), ..., resident=True)` — pandas' nunique / astype(str) / unique / mean / min /
max / np.quantile per column, then the transformed frame uploaded — and (ii) `pp.fit_feed(X, y, device=...)`: every numeric
column uploaded once, profiled by ops.column_profile (csrc/prep_fit.hip), the fit read off the profile, the feed written by
dt_prep_transform.  Then `DeepTable.fit` against `DeepTable.fit_feed` for one epoch.  Each way is warmed up with one call, then
the two are alternated `--repeats` times; a host clock with the device drained at both ends; medians with min and max.  The
device fit is split with `preprocessor.TIMINGS` (which drains the device around every phase, so the split is taken in calls of
its own): uploads, launches (profile, order statistics and transform; the small result copies included) and host work (the
remainder: typing, label maps of the distinct values, quantile interpolation, host-served columns).

The frame is tools/cross_validation_bench.make_frame's layout: 26 int64 categoricals + 13 float32 continuous columns.
Appends ONE JSON line to profiles/prep_fit.jsonl (and prints it).

    python tools/prep_fit_bench.py                         # 1,048,576 rows
    python tools/prep_fit_bench.py --rows 65536"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.cross_validation_bench import F_CAT, N_CONT, make_frame      # noqa: E402
from tools.transform_bench import same_bits, stats, timed               # noqa: E402


def alternate(host, device, dev, repeats):
    timed(host, dev), timed(device, dev)                    # warm-up of either way
    host_t, dev_t = [], []
    for _ in range(repeats):
        host_t.append(timed(host, dev)[1])
        dev_t.append(timed(device, dev)[1])
    return host_t, dev_t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=1 << 20)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--batch-size', type=int, default=8192)
    ap.add_argument('--seed', type=int, default=9527)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'prep_fit.jsonl'))
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error('--repeats: a median of at least 5 calls')

    import __graft_entry__ as ge
    ge.build()
    import torch
    assert torch.cuda.is_available(), 'this benchmark measures the GPU paths'
    from deeptables_amd import functional, training
    from deeptables_amd.models import DeepTable, ModelConfig, deepnets, preprocessor as P
    dev = torch.device('cuda', 0)
    df, y = make_frame(args.rows, args.seed)
    cats = [f'C{i + 1}' for i in range(F_CAT)]
    conf = ModelConfig(categorical_columns=cats)
    pp_host, pp_dev = P.DefaultPreprocessor(conf), P.DefaultPreprocessor(conf)

    def host():
        Xt, yt = pp_host.fit_transform(df, y)
        return training.TableBatches(Xt, yt, pp_host.categorical_columns, pp_host.continuous_columns, dev, pp_host.task_,
                                     len(pp_host.labels_), var_len_categorical_columns=pp_host.var_len_categorical_columns,
                                     resident=True)

    def device():
        return pp_dev.fit_feed(df, y, device=dev, mode=True)

    host_t, dev_t = alternate(host, device, dev, args.repeats)
    want, got = host(), device()
    blocks_equal = [bool(torch.equal(a, b)) for a, b in zip(want.blocks, got.blocks)]
    equal_but_means = {k: getattr(pp_host.X_transformers[s], k) == getattr(pp_dev.X_transformers[s], k)
                       for s, k in (('label_encoder', 'maps_'), ('standard_scale', 'min_'))
                       if s in pp_host.X_transformers}
    del want, got
    splits = []
    for _ in range(args.repeats):
        P.TIMINGS = {}
        total = timed(device, dev)[1]
        phases, P.TIMINGS = P.TIMINGS, None
        splits.append({'uploads': phases.get('fit_upload', 0.0) + phases.get('upload', 0.0),
                       'launches': phases.get('fit_kernel', 0.0) + phases.get('kernel', 0.0),
                       'host_work': total - sum(phases.values()) + phases.get('host_columns', 0.0)})
    split = {k: round(statistics.median(s[k] for s in splits) * 1e3, 2) for k in ('uploads', 'launches', 'host_work')}

    def table(path):
        def run():
            functional.set_seed(args.seed)
            dt = DeepTable(ModelConfig(nets=deepnets.DeepFM, categorical_columns=cats, metrics=['AUC'], fixed_embedding_dim=True,
                                       embeddings_output_dim=16, embedding_dropout=0, earlystopping_patience=0))
            return getattr(dt, path)(df, y, batch_size=args.batch_size, epochs=1, verbose=0)[1].history
        return run

    fit_t, feed_t = alternate(table('fit'), table('fit_feed'), dev, args.repeats)
    line = {'bench': 'prep_fit', 'rows': len(df), 'layout': f'{F_CAT} int64 categorical + {N_CONT} float32 continuous',
            'source_hash': ge.source_hash(), 'gpu': torch.cuda.get_device_name(dev),
            'sort_passes_per_column': sorted(set(pp_dev.last_profile_passes)),
            'host_fit_transform_plus_feed_ms': stats(host_t), 'fit_feed_ms': stats(dev_t), 'fit_feed_split_ms': split,
            'host_over_device': round(statistics.median(host_t) / statistics.median(dev_t), 2),
            'deeptable_fit_ms': stats(fit_t), 'deeptable_fit_feed_ms': stats(feed_t),
            'deeptable_fit_over_fit_feed': round(statistics.median(fit_t) / statistics.median(feed_t), 2),
            'batch_size': args.batch_size, 'feed_blocks_bit_identical': blocks_equal, 'attributes_equal': equal_but_means}
    text = json.dumps(line)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
