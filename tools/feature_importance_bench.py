# -*- coding:utf-8 -*-
"""Times permutation feature importance both ways on one fitted DeepFM (GPU, not a test): (i) the loop a user could write
before utils/feature_importance.py — per pass copy the frame, permute the raw column, `preprocessor.transform_X`,
`DeepModel.predict`, `metrics.compute_metric` — and (ii) the device path (`permutation_scores(device=True)`): the frame
transformed once into a resident feed, per pass a column gather + swap (csrc/feed_columns.hip), one fused inference launch per
batch, the metric kernels and their small read.  The same model, rows, seed and permutations; each path is warmed up with one
pass, then the two are alternated; a host clock around work that ends in a synchronise.  The benchmark's DeepFM column layout
(26 categorical + 13 continuous columns, embedding width 16), metric 'auc', n_iter 5.  Appends ONE JSON line per configuration
to profiles/feature_importance.jsonl (and prints it).

    python tools/feature_importance_bench.py                           # 1,048,576 rows, columns C1 and I1
    python tools/feature_importance_bench.py --rows 65536 --columns C1,C2,I1,I2

The hand-written loop costs seconds per pass at this size, so it is timed on the `--columns` only (two by default: one
categorical, one continuous; 11 passes); its time per pass does not depend on which column is permuted.  The device path is
timed on the same columns and, on its own, over all 39 (196 passes)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

F_CAT, N_CONT, D, VOCAB = 26, 13, 16, 1000


def make_frame(rows, seed):
    import numpy as np
    import pandas as pd
    rng = np.random.default_rng(seed)
    cols = {f'C{i + 1}': rng.integers(0, VOCAB, rows) for i in range(F_CAT)}
    cols.update({f'I{j + 1}': rng.normal(size=rows).astype(np.float32) for j in range(N_CONT)})
    df = pd.DataFrame(cols)
    z = (df['C1'].values % 7 - 3) * 0.4 + df['I1'].values + 0.5 * df['I2'].values + rng.normal(size=rows) * 0.5
    return df, (z > 1.0).astype(np.int64)


def hand_loop(dt, df, y, metric, n_iter, columns, seed, batch_size):
    """-> (base_score, decreases, seconds of every pass): mode 'max', one torch.randperm per (iteration, column) from a
    generator on the model's device, as the new module draws them"""
    import numpy as np
    import torch
    from deeptables_amd import metrics
    pp, dm = dt.preprocessor, dt.model
    y_enc = pp.transform_y(y)
    g = torch.Generator(device=dm.device).manual_seed(seed)
    times = []

    def score(frame):
        t0 = time.perf_counter()
        out = dm.predict(pp.transform_X(frame), batch_size=batch_size)
        v = metrics.compute_metric(metric, y_enc, out, dm.task)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        return v

    base = score(df)
    dec = np.zeros((n_iter, len(columns)))
    for i in range(n_iter):
        for c, name in enumerate(columns):
            t0 = time.perf_counter()
            perm = torch.randperm(len(df), generator=g, device=dm.device).cpu().numpy()
            frame = df.copy()
            frame[name] = df[name].values[perm]
            lead = time.perf_counter() - t0
            dec[i, c] = base - score(frame)
            times[-1] += lead
    return base, dec, times


def device_run(dt, df, y, metric, n_iter, columns, seed, batch_size):
    import torch
    from deeptables_amd.utils import feature_importance as FI
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = FI.permutation_scores(dt, df, y, metric, n_iter=n_iter, mode='max', random_state=seed, batch_size=batch_size,
                                columns=columns, device=True)
    torch.cuda.synchronize()
    return res, time.perf_counter() - t0


def device_split(dt, df, y, metric, columns, seed, batch_size, passes):
    """the device path's pass taken apart with a synchronise after each part -> ms per pass of (permute + restore, score,
    metric), and of building the feed once"""
    import torch
    from deeptables_amd import metrics, ops
    from deeptables_amd.utils import feature_importance as FI
    dm = dt.model
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    feed = FI.make_feed(dt, df, dt.preprocessor.transform_y(y))
    torch.cuda.synchronize()
    build = time.perf_counter() - t0
    smap = dt.preprocessor.source_columns()
    g = FI._generator(dm.device, seed)
    acc = {'permute': 0.0, 'score': 0.0, 'metric': 0.0}
    for k in range(passes + 1):                                  # (the first pass warms up and is not counted)
        name = columns[k % len(columns)]
        tg = FI.feed_targets(dm, feed, smap, [name])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        perm = FI._draw(feed.n, g)
        done = [ops.permute_columns(feed.blocks[b], cols, perm) for b, cols in tg.items()]
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        out = dm.score_batches(feed, batch_size)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        metrics.epoch_metrics([metric], feed.y, out, dm.task)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        for h in done:
            h.restore()
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        if k:
            acc['permute'] += (t1 - t0) + (t4 - t3)
            acc['score'] += t2 - t1
            acc['metric'] += t3 - t2
    return {k: round(1e3 * v / passes, 3) for k, v in acc.items()}, round(1e3 * build, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=1 << 20)
    ap.add_argument('--columns', default='C1,I1')
    ap.add_argument('--n-iter', type=int, default=5)
    ap.add_argument('--metric', default='auc')
    ap.add_argument('--batch-size', type=int, default=8192)
    ap.add_argument('--train-steps', type=int, default=30)
    ap.add_argument('--seed', type=int, default=7)
    ap.add_argument('--skip-all-columns', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'feature_importance.jsonl'))
    args = ap.parse_args()

    import __graft_entry__ as ge
    ge.build()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), 'this benchmark measures the GPU paths'
    from deeptables_amd import functional
    from deeptables_amd.models import DeepTable, ModelConfig, deepnets
    columns = args.columns.split(',')
    df, y = make_frame(args.rows, args.seed)
    functional.set_seed(args.seed)
    conf = ModelConfig(nets=deepnets.DeepFM, categorical_columns=[f'C{i + 1}' for i in range(F_CAT)], metrics=['AUC'],
                       fixed_embedding_dim=True, embeddings_output_dim=D, embedding_dropout=0, earlystopping_patience=0)
    dt = DeepTable(config=conf)
    dt.fit(df, y, batch_size=args.batch_size, epochs=1, steps_per_epoch=args.train_steps, validation_split=0, verbose=0)
    assert dt.model.inference_plan() is not None, 'the DeepFM graph should take its inference plan'
    bs, m = args.batch_size, args.metric

    # warm-up: one pass per path and shape
    hand_loop(dt, df, y, m, 1, columns[:1], args.seed, bs)
    device_run(dt, df, y, m, 1, columns[:1], args.seed, bs)
    # alternate: loop, device, device (a second device run shows its spread; a second loop run would double the job)
    hb, hd, h_times = hand_loop(dt, df, y, m, args.n_iter, columns, args.seed, bs)
    res, d_s = device_run(dt, df, y, m, args.n_iter, columns, args.seed, bs)
    res2, d_s2 = device_run(dt, df, y, m, args.n_iter, columns, args.seed, bs)
    passes = 1 + args.n_iter * len(columns)
    split, build_ms = device_split(dt, df, y, m, columns, args.seed, bs, passes=10)
    line = {'bench': 'feature_importance', 'rows': args.rows, 'layout': f'{F_CAT} categorical + {N_CONT} continuous, D {D}',
            'nets': 'DeepFM', 'metric': m, 'n_iter': args.n_iter, 'columns': columns, 'passes': passes, 'batch_size': bs,
            'source_hash': ge.source_hash(), 'path': res['path'],
            'loop_s': round(sum(h_times), 3), 'loop_ms_per_pass': round(1e3 * sum(h_times) / len(h_times), 1),
            'loop_ms_per_pass_min_max': [round(1e3 * min(h_times), 1), round(1e3 * max(h_times), 1)],
            'device_s': round(d_s, 3), 'device_s_again': round(d_s2, 3),
            'device_ms_per_pass_with_feed_build': round(1e3 * d_s / passes, 2),
            'device_feed_build_ms': build_ms, 'device_pass_split_ms': split,
            'loop_over_device': round(sum(h_times) / d_s, 1),
            'loop_pass_over_device_pass': round((sum(h_times) / len(h_times)) / (1e-3 * sum(split.values())), 1),
            'base_score': {'loop': hb, 'device': res['base_score']},
            'max_decrease_difference': float(np.abs(res['score_decreases'] - hd).max()),
            'max_abs_decrease': float(np.abs(hd).max()),
            'device_runs_equal': bool(np.array_equal(res['score_decreases'], res2['score_decreases']))}
    if not args.skip_all_columns:
        every = df.columns.to_list()
        res_all, d_all = device_run(dt, df, y, m, args.n_iter, every, args.seed, bs)
        line['device_all_columns'] = {'columns': len(every), 'passes': 1 + args.n_iter * len(every), 's': round(d_all, 3),
                                      'ms_per_pass_with_feed_build': round(1e3 * d_all / (1 + args.n_iter * len(every)), 2),
                                      'loop_s_at_its_ms_per_pass': round((1 + args.n_iter * len(every)) * sum(h_times) / len(h_times), 1)}
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'a') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
