# -*- coding:utf-8 -*-
"""Times an epoch's AUC on resident outputs both ways (GPU, not a test): (i) the host path — copy scores and labels to the
host, `metrics.compute_metric('AUC', ...)` = sklearn.metrics.roc_auc_score — and (ii) `metrics.compute_metrics_device`,
which ends in its small device-to-host read.  Seeded scores and labels, 3 % positives; both paths are warmed up, then
alternated; a host clock around work that ends in a synchronise.  Prints ONE JSON line (profiles/metrics_bench.jsonl).

    python tools/metrics_bench.py                      # n = 8192 * 1024
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/metrics_bench.py --paths device --repeats 3
    python tools/metrics_bench.py --stats-csv <dir>/.../*_kernel_stats.csv     # adds the sort's bytes over its kernel time
    python tools/metrics_bench.py --bench scores       # log loss, precision / recall, average precision: one line per leg

`--bench scores` times the metric names csrc/metrics.hip serves beyond AUC against what a user had before them: a callable
metric wrapping sklearn.metrics.log_loss / precision_score / average_precision_score, which `metrics.epoch_metrics` sends to
the host path, copies included.  The same data, the same protocol, one JSON line per leg.

The yardstick is the project's own step: the DeepFM step trains 8192 rows in 95.7 us, these rows in 98 ms."""
import argparse
import csv
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STEP_US, STEP_ROWS = 95.7, 8192


def sort_bytes(n, tile):
    """bytes the radix sort asks of memory for n pairs: per pass the histogram reads the keys, the scatter reads and writes
    keys and values and reads the keys once more for its per-wave counts; the counts table is written, scanned and read"""
    tiles = -(-n // tile)
    per_pass = 4 * n + (4 * n + 8 * n + 8 * n) + 4 * 256 * tiles * 4
    return 4 * per_pass


# --bench scores: (leg, the names the device serves, the callable a user wrote before that, or None for a device-only leg)
def score_legs():
    from sklearn.metrics import average_precision_score, log_loss, precision_score

    def sk_log_loss(y_true, y_prob):
        return log_loss(y_true.reshape(-1), y_prob.reshape(-1).astype('float64'))

    def sk_precision(y_true, y_prob):
        return precision_score(y_true.reshape(-1), y_prob.reshape(-1) > 0.5, zero_division=0)

    def sk_average_precision(y_true, y_prob):
        return average_precision_score(y_true.reshape(-1), y_prob.reshape(-1))

    return [('logloss', ['binary_crossentropy'], sk_log_loss),
            ('precision_recall', ['Precision', 'Recall'], sk_precision),
            ('average_precision', ['average_precision'], sk_average_precision),
            ('ctr_set', ['AUC', 'average_precision', 'binary_crossentropy', 'Precision', 'Recall'], None)]


def bench_scores(args, base, label, score):
    """one JSON line per leg: the device call against the callable on the host path, warmed up, alternated, a host clock around
    work that ends in a synchronise (the host path ends in numpy, the device path in its read)"""
    import torch
    from deeptables_amd import metrics
    for leg, names, fn in score_legs():
        run = {'device': lambda: metrics.compute_metrics_device(names, label, score, 'binary')}
        if fn is not None and 'host' in args.paths.split(','):
            run['host'] = lambda: metrics.epoch_metrics([fn], label, score, 'binary')
        times, values = {p: [] for p in run}, {}
        for p in run:
            for _ in range(args.warmup):
                values[p] = run[p]()
        torch.cuda.synchronize()
        for _ in range(args.repeats):
            for p in run:                     # alternated
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                values[p] = run[p]()
                torch.cuda.synchronize()
                times[p].append((time.perf_counter() - t0) * 1e3)
        res = dict(base, bench='metrics_scores', leg=leg, metrics=names)
        for p in run:
            res[f'{p}_ms'] = round(statistics.median(times[p]), 3)
            res[f'{p}_ms_all'] = [round(t, 3) for t in times[p]]
            res[f'{p}_values'] = values[p]
        if 'host' in run:
            res['host_callable'] = fn.__name__
            res['host_over_device'] = round(res['host_ms'] / res['device_ms'], 1)
            res['difference'] = abs(values['host'][fn.__name__] - values['device'][names[0]])
        res['device_over_yardstick'] = round(res['device_ms'] / res['yardstick_ms'], 4)
        print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bench', default='auc', choices=['auc', 'scores'])
    ap.add_argument('--rows', type=int, default=8192 * 1024)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--paths', default='host,device')
    ap.add_argument('--stats-csv', default=None, help='rocprofv3 --kernel-trace --stats kernel_stats.csv of a --paths device run')
    ap.add_argument('--stats-calls', type=int, default=None, help='compute_metrics_device calls in that run (warmup + repeats)')
    args = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as g
    from deeptables_amd import _lib, metrics
    tile = _lib.lib().dt_metric_sort_tile()
    n = args.rows
    res = {'bench': 'metrics_auc', 'rows': n, 'positives': 0.03, 'source_hash': g.source_hash(), 'sort_tile': tile,
           'sort_bytes': sort_bytes(n, tile), 'yardstick_ms': round(n / STEP_ROWS * STEP_US / 1e3, 2),
           'yardstick': f'{n // STEP_ROWS} DeepFM steps of {STEP_US} us'}
    if args.stats_csv:
        rows = list(csv.DictReader(open(args.stats_csv)))
        calls = args.stats_calls or (args.warmup + args.repeats)
        mine = re.compile(r'\b(k_(?:sort|auc|sums|argmax|score|ap)_[a-z0-9_]+)')
        per = {mine.search(r['Name']).group(1): float(r['TotalDurationNs']) / calls / 1e6 for r in rows if mine.search(r['Name'])}
        sort_ms = sum(v for k, v in per.items() if k.startswith('k_sort_'))
        res.update(kernel_ms_per_call={k: round(v, 4) for k, v in sorted(per.items())}, kernel_ms=round(sum(per.values()), 4),
                   sort_kernel_ms=round(sort_ms, 4),
                   sort_gbytes_per_s=round(res['sort_bytes'] / sort_ms / 1e6, 1) if sort_ms else None)
        print(json.dumps(res))
        return
    if not torch.cuda.is_available():
        raise SystemExit('tools/metrics_bench.py measures on the GPU; there is none here')
    dev = torch.device('cuda', 0)
    gen = torch.Generator(device=dev).manual_seed(20)
    label = (torch.rand(n, device=dev, generator=gen) < 0.03).float()
    score = torch.sigmoid(torch.randn(n, device=dev, generator=gen) + 0.8 * label - 2).reshape(n, 1).contiguous()
    paths = args.paths.split(',')
    if args.bench == 'scores':
        del res['sort_bytes']
        return bench_scores(args, res, label, score)

    def host():
        yp, yt = score.cpu().numpy(), label.cpu().numpy()
        return metrics.compute_metric('AUC', yt, yp, 'binary')

    def device():
        return metrics.compute_metrics_device(['AUC'], label, score, 'binary')['AUC']

    run = {'host': host, 'device': device}
    times, values = {p: [] for p in paths}, {}
    for p in paths:
        for _ in range(args.warmup):
            values[p] = run[p]()
    torch.cuda.synchronize()
    for _ in range(args.repeats):
        for p in paths:                       # alternated
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            values[p] = run[p]()
            torch.cuda.synchronize()
            times[p].append((time.perf_counter() - t0) * 1e3)
    for p in paths:
        res[f'{p}_ms'] = round(statistics.median(times[p]), 3)
        res[f'{p}_ms_all'] = [round(t, 3) for t in times[p]]
        res[f'{p}_auc'] = values[p]
    if 'host' in paths and 'device' in paths:
        res['host_over_device'] = round(res['host_ms'] / res['device_ms'], 1)
        res['auc_difference'] = abs(values['host'] - values['device'])
    if 'device' in paths:
        res['device_over_yardstick'] = round(res['device_ms'] / res['yardstick_ms'], 4)
        res['workspace_bytes'] = int(_lib.lib().dt_metric_auc_workspace_bytes(n))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
