# -*- coding:utf-8 -*-
"""Times the way from a raw frame to a resident feed both ways on one fitted preprocessor (GPU, not a test): (i) the host
yardstick `TableBatches(pp.transform_X(X), ..., resident=True)` — pandas step by step, `.values`, `astype`, upload, unchanged
from before `transform_feed` existed — and (ii) `pp.transform_feed(X, ...)`: every numeric column uploaded as it is, one
dt_prep_transform launch per block (csrc/prep_transform.hip), columns the kernel cannot serve through the fitted host steps
alone.  The same frame and fitted preprocessor; each way is warmed up with one call, then the two are alternated `--repeats`
times; a host clock with the device drained at both ends; the medians are reported with their min and max.  The device call is
split with `preprocessor.TIMINGS` (which drains the device around every phase, so the split is taken in calls of its own):
upload of the raw columns, host-served columns (their pandas steps and uploads), kernel launches (descriptor packing and upload
included), and the remainder (frame handling, y).  Both feeds are compared bit by bit once.

Two frames of the benchmark's column layout (tools/cross_validation_bench.make_frame: 26 int64 categoricals, 13 float32
continuous columns): as it is — every column numeric, nothing host-served — and with `--string-columns` (4) of the categoricals
turned into strings, which shows what the per-column fallback costs.  Appends ONE JSON line per frame to
profiles/device_transform.jsonl (and prints it).

    python tools/transform_bench.py                        # 1,048,576 rows
    python tools/transform_bench.py --rows 65536 --repeats 7"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.cross_validation_bench import F_CAT, N_CONT, make_frame      # noqa: E402


def timed(fn, dev):
    import torch
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return out, time.perf_counter() - t0


def stats(xs):
    return {'median': round(statistics.median(xs) * 1e3, 2), 'min': round(min(xs) * 1e3, 2), 'max': round(max(xs) * 1e3, 2),
            'n': len(xs)}


def same_bits(a, b):
    import torch
    view = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t
    return a.kinds == b.kinds and all(torch.equal(view(x), view(y)) for x, y in zip(a.blocks + [a.y], b.blocks + [b.y]))


def measure(name, df, y, args, dev, source_hash):
    import torch
    from deeptables_amd import training
    from deeptables_amd.models import ModelConfig, preprocessor as P
    conf = ModelConfig(categorical_columns=[f'C{i + 1}' for i in range(F_CAT)])
    pp = P.DefaultPreprocessor(conf)
    _, fit_s = timed(lambda: pp.fit_transform(df, y), dev)
    num_classes = len(pp.labels_)

    def host():
        return training.TableBatches(pp.transform_X(df), pp.transform_y(y), pp.categorical_columns, pp.continuous_columns, dev,
                                     pp.task_, num_classes, var_len_categorical_columns=pp.var_len_categorical_columns,
                                     resident=True)

    def device():
        return pp.transform_feed(df, y, device=dev, mode=True)

    _, plan_s = timed(pp.device_plan, dev)
    want, _ = timed(host, dev)                      # warm-up of either way; the feeds compared once
    got, _ = timed(device, dev)
    equal = same_bits(got, want)
    host_columns = list(got.host_columns)
    del want, got
    host_t, dev_t = [], []
    for _ in range(args.repeats):
        host_t.append(timed(host, dev)[1])
        dev_t.append(timed(device, dev)[1])
    splits = []
    for _ in range(args.repeats):
        P.TIMINGS = {}
        total = timed(device, dev)[1]
        phases, P.TIMINGS = P.TIMINGS, None
        phases['remainder'] = total - sum(phases.values())
        splits.append(phases)
    split = {k: round(statistics.median(s.get(k, 0.0) for s in splits) * 1e3, 2) for k in ('upload', 'host_columns', 'kernel',
                                                                                           'remainder')}
    raw_bytes = int(sum(df[c].values.nbytes for c in df.columns if c not in host_columns))
    feed_bytes = len(df) * 4 * (F_CAT + N_CONT)
    line = {'bench': 'device_transform', 'frame': name, 'rows': len(df), 'layout': f'{F_CAT} categorical + {N_CONT} continuous',
            'source_hash': source_hash, 'gpu': torch.cuda.get_device_name(dev), 'host_columns': host_columns,
            'fit_transform_s_once': round(fit_s, 3), 'plan_ms_once': round(plan_s * 1e3, 2),
            'host_ms': stats(host_t), 'device_ms': stats(dev_t), 'device_split_ms': split,
            'host_over_device': round(statistics.median(host_t) / statistics.median(dev_t), 1),
            'raw_bytes_uploaded': raw_bytes, 'feed_bytes_written': feed_bytes,
            'upload_GB_per_s': round(raw_bytes / max(split['upload'], 1e-9) / 1e6, 2),
            'kernel_GB_per_s_read_plus_written': round((raw_bytes + feed_bytes) / max(split['kernel'], 1e-9) / 1e6, 1),
            'feeds_bit_identical': bool(equal)}
    text = json.dumps(line)
    print(text, flush=True)
    with open(args.out, 'a') as f:
        f.write(text + '\n')
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=1 << 20)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--string-columns', type=int, default=4)
    ap.add_argument('--seed', type=int, default=9527)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'device_transform.jsonl'))
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error('--repeats: a median of at least 5 calls')

    import __graft_entry__ as ge
    ge.build()
    import torch
    assert torch.cuda.is_available(), 'this benchmark measures the GPU paths'
    dev = torch.device('cuda', 0)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    df, y = make_frame(args.rows, args.seed)
    measure('numeric', df, y, args, dev, ge.source_hash())
    if args.string_columns > 0:
        df = df.copy()
        for i in range(args.string_columns):
            c = f'C{i + 1}'
            df[c] = 'v' + df[c].astype(str)
        measure(f'{args.string_columns} string columns', df, y, args, dev, ge.source_hash())


if __name__ == '__main__':
    main()
