# -*- coding:utf-8 -*-
"""Times loss + backward of a train step's loss on resident logits both ways (GPU, not a test): through csrc/loss.hip
(losses.device_loss: at most two launches, backward hands out the saved dz) and through the torch op chains that
DT_AMD_DEVICE_LOSS=0 restores (the code of the commit before the kernels), at B = 8192 and C = 1, 10, 100 over the kinds that
apply to each C, with and without per-row weights.  The unweighted binary cross-entropy is not a row: it keeps its own
one-launch kernel (dt_bce_logits) on both legs.  `--set reg` times csrc/loss_reg.hip instead: Keras' regression losses
(losses.named_loss -> dt_loss_reg) and GHMCLoss.calc (dt_ghmc) at [8192, 1] and [8192, 16], each against its torch
chain under DT_AMD_DEVICE_LOSS=0 — for GHM-C that chain is the `calc` of the commit before the kernel.

    python tools/loss_bench.py --out profiles/losses.jsonl
    python tools/loss_bench.py --set reg --out profiles/losses_reg.jsonl
    rocprofv3 --kernel-trace --output-format csv -d <dir> -o kernel -- python tools/loss_bench.py --count kernel
    rocprofv3 --kernel-trace --output-format csv -d <dir> -o torch  -- python tools/loss_bench.py --count torch
    python tools/loss_bench.py --trace kernel=<dir>/.../kernel_kernel_trace.csv --trace torch=<...> --out profiles/losses.jsonl

Method: one process; logits, targets and weights are device resident; the call is what DeepModel._forward_backward does
with the logits — the loss function, then `loss.backward(losses.unit_grad)` into a leaf whose .grad was dropped.  Both paths
are warmed up, then alternated window by window: `--repeats` windows of `--calls` calls per path, each window between two
device events (the second one synchronised); a window's time per call is its time / calls; the median of the windows is
reported with min and max.  These are CALL times, host enqueue included — at these sizes the host is the slower side on
both paths, and what the kernels remove is launches.  The launch count of a path comes from a kernel trace in a run of its
own (--count: every row `--calls` times on one path, a marker kernel between rows; --trace splits the trace at the markers).
Prints one JSON line per row and appends it to --out."""
import argparse
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BATCH = 8192
ROWS = [('bce', 1, True), ('mse', 1, False), ('mse', 1, True), ('mae', 1, False), ('binary_focal', 1, False)] + \
    [r for C in (10, 100) for r in (('bce', C, True), ('cce', C, False), ('cce', C, True), ('mse', C, False), ('mae', C, False),
                                    ('binary_focal', C, False), ('categorical_focal', C, False),
                                    ('categorical_focal', C, True))]
REG_KINDS = ('huber', 'log_cosh', 'msle', 'mape', 'poisson')
ROWS_REG = [(k, C, False) for C in (1, 16) for k in REG_KINDS + ('ghmc',)] + [('huber', 1, True), ('huber', 16, True)]
NAMES = {'bce': 'binary_crossentropy', 'cce': 'categorical_crossentropy', 'mse': 'mse', 'mae': 'mae'}
MARKER = 'k_sgd_dense'          # a kernel no loss path launches: dt_sgd_dense_step on a scratch tensor separates the rows


def row_id(kind, C, weighted):
    return f'{kind}/C{C}/{"weighted" if weighted else "unweighted"}'


def make_case(kind, C, weighted, dev):
    """(leaf logits, fn(z) -> loss) on seeded data: one-hot targets for the categorical kinds, 0 / 1 for the binary ones"""
    import torch
    from deeptables_amd import _lib, losses
    from deeptables_amd.models.layers import BinaryFocalLoss, CategoricalFocalLoss
    g = torch.Generator().manual_seed(100 * C + len(kind))
    if kind in REG_KINDS:
        # predictions and targets in [0.05, 5]: inside the domain of every kind (MSLE, Poisson), off MAPE's |t| = 0
        z = (torch.rand(BATCH, C, generator=g) * 4.95 + 0.05).to(dev).requires_grad_(True)
        y = (torch.rand(BATCH, C, generator=g) * 4.95 + 0.05).to(dev)
        w = (torch.rand(BATCH, generator=g) + 0.5).to(dev) if weighted else None
        return z, lambda zz: losses.named_loss(kind, zz, y, w)
    z = torch.randn(BATCH, C, generator=g).to(dev).requires_grad_(True)
    if kind == 'ghmc':
        # one object per path, so that both see the same sequence of calls and carry the same acc_sum
        from deeptables_amd.models.layers import GHMCLoss
        y = (torch.rand(BATCH, C, generator=g) < 0.25).float().to(dev)
        objs = {'1': GHMCLoss(bins=10, momentum=0.75), '0': GHMCLoss(bins=10, momentum=0.75)}
        return z, lambda zz: objs[os.environ['DT_AMD_DEVICE_LOSS']].calc(zz, y)
    if kind in ('bce', 'binary_focal'):
        y = (torch.rand(BATCH, C, generator=g) < 0.25).float().to(dev)
    elif kind in ('mse', 'mae'):
        y = torch.randn(BATCH, C, generator=g).to(dev)
    else:
        y = torch.eye(C)[torch.randint(0, C, (BATCH,), generator=g)].to(dev)
    w = (torch.rand(BATCH, generator=g) + 0.5).to(dev) if weighted else None
    if kind == 'binary_focal':
        obj = BinaryFocalLoss()
        return z, lambda zz: losses.focal_from_logits(_lib.DT_LOSS_BINARY_FOCAL, obj, zz, y, None, torch.sigmoid)
    if kind == 'categorical_focal':
        obj = CategoricalFocalLoss()
        return z, lambda zz: losses.focal_from_logits(_lib.DT_LOSS_CATEGORICAL_FOCAL, obj, zz, y, w,
                                                      lambda t: torch.softmax(t, dim=-1))
    return z, lambda zz: losses.named_loss(NAMES[kind], zz, y, w)


def set_path(path):
    os.environ['DT_AMD_DEVICE_LOSS'] = '1' if path == 'kernel' else '0'


def one_call(z, fn, unit):
    z.grad = None
    loss = fn(z)
    loss.backward(unit)
    return loss


def split_trace(path, calls, rows=ROWS):
    """launches per call of every row from a --count run's kernel trace: dispatches in start order, split at the markers"""
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r['Start_Timestamp']))
    segments, names = [0], [{}]
    for r in rows:
        if MARKER in r['Kernel_Name']:
            segments.append(0)
            names.append({})
        else:
            segments[-1] += 1
            short = r['Kernel_Name'].split('(')[0][-60:]
            names[-1][short] = names[-1].get(short, 0) + 1
    body = segments[1:1 + len(rows)]             # segment 0: set-up and the warm pass
    if len(body) != len(rows):
        raise SystemExit(f'{path}: {len(segments)} segments for {len(rows)} rows')
    return {row_id(*row): {'launches_per_call': n / calls, 'kernels': len(k)} for row, n, k in zip(rows, body, names[1:])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=24)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--count', choices=['kernel', 'torch'], default=None)
    ap.add_argument('--trace', action='append', default=[], help='kernel=<kernel_trace.csv> / torch=<kernel_trace.csv>')
    ap.add_argument('--out', default=None)
    ap.add_argument('--set', choices=['train', 'reg'], default='train', help="reg: the rows of csrc/loss_reg.hip")
    a = ap.parse_args()
    rows = ROWS_REG if a.set == 'reg' else ROWS
    traces = {}
    for spec in a.trace:
        path, _, file = spec.partition('=')
        traces[path] = split_trace(file, a.calls, rows)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('loss_bench needs the GPU: nothing is measured without one')
    import __graft_entry__ as g
    from deeptables_amd import losses
    from deeptables_amd._lib import check, lib, ptr, stream_ptr
    dev = torch.device('cuda', 0)
    unit = losses.unit_grad(dev)
    cases = [(row, make_case(*row, dev)) for row in rows]
    if a.count:
        scratch = torch.zeros(64, device=dev)
        set_path(a.count)
        for _, (z, fn) in cases:                  # warm pass: code objects, lazy state
            one_call(z, fn, unit)
        for _, (z, fn) in cases:
            check(lib().dt_sgd_dense_step(ptr(scratch), ptr(scratch), 64, 0.0, stream_ptr()), 'marker')
            for _ in range(a.calls):
                one_call(z, fn, unit)
        check(lib().dt_sgd_dense_step(ptr(scratch), ptr(scratch), 64, 0.0, stream_ptr()), 'marker')
        torch.cuda.synchronize()
        print(json.dumps({'tool': 'loss_bench', 'count': a.count, 'rows': len(rows), 'calls': a.calls}))
        return
    if a.repeats * a.calls < 200:
        raise SystemExit('--repeats x --calls: at least 200 timed calls per path')
    lines = []
    for row, (z, fn) in cases:
        kind, C, weighted = row
        res = {'tool': 'loss_bench', 'row': row_id(*row), 'kind': kind, 'batch': BATCH, 'classes': C, 'weighted': weighted,
               'source_hash': g.source_hash(), 'repeats': a.repeats, 'calls_per_window': a.calls, 'warmup': a.warmup,
               # the commit before the kernels has no torch path for these rows at all: they raised
               'parent_runs_this_row': not (kind == 'mae' or (kind == 'categorical_focal' and weighted))
               if a.set == 'train' else kind == 'ghmc'}
        value, us = {}, {'kernel': [], 'torch': []}
        for path in ('kernel', 'torch'):
            set_path(path)
            for _ in range(a.warmup):
                one_call(z, fn, unit)
            value[path] = float(one_call(z, fn, unit).detach())
            value[path + '_grad'] = z.grad.detach().clone()
        torch.cuda.synchronize()
        for _ in range(a.repeats):
            for path in ('kernel', 'torch'):
                set_path(path)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.calls):
                    one_call(z, fn, unit)
                e1.record()
                e1.synchronize()
                us[path].append(e0.elapsed_time(e1) * 1e3 / a.calls)
        for path in ('kernel', 'torch'):
            res[path] = {'us_median': statistics.median(us[path]), 'us_min': min(us[path]), 'us_max': max(us[path])}
            if path in traces:
                res[path].update(traces[path][row_id(*row)])
        gk, gt = value['kernel_grad'], value['torch_grad']
        res['loss_kernel'], res['loss_torch'] = value['kernel'], value['torch']
        res['grad_max_abs_diff_over_max'] = float((gk - gt).abs().max() / gt.abs().max())
        res['kernel_over_torch'] = res['kernel']['us_median'] / res['torch']['us_median']
        line = json.dumps(res)
        print(line)
        lines.append(line)
    set_path('kernel')
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or '.', exist_ok=True)
        with open(a.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
