# -*- coding:utf-8 -*-
"""Times the layer-path train step of bench.py's DeepFM configuration (26 categorical fields, 13 continuous columns, D = 16,
the default 128 x 64 tower, batch 8192, Adam) with and without the Keras L1 / L2 regularizers, and the three regularizer
launches on their own.  DT_AMD_FUSED=0 forces the layer path; the vocabulary is cut to 10082 ids per field so that the
packed table (26 x 10082 x 16 = 4,194,112 floats) sits just under layers.DENSE_GRAD_MAX_ELEMS and keeps a dense gradient.

    --variant off     no regularizer anywhere
    --variant on      embeddings_regularizer='l2' and dnn_params['kernel_regularizer']='l2' (a tree that predates the feature
                      ignores both: that is the unregularised step of that tree)
    --variant torch   the same configuration, the penalty formed by a torch-op restatement (abs / sum / mul / square / sum /
                      mul / add per tensor and their autograd nodes) instead of ops.regularization_penalty: a switch of this
                      tool only, the library has no such path
    --tree PATH       import deeptables_amd from another checkout of the repository (the parent commit, built there)

Method: the batch is device resident; warm-up steps first; then `--repeats` windows of `--steps` train steps, each window
between two device events (the second one synchronised); the per-step time of a window is its time / steps; the median of
the windows is reported with min and max.  The device's clocks (rocm-smi --showclocks, a read-only query) are recorded
before and after.  One job on the card; prints ONE JSON line and appends it to --out (profiles/regularizers.jsonl).
With --kernels the penalty call (two launches) and the gradient call (one launch) are also timed on their own, on the model's
regularised tensors, and set against the bytes they move (penalty: 4 n read; gradient: 4 n read + 4 n written).  Those are
CALL times — host enqueue included, and at these sizes the host is the slower side; the kernels' own times come from a
`rocprofv3 --kernel-trace --stats -- python tools/regularizer_bench.py --variant on` run of its own (k_reg_partial,
k_reg_total, k_reg_grad in its kernel statistics)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

os.environ['DT_AMD_FUSED'] = '0'

F, VOCAB, ND, D, BATCH = 26, 10082, 13, 16, 8192


def clocks():
    try:
        out = subprocess.run(['rocm-smi', '--showclocks', '--json'], capture_output=True, timeout=30, text=True).stdout
        card = next(iter(json.loads(out).values()))
        return {k: v for k, v in card.items() if 'sclk' in k or 'mclk' in k or 'fclk' in k}
    except Exception as e:                      # the figures stand without them, the record says they are missing
        return {'unavailable': type(e).__name__}


def build(variant, seed=0):
    from deeptables_amd import functional
    from deeptables_amd.models import DeepModel, ModelConfig, deepnets
    from deeptables_amd.models.metainfo import CategoricalColumn, ContinuousColumn
    functional.set_seed(seed)
    dnn = {'hidden_units': ((128, 0, False), (64, 0, False)), 'activation': 'relu'}
    extra = {}
    if variant in ('on', 'torch'):
        dnn['kernel_regularizer'] = 'l2'
        extra['embeddings_regularizer'] = 'l2'
    conf = ModelConfig(nets=deepnets.DeepFM, fixed_embedding_dim=True, embeddings_output_dim=D, embedding_dropout=0,
                       metrics=[], dnn_params=dnn, **extra)
    cats = [CategoricalColumn(f'C{i}', VOCAB, D) for i in range(F)]
    conts = [ContinuousColumn('input_continuous_all', [f'I{j}' for j in range(ND)])]
    dm = DeepModel('binary', 2, conf, cats, conts)
    dm.build()
    dm.model.train()
    return dm


def torch_penalty(tensors, coeffs):
    total = None
    for t, (l1, l2) in zip(tensors, coeffs):
        for c, term in ((l1, lambda: t.abs().sum()), (l2, lambda: t.square().sum())):
            if c:
                p = term() * c
                total = p if total is None else total + p
    return total


def time_windows(fn, warmup, repeats, steps):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3 / steps)
    return {'us_median': statistics.median(us), 'us_min': min(us), 'us_max': max(us)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--variant', required=True, choices=['off', 'on', 'torch'])
    ap.add_argument('--tree', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument('--label', default=None)
    ap.add_argument('--repeats', type=int, default=24)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--kernels', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.repeats < 20:
        raise SystemExit('--repeats: at least 20 windows')
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('regularizer_bench needs the GPU: nothing is measured without one')
    from deeptables_amd import _lib, ops
    has_feature = hasattr(ops, 'regularization_penalty')
    if a.variant == 'torch':
        if not has_feature:
            raise SystemExit('--variant torch needs a tree with the regularizers')
        ops.regularization_penalty = torch_penalty
    before = clocks()
    dm = build(a.variant)
    dev = dm.device
    g = torch.Generator().manual_seed(1)
    idx = torch.randint(0, VOCAB, (BATCH, F), generator=g).int().to(dev)
    dense = torch.randn(BATCH, ND, generator=g).to(dev)
    y = (torch.rand(BATCH, 1, generator=g) < 0.25).float().to(dev)
    res = {'tool': 'regularizer_bench', 'label': a.label or a.variant, 'variant': a.variant,
           'source_hash': _lib.lib().dt_source_hash().decode(), 'has_regularizers': has_feature,
           'regularised': bool(has_feature and dm.model.has_regularizers()),
           'shape': {'fields': F, 'vocab': VOCAB, 'dense': ND, 'D': D, 'batch': BATCH, 'tower': [128, 64], 'optimizer': 'adam'},
           'fused_plan': type(dm.fused_plan()).__name__, 'repeats': a.repeats, 'steps_per_window': a.steps, 'warmup': a.warmup}
    res['train_step'] = time_windows(lambda: dm.train_step([idx, dense], y), a.warmup, a.repeats, a.steps)
    res['loss'] = float(dm.train_step([idx, dense], y)[0])
    if a.kernels and a.variant == 'on' and has_feature:
        terms = dm.model.weight_penalties()
        tensors, coeffs = [t.detach() for t, _ in terms], [c for _, c in terms]
        n = sum(t.numel() for t in tensors)
        go = torch.ones(1, device=dev)
        outs = [torch.empty_like(t) for t in tensors]
        fwd = time_windows(lambda: ops.reg_penalty_raw(tensors, coeffs), 10, a.repeats, 50)
        bwd = time_windows(lambda: ops.reg_grad_raw(tensors, outs, coeffs, go), 10, a.repeats, 50)
        res['kernels'] = {'tensors': len(tensors), 'elements': n,
                          'penalty_call_two_launches': {**fwd, 'bytes': 4 * n, 'GBps_at_median': 4 * n / fwd['us_median'] * 1e-3},
                          'gradient_call_one_launch': {**bwd, 'bytes': 8 * n, 'GBps_at_median': 8 * n / bwd['us_median'] * 1e-3}}
    res['clocks'] = {'before': before, 'after': clocks()}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or '.', exist_ok=True)
        with open(a.out, 'a') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
