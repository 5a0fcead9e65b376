# -*- coding:utf-8 -*-
"""Times the layer-path train step of an xDeepFM, an AutoInt and a ['dnn_nets'] graph at bench.py's shape (26 categorical
fields x 1,000,000 ids, D = 16, 13 continuous columns, batch 8192, Adam) with ModelConfig.embedding_dropout 0 and 0.3 (the
reference default), each with DT_AMD_EMB_DROPOUT=1 (the dropout inside the gather launch, csrc/emb_dropout.hip) and =0 (one
torch SpatialDropout1D chain per column).  None of the three graphs has a fused train plan: every step goes through
MultiColumnEmbedding.call.  On a tree that predates the feature the switch does nothing; that is the parent's figure.

    --tree PATH       import deeptables_amd from another checkout of the repository (the parent commit, built there)
    --graphs a,b      a subset of xdeepfm,autoint,dnn
    --rates / --switches   subsets of 0,0.3 and of 1,0 (one configuration alone, e.g. under a kernel trace)

Method: the batch is device resident; warm-up steps first; then `--repeats` windows of `--steps` train steps, each window
between two device events (the second one synchronised); the per-step time of a window is its time / steps; the median of the
windows is reported with min and max (the repeat spread).  One job on the card.  Prints ONE JSON line per (graph, rate,
switch) and appends it to --out (profiles/emb_dropout_bench.jsonl)."""
import argparse
import json
import os
import statistics
import sys

F, VOCAB, ND, D, BATCH = 26, 1_000_000, 13, 16, 8192


def build(graph, rate, vocab, seed=0):
    from deeptables_amd import functional
    from deeptables_amd.models import DeepModel, ModelConfig, deepnets
    from deeptables_amd.models.metainfo import CategoricalColumn, ContinuousColumn
    functional.set_seed(seed)
    nets = {'xdeepfm': deepnets.xDeepFM, 'autoint': deepnets.AutoInt, 'dnn': ['dnn_nets']}[graph]
    conf = ModelConfig(nets=nets, fixed_embedding_dim=True, embeddings_output_dim=D, embedding_dropout=rate, dense_dropout=0,
                       metrics=[])
    cats = [CategoricalColumn(f'C{i}', vocab, D) for i in range(F)]
    conts = [ContinuousColumn('input_continuous_all', [f'I{j}' for j in range(ND)])]
    dm = DeepModel('binary', 2, conf, cats, conts)
    dm.build()
    dm.model.train()
    return dm


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
    ap.add_argument('--tree', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument('--label', default='this')
    ap.add_argument('--graphs', default='xdeepfm,autoint,dnn')
    ap.add_argument('--rates', default='0,0.3')
    ap.add_argument('--switches', default='1,0')
    ap.add_argument('--vocab', type=int, default=VOCAB)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('emb_dropout_bench needs the GPU: nothing is measured without one')
    from deeptables_amd import _lib, ops
    has_feature = hasattr(ops, 'embedding_drop_fwd_launch')
    g = torch.Generator().manual_seed(1)
    idx_h = torch.randint(0, a.vocab, (BATCH, F), generator=g).int()
    dense_h = torch.randn(BATCH, ND, generator=g)
    y_h = (torch.rand(BATCH, 1, generator=g) < 0.25).float()
    for graph in a.graphs.split(','):
        for rate in [float(r) for r in a.rates.split(',')]:
            dm = build(graph, rate, a.vocab)
            dev = dm.device
            idx, dense, y = idx_h.to(dev), dense_h.to(dev), y_h.to(dev)
            for switch in a.switches.split(','):
                os.environ['DT_AMD_EMB_DROPOUT'] = switch                  # read at every call
                launches = []
                if has_feature:
                    real = ops.embedding_drop_fwd_launch
                    ops.embedding_drop_fwd_launch = lambda *p, **k: (launches.append(1), real(*p, **k))[1]
                loss = float(dm.train_step([idx, dense], y)[0])
                if has_feature:
                    ops.embedding_drop_fwd_launch = real
                res = {'tool': 'emb_dropout_bench', 'label': a.label, 'graph': graph, 'embedding_dropout': rate,
                       'DT_AMD_EMB_DROPOUT': int(switch), 'has_fused_emb_dropout': has_feature,
                       'fused_launches_per_step': len(launches), 'source_hash': _lib.lib().dt_source_hash().decode(),
                       'shape': {'fields': F, 'vocab': a.vocab, 'dense': ND, 'D': D, 'batch': BATCH, 'optimizer': 'adam'},
                       'fused_plan': type(dm.fused_plan()).__name__, 'repeats': a.repeats, 'steps_per_window': a.steps,
                       'warmup': a.warmup,
                       'train_step': time_windows(lambda: dm.train_step([idx, dense], y), a.warmup, a.repeats, a.steps),
                       'first_loss': loss}
                line = json.dumps(res)
                print(line, flush=True)
                if a.out:
                    os.makedirs(os.path.dirname(os.path.abspath(a.out)) or '.', exist_ok=True)
                    with open(a.out, 'a') as f:
                        f.write(line + '\n')
            del dm, idx, dense, y
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
