# -*- coding:utf-8 -*-
"""Times DeepModel inference on the benchmark's Criteo shape (26 categorical fields x 1 M ids, 13 continuous columns,
D = 16, the default 128 x 64 tower) for the fused inference plan (fused.InferDeepFM / InferDCN / InferStack: one
k_infer_prep launch per call, one k_infer or k_infer_sparse launch per batch) and for the layer-by-layer forward
(DT_AMD_FUSED_PREDICT=0), at batch sizes 128 (DeepTable's default), 8192 and 65536, for the graphs of CONFIGS: DeepFM, DCN,
ModelConfig's default ['dnn_nets'], WideDeep ['linear', 'dnn_nets'], the FM model ['linear', 'fm_nets'] and xDeepFM
['linear', 'cin_nets', 'dnn_nets'] with the default CIN (128, 128) (fused.InferXDeepFM: 2 + 2 launches per batch), and AutoInt
['autoint_nets'] as bench.py builds it (embedding size 32, three interacting layers of four heads, residual on;
fused.InferAutoInt: one launch per batch), and AFM ['linear', 'afm_nets'] (the AFM paper's model, hidden_factor 16;
fused.InferAFM: one launch per batch), and PNN ['pnn_nets'] as bench.py builds it (inner ++ outer 'mat' ++ xn -> tower;
fused.InferPNN: one launch per batch), and FGCNN ['fgcnn_dnn_nets'] with the default blocks (fused.InferFGCNN: 2 x 2 + 1
launches per batch).  Both paths of a configuration run in the same process on the same model and rows.  Prints one JSON line: {"configs": {name: {...}}}.

Both paths score the same device-resident rows (training.TableBatches) and write every batch's output into device memory;
the timed region is what `DeepModel.predict` does after its feed is built, up to the outputs of the last batch (the host copy
of the result is left out: it is the same for both paths).  Device events around each call, warm-up calls first, the
median of the repeats reported (run-to-run spread as min / max).

    python tools/predict_bench.py [--configs deepfm,dcn,dnn,widedeep,fm,xdeepfm,autoint,afm,pnn,fgcnn] [--rows N] [--batches 128,8192,65536]
                                  [--repeats R] [--warmup W] [--paths fused,layer]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

F, VOCAB, ND, D = 26, 1_000_000, 13, 16
CONFIGS = {'deepfm': ['linear', 'fm_nets', 'dnn_nets'], 'dcn': ['dcn_nets'], 'dnn': ['dnn_nets'],
           'widedeep': ['linear', 'dnn_nets'], 'fm': ['linear', 'fm_nets'],
           'xdeepfm': ['linear', 'cin_nets', 'dnn_nets'],           # cin_params' default: cross_layer_size (128, 128)
           'autoint': ['autoint_nets'], 'afm': ['linear', 'afm_nets'],
           'pnn': ['pnn_nets'],                                     # bench.py --model PNN: deepnets.PNN, every default
           'fgcnn': ['fgcnn_dnn_nets']}                             # bench.py --model FGCNN: deepnets.FGCNN, default fgcnn_params
# what a configuration changes of the shape above (bench.py's AutoInt graph: MODEL_PARAMS['AutoInt'], embedding size 32)
EXTRA = {'autoint': {'D': 32, 'autoint_params': {'num_attention': 3, 'num_heads': 4, 'dropout_rate': 0, 'use_residual': True}},
         'afm': {'afm_params': {'hidden_factor': 16, 'dropout_rate': 0}}}


def build_model(nets, seed=0, D=D, **extra):
    from deeptables_amd import functional
    from deeptables_amd.models import DeepModel, ModelConfig
    from deeptables_amd.models.metainfo import CategoricalColumn, ContinuousColumn
    functional.set_seed(seed)
    conf = ModelConfig(nets=list(nets), fixed_embedding_dim=True, embeddings_output_dim=D, embedding_dropout=0,
                       metrics=[], **extra)
    cats = [CategoricalColumn(f'C{i}', VOCAB, D) for i in range(F)]
    conts = [ContinuousColumn('input_continuous_all', [f'I{j}' for j in range(ND)])]
    dm = DeepModel('binary', 2, conf, cats, conts)
    dm.build()
    return dm


def make_feed(dm, n, seed=1):
    from deeptables_amd import training

    class _Frame:                       # training.TableBatches reads X['cat'] / X[column name] of a non-DataFrame
        def __init__(self, d):
            self.d = d

        def __len__(self):
            return n

        def __getitem__(self, k):
            return self.d[k]
    g = np.random.default_rng(seed)
    X = _Frame({'cat': g.integers(0, VOCAB, (n, F)), 'input_continuous_all': g.standard_normal((n, ND)).astype(np.float32)})
    return training.TableBatches(X, None, dm.categorical_columns, dm.continuous_columns, dm.device, resident=True)


def fused_call(dm, data, B):
    plan = dm.inference_plan()
    return lambda: plan.run_batches(data, B)[1]


def layer_call(dm, data, B):
    out = torch.empty((data.n, 1), dtype=torch.float32, device=dm.device)

    def run():
        r = 0
        with torch.no_grad():
            for ins, _ in data.iterate(B, False, drop_remainder=False):
                o = torch.sigmoid(dm.model(ins))
                out[r:r + o.shape[0]].copy_(o)
                r += o.shape[0]
        return out
    return run


def time_call(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def run_config(name, a):
    dm = build_model(CONFIGS[name], **EXTRA.get(name, {}))
    dm.model.eval()
    if 'fused' in a.paths.split(',') and dm.inference_plan() is None:
        raise SystemExit(f'the {name} graph has no inference plan')
    data = make_feed(dm, a.rows)
    res, outs = {'nets': CONFIGS[name], **EXTRA.get(name, {})}, {}
    for path in a.paths.split(','):
        res[path] = {}
        for B in [int(b) for b in a.batches.split(',')]:
            os.environ['DT_AMD_FUSED_PREDICT'] = '1' if path == 'fused' else '0'
            fn = fused_call(dm, data, B) if path == 'fused' else layer_call(dm, data, B)
            ms = time_call(fn, a.warmup, a.repeats)
            med = statistics.median(ms)
            res[path][str(B)] = {'rows_per_s': a.rows / (med * 1e-3), 'ms_median': med, 'ms_min': min(ms), 'ms_max': max(ms)}
            outs[(path, B)] = fn().clone()
    os.environ.pop('DT_AMD_FUSED_PREDICT', None)
    if 'fused' in res and 'layer' in res:
        res['speedup'] = {b: res['fused'][b]['rows_per_s'] / res['layer'][b]['rows_per_s'] for b in res['fused'] if b in res['layer']}
        res['max_abs_diff'] = max(float((outs[('fused', B)] - outs[('layer', B)]).abs().max())
                                  for (p, B) in outs if p == 'fused' and ('layer', B) in outs)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', default=','.join(CONFIGS))
    ap.add_argument('--rows', type=int, default=262144)
    ap.add_argument('--batches', default='128,8192,65536')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--paths', default='fused,layer')
    a = ap.parse_args()
    res = {'metric': 'predict_rows_per_s', 'shape': {'fields': F, 'vocab': VOCAB, 'dense': ND, 'D': D, 'tower': [128, 64]},
           'rows': a.rows, 'repeats': a.repeats, 'warmup': a.warmup, 'configs': {}}
    for name in a.configs.split(','):
        res['configs'][name] = run_config(name, a)
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
