# -*- coding:utf-8 -*-
"""Times k-fold cross-validation of the benchmark's DeepFM both ways (GPU, not a test): (i) the host path of
models/cross_validation.py — the loop a user writes over the API the project had before: per fold `iloc` slices of the
transformed frame, `DeepModel.fit(X_tr, y_tr, validation_data=(X_val, y_val))`, `DeepModel.predict` on the validation slice and
on the freshly transformed X_test, numpy for the out-of-fold rows and the mean — and (ii) the device path: one transform and one
upload per frame, the folds cut out of the resident feed with `ops.take_rows` (csrc/feed_rows.hip), `put_rows` for the
out-of-fold rows, `ensemble_mean` for the test mean, one copy back per result.  The same rows, folds and seed; 26 categorical +
13 continuous columns, embedding width 16, 5 folds, 1 epoch, batches of 8192, an X_test a quarter of the rows.

Both paths are timed through `DeepTable.fit_cross_validation` with `cross_validation.TIMINGS` set, which drains the device
around every phase: transform, upload, fold cutting, training, scoring, mean, copy back.  The host path's uploads happen inside
`DeepModel.fit` and `predict`, so they are part of its training and scoring figures; its 'cut' is the pandas slicing.  The two
runs train their own fold models (from the same seed; the fused steps' atomics do not promise the same bits), so
`max_result_difference` between them is training noise; `restatement_difference` compares the device run's results with the
host-way recomputation from the SAME fold models, which the tests hold to zero.  Appends ONE JSON line to
profiles/cross_validation.jsonl (and prints it).

    python tools/cross_validation_bench.py                    # 1,048,576 rows, X_test 262,144
    python tools/cross_validation_bench.py --rows 65536"""
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


def run(path, df, y, X_test, args):
    """one fit_cross_validation on a fresh DeepTable -> (DeepTable, results, seconds, phase seconds)"""
    import torch
    from deeptables_amd import functional
    from deeptables_amd.models import DeepTable, ModelConfig, cross_validation as CV, deepnets
    functional.set_seed(args.seed)
    torch.manual_seed(args.seed)
    conf = ModelConfig(nets=deepnets.DeepFM, categorical_columns=[f'C{i + 1}' for i in range(F_CAT)], metrics=['AUC'],
                       fixed_embedding_dim=True, embeddings_output_dim=D, embedding_dropout=0, earlystopping_patience=0)
    dt = DeepTable(config=conf)
    CV.TIMINGS = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = dt.fit_cross_validation(df, y, X_test=X_test, num_folds=args.folds, batch_size=args.batch_size, epochs=args.epochs,
                                  verbose=0, random_state=args.seed, device=(path == 'device'))
    torch.cuda.synchronize()
    total = time.perf_counter() - t0
    phases, CV.TIMINGS = CV.TIMINGS, None
    assert dt.last_cv_path == path
    return dt, out, total, {k: round(v, 3) for k, v in phases.items()}


def restate(dt, df, X_test, args):
    """the device run's results recomputed the host way from its own fold models"""
    import numpy as np
    from deeptables_amd.models import cross_validation as CV
    pp = dt.preprocessor
    X_t = pp.transform_X(df)
    folds = CV.make_folds(dt, X_t, None, args.folds, False, None, args.seed)
    oof, mean = np.full((len(df), 1), np.nan), None
    T_t = pp.transform_X(X_test)
    for (tr, va), dm in zip(folds, dt.get_model('all')):
        oof[va] = dm.predict(X_t.iloc[va], batch_size=args.batch_size)
        p = dm.predict(T_t, batch_size=args.batch_size)
        mean = p / len(folds) if mean is None else mean + p / len(folds)
    return np.hstack([1.0 - oof, oof]), np.hstack([1.0 - mean, mean])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=1 << 20)
    ap.add_argument('--test-rows', type=int, default=None)
    ap.add_argument('--folds', type=int, default=5)
    ap.add_argument('--epochs', type=int, default=1)
    ap.add_argument('--batch-size', type=int, default=8192)
    ap.add_argument('--seed', type=int, default=9527)
    ap.add_argument('--warm-rows', type=int, default=65536)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cross_validation.jsonl'))
    args = ap.parse_args()

    import __graft_entry__ as ge
    ge.build()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), 'this benchmark measures the GPU paths'
    test_rows = args.test_rows if args.test_rows is not None else args.rows // 4
    df, y = make_frame(args.rows, args.seed)
    X_test, _ = make_frame(test_rows, args.seed + 1)
    # warm-up: both paths once on a slice (kernel loading, graph capture of the batch shape, the allocator)
    w = min(args.warm_rows, args.rows)
    for path in ('host', 'device'):
        run(path, df.iloc[:w], y[:w], X_test.iloc[:max(w // 4, 1)], args)
    dt_h, out_h, s_h, ph_h = run('host', df, y, X_test, args)
    dt_d, out_d, s_d, ph_d = run('device', df, y, X_test, args)
    del dt_h
    oof_r, test_r = restate(dt_d, df, X_test, args)
    line = {'bench': 'cross_validation', 'rows': args.rows, 'test_rows': test_rows, 'folds': args.folds, 'epochs': args.epochs,
            'batch_size': args.batch_size, 'layout': f'{F_CAT} categorical + {N_CONT} continuous, D {D}', 'nets': 'DeepFM',
            'source_hash': ge.source_hash(),
            'host_s': round(s_h, 3), 'host_phases_s': ph_h, 'host_s_outside_training': round(s_h - ph_h.get('train', 0.0), 3),
            'device_s': round(s_d, 3), 'device_phases_s': ph_d, 'device_train_s': ph_d.get('train', 0.0),
            'device_s_outside_training': round(s_d - ph_d.get('train', 0.0), 3),
            'max_result_difference': {'oof': float(np.nanmax(np.abs(out_h[0] - out_d[0]))),
                                      'test_mean': float(np.abs(out_h[2] - out_d[2]).max())},
            'restatement_difference': {'oof': float(np.nanmax(np.abs(oof_r - out_d[0]))),
                                       'test_mean': float(np.abs(test_r - out_d[2]).max())},
            'nan_rows': [int(np.isnan(out_h[0]).any(1).sum()), int(np.isnan(out_d[0]).any(1).sum())]}
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'a') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
