# -*- coding:utf-8 -*-
"""Times Shapley values both ways on one fitted DeepFM (GPU, not a test): (i) the loop a user could write before utils/shap.py —
per explained row and chunk of coalitions build the frame of hybrid raw rows, `preprocessor.transform_X`, `DeepModel.predict`,
a float64 mean over the background and the regression in numpy — and (ii) the device path
(`DeepTablesExplainer(device=True)`): background and explained rows transformed once into resident feeds, per chunk
dt_coalition_fill per feed block, the fused inference launches, dt_coalition_mean, and one dt_shap_solve
(csrc/coalition.hip).  The same model, background, explained rows and coalition plan (`coalition_plan` / `solve_matrix`: both
loops read it); each path is warmed up on one explained row, then the two are alternated `--repeats` times; a host clock
around work that ends in a synchronise (the device path ends in the read of phi).  The benchmark's DeepFM column layout
(26 categorical + 13 continuous columns, embedding width 16), 50 background rows, nsamples 'auto' (2 * 39 + 2048 coalitions,
so 106,300 hybrid rows per explained row).  Appends ONE JSON line to profiles/shap.jsonl (and prints it).

    python tools/shap_bench.py                       # 4 explained rows, 3 alternations
    python tools/shap_bench.py --explain 8 --repeats 5"""
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


def hand_loop(dt, bg, X, masks, P, batch_size, chunk_rows):
    """-> (phi float64 [R, M], seconds per explained row): every raw column a player (all 39 feed the model)"""
    import numpy as np
    import pandas as pd
    import torch
    pp, dm = dt.preprocessor, dt.model
    cols = bg.columns.to_list()
    S, M = masks.shape
    Nb = len(bg)
    f = lambda frame: np.asarray(dm.predict(pp.transform_X(frame), batch_size=batch_size)).reshape(len(frame), -1)[:, 0]
    e0 = f(bg).astype(np.float64).mean()
    fx = f(X).astype(np.float64)
    step = max(1, chunk_rows // Nb)
    z_last = masks[:, -1].astype(np.float64)
    phi, times = np.zeros((len(X), M)), []
    for r in range(len(X)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ey = np.zeros(S)
        for s0 in range(0, S, step):
            m = masks[s0:s0 + step]
            data = {}
            for k, c in enumerate(cols):
                col = np.tile(bg[c].values, len(m))
                col[np.repeat(m[:, k], Nb)] = X[c].values[r]
                data[c] = col
            out = f(pd.DataFrame(data, columns=cols))
            ey[s0:s0 + len(m)] = out.astype(np.float64).reshape(len(m), Nb).mean(axis=1)
        y = ey - e0 - z_last * (fx[r] - e0)
        phi[r, :-1] = P @ y
        phi[r, -1] = (fx[r] - e0) - phi[r, :-1].sum()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return phi, times


def device_run(ex, X, batch_size):
    """-> (phi, seconds of the whole call: both feeds built, every explained row, the read of the results)"""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    phi = ex.get_shap_values(X, batch_size=batch_size)
    torch.cuda.synchronize()
    return phi, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=1 << 16, help='rows of the training frame')
    ap.add_argument('--background', type=int, default=50)
    ap.add_argument('--explain', type=int, default=4)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--batch-size', type=int, default=8192)
    ap.add_argument('--train-steps', type=int, default=30)
    ap.add_argument('--seed', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'shap.jsonl'))
    args = ap.parse_args()

    import __graft_entry__ as ge
    ge.build()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), 'this benchmark measures the GPU paths'
    from deeptables_amd import functional
    from deeptables_amd.models import DeepTable, ModelConfig, deepnets
    from deeptables_amd.utils import shap as SH
    df, y = make_frame(args.rows, args.seed)
    functional.set_seed(args.seed)
    conf = ModelConfig(nets=deepnets.DeepFM, categorical_columns=[f'C{i + 1}' for i in range(F_CAT)], metrics=['AUC'],
                       fixed_embedding_dim=True, embeddings_output_dim=D, embedding_dropout=0, earlystopping_patience=0)
    dt = DeepTable(config=conf)
    dt.fit(df, y, batch_size=args.batch_size, epochs=1, steps_per_epoch=args.train_steps, validation_split=0, verbose=0)
    assert dt.model.inference_plan() is not None, 'the DeepFM graph should take its inference plan'
    ex = SH.DeepTablesExplainer(dt, df, num_samples=args.background, device=True)
    assert len(ex.players) == F_CAT + N_CONT
    t0 = time.perf_counter()
    masks, weights, P = ex.plan('auto')
    plan_s = time.perf_counter() - t0
    X = df.iloc[1000:1000 + args.explain]
    bs = args.batch_size

    hand_loop(dt, ex.background, X.iloc[:1], masks, P, bs, SH.SHAP_MAX_SYNTH_ROWS)                 # warm-up, one row each
    device_run(ex, X.iloc[:1], bs)
    loop_rows, device_calls, phis = [], [], []
    for _ in range(args.repeats):
        hp, times = hand_loop(dt, ex.background, X, masks, P, bs, SH.SHAP_MAX_SYNTH_ROWS)
        dp, d_s = device_run(ex, X, bs)
        assert ex.last_path == 'device'
        loop_rows += times
        device_calls.append(d_s)
        phis.append(dp)
    dev_row = [s / args.explain for s in device_calls]
    line = {'bench': 'shap', 'layout': f'{F_CAT} categorical + {N_CONT} continuous, D {D}', 'nets': 'DeepFM',
            'background': len(ex.background), 'players': len(ex.players), 'coalitions': int(len(masks)),
            'hybrid_rows_per_explained_row': int(len(masks) * len(ex.background)), 'explained_rows': args.explain,
            'repeats': args.repeats, 'batch_size': bs, 'source_hash': ge.source_hash(), 'path': ex.last_path,
            'plan_and_solve_matrix_s_once': round(plan_s, 3),
            'loop_s_per_explained_row': {'median': round(float(np.median(loop_rows)), 4), 'min': round(min(loop_rows), 4),
                                         'max': round(max(loop_rows), 4), 'n': len(loop_rows)},
            'device_s_per_explained_row_with_feed_build': {'median': round(float(np.median(dev_row)), 5),
                                                           'min': round(min(dev_row), 5), 'max': round(max(dev_row), 5),
                                                           'n': len(dev_row)},
            'loop_over_device': round(float(np.median(loop_rows) / np.median(dev_row)), 1),
            'max_phi_difference': float(np.abs(dp - hp).max()), 'max_abs_phi': float(np.abs(hp).max()),
            'device_runs_equal': bool(all(np.array_equal(p, phis[0]) for p in phis))}
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'a') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
