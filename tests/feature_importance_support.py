# -*- coding:utf-8 -*-
"""Shared by tests/test_feature_importance_host.py and tests/test_feature_importance_gpu.py: the frames, the loop a user
writes by hand (the yardstick of utils/feature_importance.py), the bars, and what lets a small `DeepTable` run on CPU tensors.

The layers' hot path has no CPU fallback (the embedding gather and BatchNormalization are HIP kernels), so a host test that needs
a model's outputs swaps torch restatements of exactly those three ops in (`cpu_kernels`) and trains with torch's Adam
(`fit_cpu`).  Everything else is the project's own code: the preprocessor, the functional graph, `TableBatches`,
`DeepModel.predict` / `score_batches`, the metrics."""
import numpy as np
import pandas as pd
import torch

from tests import scores_reference as S

TOWER = {'hidden_units': ((8, 0, False), (4, 0, False)), 'activation': 'relu'}


# ---- CPU stand-ins for the three kernels a ['dnn_nets'] forward launches ------------------------------------------------------
def _lookup(idx, table, row_offset, vocab, holder=None, dense_grad=False, oob=None, dropout=None):
    assert dropout is None
    rows = idx.to(torch.int64) + row_offset[None, :]
    return table[rows], rows


def _bn_train(x, gamma, beta, moving_mean, moving_var, eps=1e-3, momentum=0.99):
    mean, var = x.mean(0), x.var(0, unbiased=False)
    with torch.no_grad():
        moving_mean.mul_(momentum).add_((1 - momentum) * mean)
        moving_var.mul_(momentum).add_((1 - momentum) * var)
    return (x - mean) * torch.rsqrt(var + eps) * gamma + beta


def _bn_infer(x, gamma, beta, moving_mean, moving_var, eps=1e-3):
    return (x - moving_mean) * torch.rsqrt(moving_var + eps) * gamma + beta


def cpu_kernels(mp):
    """mp: a pytest MonkeyPatch.  The inference plans are switched off: they launch."""
    from deeptables_amd import ops
    mp.setattr(ops, 'embedding_lookup', _lookup)
    mp.setattr(ops, 'batchnorm_train', _bn_train)
    mp.setattr(ops, 'batchnorm_infer', _bn_infer)
    mp.setenv('DT_AMD_FUSED_PREDICT', '0')


def fit_cpu(df, y, conf, epochs=2, seed=3, lr=0.01, preprocessor=None):
    """DeepTable.fit's steps on the CPU (under `cpu_kernels`): fit_transform, build, `epochs` passes of torch Adam"""
    from deeptables_amd import functional, training
    from deeptables_amd.models import DeepTable, deepmodel
    functional.set_seed(seed)
    dt = DeepTable(config=conf, preprocessor=preprocessor)
    pp = dt.preprocessor
    X_t, y_t = pp.fit_transform(df, y)
    dm = deepmodel.DeepModel(dt.task, dt.num_classes, conf, pp.categorical_columns, pp.continuous_columns,
                             var_categorical_len_columns=getattr(pp, 'var_len_categorical_columns', None))
    dm.build('cpu')
    feed = training.TableBatches(X_t, y_t, dm.categorical_columns, dm.continuous_columns, 'cpu', dm.task, dm.num_classes)
    opt = torch.optim.Adam(dm.model.parameters(), lr=lr)
    g = torch.Generator().manual_seed(seed)
    for _ in range(epochs):
        dm.model.train()
        for ins, yb in feed.iterate(64, True, True, generator=g):
            opt.zero_grad()
            dm._loss(dm.model(ins), yb).backward()
            opt.step()
    dm.model.eval()
    dt.model = dm
    return dt


# ---- frames ---------------------------------------------------------------------------------------------------------------
def mixed_frame(n=400, seed=0):
    """every way a raw column reaches the model: a string categorical with missing values, an int column auto_categorize picks
    up (with cat_remain_numeric: continuous c_int + categorical c_int_cat, and c_int_discrete with auto_discrete), floats
    with NaNs, a constant, an excluded column and a '|'-separated var-len column"""
    rng = np.random.default_rng(seed)
    s = rng.choice(['a', 'b', 'c', 'd'], n).astype(object)
    s[rng.random(n) < 0.1] = None
    f = rng.normal(size=n)
    f[rng.random(n) < 0.1] = np.nan
    tags = ['|'.join(rng.choice(['p', 'q', 'r', 's', 't'], rng.integers(1, 4), replace=False)) for _ in range(n)]
    return pd.DataFrame({'c_str': s, 'c_int': rng.integers(0, 7, n), 'f_nan': f, 'f_two': rng.normal(size=n) * 3 + 1,
                         'const': np.full(n, 2.5), 'excluded': rng.normal(size=n), 'tags': tags})


def mixed_config(**kw):
    from deeptables_amd.models import ModelConfig
    return ModelConfig(nets=['dnn_nets'], dnn_params=TOWER, embedding_dropout=0, auto_categorize=True, cat_remain_numeric=True,
                       auto_discrete=True, auto_scale=True, exclude_columns=['excluded'],
                       var_len_categorical_columns=[('tags', '|', 'max')], earlystopping_patience=0, **kw)


def task_frame(task, n=600, seed=0):
    """4 categorical + 3 continuous columns and labels that depend on one of each"""
    rng = np.random.default_rng(seed)
    df = pd.DataFrame({'job': rng.choice(['admin', 'tech', 'services', 'retired'], n), 'marital': rng.choice(['m', 's', 'd'], n),
                       'region': rng.choice(['n', 'e', 's', 'w', 'c'], n), 'flag': rng.choice(['y', 'n'], n),
                       'age': rng.integers(18, 80, n).astype(np.float32), 'balance': rng.normal(1000, 500, n).astype(np.float32),
                       'rate': rng.random(n).astype(np.float32)})
    z = (df['age'].values - 50) / 20 + (df['job'] == 'tech').values * 1.5 + rng.normal(size=n) * 0.3
    if task == 'binary':
        y = np.where(z > 0, 'yes', 'no')
    elif task == 'multiclass':
        y = np.digitize(z, [-0.5, 0.7])
    else:
        y = (z * 2 + 1).astype(np.float64) + rng.normal(size=n) * 1e-3
    return df, y


TASK_METRICS = {'binary': ['auc', 'log_loss', 'accuracy'], 'multiclass': ['accuracy'], 'regression': ['rmse']}


def task_config(task, nets=('dnn_nets',), **kw):
    from deeptables_amd.models import ModelConfig
    return ModelConfig(nets=list(nets), dnn_params=TOWER, embedding_dropout=0, task=task, auto_categorize=False,
                       metrics=TASK_METRICS[task], earlystopping_patience=0, **kw)


# ---- the yardstick --------------------------------------------------------------------------------------------------------
def hand_loop(dt, df, y, metric, n_iter, mode, seed, columns=None, batch_size=128, device='cpu', on_pass=None):
    """Permutation importance with the public functions the project had before utils/feature_importance.py: per pass copy the
    frame, permute the raw column, preprocessor.transform_X, DeepModel.predict, metrics.compute_metric; one seeded
    torch.randperm per (iteration, column), iteration-major -> (base_score, score_decreases)"""
    from deeptables_amd import metrics
    pp, dm = dt.preprocessor, dt.model
    sign = {'min': -1.0, 'max': 1.0}[mode]
    y_enc = pp.transform_y(y)
    columns = df.columns.to_list() if columns is None else columns
    g = torch.Generator(device=device).manual_seed(seed)

    def score(frame, i, c):
        out = dm.predict(pp.transform_X(frame), batch_size=batch_size)
        if on_pass is not None:
            on_pass(i, c, out)
        return sign * metrics.compute_metric(metric, y_enc, out, dm.task)

    base = score(df, None, None)
    dec = np.zeros((n_iter, len(columns)))
    for i in range(n_iter):
        for c, name in enumerate(columns):
            perm = torch.randperm(len(df), generator=g, device=device).cpu().numpy()
            frame = df.copy()
            frame[name] = df[name].values[perm]
            dec[i, c] = base - score(frame, i, c)
    return base, dec


# ---- bars -----------------------------------------------------------------------------------------------------------------
def metric_bar(metric, n_out, value):
    """The bar at which the existing GPU tests hold the device's value of `metric` to metrics.compute_metric's, for a value
    of this size over n_out outputs"""
    key = metric.lower()
    if key == 'auc':
        return 1e-12                                            # tests/test_metrics_gpu.py:371
    if key in ('accuracy', 'acc'):
        return 0.0                                              # tests/test_metrics_gpu.py:371 (held equal)
    if key in ('log_loss', 'logloss'):
        return (S.sum_bound(n_out, S.E_BCE) + 2 * S.U) * abs(value)        # tests/test_scores_gpu.py:557 and :573
    if key == 'rmse':
        # tests/test_scores_gpu.py:567 holds mse to 1e-6 of the host's float32 mean; the square root halves a relative
        # difference and the host's float32 sqrt adds 2^-24: 5.6e-7 <= 1e-6
        return 1e-6 * abs(value)
    raise KeyError(metric)


def decrease_tolerance(metric, n_out, base, decrease):
    """a decrease is the difference of two metric values: at most twice the bar of the larger one"""
    return 2 * metric_bar(metric, n_out, max(abs(base), abs(base - decrease)))
