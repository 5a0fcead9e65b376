# -*- coding:utf-8 -*-
"""Permutation feature importance for a fitted `DeepTable` (the interface of deeptables/utils/feature_importance.py:
`get_score_importances`, `select_features`), without eli5 and hypernets.

The score of a pass is this project's own metric on the model's activated output against the encoded labels — what
`DeepTable.evaluate` reports under that name.  For auc, log_loss, accuracy, precision, recall, mse, rmse and mae that is by
definition the quantity hypernets' `calc_score` gives on `predict` / `predict_proba`; it was not compared with a hypernets run.
`score_decreases[i, c] = base_score - score(column c permuted, iteration i)` is eli5's definition.

Two paths compute it:
  * device: the frame is transformed ONCE into a resident `training.TableBatches`; every pass permutes the model inputs a raw
    column feeds inside the feed's blocks (`ops.permute_columns`: csrc/feed_columns.hip), scores the way `DeepModel.evaluate`
    does (`DeepModel.score_batches`, `metrics.epoch_metrics`) and swaps the original values back.  Which inputs a raw column
    feeds is declared by the preprocessor (`source_columns()`); every fitted transformer works row by row, so permuting the
    raw column and transforming equals transforming and permuting those inputs with the same permutation.
  * host: per pass copy the frame, permute the raw column(s), `preprocessor.transform_X`, `DeepModel.predict`,
    `metrics.compute_metric`.  Any preprocessor, any device.

One permutation per (iteration, entry of `columns`), iteration-major, from `torch.randperm` with a `torch.Generator` on the
model's device seeded by `random_state` — for every entry, also one that is skipped, so both paths consume the same
permutations for the same seed.  This is NOT eli5's `RandomState.shuffle` stream.  The result rows are ordered by the
importance as a number (the reference sorts the stacked string array, which puts '9e-05' above '0.3')."""
import os

import numpy as np
import torch

from .. import metrics, ops, training

HOST_BATCH_SIZE = 128           # the reference's predict_proba default
DEVICE_BATCH_SIZE = 8192


def device_importance_enabled():
    """DT_AMD_DEVICE_IMPORTANCE=0 (read at every call) keeps device='auto' on the host path"""
    return os.environ.get('DT_AMD_DEVICE_IMPORTANCE', '1') != '0'


def _mode_sign(mode):
    if mode == 'min':
        return -1.0
    if mode == 'max':
        return 1.0
    raise ValueError(f'Unsupported mode:{mode}')


def _entries(X, columns):
    """[(reported name, [raw columns permuted together])]: a list / tuple entry is a group under the tuple of its names"""
    known = set(X.columns.to_list())
    out = []
    for c in (X.columns.to_list() if columns is None else list(columns)):
        members = list(c) if isinstance(c, (list, tuple)) else [c]
        if not members:
            raise ValueError('columns: an empty group')
        for m in members:
            if m not in known:
                raise ValueError(f'columns: {m!r} is not a column of X')
        out.append((tuple(members) if isinstance(c, (list, tuple)) else c, members))
    return out


def _source_map(preprocessor):
    fn = getattr(preprocessor, 'source_columns', None)
    return fn() if callable(fn) else None


def _derived(source_map, raw):
    """the transformed columns of one raw column ([]: it feeds nothing)"""
    if raw in source_map:
        return list(source_map[raw])
    return list(source_map.get(str(raw), []))


def make_feed(dt_model, X, y_encoded, cat_dtype=torch.int32, resident=None):
    """The raw frame once -> ONE feed with the encoded labels on the model's device: `preprocessor.transform_feed` (on a GPU the
    numeric columns go through one kernel launch per block), `transform_X` for a preprocessor without it or a feed that is
    asked not to be resident"""
    dm = dt_model.model
    pp = dt_model.preprocessor
    if callable(getattr(pp, 'transform_feed', None)) and resident is not False:
        return pp.transform_feed(X, y_encoded, device=dm.device, task=dm.task, num_classes=dm.num_classes, cat_dtype=cat_dtype,
                                 y_encoded=True)
    return training.TableBatches(dt_model.preprocessor.transform_X(X), y_encoded, dm.categorical_columns,
                                 dm.continuous_columns, dm.device, dm.task, dm.num_classes, cat_dtype=cat_dtype,
                                 var_len_categorical_columns=dm.var_len_categorical_columns, resident=resident)


def feed_positions(dm, feed):
    """{transformed column name: (block number of `feed`, column inside it, or None = the whole block)}: a categorical column
    is column j of the 'cat' block, a var-len column its whole 'var' block, a continuous column is column j of the 'cont'
    block of the ContinuousColumn that lists it (blocks in model input order, training.TableBatches)"""
    pos, b = {}, 0
    if dm.categorical_columns:
        for j, c in enumerate(dm.categorical_columns):
            pos[c.name] = (b, j)
        b += 1
    for c in dm.var_len_categorical_columns or []:
        pos[c.name] = (b, None)
        b += 1
    for c in dm.continuous_columns or []:
        for j, name in enumerate(c.column_names):
            pos[name] = (b, j)
        b += 1
    if b != len(feed.blocks):
        raise ValueError(f'the feed has {len(feed.blocks)} blocks, the model {b} inputs')
    return pos


def feed_targets(dm, feed, source_map, members):
    """{block number: [columns]} the raw columns `members` feed ({}: the model cannot see them)"""
    pos, targets = feed_positions(dm, feed), {}
    for raw in members:
        for name in _derived(source_map, raw):
            if name not in pos:                         # carried along by the preprocessor, not a model input
                continue
            b, j = pos[name]
            cols = range(feed.blocks[b].shape[1]) if j is None else [j]
            targets.setdefault(b, set()).update(cols)
    return {b: sorted(cols) for b, cols in targets.items()}


def _source_map_missing(preprocessor):
    return not callable(getattr(preprocessor, 'source_columns', None))


def device_refusal(dt_model, feed=None):
    """None when the device path can serve this model (and feed), else the condition that fails, in words"""
    dm = dt_model.model
    if torch.device(dm.device).type != 'cuda':
        return f'the model is on {dm.device}, not on a GPU'
    if _source_map_missing(dt_model.preprocessor):
        return f'{type(dt_model.preprocessor).__name__} declares no source_columns()'
    st = dm.config.distribute_strategy
    if st is not None and getattr(st, 'world_size', 1) > 1:
        return 'a multi-rank distribute_strategy is active'
    return None if feed is None else feed_refusal(dt_model, feed)


def feed_refusal(dt_model, feed):
    """the conditions on the feed itself: resident, int32 / float32 blocks; and a preprocessor that declares its map"""
    if _source_map_missing(dt_model.preprocessor):
        return f'{type(dt_model.preprocessor).__name__} declares no source_columns()'
    if not feed.resident:
        return 'the feed is not resident on the device'
    for kind, blk in zip(feed.kinds, feed.blocks):
        if blk.dtype not in (torch.int32, torch.float32):
            return f"the feed's '{kind}' block is {blk.dtype}, the column kernels move int32 / float32 words"
    return None


def _generator(device, random_state):
    device = torch.device(device)
    g = torch.Generator(device=device if device.type == 'cuda' else 'cpu')
    g.manual_seed(int(random_state) if random_state is not None else int.from_bytes(os.urandom(8), 'little') >> 1)
    return g


def _draw(n, g):
    return torch.randperm(n, generator=g, device=g.device)


def feed_scores(dt_model, feed, entries, metric, n_iter, sign, generator, batch_size, on_pass=None):
    """The passes of the device path over a ready feed (GPU tensors: the HIP column kernels; CPU tensors: ops.permute_columns'
    torch branch) -> (base_score, score_decreases [n_iter, len(entries)]).  on_pass(iteration or None, entry number or None,
    outputs) sees every pass's outputs (tests).  The feed is left bit for bit as it was, also when a pass raises."""
    reason = feed_refusal(dt_model, feed)
    if reason is not None:
        raise ValueError(f'feature importance on the device: {reason}')
    dm = dt_model.model
    name = metrics.metric_name(metric)
    source_map = _source_map(dt_model.preprocessor)
    targets = [feed_targets(dm, feed, source_map, members) for _, members in entries]

    def score(i, c):
        out = dm.score_batches(feed, batch_size)
        if on_pass is not None:
            on_pass(i, c, out)
        return sign * metrics.epoch_metrics([metric], feed.y, out, dm.task)[name]

    base = score(None, None)
    dec = np.zeros((n_iter, len(entries)), dtype=np.float64)
    for i in range(n_iter):
        for c, tg in enumerate(targets):
            perm = _draw(feed.n, generator)
            if not tg:
                continue                                # feeds no model input: 0.0 without a pass
            done = []
            try:
                for b, cols in tg.items():
                    done.append(ops.permute_columns(feed.blocks[b], cols, perm))
                dec[i, c] = base - score(i, c)
            finally:
                for h in reversed(done):
                    h.restore()
    return base, dec


def host_scores(dt_model, X, y_encoded, entries, metric, n_iter, sign, generator, batch_size, on_pass=None):
    """The loop a user writes by hand: per pass copy the frame, permute the raw column(s), transform_X, DeepModel.predict,
    metrics.compute_metric -> (base_score, score_decreases).  A raw column the preprocessor declares to feed nothing is 0.0
    without a pass (its permutation is drawn all the same)."""
    dm, pp = dt_model.model, dt_model.preprocessor
    source_map = _source_map(pp)

    def score(frame, i, c):
        out = dm.predict(pp.transform_X(frame), batch_size=batch_size)
        if on_pass is not None:
            on_pass(i, c, out)
        return sign * metrics.compute_metric(metric, y_encoded, out, dm.task)

    base = score(X, None, None)
    dec = np.zeros((n_iter, len(entries)), dtype=np.float64)
    for i in range(n_iter):
        for c, (_, members) in enumerate(entries):
            perm = _draw(len(X), generator).cpu().numpy()
            if source_map is not None and not any(_derived(source_map, m) for m in members):
                continue
            frame = X.copy()
            for m in members:
                frame[m] = X[m].values[perm]
            dec[i, c] = base - score(frame, i, c)
    return base, dec


def permutation_scores(dt_model, X, y, metric, n_iter=5, mode='min', random_state=None, batch_size=None, columns=None,
                       device='auto'):
    """-> {'columns': [...], 'base_score': float, 'score_decreases': float64 [n_iter, n_columns], 'path': 'device' | 'host'}.
    device: 'auto' takes the device path when the model is on a GPU, the feed resident with int32 / float32 blocks, the
    preprocessor declares `source_columns()`, no multi-rank distribute_strategy is active and DT_AMD_DEVICE_IMPORTANCE is not
    '0'; True raises and names the condition that fails; False is the host path.  batch_size None: 128 on the host path,
    min(n, 8192) on the device path; the result does not depend on it."""
    sign = _mode_sign(mode)
    dt_model._require_model()
    if int(n_iter) < 1:
        raise ValueError(f'n_iter must be at least 1, got {n_iter}')
    if X is None or len(X) == 0:
        raise ValueError('X can not be empty.')
    if len(y) != len(X):
        raise ValueError(f'y has {len(y)} entries for {len(X)} rows of X')
    if device not in ('auto', True, False):
        raise ValueError(f"device must be 'auto', True or False, got {device!r}")
    entries = _entries(X, columns)
    n_iter = int(n_iter)
    y_encoded = dt_model.preprocessor.transform_y(y)
    generator = _generator(dt_model.model.device, random_state)
    feed = None
    if device is not False:
        reason = device_refusal(dt_model)
        if reason is None and device == 'auto' and not device_importance_enabled():
            reason = 'DT_AMD_DEVICE_IMPORTANCE=0'
        if reason is None:
            feed = make_feed(dt_model, X, y_encoded, resident=None)
            reason = feed_refusal(dt_model, feed)
        if reason is not None:
            if device is True:
                raise ValueError(f'device=True: {reason}')
            feed = None
    if feed is not None:
        bs = min(len(X), DEVICE_BATCH_SIZE) if batch_size is None else int(batch_size)
        base, dec = feed_scores(dt_model, feed, entries, metric, n_iter, sign, generator, bs)
    else:
        bs = HOST_BATCH_SIZE if batch_size is None else int(batch_size)
        base, dec = host_scores(dt_model, X, y_encoded, entries, metric, n_iter, sign, generator, bs)
    return {'columns': [name for name, _ in entries], 'base_score': float(base), 'score_decreases': dec,
            'path': 'device' if feed is not None else 'host'}


def get_score_importances(dt_model, X, y, metric, n_iter=5, mode='min', random_state=None, batch_size=None, columns=None,
                          device='auto'):
    """-> array [n_columns, 2] of (column name, mean score decrease over the iterations), the largest decrease first (ordered
    by the number; ties keep the order of `columns`), laid out as the reference lays it out: numpy.stack of the names and the
    means, so `float(fi[1])` reads an importance.  A group of columns is reported under the tuple of its names (then the array
    holds objects)."""
    res = permutation_scores(dt_model, X, y, metric, n_iter=n_iter, mode=mode, random_state=random_state,
                             batch_size=batch_size, columns=columns, device=device)
    means = res['score_decreases'].mean(axis=0)
    order = np.argsort(-means, kind='stable')
    names = res['columns']
    if any(isinstance(c, tuple) for c in names):
        out = np.empty((len(names), 2), dtype=object)
        for r, k in enumerate(order):
            out[r, 0], out[r, 1] = names[k], float(means[k])
        return out
    return np.stack([[names[k] for k in order], means[order]], axis=1)


def select_features(feature_importances, threshold=0.):
    """-> (selected_columns, discard_columns): the names whose importance is above `threshold`, and those at or below it (a
    NaN importance is in neither list, as in the reference)"""
    pairs = [(fi[0], float(fi[1])) for fi in feature_importances]
    return [name for name, v in pairs if v > threshold], [name for name, v in pairs if v <= threshold]
