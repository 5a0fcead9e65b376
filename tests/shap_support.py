# -*- coding:utf-8 -*-
"""Shared by tests/test_shap_host.py and tests/test_shap_gpu.py: the value function of utils/shap.py evaluated by an
independent hand loop over frames, exact Shapley values from the definition, the bars, and a CPU fit that feeds var-len
columns (tests/feature_importance_support.py `fit_cpu` does not)."""
import itertools
from math import factorial

import numpy as np
import pandas as pd
import torch

from tests import feature_importance_support as FS

U64 = 2.0 ** -53


def mixed_labels(df):
    rng = np.random.default_rng(3)
    y = ((df['c_int'] > 3) ^ (df['f_two'] > 1)).astype(int).values
    y[rng.random(len(y)) < 0.05] ^= 1
    return y


def fit_cpu_with_var_len(df, y, conf, epochs=2, seed=3, lr=0.01):
    """FS.fit_cpu with the var-len blocks in the training feed"""
    from deeptables_amd import functional, training
    from deeptables_amd.models import DeepTable, deepmodel
    functional.set_seed(seed)
    dt = DeepTable(config=conf)
    pp = dt.preprocessor
    X_t, y_t = pp.fit_transform(df, y)
    dm = deepmodel.DeepModel(dt.task, dt.num_classes, conf, pp.categorical_columns, pp.continuous_columns,
                             var_categorical_len_columns=pp.var_len_categorical_columns)
    dm.build('cpu')
    feed = training.TableBatches(X_t, y_t, dm.categorical_columns, dm.continuous_columns, 'cpu', dm.task, dm.num_classes,
                                 var_len_categorical_columns=dm.var_len_categorical_columns)
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


def mask_key(mask):
    """bool [M] -> the subset as an integer (bit k: player k)"""
    return int(sum(1 << k for k, bit in enumerate(mask) if bit))


def hand_frames(bg, x_row, player_columns):
    """Every subset of the players, written out with pandas column assignment: subset `key` (bit k: player k taken from the
    explained row) is rows [key * Nb, (key + 1) * Nb) of the returned frame"""
    M, frames = len(player_columns), []
    for key in range(2 ** M):
        frame = bg.copy()
        for k, c in enumerate(player_columns):
            if key >> k & 1:
                frame[c] = [x_row[c].iloc[0]] * len(bg)
                frame[c] = frame[c].astype(bg[c].dtype)
        frames.append(frame)
    return pd.concat(frames, ignore_index=True)


def hand_outputs(dt, bg, X_to_explain, player_columns, batch_size=128):
    """-> float32 [R, 2^M, Nb, O]: the model's outputs for every hybrid row of every subset, by the functions the project had
    before utils/shap.py (transform_X, DeepModel.predict)"""
    out = []
    for r in range(len(X_to_explain)):
        frame = hand_frames(bg, X_to_explain.iloc[r:r + 1], player_columns)
        y = np.asarray(dt.model.predict(dt.preprocessor.transform_X(frame), batch_size=batch_size))
        out.append(y.reshape(2 ** len(player_columns), len(bg), -1))
    return np.stack(out)


def exact_shapley(v):
    """v float64 [2^M, O] indexed by subset -> phi float64 [O, M] from the definition:
    phi_i = sum over S without i of |S|! (M - |S| - 1)! / M! (v(S + i) - v(S))"""
    M = int(np.log2(len(v)))
    assert len(v) == 2 ** M
    phi = np.zeros((v.shape[1], M), dtype=np.float64)
    for i in range(M):
        others = [k for k in range(M) if k != i]
        for size in range(M):
            w = factorial(size) * factorial(M - size - 1) / factorial(M)
            for sub in itertools.combinations(others, size):
                key = sum(1 << k for k in sub)
                phi[:, i] += w * (v[key | 1 << i] - v[key])
    return phi


class ChunkOutputs:
    """on_chunk hook: keeps the outputs of every (explained row, coalition) as float64 [Nb, O] under (r, subset key)"""

    def __init__(self, masks, Nb):
        self.masks, self.Nb, self.seen, self.blocks = masks, Nb, {}, []

    def __call__(self, r, s0, s1, blocks, outputs):
        out = outputs.detach().cpu().numpy() if torch.is_tensor(outputs) else np.asarray(outputs)
        out = out.reshape(s1 - s0, self.Nb, -1)
        for s in range(s0, s1):
            self.seen[r, mask_key(self.masks[s])] = out[s - s0].astype(np.float64)
        self.blocks.append((r, s0, s1, blocks))

    def delta(self, hand):
        """the largest difference between these outputs and the hand loop's for the same hybrid row"""
        return max(float(np.abs(o - hand[r, key]).max()) for (r, key), o in self.seen.items())


def features_from_players(phi, feature_names, player_columns):
    """phi [M] over the players -> [n_features] with 0.0 for the others"""
    out = np.zeros(len(feature_names))
    for k, c in enumerate(player_columns):
        out[feature_names.index(c)] = phi[k]
    return out


def efficiency_bar(phi_row):
    return len(phi_row) * 2.0 ** -52 * np.abs(phi_row).sum()


def check_against_exact(ex, X_to_explain, phi, hook, hand, what):
    """phi (the explainer's result, one output) against exact Shapley values of the hand loop's value function, within
    2 delta + 1e-12 max|v|; the efficiency identity; non-players exactly 0.0 -> delta"""
    cols = list(ex.players)
    delta = hook.delta(hand)
    arrays = phi if isinstance(phi, list) else [phi]
    e0 = np.atleast_1d(ex.expected_value)
    for r in range(len(X_to_explain)):
        v = hand[r].astype(np.float64).mean(axis=1)                        # [2^M, O]
        want = exact_shapley(v)
        bar = 2 * delta + 1e-12 * np.abs(v).max()
        for o, arr in enumerate(arrays):
            w = features_from_players(want[o], ex.feature_names, cols)
            diff = np.abs(arr[r] - w).max()
            print(f'{what} row {r} output {o}: max|phi - exact| {diff:.3e}, bar {bar:.3e} (delta {delta:.3e}); '
                  f'max|phi| {np.abs(w).max():.3e}')
            assert diff <= bar, (what, r, o, diff, bar, delta)
            for c in ex.feature_names:
                if c not in ex.players:
                    assert arr[r, ex.feature_names.index(c)] == 0.0
            fx = np.atleast_2d(ex.fx.reshape(len(X_to_explain), -1))[r, o]
            assert abs(arr[r].sum() - (fx - e0[o])) <= efficiency_bar(arr[r]), (what, r, o)
            assert abs(e0[o] - v[0, o]) <= delta + 1e-12 * abs(v[0, o])
    return delta
