# -*- coding:utf-8 -*-
"""Shapley values for a fitted `DeepTable` (the interface of deeptables/utils/shap.py: `DeepTablesExplainer(dt_model, X,
num_samples=50)`, `get_shap_values(X_to_explain, nsamples='auto')`), without the shap package.

What is computed is KernelSHAP.  The FEATURES are the raw columns of `X`, in order; the PLAYERS are those of them that feed
at least one model input (`preprocessor.source_columns()`, `feature_importance.feed_targets`): a raw column that feeds
nothing is in no coalition and gets exactly 0.0.  A preprocessor that declares no map makes every raw column a player.
The background is all of `X` when `num_samples is None` or `len(X) <= num_samples`, else the rows
`numpy.random.RandomState(random_state).permutation(len(X))[:num_samples]` — the row set `shap.sample` draws through
`sklearn.utils.resample(replace=False, random_state=0)`; the weights are uniform.  The value of a coalition S for the
explained row x_r is
    v_r(S) = (1 / Nb) sum_b f(h(x_r, bg_b, S))
where h takes the raw columns in S from x_r and every other column from background row b, and f is the model's activated
output (`predict_proba`, or the prediction of a regression).  `expected_value = v(empty)`.

`coalition_plan` is the one source of coalitions of both paths.  It restates shap's sampling scheme IN OUTLINE — subset sizes
completed from the outside in while the budget covers a size and its complement, the rest of the budget drawn in
complementary pairs with the sizes chosen by the remaining kernel mass, duplicates merged — from its description; it was
NOT compared with a run of shap, and its random stream is not shap's.  Deviations that are deliberate:
  * no L1 feature selection (shap's `l1_reg='auto'`): the regression is plain weighted least squares under the constraint
    sum(phi) = f(x) - expected_value, in float64.  This only matters in the sampled regime; under full enumeration
    (M <= 11 players with nsamples='auto') the regression reproduces the exact Shapley values to rounding.
  * one plan serves every explained row.  shap drops the players on which a row equals every background row before it
    samples; here they stay in the plan, and their value is 0 to rounding under full enumeration.
  * the shape of the result — float64 [R, n_features] for binary and regression, a list of O such arrays for multiclass and
    multilabel, `expected_value` a float or float64 [O] — is this project's choice; it was not observed from a shap run.

The constraint is applied by eliminating the last player: with Z the coalitions as 0/1 rows, Z' = Z[:, :-1] - Z[:, -1:],
A = Z'^T W Z' and P = A^-1 Z'^T W depend on the plan alone (`solve_matrix`, once per plan, on the host);
y'_s = v(s) - v(empty) - z_{s,last} (f(x) - v(empty)), phi[:-1] = P y', phi[-1] = f(x) - v(empty) - sum(phi[:-1]).

Two paths compute it:
  * device: the background and the explained frame are each transformed ONCE into resident feeds; per explained row and chunk
    of coalitions `ops.coalition_fill` writes the hybrid rows into synthetic feed blocks (a raw column's group is the model
    inputs it feeds), `DeepModel.score_batches` scores them, `ops.coalition_mean` averages over the background and
    `ops.shap_solve` applies P (csrc/coalition.hip).  Only phi, f(x) and expected_value cross to the host.
  * host: the loop a user writes by hand: per explained row and chunk build the frame of hybrid raw rows,
    `preprocessor.transform_X`, `DeepModel.predict`, a float64 mean over the background, `P @ y'` in numpy.  Any
    preprocessor, any device."""
import itertools
import os
from math import comb

import numpy as np
import pandas as pd
import torch

from . import feature_importance as FI
from .. import ops, training

SHAP_MAX_SYNTH_ROWS = 1 << 20       # synthetic rows of one chunk on the device: S_chunk * Nb <= this
HOST_MAX_SYNTH_ROWS = 1 << 16       # ... and rows of one hybrid frame on the host path
AUTO_EXTRA = 2048                   # nsamples='auto': 2 M + 2048
SINGULAR_COND = 1e12                # A is M-conditioned under full enumeration; beyond this the plan cannot carry M values


def device_shap_enabled():
    """DT_AMD_DEVICE_SHAP=0 (read at every call) keeps device='auto' on the host path"""
    return os.environ.get('DT_AMD_DEVICE_SHAP', '1') != '0'


# ---- the plan ---------------------------------------------------------------------------------------------------------------
def _budget(M, nsamples):
    if isinstance(nsamples, str):
        if nsamples != 'auto':
            raise ValueError(f"nsamples must be 'auto' or a count, got {nsamples!r}")
        budget = 2 * M + AUTO_EXTRA
    else:
        budget = int(nsamples)
    if M <= 30:
        budget = min(budget, 2 ** M - 2)
    return budget


def coalition_plan(M, nsamples='auto', random_state=0):
    """-> (masks bool [S, M], weights float64 [S]), weights.sum() == 1: every coalition is a proper non-empty subset of the M
    players, and the set is closed under complement.  M <= 1: no coalition (shapes [0, M] and [0]).
    Budget: nsamples, 'auto' = 2 M + 2048, at most 2^M - 2 for M <= 30; a budget below M cannot determine M values: ValueError.
    Sizes s = 1, 2, ... paired with M - s are COMPLETED (every subset listed, each with the Shapley kernel weight
    (M - 1) / (C(M, s) s (M - s)), normalised by the kernel's total mass) while the remaining budget covers the pair.  What
    is left of the budget is drawn with RandomState(random_state) in complementary pairs: a size among the uncompleted ones
    by their remaining kernel mass, then a uniform subset of that size; a coalition drawn again counts again.  The drawn
    coalitions share the uncompleted sizes' mass in proportion to their counts."""
    M = int(M)
    if M < 0:
        raise ValueError(f'M must not be negative, got {M}')
    if M <= 1:
        return np.zeros((0, M), dtype=bool), np.zeros(0, dtype=np.float64)
    budget = _budget(M, nsamples)
    if budget < M:
        raise ValueError(f'nsamples={nsamples!r}: {budget} coalitions cannot determine {M} Shapley values (the regression '
                         f'is singular); at least {M} are needed')
    half = M // 2                                              # sizes 1 .. ceil((M - 1) / 2); size s stands for M - s too
    paired = (M - 1) // 2                                      # sizes whose complement has another size
    size_mass = np.array([(M - 1.0) / (s * (M - s)) for s in range(1, half + 1)])
    size_mass[:paired] *= 2.0
    total = size_mass.sum()
    masks, weights, left, full = [], [], budget, 0
    for s in range(1, half + 1):
        n_pair = comb(M, s) * (2 if s <= paired else 1)
        if n_pair > left:
            break
        w = (M - 1.0) / (comb(M, s) * s * (M - s)) / total
        for sub in itertools.combinations(range(M), s):
            m = np.zeros(M, dtype=bool)
            m[list(sub)] = True
            if s <= paired:
                masks += [m, ~m]
                weights += [w, w]
            else:                                              # M even, s = M / 2: the complements are in this list themselves
                masks.append(m)
                weights.append(w)
        left -= n_pair
        full += 1
    if full < half and left >= 2:
        rng = np.random.RandomState(random_state)
        rest = size_mass[full:] / size_mass[full:].sum()
        mass_left = size_mass[full:].sum() / total
        index, counts, order = {}, [], []
        for k in rng.choice(len(rest), 4 * left, p=rest):
            if left < 2:
                break
            s = full + 1 + int(k)
            m = np.zeros(M, dtype=bool)
            m[rng.permutation(M)[:s]] = True
            for mm in (m, ~m):
                key = mm.tobytes()
                if key in index:
                    counts[index[key]] += 1
                else:
                    index[key] = len(counts)
                    counts.append(1)
                    order.append(mm)
                    left -= 1
        if counts:
            c = np.asarray(counts, dtype=np.float64)
            masks += order
            weights += list(mass_left * c / c.sum())
    masks = np.stack(masks)
    weights = np.asarray(weights, dtype=np.float64)
    return masks, weights / weights.sum()


def solve_matrix(masks, weights):
    """P float64 [M - 1, S] = A^-1 Z'^T W for Z' = Z[:, :-1] - Z[:, -1:], A = Z'^T W Z'.  ValueError when A is singular (the
    plan's coalitions do not determine M values)."""
    Z = np.asarray(masks, dtype=np.float64)
    w = np.asarray(weights, dtype=np.float64)
    Zp = Z[:, :-1] - Z[:, -1:]
    ZtW = Zp.T * w[None, :]
    A = ZtW @ Zp
    singular = f'the {len(w)} coalitions of this plan leave the regression for {Z.shape[1]} Shapley values singular; raise nsamples'
    if np.linalg.matrix_rank(A) < A.shape[0] or np.linalg.cond(A) > SINGULAR_COND:
        raise ValueError(singular)
    try:
        return np.ascontiguousarray(np.linalg.solve(A, ZtW))
    except np.linalg.LinAlgError:
        raise ValueError(singular)


def solve_host(P, masks, ey, fx, e0):
    """ey float64 [S, O], fx [O], e0 [O] -> phi float64 [O, M] in numpy (the host path's regression)"""
    z = np.asarray(masks)[:, -1].astype(np.float64)
    delta = fx - e0
    y = (ey - e0[None, :]) - z[:, None] * delta[None, :]
    head = (P @ y).T                                            # [O, M - 1]
    return np.concatenate([head, (delta - head.sum(axis=1))[:, None]], axis=1)


def background_rows(n, num_samples, random_state=0):
    """the positions of the background rows in X (None: all of X)"""
    if num_samples is None or n <= int(num_samples):
        return None
    return np.random.RandomState(random_state).permutation(n)[:int(num_samples)]


def hybrid_frame(bg, x_row, masks, players):
    """The frame of hybrid raw rows of one explained row: for every coalition of `masks` (bool [Sc, M]) the Nb rows of `bg`
    with the players' columns the coalition holds taken from `x_row` (a one-row frame); coalition-major, background-minor."""
    Sc, Nb = len(masks), len(bg)
    data = {}
    for c in bg.columns:
        col = np.tile(np.asarray(bg[c].values), Sc)
        if c in players:
            take = np.repeat(np.asarray(masks)[:, players[c]], Nb)
            col[take] = x_row[c].values[0]
        data[c] = col
    return pd.DataFrame(data, columns=bg.columns)


# ---- the explainer ------------------------------------------------------------------------------------------------------------
class DeepTablesExplainer:
    def __init__(self, dt_model, X, num_samples=50, random_state=0, device='auto'):
        if device not in ('auto', True, False):
            raise ValueError(f"device must be 'auto', True or False, got {device!r}")
        if X is None or len(X) == 0:
            raise ValueError('X can not be empty.')
        dt_model._require_model()
        self.dt_model = dt_model
        self.num_samples = num_samples
        self.random_state = random_state
        self.device = device
        self.feature_names = X.columns.to_list()
        rows = background_rows(len(X), num_samples, random_state)
        self.background = (X if rows is None else X.iloc[rows]).reset_index(drop=True)
        source_map = FI._source_map(dt_model.preprocessor)
        dm = dt_model.model
        if source_map is None:
            fed = list(self.feature_names)
        else:
            inputs = {c.name for c in dm.categorical_columns or []} | {c.name for c in dm.var_len_categorical_columns or []}
            for c in dm.continuous_columns or []:
                inputs |= set(c.column_names)
            fed = [c for c in self.feature_names if any(d in inputs for d in FI._derived(source_map, c))]
        self.players = {c: k for k, c in enumerate(fed)}        # raw column -> player number
        self.expected_value = None
        self.last_path = None
        self._plans = {}

    # -- pieces both paths share --
    def plan(self, nsamples='auto'):
        """(masks, weights, P) for this explainer's players, computed once per nsamples"""
        if nsamples not in self._plans:
            M = len(self.players)
            masks, weights = coalition_plan(M, nsamples, self.random_state)
            self._plans[nsamples] = (masks, weights, solve_matrix(masks, weights) if M >= 2 else None)
        return self._plans[nsamples]

    def _refusal(self):
        reason = FI.device_refusal(self.dt_model)
        if reason is None and self.device == 'auto' and not device_shap_enabled():
            reason = 'DT_AMD_DEVICE_SHAP=0'
        return reason

    def _result(self, phi, fx, e0):
        """phi float64 [R, O, M] over the players -> the public shape over the features"""
        R, O, _ = phi.shape
        full = np.zeros((R, O, len(self.feature_names)), dtype=np.float64)
        for c, k in self.players.items():
            full[:, :, self.feature_names.index(c)] = phi[:, :, k]
        self.fx = fx[:, 0] if O == 1 else fx
        if O == 1:
            self.expected_value = float(e0[0])
            return full[:, 0, :]
        self.expected_value = np.asarray(e0, dtype=np.float64)
        return [np.ascontiguousarray(full[:, o, :]) for o in range(O)]

    def get_shap_values(self, X_to_explain, nsamples='auto', batch_size=None, on_chunk=None):
        """-> float64 [R, n_features] (binary, regression) or a list of O such arrays; sets `expected_value` and `last_path`.
        batch_size None: 128 on the host path, min(rows, 8192) on the device path; the result does not depend on it.
        on_chunk(r, s0, s1, blocks, outputs) sees every chunk of coalitions [s0, s1) of explained row r: on the device path
        `blocks` are the synthetic feed blocks and `outputs` the device tensor of the model's outputs; on the host path
        `blocks` is the frame of hybrid raw rows and `outputs` the numpy array `predict` returned."""
        if list(X_to_explain.columns) != self.feature_names:
            raise ValueError(f'X_to_explain has the columns {list(X_to_explain.columns)}, the explainer {self.feature_names}')
        feeds = None
        if self.device is not False:
            reason = self._refusal()
            if reason is None:
                feeds = (FI.make_feed(self.dt_model, self.background, None),
                         FI.make_feed(self.dt_model, X_to_explain, None))
                reason = FI.feed_refusal(self.dt_model, feeds[0]) or FI.feed_refusal(self.dt_model, feeds[1])
            if reason is not None:
                if self.device is True:
                    raise ValueError(f'device=True: {reason}')
                feeds = None
        plan = self.plan(nsamples)
        if feeds is not None:
            bs = None if batch_size is None else int(batch_size)
            phi, fx, e0 = feed_values(self.dt_model, feeds[0], feeds[1], self._groups(feeds[0]), plan, bs, on_chunk)
            self.last_path = 'device'
        else:
            bs = FI.HOST_BATCH_SIZE if batch_size is None else int(batch_size)
            phi, fx, e0 = host_values(self.dt_model, self.background, X_to_explain, self.players, plan, bs, on_chunk)
            self.last_path = 'host'
        return self._result(phi, fx, e0)

    def _groups(self, feed):
        """per feed block an int32 [C] numpy array: the player that owns each column, -1 for none"""
        dm = self.dt_model.model
        source_map = FI._source_map(self.dt_model.preprocessor)
        groups = [np.full(int(b.shape[1]), -1, dtype=np.int32) for b in feed.blocks]
        for raw, k in self.players.items():
            for b, cols in FI.feed_targets(dm, feed, source_map, [raw]).items():
                if (groups[b][cols] != -1).any():
                    raise ValueError(f'{raw!r} feeds a model input another raw column feeds too')
                groups[b][cols] = k
        return groups


def _outputs_2d(out):
    return out.reshape(out.shape[0], -1)


def host_values(dt_model, bg, X_to_explain, players, plan, batch_size, on_chunk=None):
    """The loop a user writes by hand -> (phi float64 [R, O, M], fx float64 [R, O], e0 float64 [O])"""
    dm, pp = dt_model.model, dt_model.preprocessor
    masks, weights, P = plan
    M, S, Nb, R = len(players), len(masks), len(bg), len(X_to_explain)

    def f(frame):
        return _outputs_2d(np.asarray(dm.predict(pp.transform_X(frame), batch_size=batch_size)))

    e0 = f(bg).astype(np.float64).mean(axis=0)
    fx = f(X_to_explain).astype(np.float64) if R else np.zeros((0, len(e0)))
    O = len(e0)
    phi = np.zeros((R, O, M), dtype=np.float64)
    if M == 0:
        return phi, fx, e0
    if M == 1:
        phi[:, :, 0] = fx - e0[None, :]
        return phi, fx, e0
    step = max(1, HOST_MAX_SYNTH_ROWS // Nb)
    for r in range(R):
        x_row = X_to_explain.iloc[r:r + 1]
        ey = np.zeros((S, O), dtype=np.float64)
        for s0 in range(0, S, step):
            s1 = min(S, s0 + step)
            frame = hybrid_frame(bg, x_row, masks[s0:s1], players)
            out = f(frame)
            if on_chunk is not None:
                on_chunk(r, s0, s1, frame, out)
            ey[s0:s1] = out.astype(np.float64).reshape(s1 - s0, Nb, O).mean(axis=1)
        phi[r] = solve_host(P, masks, ey, fx[r], e0)
    return phi, fx, e0


def feed_values(dt_model, bg_feed, x_feed, groups, plan, batch_size=None, on_chunk=None):
    """The device path over two ready feeds (GPU tensors: the HIP kernels of csrc/coalition.hip; CPU tensors: the torch
    branches of ops.coalition_fill / coalition_mean / shap_solve) -> (phi float64 [R, O, M], fx float64 [R, O], e0 float64
    [O]) as numpy arrays.  groups: per feed block the int32 [C] player of every column.  Neither feed is written."""
    for feed in (bg_feed, x_feed):
        reason = FI.feed_refusal(dt_model, feed)
        if reason is not None:
            raise ValueError(f'Shapley values on the device: {reason}')
    dm = dt_model.model
    masks, weights, P = plan
    S, M = masks.shape
    Nb, R = bg_feed.n, x_feed.n
    dev = bg_feed.blocks[0].device
    kinds = bg_feed.kinds

    def score(feed):
        bs = min(feed.n, FI.DEVICE_BATCH_SIZE) if batch_size is None else batch_size
        return _outputs_2d(dm.score_batches(feed, bs)).float().contiguous()

    e0 = ops.coalition_mean(score(bg_feed), Nb)[0]                              # [O]
    O = int(e0.shape[0])
    fx = ops.coalition_mean(score(x_feed), 1) if R else torch.zeros((0, O), dtype=torch.float64, device=dev)
    if M <= 1 or R == 0:
        phi = torch.zeros((R, O, M), dtype=torch.float64, device=dev)
        if M == 1:
            phi[:, :, 0] = fx - e0[None, :]
    else:
        packed = ops.pack_coalitions(masks).to(dev)
        P_dev = torch.from_numpy(P).to(dev)
        groups_dev = [torch.from_numpy(g).to(dev) for g in groups]
        step = max(1, SHAP_MAX_SYNTH_ROWS // Nb)
        ey = torch.empty((R, S, O), dtype=torch.float64, device=dev)
        for r in range(R):
            for s0 in range(0, S, step):
                s1 = min(S, s0 + step)
                blocks = [ops.coalition_fill(xb[r], bb, packed, M, s0, s1, gd, group_host=gh)
                          for xb, bb, gd, gh in zip(x_feed.blocks, bg_feed.blocks, groups_dev, groups)]
                out = score(training.TableBatches.from_device(blocks, kinds))
                if on_chunk is not None:
                    on_chunk(r, s0, s1, blocks, out)
                ey[r, s0:s1] = ops.coalition_mean(out, Nb)
        phi = ops.shap_solve(P_dev, packed, M, ey, fx.contiguous(), e0.contiguous())
    return phi.cpu().numpy(), fx.cpu().numpy(), e0.cpu().numpy()
