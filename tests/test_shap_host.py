# -*- coding:utf-8 -*-
"""CPU: Shapley values (deeptables_amd/utils/shap.py) — the coalition plan, the background rows, the host path against exact
Shapley values of a value function evaluated by an independent hand loop, the feed path on CPU tensors (the torch branches of
ops.coalition_fill / coalition_mean / shap_solve), routing, and the argument checks of the three entry points of
csrc/coalition.hip.

The models run on CPU tensors with torch restatements of the kernels a ['dnn_nets'] forward launches
(tests/feature_importance_support.py); nothing here launches."""
import ctypes
from math import comb

import numpy as np
import pytest
import torch

from deeptables_amd.utils import shap as SH
from tests import feature_importance_support as FS
from tests import shap_support as SS


@pytest.fixture(scope='module', autouse=True)
def _cpu_kernels():
    mp = pytest.MonkeyPatch()
    FS.cpu_kernels(mp)
    yield
    mp.undo()


@pytest.fixture(scope='module')
def fitted(_cpu_kernels):
    out = {}
    for task in ('binary', 'multiclass', 'regression'):
        df, y = FS.task_frame(task)
        out[task] = (FS.fit_cpu(df, y, FS.task_config(task), epochs=10), df, y)
    return out


@pytest.fixture(scope='module')
def fitted_mixed(_cpu_kernels):
    df = FS.mixed_frame(400)
    return SS.fit_cpu_with_var_len(df, SS.mixed_labels(df), FS.mixed_config(metrics=['auc']), epochs=3), df


# ---- 1. the plan --------------------------------------------------------------------------------------------------------------
def _closed_under_complement(masks):
    keys = {m.tobytes() for m in masks}
    return all((~m).tobytes() in keys for m in masks)


@pytest.mark.parametrize('M', range(2, 12))
def test_plan_enumerates_every_coalition_up_to_11_players(M):
    masks, w = SH.coalition_plan(M)
    assert masks.dtype == bool and masks.shape == (2 ** M - 2, M) and w.dtype == np.float64 and w.shape == (2 ** M - 2,)
    assert len({m.tobytes() for m in masks}) == 2 ** M - 2
    size = masks.sum(1)
    assert size.min() >= 1 and size.max() <= M - 1 and _closed_under_complement(masks)
    kernel = np.array([(M - 1) / (comb(M, s) * s * (M - s)) for s in size])
    assert np.abs(w - kernel / kernel.sum()).max() <= 1e-15 and abs(w.sum() - 1) <= 1e-15
    P = SH.solve_matrix(masks, w)
    assert P.shape == (M - 1, 2 ** M - 2) and P.dtype == np.float64


def test_plan_in_the_sampled_regime():
    M, budget = 20, 600
    masks, w = SH.coalition_plan(M, nsamples=budget, random_state=0)
    assert len(masks) <= budget and len({m.tobytes() for m in masks}) == len(masks)
    assert abs(w.sum() - 1) <= 1e-15 and (w > 0).all() and _closed_under_complement(masks)
    size = masks.sum(1)
    assert size.min() >= 1 and size.max() <= M - 1
    # 2 * 20 + 2 * 190 = 420 <= 600 < 420 + 2 * 1140: sizes 1, 2 (and 19, 18) are completed, no other
    counts = np.bincount(size, minlength=M + 1)
    total = sum((M - 1) / (s * (M - s)) for s in range(1, M))
    for s in (1, 2, M - 2, M - 1):
        assert counts[s] == comb(M, s)
        assert np.abs(w[size == s] - (M - 1) / (comb(M, s) * s * (M - s)) / total).max() <= 1e-15
    for s in range(3, M - 2):
        assert 0 < counts[s] < comb(M, s)
    again = SH.coalition_plan(M, nsamples=budget, random_state=0)
    assert np.array_equal(again[0], masks) and np.array_equal(again[1], w)
    other = SH.coalition_plan(M, nsamples=budget, random_state=1)
    assert other[0].shape != masks.shape or not np.array_equal(other[0], masks)
    assert SH.solve_matrix(masks, w).shape == (M - 1, len(masks))


def test_plan_edge_cases():
    for M in (0, 1):
        masks, w = SH.coalition_plan(M)
        assert masks.shape == (0, M) and w.shape == (0,)
    masks, w = SH.coalition_plan(2)
    assert sorted(m.tolist() for m in masks) == [[False, True], [True, False]] and w.tolist() == [0.5, 0.5]
    assert len(SH.coalition_plan(40)[0]) <= 2 * 40 + 2048
    assert len(SH.coalition_plan(12)[0]) <= 2 * 12 + 2048
    with pytest.raises(ValueError, match='singular'):
        SH.coalition_plan(20, nsamples=19)
    with pytest.raises(ValueError, match='nsamples'):
        SH.coalition_plan(5, nsamples='many')
    with pytest.raises(ValueError, match='singular'):                  # enough rows, but they never tell players 1 and 2 apart
        SH.solve_matrix(np.array([[1, 0, 0], [0, 1, 1], [1, 1, 1]], dtype=bool), np.ones(3) / 3)


def test_pack_coalitions():
    from deeptables_amd import ops
    rng = np.random.default_rng(0)
    for M in (1, 31, 32, 33, 70):
        masks = rng.random((9, M)) < 0.5
        words = ops.pack_coalitions(masks)
        assert words.dtype == torch.int32 and tuple(words.shape) == (9, (M + 31) // 32)
        u = words.numpy().view(np.uint32)
        for s in range(9):
            for g in range(M):
                assert bool(u[s, g // 32] >> np.uint32(g % 32) & np.uint32(1)) == bool(masks[s, g])
            for g in range(M, 32 * u.shape[1]):
                assert not u[s, g // 32] >> np.uint32(g % 32) & np.uint32(1)


# ---- 2. the background ------------------------------------------------------------------------------------------------------
def test_background_rows_are_sklearn_resample(fitted):
    from sklearn.utils import resample
    dt, df, _ = fitted['binary']
    for k in (8, 50):
        ex = SH.DeepTablesExplainer(dt, df, num_samples=k)
        want = resample(df, n_samples=k, replace=False, random_state=0)
        assert ex.background.equals(want.reset_index(drop=True))
        assert np.array_equal(SH.background_rows(len(df), k), want.index.values)
    assert SH.DeepTablesExplainer(dt, df, num_samples=None).background.equals(df)
    assert SH.DeepTablesExplainer(dt, df.iloc[:30], num_samples=50).background.equals(df.iloc[:30])
    assert SH.DeepTablesExplainer(dt, df).num_samples == 50
    assert SH.DeepTablesExplainer(dt, df).feature_names == df.columns.to_list()


# ---- 3. / 4. exact Shapley values ---------------------------------------------------------------------------------------------
def _explain(dt, df, rows, **kw):
    ex = SH.DeepTablesExplainer(dt, df, num_samples=8)
    X = df.iloc[rows]
    masks = ex.plan('auto')[0]
    hook = SS.ChunkOutputs(masks, len(ex.background))
    phi = ex.get_shap_values(X, on_chunk=hook, **kw)
    return ex, X, phi, hook


def test_host_path_gives_exact_shapley_values_on_task_frame(fitted):
    dt, df, _ = fitted['binary']
    ex, X, phi, hook = _explain(dt, df, [3, 77, 410])
    assert ex.last_path == 'host' and list(ex.players) == df.columns.to_list() and len(ex.plan('auto')[0]) == 126
    assert phi.dtype == np.float64 and phi.shape == (3, 7) and isinstance(ex.expected_value, float)
    hand = SS.hand_outputs(dt, ex.background, X, list(ex.players))
    SS.check_against_exact(ex, X, phi, hook, hand, 'host binary')
    assert np.abs(phi).max() > 1e-3
    # the result does not depend on the batch size or the chunking beyond the outputs' own differences
    small = SH.HOST_MAX_SYNTH_ROWS
    try:
        SH.HOST_MAX_SYNTH_ROWS = 8 * 10
        ex2, _, phi2, hook2 = _explain(dt, df, [3, 77, 410], batch_size=50)
    finally:
        SH.HOST_MAX_SYNTH_ROWS = small
    assert len(hook2.blocks) == 3 * 13 and len(hook.blocks) == 3
    SS.check_against_exact(ex2, X, phi2, hook2, hand, 'host binary, 10 coalitions a chunk')


def test_host_path_gives_exact_shapley_values_on_mixed_frame(fitted_mixed):
    dt, df = fitted_mixed
    ex, X, phi, hook = _explain(dt, df, [0, 5, 123])
    assert list(ex.players) == ['c_str', 'c_int', 'f_nan', 'f_two', 'tags'] and ex.last_path == 'host'
    hand = SS.hand_outputs(dt, ex.background, X, list(ex.players))
    SS.check_against_exact(ex, X, phi, hook, hand, 'host mixed')
    k = {c: i for i, c in enumerate(ex.feature_names)}
    assert (phi[:, [k['const'], k['excluded']]] == 0.0).all() and np.abs(phi).max() > 1e-4


# ---- 5. other tasks -------------------------------------------------------------------------------------------------------------
def test_multiclass_returns_one_array_per_class_and_regression_one(fitted):
    dt, df, _ = fitted['multiclass']
    ex, X, phi, hook = _explain(dt, df, [1, 2])
    assert isinstance(phi, list) and len(phi) == dt.num_classes == 3 and all(p.shape == (2, 7) for p in phi)
    assert ex.expected_value.shape == (3,) and ex.expected_value.dtype == np.float64
    hand = SS.hand_outputs(dt, ex.background, X, list(ex.players))
    SS.check_against_exact(ex, X, phi, hook, hand, 'host multiclass')
    assert np.abs(sum(phi)).max() <= 1e-6                              # the classes' probabilities sum to one (float32)
    dt, df, _ = fitted['regression']
    ex, X, phi, hook = _explain(dt, df, [1, 2])
    assert isinstance(phi, np.ndarray) and phi.shape == (2, 7) and isinstance(ex.expected_value, float)
    SS.check_against_exact(ex, X, phi, hook, SS.hand_outputs(dt, ex.background, X, list(ex.players)), 'host regression')


def test_one_player_and_none(fitted):
    from deeptables_amd.models import ModelConfig
    dt, df, y = fitted['binary']
    cols = ['job', 'marital', 'region', 'flag', 'balance', 'rate']
    conf = ModelConfig(nets=['dnn_nets'], dnn_params=FS.TOWER, embedding_dropout=0, exclude_columns=cols,
                       auto_categorize=False, earlystopping_patience=0)
    one = FS.fit_cpu(df, y, conf, epochs=1)
    ex = SH.DeepTablesExplainer(one, df, num_samples=8)
    assert list(ex.players) == ['age']
    phi = ex.get_shap_values(df.iloc[:4])
    k = df.columns.to_list().index('age')
    assert np.array_equal(phi[:, k], ex.fx - ex.expected_value) and (np.delete(phi, k, axis=1) == 0.0).all()
    ex.players = {}
    ex._plans = {}
    assert (ex.get_shap_values(df.iloc[:4]) == 0.0).all()


# ---- the feed path on CPU tensors ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', ['binary', 'multiclass', 'mixed'])
def test_feed_path_on_cpu_tensors_is_the_host_path(fitted, fitted_mixed, which):
    from deeptables_amd.utils import feature_importance as FI
    dt, df = fitted_mixed if which == 'mixed' else fitted[which][:2]
    ex = SH.DeepTablesExplainer(dt, df, num_samples=8)
    X = df.iloc[[0, 5, 123]]
    plan = ex.plan(60 if which == 'binary' else 'auto')
    Nb = len(ex.background)
    host_hook, feed_hook = SS.ChunkOutputs(plan[0], Nb), SS.ChunkOutputs(plan[0], Nb)
    hp, hfx, he0 = SH.host_values(dt, ex.background, X, ex.players, plan, 128, host_hook)
    bg_feed, x_feed = FI.make_feed(dt, ex.background, None), FI.make_feed(dt, X, None)
    before = [b.clone() for b in bg_feed.blocks + x_feed.blocks]
    fp, ffx, fe0 = SH.feed_values(dt, bg_feed, x_feed, ex._groups(bg_feed), plan, None, feed_hook)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(bg_feed.blocks + x_feed.blocks, before))
    # every synthetic block is transform_X of the host path's hybrid frame, bit for bit
    for (r, s0, s1, frame), (r2, t0, t1, blocks) in zip(host_hook.blocks, feed_hook.blocks):
        assert (r, s0, s1) == (r2, t0, t1)
        want = FI.make_feed(dt, frame, None)
        assert len(want.blocks) == len(blocks)
        for a, b in zip(want.blocks, blocks):
            assert a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))
    delta = max(float(np.abs(o - host_hook.seen[k]).max()) for k, o in feed_hook.seen.items())
    bar = 2 * delta + 1e-12 * max(np.abs(o).max() for o in host_hook.seen.values())
    assert np.abs(fp - hp).max() <= bar, (np.abs(fp - hp).max(), bar, delta)
    assert np.abs(ffx - hfx).max() <= delta + 1e-12 and np.abs(fe0 - he0).max() <= delta + 1e-12
    assert fp.shape == (3, 3 if which == 'multiclass' else 1, len(ex.players))


# ---- routing --------------------------------------------------------------------------------------------------------------------
def test_routing_and_refusals(fitted, monkeypatch):
    from deeptables_amd.utils import feature_importance as FI
    dt, df, _ = fitted['binary']
    X = df.iloc[:2]
    kw = dict(num_samples=4)
    assert SH.DeepTablesExplainer(dt, df, **kw).device == 'auto'
    ex = SH.DeepTablesExplainer(dt, df, **kw)
    host = ex.get_shap_values(X, nsamples=40)
    assert ex.last_path == 'host'                                                            # 'auto' on a CPU model
    with pytest.raises(ValueError, match='device=True: the model is on cpu, not on a GPU'):
        SH.DeepTablesExplainer(dt, df, device=True, **kw).get_shap_values(X, nsamples=40)
    with pytest.raises(ValueError, match='device must be'):
        SH.DeepTablesExplainer(dt, df, device='gpu')
    with pytest.raises(ValueError, match='columns'):
        ex.get_shap_values(X[['age', 'job']])
    with monkeypatch.context() as mp:
        mp.setattr(FI, 'device_refusal', lambda dt_model, feed=None: None)
        ex = SH.DeepTablesExplainer(dt, df, **kw)
        dev = ex.get_shap_values(X, nsamples=40)
        assert ex.last_path == 'device' and np.abs(dev - host).max() <= 1e-5
        mp.setenv('DT_AMD_DEVICE_SHAP', '0')
        ex.get_shap_values(X, nsamples=40)
        assert ex.last_path == 'host'
        ex = SH.DeepTablesExplainer(dt, df, device=True, **kw)                              # the switch is for 'auto'
        ex.get_shap_values(X, nsamples=40)
        assert ex.last_path == 'device'
    ex = SH.DeepTablesExplainer(dt, df, device=False, **kw)
    assert np.array_equal(ex.get_shap_values(X, nsamples=40), host) and ex.last_path == 'host'


# ---- 6. C-ABI -----------------------------------------------------------------------------------------------------------------
def test_coalition_entry_points_check_their_arguments_before_any_launch():
    from deeptables_amd import _lib
    lib = _lib.lib()
    P = ctypes.c_void_p(0x10000)                    # never dereferenced: every call below returns before a launch
    ODD = ctypes.c_void_p(0x10002)
    good = np.array([0, -1, 2, 2], dtype=np.int32)
    G = ctypes.c_void_p(good.ctypes.data)

    def fill(x=P, bg=P, Nb=3, C=4, masks=P, S=6, M=3, s0=1, s1=5, group=P, group_host=G, out=P):
        return lib.dt_coalition_fill(x, bg, Nb, C, masks, S, M, s0, s1, group, group_host, out, None)

    def mean(out=P, nseg=5, Nb=3, O=2, ey=P):
        return lib.dt_coalition_mean(out, nseg, Nb, O, ey, None)

    def solve(Pm=P, masks=P, S=6, M=3, ey=P, fx=P, e0=P, R=2, O=1, phi=P):
        return lib.dt_shap_solve(Pm, masks, S, M, ey, fx, e0, R, O, phi, None)

    def rejected(name, f, bad):
        for kw in bad:
            assert f(**kw) == -1, (name, kw)
            assert name.encode() in lib.dt_last_error(), (name, kw, lib.dt_last_error())

    for kw in (dict(s0=2, s1=2), dict(Nb=0), dict(C=0), dict(S=0, s0=0, s1=0)):
        assert fill(**kw) == 0, kw
    bad = [dict(Nb=-1), dict(C=-1), dict(S=-1), dict(M=0), dict(M=-2), dict(s0=-1), dict(s0=3, s1=2), dict(s1=7)]
    bad += [{p: None} for p in ('x', 'bg', 'masks', 'group', 'group_host', 'out')]
    bad += [{p: ODD} for p in ('x', 'bg', 'masks', 'group', 'out')]
    bad += [dict(s0=2, s1=2, x=None), dict(Nb=0, M=0)]                          # an empty size does not excuse the rest
    rejected('dt_coalition_fill', fill, bad)
    for values in ([0, 1, 3, 2], [0, -2, 1, 2], [2 ** 31 - 1, 0, 0, 0], [0, 0, 0, -2 ** 31]):
        g = np.array(values, dtype=np.int32)
        rejected('dt_coalition_fill', fill, [dict(group_host=ctypes.c_void_p(g.ctypes.data)),
                                             dict(group_host=ctypes.c_void_p(g.ctypes.data), s0=2, s1=2)])
        assert b'group[' in lib.dt_last_error()
    assert fill(M=33, group_host=ctypes.c_void_p(np.array([32, 0, -1, 31], dtype=np.int32).ctypes.data), s0=0, s1=0) == 0

    for kw in (dict(nseg=0), dict(O=0)):
        assert mean(**kw) == 0, kw
    rejected('dt_coalition_mean', mean, [dict(nseg=-1), dict(Nb=0), dict(Nb=-1), dict(O=-1), dict(out=None), dict(ey=None),
                                         dict(out=ODD), dict(ey=ctypes.c_void_p(0x10004)), dict(nseg=0, out=None),
                                         dict(nseg=2 ** 62, Nb=2 ** 40)])

    for kw in (dict(R=0), dict(O=0)):
        assert solve(**kw) == 0, kw
    bad = [dict(S=0), dict(S=-1), dict(M=1), dict(M=0), dict(R=-1), dict(O=-1), dict(R=0, Pm=None), dict(R=2 ** 62, O=8)]
    bad += [{p: None} for p in ('Pm', 'masks', 'ey', 'fx', 'e0', 'phi')]
    bad += [{p: ctypes.c_void_p(0x10004)} for p in ('Pm', 'ey', 'fx', 'e0', 'phi')] + [dict(masks=ODD)]
    rejected('dt_shap_solve', solve, bad)


def test_ops_wrappers_reject_bad_arguments():
    from deeptables_amd import ops
    bg = torch.zeros(3, 4, dtype=torch.int32)
    x = torch.ones(4, dtype=torch.int32)
    masks = ops.pack_coalitions(np.array([[1, 0, 1], [0, 1, 0]], dtype=bool))
    group = torch.tensor([0, -1, 2, 2], dtype=torch.int32)
    out = ops.coalition_fill(x, bg, masks, 3, 0, 2, group)
    assert out.view(2, 3, 4)[0, 0].tolist() == [1, 0, 1, 1] and out.view(2, 3, 4)[1, 2].tolist() == [0, 0, 0, 0]
    assert ops.coalition_fill(x, bg, masks, 3, 1, 1, group).shape == (0, 4)
    for g in ([0, -1, 3, 2], [0, -2, 1, 2]):
        with pytest.raises(ValueError, match='group entries'):
            ops.coalition_fill(x, bg, masks, 3, 0, 2, torch.tensor(g, dtype=torch.int32))
    with pytest.raises(ValueError, match='coalitions'):
        ops.coalition_fill(x, bg, masks, 3, 1, 3, group)
    with pytest.raises(ValueError, match='4-byte'):
        ops.coalition_fill(x.long(), bg.long(), masks, 3, 0, 2, group)
    with pytest.raises(ValueError, match='masks'):
        ops.coalition_fill(x, bg, masks, 40, 0, 2, group)
    with pytest.raises(ValueError, match='coalition_mean'):
        ops.coalition_mean(torch.zeros(7, 2), 3)
    with pytest.raises(ValueError, match='shap_solve'):
        ops.shap_solve(torch.zeros(2, 3, dtype=torch.float64), masks, 3, torch.zeros(1, 2, 1, dtype=torch.float64),
                       torch.zeros(1, 1, dtype=torch.float64), torch.zeros(1, dtype=torch.float64))
