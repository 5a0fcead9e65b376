# -*- coding:utf-8 -*-
"""GPU: permutation feature importance on the device — dt_column_gather / dt_column_swap (csrc/feed_columns.hip) against torch
indexing as int32 words at the launch's edges, the device path of utils/feature_importance.py against its host path with the
same seed, the feed bit for bit afterwards, and no [n]-sized read in a pass."""
import numpy as np
import pandas as pd
import pytest
import torch

from deeptables_amd.utils import feature_importance as F
from tests import feature_importance_support as FS

pytestmark = pytest.mark.gpu

SENTINEL = 0x5EA7BEE
FRAME = 64                      # words of sentinel on either side of every buffer
GRID_CAP_BLOCKS = 2048          # csrc/feed_columns.hip kColumnMaxBlocks: one row past it strides


# ---- 1. the kernels -----------------------------------------------------------------------------------------------------------
def _framed(dev, numel, skew=0):
    """-> (the whole sentinel-filled allocation, a [numel] int32 view FRAME words in; skew: words off 16-byte alignment)"""
    raw = torch.full((numel + 2 * FRAME + 4,), SENTINEL, dtype=torch.int32, device=dev)
    assert raw.data_ptr() % 16 == 0
    return raw, raw[FRAME + skew:FRAME + skew + numel]


def _words(kind, N, C, g):
    """[N, C] int32 words: random ids, or float32 bit patterns with NaNs of distinct payloads, +-0.0, denormals and +-Inf"""
    if kind == 'int32':
        return torch.randint(-2 ** 31, 2 ** 31 - 1, (N, C), generator=g, dtype=torch.int64).to(torch.int32)
    x = torch.randn(N * C, generator=g)
    special = torch.tensor([0x7FC00001, 0x7FC12345, 0x7F800001, -0x3FFFFF, 0x00000000, -0x80000000, 0x00000001, 0x007FFFFF,
                            -0x7FFFFFFF, 0x7F800000, -0x00800000], dtype=torch.int64).to(torch.int32)
    w = x.view(torch.int32).clone()
    pos = torch.randperm(N * C, generator=g)[:max(1, (N * C) // 3)]
    w[pos] = special[torch.arange(pos.numel()) % special.numel()]
    if N * C >= special.numel():
        assert torch.isnan(w.view(torch.float32)).any()
    return w.view(N, C)


def _perms(N, g):
    ident = torch.arange(N, dtype=torch.int64)
    rnd = torch.randperm(N, generator=g)
    fixed = rnd.clone()
    fixed[::3] = ident[::3]                          # (not a permutation any more; the gather does not care) fixed points
    fixed_perm = ident.clone()
    k = N // 2
    fixed_perm[:k] = ident[:k][torch.randperm(k, generator=g)]          # a permutation with fixed points: the upper half
    oob = rnd.clone()
    oob[0] = -1
    oob[N // 2] = N
    oob[N - 1] = 2 ** 40
    return {'identity': ident, 'reversal': ident.flip(0), 'random': rnd, 'fixed_points': fixed_perm, 'repeats': fixed,
            'out_of_range': oob}


def _run_case(dev, words, col0, width, perm, skew=0):
    """gather + swap + swap on framed device buffers against torch indexing -> nothing (asserts)"""
    from deeptables_amd._lib import lib, ptr, stream_ptr
    N, C = words.shape
    raw_b, block = _framed(dev, N * C, skew)
    raw_o, out = _framed(dev, N * width, skew)
    block.copy_(words.reshape(-1).to(dev))
    raw_b0, raw_o0 = raw_b.clone(), raw_o.clone()
    perm_d = perm.to(dev)
    src = torch.where((perm < 0) | (perm >= N), torch.arange(N, dtype=torch.int64), perm)      # out of range: the own row
    want = words[src][:, col0:col0 + width]
    h = lib()
    assert h.dt_column_gather(ptr(block), N, C, col0, width, ptr(perm_d), ptr(out), stream_ptr()) == 0, h.dt_last_error()
    assert torch.equal(raw_b, raw_b0)                                           # the block is only read
    assert torch.equal(out.view(N, width).cpu(), want)
    assert torch.equal(raw_o[:FRAME + skew], raw_o0[:FRAME + skew]) and \
        torch.equal(raw_o[FRAME + skew + N * width:], raw_o0[FRAME + skew + N * width:])
    assert h.dt_column_swap(ptr(block), N, C, col0, width, ptr(out), stream_ptr()) == 0, h.dt_last_error()
    now = block.view(N, C).cpu()
    expect = words.clone()
    expect[:, col0:col0 + width] = want
    assert torch.equal(now, expect)                                             # every other column unchanged
    assert torch.equal(out.view(N, width).cpu(), words[:, col0:col0 + width])   # buf holds the originals
    for raw, raw0, numel in ((raw_b, raw_b0, N * C), (raw_o, raw_o0, N * width)):
        assert torch.equal(raw[:FRAME + skew], raw0[:FRAME + skew]) and \
            torch.equal(raw[FRAME + skew + numel:], raw0[FRAME + skew + numel:])
    assert h.dt_column_swap(ptr(block), N, C, col0, width, ptr(out), stream_ptr()) == 0, h.dt_last_error()
    assert torch.equal(raw_b, raw_b0)                                           # bit-identical again, frames included


def _column_windows(C):
    """(col0, width): width in {1, 3, C}, col0 first, middle and last where the width fits"""
    out = set()
    for width in {1, 3, C}:
        if width <= C:
            for col0 in {0, (C - width) // 2, C - width}:
                out.add((col0, width))
    return sorted(out)


@pytest.mark.parametrize('kind', ['int32', 'float32'])
@pytest.mark.parametrize('N', [1, 255, 256, 257])
def test_column_kernels_against_torch_indexing(dev, N, kind):
    g = torch.Generator().manual_seed(100 + N)
    for C in (1, 3, 26):
        words = _words(kind, N, C, g)
        perms = _perms(N, g)
        for col0, width in _column_windows(C):
            for name, perm in perms.items():
                _run_case(dev, words, col0, width, perm)
            _run_case(dev, words, col0, width, perms['random'], skew=1)         # 4-byte, not 16-byte aligned: the same bits


@pytest.mark.parametrize('kind', ['int32', 'float32'])
def test_column_kernels_16_byte_path_and_its_misaligned_twin(dev, kind):
    """C, col0 and width multiples of 4 on 16-byte aligned buffers move uint4 words (one per row: width 4; several: width 8,
    12); the same call on buffers one word off takes the 4-byte kernels and gives the same bits"""
    g = torch.Generator().manual_seed(7)
    for N in (1, 255, 257):
        for C, windows in ((4, [(0, 4)]), (8, [(0, 4), (4, 4), (0, 8)]), (16, [(4, 8), (4, 12), (12, 4)])):
            words = _words(kind, N, C, g)
            perms = _perms(N, g)
            for col0, width in windows:
                for name in ('random', 'out_of_range', 'reversal'):
                    _run_case(dev, words, col0, width, perms[name])
                    _run_case(dev, words, col0, width, perms[name], skew=1)


def test_column_kernels_one_row_past_the_grid_cap(dev):
    """N = 2048 blocks x 256 threads + 1 rows of one column: the last row is reached by the stride, not by the grid"""
    N = GRID_CAP_BLOCKS * 256 + 1
    g = torch.Generator().manual_seed(9)
    words = _words('int32', N, 1, g)
    rnd = torch.randperm(N, generator=g)
    _run_case(dev, words, 0, 1, rnd)
    _run_case(dev, words, 0, 1, torch.arange(N, dtype=torch.int64).flip(0))


def test_permute_columns_splits_runs_and_restores(dev):
    from deeptables_amd import ops
    g = torch.Generator().manual_seed(3)
    for dtype in (torch.int32, torch.float32):
        host = _words('int32' if dtype == torch.int32 else 'float32', 300, 9, g)
        block = host.to(dev).view(dtype)
        perm = torch.randperm(300, generator=g)
        h = ops.permute_columns(block, [7, 1, 2, 5, 8], perm.to(dev))
        assert h.runs == [(1, 2), (5, 1), (7, 2)]
        want = host.clone()
        want[:, [1, 2, 5, 7, 8]] = host[perm][:, [1, 2, 5, 7, 8]]
        assert torch.equal(block.view(torch.int32).cpu(), want)
        h.restore()
        h.restore()
        assert torch.equal(block.view(torch.int32).cpu(), host)
    with pytest.raises(ValueError, match='4-byte words'):
        ops.permute_columns(torch.zeros(4, 2, dtype=torch.int64, device=dev), [0], torch.arange(4, device=dev))


# ---- 2. device path against host path -----------------------------------------------------------------------------------------
def _fit(df, y, conf, epochs=2):
    from deeptables_amd import functional
    from deeptables_amd.models import DeepTable
    functional.set_seed(5)
    dt = DeepTable(config=conf)
    dt.fit(df, y, batch_size=64, epochs=epochs, verbose=0)
    return dt


@pytest.fixture(scope='module')
def deepfm(dev):
    """DeepFM over 4 categorical + 3 continuous columns, 600 rows, binary: a graph with a fused inference plan"""
    from deeptables_amd.models import ModelConfig, deepnets
    df, y = FS.task_frame('binary')
    conf = ModelConfig(nets=deepnets.DeepFM, metrics=['auc', 'log_loss', 'accuracy'], earlystopping_patience=0,
                       fixed_embedding_dim=True, embeddings_output_dim=8, embedding_dropout=0)
    dt = _fit(df, y, conf)
    assert dt.model.inference_plan() is not None
    return dt, df, y


def _compare_paths(dt, df, y, metrics, n_iter=2, seed=21, batch_size=256, columns=None):
    """device=True against device=False with the same seed and batches -> the device result per metric.  Both paths' outputs
    come from the same kernels on the same rows, so every decrease is within twice the metric's own device-vs-host bar."""
    n_out = len(df) * (1 if dt.task != 'multiclass' else 1)
    out = {}
    for metric in metrics:
        for mode in ('min', 'max'):
            kw = dict(n_iter=n_iter, mode=mode, random_state=seed, batch_size=batch_size, columns=columns)
            host = F.permutation_scores(dt, df, y, metric, device=False, **kw)
            devc = F.permutation_scores(dt, df, y, metric, device=True, **kw)
            auto = F.permutation_scores(dt, df, y, metric, **kw)
            assert host['path'] == 'host' and devc['path'] == 'device' and auto['path'] == 'device'
            assert np.array_equal(auto['score_decreases'], devc['score_decreases']) and auto['base_score'] == devc['base_score']
            hb, hd, dd = host['base_score'], host['score_decreases'], devc['score_decreases']
            tol = np.array([[FS.decrease_tolerance(metric, n_out, hb, hd[i, c]) for c in range(hd.shape[1])]
                            for i in range(hd.shape[0])])
            diff = np.abs(dd - hd)
            print(f'{dt.task} {metric} {mode}: base device {devc["base_score"]!r} host {hb!r}; largest decrease difference '
                  f'{diff.max():.3e} (tolerance there {tol.flat[diff.argmax()]:.3e}); largest |decrease| {np.abs(hd).max():.3e}')
            assert abs(devc['base_score'] - hb) <= FS.metric_bar(metric, n_out, hb)
            assert (diff <= tol).all(), (metric, mode, diff, tol)
            assert np.abs(hd).max() > 0
            out[metric, mode] = devc
    return out


def test_device_path_is_the_host_path_on_a_graph_with_a_plan(deepfm):
    dt, df, y = deepfm
    res = _compare_paths(dt, df, y, ['auc', 'log_loss', 'accuracy'])
    assert res['auc', 'max']['columns'] == df.columns.to_list()
    fi = F.get_score_importances(dt, df, y, 'auc', n_iter=2, mode='max', random_state=21, batch_size=256)
    means = res['auc', 'max']['score_decreases'].mean(0)
    assert fi[:, 0].tolist() == [df.columns[k] for k in np.argsort(-means, kind='stable')]


@pytest.mark.parametrize('task,metric', [('multiclass', 'accuracy'), ('regression', 'rmse')])
def test_device_path_is_the_host_path_on_other_tasks(dev, task, metric):
    df, y = FS.task_frame(task)
    dt = _fit(df, y, FS.task_config(task))
    if task == 'multiclass':
        assert dt.model.inference_plan() is None                    # the layer path under eval() / no_grad
    _compare_paths(dt, df, y, [metric])


def test_device_path_with_a_column_in_both_blocks_and_a_var_len_column(dev):
    """c_int feeds the continuous block and two non-adjacent columns of the id block; tags is a whole var-len block; const
    and excluded feed nothing"""
    df = FS.mixed_frame(400)
    rng = np.random.default_rng(3)
    y = ((df['c_int'] > 3) ^ (df['f_two'] > 1)).astype(int).values
    y[rng.random(len(y)) < 0.05] ^= 1
    dt = _fit(df, y, FS.mixed_config(metrics=['auc']), epochs=3)
    assert dt.model.inference_plan() is None
    feed = F.make_feed(dt, df, dt.preprocessor.transform_y(y))
    assert feed.kinds == ['cat', 'var', 'cont']
    tg = F.feed_targets(dt.model, feed, dt.preprocessor.source_columns(), ['c_int'])
    cats, conts = dt.preprocessor.get_categorical_columns(), dt.preprocessor.get_continuous_columns()
    assert tg == {0: sorted([cats.index('c_int_cat'), cats.index('c_int_discrete')]), 2: [conts.index('c_int')]}
    assert F.feed_targets(dt.model, feed, dt.preprocessor.source_columns(), ['tags']) == {1: list(range(feed.blocks[1].shape[1]))}
    res = _compare_paths(dt, df, y, ['auc'])['auc', 'max']
    k = {c: i for i, c in enumerate(res['columns'])}
    assert (res['score_decreases'][:, [k['const'], k['excluded']]] == 0.0).all()
    grouped = _compare_paths(dt, df, y, ['auc'], columns=[['c_int', 'tags'], 'f_nan'])['auc', 'max']
    assert grouped['columns'] == [('c_int', 'tags'), 'f_nan']


# ---- 3. the feed afterwards -------------------------------------------------------------------------------------------------
def _bits(feed):
    return [b.clone() for b in feed.blocks] + [feed.y.clone()]


def _same_bits(feed, before):
    return all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(feed.blocks + [feed.y], before))


def test_feed_is_bit_identical_afterwards_also_when_a_pass_raises(deepfm, monkeypatch):
    from deeptables_amd import metrics
    dt, df, y = deepfm
    feed = F.make_feed(dt, df, dt.preprocessor.transform_y(y))
    assert F.device_refusal(dt, feed) is None and all(b.is_cuda for b in feed.blocks)
    before = _bits(feed)
    entries = F._entries(df, None)
    F.feed_scores(dt, feed, entries, 'auc', 2, 1.0, F._generator(dt.model.device, 1), 256)
    assert _same_bits(feed, before)
    real, calls, seen = metrics.epoch_metrics, [0], []

    def third_pass_raises(metrics, y_true, y_prob, task):
        calls[0] += 1
        if calls[0] == 3:
            seen.append(not _same_bits(feed, before))                 # (the feed IS permuted while the pass runs)
            raise RuntimeError('metric failed')
        return real(metrics, y_true, y_prob, task)

    monkeypatch.setattr(metrics, 'epoch_metrics', third_pass_raises)
    with pytest.raises(RuntimeError, match='metric failed'):
        F.feed_scores(dt, feed, entries, 'auc', 2, 1.0, F._generator(dt.model.device, 1), 256)
    assert seen == [True] and _same_bits(feed, before)


# ---- 4. nothing large crosses -----------------------------------------------------------------------------------------------
def test_no_row_sized_tensor_crosses_to_the_host_in_a_pass(deepfm, monkeypatch):
    """Tensor.cpu / .numpy / .tolist on a tensor of n or more elements, counted while the passes run.  The metric's own result
    buffer (metrics._OUT_WORDS words, read once per pass) must stay below n for the count to mean what it says: the 600-row
    frame is scored six times over."""
    from deeptables_amd import metrics
    dt, df, y = deepfm
    df = pd.concat([df] * 6, ignore_index=True)
    y = np.concatenate([y] * 6)
    n = len(df)
    assert metrics._OUT_WORDS < n
    big = [0]

    def counting(name):
        real = getattr(torch.Tensor, name)

        def f(self, *a, **k):
            if self.numel() >= n:
                big[0] += 1
            return real(self, *a, **k)
        return f

    with monkeypatch.context() as mp:
        for name in ('cpu', 'numpy', 'tolist'):
            mp.setattr(torch.Tensor, name, counting(name))
        feed = F.make_feed(dt, df, dt.preprocessor.transform_y(y))
        big[0] = 0
        F.feed_scores(dt, feed, F._entries(df, None), 'auc', 2, 1.0, F._generator(dt.model.device, 1), min(n, 8192))
        assert big[0] == 0
        res = F.permutation_scores(dt, df, y, 'auc', n_iter=1, device=False, columns=['age', 'job'], random_state=1)
        assert res['path'] == 'host' and big[0] >= 3                  # the host loop: at least one per pass
