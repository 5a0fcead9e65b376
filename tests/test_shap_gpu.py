# -*- coding:utf-8 -*-
"""GPU: Shapley values on the device — dt_coalition_fill / dt_coalition_mean / dt_shap_solve (csrc/coalition.hip) against numpy at
the launch's edges, the device path of utils/shap.py against hand-made frames, exact Shapley values and its host path, the
model and both feeds bit for bit afterwards, and nothing row-sized read back."""
import numpy as np
import pytest
import torch

from deeptables_amd.utils import feature_importance as FI
from deeptables_amd.utils import shap as SH
from tests import feature_importance_support as FS
from tests import shap_support as SS

pytestmark = pytest.mark.gpu

SENTINEL = 0x5EA7BEE
FRAME = 64                      # words of sentinel on either side of every buffer
GRID_CAP_BLOCKS = 2048          # csrc/coalition.hip kCoalitionMaxBlocks: one row past it strides
U = 2.0 ** -53


# ---- 7. dt_coalition_fill -----------------------------------------------------------------------------------------------------
def _framed(dev, numel, skew=0):
    """-> (the whole sentinel-filled allocation, a [numel] int32 view FRAME words in; skew: words off 16-byte alignment)"""
    raw = torch.full((numel + 2 * FRAME + 4,), SENTINEL, dtype=torch.int32, device=dev)
    assert raw.data_ptr() % 16 == 0
    return raw, raw[FRAME + skew:FRAME + skew + numel]


def _words(kind, n, rng):
    """[n] int32 words: random ids, or float32 bit patterns with NaNs of distinct payloads, +-0.0, denormals and +-Inf"""
    if kind == 'int32':
        return rng.integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32)
    w = rng.normal(size=n).astype(np.float32).view(np.int32).copy()
    special = np.array([0x7FC00001, 0x7FC12345, 0x7F800001, -0x3FFFFF, 0x00000000, -0x80000000, 0x00000001, 0x007FFFFF,
                        -0x7FFFFFFF, 0x7F800000, -0x00800000], dtype=np.int64).astype(np.int32)
    pos = rng.permutation(n)[:max(1, n // 3)]
    w[pos] = special[np.arange(len(pos)) % len(special)]
    return w


def _groups(C, M, rng):
    """int32 [C]: every player of the last mask word owns a column where C allows, groups own several columns, some -1"""
    g = rng.integers(-1, M, C).astype(np.int32)
    g[0] = M - 1                                                    # the highest bit of the last word
    if C >= 5:
        g[1], g[2], g[4] = -1, g[3], g[3]                           # a column that never moves; one group, three columns
    return g


def _fill_case(dev, kind, C, Nb, M, S, s0, s1, rng, skew=0):
    from deeptables_amd import ops
    from deeptables_amd._lib import lib, ptr, stream_ptr
    masks = rng.random((S, M)) < 0.5
    masks[s0] = True                                                # a coalition of every player and one of none
    if s1 - s0 > 1:
        masks[s0 + 1] = False
    group = _groups(C, M, rng)
    x, bg = _words(kind, C, rng), _words(kind, Nb * C, rng).reshape(Nb, C)
    rows = (s1 - s0) * Nb
    bufs = {}
    for name, host in (('x', x), ('bg', bg.reshape(-1)), ('out', np.full(rows * C, 0x0BADF00D, dtype=np.int32))):
        raw, view = _framed(dev, host.size, skew)
        view.copy_(torch.from_numpy(host).to(dev))
        bufs[name] = (raw, view, raw.clone())
    packed = ops.pack_coalitions(masks).to(dev)
    group_d = torch.from_numpy(group).to(dev)
    h = lib()
    rc = h.dt_coalition_fill(ptr(bufs['x'][1]), ptr(bufs['bg'][1]), Nb, C, ptr(packed), S, M, s0, s1, ptr(group_d),
                             group.ctypes.data, ptr(bufs['out'][1]), stream_ptr())
    assert rc == 0, h.dt_last_error()
    take = np.where(group[None, :] >= 0, masks[s0:s1][:, np.clip(group, 0, None)], False)              # [Sc, C]
    want = np.where(take[:, None, :], x[None, None, :], bg[None, :, :]).reshape(rows, C)
    got = bufs['out'][1].cpu().numpy().reshape(rows, C)
    assert np.array_equal(got, want), (kind, C, Nb, M, S, s0, s1, skew)
    for name in ('x', 'bg'):                                        # the inputs are only read
        assert torch.equal(bufs[name][0], bufs[name][2])
    raw, _, raw0 = bufs['out']
    lo, hi = FRAME + skew, FRAME + skew + rows * C
    assert torch.equal(raw[:lo], raw0[:lo]) and torch.equal(raw[hi:], raw0[hi:])
    return take


@pytest.mark.parametrize('kind', ['int32', 'float32'])
def test_coalition_fill_against_numpy_where(dev, kind):
    rng = np.random.default_rng(11)
    seen = set()
    for C in (1, 5, 8):
        for Nb in (1, 3, 50):
            for M in (1, 32, 33):
                take = _fill_case(dev, kind, C, Nb, M, 9, 0, 9, rng)
                _fill_case(dev, kind, C, Nb, M, 9, 4, 7, rng)                        # a chunk that starts at s0 > 0
                _fill_case(dev, kind, C, Nb, M, 9, 8, 9, rng)
                seen.add(bool(take.any()) and not bool(take.all()))
    assert seen == {True}


@pytest.mark.parametrize('kind', ['int32', 'float32'])
def test_coalition_fill_16_byte_path_and_its_misaligned_twin(dev, kind):
    """C a multiple of 4 on 16-byte aligned buffers moves uint4 words with a select per word; the same call on buffers one
    word off takes the 4-byte kernel and gives the same bits"""
    for C in (4, 8, 12):
        for Nb in (1, 3, 50):
            for M in (1, 32, 33):
                for skew in (0, 1):
                    _fill_case(dev, kind, C, Nb, M, 9, 2, 9, np.random.default_rng(100 * C + Nb + M), skew=skew)


def test_coalition_fill_one_row_past_the_grid_cap(dev):
    """total words = 2048 blocks x 256 threads + one row: the last row is reached by the stride, not by the grid"""
    rng = np.random.default_rng(5)
    cap = GRID_CAP_BLOCKS * 256
    assert (cap + 8) % 8 == 0 and (cap + 8) // 8 == 65537
    _fill_case(dev, 'int32', 8, 1, 33, 65537, 0, 65537, rng, skew=1)                # 4-byte words: 65537 rows of 8
    assert (cap + 2) * 4 == 262145 * 8 and 262145 == 5 * 52429
    _fill_case(dev, 'float32', 8, 5, 33, 52429 + 3, 3, 52429 + 3, rng)              # uint4 words: 262145 rows of 2


def test_coalition_fill_rejects_a_group_outside_the_players(dev):
    from deeptables_amd import ops
    from deeptables_amd._lib import DtHipError, lib, ptr, stream_ptr
    bg = torch.zeros(3, 4, dtype=torch.int32, device=dev)
    x = torch.ones(4, dtype=torch.int32, device=dev)
    masks = ops.pack_coalitions(np.ones((2, 3), dtype=bool)).to(dev)
    out = torch.full((6, 4), 7, dtype=torch.int32, device=dev)
    for bad in ([0, 1, 3, 2], [0, -2, 1, 2]):
        g = np.array(bad, dtype=np.int32)
        gd = torch.from_numpy(g).to(dev)
        assert lib().dt_coalition_fill(ptr(x), ptr(bg), 3, 4, ptr(masks), 2, 3, 0, 2, ptr(gd), g.ctypes.data, ptr(out),
                                       stream_ptr()) == -1
        with pytest.raises(ValueError, match='group entries'):
            ops.coalition_fill(x, bg, masks, 3, 0, 2, gd)
    torch.cuda.synchronize()
    assert (out == 7).all()
    with pytest.raises(DtHipError):
        ops.coalition_fill(x, bg, masks.cpu(), 3, 0, 2, torch.zeros(4, dtype=torch.int32, device=dev))


# ---- 8. dt_coalition_mean -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('O', [1, 3])
@pytest.mark.parametrize('Nb', [1, 50, 63, 64, 65, 1000])
def test_coalition_mean_against_numpy_float64(dev, Nb, O):
    from deeptables_amd import ops
    rng = np.random.default_rng(Nb * 10 + O)
    nseg = 11                                                       # three blocks of four waves
    x = (rng.normal(size=(nseg, Nb, O)) * 10.0 ** rng.integers(-3, 4, (nseg, Nb, O))).astype(np.float32)
    x[3] = np.abs(x[3])                                             # a segment without cancellation
    xd = torch.from_numpy(x.reshape(nseg * Nb, O)).to(dev)
    got = ops.coalition_mean(xd, Nb)
    assert got.dtype == torch.float64 and tuple(got.shape) == (nseg, O)
    want = x.astype(np.float64).mean(axis=1)
    bar = Nb * U * np.abs(x.astype(np.float64)).mean(axis=1)
    diff = np.abs(got.cpu().numpy() - want)
    print(f'Nb={Nb} O={O}: largest |mean - numpy| / bar {np.max(diff / bar):.3f}')
    assert (diff <= bar).all(), (diff, bar)
    again = ops.coalition_mean(xd, Nb)
    assert torch.equal(got.view(torch.int64), again.view(torch.int64))                  # the same bits on two runs
    # all segments at once is the segments one by one
    for seg in (0, nseg - 1):
        one = ops.coalition_mean(xd[seg * Nb:(seg + 1) * Nb].contiguous(), Nb)
        assert torch.equal(one.view(torch.int64), got[seg:seg + 1].view(torch.int64))
    x[5, Nb // 2, O - 1] = np.nan
    x[7, Nb - 1, 0] = np.inf
    got = ops.coalition_mean(torch.from_numpy(x.reshape(nseg * Nb, O)).to(dev), Nb).cpu().numpy()
    nan = np.zeros((nseg, O), dtype=bool)
    nan[5, O - 1] = True
    assert np.array_equal(np.isnan(got), nan) and got[7, 0] == np.inf
    keep = ~nan
    keep[7, 0] = False
    assert np.array_equal(got[keep], again.cpu().numpy()[keep])


# ---- 9. dt_shap_solve ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('O', [1, 3])
@pytest.mark.parametrize('S', [2, 126, 2100])
@pytest.mark.parametrize('M', [2, 3, 33])
def test_shap_solve_against_numpy_float64(dev, M, S, O):
    from deeptables_amd import ops
    rng = np.random.default_rng(M * 10000 + S * 10 + O)
    R = 4
    masks = rng.random((S, M)) < 0.5
    P = rng.normal(size=(M - 1, S)) / S
    ey, fx, e0 = rng.normal(size=(R, S, O)), rng.normal(size=(R, O)), rng.normal(size=O)
    packed = ops.pack_coalitions(masks).to(dev)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    got_d = ops.shap_solve(to(P), packed, M, to(ey), to(fx), to(e0))
    assert got_d.dtype == torch.float64 and tuple(got_d.shape) == (R, O, M)
    assert torch.equal(got_d.view(torch.int64), ops.shap_solve(to(P), packed, M, to(ey), to(fx), to(e0)).view(torch.int64))
    got = got_d.cpu().numpy()
    z = masks[:, -1].astype(np.float64)
    for r in range(R):
        for o in range(O):
            y = ey[r, :, o] - e0[o] - z * (fx[r, o] - e0[o])
            want = P @ y
            bar = 2 * (S + 4) * U * (np.abs(P) * (np.abs(ey[r, :, o]) + 2 * abs(e0[o]) + abs(fx[r, o]))[None, :]).sum(axis=1)
            diff = np.abs(got[r, o, :M - 1] - want)
            assert (diff <= bar).all(), (r, o, diff, bar)
            assert abs(got[r, o].sum() - (fx[r, o] - e0[o])) <= SS.efficiency_bar(got[r, o])
    cpu = ops.shap_solve(torch.from_numpy(P), packed.cpu(), M, torch.from_numpy(ey), torch.from_numpy(fx),
                         torch.from_numpy(e0)).numpy()
    assert np.abs(cpu - got).max() <= 1e-12 * max(1.0, np.abs(got).max())


# ---- 10. - 14. the paths ------------------------------------------------------------------------------------------------------
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
    conf = ModelConfig(nets=deepnets.DeepFM, metrics=['auc'], earlystopping_patience=0, fixed_embedding_dim=True,
                       embeddings_output_dim=8, embedding_dropout=0)
    dt = _fit(df, y, conf)
    assert dt.model.inference_plan() is not None
    return dt, df


ROWS = [3, 77, 410]


def _explain(dt, df, nsamples='auto', device=True, rows=ROWS, **kw):
    ex = SH.DeepTablesExplainer(dt, df, num_samples=8, device=device)
    hook = SS.ChunkOutputs(ex.plan(nsamples)[0], len(ex.background))
    phi = ex.get_shap_values(df.iloc[rows], nsamples=nsamples, on_chunk=hook, **kw)
    return ex, phi, hook


def test_device_path_end_to_end_against_frames(deepfm):
    dt, df = deepfm
    ex, phi, hook = _explain(dt, df)
    assert ex.last_path == 'device' and phi.shape == (3, 7) and phi.dtype == np.float64
    cols, Nb = list(ex.players), len(ex.background)
    masks = ex.plan('auto')[0]
    assert len(masks) == 126 and len(hook.blocks) == 3
    # every synthetic block is transform_X of the hand-made hybrid frame, bit for bit: the group map
    for r, s0, s1, blocks in hook.blocks:
        hand = SS.hand_frames(ex.background, df.iloc[ROWS[r]:ROWS[r] + 1], cols)
        pick = np.concatenate([SS.mask_key(masks[s]) * Nb + np.arange(Nb) for s in range(s0, s1)])
        want = FI.make_feed(dt, hand.iloc[pick].reset_index(drop=True), None)
        assert [b.dtype for b in want.blocks] == [b.dtype for b in blocks]
        for a, b in zip(want.blocks, blocks):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # phi against exact Shapley values of the device path's OWN value function
    for r in range(3):
        v = np.zeros((2 ** 7, 1))
        v[0], v[-1] = ex.expected_value, ex.fx[r]
        for key in range(1, 2 ** 7 - 1):
            v[key] = hook.seen[r, key].mean(axis=0)
        want = SS.exact_shapley(v)[0]
        diff = np.abs(phi[r] - SS.features_from_players(want, ex.feature_names, cols)).max()
        print(f'row {r}: max|phi - exact| {diff:.3e}, bar {1e-12 * np.abs(v).max():.3e}, max|phi| {np.abs(want).max():.3e}')
        assert diff <= 1e-12 * np.abs(v).max()
        assert abs(phi[r].sum() - (ex.fx[r] - ex.expected_value)) <= SS.efficiency_bar(phi[r])
    assert np.abs(phi).max() > 1e-3
    # the chunking does not change a bit of the outputs' means, nor does 'auto' differ from device=True
    small = SH.SHAP_MAX_SYNTH_ROWS
    try:
        SH.SHAP_MAX_SYNTH_ROWS = 8 * 10
        ex2, phi2, hook2 = _explain(dt, df, device='auto', batch_size=50)
    finally:
        SH.SHAP_MAX_SYNTH_ROWS = small
    assert ex2.last_path == 'device' and len(hook2.blocks) == 3 * 13
    delta = hook2.delta({k: v for k, v in hook.seen.items()})
    assert np.abs(phi2 - phi).max() <= 2 * delta + 1e-12


def _device_against_host(dt, df, nsamples, what, rows=ROWS):
    exh, host, hh = _explain(dt, df, nsamples, device=False, rows=rows)
    exd, devc, dh = _explain(dt, df, nsamples, device=True, rows=rows)
    assert exh.last_path == 'host' and exd.last_path == 'device' and set(hh.seen) == set(dh.seen)
    delta = dh.delta(hh.seen)
    vmax = max(np.abs(o).max() for o in hh.seen.values())
    bar = 2 * delta + 1e-12 * vmax
    for o, (a, b) in enumerate(zip(devc if isinstance(devc, list) else [devc], host if isinstance(host, list) else [host])):
        diff = np.abs(a - b).max()
        print(f'{what} output {o}: max|device - host| {diff:.3e}, bar {bar:.3e}, delta {delta:.3e}, max|phi| {np.abs(b).max():.3e}')
        assert diff <= bar, f'{what} output {o}: {diff:.3e} > {bar:.3e} with delta {delta:.3e}'
        assert np.abs(b).max() > 0
    assert np.abs(np.atleast_1d(exd.expected_value) - np.atleast_1d(exh.expected_value)).max() <= delta + 1e-12 * vmax
    return exd, devc


def test_device_path_is_the_host_path_in_the_sampled_regime(deepfm):
    dt, df = deepfm
    ex, _ = _device_against_host(dt, df, 60, 'DeepFM nsamples=60')
    assert len(ex.plan(60)[0]) <= 60


def test_device_path_is_the_host_path_on_the_layer_path_with_var_len_and_shared_columns(dev):
    df = FS.mixed_frame(400)
    dt = _fit(df, SS.mixed_labels(df), FS.mixed_config(metrics=['auc']), epochs=3)
    assert dt.model.inference_plan() is None
    ex, phi = _device_against_host(dt, df, 'auto', 'mixed', rows=[0, 5, 123])
    assert list(ex.players) == ['c_str', 'c_int', 'f_nan', 'f_two', 'tags']
    k = {c: i for i, c in enumerate(ex.feature_names)}
    assert (phi[:, [k['const'], k['excluded']]] == 0.0).all()
    feed = FI.make_feed(dt, ex.background, None)
    groups = ex._groups(feed)
    assert feed.kinds == ['cat', 'var', 'cont'] and (groups[1] == ex.players['tags']).all()
    assert (groups[0] == ex.players['c_int']).sum() == 2 and (groups[2] == ex.players['c_int']).sum() == 1


def test_device_path_is_the_host_path_on_multiclass(dev):
    df, y = FS.task_frame('multiclass')
    dt = _fit(df, y, FS.task_config('multiclass'))
    ex, phi = _device_against_host(dt, df, 'auto', 'multiclass')
    assert isinstance(phi, list) and len(phi) == 3 and ex.expected_value.shape == (3,)


def _state(dt, feeds):
    tensors = [p.detach() for p in dt.model.model.parameters()] + [b for b in dt.model.model.buffers()]
    for f in feeds:
        tensors += list(f.blocks)
    return tensors, [t.clone() for t in tensors]


def _unchanged(state):
    return all(torch.equal(a.reshape(-1).contiguous().view(torch.uint8), b.reshape(-1).view(torch.uint8)) for a, b in zip(*state))


def test_model_and_feeds_are_bit_identical_afterwards_also_when_a_chunk_raises(deepfm):
    dt, df = deepfm
    ex = SH.DeepTablesExplainer(dt, df, num_samples=8)
    bg_feed, x_feed = FI.make_feed(dt, ex.background, None), FI.make_feed(dt, df.iloc[ROWS], None)
    state = _state(dt, [bg_feed, x_feed])
    assert len(state[0]) > 6
    SH.feed_values(dt, bg_feed, x_feed, ex._groups(bg_feed), ex.plan('auto'))
    assert _unchanged(state)
    ex.get_shap_values(df.iloc[ROWS])
    assert ex.last_path == 'device' and _unchanged(state)
    calls = []

    def second_chunk_raises(r, s0, s1, blocks, outputs):
        calls.append(r)
        if len(calls) == 2:
            raise RuntimeError('chunk failed')

    with pytest.raises(RuntimeError, match='chunk failed'):
        SH.feed_values(dt, bg_feed, x_feed, ex._groups(bg_feed), ex.plan('auto'), None, second_chunk_raises)
    assert calls == [0, 1] and _unchanged(state)


def test_only_phi_fx_and_the_expected_value_cross_to_the_host(deepfm, monkeypatch):
    """Tensor.cpu / .numpy / .tolist / .item on device tensors, recorded while the device path runs over ready feeds: the three
    results, and otherwise nothing as large as the background (8 rows), let alone a coalition's or a chunk's rows"""
    dt, df = deepfm
    ex = SH.DeepTablesExplainer(dt, df, num_samples=8)
    bg_feed, x_feed = FI.make_feed(dt, ex.background, None), FI.make_feed(dt, df.iloc[ROWS], None)
    plan, groups = ex.plan('auto'), ex._groups(bg_feed)
    SH.feed_values(dt, bg_feed, x_feed, groups, plan)                               # warm: whatever the first call reads once
    moved = []

    def counting(name):
        real = getattr(torch.Tensor, name)

        def f(self, *a, **k):
            if self.is_cuda:
                moved.append((tuple(self.shape), self.dtype))
            return real(self, *a, **k)
        return f

    with monkeypatch.context() as mp:
        for name in ('cpu', 'numpy', 'tolist', 'item'):
            mp.setattr(torch.Tensor, name, counting(name))
        SH.feed_values(dt, bg_feed, x_feed, groups, plan)
    results = [((3, 1, 7), torch.float64), ((3, 1), torch.float64), ((1,), torch.float64)]
    for res in results:
        assert res in moved, (res, moved)
        moved.remove(res)
    assert all(int(np.prod(shape)) < 8 for shape, _ in moved), moved


def test_device_selection(deepfm, monkeypatch):
    dt, df = deepfm
    with monkeypatch.context() as mp:
        mp.setenv('DT_AMD_DEVICE_SHAP', '0')
        ex = SH.DeepTablesExplainer(dt, df, num_samples=4)
        ex.get_shap_values(df.iloc[:2], nsamples=40)
        assert ex.last_path == 'host'
        ex = SH.DeepTablesExplainer(dt, df, num_samples=4, device=True)            # the switch is for 'auto'
        ex.get_shap_values(df.iloc[:2], nsamples=40)
        assert ex.last_path == 'device'
    ex = SH.DeepTablesExplainer(dt, df, num_samples=4)
    ex.get_shap_values(df.iloc[:2], nsamples=40)
    assert ex.last_path == 'device'
    with monkeypatch.context() as mp:
        FS.cpu_kernels(mp)
        dfc, yc = FS.task_frame('binary', n=200)
        cpu = FS.fit_cpu(dfc, yc, FS.task_config('binary'), epochs=1)
        with pytest.raises(ValueError, match='device=True: the model is on cpu, not on a GPU'):
            SH.DeepTablesExplainer(cpu, dfc, num_samples=4, device=True).get_shap_values(dfc.iloc[:2], nsamples=40)
