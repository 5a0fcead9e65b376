# -*- coding:utf-8 -*-
"""GPU: the transform kernel (csrc/prep_transform.hip, `ops.prep_transform`) against the numpy branch of the same function with
exact equality at every launch path — one row to one row past a full grid pass, one column to more than a column chunk, both
output kinds, every operation on every source dtype, table lengths 1 to 65,537, 0 / 1 / 9 edges, the 16-byte and the
single-word store path — then `transform_feed` against `TableBatches(pp.transform_X(X))` on the frames with the hard values,
and the model-level callers.  No tolerance anywhere."""
import numpy as np
import pytest
import torch

from tests import device_transform_support as S

pytestmark = pytest.mark.gpu

SMALL_N = [1, 63, 64, 65, 257]
COLUMNS = [1, 3, 4, 33, 36]               # 33 and 36 exceed the kernel's column chunk; 4 and 36 take the 16-byte stores
TABLES = [1, 2, 1000, 65537]
EDGES = [0, 1, 9]


def _past_a_grid_pass():
    from deeptables_amd import ops
    assert (ops.PREP_TILE_ROWS, ops.PREP_CHUNK_COLS, ops.PREP_MAX_BLOCKS) == (256, 32, 1024)
    assert max(COLUMNS) > ops.PREP_CHUNK_COLS
    return ops.PREP_MAX_BLOCKS * ops.PREP_TILE_ROWS + 1


def _cells():
    cells, i = [], 0
    for kind in ('cat', 'cont'):
        for N in SMALL_N:
            for C in COLUMNS:
                cells.append((kind, N, C, i))
                i += 1
        for C in (3, 4):
            cells.append((kind, None, C, i))          # None: one row past a full grid pass
            i += 1
    return cells


def _run(cols, N, C, kind, offset, dev):
    """the kernel's block, with a sentinel word on either side of the output; offset 1: the output starts one word past a
    16-byte boundary"""
    from deeptables_amd import ops
    dtype = torch.int32 if kind == 'cat' else torch.float32
    buf = torch.full((N * C + 8,), 0x5EA7BEE, dtype=torch.int32, device=dev)
    start = 4 + offset
    out = buf[start:start + N * C].view(dtype).view(N, C)
    assert out.data_ptr() % 16 == (4 * offset) % 16
    got = ops.prep_transform(N, cols, kind, out=out)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    assert (buf[:start] == 0x5EA7BEE).all() and (buf[start + N * C:] == 0x5EA7BEE).all()
    return got.view(torch.int32).cpu()


@pytest.mark.parametrize('kind,N,C,i', _cells())
def test_kernel_is_the_cpu_branch(dev, kind, N, C, i):
    from deeptables_amd import ops
    N = _past_a_grid_pass() if N is None else N
    rng = np.random.default_rng(1000 + i)
    dtypes = S.DTYPES[i % 11:] + S.DTYPES[:i % 11]                     # C = 1 cells walk through the dtypes
    specs = S.random_columns(rng, N, C, kind, dtypes, table_len=TABLES[i % 4], n_edges=EDGES[i % 3])
    want = ops.prep_transform(N, S.columns_on(specs, 'cpu'), kind).view(torch.int32)
    cols = S.columns_on(specs, dev)
    for offset in (0, 1):
        got = _run(cols, N, C, kind, offset, dev)
        same = got == want
        assert bool(same.all()), (offset, [(r, c, specs[c]['dtype'], specs[c]['op']) for r, c in (~same).nonzero()[:5].tolist()])
    assert torch.equal(_run(cols, N, C, kind, 0, dev), got)            # the same bits on every run


def test_cells_cover_every_operation_dtype_table_and_edge_count():
    from deeptables_amd import ops
    seen, tables, edges, per_dtype = set(), set(), set(), {}
    for kind, N, C, i in _cells():
        dtypes = S.DTYPES[i % 11:] + S.DTYPES[:i % 11]
        for j in range(C):
            name = dtypes[j % 11]
            op = ops.PREP_CONT if kind == 'cont' else [ops.PREP_LOOKUP, ops.PREP_BIN, ops.PREP_COPY][j % 3]
            if op == ops.PREP_COPY and name.startswith('float'):
                op = ops.PREP_LOOKUP
            seen.add((op, name))
            per_dtype.setdefault(name, set()).add((N, C))
            if op == ops.PREP_LOOKUP and np.dtype(name).itemsize >= 4:
                tables.add(TABLES[i % 4])
            if op == ops.PREP_BIN:
                edges.add(EDGES[i % 3])
    ints = [d for d in S.DTYPES if not d.startswith('float')]
    assert seen == {(op, d) for op in (ops.PREP_LOOKUP, ops.PREP_CONT, ops.PREP_BIN) for d in S.DTYPES} | \
        {(ops.PREP_COPY, d) for d in ints}
    assert tables == set(TABLES) and edges == set(EDGES) and all(len(v) >= 2 for v in per_dtype.values())


# ---- transform_feed ------------------------------------------------------------------------------------------------------------
def _fit(frame, y, **conf):
    from deeptables_amd.models import ModelConfig
    from deeptables_amd.models.preprocessor import DefaultPreprocessor
    pp = DefaultPreprocessor(ModelConfig(**conf))
    pp.fit_transform(frame, y)
    return pp


@pytest.mark.parametrize('config', sorted(S.numeric_configs()))
def test_numeric_frame_end_to_end(dev, config, monkeypatch):
    monkeypatch.delenv('DT_AMD_DEVICE_TRANSFORM', raising=False)
    fit, y, X = S.numeric_frames()
    pp = _fit(fit, y, **S.numeric_configs()[config])
    if config == 'explicit':
        X = S.put_values_on_the_edges(pp, X)
    w = np.linspace(0.25, 4.0, len(X))
    feed = pp.transform_feed(X, y, device=dev, mode=True, sample_weight=w)
    assert feed.transform_path == 'device' and feed.host_columns == [] and feed.resident and feed.weighted
    assert all(b.device == dev for b in feed.blocks) and feed.y.device == dev
    S.assert_same_feed(feed, S.host_feed(pp, X, y, device=dev, sample_weight=w, resident=True))
    again = pp.transform_feed(X, y, device=dev, sample_weight=w)                     # 'auto' takes the device path too
    assert again.transform_path == 'device'
    S.assert_same_feed(again, feed)


def test_bank_frame_end_to_end_with_host_served_columns(dev, monkeypatch):
    from deeptables_amd.datasets import dsutils
    monkeypatch.delenv('DT_AMD_DEVICE_TRANSFORM', raising=False)
    df = dsutils.load_bank(n=600)
    y = df.pop('y')
    pp = _fit(df.iloc[:400], y.iloc[:400], auto_categorize=True, auto_discrete=True, auto_scale=True)
    X, yt = df.iloc[250:], y.iloc[250:]
    feed = pp.transform_feed(X, yt, device=dev, mode=True)
    assert feed.transform_path == 'device'
    assert feed.host_columns == [c for c in df.columns if df[c].dtype == object]
    S.assert_same_feed(feed, S.host_feed(pp, X, yt, device=dev, resident=True))
    monkeypatch.setenv('DT_AMD_DEVICE_TRANSFORM', '0')
    host = pp.transform_feed(X, yt, device=dev)
    assert host.transform_path == 'host'
    S.assert_same_feed(host, feed)
    with pytest.raises(ValueError, match='DT_AMD_DEVICE_TRANSFORM'):
        pp.transform_feed(X, yt, device=dev, mode=True)


def test_multiclass_targets_are_one_hot_as_tablebatches_forms_them(dev, monkeypatch):
    monkeypatch.delenv('DT_AMD_DEVICE_TRANSFORM', raising=False)
    fit, _, X = S.numeric_frames()
    y = np.array(['a', 'b', 'c'])[np.arange(len(fit)) % 3]
    pp = _fit(fit, y, **S.numeric_configs()['automatic'])
    feed = pp.transform_feed(X, y, device=dev, mode=True)
    assert feed.y.shape == (len(X), 3) and feed.y_ndim == 2
    S.assert_same_feed(feed, S.host_feed(pp, X, y, device=dev, resident=True))


def test_no_row_sized_tensor_crosses_back(dev, monkeypatch):
    """Tensor.cpu / .numpy / .tolist on a tensor of N or more elements, counted between the uploads and the returned feed"""
    monkeypatch.delenv('DT_AMD_DEVICE_TRANSFORM', raising=False)
    fit, y, X = S.numeric_frames()
    pp = _fit(fit, y, **S.numeric_configs()['automatic'])
    pp.transform_feed(X, y, device=dev, mode=True)                                   # the plan and its tables are in place
    n, big = len(X), [0]

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
        feed = pp.transform_feed(X, y, device=dev, mode=True)
        assert big[0] == 0 and feed.transform_path == 'device'
        S.host_feed(pp, X, y, device=dev, resident=True).blocks[0].cpu()
        assert big[0] == 1                                                           # (the counter does count)


# ---- the model-level callers ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def deepfm(dev):
    from deeptables_amd import functional
    from deeptables_amd.datasets import dsutils
    from deeptables_amd.models import DeepTable, ModelConfig, deepnets
    df = dsutils.load_bank(n=600)
    y = df.pop('y')
    functional.set_seed(11)
    dt = DeepTable(config=ModelConfig(nets=deepnets.DeepFM, metrics=['AUC', 'accuracy'], earlystopping_patience=0,
                                      fixed_embedding_dim=True, embeddings_output_dim=8, embedding_dropout=0))
    dt.fit(df, y, batch_size=64, epochs=1, verbose=0)
    return dt, df, y


def test_predict_evaluate_and_make_feed_take_the_device_path(deepfm, monkeypatch):
    dt, df, y = deepfm
    pp, dm = dt.preprocessor, dt.model
    monkeypatch.delenv('DT_AMD_DEVICE_TRANSFORM', raising=False)
    feed = dt.make_feed(df, y)
    assert feed.transform_path == 'device' and feed.resident and feed.y is not None
    S.assert_same_feed(feed, S.host_feed(pp, df, y, device=dm.device, resident=True))
    calls = [0]
    real = pp.transform_X

    def counted(*a, **k):
        calls[0] += 1
        return real(*a, **k)

    monkeypatch.setattr(pp, 'transform_X', counted, raising=False)
    proba = dt.predict_proba(df, batch_size=128)
    labels = dt.predict(df, batch_size=128)
    ev = dt.evaluate(df, y, batch_size=128)
    assert calls[0] == 0                                                             # the default path never goes through pandas
    by_feed = dm.predict(feed, batch_size=128)
    assert np.array_equal(by_feed.view(np.int32), np.asarray(dm.predict(real(df), batch_size=128)).view(np.int32))
    assert dict(dm.evaluate(feed, batch_size=128)) == dict(ev)
    monkeypatch.setenv('DT_AMD_DEVICE_TRANSFORM', '0')
    assert np.array_equal(dt.predict_proba(df, batch_size=128).view(np.int32), proba.view(np.int32))
    assert calls[0] == 1
    assert np.array_equal(dt.predict(df, batch_size=128), labels)
    assert dict(dt.evaluate(df, y, batch_size=128)) == dict(ev)
    assert dict(dm.evaluate(real(df), pp.transform_y(y), batch_size=128)) == dict(ev)   # the parent's call
    assert dt.make_feed(df, y).transform_path == 'host'
