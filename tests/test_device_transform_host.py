# -*- coding:utf-8 -*-
"""CPU: the device path of the preprocessor's transform without a GPU — what `fit_transform` records, the plan
(`DefaultPreprocessor.device_plan`), its partition into device-served and host-served columns, the numpy branch of
`ops.prep_transform` against `TableBatches(pp.transform_X(X))` bit for bit, the routing of `transform_feed`, pickling, and the
C entry `dt_prep_transform` (surface and argument checks, no launch).  No tolerance anywhere: every quantity is integer or
IEEE float64 arithmetic."""
import ctypes
import os
import pickle
import re

import numpy as np
import pandas as pd
import pytest
import torch

from tests import device_transform_support as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fit(frame, y, **conf):
    from deeptables_amd.models import ModelConfig
    from deeptables_amd.models.preprocessor import DefaultPreprocessor
    pp = DefaultPreprocessor(ModelConfig(**conf))
    pp.fit_transform(frame, y)
    return pp


@pytest.fixture(scope='module')
def bank():
    from deeptables_amd.datasets import dsutils
    df = dsutils.load_bank(n=600)
    y = df.pop('y')
    return df, y


def _with_nans(df):
    df = df.copy()
    df['balance'] = df['balance'].astype('float64')
    df.loc[df.index[::7], 'balance'] = np.nan
    df['duration'] = df['duration'].astype('float32')
    df.loc[df.index[3::11], 'duration'] = np.nan
    return df


BANK_CONFIGS = {
    'auto_categorize': (dict(auto_categorize=True), False),
    'categorize_in_place': (dict(auto_categorize=True, cat_remain_numeric=False), False),
    'explicit_scaled_binned': (dict(categorical_columns=['job', 'marital', 'age', 'day', 'campaign'], auto_scale=True,
                                    auto_discrete=True), False),
    'no_imputation_with_nans': (dict(auto_imputation=False, auto_scale=True, auto_discrete=False), True),
    'no_label_encoding': (dict(categorical_columns=['age', 'day'], auto_encode_label=False, auto_scale=True), False),
}


@pytest.mark.parametrize('name', sorted(BANK_CONFIGS))
def test_bank_frame_through_the_cpu_branch(bank, name):
    df, y = bank
    conf, nans = BANK_CONFIGS[name]
    if nans:
        df = _with_nans(df)
    if name == 'no_label_encoding':
        df = df[['age', 'day', 'balance', 'duration', 'campaign']]
    pp = _fit(df.iloc[:400], y.iloc[:400], **conf)
    X = df.iloc[300:]                                  # rows seen and unseen at fit
    got, host = S.plan_feed(pp, X)
    S.assert_same_feed(got, S.host_feed(pp, X))
    numeric = [c for c in X.columns if X[c].dtype.kind in 'biuf']
    assert host == [c for c in pp.device_plan().sources if c not in numeric]         # only the string columns are host-served
    assert [c for c in pp.device_plan().device_columns] == [c for c in pp.device_plan().sources if c in numeric]


def test_var_len_column_is_host_served_and_the_feed_is_equal():
    rng = np.random.default_rng(1)
    n = 200
    tags = ['|'.join(rng.choice(list('abcdef'), rng.integers(0, 4))) for _ in range(n)]
    df = pd.DataFrame({'a': rng.integers(0, 5, n), 'f': rng.standard_normal(n).astype(np.float32), 'tags': tags})
    y = rng.integers(0, 2, n)
    pp = _fit(df, y, var_len_categorical_columns=[('tags', '|', 'max')], categorical_columns=['a'], auto_discrete=True)
    X = df.iloc[::-1].reset_index(drop=True)
    got, host = S.plan_feed(pp, X)
    assert host == ['tags'] and got.kinds == ['cat', 'var', 'cont']
    S.assert_same_feed(got, S.host_feed(pp, X))


# ---- the synthetic all-numeric frame -------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def numeric():
    return S.numeric_frames()


@pytest.mark.parametrize('config', sorted(S.numeric_configs()))
def test_every_served_dtype_and_hard_value(numeric, config):
    fit, y, X = numeric
    pp = _fit(fit, y, **S.numeric_configs()[config])
    if config == 'explicit':
        X = S.put_values_on_the_edges(pp, X)
    plan = pp.device_plan()
    got, host = S.plan_feed(pp, X)
    assert host == [] and plan.host_columns == [] and plan.refused == {}, plan.refused       # no silent fallback
    ops_used = {o.op for o in plan.outputs()}
    assert ops_used == {'lookup', 'bin', 'cont'}
    served = {plan.fit_dtypes[o.source].name for o in plan.outputs() if o.op == 'lookup'}
    assert served == set(S.DTYPES)
    assert {plan.fit_dtypes[o.source].name for o in plan.outputs() if o.op == 'cont'} >= set(S.DTYPES) - {'bool'}
    lookups = {o.name: o for o in plan.outputs() if o.op == 'lookup'}
    one = lookups['k_one' if config == 'explicit' else 'k_one_cat']
    assert len(one.keys) == 1                                                               # a one-key table
    edges = pp.X_transformers['discreter'].edges_
    assert len(edges['v_const']) == 0                                                       # a discretiser without edges
    if config == 'automatic':
        assert pp.X_transformers['standard_scale'].range_['v_const'] == 1.0                 # a constant column
    want = S.host_feed(pp, X)
    S.assert_same_feed(got, want)
    # the hard values did reach the blocks: unseen ids, NaN and inf among the continuous values
    cat, cont = want.blocks[0], want.blocks[-1]
    names = pp.get_categorical_columns()
    k = names.index('k_int8' if config == 'explicit' else 'k_int8_cat')
    assert int(cat[:, k].max()) == lookups[names[k]].miss
    assert bool(torch.isinf(cont).any())
    # the fit frame itself goes through as well (every key seen)
    S.assert_same_feed(S.plan_feed(pp, fit)[0], S.host_feed(pp, fit))


def test_raw_keys_are_distinct_by_bit_pattern(numeric):
    from deeptables_amd.models.preprocessor import distinct_raw_values
    fit, y, X = numeric
    pp = _fit(fit, y, **S.numeric_configs()['explicit'])
    assert sorted(pp.raw_keys_) == sorted(['k_' + d for d in S.DTYPES] + ['k_one'])          # continuous-only: nothing recorded
    assert all(pp.raw_keys_[c].dtype == fit[c].dtype == pp.fit_dtypes_[c] for c in pp.raw_keys_)
    k32 = pp.raw_keys_['k_float32']
    assert np.isnan(k32).sum() == 1 and (k32 == 0).sum() == 2 and len(k32) == 6              # one NaN, -0.0 AND 0.0
    v = distinct_raw_values(np.array([np.nan, -np.nan, 0.0, -0.0, 0.0]))
    assert len(v) == 3


@pytest.mark.parametrize('config', sorted(S.numeric_configs()))
def test_lookup_tables_hold_the_host_s_answer_for_every_fit_value(numeric, config):
    from deeptables_amd import ops
    fit, y, _ = numeric
    pp = _fit(fit, y, **S.numeric_configs()[config])
    plan = pp.device_plan()
    names = pp.get_categorical_columns()
    checked = 0
    for o in plan.cat:
        if o.op != 'lookup':
            continue
        raw = pp.raw_keys_[o.source]
        frame = fit.iloc[np.zeros(len(raw), dtype=int)].reset_index(drop=True).copy()
        frame[o.source] = raw
        want = pp.transform_X(frame)[o.name].values
        keys = ops.prep_keys(raw)
        pos = np.searchsorted(o.keys, keys)
        assert (o.keys[pos] == keys).all() and (o.ids[pos] == want).all(), o.name
        assert (np.diff(o.keys.astype(object)) > 0).all() or len(o.keys) == 1
        assert o.miss == len(pp.X_transformers['label_encoder'].maps_[o.name])
        checked += 1
    assert checked >= len(S.DTYPES) + 1 and len(names) > checked          # (automatic: v_bool and v_const are looked up too)


# ---- the partition -----------------------------------------------------------------------------------------------------------
def test_partition_strings_categories_and_a_dtype_that_changed():
    rng = np.random.default_rng(2)
    n = 240
    fit = pd.DataFrame({'s': rng.choice(['x', 'y', 'z'], n), 'c': pd.Categorical(rng.choice(['p', 'q'], n)),
                        'i': rng.integers(0, 6, n), 'j': rng.integers(0, 9, n), 'f': rng.standard_normal(n)})
    y = rng.integers(0, 2, n)
    pp = _fit(fit, y, categorical_columns=['s', 'c', 'i'], auto_discrete=True)
    X = fit.copy()
    X['i'] = X['i'].astype('float64')                  # an int column arriving as float64 because of a NaN: '3.0', not '3'
    X.loc[5, 'i'] = np.nan
    got, host = S.plan_feed(pp, X)
    assert host == ['s', 'c', 'i'] and pp.device_plan().device_columns == ['j', 'f']
    want = S.host_feed(pp, X)
    S.assert_same_feed(got, want)
    k = pp.get_categorical_columns().index('i')
    assert (want.blocks[0][:, k] == len(pp.X_transformers['label_encoder'].maps_['i'])).all()      # the host says "unseen"
    got, host = S.plan_feed(pp, fit)                   # the same plan, the fit dtypes again
    assert host == ['s', 'c']
    S.assert_same_feed(got, S.host_feed(pp, fit))


# ---- routing -----------------------------------------------------------------------------------------------------------------
def test_transform_feed_routing_on_a_cpu_target(bank, monkeypatch):
    df, y = bank
    monkeypatch.delenv('DT_AMD_DEVICE_TRANSFORM', raising=False)
    pp = _fit(df, y, auto_categorize=True)
    X, yt = df.iloc[:90], y.iloc[:90]
    w = np.linspace(0.5, 2.0, 90)
    with pytest.raises(ValueError, match='cpu'):
        pp.transform_feed(X, yt, device='cpu', mode=True)
    with pytest.raises(ValueError, match='mode'):
        pp.transform_feed(X, yt, device='cpu', mode='maybe')
    feed = pp.transform_feed(X, yt, device='cpu', sample_weight=w)
    assert feed.transform_path == 'host' and 'cpu' in feed.transform_refusal
    S.assert_same_feed(feed, S.host_feed(pp, X, yt, sample_weight=w))
    assert pp.feed_refusal('cuda:0') is None                               # what a GPU target is asked (no GPU is touched)
    assert 'int32' in pp.feed_refusal('cuda:0', cat_dtype=torch.int64)
    assert 'max_resident_bytes' in pp.feed_refusal('cuda:0', n_rows=1 << 20, max_resident_bytes=1 << 20)
    monkeypatch.setenv('DT_AMD_DEVICE_TRANSFORM', '0')
    feed = pp.transform_feed(X, yt, device='cpu')
    assert feed.transform_path == 'host' and feed.transform_refusal == 'DT_AMD_DEVICE_TRANSFORM=0'
    monkeypatch.delenv('DT_AMD_DEVICE_TRANSFORM')
    assert pp.transform_feed(X, device='cpu', mode=False).transform_refusal == 'mode=False'
    del pp.raw_keys_                                                       # a preprocessor from an older dt.pkl
    assert 'raw_keys_' in pp.feed_refusal('cuda:0')
    feed = pp.transform_feed(X, yt, device='cpu')
    assert feed.transform_path == 'host'
    S.assert_same_feed(feed, S.host_feed(pp, X, yt))
    from deeptables_amd.models import ModelConfig
    from deeptables_amd.models.preprocessor import DefaultPreprocessor
    assert 'not fitted' in DefaultPreprocessor(ModelConfig()).feed_refusal('cuda:0')


def test_pickle_after_a_plan_was_built(numeric):
    fit, y, X = numeric
    pp = _fit(fit, y, **S.numeric_configs()['automatic'])
    before, _ = S.plan_feed(pp, X)
    assert pp._device_plan is not None and pp._device_plan._resident
    again = pickle.loads(pickle.dumps(pp))
    assert again._device_plan is None and pp._device_plan is not None
    assert not any(isinstance(v, torch.Tensor) for v in again.__dict__.values())
    after, host = S.plan_feed(again, X)
    assert host == []
    S.assert_same_feed(after, before)
    S.assert_same_feed(after, S.host_feed(again, X))


# ---- ops.prep_transform on CPU tensors -----------------------------------------------------------------------------------------
def test_cpu_branch_definitions_on_hand_made_columns():
    from deeptables_amd import ops
    src = np.array([np.nan, -0.0, 0.0, 2.0, np.inf, -np.inf, 1e-45], dtype=np.float32)
    keys = ops.prep_keys(np.array([0.0, -0.0, np.nan], dtype=np.float32))
    order = np.argsort(keys)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    look = ops.PrepColumn(ops.prep_source(src, 'cpu'), 'float32', ops.PREP_LOOKUP, keys=t(keys[order].view(np.int64)),
                          ids=t(np.array([10, 11, 12], dtype=np.int32)[order]), miss=99)
    binc = ops.PrepColumn(ops.prep_source(src, 'cpu'), 'float32', ops.PREP_BIN, edges=t(np.array([0.0, 2.0])), fill=2.0,
                          flags=ops.PREP_IMPUTE)
    nobin = ops.PrepColumn(ops.prep_source(src, 'cpu'), 'float32', ops.PREP_BIN, edges=t(np.zeros(0)))
    out = ops.prep_transform(7, [look, binc, nobin], 'cat')
    assert out[:, 0].tolist() == [12, 11, 10, 99, 99, 99, 99]
    assert out[:, 1].tolist() == [2, 1, 1, 2, 2, 0, 1]                        # NaN filled with 2.0; -0.0 == 0.0 is on the edge
    assert out[:, 2].tolist() == [0, 0, 0, 0, 0, 0, 0]
    big = np.array([2 ** 53 + 1, np.iinfo(np.int64).min, np.iinfo(np.int64).max, -1], dtype=np.int64)
    cont = ops.PrepColumn(ops.prep_source(big, 'cpu'), 'int64', ops.PREP_CONT, min=1.0, range=3.0, flags=ops.PREP_SCALE)
    want = ((big.astype(np.float64) - 1.0) / 3.0).astype(np.float32)
    assert np.array_equal(ops.prep_transform(4, [cont], 'cont').numpy().view(np.int32)[:, 0], want.view(np.int32))
    copy = ops.PrepColumn(ops.prep_source(big, 'cpu'), 'int64', ops.PREP_COPY)
    assert ops.prep_transform(4, [copy], 'cat')[:, 0].tolist() == torch.from_numpy(big).to(torch.int32).tolist()
    u = np.array([2 ** 64 - 1, 2 ** 63 + 7], dtype=np.uint64)
    assert ops.prep_transform(2, [ops.PrepColumn(ops.prep_source(u, 'cpu'), 'uint64', ops.PREP_COPY)], 'cat')[:, 0].tolist() == [-1, 7]
    for bad in ([cont], [ops.PrepColumn(ops.prep_source(src, 'cpu'), 'float32', ops.PREP_COPY)]):
        with pytest.raises(ValueError):
            ops.prep_transform(len(bad[0].src) // np.dtype(bad[0].dtype).itemsize, bad, 'cat')
    with pytest.raises(ValueError, match='bytes'):
        ops.prep_transform(5, [cont], 'cont')
    assert ops.prep_transform(0, [ops.PrepColumn(torch.zeros(0, dtype=torch.uint8), 'int8', ops.PREP_COPY)], 'cat').shape == (0, 1)


# ---- the C entry -------------------------------------------------------------------------------------------------------------
def test_entry_is_declared_exported_and_bound():
    from deeptables_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'dt_hip.h')).read(), flags=re.S)
    protos = dict(re.findall(r'\b(dt_prep_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;', text))
    assert sorted(protos) == ['dt_prep_transform'] == sorted(n for n in _lib.SIGNATURES if n.startswith('dt_prep_'))
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(handle, 'dt_prep_transform')
    res, args = _lib.SIGNATURES['dt_prep_transform']
    decls = [p.strip() for p in protos['dt_prep_transform'].split(',')]
    assert len(decls) == len(args) and res is ctypes.c_int
    assert ['*' in d for d in decls] == [a is ctypes.c_void_p for a in args]
    assert args[0] is ctypes.c_int64 and decls[0].startswith('int64_t')
    # the descriptor: the header's struct, the binding's mirror and the size the library was compiled with
    from deeptables_amd import ops
    struct = re.search(r'typedef struct dt_prep_col \{(.*?)\} dt_prep_col;', text, re.S).group(1)
    fields = [n.strip() for decl in struct.split(';') if decl.strip() for n in decl.replace('*', ' ').split(None, 1)[1].replace(
        'void', '').replace('uint64_t', '').replace('int32_t', '').replace('double', '').replace('const', '').split(',')]
    assert fields == [f[0] for f in ops.PrepCol._fields_]
    assert ctypes.sizeof(ops.PrepCol) == _lib.DT_PREP_COL_BYTES == 80
    defs = {m.group(1): int(m.group(2), 0) for m in re.finditer(r'^#define (DT_PREP_[A-Z0-9_]+) (0x[0-9a-fA-F]+|\d+)\s*$', text, re.M)}
    assert len(defs) == 24 and all(getattr(_lib, n) == v for n, v in defs.items())
    assert {ops.PREP_DTYPES[d] for d in S.DTYPES} == set(range(_lib.DT_PREP_DTYPE_COUNT))


def test_entry_rejects_bad_arguments_without_a_launch():
    from deeptables_amd import _lib, ops
    h = _lib.lib()
    buf = (ctypes.c_uint64 * 64)()                       # stands in for every device pointer: nothing is launched
    p = ctypes.addressof(buf)

    def call(N=8, C=1, kind=_lib.DT_PREP_OUT_I32, out=p, cols_dev=p, host=True, **field):
        col = dict(src=p, keys=p, ids=p, edges=p, fill=0.0, min=0.0, range=1.0, dtype=_lib.DT_PREP_I32, op=_lib.DT_PREP_LOOKUP,
                   n_keys=4, n_edges=0, miss=4, flags=0)
        col.update(field)
        table = (ops.PrepCol * max(C, 1))(*[ops.PrepCol(**col) for _ in range(max(C, 1))])
        rc = h.dt_prep_transform(N, cols_dev, ctypes.cast(table, ctypes.c_void_p) if host else None, C, kind, out, None)
        return rc, h.dt_last_error().decode()

    bad = [dict(N=-1), dict(C=0), dict(kind=2), dict(out=None), dict(cols_dev=None), dict(host=False), dict(out=p + 2),
           dict(cols_dev=p + 4), dict(dtype=11), dict(dtype=-1), dict(op=4), dict(op=-1), dict(n_keys=-1), dict(n_edges=-1),
           dict(op=_lib.DT_PREP_BIN, n_edges=-3), dict(flags=4), dict(src=None), dict(src=p + 2), dict(keys=None), dict(ids=None),
           dict(keys=p + 4), dict(ids=p + 2), dict(op=_lib.DT_PREP_BIN, n_edges=2, edges=None),
           dict(op=_lib.DT_PREP_BIN, n_edges=2, edges=p + 4), dict(op=_lib.DT_PREP_CONT),
           dict(kind=_lib.DT_PREP_OUT_F32), dict(op=_lib.DT_PREP_COPY, dtype=_lib.DT_PREP_F32),
           dict(op=_lib.DT_PREP_COPY, dtype=_lib.DT_PREP_F64), dict(dtype=_lib.DT_PREP_I64, src=p + 4)]
    for kw in bad:
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith('dt_prep_transform'), (kw, rc, msg)
    # N == 0: DT_OK without a launch, also without sources; empty tables need no pointers
    assert call(N=0)[0] == 0 and call(N=0, src=None)[0] == 0
    assert call(N=0, n_keys=0, keys=None, ids=None)[0] == 0
    assert call(N=0, C=3, op=_lib.DT_PREP_BIN, n_edges=0, edges=None)[0] == 0
    assert call(N=0, kind=_lib.DT_PREP_OUT_F32, op=_lib.DT_PREP_CONT, dtype=_lib.DT_PREP_F64)[0] == 0
