# -*- coding:utf-8 -*-
"""CPU: the column profile entry points (csrc/prep_fit.hip) — header, library and binding agree, arguments are refused before
any launch — and the premise of the exact fit test: on the dyadic frames pandas' mean is the exact mean."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from tests import device_transform_support as S
from tests import prep_fit_support as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('dt_column_profile_workspace_bytes', 'dt_column_profile', 'dt_column_order_stats')


def test_entries_are_declared_exported_and_bound():
    from deeptables_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'dt_hip.h')).read(), flags=re.S)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        params = re.search(r'\b%s\s*\(([^;{]*?)\)\s*;' % name, text).group(1).split(',')
        kinds = ['ptr' if '*' in d else {'int': 'int', 'int64_t': 'i64'}[d.split()[0]] for d in params]
        bound = [{ctypes.c_void_p: 'ptr', ctypes.c_int: 'int', ctypes.c_int64: 'i64'}[a] for a in _lib.SIGNATURES[name][1]]
        assert hasattr(handle, name) and bound == kinds, name
    for const in ('DT_PROFILE_TILE', 'DT_PROFILE_STAT_WORDS', 'DT_PROFILE_MAX_RANKS', 'DT_PROFILE_MAX_COLS'):
        assert int(re.search(r'^#define %s (\d+)\s*$' % const, text, re.M).group(1)) == getattr(_lib, const)


@pytest.mark.parametrize('what, args', [
    ('N = -1', dict(N=-1)), ('N = 2147483648', dict(N=1 << 31)), ('C = 0', dict(C=0)), ('cap = -1', dict(cap=-1)),
    ('null pointer', dict(stats=None)), ('unknown dtype code 11', dict(dtype=11)), ('null source', dict(src=None)),
    ('misaligned source', dict(src=0x1004)), ('null workspace', dict(ws=None)), ('at most 1024', dict(C=1025))])
def test_arguments_are_refused_before_any_launch(what, args):
    from deeptables_amd import _lib
    h = _lib.lib()
    a = dict(N=16, C=1, cap=2, stats=0x1000, dtype=_lib.DT_PREP_I64, src=0x1000, ws=0x1000)
    a.update(args)
    C = max(a['C'], 1)
    srcs, codes = (ctypes.c_void_p * C)(*[a['src']] * C), (ctypes.c_int32 * C)(*[a['dtype']] * C)
    rc = h.dt_column_profile(0x1000, 0x1000, ctypes.cast(srcs, ctypes.c_void_p), ctypes.cast(codes, ctypes.c_void_p), a['N'], a['C'],
                             a['cap'], a['stats'], 0x1000, 0x1000, a['ws'], None)
    assert rc == (-2 if a["C"] > 1024 else -1) and what in h.dt_last_error().decode()
    if set(args) <= {'N', 'C', 'cap'}:
        assert h.dt_column_profile_workspace_bytes(a['N'], a['C'], a['cap']) < 0
    if set(args) <= {'N', 'C', 'dtype'}:
        assert h.dt_column_order_stats(0x1000, 0x1000, ctypes.cast(codes, ctypes.c_void_p), a['N'], a['C'], 0x1000, 0x1000, 0x1000,
                                       0x1000, None) < 0


def test_workspace_holds_both_key_buffers_and_an_empty_frame_is_a_no_op():
    from deeptables_amd import _lib
    h = _lib.lib()
    assert h.dt_column_profile_workspace_bytes(1 << 20, 39, 1024) >= 2 * 8 * 39 * (1 << 20)
    srcs, codes = (ctypes.c_void_p * 1)(None), (ctypes.c_int32 * 1)(_lib.DT_PREP_F32)
    assert h.dt_column_profile(0x1000, 0x1000, ctypes.cast(srcs, ctypes.c_void_p), ctypes.cast(codes, ctypes.c_void_p), 0, 1, 0,
                               0x1000, None, None, None, None) == 0


def test_key_maps_are_inverse_and_ordered():
    from deeptables_amd import ops
    for name in S.DTYPES:
        a = np.concatenate([S._pool(np.random.default_rng(1), name, 64)] * 2)
        k = ops.profile_keys(a)
        back = ops.profile_values(k, name)
        nan = np.isnan(a) if a.dtype.kind == 'f' else np.zeros(len(a), bool)
        assert back.dtype == a.dtype and np.array_equal(back[~nan].view('u1'), a[~nan].view('u1')) and np.isnan(back[nan]).all()
        order = np.argsort(k, kind='stable')
        assert np.array_equal(a[order][:(~nan).sum()], np.sort(a[~nan])) and nan[order][(~nan).sum():].all()


@pytest.mark.parametrize('config', sorted(S.numeric_configs()))
def test_pandas_mean_is_the_exact_mean_on_the_dyadic_frames(config):
    from deeptables_amd.models.preprocessor import DefaultPreprocessor
    X, y, extra = P.dyadic_frame(with_host_columns=True)
    pp = DefaultPreprocessor(P.config_of(S.numeric_configs()[config], extra))
    pp.fit_transform(X, y)
    means = pp.X_transformers['imputation'].means_
    assert means
    for c, mean in means.items():
        x = X[c].values.astype(np.float64)
        x = x[~np.isnan(x)]
        exact = math.fsum(x) / len(x)               # (pandas returns a float32 mean for a float32 column)
        assert mean == (float(np.float32(exact)) if X[c].dtype == np.float32 else exact), c


def test_fit_feed_on_a_cpu_target(monkeypatch):
    from deeptables_amd.models.preprocessor import DefaultPreprocessor
    X, y, extra = P.dyadic_frame(with_host_columns=False)
    conf = P.config_of(S.numeric_configs()['automatic'], extra)
    with pytest.raises(ValueError, match='not a GPU'):
        DefaultPreprocessor(conf).fit_feed(X, y, device='cpu', mode=True)
    with pytest.raises(ValueError, match='mode must be'):
        DefaultPreprocessor(conf).fit_feed(X, y, device='cpu', mode='yes')
    host, pp = DefaultPreprocessor(conf), DefaultPreprocessor(conf)
    host.fit_transform(X, y)
    feed = pp.fit_feed(X, y, device='cpu')
    assert feed.fit_path == 'host' and 'not a GPU' in feed.fit_refusal and P.fitted_state(pp) == P.fitted_state(host)
