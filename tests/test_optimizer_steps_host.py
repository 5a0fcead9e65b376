# -*- coding:utf-8 -*-
"""Host: what `KerasAdam.step()`, `Adagrad.step()` and `RMSprop.step()` hand the library, launch by launch.  No GPU and no
built library: `training.lib` is a recorder, the tensors live on the CPU, and every pointer argument is decoded into the
name of the tensor it points to (the pattern of tests/test_host_logic.py::_decoded).  EXPECTED holds, per optimizer and
scenario, the whole call list: entry point, argument count, scalars, pointer identities and the `advance` flag.

So that the copies a step makes become visible, the recorder stands in for a dense launch: it adds 1 to the n floats at the
parameter pointer and 2 to those at every slot pointer (the tail a row launch carries is left alone)."""
import ctypes

import numpy as np
import pytest
import torch

from deeptables_amd import training as T
from deeptables_amd.ops import SparseRowGrad

KINDS = ('adam', 'adagrad', 'rmsprop')
SLOTS = {'adam': 2, 'adagrad': 1, 'rmsprop': 1, 'rmsprop_record': 1}        # slots per element
ROWS_ARG = {'dt_adam_rows_step_seg': 3, 'dt_adagrad_rows_step': 2, 'dt_rmsprop_rows_step': 3}     # index of `rows`
N_SLOTS = 1024


def _floats(addr, n):
    return np.ctypeslib.as_array((ctypes.c_float * n).from_address(addr))


class _Recorder:
    """stand-in for training.lib(): every call is recorded as (name, args) and returns 0; dt_adam_rows_slots answers
    N_SLOTS.  The pointer arrays of a multi-tensor launch die with the call: they are read out here."""

    def __init__(self):
        self.calls, self.rows_seen = [], []

    def _update(self, p, slots, n):
        _floats(p, n)[:] += 1
        for s in slots:
            _floats(s, n)[:] += 2

    def __getattr__(self, name):
        def call(*args):
            kind = name.split('_')[1]
            if name.endswith('_dense_step'):
                k = SLOTS[kind]
                self._update(args[0].value, [a.value for a in args[2:2 + k]], args[2 + k])
            elif name.endswith('_multi_step'):
                k, n_t = SLOTS[kind], args[0]
                cols = [list((ctypes.c_void_p * n_t).from_address(a.value)) for a in args[1:3 + k]]
                ns = list((ctypes.c_int64 * n_t).from_address(args[3 + k].value))
                for i in range(n_t):
                    self._update(cols[0][i], [c[i] for c in cols[2:]], ns[i])
                args = (n_t, *[[ctypes.c_void_p(v) for v in c] for c in cols], ns) + args[4 + k:]
            elif name in ROWS_ARG:
                i = ROWS_ARG[name]
                n, d = args[i + 2], args[i + 3]
                self.rows_seen.append((list((ctypes.c_int64 * n).from_address(args[i].value)),
                                       _floats(args[i + 1].value, n * d).tolist()))
            self.calls.append((name, args))
            return N_SLOTS if name == 'dt_adam_rows_slots' else 0
        return call


@pytest.fixture
def rec(monkeypatch):
    r = _Recorder()
    monkeypatch.setattr(T, 'lib', lambda: r)
    monkeypatch.setattr(T, 'stream_ptr', lambda: None)
    return r


def _names(opt, named):
    """data_ptr -> 'name' ('a|b' when several named tensors start at the same address): the scenario's tensors, the
    optimizer's slots of the named parameters, its step state and its flat slots"""
    named = dict(named)
    for name, t in list(named.items()):
        for k, v in opt.state.get(id(t), {}).items():
            if torch.is_tensor(v):
                named[f'{name}.{k}'] = v
    if opt._dev_state is not None:
        named['state'] = opt._dev_state
    if opt._flat is not None:
        named.update({f'flat.slot{i}': s for i, s in enumerate(opt._flat[2:4]) if s is not None})
    by_ptr = {}
    for n, t in named.items():
        by_ptr.setdefault(t.data_ptr(), []).append(n)
    return {p: '|'.join(sorted(ns)) for p, ns in by_ptr.items()}


def _decoded(rec, names):
    """the recorded calls with every pointer replaced by its tensor's name; a pointer to a tensor the step made for itself
    (a concatenation, a contiguous copy) reads 'tmp<k>', numbered as they appear"""
    tmp = {}

    def dec(a):
        if isinstance(a, list):
            return [dec(x) for x in a]
        if isinstance(a, ctypes.c_void_p):
            return names[a.value] if a.value in names else tmp.setdefault(a.value, f'tmp{len(tmp)}')
        return a
    out = [(name, [dec(a) for a in args]) for name, args in rec.calls]
    rec.calls.clear()
    return out


def _opt(kind, params, embs=()):
    if kind == 'adam':
        return T.KerasAdam(params, embs)
    if kind == 'adagrad':
        return T.Adagrad(params, embs)
    opt = T.RMSprop(params, embs)
    opt.stamp_in_record = kind == 'rmsprop_record'
    return opt


def _param(*shape):
    n = int(np.prod(shape))
    return torch.nn.Parameter(torch.arange(n, dtype=torch.float32).reshape(shape) / 8)


class _Emb:
    """MultiColumnEmbedding as the optimizer sees it: one packed [10, 8] table of two fields"""

    def __init__(self):
        self.table = _param(10, 8)
        self.tables = {'d8': self.table}
        self.groups = [(8, [0, 1])]
        self.sparse_grads = {}


def _piece(rows, **kw):
    rows = torch.tensor(rows, dtype=torch.int64)
    return SparseRowGrad(rows, torch.arange(rows.numel() * 8, dtype=torch.float32).reshape(-1, 8) / 4, **kw)


def _dense_scenario(rec, kind, n_grads):
    """(a): two dense parameters, no table.  (f): no gradient at all."""
    w1, w2 = _param(3, 4), _param(5)
    opt = _opt(kind, [w1, w2])
    named = {'w1': w1, 'w2': w2}
    for name, p in list(named.items())[:n_grads]:
        p.grad = torch.ones_like(p)
        named[name + '.grad'] = p.grad
    opt.step()
    return _decoded(rec, _names(opt, named))


def _table_scenario(rec, kind, pieces, hook=False, steps=1):
    """one dense parameter and one table with the given gradient pieces ((b) - (e), (j) - (l))"""
    w1, emb = _param(3, 4), _Emb()
    opt = _opt(kind, [w1, emb.table], [emb])
    w1.grad = torch.ones_like(w1)
    named = {'w1': w1, 'w1.grad': w1.grad, 'table': emb.table}
    for i, g in enumerate(pieces):
        named.update({f'rows{i}': g.rows, f'values{i}': g.values})
        if g.segments is not None:
            named.update({f'seg{k}': t for k, t in enumerate(g.segments[:5])})
    out = None
    for step in range(steps):
        emb.sparse_grads = {'d8': list(pieces)}
        if hook:
            opt.pre_dense_hook = lambda: rec.calls.append(('hook', ()))
        before = {k: v for k, v in opt.state.get(id(emb.table), {}).items() if k in ('slots', 'mark')}
        opt.step()
        assert opt.pre_dense_hook is None and emb.sparse_grads == {}
        if step == 0:
            names = _names(opt, named)            # a later step is decoded with the FIRST step's buffers
        else:
            assert before and all(opt.state[id(emb.table)][k] is v for k, v in before.items())
        out = _decoded(rec, names)
    return out


FLAT_N = 192


def _flat_group(kind):
    """a flat group of three members: a [4, 6] (24), e [5, 8] (40) inside a zero-padded [5, 16] slab, c [7]"""
    flat_p = torch.zeros(FLAT_N)
    flat_g = torch.full((FLAT_N,), 9.0)
    layout = ((5, 8), (16, 1))
    a, e, c = _param(4, 6), _param(5, 8), _param(7)
    members = [(a, 0, 24), (e, 64, 40, layout), (c, 144, 7)]
    for mb in members:
        p, off = mb[0], mb[1]
        view = torch.as_strided(flat_p, layout[0], layout[1], off) if len(mb) > 3 else flat_p[off:off + mb[2]].view(p.shape)
        view.copy_(p.data)
        p.data = view
    opt = _opt(kind, [a, e, c])
    opt.register_flat_group(flat_p, flat_g, members, FLAT_N, grad_views=True)
    return opt, flat_p, flat_g, {'a': a, 'e': e, 'c': c, 'flat_p': flat_p, 'flat_g': flat_g}


def _pads(flat):
    mask = torch.ones(FLAT_N, dtype=torch.bool)
    mask[:24] = False
    mask[144:151] = False
    torch.as_strided(mask, (5, 8), (16, 1), 64).fill_(False)
    return flat[mask]


def _flat_scenario(rec, kind, how):
    opt, flat_p, flat_g, named = _flat_group(kind)
    a, e, c = named['a'], named['e'], named['c']
    if how == 'g':                                        # every gradient is the member's view of the flat buffer
        opt.zero_grad()
        assert all(p.grad is p._dt_grad_view for p in (a, e, c)) and float(flat_g.abs().max()) == 0.0
    elif how == 'h':                                      # separate tensors: scattered, then the one flat launch
        for name in 'aec':
            named[name].grad = named[name + '.grad'] = torch.full_like(named[name].data, float(ord(name)))
    else:                                                 # (i): only the strided member carries a gradient
        e.grad = named['e.grad'] = torch.ones(5, 8)
    p0, slot0 = flat_p.clone(), opt._flat[2].clone()
    opt.step()
    out = _decoded(rec, _names(opt, named))
    if how == 'h':
        assert float(_pads(flat_g).abs().max()) == 0.0
        assert torch.equal(flat_g[:24], torch.full((24,), 97.0)) and torch.equal(flat_g[144:151], torch.full((7,), 99.0))
        assert torch.equal(torch.as_strided(flat_g, (5, 8), (16, 1), 64), torch.full((5, 8), 101.0))
    if how == 'i':                                        # the copies' update is written back, and only there
        moved = torch.zeros(FLAT_N)
        torch.as_strided(moved, (5, 8), (16, 1), 64).fill_(1.0)
        assert torch.equal(flat_p, p0 + moved)
        for s in opt._flat[2:4]:
            assert s is None or torch.equal(s, slot0 + 2 * moved)
    return out


def _run(rec, kind, scen):
    if scen == 'a':
        return _dense_scenario(rec, kind, 2)
    if scen == 'b':
        return _table_scenario(rec, kind, [_piece([1, 3, 3, 7, -1, 2])])
    if scen == 'c':
        return _table_scenario(rec, kind, [_piece([1, 3, 3, 7, -1, 2])], hook=True)
    if scen == 'd':
        out = _table_scenario(rec, kind, [_piece([1, 3], fields=-1), _piece([3, 7, 2], fields=-1)])
        assert rec.rows_seen == [([1, 3, 3, 7, 2], (np.r_[0:16, 0:24] / 4).tolist())]
        return out
    if scen == 'e':
        return _table_scenario(rec, kind, [_piece([1, 3, 7], fields=-1)])
    if scen == 'f':
        return _dense_scenario(rec, kind, 0)
    if scen in 'ghi':
        return _flat_scenario(rec, kind, scen)
    if scen == 'j':
        return _table_scenario(rec, kind, [_piece([1, 3, 3, 7, -1, 2])], steps=2)
    if scen == 'k':
        seg = (torch.zeros(2, dtype=torch.int32), torch.zeros(8, dtype=torch.int64), torch.zeros(8, dtype=torch.int32),
               torch.zeros(8, dtype=torch.int32), torch.zeros(6, dtype=torch.int32), 2, 4)
        return _table_scenario(rec, kind, [_piece([1, -1, -1, 7, -1, 2], fields=-1, segments=seg)])
    if scen == 'l':
        return _table_scenario(rec, kind, [_piece([1, 3, 7], fields=-2)])
    raise KeyError(scen)


# recorded on the commit before the three optimizers were given one step driver; 't' is test_setting_t's list
EXPECTED = {
    'adam': {
        'a': [
            ('dt_adam_state_init', ['state', 0.001, 0.9, 0.999, 0, None]),
            ('dt_adam_multi_step', [2, ['w1', 'w2'], ['w1.grad', 'w2.grad'], ['w1.m', 'w2.m'], ['w1.v', 'w2.v'], [12, 5],
                                    0.0, 0.9, 0.999, 1e-07, 'state', 1, 0.001, None]),
        ],
        'b': [
            ('dt_adam_state_init', ['state', 0.001, 0.9, 0.999, 0, None]),
            ('dt_adam_rows_slots', [6]),
            ('dt_adam_rows_step_seg', ['table', 'table.m|table.mv', 'table.v', 'rows0', 'values0', 6, 8, 2, 'table.slots', 1024,
                                       'table.mark', 0.0, 0.9, 0.999, 1e-07, 'state', 'w1', 'w1.grad', 'w1.m', 'w1.v', 12, 1,
                                       0.001, None, None, None, None, None, 0, 0, 16, None]),
        ],
        'c': [
            ('dt_adam_state_init', ['state', 0.001, 0.9, 0.999, 0, None]),
            ('dt_adam_rows_slots', [6]),
            ('dt_adam_rows_step_seg', ['table', 'table.m|table.mv', 'table.v', 'rows0', 'values0', 6, 8, 2, 'table.slots', 1024,
                                       'table.mark', 0.0, 0.9, 0.999, 1e-07, 'state', None, None, None, None, 0, 0,
                                       0.001, None, None, None, None, None, 0, 0, 16, None]),
            ('hook', []),
            ('dt_adam_dense_step', ['w1', 'w1.grad', 'w1.m', 'w1.v', 12, 0.0, 0.9, 0.999, 1e-07, 'state', 1, 0.001, None]),
        ],
        'd': [
            ('dt_adam_state_init', ['state', 0.001, 0.9, 0.999, 0, None]),
            ('dt_adam_rows_slots', [5]),
            ('dt_adam_rows_step_seg', ['table', 'table.m|table.mv', 'table.v', 'tmp0', 'tmp1', 5, 8, 0, 'table.slots', 1024,
                                       'table.mark', 0.0, 0.9, 0.999, 1e-07, 'state', 'w1', 'w1.grad', 'w1.m', 'w1.v', 12, 1,
                                       0.001, None, None, None, None, None, 0, 0, 16, None]),
        ],
        'e': [
            ('dt_adam_state_init', ['state', 0.001, 0.9, 0.999, 0, None]),
            ('dt_adam_rows_step_seg', ['table', 'table.m|table.mv', 'table.v', 'rows0', 'values0', 3, 8, -1, None, 0,
                                       None, 0.0, 0.9, 0.999, 1e-07, 'state', 'w1', 'w1.grad', 'w1.m', 'w1.v', 12, 1,
                                       0.001, None, None, None, None, None, 0, 0, 16, None]),
        ],
        'f': [
            ('dt_adam_state_init', ['state', 0.001, 0.9, 0.999, 0, None]),
            ('dt_adam_advance', ['state', 0.001, 0.9, 0.999, None]),
        ],
        'g': [
            ('dt_adam_state_init', ['state', 0.001, 0.9, 0.999, 0, None]),
            ('dt_adam_dense_step', ['a|flat_p', 'flat_g', 'a.m|flat.slot0', 'a.v|flat.slot1', 192, 0.0, 0.9, 0.999, 1e-07,
                                    'state', 1, 0.001, None]),
        ],
        'h': [
            ('dt_adam_state_init', ['state', 0.001, 0.9, 0.999, 0, None]),
            ('dt_adam_dense_step', ['a|flat_p', 'flat_g', 'a.m|flat.slot0', 'a.v|flat.slot1', 192, 0.0, 0.9, 0.999, 1e-07,
                                    'state', 1, 0.001, None]),
        ],
        'i': [
            ('dt_adam_state_init', ['state', 0.001, 0.9, 0.999, 0, None]),
            ('dt_adam_dense_step', ['tmp0', 'e.grad', 'tmp1', 'tmp2', 40, 0.0, 0.9, 0.999, 1e-07, 'state', 1, 0.001, None]),
        ],
        'j': [
            ('dt_adam_rows_slots', [6]),
            ('dt_adam_rows_step_seg', ['table', 'table.m|table.mv', 'table.v', 'rows0', 'values0', 6, 8, 2, 'table.slots', 1024,
                                       'table.mark', 0.0, 0.9, 0.999, 1e-07, 'state', 'w1', 'w1.grad', 'w1.m', 'w1.v', 12, 1,
                                       0.001, None, None, None, None, None, 0, 0, 16, None]),
        ],
        'k': [
            ('dt_adam_state_init', ['state', 0.001, 0.9, 0.999, 0, None]),
            ('dt_adam_rows_step_seg', ['table', 'table.m|table.mv', 'table.v', 'rows0', 'values0', 6, 8, -1, None, 0,
                                       None, 0.0, 0.9, 0.999, 1e-07, 'state', 'w1', 'w1.grad', 'w1.m', 'w1.v', 12, 1,
                                       0.001, 'seg0', 'seg1', 'seg2', 'seg3', 'seg4', 2, 4, 16, None]),
        ],
        'l': [
            ('dt_adam_state_init', ['state', 0.001, 0.9, 0.999, 0, None]),
            ('dt_adam_rows_step_seg', ['table', 'table.m|table.mv', 'table.v', 'rows0', 'values0', 3, 8, -2, None, 0,
                                       None, 0.0, 0.9, 0.999, 1e-07, 'state', 'w1', 'w1.grad', 'w1.m', 'w1.v', 12, 1,
                                       0.001, None, None, None, None, None, 0, 0, 16, None]),
        ],
        't': [
            ('dt_adam_state_init', ['state', 0.001, 0.9, 0.999, 5, None]),
        ],
    },
    'adagrad': {
        'a': [
            ('dt_adam_state_init', ['state', 0.001, 0.0, 0.0, 0, None]),
            ('dt_adagrad_multi_step', [2, ['w1', 'w2'], ['w1.grad', 'w2.grad'], ['w1.acc', 'w2.acc'], [12, 5],
                                       0.001, 1e-07, 'state', 1, None]),
        ],
        'b': [
            ('dt_adam_state_init', ['state', 0.001, 0.0, 0.0, 0, None]),
            ('dt_adam_rows_slots', [6]),
            ('dt_adagrad_rows_step', ['table', 'table.acc', 'rows0', 'values0', 6, 8, 2, 'table.slots', 1024, 'table.mark',
                                      0.001, 1e-07, 'state', 'w1', 'w1.grad', 'w1.acc', 12, 1, 8, None]),
        ],
        'c': [
            ('dt_adam_state_init', ['state', 0.001, 0.0, 0.0, 0, None]),
            ('dt_adam_rows_slots', [6]),
            ('dt_adagrad_rows_step', ['table', 'table.acc', 'rows0', 'values0', 6, 8, 2, 'table.slots', 1024, 'table.mark',
                                      0.001, 1e-07, 'state', None, None, None, 0, 0, 8, None]),
            ('hook', []),
            ('dt_adagrad_dense_step', ['w1', 'w1.grad', 'w1.acc', 12, 0.001, 1e-07, 'state', 1, None]),
        ],
        'd': [
            ('dt_adam_state_init', ['state', 0.001, 0.0, 0.0, 0, None]),
            ('dt_adam_rows_slots', [5]),
            ('dt_adagrad_rows_step', ['table', 'table.acc', 'tmp0', 'tmp1', 5, 8, 0, 'table.slots', 1024, 'table.mark',
                                      0.001, 1e-07, 'state', 'w1', 'w1.grad', 'w1.acc', 12, 1, 8, None]),
        ],
        'e': [
            ('dt_adam_state_init', ['state', 0.001, 0.0, 0.0, 0, None]),
            ('dt_adagrad_rows_step', ['table', 'table.acc', 'rows0', 'values0', 3, 8, -1, None, 0, None,
                                      0.001, 1e-07, 'state', 'w1', 'w1.grad', 'w1.acc', 12, 1, 8, None]),
        ],
        'f': [
            ('dt_adam_state_init', ['state', 0.001, 0.0, 0.0, 0, None]),
            ('dt_adam_advance', ['state', 0.001, 0.0, 0.0, None]),
        ],
        'g': [
            ('dt_adam_state_init', ['state', 0.001, 0.0, 0.0, 0, None]),
            ('dt_adagrad_dense_step', ['a|flat_p', 'flat_g', 'a.acc|flat.slot0', 192, 0.001, 1e-07, 'state', 1, None]),
        ],
        'h': [
            ('dt_adam_state_init', ['state', 0.001, 0.0, 0.0, 0, None]),
            ('dt_adagrad_dense_step', ['a|flat_p', 'flat_g', 'a.acc|flat.slot0', 192, 0.001, 1e-07, 'state', 1, None]),
        ],
        'i': [
            ('dt_adam_state_init', ['state', 0.001, 0.0, 0.0, 0, None]),
            ('dt_adagrad_dense_step', ['tmp0', 'e.grad', 'tmp1', 40, 0.001, 1e-07, 'state', 1, None]),
        ],
        'j': [
            ('dt_adam_rows_slots', [6]),
            ('dt_adagrad_rows_step', ['table', 'table.acc', 'rows0', 'values0', 6, 8, 2, 'table.slots', 1024, 'table.mark',
                                      0.001, 1e-07, 'state', 'w1', 'w1.grad', 'w1.acc', 12, 1, 8, None]),
        ],
        't': [
            ('dt_adam_state_init', ['state', 0.001, 0.0, 0.0, 5, None]),
        ],
    },
    'rmsprop': {
        'a': [
            ('dt_adam_state_init', ['state', 0.001, 0.0, 0.0, 0, None]),
            ('dt_rmsprop_multi_step', [2, ['w1', 'w2'], ['w1.grad', 'w2.grad'], ['w1.rms', 'w2.rms'], [12, 5],
                                       0.001, 0.9, 1e-07, 'state', 1, None]),
        ],
        'b': [
            ('dt_adam_state_init', ['state', 0.001, 0.0, 0.0, 0, None]),
            ('dt_adam_rows_slots', [6]),
            ('dt_rmsprop_rows_step', ['table', 'table.rms', 'table.stamp', 'rows0', 'values0', 6, 8, 2, 'table.slots', 1024,
                                      'table.mark', 0.001, 0.9, 1e-07, 'state', 'w1', 'w1.grad', 'w1.rms', 12, 1, 8, 1, None]),
        ],
        'c': [
            ('dt_adam_state_init', ['state', 0.001, 0.0, 0.0, 0, None]),
            ('dt_adam_rows_slots', [6]),
            ('dt_rmsprop_rows_step', ['table', 'table.rms', 'table.stamp', 'rows0', 'values0', 6, 8, 2, 'table.slots', 1024,
                                      'table.mark', 0.001, 0.9, 1e-07, 'state', None, None, None, 0, 0, 8, 1, None]),
            ('hook', []),
            ('dt_rmsprop_dense_step', ['w1', 'w1.grad', 'w1.rms', 12, 0.001, 0.9, 1e-07, 'state', 1, None]),
        ],
        'd': [
            ('dt_adam_state_init', ['state', 0.001, 0.0, 0.0, 0, None]),
            ('dt_adam_rows_slots', [5]),
            ('dt_rmsprop_rows_step', ['table', 'table.rms', 'table.stamp', 'tmp0', 'tmp1', 5, 8, 0, 'table.slots', 1024,
                                      'table.mark', 0.001, 0.9, 1e-07, 'state', 'w1', 'w1.grad', 'w1.rms', 12, 1, 8, 1, None]),
        ],
        'e': [
            ('dt_adam_state_init', ['state', 0.001, 0.0, 0.0, 0, None]),
            ('dt_rmsprop_rows_step', ['table', 'table.rms', 'table.stamp', 'rows0', 'values0', 3, 8, -1, None, 0,
                                      None, 0.001, 0.9, 1e-07, 'state', 'w1', 'w1.grad', 'w1.rms', 12, 1, 8, 1, None]),
        ],
        'f': [
            ('dt_adam_state_init', ['state', 0.001, 0.0, 0.0, 0, None]),
            ('dt_adam_advance', ['state', 0.001, 0.0, 0.0, None]),
        ],
        'g': [
            ('dt_adam_state_init', ['state', 0.001, 0.0, 0.0, 0, None]),
            ('dt_rmsprop_dense_step', ['a|flat_p', 'flat_g', 'a.rms|flat.slot0', 192, 0.001, 0.9, 1e-07, 'state', 1, None]),
        ],
        'h': [
            ('dt_adam_state_init', ['state', 0.001, 0.0, 0.0, 0, None]),
            ('dt_rmsprop_dense_step', ['a|flat_p', 'flat_g', 'a.rms|flat.slot0', 192, 0.001, 0.9, 1e-07, 'state', 1, None]),
        ],
        'i': [
            ('dt_adam_state_init', ['state', 0.001, 0.0, 0.0, 0, None]),
            ('dt_rmsprop_dense_step', ['tmp0', 'e.grad', 'tmp1', 40, 0.001, 0.9, 1e-07, 'state', 1, None]),
        ],
        'j': [
            ('dt_adam_rows_slots', [6]),
            ('dt_rmsprop_rows_step', ['table', 'table.rms', 'table.stamp', 'rows0', 'values0', 6, 8, 2, 'table.slots', 1024,
                                      'table.mark', 0.001, 0.9, 1e-07, 'state', 'w1', 'w1.grad', 'w1.rms', 12, 1, 8, 1, None]),
        ],
        't': [
            ('dt_rmsprop_rows_materialize', ['table.rms', 'table.stamp', 10, 8, 8, 1, 0.9, 'state', None]),
            ('dt_adam_state_init', ['state', 0.001, 0.0, 0.0, 5, None]),
        ],
    },
    'rmsprop_record': {
        'b': [
            ('dt_adam_state_init', ['state', 0.001, 0.0, 0.0, 0, None]),
            ('dt_adam_rows_slots', [6]),
            ('dt_rmsprop_rows_step', ['table', 'table.rec|table.rms', 'table.stamp', 'rows0', 'values0', 6, 8, 2, 'table.slots',
                                      1024, 'table.mark', 0.001, 0.9, 1e-07, 'state', 'w1', 'w1.grad', 'w1.rms', 12, 1, 12, 12,
                                      None]),
        ],
    },
}


@pytest.mark.parametrize('scen', 'abcdefghij')
@pytest.mark.parametrize('kind', KINDS)
def test_step_hands_the_library_the_same_calls(rec, kind, scen):
    """(a) two dense parameters; (b) a dense parameter riding as the tail of the table's row launch, which advances; (c) with
    `pre_dense_hook`: rows, hook, dense, and the dense launch advances; (d) two pieces of one table concatenated, fields -1
    falling back to 0; (e) fields -1 with one piece: no slots, no mark; (f) no gradients: a bare dt_adam_advance; (g) a flat
    group whose gradients are the flat views: one launch; (h) gradients as separate tensors, one member strided inside a
    padded slab: scattered, one flat launch; (i) only the strided member has a gradient: contiguous copies, written back;
    (j) the second of two steps: slots and mark reused."""
    assert _run(rec, kind, scen) == EXPECTED[kind][scen]


def test_rmsprop_slot_record_strides(rec):
    """(b) with RMSprop's stamps inside the [V, D + 4] slot record: the strides the row launch is handed"""
    assert _run(rec, 'rmsprop_record', 'b') == EXPECTED['rmsprop_record']['b']


@pytest.mark.parametrize('scen', 'kl')
def test_adam_takes_segments_and_rows_applied_in_step(rec, scen):
    """(k) a segmented gradient; (l) fields -2: neither slots nor mark"""
    assert _run(rec, 'adam', scen) == EXPECTED['adam'][scen]


@pytest.mark.parametrize('scen', 'kl')
@pytest.mark.parametrize('kind', ['adagrad', 'rmsprop'])
def test_slot_optimizers_refuse_segments_and_rows_applied_in_step(rec, kind, scen):
    with pytest.raises(ValueError, match='a sparse gradient with segments or rows applied inside the step'):
        _run(rec, kind, scen)
    assert [name for name, _ in rec.calls] == ['dt_adam_state_init']


def test_adam_refuses_to_concatenate_segments_or_applied_rows(rec):
    seg = tuple(torch.zeros(4, dtype=torch.int32) for _ in range(5)) + (1, 4)
    with pytest.raises(ValueError, match='a segmented sparse gradient cannot be concatenated with other pieces'):
        _table_scenario(rec, 'adam', [_piece([1, 2], segments=seg), _piece([3])])
    with pytest.raises(ValueError, match='applied inside the step cannot be concatenated'):
        _table_scenario(rec, 'adam', [_piece([1, 2], fields=-2), _piece([3], fields=-2)])


def test_adam_applied_in_step_launches_nothing(rec):
    """(m) after `applied_in_step()` the step only drops the gradients; the next one launches again"""
    w1, emb = _param(3, 4), _Emb()
    opt = _opt('adam', [w1, emb.table], [emb])
    w1.grad = torch.ones_like(w1)
    emb.sparse_grads = {'d8': [_piece([1, 3, 7], fields=-2)]}
    opt.applied_in_step()
    opt.step()
    assert rec.calls == [] and emb.sparse_grads == {} and opt._dev_state is None
    opt.step()
    assert [name for name, _ in rec.calls] == ['dt_adam_state_init', 'dt_adam_dense_step']


def test_adam_zero_grad_fails_on_a_broken_promise(rec):
    """(n) a fields -2 gradient still pending at zero_grad(): step() did not follow _forward_backward(apply_rows=True)"""
    emb = _Emb()
    opt = _opt('adam', [emb.table], [emb])
    emb.sparse_grads = {'d8': [_piece([1, 3, 7], fields=-2)]}
    with pytest.raises(RuntimeError, match='was not followed by optimizer.step()'):
        opt.zero_grad()
    opt.applied_in_step()
    opt.zero_grad()
    assert emb.sparse_grads == {} and not opt._applied_in_step


@pytest.mark.parametrize('kind', KINDS)
def test_setting_t(rec, kind):
    """the `t` setter: nothing without parameters; Adam re-initialises the state; the slot optimizers materialize what is
    pending under the old count first and restamp after (RMSprop's row-sparse table)"""
    opt = _opt(kind, [])
    opt.t = 3
    assert rec.calls == [] and opt._dev_state is None
    emb = _Emb()
    opt = _opt(kind, [emb.table], [emb])
    emb.sparse_grads = {'d8': [_piece([1, 3, 7])]}
    opt.step()
    rec.calls.clear()
    opt._dev_state[0] = 6
    opt.t = 5
    assert _decoded(rec, _names(opt, {'table': emb.table})) == EXPECTED[kind]['t']
    if kind == 'rmsprop':
        assert opt.state[id(emb.table)]['stamp'].tolist() == [5] * 10
    assert opt.t == 5
