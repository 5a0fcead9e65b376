# -*- coding:utf-8 -*-
"""The calls tools/make_optimizer_golden.py records and tests/test_optimizer_family_golden_gpu.py replays: dense, multi-tensor
and row steps of the seven slot-optimizer kinds (csrc/optim_slots.hip), driven through the C entry points alone, so that the
same calls run on any build of the library with this C ABI.

Inputs come from seeded CPU generators (one per case, seeded by the case's name).  Row gradients sit on a 2^-6 grid with
|g| <= 4: the sum of a row's duplicate lookups is then exact in float32 whatever order the merge's atomics take, and every
output is a pure function of the inputs.

`run(lib)` -> (inputs_hash, {'<case>/<array>': tensor on the CPU}).  The fixture keeps a 16-byte BLAKE2b digest of each
output array's bytes, not the arrays: the cases write 5.5 MB of weights and slots.  Equal digests mean equal
bytes, which for finite values is at least `torch.equal` (it also tells -0 from 0); the test checks that they are finite."""
import ctypes
import hashlib
import zlib

import numpy as np
import torch

STATE_WORDS = 272 // 4            # DT_ADAM_STATE_BYTES (include/dt_hip.h) in int32 words
LR = 1e-2
FTRL_REG = (0.02, 0.01, 0.01)     # l1, l2 (+ beta / (2 lr), folded by the caller), l2_shrinkage
# kind -> (entry-point stem, hyperparameters in the entry points' order, initial value of each slot, steps done at the start)
KINDS = {
    'adagrad': ('adagrad', (LR, 1e-7), (0.1,), 0),
    'rmsprop': ('rmsprop', (LR, 0.9, 1e-7), (0.0,), 0),
    'sgdm': ('sgdm', (LR, 0.9, 0), (0.0,), 0),
    'sgdm_nesterov': ('sgdm', (LR, 0.9, 1), (0.0,), 0),
    'adamax': ('adamax', (LR, 0.9, 0.999, 1e-7), (0.0, 0.0), 0),
    'adamax_from_1000': ('adamax', (LR, 0.9, 0.999, 1e-7), (0.0, 0.0), 1000),
    'ftrl_sqrt': ('ftrl', (LR, -0.5) + FTRL_REG, (0.1, 0.0), 0),
    'ftrl_pow': ('ftrl', (LR, -0.3) + FTRL_REG, (0.1, 0.0), 0),
}
DENSE_N = (1, 3, 257, 1031)       # + 1031 again, every array one float off its 16-byte alignment: the scalar path
DENSE_STEPS = 3
MULTI_TENSORS = 33                # 1 .. 33 elements: one tensor past the 32-tensor chunk
ROW_STEPS = 4
TAIL_N = 1031
# D -> (V, lookups): one piece per row and 64 rows per block; the scalar path; 4 pieces; 257 pieces (a thread walks)
ROW_SHAPES = {4: (40, 96), 6: (40, 96), 16: (40, 96), 1028: (6, 8)}
ROW_FIELDS = (0, 4, -1)
RMS_JUMP_AFTER, RMS_JUMP_TO = 2, 20          # dt_adam_state_init(steps_done = 20) after step 2: idle > 8 takes powf


def _dev():
    return torch.device('cuda', 0)


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _check(lib, rc, what):
    assert rc == 0, f'{what}: {lib.dt_last_error().decode()}'


class _Inputs:
    """seeded CPU tensors; every one of them enters the inputs' hash"""

    def __init__(self):
        self.hash = hashlib.sha256()

    def gen(self, case):
        return torch.Generator().manual_seed(zlib.crc32(case.encode()))

    def take(self, case, t):
        self.hash.update(case.encode())
        self.hash.update(t.numpy().tobytes())
        return t


def _offset_copy(t, off):
    """t on the device, `off` floats behind a 16-byte aligned address"""
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device=_dev())
    view = buf[off:]
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 * off
    return view


def _new_state(lib, steps_done):
    st = torch.zeros(STATE_WORDS, dtype=torch.int32, device=_dev())
    _check(lib, lib.dt_adam_state_init(_ptr(st), LR, 0.0, 0.0, steps_done, _stream()), 'dt_adam_state_init')
    return st


def _dense(lib, inp, out):
    for kind, (stem, hp, inits, done) in KINDS.items():
        f = getattr(lib, f'dt_{stem}_dense_step')
        for n, off in [(n, 0) for n in DENSE_N] + [(DENSE_N[-1], 1)]:
            case = f'dense/{kind}/n{n}' + ('_off1' if off else '')
            g = inp.gen(case)
            p = _offset_copy(inp.take(case, torch.randn(n, generator=g)), off)
            grad = inp.take(case, torch.randn(n, generator=g))
            slots = [_offset_copy(torch.full((n,), v), off) for v in inits]
            st = _new_state(lib, done)
            for k in range(DENSE_STEPS):          # gradients alternate between 0.1 x and 3 x
                gk = _offset_copy(grad * (0.1 if k % 2 == 0 else 3.0), off)
                _check(lib, f(_ptr(p), _ptr(gk), *map(_ptr, slots), n, *hp, _ptr(st), 1, _stream()), case)
            out[case + '/p'] = p
            for i, s in enumerate(slots):
                out[f'{case}/slot{i}'] = s
            out[case + '/t'] = st[:1]


def _multi(lib, inp, out):
    T = MULTI_TENSORS
    arr = lambda ts: ctypes.cast((ctypes.c_void_p * T)(*[t.data_ptr() for t in ts]), ctypes.c_void_p)
    for kind, (stem, hp, inits, done) in KINDS.items():
        case = f'multi/{kind}'
        g = inp.gen(case)
        ps = [inp.take(case, torch.randn(n, generator=g)).to(_dev()) for n in range(1, T + 1)]
        gs = [inp.take(case, torch.randn(n, generator=g)).to(_dev()) for n in range(1, T + 1)]
        slots = [[torch.full((n,), v, device=_dev()) for n in range(1, T + 1)] for v in inits]
        ns = ctypes.cast((ctypes.c_int64 * T)(*range(1, T + 1)), ctypes.c_void_p)
        st = _new_state(lib, done)
        _check(lib, getattr(lib, f'dt_{stem}_multi_step')(T, arr(ps), arr(gs), *[arr(s) for s in slots], ns, *hp, _ptr(st), 1,
                                                           _stream()), case)
        out[case + '/p'] = torch.cat(ps)
        for i, s in enumerate(slots):
            out[f'{case}/slot{i}'] = torch.cat(s)
        out[case + '/t'] = st[:1]


def _lookups(case, inp, g, V, n, fields):
    """row ids of one launch: duplicates and a few -1 (fields 0 and 4), ids inside their field's range (4), distinct (-1)"""
    if fields == -1:
        rows = torch.randperm(V, generator=g)[:min(n, V * 4 // 5)].clone()
    elif fields == 0:
        rows = torch.randint(0, V, (n,), generator=g)
    else:
        lo = torch.tensor([V * f // fields for f in range(fields)])
        hi = torch.tensor([V * (f + 1) // fields for f in range(fields)])
        f = torch.arange(n) % fields                          # occurrence i belongs to field i % fields
        rows = lo[f] + (torch.rand(n, generator=g) * (hi - lo)[f]).long()
    rows[1::max(3, n // 3)] = -1
    return inp.take(case, rows)


def _rows(lib, inp, out):
    dev = _dev()
    layouts = {k: (k, False) for k in KINDS}
    layouts['rmsprop_in_record'] = ('rmsprop', True)          # the stamps in the last column of a [V, D + 4] record
    for name, (kind, in_record) in layouts.items():
        stem, hp, inits, done = KINDS[kind]
        f = getattr(lib, f'dt_{stem}_rows_step')
        rms = stem == 'rmsprop'
        for D, (V, n_look) in ROW_SHAPES.items():
            for fields in ROW_FIELDS:
                for tail_n in (TAIL_N, 0):
                    case = f'rows/{name}/D{D}/fields{fields}/tail{tail_n}'
                    g = inp.gen(case)
                    table = inp.take(case, 0.05 * torch.randn(V, D, generator=g)).to(dev)
                    stamp = None
                    if in_record:
                        rec = torch.zeros(V, D + 4, device=dev)
                        slots, stamp = [rec[:, :D]], rec[:, D].view(torch.int32)
                    elif len(inits) == 2:                     # ONE [V, 2, D] record, as training.py allocates it
                        rec = torch.empty(V, 2, D, device=dev)
                        slots = [rec[:, 0, :], rec[:, 1, :]]
                    else:
                        rec = torch.empty(V, D, device=dev)
                        slots = [rec]
                    for s, v in zip(slots, inits):
                        s.fill_(v)
                    if rms:
                        stamp = torch.zeros(V, dtype=torch.int32, device=dev) if stamp is None else stamp
                        stamp.fill_(done)                     # nothing is pending on a new slot
                    tp = inp.take(case, torch.randn(tail_n, generator=g)).to(dev) if tail_n else None
                    tslots = [torch.full((tail_n,), v, device=dev) if tail_n else None for v in inits]
                    st = _new_state(lib, done)
                    for k in range(ROW_STEPS):
                        for launch in range(2):               # two launches a step: the last carries the tail and advances
                            last = launch == 1
                            rows = _lookups(case, inp, g, V, n_look, fields)
                            n = rows.numel()
                            vals = inp.take(case, torch.randint(-256, 257, (n, D), generator=g).float() / 64).to(dev)
                            rows = rows.to(dev)
                            n_slots = lib.dt_adam_rows_slots(n) if fields != -1 else 0
                            hslots = torch.zeros(n_slots, dtype=torch.int64, device=dev) if n_slots else None
                            mark = torch.empty(n, dtype=torch.int32, device=dev) if n_slots else None
                            tg = inp.take(case, torch.randn(tail_n, generator=g)).to(dev) if (tail_n and last) else None
                            tl = ([tp, tg] + tslots + [tail_n]) if tg is not None else ([None, None] + [None] * len(inits) + [0])
                            args = [_ptr(table)] + [_ptr(s) for s in slots] + ([_ptr(stamp)] if rms else []) + \
                                [_ptr(rows), _ptr(vals), n, D, fields, _ptr(hslots), n_slots, _ptr(mark), *hp, _ptr(st)] + \
                                [_ptr(x) for x in tl[:-1]] + [tl[-1], 1 if last else 0, int(slots[0].stride(0))] + \
                                ([int(stamp.stride(0))] if rms else []) + [_stream()]
                            _check(lib, f(*args), case)
                        if rms and k + 1 == RMS_JUMP_AFTER:
                            _check(lib, lib.dt_adam_state_init(_ptr(st), LR, 0.0, 0.0, RMS_JUMP_TO, _stream()), case)
                    out[case + '/table'] = table
                    for i, s in enumerate(slots):
                        out[f'{case}/slot{i}'] = s.clone()
                    if rms:                                   # ... and once more with the pending decay applied
                        out[case + '/stamp'] = stamp.clone()
                        _check(lib, lib.dt_rmsprop_rows_materialize(_ptr(slots[0]), _ptr(stamp), V, D, int(slots[0].stride(0)),
                                                                    int(stamp.stride(0)), hp[1], _ptr(st), _stream()), case)
                        out[case + '/materialized/slot0'] = slots[0].clone()
                        out[case + '/materialized/stamp'] = stamp.clone()
                    if tail_n:
                        out[case + '/tail_p'] = tp
                        for i, s in enumerate(tslots):
                            out[f'{case}/tail_slot{i}'] = s
                    out[case + '/t'] = st[:1]


def run(lib):
    inp, out = _Inputs(), {}
    _dense(lib, inp, out)
    _multi(lib, inp, out)
    _rows(lib, inp, out)
    torch.cuda.synchronize()
    return inp.hash.hexdigest(), {k: v.detach().cpu().contiguous() for k, v in out.items()}


def digest(t):
    return np.frombuffer(hashlib.blake2b(t.numpy().tobytes(), digest_size=16).digest(), dtype=np.uint8)
