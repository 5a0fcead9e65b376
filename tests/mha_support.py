# -*- coding:utf-8 -*-
"""Host side of the attention core tests (csrc/mha.hip: dt_mha_core_fwd / dt_mha_core_bwd, reached through ops.mha_core): the
launchers' arithmetic restated in plain Python with the source lines each function restates, the table of cases with the path
each id names, input builders, the float64 reference of deeptables/models/layers.py:129-145 in two forms (the batched matmul of
the reference, and a per-key loop in the order of the kernel's header: running max, exponentials, divide at the end), both
evaluated in float32 on the CPU as the yardstick, and the metrics every figure is measured in.  Nothing here needs a GPU;
tests/test_mha_paths_host.py checks the table against the restatement, the restatement against the library and the two forms
against each other and oracle/closed_form, tests/test_mha_kernels_gpu.py runs the kernels."""
import collections
import math
import zlib

import numpy as np
import torch

from tests import precision as P

F64, F32 = torch.float64, torch.float32
DT_OK, DT_ERR_INVALID_ARG, DT_ERR_UNSUPPORTED = 0, -1, -2


def ceil_div(a, b):
    return -(-a // b)


# ---- csrc/mha.hip: the launchers ---------------------------------------------------------------------------------------------
BRACKETS = (4, 8, 16, 32, 64)                                             # the DHMAX instantiations, mha.hip:264-268
FWD_MAX_DH, BWD_MAX_DH, DROP_MAX_F = 64, 32, 64                           # mha.hip:232
BLOCK = 256                                                               # mha.hip:223, 262


def dhmax(dh, direction):
    """DHMAX of the kernel that runs a head width, or None where the direction refuses it: mha.hip:252, 264-268 (forward),
    :290, 302-305 (backward)"""
    if dh > (FWD_MAX_DH if direction == 'fwd' else BWD_MAX_DH):
        return None
    return next(b for b in BRACKETS if dh <= b)


def vec4(direction, D, H, ld, ldg=None, offsets=()):
    """the float4 predicate: mha.hip:258-259 (forward: q, k, v, out), :295-297 (backward: q, k, v, grad_out and the three
    gradients, and ldg).  offsets: where each pointer the kernel dereferences starts, in floats from a 16-byte aligned address"""
    dh = D // H
    ok = dh % 4 == 0 and D % 4 == 0 and ld % 4 == 0 and all(o % 4 == 0 for o in offsets)
    return ok and (direction == 'fwd' or ldg % 4 == 0)


def path(direction, D, H, ld, ldg=None, offsets=()):
    """'<DHMAX>v' | '<DHMAX>s' | None: the instantiation k_mha_fwd | k_mha_bwd_q and k_mha_bwd_kv <DHMAX, VEC4> a call launches"""
    b = dhmax(D // H, direction)
    return None if b is None else f"{b}{'v' if vec4(direction, D, H, ld, ldg, offsets) else 's'}"


def grid(B, F, H):
    """(blocks, threads of the last block that own a task): mha.hip:261-262, 87-89"""
    total = B * H * F
    blocks = ceil_div(total, BLOCK)
    return blocks, total - (blocks - 1) * BLOCK


def sizes_ok(B, F, D, H):                                                 # mha.hip:234
    return B >= 0 and F > 0 and D > 0 and H > 0 and D % H == 0


def f32(x):
    return float(np.float32(x))


def rate_ok(rate):                                                        # common.h: autoint_drop
    r = f32(rate)
    return r == 0.0 or 0.0 < r < 1.0


def refusal(direction, B, F, D, H, ld, ldg, rate):
    """the code dt_mha_core_fwd / dt_mha_core_bwd returns before any launch, in the order of mha.hip:248-255 / :286-293"""
    if not rate_ok(rate) or not sizes_ok(B, F, D, H) or ld < D or (direction == 'bwd' and ldg < D):
        return DT_ERR_INVALID_ARG
    if dhmax(D // H, direction) is None or (f32(rate) > 0 and F > DROP_MAX_F):
        return DT_ERR_UNSUPPORTED
    return DT_OK


def supported(F, D, H, dropout):
    """dt_mha_core_supported: both directions take the shape (mha.hip:238-242)"""
    return sizes_ok(0, F, D, H) and D // H <= BWD_MAX_DH and not (dropout and F > DROP_MAX_F)


def threshold(rate):
    """dt_autoint_dropout_threshold (common.h: autoint_drop_threshold): float32(rate) * 2^32, exact in double, saturated to
    2^32 - 1, at least 1 for a rate > 0"""
    r = f32(rate)
    if not r > 0.0:
        return 0
    t = r * 4294967296.0
    return max(4294967295 if t >= 4294967295.0 else int(t), 1)


def keep_scale(rate):
    """1.0f / (1.0f - rate) in float32 (common.h: autoint_drop)"""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(rate)))


def dropout_hash(seed, B, H, F):
    """[B, H, F, F] int64: mha_keep's hash, mha.hip:24-25 (dt_autoint_dropout_hash; the host test holds it to the library)"""
    M = 0xFFFFFFFF
    b = torch.arange(B, dtype=torch.int64).view(B, 1, 1, 1)
    h = torch.arange(H, dtype=torch.int64).view(1, H, 1, 1)
    i = torch.arange(F, dtype=torch.int64).view(1, 1, F, 1)
    j = torch.arange(F, dtype=torch.int64).view(1, 1, 1, F)
    x = (int(seed) & M) ^ ((b * 0x9E3779B1) & M) ^ (((h * 4096 + i * 64 + j) * 0x85EBCA77) & M)
    x = x ^ (x >> 16); x = (x * 0x7FEB352D) & M; x = x ^ (x >> 15); x = (x * 0x846CA68B) & M
    return x ^ (x >> 16)


def keep_mask(seed, B, H, F, rate):
    """[B, H, F, F] float64: 0 or fl32(1 / (1 - rate)); None without dropout"""
    if not f32(rate) > 0:
        return None
    return (dropout_hash(seed, B, H, F) >= threshold(rate)).double() * keep_scale(rate)


# ---- the reference: deeptables/models/layers.py:129-145 ------------------------------------------------------------------------
def _heads(t, H):
    B, F, D = t.shape
    return t.reshape(B, F, H, D // H).permute(0, 2, 1, 3)


def mha_matmul(q, k, v, H, keep=None):
    """(out [B, F, D], lse [B, H, F]) in the dtype of q: the reference's op chain as the older tests write it, heads split on
    the last axis and concatenated on the batch axis (layers.py:130-132), one batched matmul each for the scores and the
    weighted sum, the keep mask on the softmax's output (layers.py:141: the normaliser is the undropped one)"""
    B, F, D = q.shape
    dh = D // H
    Q_, K_, V_ = (torch.cat(torch.split(t, dh, dim=2), dim=0) for t in (q, k, v))                  # [H B, F, dh]
    s = torch.matmul(Q_, K_.transpose(1, 2)) / (dh ** 0.5)
    w = torch.softmax(s, dim=-1)
    if keep is not None:
        w = w * keep.to(w.dtype).permute(1, 0, 2, 3).reshape(H * B, F, F)
    out = torch.cat(torch.split(torch.matmul(w, V_), B, dim=0), dim=2)
    return out, torch.logsumexp(s, dim=-1).reshape(H, B, F).permute(1, 0, 2)


def mha_loop(q, k, v, H, keep=None):
    """the same in the order of the kernel (mha.hip:99-120): one key at a time, first the running maximum of the scaled scores,
    then p_j = exp(s_j - m), l += p_j, acc += p_j keep_j v_j, and one division by l at the end; lse = m + log l"""
    qh, kh, vh = _heads(q, H), _heads(k, H), _heads(v, H)                                          # [B, H, F, dh]
    F, dh = qh.shape[2], qh.shape[3]
    scale = 1.0 / torch.sqrt(torch.tensor(float(dh), dtype=q.dtype))
    s = [(qh * kh[:, :, j:j + 1, :]).sum(-1) * scale for j in range(F)]                           # each [B, H, F(i)]
    m = s[0]
    for j in range(1, F):
        m = torch.maximum(m, s[j])
    l, acc = torch.zeros_like(m), torch.zeros_like(qh)
    for j in range(F):
        p = torch.exp(s[j] - m)
        l = l + p
        pk = p if keep is None else p * keep[:, :, :, j].to(p.dtype)
        acc = acc + pk[..., None] * vh[:, :, j:j + 1, :]
    out = acc / l[..., None]
    return out.permute(0, 2, 1, 3).reshape(q.shape), m + torch.log(l)


NAMES = ('out', 'lse', 'grad_q', 'grad_k', 'grad_v')
DIRECTION = {'out': 'fwd', 'lse': 'fwd', 'grad_q': 'bwd', 'grad_k': 'bwd', 'grad_v': 'bwd'}
METRICS = ('max_rel', 'row_rel')


def evaluate(form, q, k, v, up, H, keep, dt):
    """{name: tensor} of one form in `dt`: forward, and the gradients of sum(out * up) from autograd"""
    xs = [t.to(dt).clone().requires_grad_(True) for t in (q, k, v)]
    out, lse = form(*xs, H, keep)
    (out * up.to(dt)).sum().backward()
    return dict(zip(NAMES, [out.detach(), lse.detach()] + [t.grad for t in xs]))


def rows_of(name, t):
    """the rows row_rel measures: one (b, f) row of D entries for out and the gradients, so a field scaled 1e-3 is measured
    against itself; one (b, h) row of F entries for lse (a log-sum-exp may cross zero: an entry near zero has no relative
    error two evaluation orders agree on, its neighbours in the same softmax problem give it its scale)"""
    return t.reshape(-1, t.shape[-1])


def errors(name, got, ref):
    return {'max_rel': P.max_rel(got, ref), 'row_rel': P.row_rel(rows_of(name, got), rows_of(name, ref))}


Refs = collections.namedtuple('Refs', 'q k v up keep r64 loop64 yard')
_REFS = {}


def references(c):
    """inputs, the float64 reference (matmul form), the loop form in float64 and the float32 yardstick {name: {metric: the
    larger of the two forms' float32 errors against float64}} of one case: computed once and shared, never written to"""
    if c.id not in _REFS:
        q, k, v, up = build_inputs(c)
        keep = keep_mask(c.seed, c.B, c.H, c.F, c.rate)
        r64 = evaluate(mha_matmul, q, k, v, up, c.H, keep, F64)
        loop64 = evaluate(mha_loop, q, k, v, up, c.H, keep, F64)
        e32 = [evaluate(form, q, k, v, up, c.H, keep, F32) for form in (mha_matmul, mha_loop)]
        yard = {n: {m: max(errors(n, e[n], r64[n])[m] for e in e32) for m in METRICS} for n in NAMES}
        _REFS[c.id] = Refs(q, k, v, up, keep, r64, loop64, yard)
    return _REFS[c.id]


def figures(got, r64, yard, names=NAMES):
    """the figures of precision.check_step for the tensors in `got`: '<name>:<metric>' -> (direction, err_gpu, err_f32)"""
    figs = {}
    for n in names:
        assert tuple(got[n].shape) == tuple(r64[n].shape), (n, got[n].shape, r64[n].shape)
        assert bool(torch.isfinite(got[n]).all()), f'{n} is not finite'
        e = errors(n, got[n], r64[n])
        for m in METRICS:
            figs[f'{n}:{m}'] = (DIRECTION.get(n, 'bwd'), e[m], yard[n][m])
    return figs


def check(test, got, ref, names=NAMES):
    """err_gpu <= STEP_BAR['fp32'] x max(err_float32, 2^-24) in max_rel and row_rel for every tensor in `names`"""
    P.check_step(test, 'mha', 'float32', figures(got, ref.r64, ref.yard, names))


# ---- the cases -----------------------------------------------------------------------------------------------------------------
LAYOUTS = ('contig', 'prod', 'odd')
DATA = ('mild', 'signed', 'logits30', 'q1000', 'q0', 'fields')
Case = collections.namedtuple('Case', 'id B F D H layout rate seed data lse expect')


def strides(c):
    """(ld, ldg) of a layout: contiguous | the production layout, q, k, v column blocks of one [B, F, 4 D] projection output and
    the gradients of one [B, F, 4 D] buffer (models/layers.py: ops.split_cols + ops.mha_core(grad_cols=4)) | one float more
    than contiguous, which no float4 can take"""
    return {'contig': (c.D, 3 * c.D), 'prod': (4 * c.D, 4 * c.D), 'odd': (c.D + 1, 3 * c.D + 1)}[c.layout]


def plan(c, offset=0):
    """what the restatement says of a case.  offset: floats every buffer is shifted by from its 16-byte aligned start"""
    ld, ldg = strides(c)
    blocks, tail = grid(c.B, c.F, c.H)
    offs = (offset,)
    return {'fwd': path('fwd', c.D, c.H, ld, offsets=offs), 'bwd': path('bwd', c.D, c.H, ld, ldg, offs), 'dh': c.D // c.H,
            'blocks': blocks, 'tail': tail, 'thr': threshold(c.rate), 'bh_per_wave': 64 / c.F}


def case(tag, B, F, D, H, layout='contig', rate=0.0, seed=0, data='mild', lse=True, **expect):
    """id: shape, layout, the forward and the backward instantiation the case says it takes (the host test holds them to the
    restatement), and what it is there for"""
    assert 'fwd' in expect and 'bwd' in expect
    drop = f'-p{rate:g}' if rate else ''
    return Case(f"B{B}-F{F}-D{D}-H{H}-{layout}{drop}-fwd{expect['fwd']}-bwd{expect['bwd']}-{tag}", B, F, D, H, layout, rate,
                seed, data, lse, expect)


def _width_cases():
    # (dh, D, H, forward, backward): every head width of the table, contiguous
    W = [(1, 3, 3, '4s', '4s'), (2, 2, 1, '4s', '4s'), (3, 6, 2, '4s', '4s'), (4, 4, 1, '4v', '4v'), (5, 5, 1, '8s', '8s'),
         (6, 12, 2, '8s', '8s'), (8, 16, 2, '8v', '8v'), (12, 24, 2, '16v', '16v'), (16, 16, 1, '16v', '16v'),
         (17, 17, 1, '32s', '32s'), (20, 40, 2, '32v', '32v'), (32, 32, 1, '32v', '32v'),
         (33, 33, 1, '64s', None), (36, 72, 2, '64v', None), (64, 64, 1, '64v', None)]
    return [case(f'width{dh}', (3, 2, 5)[n % 3], (5, 7, 3)[n % 3], D, H, fwd=f, bwd=b, dh=dh) for n, (dh, D, H, f, b) in enumerate(W)]


WIDTH_CASES = _width_cases()
LAYOUT_CASES = [
    case('default_config', 3, 5, 4, 1, 'prod', fwd='4v', bwd='4v'), case('pad', 3, 5, 4, 1, 'odd', fwd='4s', bwd='4s'),
    case('blocks', 2, 7, 16, 2, 'prod', fwd='8v', bwd='8v'), case('pad', 2, 7, 16, 2, 'odd', fwd='8s', bwd='8s'),
    case('blocks', 2, 40, 16, 1, 'prod', fwd='16v', bwd='16v'), case('pad', 2, 5, 16, 1, 'odd', fwd='16s', bwd='16s'),
    case('blocks', 3, 5, 64, 2, 'prod', fwd='32v', bwd='32v'), case('pad', 3, 5, 64, 2, 'odd', fwd='32s', bwd='32s'),
    case('blocks', 2, 5, 64, 1, 'prod', fwd='64v', bwd=None), case('pad', 2, 5, 64, 1, 'odd', fwd='64s', bwd=None),
    case('blocks_scalar', 3, 5, 12, 2, 'prod', fwd='8s', bwd='8s'), case('blocks_scalar', 3, 5, 5, 1, 'prod', fwd='8s', bwd='8s'),
    case('no_lse', 3, 5, 8, 2, lse=False, fwd='4v', bwd='4v'), case('no_lse', 3, 5, 6, 2, lse=False, fwd='4s', bwd='4s'),
]
GRID_CASES = [
    case('grid_255', 51, 5, 4, 1, fwd='4v', bwd='4v', blocks=1, tail=255),
    case('grid_256', 32, 4, 8, 2, fwd='4v', bwd='4v', blocks=1, tail=256),
    case('grid_257', 257, 1, 4, 1, fwd='4v', bwd='4v', blocks=2, tail=1),
    case('grid_three_blocks_ragged', 43, 5, 6, 3, fwd='4s', bwd='4s', blocks=3, tail=133),
    case('one_field', 3, 1, 8, 2, fwd='4v', bwd='4v'),
    case('wave_spans_ten_heads', 11, 3, 10, 2, fwd='8s', bwd='8s'),
    case('fields_65', 2, 65, 8, 2, fwd='4v', bwd='4v', blocks=2, tail=4),
    case('fields_70', 2, 70, 6, 2, fwd='4s', bwd='4s', blocks=2, tail=24),
]
EMPTY_BATCH = (0, 5, 8, 2)                                                # (B, F, D, H): returns DT_OK and touches nothing
DROP_RATES = (0.1, 0.3, 0.5, 0.9)
TINY_RATE = 1e-12                                                         # float32(rate) * 2^32 < 1: the threshold clamps to 1
DROP_CASES = [case('dropout_at_the_field_limit', 2, 64, 12, 3, rate=r, seed=1000 + n, fwd='4v', bwd='4v')
              for n, r in enumerate(DROP_RATES)] + \
             [case('dropout_small', 16, 5, 6, 3, rate=r, seed=2000 + n, fwd='4s', bwd='4s') for n, r in enumerate(DROP_RATES)] + \
             [case('dropout_threshold_clamped', 3, 5, 8, 2, rate=TINY_RATE, seed=77, fwd='4v', bwd='4v', thr=1),
              case('dropout_blocks', 4, 26, 24, 3, 'prod', rate=0.3, seed=991, fwd='8v', bwd='8v'),
              case('dropout_pad', 4, 26, 24, 3, 'odd', rate=0.3, seed=991, fwd='8s', bwd='8s')]
HARD_SHAPES = ((3, 7, 8, 2, 'contig', '4v'), (3, 7, 12, 2, 'contig', '8s'), (2, 33, 32, 2, 'prod', '16v'))
HARD_CASES = [case(f'hard_{d}', B, F, D, H, lay, data=d, fwd=p, bwd=p) for B, F, D, H, lay, p in HARD_SHAPES for d in DATA[1:]]
CASES = WIDTH_CASES + LAYOUT_CASES + GRID_CASES + DROP_CASES + HARD_CASES
# the same values through the float4 and the one-float kernels: (contiguous, padded) pairs with equal shape, rate and seed
PAIRS = [(LAYOUT_CASES[n], LAYOUT_CASES[n + 1]) for n in (0, 2, 6)] + [(DROP_CASES[-2], DROP_CASES[-1])]
# buffers that start one float past a 16-byte boundary: the float4 shape on the one-float kernels (fix 3)
OFFSET_CASE = case('offset_by_one_float', 3, 5, 16, 2, fwd='8v', bwd='8v')
# outside the domain: (F, D, H, rate) -> what each direction returns
REFUSED = {(5, 40, 1, 0.0): (DT_OK, DT_ERR_UNSUPPORTED), (5, 64, 1, 0.0): (DT_OK, DT_ERR_UNSUPPORTED),
           (4, 65, 1, 0.0): (DT_ERR_UNSUPPORTED, DT_ERR_UNSUPPORTED), (65, 8, 2, 0.3): (DT_ERR_UNSUPPORTED, DT_ERR_UNSUPPORTED)}


def refused_case(F, D, H, rate):
    return Case(f'B2-F{F}-D{D}-H{H}-p{rate:g}-outside_the_domain', 2, F, D, H, 'contig', rate, 5, 'mild', True, {})


# through ops.dense + ops.split_cols + ops.mha_core(grad_cols=4) + residual + relu: (B, F, D, H)
LAYER_SHAPES = ((3, 5, 4, 1), (3, 40, 8, 2))

assert len({c.id for c in CASES + [OFFSET_CASE]}) == len(CASES) + 1


def rnd(g, shape, scale=1.0):
    """float64 values that float32 holds exactly: the kernel and the reference see the same inputs"""
    return (torch.randn(shape, generator=g, dtype=F64) * scale).float().double()


def _gen(tag):
    return torch.Generator().manual_seed(zlib.crc32(tag.encode()))


def build_inputs(c, same_as=None):
    """q, k, v [B, F, D] and the upstream gradient, float64 values float32 holds.  mild: relu(N(0, 1)), what the layer's relu
    projections hand the kernel.  The generator depends on the shape and the data only, so the cases of a pair see the same
    values."""
    g = _gen(f'{c.B}-{c.F}-{c.D}-{c.H}-{c.data}')
    shape = (c.B, c.F, c.D)
    q, k, v = (rnd(g, shape) for _ in range(3))
    up = rnd(g, shape)
    if c.data != 'signed':
        q, k, v = torch.relu(q), torch.relu(k), torch.relu(v)
    if c.data == 'logits30':
        q = q * 30.0
    elif c.data == 'q1000':                                    # a one-hot softmax: exp overflows without the max
        q = q * 1000.0
    elif c.data == 'q0':                                       # uniform weights; grad_k = sum_i dS_ir q_i is exactly zero
        q = torch.zeros_like(q)
    elif c.data == 'fields':
        s = torch.logspace(-3, 3, c.F, dtype=F64)[None, :, None]
        q, k, v = q * s, k * s, v * s
    assert c.data in DATA, c.data
    return [t.float().double() for t in (q, k, v, up)]


# ---- through ops: the default-config layer without its BatchNormalization -----------------------------------------------------
def build_layer(B, F, D, H):
    g = _gen(f'layer-{B}-{F}-{D}-{H}')
    return {'x': rnd(g, (B, F, D)), 'W': rnd(g, (D, 4 * D), 1.0 / math.sqrt(D)), 'b': rnd(g, (4 * D,), 0.1), 'up': rnd(g, (B, F, D))}


def layer_pre(x, W, b):
    return x @ W + b


def layer_forward(x, W, b, H, form=mha_matmul):
    """models/layers.py:119-150 of the reference without the BatchNormalization: the four relu projections as one [D, 4 D]
    product, the attention core, the residual, relu"""
    D = x.shape[-1]
    y = torch.relu(layer_pre(x, W, b))
    q, k, v, r = (y[..., i * D:(i + 1) * D] for i in range(4))
    return torch.relu(form(q, k, v, H)[0] + r)


LAYER_NAMES = ('out', 'grad_x', 'grad_W', 'grad_b')


def layer_evaluate(t, H, dt, form=mha_matmul):
    xs = [t[n].to(dt).clone().requires_grad_(True) for n in ('x', 'W', 'b')]
    out = layer_forward(*xs, H, form)
    (out * t['up'].to(dt)).sum().backward()
    return dict(zip(LAYER_NAMES, [out.detach()] + [a.grad for a in xs]))


_LAYER = {}


def layer_references(shape):
    """(inputs, float64 reference, float32 yardstick) of one layer shape, as `references`"""
    if shape not in _LAYER:
        B, F, D, H = shape
        t = build_layer(B, F, D, H)
        r64 = layer_evaluate(t, H, F64)
        e32 = [layer_evaluate(t, H, F32, form) for form in (mha_matmul, mha_loop)]
        yard = {n: {m: max(errors(n, e[n], r64[n])[m] for e in e32) for m in METRICS} for n in LAYER_NAMES}
        _LAYER[shape] = (t, r64, yard)
    return _LAYER[shape]


def params_of(cases):
    import pytest
    return [pytest.param(c, id=c.id) for c in cases]
