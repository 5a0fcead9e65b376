# -*- coding:utf-8 -*-
"""Host side of the embedding / FM / feed kernel tests (csrc/embedding.hip) and of the cross-net tests (csrc/cross.hip): the
launchers' arithmetic restated in plain Python with the source lines each function restates, the table of cases with the path
each id names, input builders, the float64 / float32 CPU references written out from the formulas in the kernels' header
comments, and the scale every figure is divided by.  Nothing here needs a GPU; tests/test_rows_paths_host.py checks the table
against the restatement, the restatement against the library and the references against oracle/reference_layers,
tests/test_rows_kernels_gpu.py runs the kernels."""
import collections
import zlib

import numpy as np
import torch

from tests import precision as P

F64, F32, I32, I64 = torch.float64, torch.float32, torch.int32, torch.int64
KINDS = ('i32', 'f32')
LDS_64K = 64 * 1024
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31


def ceil_div(a, b):
    return -(-a // b)


# ---- csrc/embedding.hip ------------------------------------------------------------------------------------------------------
LPRS = (1, 2, 4, 8, 16, 32, 64)


def fast_lpr(D):                                                          # embedding.hip:299-305
    """LPR of the fast row kernels, or None: the generic path"""
    if D % 4:
        return None
    l = D // 4
    return l if 1 <= l <= 64 and not (l & (l - 1)) else None


def row_trips(F, lpr):                                                    # embedding.hip:37-39, 99-100
    return ceil_div(F * lpr, 64)


def row_fill(F, lpr):
    """how the 64-lane trips of a row are filled: 'part' one partly filled trip | 'full' exactly 64 float4 | 'ragged' two trips,
    the second partly filled | 'multi' three trips or more | 'two_full' (LPR = 64, F = 2: every trip of that kernel is full)"""
    nv = F * lpr
    if nv < 64:
        return 'part'
    if nv == 64:
        return 'full'
    if nv < 128:
        return 'ragged'
    return 'two_full' if nv == 128 else 'multi'


def row_grid(B, D):
    """(blocks, threads) of launch_row_fwd / launch_row_bwd: embedding.hip:314, 332, 344, 357"""
    return (ceil_div(B, 4), 256) if fast_lpr(D) else (B, 64)


def generic_lds(F, D):                                                    # embedding.hip:327
    return F * D * 4


def row_fwd_refused(F, D):                                                # embedding.hip:326-331 (the generic forward only)
    return fast_lpr(D) is None and generic_lds(F, D) > LDS_64K


def _capped(total, per_block, cap):
    blocks = min(ceil_div(total, per_block), cap)
    return blocks, ceil_div(total, blocks * per_block)


def gather_path(D):                                                       # embedding.hip:377, 392-397
    return 'vec4' if D % 4 == 0 else 'generic'


def gather_grid(B, F, D):
    """(blocks, loop steps of the busiest thread) of k_gather_vec4: embedding.hip:378-381, 233-234"""
    return _capped(B * F * (D // 4), 256, 256 * 16)


def scatter_grid(n, D):                                                   # embedding.hip:428-430, 289-290
    return _capped(n * D, 256, 256 * 16)


def owned_grid(W, Fo, B, D):                                              # embedding.hip:407, 410-411, 264-265
    return _capped(W * Fo * B * (D // 4), 256, 256 * 32)


FEED_ROWS_PER_BLOCK, FEED_MAX_BLOCKS, FEED_GROUPS = 32, 256 * 64, 32     # embedding.hip:575-576, 507
FEED_CURSOR_WORDS = 16 * (1 + FEED_GROUPS)                                # include/dt_hip.h DT_FEED_CURSOR_WORDS


def feed_grid(n_rows):                                                    # embedding.hip:575-576
    return min(ceil_div(n_rows, FEED_ROWS_PER_BLOCK), FEED_MAX_BLOCKS)


def feed_G(blocks):                                                       # embedding.hip:539
    return min(blocks, FEED_GROUPS)


def feed_members(blocks, g):                                              # embedding.hip:540
    G = feed_G(blocks)
    return (blocks - g + G - 1) // G


def feed_passes(n_rows):
    """row groups of 8 the busiest wave walks: embedding.hip:514-516"""
    return ceil_div(n_rows, feed_grid(n_rows) * 4 * 8)


# ---- csrc/cross.hip ----------------------------------------------------------------------------------------------------------
CROSS_MAX_BLOCKS, CROSS_FWD_MAX_BLOCKS = 512, 2048                        # cross.hip:19, 266
CROSS_PERS = (1, 2, 3, 4, 5, 6, 7, 8, 16, 32)


def cross_per(C):                                                         # cross.hip:240-246
    need = ceil_div(C, 64)
    if need <= 8:
        return need
    per = 16
    while per < need:
        per <<= 1
    return per


def cross_blocks(B):                                                      # cross.hip:235-239
    return max(1, min(ceil_div(B, 4), CROSS_MAX_BLOCKS))


def cross_fwd_blocks(B):                                                  # cross.hip:265-266
    return min(ceil_div(B, 4), CROSS_FWD_MAX_BLOCKS)


def cross_workspace_bytes(B, C, L):                                       # cross.hip:252-255
    return 0 if min(B, C, L) <= 0 else 4 * cross_blocks(B) * 2 * L * C


def cross_fwd_refused(C):                                                 # cross.hip:263
    return cross_per(C) > 32


def cross_bwd_lds(C, L):                                                  # cross.hip:289
    return 2 * L * C * 4


def cross_bwd_refusal(C, L):
    """None, or what dt_cross_bwd's message names: cross.hip:288, 290"""
    if cross_per(C) > 32:
        return 'C'
    return 'LDS' if cross_bwd_lds(C, L) > LDS_64K else None


def cross_bwd_kernel(C, L):
    """'reg4' | 'reg8' | 'generic': DT_CROSS_BWD, cross.hip:298-306.  The macro also asks for 2 * lds <= 64 KiB before either
    register kernel (they stage w and bias behind the accumulators); that condition can never be false once L <= 8 and P <= 8:
    P <= 8 means C <= 512, so L C <= 4,096 floats and 2 * lds = 16 L C <= 65,536 bytes.  It is restated as it stands."""
    P_, lds = cross_per(C), cross_bwd_lds(C, L)
    if L <= 4 and P_ <= 8 and 2 * lds <= LDS_64K:
        return 'reg4'
    if L <= 8 and P_ <= 8 and 2 * lds <= LDS_64K:
        return 'reg8'
    return 'generic'


def reduce_plan(nblocks):
    """(trips of the two-partials loop of lane 0, whether any lane takes the tail) of k_cross_bwd_reduce: cross.hip:220-225"""
    loops, tail = 0, False
    for lane in range(64):
        k, n = lane, 0
        while k + 64 < nblocks:
            k, n = k + 128, n + 1
        loops, tail = max(loops, n), tail or k < nblocks
    return loops, tail


# ---- helpers -----------------------------------------------------------------------------------------------------------------
def rnd(g, shape, scale=1.0):
    """float64 values that float32 holds exactly: the kernel and the reference see the same inputs"""
    return (torch.randn(shape, generator=g, dtype=F64) * scale).float().double()


def _gen(tag, seed=0):
    return torch.Generator().manual_seed(zlib.crc32(tag.encode()) + seed)


def errs(name, got, r64, r32, scale):
    """(elem_cond of the kernel, elem_cond of the float32 reference) of one figure against float64"""
    assert tuple(got.shape) == tuple(r64.shape), (name, got.shape, r64.shape)
    assert bool(torch.isfinite(got).all()), f'{name} is not finite'
    return P.elem_cond(got, r64, scale), P.elem_cond(r32, r64, scale)


def check(test, kernel, figs):
    """figs: {name: (direction, got, r64, r32, scale)} -> precision.check_step on the elem_cond figures: err_gpu <=
    STEP_BAR['fp32'] x max(err_float32_reference, 2^-24)"""
    P.check_step(test, kernel, 'float32', {k: (d,) + errs(k, a, e, e32, s) for k, (d, a, e, e32, s) in figs.items()})


# ---- the row operation -------------------------------------------------------------------------------------------------------
RowCase = collections.namedtuple('RowCase', 'id B F D Nd data expect')
ROW_DATA = ('mild', 'logspace', 'offset', 'zero_rows', 'zero_field', 'all_oob', 'ids')
ZERO_FIELD = 1


def row_case(tag, B, F, D, Nd=0, data='mild', **expect):
    return RowCase(f'B{B}-F{F}-D{D}-Nd{Nd}-{tag}', B, F, D, Nd, data, expect)


def row_plan(c):
    lpr = fast_lpr(c.D)
    if lpr is None:
        return {'path': 'generic', 'lds': generic_lds(c.F, c.D), 'f_loops': ceil_div(c.F, 64), 'd_loops': ceil_div(c.D, 64),
                'grid': row_grid(c.B, c.D)}
    return {'path': 'fast', 'lpr': lpr, 'trips': row_trips(c.F, lpr), 'fill': row_fill(c.F, lpr), 'grid': row_grid(c.B, c.D),
            'idle_waves': 4 * ceil_div(c.B, 4) - c.B, 'dense_loops': ceil_div(c.Nd, 64)}


def vocab_of(F):
    return [3 + (5 * f) % 7 for f in range(F)]


# (integer ids, float ids) written over the first lookups of an 'ids' case; v = the vocabulary of the lookup's field
def special_ids(kind, v):
    """[(id, in range?, the table row of the field it reads)]"""
    if kind == 'i32':
        return [(-1, False, None), (v, False, None), (v - 1, True, v - 1), (INT_MAX, False, None), (INT_MIN, False, None)]
    return [(-0.0, True, 0), (0.9, True, 0), (v - 0.1, True, v - 1), (float(v), False, None), (2.0 ** 24, False, None),
            (3e9, False, None), (float('inf'), False, None), (float('-inf'), False, None)]


Rows = collections.namedtuple('Rows', 'idx table row_offset vocab dense ups ok rows')


def build_rows(c, kind):
    """inputs of one row case for one id kind: ids [B, F] (int32 | float32), the packed table [sum vocab, D] float64, row_offset
    int64 [F], vocab int32 [F], dense [B, Nd] | None, the four upstream gradients (emb, concat, field_sum, fm) and, from the
    ids' definition (never from a conversion of the id tensor), which lookups are in range and the packed row each reads"""
    g = _gen(c.id)
    B, F, D, Nd = c.B, c.F, c.D, c.Nd
    vocab = vocab_of(F)
    offs = np.concatenate([[0], np.cumsum(vocab)[:-1]]).astype(np.int64)
    R = int(sum(vocab))
    table = rnd(g, (R, D), 0.5)
    field_of_row = torch.repeat_interleave(torch.arange(F), torch.tensor(vocab))
    if c.data == 'logspace':
        table = (table * torch.logspace(-3, 3, F, dtype=F64)[field_of_row][:, None]).float().double()
    elif c.data == 'offset':                                   # a common offset 100 x the spread
        table = (100.0 + rnd(g, (R, D), 1.0)).float().double()
    elif c.data == 'zero_rows':
        table[::2] = 0.0
    elif c.data == 'zero_field':
        table[field_of_row == ZERO_FIELD] = 0.0
    ids = torch.stack([torch.randint(0, v, (B,), generator=g) for v in vocab], 1)          # [B, F] int64, in range
    ok = torch.ones((B, F), dtype=torch.bool)
    local = ids.clone()
    idx = ids.to(I32) if kind == 'i32' else ids.to(F32)
    if c.data == 'all_oob':
        over = torch.tensor(vocab)[None, :] + torch.randint(0, 5, (B, F), generator=g)
        idx, ok = (over.to(I32) if kind == 'i32' else over.to(F32)), torch.zeros((B, F), dtype=torch.bool)
    elif c.data == 'ids':
        flat, okf, locf = idx.reshape(-1), ok.reshape(-1), local.reshape(-1)
        n = len(special_ids(kind, 1))
        assert B * F >= 2 * n
        for rep in range(2):                                   # twice: at the front of the batch and at its very end
            for k in range(n):
                p = k if rep == 0 else B * F - 1 - k
                val, good, loc = special_ids(kind, vocab[p % F])[k]
                if kind == 'i32':
                    flat[p] = val
                else:
                    flat[p] = torch.tensor(val, dtype=F32)
                okf[p], locf[p] = good, (loc if good else 0)
    rows = torch.where(ok, torch.from_numpy(offs)[None, :] + local, torch.full_like(local, -1))
    dense = rnd(g, (B, Nd)) if Nd else None
    ups = [rnd(g, (B, F, D)), rnd(g, (B, F * D + Nd)), rnd(g, (B, F)), rnd(g, (B,))]
    return Rows(idx, table, torch.from_numpy(offs), torch.tensor(vocab, dtype=I32), dense, ups, ok, rows)


Lookup = collections.namedtuple('Lookup', 'idx table row_offset vocab ok rows')


def build_lookup(tag, lead, F, D, kind, oob_every=7):
    """ids of shape lead + (F,) into a packed table [sum vocab, D], every `oob_every`-th lookup out of range (alternately one past
    the vocabulary and -1) -> Lookup with the table in float64 and, from the ids' definition, the packed row of every lookup"""
    g = _gen(f'{tag}-{lead}-{F}-{D}')
    vocab = vocab_of(F)
    offs = torch.from_numpy(np.concatenate([[0], np.cumsum(vocab)[:-1]]).astype(np.int64))
    n = int(np.prod(lead))
    ids = torch.stack([torch.randint(0, v, (n,), generator=g) for v in vocab], 1)
    ok = torch.ones((n, F), dtype=torch.bool)
    flat, okf = ids.reshape(-1), ok.reshape(-1)
    bad = torch.arange(oob_every - 1, n * F, oob_every)
    flat[bad] = torch.where(torch.arange(len(bad)) % 2 == 0, torch.tensor(vocab)[bad % F], torch.full((len(bad),), -1))
    okf[bad] = False
    rows = torch.where(ok, offs[None, :] + ids, torch.full_like(ids, -1))
    shape = tuple(lead) + (F,)
    return Lookup((ids.to(I32) if kind == 'i32' else ids.to(F32)).reshape(shape), rnd(g, (int(sum(vocab)), D), 0.5), offs,
                  torch.tensor(vocab, dtype=I32), ok.reshape(shape), rows.reshape(shape))


RowRef = collections.namedtuple('RowRef', 'emb concat fsum fm grad_rows grad_table')


def _fsum(t, dim, flip):
    return (t.flip(dim) if flip else t).sum(dim)


def rows_forward(emb, dense, dt, flip=False):
    """concat, field sum and FM of the gathered rows emb [B, F, D] in `dt`, from the header of csrc/embedding.hip:
    concat = [flatten(emb), dense];  field_sum[b, f] = sum_d emb;  fm[b] = 0.5 sum_d ((sum_f emb)^2 - sum_f emb^2)"""
    e = emb.to(dt)
    B = e.shape[0]
    concat = e.reshape(B, -1) if dense is None else torch.cat([e.reshape(B, -1), dense.to(dt)], 1)
    S, Q = _fsum(e, 1, flip), _fsum(e * e, 1, flip)
    return concat, _fsum(e, 2, flip), 0.5 * _fsum(S * S - Q, 1, flip)


def row_gradient(emb, g_emb, g_concat, g_fsum, g_fm, dt, flip=False):
    """grad_rows[b, f, d] = g_emb + g_concat[b, f D + d] + g_field_sum[b, f] + g_fm[b] (S[b, d] - emb[b, f, d]); an absent
    gradient counts as zero (embedding.hip:90)"""
    e = emb.to(dt)
    B, F, D = e.shape
    g = torch.zeros_like(e)
    if g_emb is not None:
        g = g + g_emb.to(dt)
    if g_concat is not None:
        g = g + g_concat.to(dt)[:, :F * D].reshape(B, F, D)
    if g_fsum is not None:
        g = g + g_fsum.to(dt)[:, :, None]
    if g_fm is not None:
        g = g + g_fm.to(dt)[:, None, None] * (_fsum(e, 1, flip)[:, None, :] - e)
    return g


def scatter(rows, g, R, dt, base=None):
    """grad_table[row] += g for every lookup with row >= 0 (embedding.hip:285-296), in lookup order"""
    D = g.shape[-1]
    out = torch.zeros((R, D), dtype=dt) if base is None else base.to(dt).clone()
    rows, g = rows.reshape(-1), g.to(dt).reshape(-1, D)
    live = rows >= 0
    return out.index_add_(0, rows[live], g[live])


def gather(r):
    """emb [B, F, D] float64 of the built inputs: the table row of every lookup in range, zero for the others"""
    return r.table[r.rows.clamp(min=0)] * r.ok[:, :, None].double()


def rows_reference(r, dt, flip=False, which=(True, True, True, True)):
    """every output of the fused forward and backward in `dt` (flip: the sums taken in the opposite order).  `which` says which of
    the four upstream gradients (emb, concat, field_sum, fm) are present."""
    emb = gather(r)
    concat, fsum, fm = rows_forward(emb, r.dense, dt, flip)
    ups = [u if w else None for u, w in zip(r.ups, which)]
    gr = row_gradient(emb, *ups, dt, flip)
    return RowRef(emb.to(dt), concat, fsum, fm, gr, scatter(r.rows, gr, r.table.shape[0], dt))


def rows_scales(r, which=(True, True, True, True)):
    """the sum of the magnitudes of the terms every element is made of, in float64.  FM: 0.5 sum_d ((sum_f |x|)^2 + sum_f x^2):
    the minuend and the subtrahend both count, so F = 1 (true value 0) has a nonzero scale.  The row gradient: |g_emb| +
    |g_concat| + |g_fsum| + |g_fm| (sum_f |x| + |x|)."""
    a = gather(r).abs()
    B, F, D = a.shape
    ups = [u.abs() if w else None for u, w in zip(r.ups, which)]
    s_fm = 0.5 * ((a.sum(1) ** 2).sum(1) + (a * a).sum(1).sum(1))
    s_gr = torch.zeros_like(a)
    if ups[0] is not None:
        s_gr = s_gr + ups[0]
    if ups[1] is not None:
        s_gr = s_gr + ups[1][:, :F * D].reshape(B, F, D)
    if ups[2] is not None:
        s_gr = s_gr + ups[2][:, :, None]
    if ups[3] is not None:
        s_gr = s_gr + ups[3][:, None, None] * (a.sum(1)[:, None, :] + a)
    return RowRef(None, None, a.sum(2), s_fm, s_gr, scatter(r.rows, s_gr, r.table.shape[0], F64))


_ROWS = {}


def rows_refs(c, kind):
    """(inputs, float64 reference, float32 reference, scales) of one case: computed once and shared, never written to"""
    key = (c.id, kind)
    if key not in _ROWS:
        r = build_rows(c, kind)
        _ROWS[key] = (r, rows_reference(r, F64), rows_reference(r, F32), rows_scales(r))
    return _ROWS[key]


def row_figs(got, r64, r32, sc, names=('fsum', 'fm', 'grad_rows', 'grad_table')):
    """the figures of precision.check_step for the outputs present in `got` (a dict)"""
    d = {'fsum': 'fwd', 'fm': 'fwd', 'grad_rows': 'bwd', 'grad_table': 'bwd'}
    return {n: (d[n], got[n], getattr(r64, n), getattr(r32, n), getattr(sc, n)) for n in names if got.get(n) is not None}


def _fast_cases():
    # (F, D) per LPR at the four fillings: one partly filled trip, exactly 64 float4, two trips with a ragged second, >= three
    # trips.  LPR = 64 has no partly filled trip (F = 1 is exactly 64 float4): F = 2 gives two full trips instead.
    FD = {4: (1, 64, 65, 130), 8: (3, 32, 33, 70), 16: (1, 16, 26, 39), 32: (7, 8, 9, 17), 64: (3, 4, 5, 9), 128: (1, 2, 3, 5),
          256: (1, 2, 3)}
    out, k = [], 0
    for D, Fs in FD.items():
        for F in Fs:
            lpr = D // 4
            B, Nd = (1, 3, 5)[k % 3], (0, 1, 13, 70)[k % 4]
            k += 1
            fill = row_fill(F, lpr)
            out.append(row_case(f'lpr{lpr}_{fill}', B, F, D, Nd, path='fast', lpr=lpr, fill=fill, trips=row_trips(F, lpr)))
    return out


FAST_CASES = _fast_cases()
GENERIC_CASES = [
    row_case('generic_D1', 3, 5, 1, 13, path='generic'), row_case('generic_D3', 5, 4, 3, 0, path='generic'),
    row_case('generic_D6', 3, 7, 6, 1, path='generic'), row_case('generic_D10', 1, 4, 10, 70, path='generic'),
    row_case('generic_D12_multiple_of_4', 3, 5, 12, 13, path='generic'),
    row_case('generic_D20_multiple_of_4', 5, 3, 20, 0, path='generic'),
    row_case('generic_D260_d_loop', 3, 3, 260, 1, path='generic', d_loops=5),
    row_case('generic_D512_d_loop', 1, 2, 512, 13, path='generic', d_loops=8),
    row_case('generic_F70_f_loop', 3, 70, 3, 70, path='generic', f_loops=2),
    row_case('generic_at_the_64KiB_limit', 2, 32, 512, 0, path='generic', lds=LDS_64K),
]
ROW_REFUSED = (33, 512)                                     # (F, D): one field past the 64 KiB row buffer
HARD_FAST, HARD_GENERIC = (5, 7, 32, 13), (5, 7, 6, 13)    # LPR = 8 | generic
HARD_ROW_CASES = [row_case(f'hard_{d}', *shape, data=d) for shape in (HARD_FAST, HARD_GENERIC)
                  for d in ('logspace', 'offset', 'zero_rows', 'zero_field', 'all_oob')] + \
                 [row_case('hard_F1', 3, 1, 16, 0), row_case('hard_F1', 3, 1, 6, 0),
                  row_case('hard_F1_offset', 3, 1, 16, 0, data='offset'), row_case('hard_F1_offset', 3, 1, 6, 0, data='offset')]
ID_CASES = [row_case('ids_lpr1', 3, 6, 4, 1, data='ids', lpr=1), row_case('ids_lpr8', 3, 9, 32, 0, data='ids', lpr=8),
            row_case('ids_lpr64', 6, 3, 256, 13, data='ids', lpr=64), row_case('ids_generic', 3, 6, 6, 1, data='ids', path='generic')]
ROW_CASES = FAST_CASES + GENERIC_CASES + HARD_ROW_CASES + ID_CASES
# the C entry points with null outputs / gradients: one fast and one generic shape, out-of-range ids among the lookups
POINTER_CASES = [row_case('pointers_fast', 5, 9, 32, 13, data='ids'), row_case('pointers_generic', 5, 9, 6, 13, data='ids')]

# dt_embedding_fwd alone: (B, F, D)
GATHER_CASES = [(5, 3, 4), (5, 3, 12), (3, 2, 260), (5, 3, 6), (2049, 8, 256)]
# dt_embedding_bwd_dense: (tag, lookups, D, table rows)
SCATTER_WRAP = (4100, 256, 50)
# dt_embedding_gather_owned: (W, B, F, f0, f1, D)
OWNED_CASES = [(1, 5, 6, 0, 2, 16), (3, 5, 6, 2, 4, 16), (3, 4, 6, 4, 6, 8), (1, 5, 6, 3, 3, 16), (3, 1, 6, 0, 6, 4),
               (1, 8193, 2, 1, 2, 1024)]
# dt_feed_gather: (n_rows, row bytes of each block)
FEED_CASES = [(1, (4,)), (7, (12,)), (8, (4, 12, 260)), (9, (1028,)), (33, (4, 12, 260)), (1000, (260, 4, 12)),
              (9, (4, 8, 12, 16, 4, 260, 8, 1028)), (33, (1028, 1028, 4)), (1000, (4, 8, 12, 16, 4, 200, 8, 100)),
              (FEED_MAX_BLOCKS * FEED_ROWS_PER_BLOCK + 1, (4,))]
FEED_CURSOR_LAUNCHES = (33, 1100, 7, FEED_MAX_BLOCKS * FEED_ROWS_PER_BLOCK + 1)      # one cursor through all four
FEED_UNEVEN_GRIDS = (35, 63, 95)                            # blocks: ticket groups of 2 | 1, 2 | 1 and 3 | 2 members


# ---- cross -------------------------------------------------------------------------------------------------------------------
CrossCase = collections.namedtuple('CrossCase', 'id B C L data expect')
CROSS_DATA = ('mild', 'perp', 'w_zero', 'bias_minus_x', 'growth', 'logspace', 'zero_rows', 'zero_column')
ZERO_COLUMN = 1
CROSS_FIGURES = ('y', 'dx', 'dw', 'db')


def cross_case(tag, B, C, L, data='mild', **expect):
    return CrossCase(f'B{B}-C{C}-L{L}-{tag}', B, C, L, data, expect)


def cross_plan(c):
    nb = cross_blocks(c.B)
    loops, tail = reduce_plan(nb)
    return {'per': cross_per(c.C), 'bwd': cross_bwd_kernel(c.C, c.L), 'nblocks': nb, 'fwd_blocks': cross_fwd_blocks(c.B),
            'reduce_loops': loops, 'reduce_tail': tail, 'bwd_stride': c.B > 4 * nb, 'fwd_stride': c.B > 4 * cross_fwd_blocks(c.B),
            'lds': cross_bwd_lds(c.C, c.L)}


def _cross_cases():
    out = []
    Ls = {'reg4': (1, 4), 'reg8': (5, 8), 'generic': (9, 9)}
    for i, C in enumerate((1, 64, 65, 129, 193, 257, 321, 385, 449, 512)):
        for kern, pair in Ls.items():
            L = pair[i % 2]
            out.append(cross_case(f'per{cross_per(C)}_{kern}', 5, C, L, per=cross_per(C), bwd=kern))
    out += [cross_case('per8_reg8_LC_4096', 5, 512, 8, per=8, bwd='reg8', lds=32768),
            cross_case('per16_generic', 5, 513, 2, per=16, bwd='generic'),
            cross_case('per16_generic_at_the_LDS_limit', 3, 1024, 8, per=16, bwd='generic', lds=LDS_64K),
            cross_case('per32_generic', 3, 1025, 3, per=32, bwd='generic'),
            cross_case('per32_generic_at_both_limits', 3, 2048, 4, per=32, bwd='generic', lds=LDS_64K),
            cross_case('no_layers', 5, 65, 0, per=2)]
    for B, nb in ((1, 1), (4, 1), (5, 2), (256, 64), (257, 65), (513, 129), (2048, 512), (2049, 512), (2053, 512)):
        out.append(cross_case(f'grid_{nb}_partials', B, 7, 2, nblocks=nb, bwd='reg4', bwd_stride=B > 2048))
    out += [cross_case('grid_512_partials_generic', 2053, 7, 9, nblocks=512, bwd='generic', bwd_stride=True),
            cross_case('forward_grid_cap', 8193, 7, 1, fwd_blocks=2048, fwd_stride=True)]
    return out


CROSS_PATH_CASES = _cross_cases()
# every hard input on a shallow and a deep shape of each backward family: reg4 | P = 16 generic at L = 2, reg8 | P = 3 generic at L = 8 | 9
HARD_REG, HARD_GEN, HARD_REG_DEEP, HARD_GEN_DEEP = (9, 130, 2), (9, 530, 2), (9, 130, 8), (9, 130, 9)
HARD_CROSS_SHAPES = (HARD_REG, HARD_GEN, HARD_REG_DEEP, HARD_GEN_DEEP)
HARD_CROSS_CASES = [cross_case(f'hard_{d}', *shape, data=d) for shape in HARD_CROSS_SHAPES for d in CROSS_DATA[1:]]
CROSS_CASES = CROSS_PATH_CASES + HARD_CROSS_CASES
CROSS_REFUSED_C = 2049                                       # both directions
CROSS_FORWARD_ONLY = (2048, 5)                               # (C, L): the forward runs, the backward refuses L C = 10,240
CROSS_CONTRACT_CASES = [cross_case('contract_reg', 5, 65, 2, bwd='reg4'), cross_case('contract_generic', 5, 65, 9, bwd='generic')]


CROSS_SCALE_GROWTH = 8.0


def build_cross(c):
    """([x [B, C], w [L, C], bias [L, C]] float64, upstream gradient): x ~ N(0, 0.5), bias ~ N(0, 0.1), and
    w ~ N(0, sigma) with sigma = min(1 / sqrt(C), 1 / (0.8 L max_b sum_c |x|)).

    Why w is that small.  The figures are divided by precision.abs_scale on the whole layer: the L-layer composition on |x|, |w|,
    |b|.  It rightly carries what one layer's cancellation passes on to the next, but it also grows by 1 + sum_c |x| |w| per
    layer whether or not anything cancels.  With w ~ 1 / sqrt(C) that factor is 1 + 0.32 sqrt(C): (8.2)^9 at C = 512, a scale
    1e8 times the value, under which a dropped layer passes.  With E|w| = 0.8 sigma the factor is at most 1 + 1 / L per layer and
    e over L layers, so the scale stays within CROSS_SCALE_GROWTH of |x_0| + sum_l |b_l| at every depth (the host test asserts
    that, and that a dropped layer, a dropped term and a zeroed grad_w row go red on every case).  s_l = x_l . w_l is then of
    order 1 / (L sqrt(C)) against |x| ~ 0.5: 1e4 times the bar's reach at the largest shape.  'growth' keeps its own w: there
    x . w = 1 with every product positive, so the scale and the value double together."""
    g = _gen(c.id)
    B, C, L = c.B, c.C, c.L
    x, w, b = rnd(g, (B, C), 0.5), rnd(g, (L, C)), rnd(g, (L, C), 0.1)
    up = rnd(g, (B, C))
    xbar = rnd(g, (C,), 0.5)
    if c.data == 'bias_minus_x':                               # rows close to one row xbar, bias_0 = -xbar: x_1 = x_0 s + (x_0 - xbar)
        x = (xbar[None, :] * (1.0 + 1e-3 * torch.randn((B, C), generator=g, dtype=F64))).float().double()
        b[0] = -xbar
    elif c.data == 'growth':
        x = (xbar[None, :] + 0.05 * torch.randn((B, C), generator=g, dtype=F64)).float().double()
    elif c.data == 'logspace':                                 # columns scaled 1e-3 .. 1e3
        x = (x * torch.logspace(-3, 3, C, dtype=F64)[None, :]).float().double()
    elif c.data == 'zero_rows':
        x[::2] = 0.0
    elif c.data == 'zero_column':
        x[:, ZERO_COLUMN] = 0.0
    if L:
        w = (w * min(1.0 / np.sqrt(C), 1.0 / (0.8 * L * float(x.abs().sum(1).max())))).float().double()
    if c.data == 'perp':                                       # every row orthogonal to every w_l: s_0 ~ 0 against |x| . |w|
        q, _ = torch.linalg.qr(w.T)                            # [C, L]
        x = (x - (x @ q) @ q.T).float().double()
    elif c.data == 'w_zero':
        w = torch.zeros_like(w)
    elif c.data == 'growth':                                   # x_l . w_l ~ 2^l: the row doubles with every layer
        w = (xbar / (xbar * xbar).sum())[None, :].expand(L, C).float().double().contiguous()
    assert c.data in CROSS_DATA, c.data
    return [x, w, b], up


def cross_layer(x, w, b):
    """x_{l+1} = x_0 (x_l . w_l) + x_l + b_l (cross.hip:5), in the dtype of its arguments; autograd-friendly (the scales)"""
    xl = x
    for l in range(w.shape[0]):
        xl = x * (xl * w[l]).sum(1, keepdim=True) + xl + b[l]
    return xl


def cross_reference(inputs, up, dt, perm=None):
    """[y, grad_x, grad_w, grad_b] in `dt` from the header of csrc/cross.hip: t_l = g_{l+1} . x_0; g_l = g_{l+1} + w_l t_l;
    grad_w_l = sum_b x_l t_l; grad_b_l = sum_b g_{l+1}; grad_x = g_0 + sum_l g_{l+1} s_l.  perm: the batch walked in that order"""
    x, w, b = [t.to(dt) for t in inputs]
    g = up.to(dt)
    if perm is not None:
        x, g = x[perm], g[perm]
    L = w.shape[0]
    xs, s = [x], []
    for l in range(L):
        s.append((xs[l] * w[l]).sum(1, keepdim=True))
        xs.append(x * s[l] + xs[l] + b[l])
    gw, gb, acc = torch.zeros_like(w), torch.zeros_like(b), torch.zeros_like(x)
    for l in range(L - 1, -1, -1):
        t = (g * x).sum(1, keepdim=True)
        gw[l], gb[l] = (xs[l] * t).sum(0), g.sum(0)
        acc = acc + g * s[l]
        g = g + w[l] * t
    y, gx = xs[L], g + acc
    if perm is not None:
        inv = torch.argsort(perm)
        y, gx = y[inv], gx[inv]
    return [y, gx, gw, gb]


CrossRef = collections.namedtuple('CrossRef', 'inputs up r64 r32 scales')
_CROSS = {}


def cross_refs(c):
    """the references of one cross case, computed once and shared.  Scales: precision.abs_scale on the whole layer, as
    test_cross_is_fp32_class does; build_cross says how the inputs keep that composition from outgrowing the values."""
    if c.id not in _CROSS:
        inputs, up = build_cross(c)
        s_out, s_in = P.abs_scale(cross_layer, inputs, up)
        s_in = [torch.zeros_like(t) if s is None else s for s, t in zip(s_in, inputs)]          # (L = 0: no w, no bias)
        _CROSS[c.id] = CrossRef(inputs, up, cross_reference(inputs, up, F64), cross_reference(inputs, up, F32), [s_out] + s_in)
    return _CROSS[c.id]


def cross_figs(got, ref, names=CROSS_FIGURES):
    d = {'y': 'fwd', 'dx': 'bwd', 'dw': 'bwd', 'db': 'bwd'}
    return {n: (d[n], a, e, e32, s) for n, a, e, e32, s in zip(CROSS_FIGURES, got, ref.r64, ref.r32, ref.scales)
            if n in names and a is not None}


def run_cross_gpu(ref, dev):
    """[y, grad_x, grad_w, grad_b] of ops.cross on float32 copies of the reference's inputs"""
    from deeptables_amd import ops
    xs = [t.float().to(dev).requires_grad_(True) for t in ref.inputs]
    y = ops.cross(*xs)
    y.backward(ref.up.float().to(dev))
    return [y.detach()] + [t.grad for t in xs]


def params_of(cases):
    import pytest
    return [pytest.param(c, id=c.id) for c in cases]


def kind_params(cases):
    import pytest
    return [pytest.param(c, k, id=f'{k}-{c.id}') for c in cases for k in KINDS]


for _cases in (ROW_CASES + POINTER_CASES, CROSS_CASES + CROSS_CONTRACT_CASES):
    assert len({c.id for c in _cases}) == len(_cases)
