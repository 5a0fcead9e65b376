# -*- coding:utf-8 -*-
"""GPU: the kernels of csrc/embedding.hip (gather, fused embedding + concat + field sum + FM rows, dense scatter, owner-side
gather, feed gather) and csrc/cross.hip (the cross net) against plain float64 references of the same operations on the same
float32-rounded inputs, at every branch of their launchers, at their shape limits, on hard inputs and on their buffer contracts.

Paths (tests/rows_support.py holds the tables and the restated launch arithmetic; tests/test_rows_paths_host.py proves each id
against it): k_row_fwd / k_row_bwd at every LPR = 1 .. 64 with one partly filled trip, exactly 64 float4, a ragged second trip
and three trips or more, both id kinds, B = 1 | 3 | 5, Nd = 0 | 1 | 13 | 70; the generic row kernels at D = 1 .. 512, F = 70, at
the 64 KiB row buffer and refused one field past it; k_gather_vec4, k_scatter_add_rows, k_gather_owned and k_feed_gather one loop
step past their grid caps; the feed's two-level tickets with fewer than 32 blocks, an uneven group and 16,384 blocks; all ten
PER of k_cross_fwd, k_cross_bwd_reg<P, 4 | 8> and k_cross_bwd<P> for every P, 1 .. 512 partials in k_cross_bwd_reduce, the
grid-stride loops of both directions, L = 0, both LDS limits and the forward-only shape between them.

Bars (tests/precision.py; no number of it changed).  Bit-exact: emb, concat, rows, oob_count, gather_owned, feed_gather, the
scatter without duplicates.  Everything else per element: |e| / (sum of the magnitudes of the element's terms, float64), then
the max (precision.elem_cond), held to err_gpu <= STEP_BAR['fp32'] = 12 x max(err of the float32 CPU reference, 2^-24).
Scales: field_sum sum_d |x|; FM 0.5 sum_d ((sum_f |x|)^2 + sum_f x^2) (F = 1: true value 0, scale not); the row gradient
|g_emb| + |g_concat| + |g_fsum| + |g_fm| (sum_f |x| + |x|); the table gradient the scatter of that; cross precision.abs_scale on
the whole layer.  That scale is the L-layer composition on |x|, |w|, |b| and grows by 1 + sum_c |x| |w| per layer, so the cross
inputs draw w small enough that it stays within 8 x (|x_0| + sum_l |b_l|) at every depth (rows_support.build_cross), and the
hard inputs run at L = 2 (reg4, P = 16 generic) as well as at L = 8 | 9.  tests/test_rows_paths_host.py holds that bound and
puts wrong float32 arithmetic through this module's check on every cross case with a layer: a skipped layer, grad_x without its
sum_l g_{l+1} s_l, a zeroed grad_w row, a copied y column and s_l / t_l from bf16-rounded operands are each at least 40 x over
the bar on every case (smallest: the zeroed grad_w row on B9-C530-L2-hard_bias_minus_x, 506 against 12).

Contracts, through the C entry points on pre-filled buffers: each forward output NULL with the others present; each incoming
gradient alone, all four, none (grad_rows all zero from NaN), concat_stride = F D + Nd and = F D; a refused shape writes
nothing; dt_embedding_bwd_dense adds into grad_table; dt_cross_bwd overwrites grad_x (NaN beforehand), adds to grad_w / grad_b,
takes either as NULL and stays inside dt_cross_workspace_bytes; dt_cross_fwd with save_s NULL gives the same out.

Repeats: out, grad_x and the register kernels' grad_w / grad_b of the cross net take no float atomics and repeat bit for bit
(test_cross_repeats); the generic kernel's grad_w / grad_b (LDS atomics) and the scatter (global atomics) are held to the bar only.

MI355X, the largest figure over the cases of each test (one DT_PRECISION_LOG run), err_gpu / max(err_f32, 2^-24) in elem_cond,
bar 12.  Largest of all: grad_table 1.81 (scatter, 200 lookups on 7 rows, zero table), grad_rows 1.62 (dt_fm_bwd, B1-F16-D16),
db 1.62 (B5-C7-L2), field_sum 1.61 (B2-F32-D512, the 64 KiB generic row), dx 1.58 (hard growth, L = 8), y 1.33 (B5-C257-L4),
fm 1.26 (hard offset, D = 6).  No figure is within 2x of the bar (nearest: 6.6x below), no test went red on the unchanged
kernels and no kernel was changed.
  test                       fsum   fm     grad_rows  grad_table
  rows (fused, 74 runs)      1.61   0.72              1.38
  rows (dt_fm_fwd / _bwd)           0.72   1.62
  hard:logspace              0.94   0.52   1.19       1.06
  hard:offset                0.94   1.26   1.00       1.00
  hard:zero_rows             0.49   0.31   1.00       1.00
  hard:zero_field            0.59   0.19   1.00       1.00
  hard:all_oob               0.00   0.00   0.00       0.00
  hard:F1 (mild | offset)    0.15   0.13   0.00       0.80
  ids                        0.94   0.48   1.36       1.03
  pointers: forward          1.43   0.38
  pointers: backward                       1.00
  scatter (+ gather's)                                1.81
  test                       y      dx     dw     db
  cross paths                1.33   1.21   1.00   1.62
  hard:perp                  1.00   1.00   0.25   1.26
  hard:w_zero                1.00   0.00   0.35   1.00
  hard:bias_minus_x          1.00   0.86   0.11   1.00
  hard:growth                1.31   1.58   0.43   1.49
  hard:logspace              1.00   1.19   0.57   1.16
  hard:zero_rows             1.00   0.98   0.24   0.97
  hard:zero_column           1.08   1.00   0.24   1.08
  forward only (2048, 5)     1.00
  contracts                  1.00   1.29   0.46   1.23
  repeats                    1.02   1.00   0.16   1.06
Mutants, each built once in a scratch copy as a library of its own and run once on the MI355X (tests of this module red / of
the 179 tests of test_kernels_gpu.py, test_precision_gpu.py and test_edge_cases_gpu.py red):
  1 oob_count incremented without the c == 0 guard in k_row_fwd                      18 / 0   (ids at LPR 8 | 64, all-oob, pointers)
  2 group_sum<32> without its __shfl_xor 16 step                                      8 / 0   (the four LPR = 32 cases, both kinds)
  3 k_scatter_add_rows: row >= 0 -> row > 0                                          75 / 16
  4 k_gather_vec4 without its grid-stride step                                        2 / 0   (B = 2,049, F = 8, D = 256)
  5 members of k_feed_gather = gridDim.x / G                                          1 / 0   (uneven groups, 95 blocks)
  6 k_cross_bwd_reduce without its tail                                              73 / 10  (every partial count but 512)
  7 k_cross_bwd_reg<P, 4> chosen for L <= 5                                           6 / 0   (the five L = 5 cases, one repeated)
  8 k_row_bwd_generic without the g_fm term's - emb                                  36 / 3
Mutant 5 is the one path covered by timing only: a ticket group that fires one arrival early still leaves its tickets at zero
and the position right whenever the blocks' arrivals fall inside one store's latency.
test_feed_tickets_with_uneven_groups_over_many_launches spreads them (wide rows, 24 launches on one cursor) and caught it at 95
blocks (groups of 3 | 2 members), not at 35 or 63.  It can miss that mutant; it cannot fail on the right arithmetic.
"""
import ctypes

import pytest
import torch

from tests import precision as P
from tests import rows_support as S

pytestmark = pytest.mark.gpu

F64, F32, I32, I64 = torch.float64, torch.float32, torch.int32, torch.int64
DT_OK, DT_ERR_INVALID_ARG, DT_ERR_UNSUPPORTED = 0, -1, -2
NAN = float('nan')


def _kind_code(kind):
    from deeptables_amd import _lib
    return _lib.DT_IDX_I32 if kind == 'i32' else _lib.DT_IDX_F32


def _last_error():
    from deeptables_amd._lib import lib
    return lib().dt_last_error().decode()


def _filled(shape, value, dev, dtype=F32):
    return torch.full(tuple(shape), value, dtype=dtype, device=dev)


# ---- the fused row kernels through ops ---------------------------------------------------------------------------------------
def _run_rows(test, c, kind, dev):
    """ops.embed_fm_linear forward + backward (dense table gradient: the scatter) and ops.fm forward + backward on the same rows"""
    from deeptables_amd import ops
    r, r64, r32, sc = S.rows_refs(c, kind)
    B, F, D, Nd = c.B, c.F, c.D, c.Nd
    table = r.table.float().to(dev).requires_grad_(True)
    dense = None if r.dense is None else r.dense.float().to(dev).requires_grad_(True)
    oob = torch.zeros(1, dtype=I32, device=dev)
    emb, concat, fsum, fm, rows = ops.embed_fm_linear(r.idx.to(dev), table, r.row_offset.to(dev), r.vocab.to(dev), dense,
                                                      dense_grad=True, oob=oob)
    assert torch.equal(emb.detach().cpu(), r64.emb.float()), 'emb'
    assert torch.equal(concat.detach().cpu(), r64.concat.float()), 'concat'
    assert torch.equal(rows.cpu(), r.rows), 'rows'
    assert int(oob.item()) == int((~r.ok).sum()), ('oob_count', int(oob.item()), int((~r.ok).sum()))
    ue, uc, us, um = [u.float().to(dev) for u in r.ups]
    ((emb * ue).sum() + (concat * uc).sum() + (fsum * us).sum() + (fm.reshape(-1) * um).sum()).backward()
    S.check(f'{test}[{kind}][{c.id}]', 'embed_fm_linear',
            S.row_figs({'fsum': fsum.detach(), 'fm': fm.detach().reshape(-1), 'grad_table': table.grad}, r64, r32, sc))
    if Nd:
        assert torch.equal(dense.grad, uc[:, F * D:]), 'the dense part of the concat gradient'
    if kind == 'i32':                                       # dt_fm_fwd / dt_fm_bwd do not see the ids: once per case
        only = (False, False, False, True)
        f64, f32, fsc = S.rows_reference(r, F64, which=only), S.rows_reference(r, F32, which=only), S.rows_scales(r, only)
        x = r64.emb.float().to(dev).requires_grad_(True)
        out = ops.fm(x)
        assert out.shape == (B, 1)
        out.backward(um.view(B, 1))
        S.check(f'{test}:fm[{c.id}]', 'fm', S.row_figs({'fm': out.detach().reshape(-1), 'grad_rows': x.grad}, f64, f32, fsc))
    return r, fsum.detach(), fm.detach().reshape(-1), table.grad


@pytest.mark.parametrize('c,kind', S.kind_params(S.FAST_CASES + S.GENERIC_CASES))
def test_row_paths(dev, c, kind):
    _run_rows('rows', c, kind, dev)


@pytest.mark.parametrize('c,kind', S.kind_params(S.HARD_ROW_CASES))
def test_row_hard_inputs(dev, c, kind):
    r, fsum, fm, gtable = _run_rows(f'rows_hard:{c.data}', c, kind, dev)
    if c.data == 'all_oob':                                  # nothing gathered, nothing scattered
        assert not bool(fsum.any()) and not bool(fm.any()) and not bool(gtable.any())
    if c.data == 'zero_field':
        assert not bool(fsum[:, S.ZERO_FIELD].any())


@pytest.mark.parametrize('c,kind', S.kind_params(S.ID_CASES))
def test_out_of_range_ids(dev, c, kind):
    """-1, vocab, INT_MAX, INT_MIN | float(vocab), 2^24, 3e9, +-inf are out of range; vocab - 1 | -0.0, 0.9, vocab - 0.1 are not:
    oob_count is the number of out-of-range LOOKUPS (not lanes), their rows read zero in emb and concat (bit-exact in _run_rows),
    add nothing to field_sum and fm, get rows_out = -1 and are skipped by the scatter"""
    r, fsum, fm, gtable = _run_rows('rows_ids', c, kind, dev)
    assert 0 < int((~r.ok).sum()) < r.ok.numel()
    assert not bool(fsum.cpu()[~r.ok].any())
    never = torch.ones(r.table.shape[0], dtype=torch.bool)
    never[r.rows[r.ok]] = False
    assert not bool(gtable.cpu()[never].any())


# ---- the C entry points of the row kernels -----------------------------------------------------------------------------------
FWD_OUTS = ('emb_out', 'concat_out', 'field_sum', 'fm_out', 'rows_out', 'oob_count')


def _raw_row_fwd(c, kind, r, dev, absent=()):
    """dt_embed_fm_linear_fwd on buffers pre-filled with NaN / -7 -> (rc, {name: tensor | None})"""
    from deeptables_amd._lib import lib, ptr, stream_ptr
    B, F, D = c.B, c.F, c.D
    outs = {'emb_out': _filled((c.B, F, D), NAN, dev), 'concat_out': _filled((c.B, F * D + c.Nd), NAN, dev),
            'field_sum': _filled((c.B, F), NAN, dev), 'fm_out': _filled((c.B,), NAN, dev),
            'rows_out': _filled((c.B, F), -7, dev, I64), 'oob_count': torch.zeros(1, dtype=I32, device=dev)}
    for name in absent:
        outs[name] = None
    keep = [r.idx.to(dev), r.table.float().to(dev), r.row_offset.to(dev), r.vocab.to(dev),
            None if r.dense is None else r.dense.float().to(dev)]
    rc = lib().dt_embed_fm_linear_fwd(ptr(keep[0]), _kind_code(kind), ptr(keep[1]), ptr(keep[2]), ptr(keep[3]), ptr(keep[4]), B, F, D,
                                      c.Nd, *[ptr(outs[n]) for n in FWD_OUTS], stream_ptr())
    torch.cuda.synchronize()
    return rc, outs


def _check_row_fwd(test, c, kind, outs):
    r, r64, r32, sc = S.rows_refs(c, kind)
    exact = {'emb_out': r64.emb.float(), 'concat_out': r64.concat.float(), 'rows_out': r.rows}
    for name, want in exact.items():
        if outs[name] is not None:
            assert torch.equal(outs[name].cpu(), want), name
    if outs['oob_count'] is not None:
        assert int(outs['oob_count'].item()) == int((~r.ok).sum())
    S.check(test, 'embed_fm_linear', S.row_figs({'fsum': outs['field_sum'], 'fm': outs['fm_out']}, r64, r32, sc))


@pytest.mark.parametrize('absent', FWD_OUTS + ('nothing',))
@pytest.mark.parametrize('c,kind', S.kind_params(S.POINTER_CASES))
def test_forward_outputs_are_optional(dev, c, kind, absent):
    r = S.rows_refs(c, kind)[0]
    rc, outs = _raw_row_fwd(c, kind, r, dev, absent=() if absent == 'nothing' else (absent,))
    assert rc == DT_OK, _last_error()
    _check_row_fwd(f'pointers:fwd:{absent}[{kind}][{c.id}]', c, kind, outs)


GRADS = ('g_emb', 'g_concat', 'g_field_sum', 'g_fm')
BWD_COMBOS = [(True, False, False, False), (False, True, False, False), (False, False, True, False), (False, False, False, True),
              (True, True, True, True), (False, False, False, False)]


def _raw_row_bwd(c, r, emb, which, dev, tight_concat=False):
    """dt_embed_fm_linear_bwd with the gradients of `which` present -> (rc, grad_rows pre-filled with NaN)"""
    from deeptables_amd._lib import lib, ptr, stream_ptr
    F, D = c.F, c.D
    ups = [u.float().to(dev) if w else None for u, w in zip(r.ups, which)]
    stride = F * D + c.Nd
    if tight_concat and ups[1] is not None:
        ups[1], stride = ups[1][:, :F * D].contiguous(), F * D
    embd = emb.float().to(dev)
    grad_rows = _filled((c.B, F, D), NAN, dev)
    rc = lib().dt_embed_fm_linear_bwd(ptr(embd), ptr(ups[0]), ptr(ups[1]), stride, ptr(ups[2]), ptr(ups[3]), c.B, F, D,
                                      ptr(grad_rows), stream_ptr())
    torch.cuda.synchronize()
    return rc, grad_rows


@pytest.mark.parametrize('which', BWD_COMBOS, ids=lambda w: '+'.join(n for n, k in zip(GRADS, w) if k) or 'none')
@pytest.mark.parametrize('c', S.params_of(S.POINTER_CASES))
def test_incoming_gradients_are_optional(dev, c, which):
    """each of the four incoming gradients alone, all four and none (grad_rows all zero from a NaN pre-fill); g_concat with
    concat_stride = F D + Nd, and once more packed to concat_stride = F D"""
    r, r64, _, _ = S.rows_refs(c, 'i32')
    f64, f32, sc = S.rows_reference(r, F64, which=which), S.rows_reference(r, F32, which=which), S.rows_scales(r, which)
    for tight in ((False, True) if which[1] else (False,)):
        rc, grad_rows = _raw_row_bwd(c, r, r64.emb, which, dev, tight_concat=tight)
        assert rc == DT_OK, _last_error()
        if not any(which):
            assert not bool(grad_rows.any())
        S.check(f'pointers:bwd:{"+".join(n for n, k in zip(GRADS, which) if k) or "none"}[{c.id}]', 'embed_fm_linear',
                S.row_figs({'grad_rows': grad_rows}, f64, f32, sc))


def test_backward_refuses_a_concat_stride_below_the_row_and_fm_without_emb(dev):
    from deeptables_amd._lib import lib, ptr, stream_ptr
    c = S.POINTER_CASES[0]
    r, r64, _, _ = S.rows_refs(c, 'i32')
    g = r.ups[1].float().to(dev)
    out = _filled((c.B, c.F, c.D), -7.0, dev)
    assert lib().dt_embed_fm_linear_bwd(None, None, ptr(g), c.F * c.D - 1, None, None, c.B, c.F, c.D, ptr(out), stream_ptr()) == DT_ERR_INVALID_ARG
    gf = r.ups[3].float().to(dev)
    assert lib().dt_embed_fm_linear_bwd(None, None, None, 0, None, ptr(gf), c.B, c.F, c.D, ptr(out), stream_ptr()) == DT_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())


@pytest.mark.parametrize('kind', S.KINDS)
def test_generic_row_buffer_limit(dev, kind):
    """F D = 16,384 floats fills the 64 KiB row buffer and runs (a case of test_row_paths); one field more is refused by name and
    writes nothing"""
    F, D = S.ROW_REFUSED
    assert S.row_fwd_refused(F, D) and not S.row_fwd_refused(F - 1, D)
    c = S.row_case('refused', 2, F, D)
    r = S.build_rows(c, kind)
    rc, outs = _raw_row_fwd(c, kind, r, dev)
    assert rc == DT_ERR_UNSUPPORTED and f'F*D={F * D}' in _last_error(), _last_error()
    assert all(bool(torch.isnan(outs[n]).all()) for n in ('emb_out', 'concat_out', 'field_sum', 'fm_out'))
    assert bool((outs['rows_out'] == -7).all()) and int(outs['oob_count'].item()) == 0


# ---- dt_embedding_fwd --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', S.KINDS)
@pytest.mark.parametrize('B,F,D', S.GATHER_CASES)
def test_embedding_gather(dev, B, F, D, kind):
    """k_gather_vec4 for D % 4 == 0 (also D = 12, 260: no power of two), the generic row kernel otherwise; B = 2,049, F = 8,
    D = 256 is one step of the grid-stride loop past the 4,096-block cap; small cases also scatter their gradient"""
    from deeptables_amd import ops
    lk = S.build_lookup('gather', (B,), F, D, kind, oob_every=5)
    small = B * F * D <= 2 ** 16
    table = lk.table.float().to(dev).requires_grad_(small)
    oob = torch.zeros(1, dtype=I32, device=dev)
    emb, rows = ops.embedding_lookup(lk.idx.to(dev), table, lk.row_offset.to(dev), lk.vocab.to(dev), dense_grad=True, oob=oob)
    want = lk.table.float()[lk.rows.clamp(min=0)] * lk.ok[:, :, None]
    assert torch.equal(emb.detach().cpu(), want) and torch.equal(rows.cpu(), lk.rows)
    assert int(oob.item()) == int((~lk.ok).sum()) > 0
    if small:
        up = S.rnd(torch.Generator().manual_seed(B + F + D), (B, F, D))
        emb.backward(up.float().to(dev))
        R = lk.table.shape[0]
        S.check(f'gather:scatter[{B},{F},{D},{kind}]', 'embed_fm_linear',
                {'grad_table': ('bwd', table.grad, S.scatter(lk.rows, up, R, F64), S.scatter(lk.rows, up, R, F32),
                                S.scatter(lk.rows, up.abs(), R, F64))})


@pytest.mark.parametrize('B,F', [(0, 3), (3, 0)])
def test_empty_gather_touches_nothing(dev, B, F):
    from deeptables_amd._lib import lib, ptr, stream_ptr
    lk = S.build_lookup('gather', (3,), 3, 4, 'i32')
    bufs = [lk.idx.to(dev), lk.table.float().to(dev), lk.row_offset.to(dev), lk.vocab.to(dev)]
    out, rows, oob = _filled((3, 3, 4), -7.0, dev), _filled((3, 3), -7, dev, I64), torch.zeros(1, dtype=I32, device=dev)
    assert lib().dt_embedding_fwd(ptr(bufs[0]), _kind_code('i32'), ptr(bufs[1]), ptr(bufs[2]), ptr(bufs[3]), B, F, 4, ptr(out), ptr(rows),
                                  ptr(oob), stream_ptr()) == DT_OK
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((rows == -7).all()) and int(oob.item()) == 0


# ---- dt_embedding_bwd_dense --------------------------------------------------------------------------------------------------
def _scatter_case(tag):
    g = torch.Generator().manual_seed(len(tag))
    if tag == 'no_duplicates':                              # 37 distinct rows of 50, D = 5
        n, D, R = 37, 5, 50
        rows = torch.randperm(R, generator=g)[:n]
    elif tag == 'one_row_4096_times':
        n, D, R = 4096, 8, 5
        rows = torch.full((n,), 3, dtype=I64)
    elif tag == 'collisions_with_dead_rows_and_row_0':      # rows -1 .. 6: heavy collisions, -1 among live rows, row 0 live
        n, D, R = 200, 6, 7
        rows = torch.randint(-1, R, (n,), generator=g)
        rows[:3] = torch.tensor([0, -1, 0])
    else:
        assert tag == 'grid_stride_wrap'
        n, D, R = S.SCATTER_WRAP
        rows = torch.randint(-1, R, (n,), generator=g)
    return rows.to(I64), S.rnd(g, (n, D)), S.rnd(g, (R, D))


@pytest.mark.parametrize('prefill', [False, True], ids=['zero_table', 'prefilled_table'])
@pytest.mark.parametrize('tag', ['no_duplicates', 'one_row_4096_times', 'collisions_with_dead_rows_and_row_0', 'grid_stride_wrap'])
def test_dense_scatter(dev, tag, prefill):
    """grad_table[row] += g for row >= 0: it ADDS (a pre-filled table comes back as pre-fill + sum), skips -1, serves row 0"""
    from deeptables_amd._lib import lib, ptr, stream_ptr
    rows, g, base = _scatter_case(tag)
    if not prefill:
        base = torch.zeros_like(base)
    R, D = base.shape
    table = base.float().to(dev)
    rd, gd = rows.to(dev), g.float().to(dev)
    assert lib().dt_embedding_bwd_dense(ptr(rd), ptr(gd), rows.numel(), D, ptr(table), stream_ptr()) == DT_OK, _last_error()
    torch.cuda.synchronize()
    r64, r32 = S.scatter(rows, g, R, F64, base), S.scatter(rows, g, R, F32, base)
    scale = S.scatter(rows, g.abs(), R, F64, base.abs())
    if tag == 'no_duplicates' and not prefill:
        assert torch.equal(table.cpu(), r64.float())         # 0 + g: the upstream gradient bit for bit
    S.check(f'scatter:{tag}:{"prefilled" if prefill else "zero"}', 'embed_fm_linear', {'grad_table': ('bwd', table, r64, r32, scale)})
    untouched = torch.ones(R, dtype=torch.bool)
    untouched[rows[rows >= 0]] = False
    assert torch.equal(table.cpu()[untouched], base.float()[untouched])


# ---- dt_embedding_gather_owned -----------------------------------------------------------------------------------------------
GUARD = 64


def _raw_owned(lk, kind, W, B, F, f0, f1, D, dev):
    from deeptables_amd._lib import lib, ptr, stream_ptr
    Fo = f1 - f0
    n = W * Fo * B
    out, rows = _filled((n * D + GUARD,), NAN, dev), _filled((n + GUARD,), -7, dev, I64)
    oob = torch.zeros(1, dtype=I32, device=dev)
    keep = [lk.idx.to(dev), lk.table.float().to(dev), lk.row_offset.to(dev), lk.vocab.to(dev)]
    rc = lib().dt_embedding_gather_owned(ptr(keep[0]), _kind_code(kind), ptr(keep[1]), ptr(keep[2]), ptr(keep[3]), W, B, F, f0, f1, D,
                                         ptr(out), ptr(rows), ptr(oob), stream_ptr())
    torch.cuda.synchronize()
    return rc, out, rows, oob, n


@pytest.mark.parametrize('kind', S.KINDS)
@pytest.mark.parametrize('W,B,F,f0,f1,D', S.OWNED_CASES)
def test_gather_owned(dev, W, B, F, f0, f1, D, kind):
    """ids [W, B, F] of the fields [f0, f1) -> rows in [W, F_own, B, D] order and their packed row ids in [W, F_own, B] order;
    out-of-range ids counted once per lookup of the owned fields; an empty range touches nothing; the last case is one loop step
    past the 8,192-block cap"""
    lk = S.build_lookup('owned', (W, B), F, D, kind, oob_every=5)
    rc, out, rows, oob, n = _raw_owned(lk, kind, W, B, F, f0, f1, D, dev)
    assert rc == DT_OK, _last_error()
    own_rows, own_ok = lk.rows[:, :, f0:f1].permute(0, 2, 1), lk.ok[:, :, f0:f1].permute(0, 2, 1)          # [W, Fo, B]
    want = lk.table.float()[own_rows.clamp(min=0)] * own_ok[..., None]
    assert torch.equal(out[:n * D].cpu(), want.reshape(-1)) and torch.equal(rows[:n].cpu(), own_rows.reshape(-1))
    assert bool(torch.isnan(out[n * D:]).all()) and bool((rows[n:] == -7).all())
    assert int(oob.item()) == int((~own_ok).sum())
    if f1 > f0:
        assert int(oob.item()) > 0


def test_gather_owned_refuses_a_row_that_is_no_multiple_of_four(dev):
    lk = S.build_lookup('owned', (1, 5), 6, 6, 'i32')
    rc, out, rows, oob, n = _raw_owned(lk, 'i32', 1, 5, 6, 0, 2, 6, dev)
    assert rc == DT_ERR_INVALID_ARG and 'D=6' in _last_error()
    assert bool(torch.isnan(out).all()) and bool((rows == -7).all()) and int(oob.item()) == 0


# ---- dt_feed_gather ----------------------------------------------------------------------------------------------------------
N_SRC = 50


def _feed_blocks(row_bytes, n_rows, dev, seed):
    g = torch.Generator().manual_seed(seed)
    src = [torch.randint(-2 ** 31, 2 ** 31 - 1, (N_SRC, rb // 4), generator=g, dtype=I64).to(I32).to(dev) for rb in row_bytes]
    dst = [_filled((n_rows * (rb // 4) + GUARD,), -7, dev, I32) for rb in row_bytes]
    return src, dst


def _raw_feed(sel, n_rows, src, dst, row_bytes, cursor):
    from deeptables_amd._lib import lib, ptr, stream_ptr
    nb = len(src)
    arr = ctypes.c_void_p * nb
    a, b, rb = arr(*[t.data_ptr() for t in src]), arr(*[t.data_ptr() for t in dst]), (ctypes.c_int * nb)(*row_bytes)
    rc = lib().dt_feed_gather(ptr(sel), n_rows, nb, ctypes.cast(a, ctypes.c_void_p), ctypes.cast(b, ctypes.c_void_p),
                              ctypes.cast(rb, ctypes.c_void_p), ptr(cursor), stream_ptr())
    torch.cuda.synchronize()
    return rc


def _check_feed(sel_window, src, dst, row_bytes):
    n = sel_window.numel()
    for s, d, rb in zip(src, dst, row_bytes):
        w = rb // 4
        assert torch.equal(d[:n * w].reshape(n, w), s[sel_window]), f'block of {rb}-byte rows'
        assert bool((d[n * w:] == -7).all()), 'wrote past the destination'


@pytest.mark.parametrize('n_rows,row_bytes', S.FEED_CASES, ids=lambda v: str(v).replace(' ', ''))
def test_feed_gather(dev, n_rows, row_bytes):
    """dst[b][i, :] = src[b][sel[i], :] bit for bit, no cursor: 1, 3 and 8 blocks, rows of 4 .. 1,028 bytes (wider than the 64
    lanes of a wave, alone and summed over the blocks), a last partial group of 8 rows, one launch past the 16,384-block cap"""
    src, dst = _feed_blocks(row_bytes, n_rows, dev, n_rows + len(row_bytes))
    sel = torch.randint(0, N_SRC, (n_rows,), generator=torch.Generator().manual_seed(n_rows), dtype=I64).to(dev)
    assert _raw_feed(sel, n_rows, src, dst, list(row_bytes), None) == DT_OK, _last_error()
    _check_feed(sel, src, dst, row_bytes)


def test_feed_cursor_walks_the_selection(dev):
    """one cursor through four launches (2 blocks: G = gridDim; 35 blocks: groups of 2 and of 1 members; 1 block; 16,384 blocks):
    after each the position is the sum of n_rows, every ticket word is zero again and the rows came from the advanced position"""
    from deeptables_amd import _lib
    assert _lib.DT_FEED_CURSOR_WORDS == S.FEED_CURSOR_WORDS
    row_bytes = [4, 12]
    total = sum(S.FEED_CURSOR_LAUNCHES)
    sel = torch.randint(0, N_SRC, (total,), generator=torch.Generator().manual_seed(5), dtype=I64).to(dev)
    cursor = torch.zeros(S.FEED_CURSOR_WORDS, dtype=I64, device=dev)
    pos = 0
    for n_rows in S.FEED_CURSOR_LAUNCHES:
        src, dst = _feed_blocks(row_bytes, n_rows, dev, n_rows)
        assert _raw_feed(sel, n_rows, src, dst, row_bytes, cursor) == DT_OK, _last_error()
        _check_feed(sel[pos:pos + n_rows], src, dst, row_bytes)
        pos += n_rows
        assert int(cursor[0].item()) == pos and not bool(cursor[1:].any()), (n_rows, int(cursor[0].item()))


@pytest.mark.parametrize('blocks', S.FEED_UNEVEN_GRIDS)
def test_feed_tickets_with_uneven_groups_over_many_launches(dev, blocks):
    """a grid that is no multiple of 32: some ticket groups have one member more than the others.  A group that fires one arrival
    early leaves a ticket behind, or moves the position under a block that has not read it, only when the arrivals fall far enough
    apart in time: wide rows (1,340 bytes over 8 blocks) spread them, and the same cursor goes through 24 launches, each checked
    for its position, its zeroed tickets and every row."""
    row_bytes = [4, 8, 12, 16, 4, 260, 8, 1028]
    n_rows, launches = blocks * S.FEED_ROWS_PER_BLOCK - 5, 24
    assert S.feed_grid(n_rows) == blocks and len({S.feed_members(blocks, g) for g in range(S.feed_G(blocks))}) == 2
    sel = torch.randint(0, N_SRC, (n_rows * (launches + 40),), generator=torch.Generator().manual_seed(blocks), dtype=I64).to(dev)
    cursor = torch.zeros(S.FEED_CURSOR_WORDS, dtype=I64, device=dev)
    src, dst = _feed_blocks(row_bytes, n_rows, dev, blocks)
    for k in range(launches):
        assert _raw_feed(sel, n_rows, src, dst, row_bytes, cursor) == DT_OK, _last_error()
        assert int(cursor[0].item()) == (k + 1) * n_rows and not bool(cursor[1:].any()), (k, cursor[:2].tolist())
        _check_feed(sel[k * n_rows:(k + 1) * n_rows], src, dst, row_bytes)


def test_feed_gather_refuses_a_row_size_that_is_no_multiple_of_four(dev):
    src, dst = _feed_blocks([4, 8], 9, dev, 1)
    sel = torch.zeros(9, dtype=I64, device=dev)
    assert _raw_feed(sel, 9, src, dst, [4, 6], None) == DT_ERR_INVALID_ARG and 'multiple of 4' in _last_error()
    assert all(bool((d == -7).all()) for d in dst)


# ---- cross -------------------------------------------------------------------------------------------------------------------
def _run_cross(test, c, dev):
    ref = S.cross_refs(c)
    got = S.run_cross_gpu(ref, dev)
    S.check(f'{test}[{c.id}]', 'cross', S.cross_figs(got, ref))
    return got, ref


@pytest.mark.parametrize('c', S.params_of(S.CROSS_PATH_CASES))
def test_cross_paths(dev, c):
    got, ref = _run_cross('cross', c, dev)
    if c.L == 0:                                             # no layer: out == x and grad_x == grad_out bit for bit
        assert torch.equal(got[0].cpu(), ref.inputs[0].float()) and torch.equal(got[1].cpu(), ref.up.float())


@pytest.mark.parametrize('c', S.params_of(S.HARD_CROSS_CASES))
def test_cross_hard_inputs(dev, c):
    _run_cross(f'cross_hard:{c.data}', c, dev)


def _raw_cross_fwd(xs, B, C, L, out, save_s):
    from deeptables_amd._lib import lib, ptr, stream_ptr
    return lib().dt_cross_fwd(ptr(xs[0]), ptr(xs[1]), ptr(xs[2]), B, C, L, ptr(out), ptr(save_s), stream_ptr())


def _raw_cross_bwd(xs, save_s, gy, B, C, L, gx, gw, gb, ws):
    from deeptables_amd._lib import lib, ptr, stream_ptr
    return lib().dt_cross_bwd(ptr(xs[0]), ptr(xs[1]), ptr(xs[2]), ptr(save_s), ptr(gy), B, C, L, ptr(gx), ptr(gw), ptr(gb), ptr(ws),
                              stream_ptr())


def test_cross_column_limit(dev):
    """C = 2,048 runs (a case of test_cross_paths); C = 2,049 is refused in both directions and nothing is written"""
    from deeptables_amd._lib import lib
    B, C, L = 2, S.CROSS_REFUSED_C, 1
    xs = [torch.zeros((B, C), device=dev), torch.zeros((L, C), device=dev), torch.zeros((L, C), device=dev)]
    out, save_s = _filled((B, C), -7.0, dev), _filled((B, L), -7.0, dev)
    assert _raw_cross_fwd(xs, B, C, L, out, save_s) == DT_ERR_UNSUPPORTED and f'C={C} exceeds 2048' in _last_error()
    gx, gw, gb = _filled((B, C), -7.0, dev), _filled((L, C), -7.0, dev), _filled((L, C), -7.0, dev)
    ws = _filled((2 * L * C,), -7.0, dev)
    assert _raw_cross_bwd(xs, save_s, out, B, C, L, gx, gw, gb, ws) == DT_ERR_UNSUPPORTED and f'C={C} exceeds 2048' in _last_error()
    torch.cuda.synchronize()
    assert all(bool((t == -7.0).all()) for t in (out, save_s, gx, gw, gb, ws))
    assert lib().dt_cross_workspace_bytes(B, C, L) == S.cross_workspace_bytes(B, C, L)


def test_cross_forward_accepts_what_the_backward_refuses(dev):
    """C = 2,048, L = 5: the forward keeps no LDS and runs; the backward's accumulator is L C = 10,240 > 8,192 floats and it
    refuses by name, leaving no gradient.  The asymmetry is pinned as it is."""
    from deeptables_amd import ops
    from deeptables_amd._lib import DtHipError
    C, L = S.CROSS_FORWARD_ONLY
    c = S.cross_case('forward_only', 3, C, L)
    assert not S.cross_fwd_refused(C) and S.cross_bwd_refusal(C, L) == 'LDS'
    ref = S.cross_refs(c)
    xs = [t.float().to(dev).requires_grad_(True) for t in ref.inputs]
    y = ops.cross(*xs)
    S.check(f'cross:forward_only[{c.id}]', 'cross', S.cross_figs([y.detach(), None, None, None], ref))
    with pytest.raises(DtHipError, match=rf'L\*C={L * C} exceeds the 8192-float LDS accumulator'):
        y.backward(ref.up.float().to(dev))
    torch.cuda.synchronize()
    assert all(t.grad is None for t in xs)


@pytest.mark.parametrize('c', S.params_of(S.CROSS_CONTRACT_CASES))
def test_cross_contracts(dev, c):
    """through the C entry points: save_s may be NULL in the forward (same out); grad_x is overwritten (NaN beforehand); grad_w
    and grad_b are added to; each of the two may be NULL; the workspace is exactly dt_cross_workspace_bytes"""
    from deeptables_amd._lib import lib
    B, C, L = c.B, c.C, c.L
    ref = S.cross_refs(c)
    xs = [t.float().to(dev) for t in ref.inputs]
    gy = ref.up.float().to(dev)
    out, out2, save_s = _filled((B, C), NAN, dev), _filled((B, C), NAN, dev), _filled((B, L), NAN, dev)
    assert _raw_cross_fwd(xs, B, C, L, out, save_s) == DT_OK and _raw_cross_fwd(xs, B, C, L, out2, None) == DT_OK
    assert torch.equal(out, out2)
    nbytes = lib().dt_cross_workspace_bytes(B, C, L)
    assert nbytes == S.cross_workspace_bytes(B, C, L) and nbytes % 4 == 0
    g = torch.Generator().manual_seed(13)
    bw, bb = S.rnd(g, (L, C)), S.rnd(g, (L, C))
    shifted = ref._replace(r64=ref.r64[:2] + [ref.r64[2] + bw, ref.r64[3] + bb],
                           r32=ref.r32[:2] + [ref.r32[2] + bw.float(), ref.r32[3] + bb.float()],
                           scales=ref.scales[:2] + [ref.scales[2] + bw.abs(), ref.scales[3] + bb.abs()])
    for has_w, has_b in ((True, True), (False, True), (True, False)):
        gx = _filled((B, C), NAN, dev)
        gw, gb = (bw.float().to(dev) if has_w else None), (bb.float().to(dev) if has_b else None)
        ws = _filled((nbytes // 4 + GUARD,), NAN, dev)
        ws[nbytes // 4:] = -7.0
        assert _raw_cross_bwd(xs, save_s, gy, B, C, L, gx, gw, gb, ws) == DT_OK, _last_error()
        torch.cuda.synchronize()
        S.check(f'cross:contract:w{int(has_w)}b{int(has_b)}[{c.id}]', 'cross', S.cross_figs([out, gx, gw, gb], shifted))
        assert bool((ws[nbytes // 4:] == -7.0).all()) and not bool(torch.isnan(ws[:nbytes // 4]).any())


@pytest.mark.parametrize('shape', [(2053, 7, 2), (5, 193, 5), (2053, 7, 9), (5, 513, 2)], ids=lambda s: '-'.join(map(str, s)))
def test_cross_repeats(dev, shape):
    """out and grad_x take no atomics on any path, the register kernels' grad_w / grad_b none either: they repeat bit for bit.
    The generic kernel merges grad_w / grad_b with LDS float atomics: held to the bar only."""
    c = next(c for c in S.CROSS_PATH_CASES if (c.B, c.C, c.L) == shape)
    a, _ = _run_cross('cross:repeat', c, dev)
    b, _ = _run_cross('cross:repeat', c, dev)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    if S.cross_bwd_kernel(c.C, c.L) != 'generic':
        assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
