# -*- coding:utf-8 -*-
"""Host: the case table of tests/mha_support.py against the launch arithmetic it restates (an id can never drift from the path
it names), that every template instantiation and every launcher branch of csrc/mha.hip has a case, the restatement against
dt_mha_core_supported, dt_autoint_dropout_threshold and dt_autoint_dropout_hash, the two float64 forms of the reference against
each other and oracle/closed_form, and every GPU case's references against themselves before an input reaches a GPU."""
import itertools

import numpy as np
import pytest
import torch

from tests import mha_support as S
from tests import precision as P

F64 = torch.float64


# ---- the restatement at the figures the ids and the docstrings quote ------------------------------------------------------------
def test_restatement_at_the_quoted_figures():
    assert [S.dhmax(dh, 'fwd') for dh in (1, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65)] == [4, 4, 8, 8, 16, 16, 32, 32, 64, 64, None]
    assert [S.dhmax(dh, 'bwd') for dh in (1, 4, 5, 8, 9, 16, 17, 32, 33, 64)] == [4, 4, 8, 8, 16, 16, 32, 32, None, None]
    assert S.vec4('fwd', 16, 2, 16) and S.vec4('bwd', 16, 2, 64, 64) and not S.vec4('bwd', 16, 2, 16, 49)
    assert not S.vec4('fwd', 16, 2, 17) and not S.vec4('fwd', 12, 2, 12) and not S.vec4('fwd', 6, 1, 8)
    assert S.vec4('fwd', 16, 2, 16, offsets=(0, 4, 64)) and not S.vec4('fwd', 16, 2, 16, offsets=(0, 1))
    assert S.path('fwd', 64, 1, 64) == '64v' and S.path('bwd', 64, 1, 64, 192) is None and S.path('bwd', 17, 1, 17, 51) == '32s'
    assert [S.grid(B, F, H) for B, F, H in ((51, 5, 1), (32, 4, 2), (257, 1, 1), (43, 5, 3))] == [(1, 255), (1, 256), (2, 1), (3, 133)]
    assert [S.threshold(r) for r in (0.0, 0.5, 0.3, 1e-12, 0.9999999, 0.99999999)] == \
        [0, 2 ** 31, 1288490240, 1, 4294966784, 4294967295]
    assert int(0.3 * 2 ** 32) == 1288490188                                   # the Python double's: not the kernels'
    assert S.keep_scale(0.5) == 2.0 and S.keep_scale(0.3) == float(np.float32(1) / np.float32(0.7)) != 1.0 / 0.7
    assert S.strides(S.LAYOUT_CASES[0]) == (16, 16) and S.strides(S.LAYOUT_CASES[1]) == (5, 13)


# ---- the restatement against the library ----------------------------------------------------------------------------------------
THRESHOLD_RATES = (0.1, 0.2, 0.25, 0.3, 0.4, 0.5, 0.7, 0.9, 1e-12, 0.9999999)


@pytest.mark.parametrize('rate', THRESHOLD_RATES)
def test_dropout_threshold_equals_the_library(rate):
    """the kernels take the rate as a C float: the restatement, ops.autoint_dropout_threshold and the keep scale of
    ops.autoint_dropout_keep go through float32 as they do"""
    from deeptables_amd import _lib, ops
    want = int(_lib.lib().dt_autoint_dropout_threshold(rate))
    assert S.threshold(rate) == want and ops.autoint_dropout_threshold(rate) == want
    keep = ops.autoint_dropout_keep(5, 2, 2, 7, rate)
    mine = S.keep_mask(5, 2, 2, 7, rate)
    assert torch.equal(keep.double(), mine) and set(keep.unique().tolist()) <= {0.0, S.keep_scale(rate)}


def test_dropout_threshold_off_and_saturated():
    from deeptables_amd import _lib
    lib = _lib.lib()
    for rate in (0.0, -0.5, 1.0, 2.0, 0.99999999):
        assert int(lib.dt_autoint_dropout_threshold(rate)) == S.threshold(rate), rate
    assert S.threshold(-0.5) == 0 and S.threshold(1.0) == S.threshold(2.0) == 4294967295


def test_hash_restatement_equals_the_library():
    from deeptables_amd import _lib
    lib = _lib.lib()
    x = S.dropout_hash(991, 3, 4, 64)
    for b, h, i, j in ((0, 0, 0, 0), (2, 3, 63, 63), (1, 2, 5, 40), (2, 0, 63, 0), (0, 3, 0, 63)):
        assert int(x[b, h, i, j]) == int(lib.dt_autoint_dropout_hash(991, b, h, i, j))


def test_supported_restatement_equals_the_library():
    from deeptables_amd import _lib, ops
    lib = _lib.lib()
    Fs, Ds, Hs = (0, 1, 5, 64, 65, 70, 1000), (0, 1, 4, 6, 32, 33, 40, 64, 65, 66, 128, 130), (0, 1, 2, 3, 4)
    for F, D, H, drop in itertools.product(Fs, Ds, Hs, (0, 1)):
        assert bool(lib.dt_mha_core_supported(F, D, H, drop)) == S.supported(F, D, H, drop), (F, D, H, drop)
    for (F, D, H, rate), (fwd, bwd) in S.REFUSED.items():
        assert not S.supported(F, D, H, rate > 0) and not ops.mha_supported(F, D, H, rate)
        assert S.refusal('fwd', 2, F, D, H, D, None, rate) == fwd and S.refusal('bwd', 2, F, D, H, D, 3 * D, rate) == bwd
    assert ops.mha_supported(5, 4, 1) and ops.mha_supported(64, 32, 1, 0.5) and ops.mha_supported(70, 8, 2, 0.0)
    # supported == both directions launch, at every valid stride
    for F, D, H, rate in itertools.product((1, 64, 65), (4, 32, 33, 64, 65, 6), (1, 2, 4), (0.0, 0.3)):
        both = S.refusal('fwd', 1, F, D, H, D, None, rate) == S.DT_OK and S.refusal('bwd', 1, F, D, H, D, D, rate) == S.DT_OK
        assert both == S.supported(F, D, H, rate > 0), (F, D, H, rate)


def test_refusals_in_the_launchers_order():
    ok = dict(B=2, F=5, D=8, H=2, ld=8, ldg=24, rate=0.0)
    for change, fwd, bwd in (({}, 0, 0), ({'D': 9}, -1, -1), ({'ld': 7}, -1, -1), ({'ldg': 7}, 0, -1), ({'rate': 1.0}, -1, -1),
                             ({'rate': -0.25}, -1, -1), ({'rate': float('nan')}, -1, -1), ({'B': -1}, -1, -1), ({'F': 0}, -1, -1),
                             ({'H': 0}, -1, -1), ({'F': 65, 'rate': 0.5}, -2, -2), ({'F': 65}, 0, 0), ({'F': 64, 'rate': 0.5}, 0, 0),
                             ({'D': 66, 'H': 2, 'ld': 66, 'ldg': 66}, 0, -2), ({'D': 65, 'H': 1, 'ld': 65, 'ldg': 65}, -2, -2),
                             ({'D': 130, 'H': 2, 'ld': 3, 'ldg': 130}, -1, -1), ({'B': 0}, 0, 0), ({'B': 0, 'D': 65, 'H': 1, 'ld': 65, 'ldg': 65}, -2, -2)):
        a = dict(ok, **change)
        assert S.refusal('fwd', **a) == fwd and S.refusal('bwd', **a) == bwd, change


def test_refusals_equal_the_library():
    """every refusal comes before the empty-batch return and before a pointer is looked at: with B = 0 and null pointers the
    entry points themselves answer, without a GPU"""
    from deeptables_amd import _lib
    lib = _lib.lib()
    for F, (D, H), pad, rate in itertools.product((0, 1, 64, 65), ((8, 2), (9, 2), (33, 1), (64, 1), (65, 1), (130, 2), (0, 1), (4, 0)),
                                                  (-1, 0, 1), (0.0, 0.3, 1.0, -0.5, float('nan'))):
        ld, ldg = D + pad, 3 * D + pad if pad >= 0 else D - 1
        got_f = lib.dt_mha_core_fwd(None, None, None, 0, F, D, H, ld, rate, 1, None, None, None, None)
        got_b = lib.dt_mha_core_bwd(None, None, None, None, None, 0, F, D, H, ld, ldg, rate, 1, None, None, None, None, None)
        assert got_f == S.refusal('fwd', 0, F, D, H, ld, ldg, rate), (F, D, H, ld, rate, lib.dt_last_error())
        assert got_b == S.refusal('bwd', 0, F, D, H, ld, ldg, rate), (F, D, H, ld, ldg, rate, lib.dt_last_error())


# ---- case hygiene ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', S.params_of(S.CASES + [S.OFFSET_CASE]))
def test_case_takes_the_path_its_id_names(c):
    plan = S.plan(c)
    for k, want in c.expect.items():
        assert plan[k] == want, (c.id, k, plan[k], want)
    assert f"-fwd{plan['fwd']}-bwd{plan['bwd']}-" in c.id and f'-{c.layout}' in c.id
    ld, ldg = S.strides(c)
    assert S.refusal('fwd', c.B, c.F, c.D, c.H, ld, ldg, c.rate) == S.DT_OK
    assert (S.refusal('bwd', c.B, c.F, c.D, c.H, ld, ldg, c.rate) == S.DT_OK) == (plan['bwd'] is not None)
    assert c.B * c.H * c.F <= 2000 and c.F <= 70 and c.layout in S.LAYOUTS and c.data in S.DATA


def test_the_table_covers_every_instantiation_and_every_launcher_branch():
    plans = [(c, S.plan(c)) for c in S.CASES]
    every = {f'{b}{p}' for b in S.BRACKETS for p in 'vs'}
    assert {p['fwd'] for _, p in plans} == every                               # k_mha_fwd<4 .. 64, true | false>
    assert {p['bwd'] for _, p in plans} == {e for e in every if not e.startswith('64')} | {None}       # k_mha_bwd<4 .. 32, ..>
    # the widths of the table, each in both directions up to 32 and forward only beyond
    assert [p['dh'] for _, p in plans[:len(S.WIDTH_CASES)]] == [1, 2, 3, 4, 5, 6, 8, 12, 16, 17, 20, 32, 33, 36, 64]
    assert all(c.layout == 'contig' for c in S.WIDTH_CASES)
    assert [(p['fwd'][-1], p['bwd'] and p['bwd'][-1]) for _, p in plans[:len(S.WIDTH_CASES)]] == \
        [('s', 's')] * 3 + [('v', 'v')] + [('s', 's')] * 2 + [('v', 'v')] * 3 + [('s', 's')] + [('v', 'v')] * 2 + \
        [('s', None), ('v', None), ('v', None)]
    assert any(c.D % 4 == 0 and (c.D // c.H) % 4 for c in S.WIDTH_CASES)        # D = 12, H = 2: D % 4 alone is not enough
    # layouts: every float4 bracket in the production layout, every bracket padded by one float; scalar widths in blocks; no lse
    lay = {(c.layout, p['fwd']) for c, p in plans}
    assert lay >= {('prod', f'{b}v') for b in S.BRACKETS} | {('odd', f'{b}s') for b in S.BRACKETS} | {('prod', '8s')}
    assert {(c.layout, p['bwd']) for c, p in plans} >= {('prod', f'{b}v') for b in S.BRACKETS[:4]} | {('odd', f'{b}s') for b in S.BRACKETS[:4]}
    assert {p['fwd'] for c, p in plans if not c.lse} == {'4v', '4s'}
    assert any((c.F, c.D, c.H, c.layout) == (5, 4, 1, 'prod') for c in S.CASES)                          # the default configuration
    for a, b in S.PAIRS:                                                        # same shape and values, float4 against one float
        assert (a.B, a.F, a.D, a.H, a.rate, a.seed, a.data) == (b.B, b.F, b.D, b.H, b.rate, b.seed, b.data)
        assert S.plan(a)['bwd'][-1] == 'v' and S.plan(b)['bwd'][-1] == 's' and S.plan(a)['bwd'][:-1] == S.plan(b)['bwd'][:-1]
        assert all(torch.equal(x, y) for x, y in zip(S.build_inputs(a), S.build_inputs(b)))
    assert any(a.rate > 0 for a, _ in S.PAIRS)
    # buffers one float off a 16-byte boundary: the float4 shape falls to the one-float kernels in both directions
    assert (S.plan(S.OFFSET_CASE)['fwd'], S.plan(S.OFFSET_CASE, offset=1)['fwd']) == ('8v', '8s')
    assert (S.plan(S.OFFSET_CASE)['bwd'], S.plan(S.OFFSET_CASE, offset=1)['bwd']) == ('8v', '8s')
    # grid edges
    assert {(p['blocks'], p['tail']) for _, p in plans} >= {(1, 255), (1, 256), (2, 1), (3, 133)}
    assert any((c.B, c.H, c.F) == (257, 1, 1) for c in S.CASES) and any(c.F == 1 and c.H == 2 for c in S.CASES)
    assert any(c.F == 3 and c.H == 2 and p['bh_per_wave'] > 10 for c, p in plans)
    assert {c.F for c in S.CASES if c.rate == 0} >= {65, 70} and S.EMPTY_BATCH[0] == 0
    # dropout
    for F in (64, 5):
        assert [c.rate for c in S.DROP_CASES if c.F == F and c.rate != S.TINY_RATE] == list(S.DROP_RATES)
    assert all(c.H >= 3 for c in S.DROP_CASES if c.F in (64, 5) and c.rate != S.TINY_RATE)
    assert any(p['thr'] == 1 for c, p in plans if c.rate > 0) and S.TINY_RATE * 2 ** 32 < 1
    assert all(c.F <= S.DROP_MAX_F for c in S.DROP_CASES) and {c.F for c in S.DROP_CASES} >= {S.DROP_MAX_F}
    # hard inputs: every kind on a float4, a one-float and a production-layout shape
    for B, F, D, H, lay_, _ in S.HARD_SHAPES:
        assert {c.data for c in S.HARD_CASES if (c.B, c.F, c.D, c.H, c.layout) == (B, F, D, H, lay_)} == set(S.DATA[1:])
    assert [p for *_, p in S.HARD_SHAPES] == ['4v', '8s', '16v']
    # the refused shapes of the domain
    assert set(S.REFUSED) == {(5, 40, 1, 0.0), (5, 64, 1, 0.0), (4, 65, 1, 0.0), (65, 8, 2, 0.3)}


# ---- the references -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', S.params_of(S.CASES + [S.OFFSET_CASE]))
def test_references_are_fit_to_measure_against(c):
    from oracle import closed_form as C
    ref = S.references(c)
    for t in (ref.q, ref.k, ref.v, ref.up):
        assert torch.equal(t, t.float().double())                              # float32 holds every input exactly
    # the two float64 forms agree to 1e-10 of each tensor's largest entry, and with the oracle where it applies (no dropout)
    for n in S.NAMES:
        a, b = ref.r64[n], ref.loop64[n]
        assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()), n
        assert float((a - b).abs().max()) <= 1e-10 * max(float(a.abs().max()), 1.0), (n, float((a - b).abs().max()))
    if ref.keep is None:
        want = C.mha_core(ref.q.numpy(), ref.k.numpy(), ref.v.numpy(), c.H)
        assert float(np.abs(ref.r64['out'].numpy() - want).max()) <= 1e-10 * max(float(np.abs(want).max()), 1.0)
    # the float32 yardstick is finite; nothing to measure is zero everywhere except where the case says so
    for n in S.NAMES:
        for m in S.METRICS:
            assert np.isfinite(ref.yard[n][m]), (n, m)
        zero_ok = (c.data == 'q0' and n == 'grad_k') or (c.F == 1 and n in ('grad_q', 'grad_k'))
        assert zero_ok or float(ref.r64[n].abs().max()) > 0, f'{n} of {c.id} is zero everywhere: nothing to measure'
    # what the hard inputs are meant to be
    w = torch.softmax(S._heads(ref.q, c.H) @ S._heads(ref.k, c.H).transpose(-1, -2) / (c.D // c.H) ** 0.5, -1)
    if c.data == 'q0':
        assert not bool(ref.r64['grad_k'].any()) and bool(ref.r64['grad_q'].any()) and torch.allclose(w, torch.full_like(w, 1.0 / c.F))
    if c.data == 'q1000':
        scores = S._heads(ref.q, c.H) @ S._heads(ref.k, c.H).transpose(-1, -2) / (c.D // c.H) ** 0.5
        assert float(scores.max()) > 89.0 and float(w.amax(-1).median()) > 0.999          # expf overflows; one-hot rows
    if c.data == 'signed':
        assert float(ref.q.min()) < 0 and float(ref.k.min()) < 0 and float(ref.v.min()) < 0
    if c.data == 'fields':
        top = ref.q.abs().amax((0, 2))
        assert float(top.max() / top.min()) > 1e5
    if c.F == 1:                                                                # softmax of one score: weight 1, no gradient to q, k
        assert not bool(ref.r64['grad_q'].any()) and not bool(ref.r64['grad_k'].any()) and torch.equal(ref.r64['grad_v'], ref.up)


@pytest.mark.parametrize('c', S.params_of(S.DROP_CASES))
def test_dropout_cases_drop_their_share(c):
    """a condition on the chosen seeds: the dropped share of the restated mask is within 0.05 of the rate, the mask is not
    symmetric (the backward's second role reads it as (i, r): swapped indices would show), and differs between heads"""
    keep = S.references(c).keep
    assert set(keep.unique().tolist()) <= {0.0, S.keep_scale(c.rate)}
    dropped = float((keep == 0).double().mean())
    assert abs(dropped - S.f32(c.rate)) <= 0.05, (dropped, c.rate)
    if c.rate != S.TINY_RATE:
        assert not torch.equal(keep, keep.transpose(-1, -2)) and not torch.equal(keep[:, 0], keep[:, c.H - 1])
        assert not torch.equal(keep[0], keep[c.B - 1])
    else:
        assert dropped == 0.0 and S.threshold(c.rate) == 1


def test_a_wrong_threshold_or_swapped_mask_goes_red():
    """the bar the kernels are held to, on the defects the dropout cases are there for: the float32 loop form with the Python
    double's threshold where a hash lands in the gap, with the mask transposed, and without the h * 4096 term"""
    c = S.DROP_CASES[1]
    ref = S.references(c)
    good = S.evaluate(S.mha_loop, ref.q, ref.k, ref.v, ref.up, c.H, ref.keep, torch.float32)
    S.check('host:unmutated', good, ref)
    one_head = S.keep_mask(c.seed, c.B, 1, c.F, c.rate).expand(c.B, c.H, c.F, c.F)
    flipped = ref.keep.clone()
    flipped[1, 2, 3, 4] = S.keep_scale(c.rate) - flipped[1, 2, 3, 4]            # one weight on the other side of the threshold
    for name, keep in (('transposed', ref.keep.transpose(-1, -2)), ('no_head_term', one_head), ('one_flip', flipped)):
        bad = S.evaluate(S.mha_loop, ref.q, ref.k, ref.v, ref.up, c.H, keep, torch.float32)
        figs = S.figures(bad, ref.r64, ref.yard)
        ratios = {k: g / max(f, P.FLOOR) for k, (_, g, f) in figs.items()}
        assert max(ratios.values()) > 100 * P.STEP_BAR['fp32'], (name, ratios)


@pytest.mark.parametrize('F,D,H,rate', list(S.REFUSED))
def test_layer_core_outside_the_domain_is_the_reference(F, D, H, rate):
    """MultiheadAttention._core_by_ops, what the layer runs where dt_mha_core_supported says no, in float64 on the CPU"""
    from deeptables_amd.models import layers
    c = S.refused_case(F, D, H, 0.0)
    q, k, v, up = S.build_inputs(c)
    want = S.evaluate(S.mha_matmul, q, k, v, up, H, None, F64)
    layer = layers.MultiheadAttention({'num_heads': H, 'dropout_rate': rate})
    xs = [t.clone().requires_grad_(True) for t in (q, k, v)]
    out = layer._core_by_ops(*xs, 0.0)
    (out * up).sum().backward()
    for n, a in zip(('out', 'grad_q', 'grad_k', 'grad_v'), [out.detach()] + [t.grad for t in xs]):
        assert float((a - want[n]).abs().max()) <= 1e-12 * max(float(want[n].abs().max()), 1.0), n
    if rate > 0:                                                # dropout on the weights: kept weights scaled, rows differ per call
        torch.manual_seed(0)
        a, b = layer._core_by_ops(q, k, v, rate), layer._core_by_ops(q, k, v, rate)
        assert not torch.equal(a, b) and bool(torch.isfinite(a).all())


@pytest.mark.parametrize('shape', S.LAYER_SHAPES)
def test_layer_references_are_fit_to_measure_against(shape):
    """no relu unit of the projections or of the output sits within float32's reach of its kink, so two precisions agree on
    every derivative"""
    B, F, D, H = shape
    t, r64, yard = S.layer_references(shape)
    pre = S.layer_pre(t['x'], t['W'], t['b'])
    scale = t['x'].abs() @ t['W'].abs() + t['b'].abs()
    assert float((pre.abs() / scale).min()) > P.KINK_TOL['fp32']
    y = torch.relu(pre)
    core = S.mha_matmul(y[..., :D], y[..., D:2 * D], y[..., 2 * D:3 * D], H)[0] + y[..., 3 * D:]
    assert float(core.min()) >= 0 and float(core[core > 0].min()) > P.KINK_TOL['fp32'] * float(core.max())
    for n in S.LAYER_NAMES:
        assert float(r64[n].abs().max()) > 0 and all(np.isfinite(yard[n][m]) for m in S.METRICS)
    from deeptables_amd import _lib
    assert not _lib.lib().dt_autoint_supported(F, D, H) and S.supported(F, D, H, False)     # the generic path, inside its domain
