# -*- coding:utf-8 -*-
"""Host: the case tables of tests/rows_support.py against the launch arithmetic it restates (an id can never drift from the path
it names), that every template instantiation and every launcher branch of csrc/embedding.hip and csrc/cross.hip has a case, the
restatement against dt_cross_workspace_bytes, the float64 references against oracle/reference_layers, and every GPU case's
references against themselves before an input reaches a GPU: the float32 reference in another summation order stays within the
bar the kernels will be held to, no scale is zero except where every term is zero, the composed cross scale stays within
CROSS_SCALE_GROWTH of what the element is made of, and wrong cross arithmetic goes over that bar on every cross case."""
import pytest
import torch

from tests import precision as P
from tests import rows_support as S

F64, F32 = torch.float64, torch.float32


# ---- the restatement at the figures the ids and the docstrings quote ---------------------------------------------------------------
def test_restatement_at_the_quoted_figures():
    assert [S.fast_lpr(D) for D in (4, 8, 16, 32, 64, 128, 256)] == list(S.LPRS)
    assert all(S.fast_lpr(D) is None for D in (1, 3, 6, 10, 12, 20, 260, 512, 0))
    assert S.row_trips(130, 1) == 3 and S.row_trips(1, 64) == 1 and S.row_trips(3, 64) == 3 and S.row_trips(33, 2) == 2
    assert S.row_grid(5, 16) == (2, 256) and S.row_grid(5, 6) == (5, 64)
    assert S.generic_lds(32, 512) == S.LDS_64K and not S.row_fwd_refused(32, 512) and S.row_fwd_refused(*S.ROW_REFUSED)
    assert not S.row_fwd_refused(1000, 256)                                    # the fast path has no row buffer
    assert S.gather_grid(2049, 8, 256) == (4096, 2) and 2049 * 8 * 64 == 1049088 and S.gather_grid(2048, 8, 256) == (4096, 1)
    assert S.scatter_grid(4100, 256) == (4096, 2) and S.scatter_grid(4096, 256) == (4096, 1)
    assert S.owned_grid(1, 1, 8193, 1024) == (8192, 2) and S.owned_grid(1, 1, 8192, 1024) == (8192, 1)
    assert S.feed_grid(1) == 1 and S.feed_grid(33) == 2 and S.feed_grid(1100) == 35 and S.feed_grid(524289) == 16384
    assert S.feed_passes(524288) == 1 and S.feed_passes(524289) == 2
    assert S.feed_G(2) == 2 and S.feed_G(35) == 32 and [S.feed_members(35, g) for g in (0, 2, 3, 31)] == [2, 2, 1, 1]
    assert sum(S.feed_members(35, g) for g in range(32)) == 35 and S.feed_members(16384, 7) == 512
    assert S.FEED_CURSOR_WORDS == 528
    assert [S.cross_per(C) for C in (1, 64, 65, 129, 193, 257, 321, 385, 449, 512, 513, 1024, 1025, 2048, 2049)] == \
        [1, 1, 2, 3, 4, 5, 6, 7, 8, 8, 16, 16, 32, 32, 64]
    assert [S.cross_blocks(B) for B in (1, 4, 5, 256, 257, 513, 2048, 2049, 2053)] == [1, 1, 2, 64, 65, 129, 512, 512, 512]
    assert S.cross_fwd_blocks(8192) == 2048 == S.cross_fwd_blocks(8193)
    assert [S.cross_bwd_kernel(512, L) for L in (1, 4, 5, 8, 9)] == ['reg4', 'reg4', 'reg8', 'reg8', 'generic']
    assert S.cross_bwd_kernel(513, 1) == 'generic' and S.cross_bwd_kernel(65, 9) == 'generic'
    assert S.cross_bwd_refusal(2048, 4) is None and S.cross_bwd_refusal(1024, 8) is None
    assert S.cross_bwd_refusal(*S.CROSS_FORWARD_ONLY) == 'LDS' and not S.cross_fwd_refused(S.CROSS_FORWARD_ONLY[0])
    assert S.cross_bwd_refusal(S.CROSS_REFUSED_C, 1) == 'C' and S.cross_fwd_refused(S.CROSS_REFUSED_C)
    assert [S.reduce_plan(n) for n in (1, 2, 64, 65, 129, 512)] == [(0, True), (0, True), (0, True), (1, True), (1, True), (4, False)]


def test_the_staging_condition_of_the_register_kernels_is_never_false():
    """`2 * lds <= 64 KiB` in DT_CROSS_BWD (rows_support.cross_bwd_kernel): once L <= 8 and P <= 8, L C <= 4,096"""
    for C in range(1, 513):
        assert S.cross_per(C) <= 8
        for L in range(0, 9):
            assert 2 * S.cross_bwd_lds(C, L) <= S.LDS_64K and S.cross_bwd_kernel(C, L) == ('reg4' if L <= 4 else 'reg8')
    assert S.cross_per(513) > 8


def test_workspace_restatement_equals_the_library():
    from deeptables_amd import _lib
    lib = _lib.lib()
    for B in list(range(0, 70)) + [255, 256, 257, 513, 2047, 2048, 2049, 2053, 8193, 100000]:
        for C, L in ((1, 1), (7, 2), (65, 9), (2048, 4), (512, 8), (7, 0), (0, 3)):
            assert lib.dt_cross_workspace_bytes(B, C, L) == S.cross_workspace_bytes(B, C, L), (B, C, L)


# ---- case hygiene -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', S.params_of(S.ROW_CASES + S.POINTER_CASES))
def test_row_case_takes_the_path_its_id_names(c):
    plan = S.row_plan(c)
    if c in S.FAST_CASES + S.GENERIC_CASES:
        assert c.expect, 'a path case states what it expects of the plan'
    for k, want in c.expect.items():
        assert plan[k] == want, (c.id, k, plan[k], want)
    assert not S.row_fwd_refused(c.F, c.D) and c.data in S.ROW_DATA
    assert c.B * c.F * c.D <= 2 ** 21                                            # every buffer of a row case stays under 8 MB


@pytest.mark.parametrize('c', S.params_of(S.CROSS_CASES + S.CROSS_CONTRACT_CASES))
def test_cross_case_takes_the_path_its_id_names(c):
    plan = S.cross_plan(c)
    if c in S.CROSS_PATH_CASES:
        assert c.expect
    for k, want in c.expect.items():
        assert plan[k] == want, (c.id, k, plan[k], want)
    assert not S.cross_fwd_refused(c.C) and S.cross_bwd_refusal(c.C, c.L) is None and c.data in S.CROSS_DATA


def test_the_tables_cover_every_instantiation_and_every_launcher_branch():
    # k_row_fwd<KIND, LPR, true> (both kinds: kind_params), k_row_fwd<I32, LPR, false> (dt_fm_fwd) and k_row_bwd<LPR> run for
    # every fast case: every LPR at every filling its kernel can have
    fills = {(S.row_plan(c)['lpr'], S.row_plan(c)['fill']) for c in S.FAST_CASES}
    want = {(l, f) for l in S.LPRS for f in ('part', 'full', 'ragged', 'multi')} - {(64, 'part'), (64, 'ragged')} | {(64, 'two_full')}
    assert fills == want, fills ^ want
    assert {S.row_plan(c)['trips'] for c in S.FAST_CASES} >= {1, 2, 3}
    assert {c.B for c in S.FAST_CASES} == {1, 3, 5} and {c.Nd for c in S.FAST_CASES} == {0, 1, 13, 70}
    for lpr in S.LPRS:                                                           # ... with idle waves and without, per kernel
        assert {S.row_plan(c)['idle_waves'] > 0 for c in S.FAST_CASES if S.row_plan(c)['lpr'] == lpr} >= {True}
    assert any(S.row_plan(c)['dense_loops'] == 2 for c in S.FAST_CASES)          # the k += 64 loop of the dense tail
    # k_row_fwd_generic<KIND, GATHER>, k_row_bwd_generic
    gen = [S.row_plan(c) for c in S.GENERIC_CASES]
    assert all(p['path'] == 'generic' for p in gen)
    assert {c.D for c in S.GENERIC_CASES} == {1, 3, 6, 10, 12, 20, 260, 512}
    assert any(p['f_loops'] == 2 for p in gen) and any(p['d_loops'] > 1 for p in gen) and any(c.Nd == 70 for c in S.GENERIC_CASES)
    assert any(p['lds'] == S.LDS_64K for p in gen) and S.row_fwd_refused(*S.ROW_REFUSED)
    assert (S.ROW_REFUSED[0] - 1, S.ROW_REFUSED[1]) in {(c.F, c.D) for c in S.GENERIC_CASES}
    # ids, hard inputs, pointers: one shape per kernel family each
    assert [S.row_plan(c).get('lpr') for c in S.ID_CASES] == [1, 8, 64, None] and all(c.data == 'ids' for c in S.ID_CASES)
    for shape in (S.HARD_FAST, S.HARD_GENERIC):
        assert {c.data for c in S.HARD_ROW_CASES if (c.B, c.F, c.D, c.Nd) == shape} == \
            {'logspace', 'offset', 'zero_rows', 'zero_field', 'all_oob'}
    assert S.fast_lpr(S.HARD_FAST[2]) == 8 and S.fast_lpr(S.HARD_GENERIC[2]) is None
    assert {(c.F, S.row_plan(c)['path'], c.data) for c in S.HARD_ROW_CASES if c.F == 1} == \
        {(1, p, d) for p in ('fast', 'generic') for d in ('mild', 'offset')}
    assert [S.row_plan(c)['path'] for c in S.POINTER_CASES] == ['fast', 'generic'] and all(c.Nd > 0 for c in S.POINTER_CASES)
    # dt_embedding_fwd: k_gather_vec4 at D = 4, 12, 260, one loop step past its cap; D % 4 != 0 -> the generic row kernel
    assert {D for _, _, D in S.GATHER_CASES if S.gather_path(D) == 'vec4'} >= {4, 12, 260}
    assert any(S.gather_path(D) == 'generic' for _, _, D in S.GATHER_CASES)
    assert {S.gather_grid(*t)[1] for t in S.GATHER_CASES if S.gather_path(t[2]) == 'vec4'} == {1, 2}
    assert S.scatter_grid(*S.SCATTER_WRAP[:2]) == (4096, 2)
    # dt_embedding_gather_owned
    assert {t[0] for t in S.OWNED_CASES} == {1, 3} and any(t[3] == t[4] for t in S.OWNED_CASES)
    assert {(t[3] == 0, t[4] == t[2]) for t in S.OWNED_CASES if t[3] != t[4]} == {(True, False), (False, False), (False, True), (True, True)}
    assert {S.owned_grid(W, f1 - f0, B, D)[1] for W, B, F, f0, f1, D in S.OWNED_CASES if f1 > f0} == {1, 2}
    # dt_feed_gather
    assert {len(rb) for _, rb in S.FEED_CASES} == {1, 3, 8} and {b for _, rb in S.FEED_CASES for b in rb} >= {4, 12, 260, 1028}
    assert {n for n, _ in S.FEED_CASES} >= {1, 7, 8, 9, 33, 1000}
    assert any(sum(rb) > 256 and max(rb) <= 256 for _, rb in S.FEED_CASES) and any(max(rb) > 256 for _, rb in S.FEED_CASES)
    grids = [S.feed_grid(n) for n in S.FEED_CURSOR_LAUNCHES]
    assert any(1 < g < 32 for g in grids) and 1 in grids and S.FEED_MAX_BLOCKS in grids
    assert any(g % 32 and g > 32 and len({S.feed_members(g, k) for k in range(32)}) == 2 for g in grids)
    assert all(len({S.feed_members(b, k) for k in range(32)}) == 2 for b in S.FEED_UNEVEN_GRIDS) and len(S.FEED_UNEVEN_GRIDS) == 3
    assert any(S.feed_passes(n) == 2 for n, _ in S.FEED_CASES) and any(S.feed_passes(n) == 2 for n in S.FEED_CURSOR_LAUNCHES)
    # cross: k_cross_fwd<PER> for all ten PER; k_cross_bwd_reg<P, 4 | 8> and k_cross_bwd<P> for P = 1 .. 8; k_cross_bwd<16 | 32>
    plans = [(c, S.cross_plan(c)) for c in S.CROSS_PATH_CASES]
    assert {p['per'] for _, p in plans} == set(S.CROSS_PERS)
    assert {(p['per'], p['bwd']) for c, p in plans if c.L > 0} == \
        {(per, k) for per in range(1, 9) for k in ('reg4', 'reg8', 'generic')} | {(16, 'generic'), (32, 'generic')}
    assert {c.C for c, _ in plans} >= {1, 64, 65, 129, 193, 257, 321, 385, 449, 512, 513, 1024, 1025, 2048}
    for kern, Ls in (('reg4', {1, 4}), ('reg8', {5, 8})):
        assert {c.L for c, p in plans if p['bwd'] == kern} >= Ls
    assert any(c.L == 0 for c, _ in plans) and {c.L for c, p in plans if p['per'] <= 8 and p['bwd'] == 'generic'} == {9}
    assert {c.C for c, p in plans if c.L == 9} >= {65, 512}
    assert {(c.C, c.L) for c, p in plans if p['lds'] == S.LDS_64K} == {(2048, 4), (1024, 8)} and any(p['lds'] == 32768 and p['bwd'] == 'reg8' for _, p in plans)
    assert {c.B for c, _ in plans} >= {1, 4, 5, 256, 257, 513, 2048, 2049, 2053, 8193}
    assert {p['nblocks'] for _, p in plans} >= {1, 2, 64, 65, 129, 512}
    assert {(p['reduce_loops'] > 0, p['reduce_tail']) for _, p in plans} == {(False, True), (True, True), (True, False)}
    assert {(p['bwd'], p['bwd_stride']) for _, p in plans} >= {('reg4', True), ('generic', True), ('reg4', False)}
    assert any(p['fwd_stride'] for _, p in plans)
    for shape in S.HARD_CROSS_SHAPES:
        assert {c.data for c in S.HARD_CROSS_CASES if (c.B, c.C, c.L) == shape} == set(S.CROSS_DATA[1:])
    assert [(S.cross_per(C), S.cross_bwd_kernel(C, L), L) for _, C, L in S.HARD_CROSS_SHAPES] == \
        [(3, 'reg4', 2), (16, 'generic', 2), (3, 'reg8', 8), (3, 'generic', 9)]
    assert [S.cross_plan(c)['bwd'] for c in S.CROSS_CONTRACT_CASES] == ['reg4', 'generic']


# ---- the references against the oracle ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('c,kind', S.kind_params([S.FAST_CASES[5], S.GENERIC_CASES[2], S.ID_CASES[1]]))
def test_row_references_agree_with_the_oracle(c, kind):
    from oracle import reference_layers as R
    r, r64, _, _ = S.rows_refs(c, kind)
    idx = r.idx.clone()
    idx[~r.ok] = 0                                             # the oracle has no range check: ask it for row 0, mask afterwards
    tables = [r.table[o:o + v] for o, v in zip(r.row_offset.tolist(), r.vocab.tolist())]
    emb = torch.cat(R.multi_column_embedding(idx, tables), 1) * r.ok[:, :, None]
    assert torch.equal(emb, r64.emb)
    x = emb.clone().requires_grad_(True)
    fm = R.fm(x)
    assert torch.allclose(fm.reshape(-1), r64.fm, rtol=1e-12, atol=1e-12) and torch.allclose(emb.sum(-1), r64.fsum, rtol=1e-13, atol=0)
    flat = x.reshape(c.B, -1)
    concat = flat if r.dense is None else torch.cat([flat, r.dense], 1)
    assert torch.equal(concat.detach(), r64.concat)
    ((x * r.ups[0]).sum() + (concat * r.ups[1]).sum() + (x.sum(-1) * r.ups[2]).sum() + (fm.reshape(-1) * r.ups[3]).sum()).backward()
    assert torch.allclose(x.grad, r64.grad_rows, rtol=1e-11, atol=1e-11)
    want = torch.zeros_like(r.table).index_put_((r.rows[r.ok],), x.grad[r.ok], accumulate=True)
    assert torch.allclose(want, r64.grad_table, rtol=1e-11, atol=1e-11)


@pytest.mark.parametrize('c', S.params_of([S.CROSS_PATH_CASES[4], S.CROSS_PATH_CASES[8], S.HARD_CROSS_CASES[3]]))
def test_cross_reference_agrees_with_the_oracle(c):
    from oracle import reference_layers as R
    ref = S.cross_refs(c)
    xs = [t.clone().requires_grad_(True) for t in ref.inputs]
    y = R.cross(xs[0], [xs[1][i].unsqueeze(1) for i in range(c.L)], [xs[2][i].unsqueeze(1) for i in range(c.L)])
    (y * ref.up).sum().backward()
    for name, a, e, s in zip(S.CROSS_FIGURES, [y.detach()] + [t.grad for t in xs], ref.r64, ref.scales):
        assert P.elem_cond(a, e, s) <= 2.0 ** -45, name


# ---- the references alone -----------------------------------------------------------------------------------------------------
ZERO_OK = {'all_oob': {'fsum', 'fm', 'grad_table'}}


def _zero_scale_means_zero_terms(name, ref, scale):
    dead = scale == 0
    assert not bool(ref[dead].any()), f'{name}: a zero scale under a nonzero reference'


@pytest.mark.parametrize('c,kind', S.kind_params(S.ROW_CASES + S.POINTER_CASES))
def test_row_references_are_fit_to_measure_against(c, kind):
    r, r64, r32, sc = S.rows_refs(c, kind)
    for t in [r.table, r.dense] + r.ups:
        assert t is None or torch.equal(t, t.float().double())                  # float32 holds every input exactly
    flipped = S.rows_reference(r, F32, flip=True)
    got = {n: getattr(flipped, n) for n in ('fsum', 'fm', 'grad_rows', 'grad_table')}
    S.check('host:f32_flipped', 'embed_fm_linear', S.row_figs(got, r64, r32, sc))
    for n in got:
        assert bool(torch.isfinite(getattr(r64, n)).all())
        _zero_scale_means_zero_terms(n, getattr(r64, n), getattr(sc, n))
        if n not in ZERO_OK.get(c.data, ()) and not (c.F == 1 and n == 'fm'):
            assert float(getattr(r64, n).abs().max()) > 0, f'{n} of {c.id} is zero everywhere: nothing to measure'
        assert float(getattr(sc, n).max()) > 0 or c.data == 'all_oob'
    # what the hard inputs are meant to be
    if c.F == 1:
        assert float(r64.fm.abs().max()) < 1e-9 * float(sc.fm.min()) and float(sc.fm.min()) > 0     # true value 0, scale not
    if c.data == 'offset':
        assert float(r.table.mean()) > 50 * float(r.table.std())
    if c.data == 'all_oob':
        assert not bool(r.ok.any()) and not bool(r64.emb.any()) and not bool(r64.grad_table.any()) and bool(r64.grad_rows.any())
    if c.data == 'zero_field':
        assert not bool(r64.emb[:, S.ZERO_FIELD].any()) and not bool(r64.fsum[:, S.ZERO_FIELD].any()) and bool(r64.grad_rows[:, S.ZERO_FIELD].any())
    if c.data == 'zero_rows':
        assert bool((r64.emb.abs().sum(-1) == 0).any()) and bool((r64.emb.abs().sum(-1) > 0).any())
    if c.data == 'ids':
        specials = S.special_ids(kind, 5)
        assert int((~r.ok).sum()) == 2 * sum(1 for _, good, _ in specials if not good) and bool(r.ok.any())
        assert bool((r.rows[~r.ok] == -1).all()) and bool((r.rows[r.ok] >= 0).all())


@pytest.mark.parametrize('c', S.params_of(S.CROSS_CASES + S.CROSS_CONTRACT_CASES))
def test_cross_references_are_fit_to_measure_against(c):
    ref = S.cross_refs(c)
    for t in ref.inputs + [ref.up]:
        assert torch.equal(t, t.float().double())
    perm = torch.randperm(c.B, generator=torch.Generator().manual_seed(c.B))
    S.check('host:f32_permuted', 'cross', S.cross_figs(S.cross_reference(ref.inputs, ref.up, F32, perm=perm), ref))
    for name, e, s in zip(S.CROSS_FIGURES, ref.r64, ref.scales):
        assert bool(torch.isfinite(e).all()), name
        _zero_scale_means_zero_terms(name, e, s)
        if c.L > 0 or name in ('y', 'dx'):
            assert float(e.abs().max()) > 0, name
    x, w, b = ref.inputs
    if c.data != 'growth':                                      # the composed scale has not outgrown what the element is made of
        assert float((ref.scales[0] / (x.abs() + b.abs().sum(0)[None, :])).max()) <= S.CROSS_SCALE_GROWTH
    if c.data == 'perp':
        s0, big = (x * w[0]).sum(1).abs(), (x.abs() * w[0].abs()).sum(1)
        assert float((s0 / big).max()) < 1e-6
    if c.data == 'bias_minus_x':
        assert float((x + b[0]).abs().max()) < 1e-2 * float(x.abs().max())
    if c.data == 'growth':
        assert float(ref.r64[0].abs().max()) > 2.0 ** (c.L - 2) * float(x.abs().max())
    if c.data == 'w_zero':
        assert torch.equal(ref.r64[0], x + b.sum(0)[None, :]) or torch.allclose(ref.r64[0], x + b.sum(0)[None, :], rtol=1e-14, atol=1e-14)
    if c.data == 'zero_rows':
        assert not bool(x[::2].any()) and bool(ref.r64[1][::2].any())
    if c.data == 'zero_column':                                 # x_0 of the column is zero: x_l there is the sum of the biases
        assert torch.equal(ref.r64[0][:, S.ZERO_COLUMN], b[:, S.ZERO_COLUMN].sum().expand(c.B)) and not bool(ref.r64[2][0, S.ZERO_COLUMN])


# ---- the cross bar has teeth on every case ------------------------------------------------------------------------------------
CROSS_MUTANTS = {'dropped_layer': ('y',), 'dropped_acc_term': ('dx',), 'zeroed_dw_row': ('dw',), 'swapped_column': ('y',),
                 'bf16_operands': ('y', 'dx', 'dw')}


def _mutated_cross(ref, mutant):
    """rows_support.cross_reference in float32 with one thing wrong: the middle layer of the forward skipped | grad_x without
    its sum_l g_{l+1} s_l | grad_w of the middle layer zero | y column 3 a copy of column 4 | s_l and t_l from operands rounded
    to bf16"""
    x, w, b = [t.float() for t in ref.inputs]
    g = ref.up.float()
    L, mid = w.shape[0], w.shape[0] // 2

    def dot(u, v):
        if mutant == 'bf16_operands':
            u, v = u.bfloat16().float(), v.bfloat16().float()
        return (u * v).sum(1, keepdim=True)

    xs, s = [x], []
    for l in range(L):
        s.append(dot(xs[l], w[l].expand_as(x)))
        xs.append(xs[l] if mutant == 'dropped_layer' and l == mid else x * s[l] + xs[l] + b[l])
    gw, gb, acc = torch.zeros_like(w), torch.zeros_like(b), torch.zeros_like(x)
    for l in range(L - 1, -1, -1):
        t = dot(g, x)
        gw[l], gb[l] = (xs[l] * t).sum(0), g.sum(0)
        acc = acc + g * s[l]
        g = g + w[l] * t
    y, gx = xs[L].clone(), g if mutant == 'dropped_acc_term' else g + acc
    if mutant == 'zeroed_dw_row':
        gw[mid] = 0.0
    if mutant == 'swapped_column':
        y[:, 3] = y[:, 4]
    return [y, gx, gw, gb]


@pytest.mark.parametrize('c', S.params_of([c for c in S.CROSS_CASES + S.CROSS_CONTRACT_CASES if c.L > 0]))
def test_a_wrong_cross_net_goes_red_on_every_case(c):
    """the bar the kernels are held to, on wrong float32 arithmetic: on every case with a layer, the unmutated float32 formula
    passes and each mutant is over the bar in (one of) the figures it damages.  Left out only where the mutant changes nothing:
    w = 0 has no s_l (the acc term is zero) and C < 5 has no columns 3 and 4."""
    ref = S.cross_refs(c)
    S.check('host:unmutated', 'cross', S.cross_figs(_mutated_cross(ref, None), ref))
    for mutant, damaged in CROSS_MUTANTS.items():
        if (mutant == 'dropped_acc_term' and c.data == 'w_zero') or (mutant == 'swapped_column' and c.C < 5):
            continue
        figs = S.cross_figs(_mutated_cross(ref, mutant), ref)
        ratios = {n: g / max(f, P.FLOOR) for n, (g, f) in ((n, S.errs(n, *figs[n][1:])) for n in damaged)}
        assert max(ratios.values()) > P.STEP_BAR['fp32'], (mutant, ratios)
