# -*- coding:utf-8 -*-
"""Host: the case table of tests/pairwise_support.py against the dispatch arithmetic it restates — an id can never drift
from the shape it names — and every GPU case's references against themselves, before an input reaches a GPU: the float64
reference is finite, it is nonzero wherever the case measures, and the float32 CPU reference walked over a permuted batch
(float32 in another summation order) stays within the bar the kernel will be held to."""
import pytest
import torch

from tests import pairwise_support as S
from tests import precision as P

F64, F32 = torch.float64, torch.float32


# ---- the plans, at the figures the ids quote -------------------------------------------------------------------------------
def test_plans_at_the_quoted_shapes():
    assert S.op16_plan(1000) == (63, 1, 63)                              # the largest batch of the older tests: one split
    assert S.op16_plan(1008) == (63, 1, 63) and S.op16_plan(1009) == (64, 8, 8) and S.op16_plan(1040) == (65, 8, 9)
    assert S.generic_wgrad_plan(1024) == (1, 1024) and S.generic_wgrad_plan(1025) == (2, 576)
    assert S.generic_wgrad_plan(16384) == (16, 1024) and S.generic_wgrad_plan(16385) == (16, 1088)
    assert S.mfma_bwd(36, 16) and not S.mfma_bwd(37, 16) and not S.mfma_bwd(3, 17)
    assert S.lds16_bwd_x(36) == 149992
    assert not S.afm_blocked(6, 8) and S.afm_blocked(8, 8) and S.afm_blocked(64, 64) and not S.afm_blocked(68, 33)
    assert [S.afm_hmax(H) for H in (1, 16, 17, 32, 33, 64)] == [16, 16, 32, 32, 64, 64]
    assert S.pair_grid(8192, False, True) == (2048, 1) and S.pair_grid(8193, False, True) == (2048, 2)
    assert S.pair_grid(1024, True, False) == (256, 1) and S.pair_grid(1025, True, False) == (256, 2)
    assert S.pair_grid(8193, False, False) == (2048, 2)
    assert S.afm_grid(2048, True) == (2048, 1) and S.afm_grid(2049, True) == (2048, 2)
    assert S.afm_grid(512, False) == (512, 1) and S.afm_grid(513, False) == (512, 2)
    assert S.lds_bilinear_bwd_x(64) == 66304 and S.lds_bilinear_bwd_x(63) == 65028 <= 64 * 1024
    assert S.lds_generic_fwd(64) == 49664 and S.lds_generic_wgrad(64) == 32768


def test_refusal_sizes():
    """the shapes test_refusals of the GPU module runs: which side of which bound each lies on"""
    assert S.lds_pair_fwd(26, 40) == 18372 and S.lds_pair_bwd(26, 40, 'outer_vec') == 73840 > 64 * 1024
    assert S.lds_generic_fwd(65) <= 64 * 1024 and S.lds_generic_fwd(77) <= 64 * 1024 < S.lds_generic_fwd(79)
    assert S.afm_lds_fwd(40, 64, 64) <= 150 * 1024 < S.afm_lds_bwd(40, 64, 64)
    assert S.afm_lds_bwd(4, 8, 64) <= 150 * 1024                         # H = 65 is refused for H, not for LDS
    assert S.lds_bilinear_bwd_x(64) <= 150 * 1024                        # within what the launch opts in to


@pytest.mark.parametrize('c', S.params_of(S.PATH_CASES + S.AFM_CASES))
def test_case_takes_the_path_its_id_names(c):
    e = dict(c.expect)
    assert e, 'a path case states what it expects of the plans'
    pair = c.kind in S.PAIR_KINDS
    got = {
        'pair_fwd': lambda: S.pair_grid(c.B, c.kind != 'inner', True),
        'pair_bwd': lambda: S.pair_grid(c.B, c.kind != 'inner', False),
        'pairs': lambda: S.n_pairs(c.F),
        'fd': lambda: c.F * c.D,
        'wgrad': lambda: S.generic_wgrad_plan(c.B),
        'last': lambda: c.B - (S.generic_wgrad_plan(c.B)[0] - 1) * S.generic_wgrad_plan(c.B)[1],
        'nacc': lambda: S.wgrad_accumulators(c.D),
        'mfma': lambda: S.mfma_bwd(c.F, c.D),
        'op16': lambda: S.op16_plan(c.B),
        'last_tiles': lambda: S.op16_plan(c.B)[0] - (S.op16_plan(c.B)[1] - 1) * S.op16_plan(c.B)[2],
        'lds16': lambda: S.lds16_bwd_x(c.F),
        'bil_lds': lambda: S.lds_bilinear_bwd_x(c.D),
        'idle_waves': lambda: sum(a == b for a, b in S.op16_wave_ranges(c.F)),
        'flush': lambda: any(len({S.pair_fields(c.F)[p][0] for p in range(a, b)}) > 1 for a, b in S.op16_wave_ranges(c.F)),
        'hmax': lambda: S.afm_hmax(c.H),
        'blocked': lambda: S.afm_blocked(c.D, c.H),
        'nblk': lambda: (((c.D + 3) & ~3) // 4) * (S.afm_hmax(c.H) // 4),
        'pooled_passes': lambda: S.ceil_div(c.D, 16),
        'afm_fwd': lambda: S.afm_grid(c.B, True),
        'afm_bwd': lambda: S.afm_grid(c.B, False),
    }
    for k, v in e.items():
        assert got[k]() == v, (c.id, k, got[k](), v)
    # every case launches: inside the LDS bound of each kernel it reaches
    if pair:
        assert S.lds_pair_fwd(c.F, c.D) <= 64 * 1024 and S.lds_pair_bwd(c.F, c.D, c.kind) <= 64 * 1024
    elif c.kind == 'afm':
        assert c.H <= 64 and S.afm_lds_fwd(c.F, c.D, c.H) <= 150 * 1024 and S.afm_lds_bwd(c.F, c.D, c.H) <= 150 * 1024
    else:
        assert c.D <= 64
        if S.mfma_bwd(c.F, c.D):
            assert S.lds16_bwd_x(c.F) <= 150 * 1024
        else:
            assert S.lds_generic_fwd(c.D) <= 64 * 1024 and S.lds_bilinear_bwd_x(c.D) <= 150 * 1024


def test_the_table_covers_the_listed_paths():
    ids = set(S.BY_ID)
    assert all(i in ids for i in S.LAYOUT_IDS + S.REPEAT_IDS)
    for kind in S.MAT_KINDS:
        mine = [c for c in S.PATH_CASES if c.kind == kind]
        assert {c.B for c in mine if (c.F, c.D) == (3, 5)} == {63, 64, 65, 1025}
        assert {c.B for c in mine if (c.F, c.D) == (3, 16)} == {1, 15, 16, 17, 65, 1009, 1040}
        assert {(c.B, c.F, c.D) for c in mine} >= {(9, 3, 17), (9, 3, 33), (65, 3, 64), (65, 3, 63), (16385, 2, 3), (17, 37, 16),
                                                   (17, 2, 16), (17, 5, 16), (17, 36, 16)}
    for kind in S.PAIR_KINDS:
        shapes = {(c.B, c.F, c.D) for c in S.PATH_CASES if c.kind == kind}
        assert shapes >= {(1, 2, 1), (5, 2, 4), (7, 12, 3), (9, 3, 70), (8193, 3, 2)}
        assert ((1025, 3, 4) in shapes) == (kind != 'inner')
    afm = S.AFM_CASES
    assert {(c.H, c.act) for c in afm if (c.B, c.F, c.D) == (9, 4, 8) and c.bias} >= {
        (H, a) for H in (1, 16, 17, 32, 33, 64) for a in ('relu', 'tanh')}
    assert any(not c.bias for c in afm)
    for data in S.HARD_DATA:
        assert {(c.kind, c.B, c.F, c.D) for c in S.HARD_CASES if c.data == data} == set(S.HARD_SHAPES)


# ---- the references alone --------------------------------------------------------------------------------------------------
# figures that are zero by construction: a flat softmax (pv = 0) sends no gradient to Wa and ba; with one dominant pair the
# softmax is one-hot to float64's last bit for most rows and the parameter gradients are e^-200 of anything measurable
ZERO_OK = {'afm_flat': {'dWa', 'dba'}, 'afm_dominant': {'dWa', 'dba', 'dpv'}}


@pytest.mark.parametrize('c', S.params_of(S.ALL_CASES))
def test_references_are_fit_to_measure_against(c):
    inputs, up, refs, scales = S.references(c)
    r64, r32 = refs[F64], refs[F32]
    names = S.figure_names(c)
    for name, t in zip(names, r64):
        if t is None:
            assert c.kind == 'afm' and not c.bias and name == 'dba'
            continue
        assert bool(torch.isfinite(t).all()), name
        if name not in ZERO_OK.get(c.data, ()):
            assert float(t.abs().max()) > 0.0, f'{name} of {c.id} is zero everywhere: nothing to measure'
    for t in inputs + [up]:
        assert t is None or torch.equal(t, t.float().double())                   # float32 holds every input exactly
    # float32 in another summation order, held to the GPU's bar
    perm = torch.randperm(c.B, generator=torch.Generator().manual_seed(c.B))
    r32p = S.run_reference(c, inputs, up, F32, perm=perm)
    figs = S.figures(c, r32p, r64, r32, scales)
    ratios = {k: g / max(f, P.FLOOR) for k, (_, g, f) in figs.items()}
    assert all(v <= P.STEP_BAR['fp32'] for v in ratios.values()), (c.id, ratios)
    # what the hard inputs are meant to be
    if c.data == 'zero_field':
        zp = S.pairs_with(c.F, S.ZERO_FIELD)
        assert len(zp) == c.F - 1 and not bool(r64[0][:, zp].any()) and bool(r64[0].any())
    if c.data == 'zero_rows':
        rows = S.ZERO_ROWS(c.B)
        assert not bool(r64[1][rows].any()) and bool(r64[1].any())
    if c.kind == 'afm':
        logits, pre, scale = S.afm_logits(c, inputs)
        if c.act == 'relu':                                     # no unit on its kink: precision.py, KINK_TOL
            assert bool((pre.abs() >= P.KINK_TOL['fp32'] * scale).all()), f'{c.id}: a relu unit within fp32 rounding of 0'
        if c.data == 'afm_flat':
            assert not bool(logits.any())
        if c.data == 'afm_dominant':
            top = logits.sort(dim=1, descending=True).values
            assert float((top[:, 0] - top[:, 1]).min()) >= 100.0
            assert bool((logits.argmax(1) == 0).all())
        if c.data == 'afm_x30':
            assert float(pre.abs().max()) > 100.0
