# -*- coding:utf-8 -*-
"""Host: the case table of tests/cin_support.py against the dispatch arithmetic it restates (an id can never drift from the
shape it names), the restatement against the size and predicate functions of the library (which run without a GPU), and every
GPU case's references against themselves before an input reaches a GPU: the float64 reference is finite and nonzero wherever
the case measures, the float32 CPU reference over a permuted batch stays within the bar the kernel will be held to, the CPU
emulation of the lower classes stays within theirs, and the share of relu units the kink mask removes stays under its cap."""
import itertools

import pytest
import torch

from tests import cin_support as S
from tests import precision as P

F64, F32 = torch.float64, torch.float32
KiB160 = 160 * 1024


# ---- the plans, at the figures the ids and DESIGN.md quote -----------------------------------------------------------------
def test_plans_at_the_quoted_shapes():
    # the exact kernels
    assert S.f32_dgrad(32, 128) == (64, 1) and S.f32_dgrad(33, 128) == (64, 2) and S.f32_dgrad(64, 128) == (64, 2)
    assert S.f32_dgrad(65, 128) == (64, 4) and S.f32_dgrad(128, 129) == (128, 4) and S.f32_dgrad(20, 130) == (128, 1)
    assert S.f32_dgrad(40, 256) == (128, 2)
    assert S.f32_wgrad(70, 3, 40, 256, 10) == (1, 2, 11, 64, 60)
    assert S.f32_wgrad(44, 5, 7, 33, 16) == (1, 1, 11, 64, 64) and (5 * 7 * 33) % 4 == 3
    assert S.f32_wgrad(700, 2, 3, 5, 4) == (1, 1, 44, 64, 48)
    assert S.f32_wgrad(40, 26, 26, 128, 16) == (3, 1, 10, 64, 64)
    assert S.f32_wgrad(3277, 4, 8, 32, 10) == (1, 1, 257, 128, 2)
    assert not S.f32_slabs(3, 5, 6) and S.f32_slabs(3, 40, 256) and not S.f32_slabs(3, 5, 6, ws=False)
    assert S.vec4(12, F0=3, Hk=20) and not S.vec4(10, F0=3, Hk=40) and not S.vec4(4, x0_bs=18, xk_bs=8)
    assert S.f32_fwd_lds(300, 4) == 176640 and S.f32_fwd_lds(299, 4) == 175616 and S.f32_fwd_lds(275, 4) <= KiB160 < S.f32_fwd_lds(276, 4)
    assert S.f32_dgrad_lds(128, 8, 100) == 187408 and S.f32_dgrad_lds(128, 8, 64) <= KiB160
    assert S.cin_nb(128) == 1 and S.cin_nb(1) == 128 and S.cin_nb(12) == 12 and S.cin_nb(100) == 3
    # the bf16 kernels
    assert not S.cinb_wide(32767) and S.cinb_wide(32768) and S.cinb_wide(257 * 128)
    assert [S.cinb_ks(h) for h in (1, 32, 33, 64, 65, 128)] == [2, 2, 4, 4, 8, 8]
    assert S.noz_lds(100, 2, True) == 163840 and S.noz_lds(101, 2, True) == 164864
    assert S.noz_lds(52, 33, True) == 163840 and S.noz_lds(53, 33, True) > KiB160
    assert S.bf16_fwd('bf16x3', 257, 101, 2, 8, 128, 'relu')[0] == 'z'
    assert S.bf16_fwd('bf16x3', 9, 3, 5, 6, 4, 'tanh')[0] == 'z' and S.bf16_fwd('bf16x3', 9, 3, 5, 6, 4, 'relu')[:2] == ('noz4', 2)
    assert S.zform_lds('bf16x3', 128, 100) == 158208 and S.zform_lds('bf16x3', 128, 128) == 170496
    assert S.zform_lds('bf16', 128, 128) == 154112
    assert S.dgrad_lds(8, 2, 8, 63) == 163840 and S.dgrad_lds(8, 2, 8, 64) > KiB160
    assert S.dgrad_lds(8, 2, 4, 125) == 162816 and S.dgrad_lds(8, 2, 4, 126) == 164864
    assert S.dgrad_lds(16, 2, 4, 93) == 162816 and S.dgrad_lds(16, 2, 4, 94) == 164864
    assert S.dgrad_lds(16, 1, 4, 127) == 163840 and S.dgrad_lds(16, 1, 4, 128) == 165888 and S.dgrad_lds(8, 1, 4, 128) <= KiB160
    assert S.bf16_dgrad('bf16x3', 257, 63, 2, 8, 128)[:3] == (8, 1, 8) and S.bf16_dgrad('bf16x3', 257, 64, 2, 8, 128)[:3] == (8, 1, 4)
    assert S.bf16_dgrad('bf16x3', 2049, 4, 8, 129, 16)[:3] == (16, 1, 4) and S.bf16_dgrad('bf16', 2049, 4, 65, 40, 16)[:3] == (8, 4, 4)
    assert S.bf16_wgrad('bf16x3', 257, 3, 5, 33, 128) == ('wide', 1, 1, 1, 172, 192, 64)
    assert S.bf16_wgrad('bf16', 40, 26, 26, 128, 16) == ('wide', 1, 22, 2, 10, 64, 64)
    assert S.bf16_wgrad('bf16', 9, 90, 6, 40, 4)[0] == 'wide' and S.bf16_wgrad('bf16', 9, 91, 6, 40, 4)[0] == 'tile'
    assert S.bf16_wgrad('bf16', 9, 90, 6, 40, 4, xk_bs=6 * 4 + 2)[0] == 'tile'
    assert S.bf16_wgrad('bf16x3', 3277, 4, 8, 32, 10) == ('tile', 1, 1, 257, 128, 2)
    assert S.pool_grid(8200, 130, 2) == (4096, 2) and S.pool_grid(8192, 130, 2) == (4096, 1)


@pytest.mark.parametrize('mode,F0,Hk,L,D,what,lds', S.FORWARD_ONLY)
def test_forward_only_shapes(mode, F0, Hk, L, D, what, lds):
    """DESIGN.md's table: the forward launches at any batch, the backward refuses and for this reason"""
    for B in (1, 40000):
        assert S.fwd_launches(mode, B, F0, Hk, L, D, 'relu')
        assert S.bwd_refusal(mode, B, F0, Hk, L, D) == what
    if lds is not None:
        assert (S.f32_dgrad_lds(Hk, L, D) if mode == 'float32' else S.bf16_dgrad(mode, 1, F0, Hk, L, D)[3]) == lds > KiB160


def test_refused_and_both_run_shapes():
    for mode, F0, Hk, L, D, what, lds in S.REFUSED:
        assert not S.fwd_launches(mode, 1, F0, Hk, L, D, 'relu'), (mode, F0, Hk, L, D)
        if lds is not None:
            assert lds == (S.f32_fwd_lds(F0, Hk) if mode == 'float32' else S.bf16_fwd(mode, 1, F0, Hk, L, D, 'relu')[2])
    for mode, F0, Hk, L, D in S.BOTH_RUN:
        assert S.fwd_launches(mode, 2, F0, Hk, L, D, 'relu') and S.bwd_refusal(mode, 2, F0, Hk, L, D) is None, (mode, F0, Hk, L, D)
    # the shape an xDeepFM with 100 fields and CIN width 200 asks of the default mode
    assert S.fwd_launches('bf16x3', 4096, 100, 100, 200, 16, 'relu') and S.bwd_refusal('bf16x3', 4096, 100, 100, 200, 16) == 'LDS'


# ---- the restatement against the library -----------------------------------------------------------------------------------
GRID = list(itertools.product((1, 3, 26, 52, 53, 100, 101, 128, 129, 276, 300), (1, 5, 32, 33, 64, 65, 100, 128, 129),
                              (1, 6, 128, 129, 256, 257, 300), (1, 4, 10, 16, 128, 129, 132)))


def test_sizes_and_predicates_equal_the_library():
    from deeptables_amd import _lib
    lib = _lib.lib()
    codes = {'relu': 1, 'linear': 0, 'tanh': 3}
    for F0, Hk, L, D in GRID:
        for B in (1, 9, 70, 700, 3277):
            kb, nb, splits, rps, last = S.f32_wgrad(B, F0, Hk, L, D)
            assert lib.dt_cin_bwd_workspace_bytes(B, F0, Hk, L, D) == splits * F0 * Hk * L * 4 == S.f32_bwd_workspace_bytes(B, F0, Hk, L, D)
            assert 0 < last <= rps and rps % 64 == 0 and (splits - 1) * rps + last == B * D
        assert lib.dt_cin_bf16_workspace_bytes(F0, Hk, L) == S.bf16_workspace_bytes('bf16', F0, Hk, L)
        assert lib.dt_cin_bf16x3_workspace_bytes(F0, Hk, L) == S.bf16_workspace_bytes('bf16x3', F0, Hk, L)
        for mode in S.MODES:
            assert lib.dt_cin_packed_bytes(S.MODE_CODE[mode], F0, Hk, L) == S.packed_bytes(mode, F0, Hk, L)
            for act, code in codes.items():
                want = {S.fwd_launches(mode, B, F0, Hk, L, D, act) for B in (1, 40000)}
                assert len(want) == 1, f'{mode} {F0, Hk, L, D, act}: the narrow and the wide batch disagree'
                assert bool(lib.dt_cin_fwd_supported(S.MODE_CODE[mode], F0, Hk, L, D, code)) == want.pop(), (mode, F0, Hk, L, D, act)
    assert lib.dt_cin_bwd_workspace_bytes(0, 3, 3, 3, 3) == 0 and lib.dt_cin_bf16_workspace_bytes(0, 3, 3) == 0
    assert lib.dt_cin_packed_bytes(0, 0, 3, 3) == -1 and lib.dt_cin_fwd_supported(7, 3, 3, 3, 3, 0) == 0


# ---- case hygiene ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', S.params_of(S.PATH_CASES + S.ACT_CASES))
def test_case_takes_the_path_its_id_names(c):
    if c in S.PATH_CASES:
        assert c.expect, 'a path case states what it expects of the plans'
    plans = {m: S.plan(c, m) for m in S.MODES}
    for key, want in c.expect.items():
        mode, k = key.split(':')
        assert mode in c.modes or mode == 'bf16', key
        assert plans[mode][k] == want, (c.id, key, plans[mode][k], want)


@pytest.mark.parametrize('c', S.params_of(S.ALL_CASES))
def test_case_launches_inside_every_bound(c):
    for mode in c.modes:
        assert S.fwd_launches(mode, c.B, c.F0, c.Hk, c.L, c.D, c.act) and S.bwd_refusal(mode, c.B, c.F0, c.Hk, c.L, c.D) is None
        for kern, lds in S.lds_requests(c, mode).items():
            assert lds <= KiB160, (c.id, mode, kern, lds)
    assert c.B * c.L * c.D < 2 ** 31 and c.B * max(c.F0, c.Hk) * c.D < 2 ** 31


def test_the_table_covers_the_listed_paths():
    shapes = {(c.B, c.F0, c.Hk, c.L, c.D) for c in S.PATH_CASES}
    assert shapes >= {(9, 3, 5, 6, 3), (9, 3, 32, 128, 8), (9, 3, 33, 129, 8), (9, 2, 64, 36, 4), (9, 2, 65, 40, 8), (5, 2, 128, 256, 4),
                      (9, 3, 20, 130, 12), (70, 3, 40, 256, 10), (44, 5, 7, 33, 16), (700, 2, 3, 5, 4), (40, 26, 26, 128, 16),
                      (1, 4, 4, 8, 128), (11, 7, 9, 5, 1), (9, 26, 40, 8, 4), (9, 90, 6, 40, 4), (9, 91, 6, 40, 4), (257, 3, 5, 33, 128),
                      (2049, 4, 33, 40, 16), (2049, 4, 65, 40, 16), (2049, 4, 8, 129, 16), (3277, 4, 8, 32, 10), (257, 100, 2, 8, 128),
                      (257, 101, 2, 8, 128), (257, 63, 2, 8, 128), (257, 64, 2, 8, 128), (257, 52, 33, 8, 128)}
    assert all(c.modes == S.MODES for c in S.PATH_CASES if (c.B, c.F0, c.Hk) != (257, 52, 33))
    # every instantiation of the three dgrad families, every forward kernel at both block sizes, both weight-gradient kernels
    plans = [(m, S.plan(c, m)) for c in S.PATH_CASES for m in c.modes]
    assert {p['dgrad'] for m, p in plans if m == 'float32'} == {(lh, jb) for lh in (64, 128) for jb in (1, 2, 4)}
    for mode in ('bf16x3', 'bf16'):
        got = {p['dgrad'] for m, p in plans if m == mode}
        assert got == {(ls, jb, 4) for ls in (8, 16) for jb in (1, 2, 4)} | {(8, 1, 8), (8, 2, 8)}, (mode, got)
        assert {p['wgrad_kind'] for m, p in plans if m == mode} == {'wide', 'tile'}
        assert {p['wgrad'][1] for m, p in plans if m == mode and p['wgrad_kind'] == 'wide'} == {1, 2}        # k groups: sub1 < nsub in the first
    x3 = [p for m, p in plans if m == 'bf16x3']
    assert {p['fwd'] for p in x3} == {('noz4', 2), ('noz4', 4), ('noz8', 2), ('noz8', 4), ('z',)}
    assert any(p['fwd'] == ('z',) and p['wide'] for p in x3) and any(p['fwd'][0] == 'noz8' and p['filter_tiles'] == 2 for p in x3)
    assert {p['reduce_tail'] != 0 for m, p in plans if m == 'float32' and p['slabs'] and p['splits'] > 8} == {True}
    assert {a for c in S.ACT_CASES for a in [c.act]} == set(S.SMOOTH_ACTS) | {'linear'}
    assert {c.data for c in S.HARD_CASES} == {'logspace', 'zero_field', 'zero_rows', 'zero_xk', 'cancel', 'relu_dead', 'relu_alive',
                                              'x30', 'one_hot'}
    assert all(c.modes == S.HARD_MODES for c in S.HARD_CASES)
    assert S.pool_grid(*[S.POOL_CASES[0][i] for i in (0, 1, 3)])[1] == 2


# ---- the references alone --------------------------------------------------------------------------------------------------
MASK_CAP = {'fp32': 0.005, 'bf16': 0.20}


def _classes(c):
    return sorted({S.fwd_class(m) for m in c.modes}) if c.act in S.KINKED else ['fp32']


@pytest.mark.parametrize('c', S.params_of(S.ALL_CASES + S.LIMIT_CASES))
def test_references_are_fit_to_measure_against(c):
    for cls in _classes(c):
        ref = S.references(c, cls)
        for name, t in zip(S.FIGURES, ref.r64):
            if t is None:
                assert name == 'db' and not c.bias
                continue
            assert bool(torch.isfinite(t).all()), name
            if name not in S.ZERO_OK.get(c.data, ()):
                assert float(t.abs().max()) > 0.0, f'{name} of {c.id} is zero everywhere: nothing to measure'
        for t in ref.inputs + [ref.up]:
            assert t is None or torch.equal(t, t.float().double())              # float32 holds every input exactly
        # the kink mask's share is a cap, not a figure (the b17 class shares the fp32 forward: the same mask)
        assert ref.masked <= MASK_CAP[cls], f'{c.id}: the {cls} kink mask removes {ref.masked:.4f} of the units'
        # float32 in another summation order, held to the bar of the fp32-class kernels
        perm = torch.randperm(c.B, generator=torch.Generator().manual_seed(c.B))
        r32p = S.run_reference(c, ref.inputs, ref.up, F32, perm=perm)
        S.check('host:f32_permuted', c, 'float32', r32p, ref, record=False)
    # what the hard inputs are meant to be
    ref = S.references(c)
    if c.data == 'zero_field':
        assert bool(ref.r64[1][:, S.ZERO_FIELD].any())                            # the zero field's own gradient is not zero
        assert not bool(ref.r64[3].reshape(c.F0, c.Hk, c.L)[S.ZERO_FIELD].any())
    if c.data == 'zero_rows':
        rows = S.ZERO_ROWS(c.B)
        assert not bool(ref.r64[1][rows].any()) and not bool(ref.r64[2][rows].any()) and bool(ref.r64[1].any())
    if c.data == 'cancel':
        assert float((ref.pre.abs() / ref.s_fwd).max()) <= 2.0 ** -10
    if c.data == 'relu_dead':
        assert bool((ref.pre < 0).all())
    if c.data == 'relu_alive':
        assert bool((ref.pre > 0).all())
    if c.data == 'x30':
        assert float((ref.pre.abs() > 5).double().mean()) > 0.3
    if c.data == 'one_hot':
        b, l, d = S.ONE_HOT
        keep = torch.zeros(c.B, c.D, dtype=torch.bool)
        keep[b, d] = True
        for g in ref.r64[1:3]:
            assert not bool(g.permute(0, 2, 1)[~keep].any()) and bool(g[b, :, d].all())


# every case but the one large reference, (257, 52, 33, 8, 128): its Z alone is 56 M elements per bf16 part
EMULATED = [c for c in S.ALL_CASES if c.B * c.D * c.F0 * c.Hk <= 2 ** 24]
assert len(EMULATED) == len(S.ALL_CASES) - 1


@pytest.mark.parametrize('c,mode', S.mode_params([c for c in EMULATED if set(c.modes) & {'bf16x3', 'bf16'}]))
def test_lower_class_emulation_stays_within_its_bars(c, mode):
    """two bf16 parts and three products (the bf16x3 backward), one bf16 product (bf16): the bars the kernels of these classes
    are held to hold for the arithmetic the classes are named after, on the same inputs; the headroom is printed"""
    if mode == 'float32':
        return
    ref = S.references(c, S.fwd_class(mode))
    emu = S.emulate(c, ref, mode)
    errs = S.errors(emu, ref)
    room = {}
    for name, (ec, rms) in errs.items():
        cls = S.figure_class(mode, name)
        if cls == 'fp32':
            continue
        room[name] = (P.KINK_TOL[cls] / max(ec, 1e-300), P.COND_BAR[cls] / max(rms, 1e-300))
        assert ec <= P.KINK_TOL[cls] and rms <= P.COND_BAR[cls], (c.id, mode, name, ec, rms)
    print(f'{mode} {c.id}: headroom (elem_cond, cond_rms) ' + ' '.join(f'{k}={a:.1f}x/{b:.1f}x' for k, (a, b) in room.items()))
