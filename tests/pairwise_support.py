# -*- coding:utf-8 -*-
"""Host side of the pairwise-interaction kernel tests (csrc/product.hip, the AFM and bilinear halves of csrc/interaction.hip):
the dispatch arithmetic of the launchers restated in plain Python, the table of cases with the path each id names, input
builders and the float64 / float32 CPU references.  Nothing here needs a GPU; tests/test_pairwise_paths_host.py checks the
table against the plans and the references against themselves, tests/test_pairwise_kernels_gpu.py runs the kernels."""
import collections
import math
import zlib

import torch

from tests import precision as P

F64, F32 = torch.float64, torch.float32


def ceil_div(a, b):
    return -(-a // b)


def n_pairs(F):
    return F * (F - 1) // 2


# ---- the launchers' arithmetic ---------------------------------------------------------------------------------------------
def op16_plan(B):
    """(ntiles, splits, tiles_per_split) of k_op16_fwd / k_op16_bwd_k / k_bil16_fwd / k_bil16_bwd_w: product.hip:502-505 and
    539-542, interaction.hip:755-758 and 782-785"""
    ntiles = ceil_div(B, 16)
    splits = 8 if ntiles >= 64 else 1
    tps = ceil_div(ntiles, splits)
    return ntiles, ceil_div(ntiles, tps), tps


def generic_wgrad_plan(B):
    """(splits, rows_per_split) of k_op_mat_bwd_k / k_bilinear_bwd_w: product.hip:550-553, interaction.hip:795-798"""
    splits = min(ceil_div(B, 1024), 16)
    rps = ceil_div(ceil_div(B, splits), 64) * 64
    return ceil_div(B, rps), rps


def wgrad_accumulators(D):
    """how many of acc[0..15] a thread of k_op_mat_bwd_k / k_bilinear_bwd_w uses: outputs t = tid + 256 k < D * D
    (product.hip:240-250, interaction.hip:430-440)"""
    return ceil_div(D * D, 256)


def pair_grid(B, has_param_grad, fwd):
    """(blocks, rows the busiest wave walks) of k_pair_dot_fwd / k_pair_dot_bwd: row_grid(B, 4 waves, cap) with the cap 2048,
    or 256 for a backward that accumulates a kernel gradient in LDS (product.hip:263-267, 456, 468)"""
    cap = 2048 if (fwd or not has_param_grad) else 256
    blocks = max(1, min(ceil_div(B, 4), cap))
    return blocks, ceil_div(B, 4 * blocks)


def afm_grid(B, fwd):
    """(blocks, rows the busiest block walks) of k_afm_fwd / k_afm_bwd (interaction.hip:710, 734)"""
    blocks = min(B, 2048 if fwd else 512)
    return blocks, ceil_div(B, blocks)


def afm_hmax(H):
    """the HMAX instantiation (interaction.hip:691)"""
    return 16 if H <= 16 else (32 if H <= 32 else 64)


def afm_blocked(D, H):
    """whether k_afm_bwd forms grad_Wa in 4x4 register blocks (interaction.hip:198-199)"""
    dp4 = (D + 3) & ~3
    return D % 4 == 0 and (dp4 // 4) * (afm_hmax(H) // 4) <= 256


def mfma_bwd(F, D):
    """whether the backward of outer 'mat' / bilinear runs on the D = 16 MFMA kernels (product.hip:534, interaction.hip:777)"""
    return D == 16 and 4 * 16 * F * 16 * 4 + F * F * 2 <= 150 * 1024


def op16_wave_ranges(F):
    """the pair range [begin, end) of each of the four waves of k_*16_bwd_x (product.hip:374, interaction.hip:562)"""
    Pn = n_pairs(F)
    return [(Pn * w // 4, Pn * (w + 1) // 4) for w in range(4)]


def pair_fields(F):
    return [(i, j) for i in range(F - 1) for j in range(i + 1, F)]


# dynamic LDS in bytes
def lds_pair_fwd(F, D):                                                     # product.hip:454
    return 4 * F * (D + 1) * 4 + 2 * n_pairs(F) * 2 + 16


def lds_pair_bwd(F, D, kind):                                               # product.hip:465-466
    nk = {'inner': 0, 'outer_vec': n_pairs(F) * D, 'outer_num': n_pairs(F)}[kind]
    return (4 * (F * D + n_pairs(F)) + nk) * 4


def lds_generic_fwd(D):                                                     # product.hip:509, 530; interaction.hip:763
    return (D * D + 2 * 64 * (D + 1)) * 4


def lds_bilinear_bwd_x(D):                                                  # interaction.hip:790
    return (D * D + 3 * 64 * (D + 1)) * 4


def lds_generic_wgrad(D):                                                   # product.hip:555, interaction.hip:799
    return 2 * 64 * D * 4


def lds16_bwd_x(F):                                                         # product.hip:535, interaction.hip:778
    return 4 * 16 * F * 16 * 4 + F * (F - 1) * 2 + 16


def afm_lds_fwd(F, D, H):                                                   # interaction.hip:692-695
    Pn, HM = n_pairs(F), afm_hmax(H)
    return (D * HM + 2 * HM + 64 + 8 + F * D + Pn) * 4 + 2 * Pn * 2 + 16


def afm_lds_bwd(F, D, H):                                                   # interaction.hip:696-700
    Pn, HM, dp4 = n_pairs(F), afm_hmax(H), (D + 3) & ~3
    return (2 * D * HM + 4 * HM + Pn * HM + 2 * Pn * dp4 + 8 + F * D + D) * 4 + 2 * Pn * 2 + 16


# ---- the operations --------------------------------------------------------------------------------------------------------
PAIR_KINDS = ('inner', 'outer_vec', 'outer_num')
MAT_KINDS = ('outer_mat', 'bil_field_interaction', 'bil_field_each', 'bil_field_all')
KERNEL_OF = {'inner': 'inner', 'outer_vec': 'outer', 'outer_num': 'outer', 'outer_mat': 'outer', 'afm': 'afm',
             'bil_field_interaction': 'bilinear', 'bil_field_each': 'bilinear', 'bil_field_all': 'bilinear'}

Case = collections.namedtuple('Case', 'id kind B F D H act bias data metric expect seed')


def case(id, kind, B, F, D, H=None, act=None, bias=True, data='mild', metric='rel', expect=None, seed=0):
    return Case(f'{kind}-{id}', kind, B, F, D, H, act, bias, data, metric, expect or {}, seed)


def figure_names(c):
    return {'inner': ['out', 'dx'], 'afm': ['out', 'dx', 'dWa', 'dba', 'dpv']}.get(
        c.kind, ['out', 'dx', 'dW' if c.kind.startswith('bil') else 'dk'])


def param_shapes(c):
    """[(shape, scale of the randn data) | None] of the parameters after x"""
    Pn, D, F = n_pairs(c.F), c.D, c.F
    if c.kind == 'inner':
        return []
    if c.kind.startswith('outer'):
        return [({'outer_mat': (D, Pn, D), 'outer_vec': (Pn, D), 'outer_num': (Pn, 1)}[c.kind], 0.3)]
    if c.kind.startswith('bil'):
        nW = {'bil_field_interaction': Pn, 'bil_field_each': F - 1, 'bil_field_all': 1}[c.kind]
        return [((nW, D, D), 1.0 / math.sqrt(D))]
    return [((D, c.H), 1.0 / math.sqrt(D)), ((c.H,), 0.1) if c.bias else None, ((c.H, 1), 0.5)]


def out_shape(c):
    Pn = n_pairs(c.F)
    return {'afm': (c.B, c.D)}.get(c.kind, (c.B, Pn, c.D) if c.kind.startswith('bil') else (c.B, Pn))


def ref_fn(c):
    """the float restatement of oracle/reference_layers.py as fn(x, *params); AFM with an identity out_kernel"""
    from oracle import reference_layers as R
    fields = lambda t: [t[:, i:i + 1] for i in range(c.F)]
    if c.kind == 'inner':
        return lambda x: R.inner_product(fields(x))
    if c.kind.startswith('outer'):
        return lambda x, k: R.outer_product(fields(x), k, c.kind[6:])
    if c.kind.startswith('bil'):
        return lambda x, W: R.bilinear_interaction(x, list(W), c.kind[4:])
    return lambda x, Wa, ba, pv: R.afm(fields(x), Wa, ba, pv, torch.eye(c.D, dtype=x.dtype), c.act)


def gpu_fn(c):
    from deeptables_amd import ops
    if c.kind == 'inner':
        return ops.inner_product
    if c.kind.startswith('outer'):
        return lambda x, k: ops.outer_product(x, k, c.kind[6:])
    if c.kind.startswith('bil'):
        return lambda x, W: ops.bilinear_interaction(x, W, c.kind[4:])
    return lambda x, Wa, ba, pv: ops.afm_pool(x, Wa, ba, pv, c.act)


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def rnd(g, shape, scale=1.0):
    """float64 values that float32 holds exactly: the kernel and the reference see the same inputs"""
    return (torch.randn(shape, generator=g, dtype=F64) * scale).float().double()


ZERO_FIELD = 1                # the field the 'zero_field' data zeroes


def ZERO_ROWS(B):
    """the rows whose upstream gradient the 'zero_rows' data zeroes"""
    return sorted({0, B // 2, B - 1})


def pairs_with(F, f):
    return [p for p, (i, j) in enumerate(pair_fields(F)) if f in (i, j)]


def build_inputs(c):
    """-> ([x, *params] float64 (None for an absent AFM bias), upstream gradient float64)"""
    g = torch.Generator().manual_seed(zlib.crc32(c.id.encode()) + c.seed)
    B, F, D = c.B, c.F, c.D
    x = rnd(g, (B, F, D))
    params = [None if s is None else rnd(g, s[0], s[1]) for s in param_shapes(c)]
    up = rnd(g, out_shape(c))
    if c.data == 'logspace':                                    # field magnitudes 1e-3 .. 1e3
        x = (x * torch.logspace(-3, 3, F, dtype=F64)[None, :, None]).float().double()
    elif c.data == 'zero_field':
        x[:, ZERO_FIELD] = 0.0
    elif c.data == 'zero_rows':
        up[ZERO_ROWS(B)] = 0.0
    elif c.data == 'cancel':                                    # x_1 = -x_0, and pairs (0,2), (1,2) with the same upstream
        x[:, 1] = -x[:, 0]
        if F > 2:
            pf = pair_fields(F)
            up[:, pf.index((1, 2))] = up[:, pf.index((0, 2))]
    elif c.data == 'afm_flat':                                  # pv = 0: every logit 0, every score 1 / P
        params[2] = torch.zeros_like(params[2])
    elif c.data == 'afm_dominant':                              # pair (0, 1) aligned with Wa pv and large, the rest small
        w = (params[0] @ params[2]).reshape(-1)
        x = (x * 0.01).float().double()
        x[:, 0] = (10.0 * torch.sign(w) * (1.0 + x[:, 0].abs())).float().double()
        x[:, 1] = (10.0 * (1.0 + x[:, 1].abs())).float().double()
    elif c.data == 'afm_x30':
        x = (x * 30.0).float().double()
    else:
        assert c.data == 'mild', c.data
    return [x] + params, up


def afm_logits(c, inputs, dt=F64):
    """[B, P] attention logits and the pre-activations [B, P, H] with their |A| |B| scale, in float64"""
    from oracle import reference_layers as R
    x, Wa, ba, pv = [None if t is None else t.to(dt) for t in inputs]
    pf = pair_fields(c.F)
    bi = x[:, [i for i, _ in pf]] * x[:, [j for _, j in pf]]
    pre = bi @ Wa + (0 if ba is None else ba)
    scale = bi.abs() @ Wa.abs() + (0 if ba is None else ba.abs())
    return (R._activation(c.act)(pre) @ pv).squeeze(-1), pre, scale


def run_reference(c, inputs, up, dt, perm=None):
    """[out, dx, dparam ...] of the CPU reference in `dt`; with `perm` the batch is walked in that order (another summation
    order for the parameter gradients) and out / dx are put back in the caller's order"""
    xs = [None if t is None else t.to(dt).clone() for t in inputs]
    u = up.to(dt)
    if perm is not None:
        xs[0], u = xs[0][perm].clone(), u[perm]
    xs = [None if t is None else t.requires_grad_(True) for t in xs]
    out = ref_fn(c)(*xs)
    (out * u).sum().backward()
    res = [out.detach()] + [None if t is None else t.grad for t in xs]
    if perm is not None:
        inv = torch.argsort(perm)
        res[0], res[1] = res[0][inv], res[1][inv]
    return res


_CACHE = {}


def references(c):
    """inputs, upstream gradient, {dtype: [out, dx, dparam ...]} and (for metric 'cond') the |A| |B| scale of every figure;
    computed once per case and shared, never written to"""
    if c.id not in _CACHE:
        inputs, up = build_inputs(c)
        refs = {dt: run_reference(c, inputs, up, dt) for dt in (F64, F32)}
        scales = None
        if c.metric == 'cond':
            assert c.kind != 'afm'                            # sums and products only
            s_out, s_in = P.abs_scale(ref_fn(c), inputs, up)
            scales = [s_out] + s_in
        _CACHE[c.id] = (inputs, up, refs, scales)
    return _CACHE[c.id]


def figures(c, got, r64, r32, scales=None):
    """{name: (direction, err of `got`, err of the float32 reference)} in the case's metric"""
    figs = {}
    for k, (name, a, e64, e32) in enumerate(zip(figure_names(c), got, r64, r32)):
        if e64 is None:
            assert a is None, name
            continue
        assert a.shape == e64.shape, (name, a.shape, e64.shape)
        assert bool(torch.isfinite(a).all()), name
        if c.metric == 'cond':
            figs[name] = ('fwd' if k == 0 else 'bwd', P.elem_cond(a, e64, scales[k]), P.elem_cond(e32, e64, scales[k]))
        else:
            m = P.row_rel if e64.dim() >= 2 else P.max_rel
            figs[name] = ('fwd' if k == 0 else 'bwd', m(a, e64), m(e32, e64))
    return figs


def run_gpu(c, inputs, up, dev):
    """[out, dx, dparam ...] of the HIP op on float32 copies of the inputs"""
    xs = [None if t is None else t.float().to(dev).requires_grad_(True) for t in inputs]
    out = gpu_fn(c)(*xs)
    assert out.shape == tuple(out_shape(c)) and out.dtype == F32
    out.backward(up.float().to(dev))
    return [out.detach()] + [None if t is None else t.grad for t in xs]


def check_case(test, c, dev):
    """the runner: float64 and float32 CPU references and the GPU op on the same inputs, every figure within
    STEP_BAR x max(error of the float32 reference, 2^-24) through precision.check_step -> (got, float64 reference)"""
    inputs, up, refs, scales = references(c)
    got = run_gpu(c, inputs, up, dev)
    P.check_step(f'{test}[{c.id}]', KERNEL_OF[c.kind], 'float32', figures(c, got, refs[F64], refs[F32], scales))
    return got, refs[F64]


# ---- the cases -------------------------------------------------------------------------------------------------------------
def _path_cases():
    cs = []
    for kind in PAIR_KINDS:
        par = kind != 'inner'
        cs += [case('B1-F2-D1-one_pair_one_lane', kind, 1, 2, 1, expect={'pair_fwd': (1, 1), 'pair_bwd': (1, 1)}),
               case('B5-F2-D4-two_blocks', kind, 5, 2, 4, expect={'pair_fwd': (2, 1), 'pair_bwd': (2, 1)}),
               case('B7-F12-D3-P66_second_lane_pass', kind, 7, 12, 3, expect={'pairs': 66}),
               case('B9-F3-D70-FD210_four_staging_passes', kind, 9, 3, 70, expect={'fd': 210}),
               case('B8193-F3-D2-fwd_2048_blocks_second_row' + ('-bwd_256_blocks_9_rows' if par else '-bwd_second_row'),
                    kind, 8193, 3, 2, expect={'pair_fwd': (2048, 2), 'pair_bwd': (256, 9) if par else (2048, 2)})]
        if par:
            cs.append(case('B1025-F3-D4-bwd_256_block_cap_second_row', kind, 1025, 3, 4,
                           expect={'pair_fwd': (257, 1), 'pair_bwd': (256, 2)}))
    for kind in MAT_KINDS:
        cs += [case('B63-F3-D5-generic-one_partial_tile', kind, 63, 3, 5, expect={'wgrad': (1, 64), 'nacc': 1, 'mfma': False}),
               case('B64-F3-D5-generic-one_full_tile', kind, 64, 3, 5, expect={'wgrad': (1, 64), 'nacc': 1}),
               case('B65-F3-D5-generic-second_tile_one_row', kind, 65, 3, 5, expect={'wgrad': (1, 128), 'nacc': 1}),
               case('B9-F3-D17-generic-acc1', kind, 9, 3, 17, expect={'nacc': 2, 'mfma': False}),
               case('B9-F3-D33-generic-acc4', kind, 9, 3, 33, expect={'nacc': 5}),
               case('B65-F3-D63-generic-16_accumulators-bwd_x_65028_B_last_under_64KiB', kind, 65, 3, 63, expect={'nacc': 16, 'bil_lds': 65028}),
               case('B65-F3-D64-generic-16_accumulators-bwd_x_66304_B', kind, 65, 3, 64, expect={'nacc': 16, 'bil_lds': 66304}),
               case('B1025-F3-D5-generic-2_splits_of_576_last_449', kind, 1025, 3, 5, expect={'wgrad': (2, 576), 'last': 449}),
               case('B16385-F2-D3-generic-16_splits_of_1088_last_65', kind, 16385, 2, 3,
                    expect={'wgrad': (16, 1088), 'last': 65}),
               case('B17-F37-D16-fwd_mfma-bwd_generic', kind, 17, 37, 16, expect={'mfma': False, 'op16': (2, 1, 2)})]
        cs += [case(f'B{B}-F3-D16-mfma', kind, B, 3, 16, expect={'mfma': True, 'op16': (ceil_div(B, 16), 1, ceil_div(B, 16))})
               for B in (1, 15, 16, 17, 65)]
        cs += [case('B17-F2-D16-mfma-P1_three_idle_waves', kind, 17, 2, 16, expect={'mfma': True, 'pairs': 1, 'idle_waves': 3}),
               case('B17-F5-D16-mfma-dxi_flushed_in_mid_range', kind, 17, 5, 16, expect={'mfma': True, 'flush': True}),
               case('B17-F36-D16-mfma-largest_F_149992_B', kind, 17, 36, 16, expect={'mfma': True, 'lds16': 149992}),
               case('B1009-F3-D16-mfma-64_tiles_8_splits_of_8', kind, 1009, 3, 16, expect={'mfma': True, 'op16': (64, 8, 8)}),
               case('B1040-F3-D16-mfma-65_tiles_8_splits_of_9_last_2', kind, 1040, 3, 16,
                    expect={'mfma': True, 'op16': (65, 8, 9), 'last_tiles': 2})]
    return cs


def _afm_cases():
    cs = []
    for act in ('relu', 'tanh'):
        cs += [case(f'B9-F4-D8-H{H}-{act}-hmax{afm_hmax(H)}', 'afm', 9, 4, 8, H, act,
                    expect={'hmax': afm_hmax(H), 'blocked': True}) for H in (1, 16, 17, 32, 33, 64)]
    cs += [case('B9-F4-D6-H8-relu-unblocked_DP4_8', 'afm', 9, 4, 6, 8, 'relu', expect={'hmax': 16, 'blocked': False}),
           case('B9-F4-D33-H8-relu-unblocked-three_pooled_passes', 'afm', 9, 4, 33, 8, 'relu',
                expect={'blocked': False, 'pooled_passes': 3}),
           case('B3-F3-D68-H33-tanh-unblocked_nblk272', 'afm', 3, 3, 68, 33, 'tanh',
                expect={'hmax': 64, 'blocked': False, 'nblk': 272}),
           case('B513-F3-D6-H8-relu-unblocked-bwd_block0_two_rows', 'afm', 513, 3, 6, 8, 'relu',
                expect={'blocked': False, 'afm_bwd': (512, 2), 'afm_fwd': (513, 1)}),
           case('B2049-F3-D4-H8-relu-fwd_second_row-bwd_5_rows', 'afm', 2049, 3, 4, 8, 'relu',
                expect={'blocked': True, 'afm_fwd': (2048, 2), 'afm_bwd': (512, 5)}),
           case('B9-F24-D8-H8-relu-P276_second_thread_pass', 'afm', 9, 24, 8, 8, 'relu', expect={'pairs': 276}),
           case('B9-F3-D8-H8-tanh-P3_three_waves_minus_inf', 'afm', 9, 3, 8, 8, 'tanh', expect={'pairs': 3}),
           case('B9-F4-D8-H8-relu-no_bias', 'afm', 9, 4, 8, 8, 'relu', bias=False, expect={'blocked': True}),
           case('B9-F4-D6-H8-tanh-no_bias-unblocked', 'afm', 9, 4, 6, 8, 'tanh', bias=False, expect={'blocked': False})]
    return cs


HARD_DATA = ('logspace', 'zero_field', 'zero_rows', 'cancel')
HARD_SHAPES = [('outer_mat', 65, 3, 5), ('outer_mat', 17, 3, 16), ('bil_field_interaction', 65, 3, 5),
               ('bil_field_interaction', 17, 3, 16), ('bil_field_each', 65, 3, 5), ('bil_field_each', 17, 3, 16),
               ('bil_field_all', 65, 3, 5), ('bil_field_all', 17, 3, 16), ('outer_vec', 9, 4, 6), ('inner', 9, 4, 6)]


def _hard_cases():
    cs = [case(f'B{B}-F{F}-D{D}-{data}', kind, B, F, D, data=data,
               metric='cond' if data in ('logspace', 'cancel') else 'rel')
          for data in HARD_DATA for kind, B, F, D in HARD_SHAPES]
    cs += [case('B9-F4-D8-H8-tanh-flat_softmax', 'afm', 9, 4, 8, 8, 'tanh', data='afm_flat'),
           case('B9-F4-D6-H8-linear-flat_softmax-unblocked', 'afm', 9, 4, 6, 8, 'linear', data='afm_flat'),
           case('B9-F4-D8-H8-linear-dominant_pair', 'afm', 9, 4, 8, 8, 'linear', data='afm_dominant'),
           case('B9-F4-D8-H8-tanh-x30', 'afm', 9, 4, 8, 8, 'tanh', data='afm_x30')]
    return cs


PATH_CASES = _path_cases()
AFM_CASES = _afm_cases()
HARD_CASES = _hard_cases()
ALL_CASES = PATH_CASES + AFM_CASES + HARD_CASES
BY_ID = {c.id: c for c in ALL_CASES}
assert len(BY_ID) == len(ALL_CASES)

# the cases the layout and repeatability tests of the GPU module reuse (their references are the shared ones)
LAYOUT_IDS = ['inner-B7-F12-D3-P66_second_lane_pass', 'outer_vec-B7-F12-D3-P66_second_lane_pass',
              'outer_mat-B65-F3-D5-generic-second_tile_one_row', 'outer_mat-B17-F5-D16-mfma-dxi_flushed_in_mid_range',
              'bil_field_each-B65-F3-D5-generic-second_tile_one_row', 'bil_field_each-B17-F5-D16-mfma-dxi_flushed_in_mid_range',
              'afm-B9-F4-D6-H8-relu-unblocked_DP4_8']
REPEAT_IDS = ['inner-B8193-F3-D2-fwd_2048_blocks_second_row-bwd_second_row',
              'outer_vec-B1025-F3-D4-bwd_256_block_cap_second_row',
              'outer_mat-B1025-F3-D5-generic-2_splits_of_576_last_449',
              'outer_mat-B1040-F3-D16-mfma-65_tiles_8_splits_of_9_last_2',
              'bil_field_interaction-B1025-F3-D5-generic-2_splits_of_576_last_449',
              'bil_field_all-B1040-F3-D16-mfma-65_tiles_8_splits_of_9_last_2',
              'afm-B513-F3-D6-H8-relu-unblocked-bwd_block0_two_rows']


def params_of(cases):
    import pytest
    return [pytest.param(c, id=c.id) for c in cases]
