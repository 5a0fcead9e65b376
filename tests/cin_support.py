# -*- coding:utf-8 -*-
"""Host side of the CIN kernel tests (csrc/cin.hip, csrc/cin_bf16.hip): the dispatch arithmetic of the launchers restated in
plain Python, the table of cases with the path each id names, input builders, the float64 / float32 CPU references with their
|A| |B| scales, and a CPU emulation of the two lower precision classes.  Nothing here needs a GPU;
tests/test_cin_paths_host.py checks the table against the plans and the library's size functions and the references against
themselves, tests/test_cin_kernels_gpu.py runs the kernels."""
import collections
import zlib

import numpy as np
import torch

from tests import precision as P

F64, F32 = torch.float64, torch.float32
MODES = ('float32', 'bf16x3', 'bf16')
MODE_CODE = {'float32': 0, 'bf16': 1, 'bf16x3': 2}                      # DT_CIN_F32 / _BF16 / _BF16X3 (include/dt_hip.h)
LDS_MAX = 160 * 1024


def ceil_div(a, b):
    return -(-a // b)


# ---- csrc/cin.hip ----------------------------------------------------------------------------------------------------------
def cin_slab(F, D):                                                       # cin.hip:32-36
    s = F * D
    if D < 32:
        s += ((D - (s % 32)) % 32 + 32) % 32
    return s


def cin_nb(D):                                                            # cin.hip:37-39
    return 128 // D if 128 % D == 0 else 128 // D + 2


def cin_hkp(Hk):                                                          # cin.hip:74
    return (Hk + 3) & ~3


def cin_xks(Hk):                                                          # cin.hip:75-78
    h = cin_hkp(Hk)
    return h if (h >> 2) & 1 else h + 4


def f32_fwd_lds(F0, Hk):                                                  # cin.hip:613 (and :602)
    return (128 * cin_xks(Hk) + 2 * 128 * 20 + 128 * (F0 | 1)) * 4


def f32_fwd_grid(B, L, D):                                                # cin.hip:616
    return ceil_div(B * D, 128), ceil_div(L, 128)


def f32_dgrad(Hk, L):
    """(LH, JB) of the k_cin_dgrad instantiation: cin.hip:703-715"""
    jb = ceil_div(Hk, 32)
    return (64 if L <= 128 else 128), (1 if jb <= 1 else 2 if jb <= 2 else 4)


def f32_dgrad_lds(Hk, L, D):                                              # cin.hip:633
    LH, _ = f32_dgrad(Hk, L)
    return (cin_nb(D) * cin_slab(Hk, D) + 2 * 32 * (2 * LH + 4) + 4) * 4


def _batch_splits(M, blocks, budget):
    """(splits, rows_per_split, rows of the last split): cin.hip:652-656, cin_bf16.hip:1409-1413 and 1420-1424"""
    splits = max(1, budget // blocks)
    rps = ceil_div(ceil_div(M, splits), 64) * 64
    splits = ceil_div(M, rps)
    return splits, rps, M - (splits - 1) * rps


def f32_wgrad(B, F0, Hk, L, D):
    """(kblocks, nblocks, splits, rows_per_split, rows of the last split) of k_cin_wgrad: cin.hip:647-659, 720"""
    kblocks, nblocks = ceil_div(F0 * Hk, 256), ceil_div(L, 128)
    return (kblocks, nblocks) + _batch_splits(B * D, kblocks * nblocks, 512)


def f32_wgrad_lds(F0, Hk):                                                # cin.hip:725
    return 68 * (F0 + Hk + 128) * 4


def f32_slabs(F0, Hk, L, ws=True):
    """whether the batch splits store slabs for k_cin_wgrad_reduce (else: memset + float atomics): cin.hip:723"""
    return bool(ws) and (F0 * Hk * L) % 4 == 0


def vec4(D, x0_bs=None, xk_bs=None, F0=0, Hk=0):
    """the 16-byte staging of the weight-gradient kernels, for 16-byte aligned tensors: cin.hip:388-389, cin_bf16.hip:821-822
    and 1403-1404"""
    x0_bs = F0 * D if x0_bs is None else x0_bs
    xk_bs = Hk * D if xk_bs is None else xk_bs
    return D % 4 == 0 and x0_bs % 4 == 0 and xk_bs % 4 == 0


def f32_bwd_workspace_bytes(B, F0, Hk, L, D):                             # cin.hip:662-665
    if min(B, F0, Hk, L, D) <= 0:
        return 0
    return f32_wgrad(B, F0, Hk, L, D)[2] * F0 * Hk * L * 4


def f32_fwd_launches(F0, Hk, L, D):                                       # cin.hip:595, 614 (cin_f32_fwd_ok, :600-603)
    return min(F0, Hk, L, D) > 0 and D <= 128 and f32_fwd_lds(F0, Hk) <= LDS_MAX


def f32_bwd_refusal(F0, Hk, L, D):
    """None, or the limit dt_cin_layer_bwd names: cin.hip:595, 700-701, 634"""
    if D > 128:
        return 'D'
    if L > 256:
        return 'L'
    if Hk > 128:
        return 'Hk'
    return 'LDS' if f32_dgrad_lds(Hk, L, D) > LDS_MAX else None


# ---- csrc/cin_bf16.hip -----------------------------------------------------------------------------------------------------
NP_FWD = {'bf16x3': 3, 'bf16': 1}
NP_BWD = {'bf16x3': 2, 'bf16': 1}


def cb_hp(Hk):                                                            # cin_bf16.hip:74
    return (Hk + 7) & ~7


def cb_lq(L):                                                             # cin_bf16.hip:75
    return (L + 15) & ~15


def cinb_nT(F0, Hk, L):                                                   # cin_bf16.hip:1158
    return ceil_div(L, 128) * 128 * F0 * cb_hp(Hk)


def cinb_nN(F0, Hk, L):                                                   # cin_bf16.hip:1159
    return F0 * ceil_div(Hk, 32) * 32 * cb_lq(L)


def bf16_workspace_bytes(mode, F0, Hk, L):                                # cin_bf16.hip:1160-1165
    if min(F0, Hk, L) <= 0:
        return 0
    return 2 * (NP_FWD[mode] * cinb_nT(F0, Hk, L) + NP_BWD[mode] * cinb_nN(F0, Hk, L)) + 64


def packed_bytes(mode, F0, Hk, L):                                        # cin_bf16.hip:1283-1291
    if min(F0, Hk, L) <= 0:
        return -1
    n = F0 * Hk * L * 4 if mode == 'float32' else 2 * NP_FWD[mode] * cinb_nT(F0, Hk, L)
    return (n + 15) & ~15


def cinb_wide(M):                                                         # cin_bf16.hip:1175
    return M >= 256 * 128


def cinb_ks(Hk):                                                          # cin_bf16.hip:1204
    return 2 if cb_hp(Hk) <= 32 else 4 if cb_hp(Hk) <= 64 else 8


def noz_lds(F0, Hk, wide):                                                # cin_bf16.hip:1206-1207
    return F0 * (256 if wide else 128) * 4 + (2 if wide else 1) * 3 * 128 * (16 * cinb_ks(Hk) + 8) * 2


def zform_lds(mode, F0, Hk):                                              # cin_bf16.hip:1230-1231
    kch = 32 if NP_FWD[mode] == 1 else 16
    return 128 * ((F0 | 1) + cb_hp(Hk) + 4) * 4 + 2 * NP_FWD[mode] * 128 * (kch + 8) * 2


def smooth(act):
    return act not in (None, 'linear', 'relu')


def bf16_fwd(mode, B, F0, Hk, L, D, act):
    """(kernel, ks, LDS bytes) with kernel 'noz4' | 'noz8' | 'z' (the Z-forming k_cin_fwd_bf16; ks None): cin_bf16.hip:1200-1232"""
    if mode == 'bf16x3':
        wide, ks = cinb_wide(B * D), cinb_ks(Hk)
        if noz_lds(F0, Hk, wide) <= LDS_MAX and not smooth(act) and ks <= 4:
            return ('noz8' if wide else 'noz4'), ks, noz_lds(F0, Hk, wide)
    return 'z', None, zform_lds(mode, F0, Hk)


def bf16_shape_ok(F0, Hk, L):                                             # cinb_check, cin_bf16.hip:1150-1155
    return L <= 256 and Hk <= 128 and F0 <= 128


def bf16_fwd_launches(mode, B, F0, Hk, L, D, act):
    return min(F0, Hk, L, D) > 0 and bf16_shape_ok(F0, Hk, L) and bf16_fwd(mode, B, F0, Hk, L, D, act)[2] <= LDS_MAX


def dgrad_lds(LS, NP, WV, F0):                                            # cin_bf16.hip:1334-1337
    return 2 * 32 * WV * (F0 | 1) * 4 + 2 * NP * 32 * (16 * LS + 8) * 2


def bf16_dgrad(mode, B, F0, Hk, L, D):
    """(LSTEPS, JB, WV, LDS bytes): cin_bf16.hip:1332-1333 (dgrad_roomy), 1375-1398"""
    NP = NP_BWD[mode]
    jb = ceil_div(Hk, 32)
    LS, JB = (8 if L <= 128 else 16), (1 if jb <= 1 else 2 if jb <= 2 else 4)
    roomy = LS == 8 and JB <= 2
    WV = 8 if roomy and cinb_wide(B * D) and dgrad_lds(LS, NP, 8, F0) <= LDS_MAX else 4
    return LS, JB, WV, dgrad_lds(LS, NP, WV, F0)


def bf16_wgrad(mode, B, F0, Hk, L, D, x0_bs=None, xk_bs=None):
    """('wide', kgroups, sub-tiles per group, lgroups, splits, rows_per_split, last) of k_cin_wgrad_wide or ('tile', kblocks,
    nblocks, splits, rows_per_split, last) of k_cin_wgrad_bf16: cin_bf16.hip:1401-1429"""
    K, M = F0 * Hk, B * D
    if vec4(D, x0_bs, xk_bs, F0, Hk) and F0 + Hk <= 96:
        nsub = ceil_div(K, 32)
        kgroups = ceil_div(nsub, 8 * 4)
        spg, lgroups = ceil_div(nsub, kgroups), ceil_div(L, 64)
        return ('wide', kgroups, spg, lgroups) + _batch_splits(M, kgroups * lgroups, 256)
    kblocks, nblocks = ceil_div(K, 256), ceil_div(L, 128)
    return ('tile', kblocks, nblocks) + _batch_splits(M, kblocks * nblocks, 512)


def bf16_wgrad_lds(mode, F0, Hk, kind):                                   # cin_bf16.hip:1414, 1425
    return (F0 + Hk) * 68 * 4 + NP_BWD[mode] * (64 if kind == 'wide' else 128) * 72 * 2


def bf16_bwd_refusal(mode, B, F0, Hk, L, D):
    if not bf16_shape_ok(F0, Hk, L):
        return 'shape'
    return 'LDS' if bf16_dgrad(mode, B, F0, Hk, L, D)[3] > LDS_MAX else None


def fwd_launches(mode, B, F0, Hk, L, D, act):
    return f32_fwd_launches(F0, Hk, L, D) if mode == 'float32' else bf16_fwd_launches(mode, B, F0, Hk, L, D, act)


def bwd_refusal(mode, B, F0, Hk, L, D):
    return f32_bwd_refusal(F0, Hk, L, D) if mode == 'float32' else bf16_bwd_refusal(mode, B, F0, Hk, L, D)


def plan(c, mode):
    """every plan value of one case in one mode, keyed as the `expect` dicts name them"""
    B, F0, Hk, L, D = c.B, c.F0, c.Hk, c.L, c.D
    if mode == 'float32':
        kb, nb, splits, rps, last = f32_wgrad(B, F0, Hk, L, D)
        return {'dgrad': f32_dgrad(Hk, L), 'kblocks': kb, 'nblocks': nb, 'splits': splits, 'rps': rps, 'last': last,
                'slabs': f32_slabs(F0, Hk, L), 'vec4': vec4(D, F0=F0, Hk=Hk), 'fwd_grid': f32_fwd_grid(B, L, D),
                'fwd_lds': f32_fwd_lds(F0, Hk), 'dgrad_lds': f32_dgrad_lds(Hk, L, D), 'reduce_tail': splits % 8,
                'last_block_rows': B * D - (ceil_div(B * D, 128) - 1) * 128}
    kern, ks, lds = bf16_fwd(mode, B, F0, Hk, L, D, c.act)
    LS, JB, WV, dl = bf16_dgrad(mode, B, F0, Hk, L, D)
    wg = bf16_wgrad(mode, B, F0, Hk, L, D)
    bm = 256 if kern == 'noz8' else 128
    return {'fwd': (kern, ks) if ks else (kern,), 'fwd_lds': lds, 'dgrad': (LS, JB, WV), 'dgrad_lds': dl, 'wgrad': wg[:-3],
            'wgrad_kind': wg[0], 'splits': wg[-3], 'rps': wg[-2], 'last': wg[-1], 'wide': cinb_wide(B * D),
            'filter_tiles': ceil_div(L, 128), 'vec_epilogue': D % 4 == 0,
            'last_block_rows': B * D - (ceil_div(B * D, bm) - 1) * bm,
            'x_slots': ceil_div((F0 + Hk) * 16, 512) if wg[0] == 'wide' else None}


def lds_requests(c, mode):
    """{kernel: dynamic LDS bytes} of every launch the case makes in `mode`"""
    if mode == 'float32':
        return {'fwd': f32_fwd_lds(c.F0, c.Hk), 'dgrad': f32_dgrad_lds(c.Hk, c.L, c.D), 'wgrad': f32_wgrad_lds(c.F0, c.Hk)}
    p = plan(c, mode)
    return {'fwd': p['fwd_lds'], 'dgrad': p['dgrad_lds'], 'wgrad': bf16_wgrad_lds(mode, c.F0, c.Hk, p['wgrad_kind'])}


# ---- the operation ---------------------------------------------------------------------------------------------------------
Case = collections.namedtuple('Case', 'id modes B F0 Hk L D bias act data expect seed')


def case(tag, B, F0, Hk, L, D, modes=MODES, bias=True, act='relu', data='mild', expect=None, seed=0):
    return Case(f'B{B}-F{F0}-H{Hk}-L{L}-D{D}-{act}-{tag}', tuple(modes), B, F0, Hk, L, D, bias, act, data, expect or {}, seed)


FIGURES = ('y', 'dx0', 'dxk', 'dW', 'db')


def lin(c):
    """the layer before its activation: the einsum of tests/test_precision_gpu.py, as fn(x0, xk, W, b)"""
    def fn(x0, xk, W, b):
        z = (x0[:, :, None, :] * xk[:, None, :, :]).permute(0, 3, 1, 2).reshape(c.B * c.D, c.F0 * c.Hk)      # [(b, d), (i, j)]
        y = (z @ W).reshape(c.B, c.D, c.L).permute(0, 2, 1)
        return y + (b[None, :, None] if b is not None else 0)
    return fn


def act_fn(name):
    from oracle import reference_layers as R
    return R._activation(name)


def act_grad(name, pre):
    """act'(pre) in float64"""
    p = pre.detach().clone().requires_grad_(True)
    act_fn(name)(p).sum().backward()
    return p.grad


def rnd(g, shape, scale=1.0):
    """float64 values that float32 holds exactly: the kernel and the reference see the same inputs"""
    return (torch.randn(shape, generator=g, dtype=F64) * scale).float().double()


ZERO_FIELD = 1
ONE_HOT = (2, 3, 1)                 # the (b, l, d) of the one nonzero upstream gradient of the 'one_hot' data


def ZERO_ROWS(B):
    return sorted({0, B // 2, B - 1})


def build_inputs(c):
    """-> ([x0, xk, W, b | None] float64, upstream gradient float64): N(0, 0.5) inputs, W ~ N(0, 1 / K), b ~ N(0, 0.1), as
    tests/test_precision_gpu.py draws them"""
    g = torch.Generator().manual_seed(zlib.crc32(c.id.encode()) + c.seed)
    B, F0, Hk, L, D = c.B, c.F0, c.Hk, c.L, c.D
    x0, xk = rnd(g, (B, F0, D), 0.5), rnd(g, (B, Hk, D), 0.5)
    W = rnd(g, (F0 * Hk, L), 1.0 / np.sqrt(F0 * Hk))
    b = rnd(g, (L,), 0.1) if c.bias else None
    up = rnd(g, (B, L, D))
    if c.data == 'logspace':                                   # field magnitudes 1e-3 .. 1e3 in x0 and in xk
        x0 = (x0 * torch.logspace(-3, 3, F0, dtype=F64)[None, :, None]).float().double()
        xk = (xk * torch.logspace(-3, 3, Hk, dtype=F64)[None, :, None]).float().double()
    elif c.data == 'zero_field':
        x0[:, ZERO_FIELD] = 0.0
    elif c.data == 'zero_rows':
        x0[ZERO_ROWS(B)] = 0.0
        xk[ZERO_ROWS(B)] = 0.0
    elif c.data == 'zero_xk':
        xk = torch.zeros_like(xk)
    elif c.data == 'cancel':                                   # maps (2t, 2t+1): xk' = xk (1 + 2^-10), W' = -W: |y| ~ 2^-10 |A| |B|
        assert Hk % 2 == 0
        xk[:, 1::2] = (xk[:, 0::2] * (1.0 + 2.0 ** -10)).float().double()
        W3 = W.reshape(F0, Hk, L)
        W3[:, 1::2] = -W3[:, 0::2]
        b = None if b is None else torch.zeros_like(b)
    elif c.data == 'relu_dead':
        b = torch.full((L,), -10.0, dtype=F64)
    elif c.data == 'relu_alive':
        b = torch.full((L,), 10.0, dtype=F64)
    elif c.data == 'x30':
        x0 = (x0 * 30.0).float().double()
    elif c.data == 'one_hot':
        one = torch.zeros_like(up)
        one[ONE_HOT] = up[ONE_HOT]
        up = one
    else:
        assert c.data == 'mild', c.data
    return [x0, xk, W, b], up


def run_reference(c, inputs, up, dt, perm=None):
    """[y, dx0, dxk, dW, db | None] of the CPU reference in `dt`; with `perm` the batch is walked in that order (another summation
    order for grad_W and grad_b) and y / dx0 / dxk are put back in the caller's order"""
    xs = [None if t is None else t.to(dt).clone() for t in inputs]
    u = up.to(dt)
    if perm is not None:
        xs[0], xs[1], u = xs[0][perm].clone(), xs[1][perm].clone(), u[perm]
    xs = [None if t is None else t.requires_grad_(True) for t in xs]
    y = act_fn(c.act)(lin(c)(*xs))
    (y * u).sum().backward()
    res = [y.detach()] + [None if t is None else t.grad for t in xs]
    if perm is not None:
        inv = torch.argsort(perm)
        res[0], res[1], res[2] = res[0][inv], res[1][inv], res[2][inv]
    return res


# selu' jumps at 0 as relu' does (from scale alpha = 1.758 to scale = 1.051: csrc/common.h act_grad_from_y takes the side from the
# sign of the rounded output), so its units within the forward's reach of 0 are masked like relu's
KINKED = ('relu', 'selu')
Ref = collections.namedtuple('Ref', 'inputs up masked r64 r32 scales pre s_fwd')
_CACHE = {}


def fwd_class(mode):
    return P.CLAIMS[('cin', mode)][0]


def references(c, cls='fp32'):
    """the references of one case for a forward of class `cls` ('fp32': float32 and bf16x3 modes, 'bf16'): the upstream gradient
    with the relu units zeroed that lie within the class's reach of their kink (precision.kink_mask), the share of units that
    removed, float64 and float32 results and the |A| |B| scale of every figure.  Computed once and shared, never written to.

    Scales: the forward's is |x0| |xk| |W| + |b|; a gradient's the same contraction of the magnitudes with the upstream
    gradient |up| act'(pre) (relu / linear: 0 or 1, exact).  A smooth activation's derivative is formed from the ROUNDED output
    (tanh: 1 - y^2), so its error is absolute, of the order of the output's rounding, however small the derivative is: there the
    gradients are measured against |up| max(|act'|, 1), and the output against |act'| x (forward scale) + |y| (the propagated
    rounding of the pre-activation plus the result's own)."""
    if c.act not in KINKED:
        cls = 'fp32'
    key = (c.id, cls)
    if key not in _CACHE:
        inputs, up = build_inputs(c)
        f = lin(c)
        with torch.no_grad():
            pre = f(*inputs)
        s_fwd = P.abs_forward(f, inputs)
        upm = P.kink_mask(pre, s_fwd, up, 'relu' if c.act in KINKED else c.act, cls).contiguous()    # (where() takes pre's strides)
        masked = float(((upm != up).sum()) / max(int((up != 0).sum()), 1))
        r64, r32 = run_reference(c, inputs, upm, F64), run_reference(c, inputs, upm, F32)
        if c.act == 'relu':
            up_eff, s_out_of = upm * (pre > 0), None
        elif smooth(c.act):
            da = act_grad(c.act, pre).abs()
            up_eff, s_out_of = upm * da.clamp(min=1.0), da
        else:
            up_eff, s_out_of = upm, None
        s_out, s_in = P.abs_scale(f, inputs, up_eff)
        if s_out_of is not None:
            s_out = s_out * s_out_of + r64[0].abs()
        _CACHE[key] = Ref(inputs, upm, masked, r64, r32, [s_out] + s_in, pre, s_fwd)
    return _CACHE[key]


def errors(got, ref):
    """{figure: (elem_cond, cond_rms | None)} of `got` against the float64 reference (grad_b: col_cond)"""
    out = {}
    for name, a, e, s in zip(FIGURES, got, ref.r64, ref.scales):
        if e is None:
            assert a is None, name
            continue
        assert a.shape == e.shape, (name, a.shape, e.shape)
        assert bool(torch.isfinite(a).all()), name
        live = bool((P._d(s) > 0).any())
        out[name] = ((P.col_cond if name == 'db' else P.elem_cond)(a, e, s), P.cond_rms(a, e, s) if live else 0.0)
    return out


def figure_class(mode, name):
    return P.bar_of('cin', mode, 'fwd' if name == 'y' else 'bwd')


def check(test, c, mode, got, ref, record=True):
    """the bars: an fp32-class figure within STEP_BAR['fp32'] x max(the float32 CPU reference's elem_cond, 2^-24); a b17- or
    bf16-class figure within KINK_TOL[class] per element and COND_BAR[class] in the root mean square -> {figure: ratio}"""
    mine, f32 = errors(got, ref), errors(ref.r32, ref)
    ratios, bad = {}, {}
    for name, (ec, rms) in mine.items():
        cls = figure_class(mode, name)
        if cls == 'fp32':
            ratios[name] = ec / max(f32[name][0], P.FLOOR)
            if not ratios[name] <= P.STEP_BAR['fp32']:
                bad[name] = ('elem_cond / max(float32 reference, 2^-24)', ratios[name], P.STEP_BAR['fp32'], ec, f32[name][0])
        else:
            ratios[name] = ec / P.KINK_TOL[cls]
            ratios[name + '_rms'] = rms / P.COND_BAR[cls]
            if not ec <= P.KINK_TOL[cls]:
                bad[name] = ('elem_cond', ec, P.KINK_TOL[cls])
            if not rms <= P.COND_BAR[cls]:
                bad[name + '_rms'] = ('cond_rms', rms, P.COND_BAR[cls])
    if record:
        P.record(f'{test}[{mode}][{c.id}]', **ratios)
    assert not bad, f'cin/{mode} {c.id}: {bad}'
    return ratios


def run_gpu(c, mode, ref, dev, xk_view=None):
    """[y, dx0, dxk, dW, db | None] of ops.cin_layer on float32 copies of the reference's inputs"""
    from deeptables_amd import ops
    xs = [None if t is None else t.float().to(dev).requires_grad_(True) for t in ref.inputs]
    y = ops.cin_layer(xs[0], xs[1] if xk_view is None else xk_view, xs[2], xs[3], c.act, mode)
    assert y.shape == (c.B, c.L, c.D) and y.dtype == F32
    y.backward(ref.up.float().to(dev))
    return [y.detach()] + [None if t is None else t.grad for t in xs]


# ---- the lower classes on the CPU ------------------------------------------------------------------------------------------
def _np_act(name, v):
    with torch.no_grad():
        return act_fn(name)(torch.from_numpy(np.ascontiguousarray(v))).numpy()


def _np_act_grad_from_y(name, y):
    """the derivative as the kernels form it from the rounded output (csrc/common.h act_grad_from_y)"""
    y = y.astype(np.float32)
    one = np.float32(1)
    if name in (None, 'linear'):
        return np.ones_like(y)
    if name == 'relu':
        return (y > 0).astype(np.float32)
    if name == 'sigmoid':
        return y * (one - y)
    if name == 'tanh':
        return one - y * y
    if name == 'elu':
        return np.where(y > 0, one, y + one).astype(np.float32)
    if name == 'selu':
        return np.where(y > 0, np.float32(1.0507009873554805), y + np.float32(1.0507009873554805 * 1.6732632423543772)).astype(np.float32)
    if name == 'softplus':
        return (one - np.exp(-y)).astype(np.float32)
    if name == 'softsign':
        return ((one - np.abs(y)) ** 2).astype(np.float32)
    assert name == 'exponential', name
    return y


def _split_dot(A, Bm, parts):
    """sum over the kept products (p + q < parts) of the bf16 parts of A [n, k] and Bm [k, m], accumulated in float64"""
    from tests.test_split_bf16_arithmetic import split
    a, _ = split(A, parts)
    b, _ = split(Bm, parts)
    out = np.zeros((A.shape[0], Bm.shape[1]))
    for p in range(parts):
        for q in range(parts - p):
            out += a[p].astype(np.float64) @ b[q].astype(np.float64)
    return out


def emulate(c, ref, mode):
    """[y, dx0, dxk, dW, db | None] of the lower class(es) of `mode` in numpy: 'bf16x3' keeps the float32 CPU forward and forms
    the three backward products from two bf16 parts per operand (three products each); 'bf16' forms the forward and the
    backward from one bf16 product.  Operands as the kernels split them: Z = x0 xk rounded to float32 first, G = up act'(y)."""
    parts = NP_BWD[mode]
    x0, xk, W, b = [None if t is None else t.float().numpy() for t in ref.inputs]
    B, F0, Hk, L, D = c.B, c.F0, c.Hk, c.L, c.D
    Z = (x0[:, :, None, :] * xk[:, None, :, :]).transpose(0, 3, 1, 2).reshape(B * D, F0 * Hk).astype(np.float32)
    if mode == 'bf16':
        pre = _split_dot(Z, W, 1).astype(np.float32) + (0 if b is None else b[None, :])
        y = _np_act(c.act, pre.astype(np.float32))
    else:
        y = ref.r32[0].numpy().transpose(0, 2, 1).reshape(B * D, L)
    G = (ref.up.float().numpy().transpose(0, 2, 1).reshape(B * D, L) * _np_act_grad_from_y(c.act, y)).astype(np.float32)
    T = _split_dot(G, np.ascontiguousarray(W.T), parts).reshape(B, D, F0, Hk)
    dx0 = np.einsum('bdij,bjd->bid', T, xk.astype(np.float64))
    dxk = np.einsum('bdij,bid->bjd', T, x0.astype(np.float64))
    dW = _split_dot(np.ascontiguousarray(Z.T), G, parts)
    res = [torch.from_numpy(np.ascontiguousarray(y.reshape(B, D, L).transpose(0, 2, 1))).double(), torch.from_numpy(dx0),
           torch.from_numpy(dxk), torch.from_numpy(dW), None if b is None else torch.from_numpy(G.astype(np.float64).sum(0))]
    return res


# ---- the cases -------------------------------------------------------------------------------------------------------------
X3 = ('bf16x3',)


def _path_cases():
    e = lambda **kw: {k.replace('__', ':'): v for k, v in kw.items()}
    return [
        case('D3_atomic_ws_noz4_ks2_tile_wgrad', 9, 3, 5, 6, 3, expect=e(
            float32__slabs=False, float32__vec4=False, float32__dgrad=(64, 1), bf16x3__fwd=('noz4', 2), bf16x3__wgrad_kind='tile',
            bf16__wgrad_kind='tile', bf16x3__vec_epilogue=False)),
        case('dgrad_64_1_ks2_LS8_one_tile_lgroups2', 9, 3, 32, 128, 8, expect=e(
            float32__dgrad=(64, 1), bf16x3__fwd=('noz4', 2), bf16x3__dgrad=(8, 1, 4), bf16__dgrad=(8, 1, 4), bf16x3__filter_tiles=1,
            bf16x3__wgrad=('wide', 1, 3, 2), bf16__wgrad=('wide', 1, 3, 2))),
        case('dgrad_128_2_ks4_LS16_two_tiles_lgroups3', 9, 3, 33, 129, 8, expect=e(
            float32__dgrad=(128, 2), float32__fwd_grid=(1, 2), bf16x3__fwd=('noz4', 4), bf16x3__dgrad=(16, 2, 4),
            bf16__dgrad=(16, 2, 4), bf16x3__filter_tiles=2, bf16x3__wgrad=('wide', 1, 4, 3), bf16__wgrad=('wide', 1, 4, 3))),
        case('dgrad_64_2_noz4_ks4', 9, 2, 64, 36, 4, expect=e(
            float32__dgrad=(64, 2), bf16x3__fwd=('noz4', 4), bf16x3__dgrad=(8, 2, 4), bf16__dgrad=(8, 2, 4))),
        case('dgrad_64_4_zforming', 9, 2, 65, 40, 8, expect=e(
            float32__dgrad=(64, 4), bf16x3__fwd=('z',), bf16x3__dgrad=(8, 4, 4), bf16__dgrad=(8, 4, 4))),
        case('dgrad_128_4_both_backward_limits_tile_wgrad', 5, 2, 128, 256, 4, expect=e(
            float32__dgrad=(128, 4), bf16x3__dgrad=(16, 4, 4), bf16__dgrad=(16, 4, 4), bf16x3__wgrad_kind='tile',
            bf16__wgrad_kind='tile', bf16x3__fwd=('z',))),
        case('dgrad_128_1_D12_vec4', 9, 3, 20, 130, 12, expect=e(
            float32__dgrad=(128, 1), float32__vec4=True, bf16x3__dgrad=(16, 1, 4), bf16__dgrad=(16, 1, 4))),
        case('dgrad_128_2_11_splits_reduce_8_plus_3_last_60_scalar', 70, 3, 40, 256, 10, expect=e(
            float32__dgrad=(128, 2), float32__splits=11, float32__reduce_tail=3, float32__last=60, float32__vec4=False,
            float32__slabs=True)),
        case('11_splits_KL1155_atomic_ws', 44, 5, 7, 33, 16, expect=e(
            float32__splits=11, float32__slabs=False, float32__vec4=True)),
        case('44_splits', 700, 2, 3, 5, 4, expect=e(float32__splits=44, float32__last=48)),
        case('kblocks3_spg22_lgroups2', 40, 26, 26, 128, 16, expect=e(
            float32__kblocks=3, float32__splits=10, bf16x3__wgrad=('wide', 1, 22, 2), bf16__wgrad=('wide', 1, 22, 2))),
        case('wgrad_wide_two_k_groups_of_17_sub_tiles', 9, 26, 40, 8, 4, expect=e(
            bf16x3__wgrad=('wide', 2, 17, 1), bf16__wgrad=('wide', 2, 17, 1), float32__kblocks=5)),
        case('D128_B1', 1, 4, 4, 8, 128, expect=e(float32__fwd_grid=(1, 1), float32__splits=2, bf16x3__fwd=('noz4', 2))),
        case('D1', 11, 7, 9, 5, 1, expect=e(float32__vec4=False, float32__last_block_rows=11, bf16x3__wgrad_kind='tile')),
        case('wgrad_wide_three_x_slots', 9, 90, 6, 40, 4, expect=e(
            bf16x3__wgrad_kind='wide', bf16__wgrad_kind='wide', bf16x3__x_slots=3, bf16__x_slots=3)),
        case('wgrad_tile_F0_plus_Hk_97', 9, 91, 6, 40, 4, expect=e(bf16x3__wgrad_kind='tile', bf16__wgrad_kind='tile')),
        # wide batches, B D >= 32768
        case('wide_noz8_ks2_dgrad_8_1_8_172_wide_splits', 257, 3, 5, 33, 128, expect=e(
            bf16x3__wide=True, bf16x3__fwd=('noz8', 2), bf16x3__dgrad=(8, 1, 8), bf16__dgrad=(8, 1, 8),
            bf16x3__wgrad=('wide', 1, 1, 1), bf16x3__splits=172, bf16__splits=172)),
        case('wide_noz8_ks4_dgrad_8_2_8', 2049, 4, 33, 40, 16, expect=e(
            bf16x3__wide=True, bf16x3__fwd=('noz8', 4), bf16x3__dgrad=(8, 2, 8), bf16__dgrad=(8, 2, 8))),
        case('wide_zforming_dgrad_8_4_four_waves', 2049, 4, 65, 40, 16, expect=e(
            bf16x3__wide=True, bf16x3__fwd=('z',), bf16x3__dgrad=(8, 4, 4), bf16__dgrad=(8, 4, 4))),
        case('wide_noz8_two_filter_tiles_dgrad_16_1_four_waves', 2049, 4, 8, 129, 16, expect=e(
            bf16x3__wide=True, bf16x3__fwd=('noz8', 2), bf16x3__filter_tiles=2, bf16x3__dgrad=(16, 1, 4), bf16__dgrad=(16, 1, 4))),
        case('wide_M32770_scalar_epilogue_last_block_2_rows_257_splits_last_2', 3277, 4, 8, 32, 10, expect=e(
            bf16x3__wide=True, bf16x3__fwd=('noz8', 2), bf16x3__vec_epilogue=False, bf16x3__last_block_rows=2,
            bf16x3__wgrad_kind='tile', bf16x3__splits=257, bf16x3__last=2, bf16__splits=257, bf16__last=2,
            float32__splits=257, float32__last=2, float32__reduce_tail=1)),
        case('wide_noz8_163840_B', 257, 100, 2, 8, 128, expect=e(
            bf16x3__fwd=('noz8', 2), bf16x3__fwd_lds=163840, bf16x3__dgrad=(8, 1, 4))),
        case('wide_F0_101_falls_back_to_zforming', 257, 101, 2, 8, 128, expect=e(bf16x3__fwd=('z',), bf16x3__wide=True)),
        case('wide_x3_dgrad_eight_waves_163840_B', 257, 63, 2, 8, 128, expect=e(
            bf16x3__dgrad=(8, 1, 8), bf16x3__dgrad_lds=163840, bf16__dgrad=(8, 1, 8))),
        case('wide_x3_dgrad_falls_back_to_four_waves', 257, 64, 2, 8, 128, expect=e(
            bf16x3__dgrad=(8, 1, 4), bf16__dgrad=(8, 1, 8))),
        case('wide_noz8_ks4_163840_B', 257, 52, 33, 8, 128, modes=X3, expect=e(
            bf16x3__fwd=('noz8', 4), bf16x3__fwd_lds=163840, bf16x3__dgrad=(8, 2, 8))),
    ]


SMOOTH_ACTS = ('sigmoid', 'tanh', 'elu', 'selu', 'softplus', 'softsign', 'exponential')
ACT_CASES = [case('act', 9, 3, 5, 6, 4, act=a, expect={'bf16x3:fwd': ('z',)}) for a in SMOOTH_ACTS] + \
            [case('act', 9, 3, 5, 6, 4, act='linear', bias=False)]

# limits that still run: D > 128 in the bf16 modes, three filter tiles in the exact forward
LIMIT_RUN_CASES = [case('D132_bf16_modes_only', 3, 3, 5, 6, 132, modes=('bf16x3', 'bf16'))]

HARD_MODES = ('float32', 'bf16x3')
HARD_SHAPE = (9, 4, 6, 8, 8)


def _hard_cases():
    h = lambda tag, data, act='relu', **kw: case(tag, *HARD_SHAPE, modes=HARD_MODES, act=act, data=data, **kw)
    return [h('fields_1e-3_to_1e3', 'logspace'), h('fields_1e-3_to_1e3', 'logspace', act='linear'),
            h('zero_field', 'zero_field'), h('zero_batch_rows', 'zero_rows'), h('zero_xk', 'zero_xk'),
            h('filter_rows_cancel', 'cancel', act='linear'), h('relu_all_dead', 'relu_dead'), h('relu_all_alive', 'relu_alive'),
            h('saturated', 'x30', act='tanh'), h('saturated', 'x30', act='sigmoid'), h('one_hot_upstream', 'one_hot', act='linear')]


PATH_CASES = _path_cases()
HARD_CASES = _hard_cases()
ALL_CASES = PATH_CASES + ACT_CASES + LIMIT_RUN_CASES + HARD_CASES
BY_ID = {c.id: c for c in ALL_CASES}
assert len(BY_ID) == len(ALL_CASES)

# figures that are zero by construction
ZERO_OK = {'zero_xk': {'y', 'dx0', 'dW'}, 'relu_dead': {'y', 'dx0', 'dxk', 'dW', 'db'}}
# the bias is replaced by a constant or dropped
NO_BIAS_NOISE = ('cancel',)


def by_shape(B, F0, Hk, L, D, act='relu'):
    return next(c for c in PATH_CASES + ACT_CASES if (c.B, c.F0, c.Hk, c.L, c.D, c.act) == (B, F0, Hk, L, D, act))


STRIDED = by_shape(9, 3, 5, 6, 4, 'linear')
REPEAT_SHAPES = [(70, 3, 40, 256, 10), (40, 26, 26, 128, 16), (3277, 4, 8, 32, 10)]

# forward runs, backward refuses: (mode, F0, Hk, L, D, what the message names, LDS bytes of the refused dgrad | None)
FORWARD_ONLY = [
    ('bf16x3', 126, 4, 8, 4, 'LDS', 164864), ('bf16x3', 94, 4, 129, 4, 'LDS', 164864), ('bf16x3', 128, 100, 8, 4, 'LDS', 166912),
    ('bf16', 128, 4, 129, 4, 'LDS', 165888),
    ('float32', 4, 128, 8, 100, 'LDS', 187408), ('float32', 4, 129, 8, 4, 'Hk', None), ('float32', 4, 4, 257, 4, 'L', None),
    ('float32', 4, 4, 300, 4, 'L', None),
]
# neither runs: (mode, F0, Hk, L, D, what the forward's message names, LDS bytes | None)
REFUSED = [('bf16x3', 128, 128, 8, 4, 'LDS', 170496), ('float32', 4, 4, 8, 129, 'D', None), ('float32', 300, 4, 8, 4, 'LDS', 176640),
           ('bf16', 129, 4, 8, 4, 'shape', None), ('bf16x3', 4, 129, 8, 4, 'shape', None), ('bf16', 4, 4, 257, 4, 'shape', None)]
# the largest shapes of each mode that do both: the other side of the limits above
BOTH_RUN = [('bf16x3', 125, 4, 8, 4), ('bf16x3', 93, 4, 129, 4), ('bf16', 128, 128, 8, 4), ('bf16', 127, 4, 129, 4),
            ('float32', 128, 128, 8, 4), ('float32', 4, 128, 8, 64)]



def limit_case(mode, F0, Hk, L, D, B=2):
    # (bf16 at contraction lengths of 512 and more: |pre| / (|A| |B|) ~ K^-1/2 nears the class's 2^-7 and the kink mask would
    # remove a third of the relu units: linear there, the cap stays)
    return case('limit', B, F0, Hk, L, D, modes=(mode,), act='linear' if mode == 'bf16' else 'relu')


# the cases the limit tests of the GPU module measure (the forward alone where the backward refuses)
LIMIT_CASES = [limit_case(*t[:5]) for t in FORWARD_ONLY] + [limit_case(*t) for t in BOTH_RUN]
# every shape at which dt_cin_fwd_supported is compared with the return code of the three forwards at B = 1
SUPPORT_SHAPES = sorted({t[1:5] for t in FORWARD_ONLY + REFUSED + BOTH_RUN} | {(3, 5, 6, 132), (4, 4, 8, 128), (275, 4, 8, 4), (276, 4, 8, 4)})

POOL_CASES = [(8200, 130, 4, 2), (5, 6, 8, 0), (5, 6, 8, 5), (3, 7, 12, 3)]     # (B, L, D, half)


def pool_grid(B, L, half):
    """(blocks, elements the busiest thread walks) of k_cin_pool: cin.hip:745-747"""
    n = B * (L - half)
    blocks = min(ceil_div(n, 256), 256 * 16)
    return blocks, ceil_div(n, blocks * 256)


def params_of(cases):
    import pytest
    return [pytest.param(c, id=c.id) for c in cases]


def mode_params(cases):
    import pytest
    return [pytest.param(c, m, id=f'{m}-{c.id}') for c in cases for m in c.modes]
