# -*- coding:utf-8 -*-
"""GPU: the Compressed-Interaction-Network kernels of csrc/cin.hip (exact fp32 MFMA) and csrc/cin_bf16.hip (split-bf16 'bf16x3',
plain 'bf16') against the float64 reference of the same layer on the same float32-rounded inputs, at every launch path of the
three dispatchers, at their shape limits and on inputs that are hard for the layer.  Every case compares y, grad_x0, grad_xk,
grad_W and (with a bias) grad_b in each mode it lists.

Paths (tests/cin_support.py holds the table and the restated dispatch arithmetic; tests/test_cin_paths_host.py proves each id
against it and the restatement against the library's own size functions): all six k_cin_dgrad<LH, JB> and all eight
k_cin_dgrad_bf16(_4) instantiations per part count; the Z-free forward at ks = 2 | 4 in four- and eight-wave blocks, over two
filter tiles, with the scalar epilogue and a last block of 2 rows, at exactly 163,840 B of LDS and one field past it; the
Z-forming forward at a narrow and a wide batch; k_cin_wgrad_wide | k_cin_wgrad_bf16 on both sides of F0 + Hk = 96;
k_cin_wgrad_reduce with 11 = 8 + 3 and 257 = 32 x 8 + 1 slabs; the memset + atomics branch of the workspace backward
(K L % 4 != 0) with 1, 11 and 44 batch splits; D = 1, D = 128 with B = 1, D = 132 in the bf16 modes.

Bars (tests/precision.py; no number of it changed), per element: |e| / (|A| |B| of the same contraction), then the max
(precision.elem_cond; grad_b: col_cond).
  fp32-class figures (everything in float32 mode, the bf16x3 forward): yardstick B,
      elem_cond(gpu) <= STEP_BAR['fp32'] = 12 x max(elem_cond(float32 CPU reference), 2^-24).
  b17-class (bf16x3 backward) and bf16-class figures: elem_cond <= KINK_TOL[class] (2^-14, 2^-7: the per-element reach of the
      class) and cond_rms <= COND_BAR[class] (128 U, 65536 U).  A wrong index gives an elem_cond of order 1.
The upstream gradient of relu (and selu: its derivative jumps at 0 too) units within KINK_TOL[forward class] of the kink is
zeroed; the share that removes is capped by the host test (0.5 % fp32 / b17, 20 % bf16).

Contracts, through the C entry points on pre-filled buffers: dt_cin_layer_bwd_ws overwrites grad_x0, grad_xk and grad_W (NaN
beforehand; slab and atomic branch); dt_cin_layer_bwd adds to grad_x0 and grad_W and overwrites grad_xk; the bf16 / bf16x3
backwards overwrite both grad_x and add to grad_W and grad_b; B = 0 returns OK and touches nothing; a misaligned ws or grad_W is
refused; x0_bstride > F0 D and a channel slice as xk give the bits of their contiguous copies.

Repeats: the forward, both grad_x and the float32 workspace grad_W take no atomics and repeat bit for bit (test_repeatable).
grad_b (every mode) and the bf16 / bf16x3 grad_W are merged with float atomics in the order the hardware serves them: they are
held to the bar only.

MI355X, the largest figure over the cases of each test (DT_PRECISION_LOG; the forward, grad_x and the float32 grad_W repeat to the
digit, the atomically merged figures show one run).  Largest of all: float32 grad_xk 3.54 of 12 at (257, 100, 2, 8, 128), float32
y 2.64 at (40, 26, 26, 128, 16), bf16x3 y 1.74 at (257, 101, 2, 8, 128); bf16 grad_x0 0.92 of its per-element reach at
(257, 101, 2, 8, 128); bf16x3 grad_W 0.56 of its rms bar on the one-hot upstream gradient.  No figure reached a bar and no kernel
arithmetic was changed; the two LDS refusals of the dgrad launchers now name F0, Hk, L and D.
fp32-class figures, err_gpu / max(err_f32, 2^-24) in elem_cond (bar 12):
  test             float32: y    dx0   dxk   dW    db       bf16x3: y
  paths                     2.64  1.10  3.54  1.21  1.51            1.74
  activations               1.20  1.08  1.46  1.36  0.62            1.15
  hard:logspace             1.20  0.82  0.95  1.50  0.42            1.26
  hard:zero_field           1.69  0.86  0.69  1.00  0.51            0.76
  hard:zero_rows            0.87  0.87  0.93  1.00  0.35            0.86
  hard:zero_xk              0.00  0.00  1.04  0.00  0.23            0.00
  hard:cancel               0.65  0.33  0.74  0.98  0.23            0.30
  hard:relu_dead            0.00  0.00  0.00  0.00  0.00            0.00
  hard:relu_alive           0.82  0.83  0.82  0.89  0.26            0.78
  hard:x30                  0.98  0.83  0.83  0.67  0.36            0.75
  hard:one_hot              0.90  0.66  0.87  1.00  0.00            0.48
  contracts                 1.04  0.90  0.84  1.21  1.51            0.43
  strided xk                1.04  1.08  1.30  0.89                  0.57
  repeatable                2.64  0.65  0.84  0.58  0.67            0.64
  limits                    1.18  0.64  1.45  0.84  0.62            1.17
  pool                      0.79
lower-class figures as a share of their bars, elem_cond / KINK_TOL | cond_rms / COND_BAR (bar 1):
  test             bf16x3: dx0         dxk         dW          db           bf16: y           dx0         dxk         dW          db
  paths                   0.39 | 0.34 0.28 | 0.36 0.29 | 0.32 0.00 | 0.00       0.66 | 0.17 0.92 | 0.37 0.83 | 0.37 0.79 | 0.34 0.00 | 0.00
  activations             0.18 | 0.21 0.22 | 0.27 0.08 | 0.21 0.00 | 0.00       0.36 | 0.28 0.37 | 0.21 0.50 | 0.28 0.35 | 0.21 0.02 | 0.02
  hard:logspace           0.21 | 0.36 0.20 | 0.41 0.06 | 0.17 0.00 | 0.00
  hard:zero_field         0.20 | 0.27 0.22 | 0.34 0.10 | 0.22 0.00 | 0.00
  hard:zero_rows          0.09 | 0.21 0.17 | 0.28 0.22 | 0.39 0.00 | 0.00
  hard:zero_xk            0.00 | 0.00 0.10 | 0.20 0.00 | 0.00 0.00 | 0.00
  hard:cancel             0.00 | 0.00 0.07 | 0.16 0.05 | 0.14 0.00 | 0.00
  hard:relu_dead          0.00 | 0.00 0.00 | 0.00 0.00 | 0.00 0.00 | 0.00
  hard:relu_alive         0.08 | 0.16 0.10 | 0.20 0.05 | 0.12 0.00 | 0.00
  hard:x30                0.03 | 0.04 0.03 | 0.04 0.01 | 0.03 0.00 | 0.00
  hard:one_hot            0.08 | 0.37 0.12 | 0.53 0.19 | 0.56 0.00 | 0.00
  contracts               0.11 | 0.30 0.12 | 0.36 0.21 | 0.20 0.00 | 0.00       0.30 | 0.15 0.45 | 0.29 0.58 | 0.37 0.61 | 0.22 0.00 | 0.00
  strided xk              0.07 | 0.20 0.11 | 0.27 0.08 | 0.21                   0.36 | 0.28 0.27 | 0.21 0.46 | 0.28 0.35 | 0.21
  repeatable              0.08 | 0.10 0.15 | 0.13 0.06 | 0.07 0.00 | 0.00       0.51 | 0.13 0.30 | 0.10 0.44 | 0.13 0.22 | 0.07 0.00 | 0.00
  limits                  0.14 | 0.28 0.02 | 0.05 0.40 | 0.42 0.00 | 0.00       0.10 | 0.05 0.08 | 0.05 0.06 | 0.04 0.70 | 0.35 0.00 | 0.00
Mutants, each run once on the MI355X (tests of this module red / of the 55 older CIN kernel tests red): k_cin_dgrad<64,2>
dispatched where <64,4> belongs 4 / 0; the bf16 dgrad <8,2> where <8,4> belongs 5 / 0; k_cin_wgrad_reduce without its tail loop
32 / 17; the last batch split skipped in k_cin_wgrad 53 / 20 and in k_cin_wgrad_wide 63 / 19; the Z-free forward's ks threshold
32 -> 40: 6 / 0; overwrite forced to 0 in the workspace dgrad 49 / 18 (the older tests see it because fresh allocations were not
zero in that run; the NaN pre-fill of test_workspace_backward_overwrites does not depend on that); k_cin_pool without its
grid-stride step 1 / 0; has[u] of k_cin_wgrad_wide ignoring sub1 (inside nsub) 1 / 9, plus the bf16x3 run of the same two-k-group
case, which the ks mutant of the same library also turns red.  (Three libraries of mutants with disjoint (mode, figure) footprints;
each failure is attributed by the figures its message names.)
"""
import ctypes

import pytest
import torch

from tests import cin_support as S
from tests import precision as P

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32


def _ref(c, mode):
    return S.references(c, S.fwd_class(mode))


def _run_check(test, c, mode, dev):
    ref = _ref(c, mode)
    got = S.run_gpu(c, mode, ref, dev)
    S.check(test, c, mode, got, ref)
    if not c.bias:
        assert got[4] is None
    return got, ref


# ---- every launch path -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c,mode', S.mode_params(S.PATH_CASES + S.LIMIT_RUN_CASES))
def test_paths(dev, c, mode):
    _run_check('paths', c, mode, dev)


@pytest.mark.parametrize('c,mode', S.mode_params(S.ACT_CASES))
def test_activations(dev, c, mode):
    """the <true> instantiations of the three forwards (bf16x3: the Z-forming kernel for any activation but linear / relu) and
    act_grad_from_y in the three backwards"""
    _run_check('activations', c, mode, dev)


# ---- hard inputs -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c,mode', S.mode_params(S.HARD_CASES))
def test_hard_inputs(dev, c, mode):
    got, ref = _run_check(f'hard:{c.data}', c, mode, dev)
    y, dx0, dxk, dW, db = got
    if c.data == 'zero_field':
        assert not bool(dW.reshape(c.F0, c.Hk, c.L)[S.ZERO_FIELD].any()) and bool(dx0[:, S.ZERO_FIELD].any())
    if c.data == 'zero_rows':
        rows = S.ZERO_ROWS(c.B)
        assert not bool(dx0[rows].any()) and not bool(dxk[rows].any()) and bool(dx0.any())
    if c.data == 'zero_xk':
        assert not bool(dx0.any()) and not bool(dW.any()) and bool(dxk.any())
        assert torch.equal(y, torch.relu(ref.inputs[3].float().to(dev))[None, :, None].expand_as(y))
    if c.data == 'relu_dead':
        assert not any(bool(t.any()) for t in got)                        # every gradient exactly zero
    if c.data == 'relu_alive':
        assert bool((y > 0).all())
    if c.data == 'one_hot':                                               # the gradient lands in the rows (b, :, d) and nowhere else
        b, l, d = S.ONE_HOT
        keep = torch.zeros(c.B, c.D, dtype=torch.bool, device=dev)
        keep[b, d] = True
        for g in (dx0, dxk):
            assert not bool(g.permute(0, 2, 1)[~keep].any()) and bool(g[b, :, d].all())
        assert not bool(dW[:, [k for k in range(c.L) if k != l]].any()) and not bool(db[[k for k in range(c.L) if k != l]].any())


# ---- the C entry points ----------------------------------------------------------------------------------------------------
FWD = {'float32': 'dt_cin_layer_fwd', 'bf16': 'dt_cin_layer_fwd_bf16', 'bf16x3': 'dt_cin_layer_fwd_bf16x3'}
BWD = {'float32': 'dt_cin_layer_bwd', 'ws': 'dt_cin_layer_bwd_ws', 'bf16': 'dt_cin_layer_bwd_bf16', 'bf16x3': 'dt_cin_layer_bwd_bf16x3'}


def _workspace(mode, c, dev):
    from deeptables_amd._lib import lib
    n = {'ws': lambda: lib().dt_cin_bwd_workspace_bytes(c.B, c.F0, c.Hk, c.L, c.D),
         'bf16': lambda: lib().dt_cin_bf16_workspace_bytes(c.F0, c.Hk, c.L),
         'bf16x3': lambda: lib().dt_cin_bf16x3_workspace_bytes(c.F0, c.Hk, c.L)}.get(mode, lambda: 0)()
    return torch.empty(((max(n, 16) + 3) // 4,), dtype=F32, device=dev) if mode != 'float32' else None


def _raw_fwd(mode, c, x0, xk, W, b, y, x0_bs=None, xk_bs=None):
    from deeptables_amd import _lib
    from deeptables_amd._lib import lib, ptr, stream_ptr
    args = [ptr(x0), ptr(xk), ptr(W), ptr(b), _lib.act_code(c.act, 'CIN'), c.B, c.F0, c.Hk, c.L, c.D,
            c.F0 * c.D if x0_bs is None else x0_bs, c.Hk * c.D if xk_bs is None else xk_bs, ptr(y)]
    if mode != 'float32':
        args.append(ptr(_workspace(mode, c, y.device)))
    return getattr(lib(), FWD[mode])(*args, stream_ptr())


def _raw_bwd(entry, c, x0, xk, W, y, gy, gx0, gxk, gW, gb, ws=None, x0_bs=None, xk_bs=None, B=None):
    from deeptables_amd import _lib
    from deeptables_amd._lib import lib, ptr, stream_ptr
    args = [ptr(x0), ptr(xk), ptr(W), ptr(y), ptr(gy), _lib.act_code(c.act, 'CIN'), c.B if B is None else B, c.F0, c.Hk, c.L, c.D,
            c.F0 * c.D if x0_bs is None else x0_bs, c.Hk * c.D if xk_bs is None else xk_bs, ptr(gx0), ptr(gxk), ptr(gW), ptr(gb)]
    if entry != 'float32':
        args.append(ws if isinstance(ws, ctypes.c_void_p) else ptr(ws))
    return getattr(lib(), BWD[entry])(*args, stream_ptr())


def _device_inputs(c, mode, dev):
    """the reference of the case, its inputs on the device, y of the mode's forward and the upstream gradient"""
    ref = _ref(c, mode)
    x0, xk, W, b = [None if t is None else t.float().to(dev) for t in ref.inputs]
    y = torch.empty((c.B, c.L, c.D), dtype=F32, device=dev)
    assert _raw_fwd(mode, c, x0, xk, W, b, y) == 0
    return ref, x0, xk, W, b, y, ref.up.float().contiguous().to(dev)


def _filled(shape, value, dev):
    return torch.full(shape, value, dtype=F32, device=dev)


WS_BRANCH = {'slabs': (70, 3, 40, 256, 10), 'atomics_one_split': (9, 3, 5, 6, 3), 'atomics_11_splits': (44, 5, 7, 33, 16)}


@pytest.mark.parametrize('branch', sorted(WS_BRANCH))
def test_workspace_backward_overwrites(dev, branch):
    """ops allocates the three gradients with torch.empty for dt_cin_layer_bwd_ws: NaN beforehand, the result afterwards, on
    the slab branch (k_cin_wgrad_reduce's overwrite) and on the K L % 4 != 0 branch (memset, then float atomics)"""
    c = S.by_shape(*WS_BRANCH[branch])
    assert S.f32_slabs(c.F0, c.Hk, c.L) == (branch == 'slabs')
    ref, x0, xk, W, b, y, gy = _device_inputs(c, 'float32', dev)
    nan = float('nan')
    gx0, gxk, gW = _filled(x0.shape, nan, dev), _filled(xk.shape, nan, dev), _filled(W.shape, nan, dev)
    gb = torch.zeros((c.L,), dtype=F32, device=dev)
    ws = _workspace('ws', c, dev).fill_(nan)
    assert _raw_bwd('ws', c, x0, xk, W, y, gy, gx0, gxk, gW, gb, ws) == 0
    S.check(f'contract:ws_overwrites:{branch}', c, 'float32', [y, gx0, gxk, gW, gb], ref)


def test_plain_backward_adds_to_grad_x0_and_grad_W_and_overwrites_grad_xk(dev):
    c = S.by_shape(70, 3, 40, 256, 10)
    ref, x0, xk, W, b, y, gy = _device_inputs(c, 'float32', dev)
    g = torch.Generator().manual_seed(11)
    b0, bW, bb = S.rnd(g, tuple(x0.shape)), S.rnd(g, tuple(W.shape)), S.rnd(g, (c.L,))
    gx0, gW, gb = b0.float().to(dev), bW.float().to(dev), bb.float().to(dev)
    gxk = _filled(xk.shape, float('nan'), dev)
    assert _raw_bwd('float32', c, x0, xk, W, y, gy, gx0, gxk, gW, gb) == 0
    before = [None, b0, None, bW, bb]
    shifted = ref._replace(r64=[r if a is None else r + a for r, a in zip(ref.r64, before)],
                           r32=[r if a is None else r + a.float() for r, a in zip(ref.r32, before)],
                           scales=[s if a is None else s + a.abs() for s, a in zip(ref.scales, before)])
    S.check('contract:plain_adds', c, 'float32', [y, gx0, gxk, gW, gb], shifted)


@pytest.mark.parametrize('mode', ['bf16x3', 'bf16'])
@pytest.mark.parametrize('shape', [(9, 3, 32, 128, 8), (9, 3, 5, 6, 3)], ids=['wide_wgrad', 'tile_wgrad'])
def test_bf16_backward_overwrites_grad_x_and_adds_to_grad_W_and_grad_b(dev, mode, shape):
    c = S.by_shape(*shape)
    ref, x0, xk, W, b, y, gy = _device_inputs(c, mode, dev)
    g = torch.Generator().manual_seed(12)
    bW, bb = S.rnd(g, tuple(W.shape)), S.rnd(g, (c.L,))
    gW, gb = bW.float().to(dev), bb.float().to(dev)
    gx0, gxk = _filled(x0.shape, float('nan'), dev), _filled(xk.shape, float('nan'), dev)
    assert _raw_bwd(mode, c, x0, xk, W, y, gy, gx0, gxk, gW, gb, _workspace(mode, c, dev)) == 0
    before = [None, None, None, bW, bb]
    shifted = ref._replace(r64=[r if a is None else r + a for r, a in zip(ref.r64, before)],
                           r32=[r if a is None else r + a.float() for r, a in zip(ref.r32, before)],
                           scales=[s if a is None else s + a.abs() for s, a in zip(ref.scales, before)])
    S.check('contract:bf16_overwrites_adds', c, mode, [y, gx0, gxk, gW, gb], shifted)


@pytest.mark.parametrize('entry', ['float32', 'ws', 'bf16x3', 'bf16'])
def test_empty_batch_touches_nothing(dev, entry):
    c = S.by_shape(9, 3, 5, 6, 3)
    mode = 'float32' if entry == 'ws' else entry
    ref, x0, xk, W, b, y, gy = _device_inputs(c, mode, dev)
    bufs = [_filled(s, -7.0, dev) for s in (x0.shape, xk.shape, W.shape, (c.L,), y.shape)]
    ws = _filled((4096,), -7.0, dev)
    empty = c._replace(B=0)
    assert _raw_fwd(mode, empty, x0, xk, W, b, bufs[4]) == 0
    assert _raw_bwd(entry, c, x0, xk, W, y, gy, *bufs[:4], ws=ws, B=0) == 0
    torch.cuda.synchronize()
    assert all(bool((t == -7.0).all()) for t in bufs + [ws])


def test_workspace_backward_refuses_misaligned_pointers(dev):
    from deeptables_amd._lib import lib
    c = S.by_shape(9, 3, 5, 6, 4, 'linear')
    ref, x0, xk, W, b, y, gy = _device_inputs(c, 'float32', dev)
    gx0, gxk = torch.zeros_like(x0), torch.zeros_like(xk)
    gWbuf, ws = torch.zeros(W.numel() + 4, dtype=F32, device=dev), _workspace('ws', c, dev)
    ok_gW, off_gW = gWbuf[:W.numel()], gWbuf[1:1 + W.numel()]
    off_ws = ctypes.c_void_p(ws.data_ptr() + 4)
    for gW_, ws_ in ((off_gW, ws), (ok_gW, off_ws), (ok_gW, ctypes.c_void_p(0))):
        assert _raw_bwd('ws', c, x0, xk, W, y, gy, gx0, gxk, gW_, None, ws_) != 0
        assert b'16-byte aligned' in lib().dt_last_error()
    torch.cuda.synchronize()
    assert not bool(gWbuf.any()) and not bool(gx0.any())


@pytest.mark.parametrize('shape', [(70, 3, 40, 256, 10), (9, 3, 5, 6, 3)], ids=['slabs', 'atomics'])
def test_atomic_weight_gradient_agrees_with_the_workspace_path(dev, shape, monkeypatch):
    """DT_AMD_CIN_WGRAD_ATOMIC=1: ops.cin_layer takes dt_cin_layer_bwd (float atomics into zeroed buffers)"""
    c = S.by_shape(*shape)
    a, ref = _run_check('contract:ws_path', c, 'float32', dev)
    monkeypatch.setenv('DT_AMD_CIN_WGRAD_ATOMIC', '1')
    b, _ = _run_check('contract:atomic_path', c, 'float32', dev)
    assert all(torch.equal(a[k], b[k]) for k in (0, 1, 2))                # the forward and the dgrad are the same launches


@pytest.mark.parametrize('mode', S.MODES)
def test_x0_batch_stride_through_the_entry_points(dev, mode):
    """x0 as the first F0 fields of a wider [B, F0 + 2, D] tensor (x0_bstride > F0 D) and xk as a channel slice: the bits of the
    contiguous copies, forward and backward"""
    c = S.by_shape(9, 3, 32, 128, 8)
    ref, x0, xk, W, b, y, gy = _device_inputs(c, mode, dev)
    wide0, widek = _filled((c.B, c.F0 + 2, c.D), 1e6, dev), _filled((c.B, c.Hk + 3, c.D), 1e6, dev)
    wide0[:, :c.F0], widek[:, :c.Hk] = x0, xk
    bs0, bsk = (c.F0 + 2) * c.D, (c.Hk + 3) * c.D
    y2 = torch.empty_like(y)
    assert _raw_fwd(mode, c, wide0, widek, W, b, y2, bs0, bsk) == 0
    assert torch.equal(y, y2)
    entry = 'ws' if mode == 'float32' else mode
    outs = []
    for a0, ak, s0, sk in ((x0, xk, None, None), (wide0, widek, bs0, bsk)):
        g = [torch.zeros_like(x0), torch.zeros_like(xk), torch.zeros_like(W), torch.zeros((c.L,), dtype=F32, device=dev)]
        assert _raw_bwd(entry, c, a0, ak, W, y, gy, *g, ws=_workspace(entry, c, dev), x0_bs=s0, xk_bs=sk) == 0
        outs.append(g)
    S.check('contract:bstride', c, mode, [y2] + outs[1], ref)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    if mode == 'float32':
        assert torch.equal(outs[0][2], outs[1][2])


@pytest.mark.parametrize('mode', S.MODES)
def test_strided_xk(dev, mode):
    """ops.cin_layer on xk = a channel slice of a wider tensor (the direct=False stack): bit-equal to its contiguous copy"""
    c = S.STRIDED
    a, ref = _run_check('layout:contiguous', c, mode, dev)
    base = _filled((c.B, c.Hk + 3, c.D), 1e6, dev)
    base[:, :c.Hk] = ref.inputs[1].float().to(dev)
    base.requires_grad_(True)
    view = base[:, :c.Hk]
    assert not view.is_contiguous()
    got = S.run_gpu(c, mode, ref, dev, xk_view=view)
    got[2] = base.grad[:, :c.Hk]
    assert not bool(base.grad[:, c.Hk:].any())
    S.check('layout:strided_xk', c, mode, got, ref)
    assert all(torch.equal(a[k], got[k]) for k in ((0, 1, 2, 3) if mode == 'float32' else (0, 1, 2)))


# ---- repeatability ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', S.MODES)
@pytest.mark.parametrize('shape', S.REPEAT_SHAPES, ids=lambda s: '-'.join(map(str, s)))
def test_repeatable(dev, shape, mode):
    c = S.by_shape(*shape)
    a, _ = _run_check('repeatable', c, mode, dev)
    b, _ = _run_check('repeatable', c, mode, dev)
    assert torch.equal(a[0], b[0]), 'forward'
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), 'grad_x'
    if mode == 'float32':
        assert S.f32_slabs(c.F0, c.Hk, c.L) and torch.equal(a[3], b[3]), 'grad_W through the workspace'


# ---- limits ----------------------------------------------------------------------------------------------------------------
NAMES = {'LDS': r'F0={F0} Hk={Hk} L={L} D={D}: the dgrad tiles need {lds} B of LDS', 'L': r'L={L} > 256', 'Hk': r'Hk={Hk} > 128',
         'D': r'D={D} > 128', 'shape': r'L <= 256, Hk <= 128, F0 <= 128 \(L={L} Hk={Hk} F0={F0}\)'}


def _supported(mode, F0, Hk, L, D, act='relu'):
    from deeptables_amd import _lib
    return bool(_lib.lib().dt_cin_fwd_supported(S.MODE_CODE[mode], F0, Hk, L, D, _lib.act_code(act, 'CIN')))


_limit_case = S.limit_case


@pytest.mark.parametrize('mode,F0,Hk,L,D,what,lds', S.FORWARD_ONLY)
def test_forward_runs_backward_refuses(dev, mode, F0, Hk, L, D, what, lds):
    """the shapes DESIGN.md lists: dt_cin_fwd_supported says yes, the forward is right, backward() raises naming the limit and
    the shape and leaves no gradient behind"""
    from deeptables_amd import ops
    from deeptables_amd._lib import DtHipError
    c = _limit_case(mode, F0, Hk, L, D)
    assert _supported(mode, F0, Hk, L, D) and S.fwd_launches(mode, 1, F0, Hk, L, D, 'relu')
    ref = _ref(c, mode)
    xs = [t.float().to(dev).requires_grad_(True) for t in ref.inputs]
    y = ops.cin_layer(*xs, c.act, mode)
    S.check('limits:forward_only', c, mode, [y.detach(), None, None, None, None],
            ref._replace(r64=[ref.r64[0]] + [None] * 4, r32=[ref.r32[0]] + [None] * 4))
    with pytest.raises(DtHipError, match=NAMES[what].format(F0=F0, Hk=Hk, L=L, D=D, lds=lds)):
        y.backward(ref.up.float().to(dev))
    torch.cuda.synchronize()
    assert all(t.grad is None for t in xs)


@pytest.mark.parametrize('mode,F0,Hk,L,D,what,lds', S.REFUSED)
def test_forward_refuses(dev, mode, F0, Hk, L, D, what, lds):
    from deeptables_amd import ops
    from deeptables_amd._lib import DtHipError
    c = _limit_case(mode, F0, Hk, L, D)
    assert not _supported(mode, F0, Hk, L, D) and not S.fwd_launches(mode, 1, F0, Hk, L, D, 'relu')
    inputs, _ = S.build_inputs(c)
    match = rf'tiles need {lds} B of LDS' if what == 'LDS' else NAMES[what].format(F0=F0, Hk=Hk, L=L, D=D)
    with pytest.raises(DtHipError, match=match):
        ops.cin_layer(*[t.float().to(dev) for t in inputs], c.act, mode)


@pytest.mark.parametrize('mode,F0,Hk,L,D', S.BOTH_RUN)
def test_largest_shapes_that_do_both(dev, mode, F0, Hk, L, D):
    """one step inside each limit of test_forward_runs_backward_refuses: forward and backward run and are right"""
    assert _supported(mode, F0, Hk, L, D)
    _run_check('limits:both_run', _limit_case(mode, F0, Hk, L, D), mode, dev)


@pytest.mark.parametrize('F0,Hk,L,D', S.SUPPORT_SHAPES)
def test_supported_agrees_with_the_forward_calls(dev, F0, Hk, L, D):
    """dt_cin_fwd_supported against what the three forwards return at B = 1, at every limit shape of this module"""
    c = S.case('supported', 1, F0, Hk, L, D, bias=False)
    inputs, _ = S.build_inputs(c)
    x0, xk, W, _ = [None if t is None else t.float().to(dev) for t in inputs]
    for mode in S.MODES:
        y = torch.empty((1, L, D), dtype=F32, device=dev)
        rc = _raw_fwd(mode, c, x0, xk, W, None, y)
        assert (rc == 0) == _supported(mode, F0, Hk, L, D) == S.fwd_launches(mode, 1, F0, Hk, L, D, 'relu'), (mode, rc)
    torch.cuda.synchronize()


@pytest.mark.parametrize('L', [257, 300])
def test_three_filter_tiles_in_the_exact_forward(dev, L):
    """covered by test_forward_runs_backward_refuses (float32, L = 257 | 300): grid.y = 3 of k_cin_fwd"""
    assert ('float32', 4, 4, L, 4, 'L', None) in S.FORWARD_ONLY and S.f32_fwd_grid(2, L, 4) == (1, 3)


# ---- the split + pool of the direct=False stack ----------------------------------------------------------------------------
@pytest.mark.parametrize('B,L,D,half', S.POOL_CASES)
def test_pool(dev, B, L, D, half):
    """ops.cin_split_pool: sum over D of the channels [half, L) against float64 (col_cond, the bar of the fp32 class); at
    n = B (L - half) > 1,048,576 a thread of k_cin_pool walks its grid-stride loop twice; the backward assembles gy from the
    hidden and the pooled gradient, each also NULL through the C entry point"""
    from deeptables_amd import ops
    from deeptables_amd._lib import lib, ptr, stream_ptr
    g = torch.Generator().manual_seed(B + L + D + half)
    y64 = S.rnd(g, (B, L, D))
    yd = y64.float().to(dev).requires_grad_(True)
    hidden, pooled = ops.cin_split_pool(yd, half)
    assert hidden.shape == (B, half, D) and pooled.shape == (B, L - half) and torch.equal(hidden, yd[:, :half])
    want, scale = y64[:, half:].sum(-1), y64[:, half:].abs().sum(-1)
    err, err32 = P.col_cond(pooled, want, scale), P.col_cond(y64.float()[:, half:].sum(-1), want, scale)
    P.record(f'pool[{B},{L},{D},{half}]', pooled=err / max(err32, P.FLOOR))
    assert err <= P.STEP_BAR['fp32'] * max(err32, P.FLOOR), (err, err32)
    gh, gp = S.rnd(g, (B, half, D)).float().to(dev), S.rnd(g, (B, L - half)).float().to(dev)
    ((hidden * gh).sum() + (pooled * gp).sum()).backward()
    want_gy = torch.cat([gh, gp[:, :, None].expand(B, L - half, D)], 1)
    assert torch.equal(yd.grad, want_gy)
    for a, b in ((None, gp), (gh if half else None, None)):
        gy = _filled((B, L, D), float('nan'), dev)
        assert lib().dt_cin_pool_bwd(ptr(a), ptr(b), B, L, D, half, ptr(gy), stream_ptr()) == 0
        want0 = want_gy.clone()
        if a is None:
            want0[:, :half] = 0
        if b is None:
            want0[:, half:] = 0
        assert torch.equal(gy, want0)
