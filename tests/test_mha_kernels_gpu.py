# -*- coding:utf-8 -*-
"""GPU: the attention core kernels of csrc/mha.hip (dt_mha_core_fwd / dt_mha_core_bwd, all ten instantiations) through the C
entry points on framed buffers, against the float64 reference of deeptables/models/layers.py:129-145 on the same float32-rounded
inputs: at every head width bracket in both row movers (float4 | one float), in the contiguous, the production ([B, F, 4 D]
column blocks) and a padded layout, at the grid edges, with the attention dropout at its field limit, and on hard inputs.

Paths: tests/mha_support.py holds the table and the restated launch arithmetic, tests/test_mha_paths_host.py proves each id
against it.

Bars (tests/precision.py; no number of it changed): out, lse, grad_q, grad_k and grad_v in max_rel and in row_rel (one (b, f) row
of D entries against itself; lse one (b, h) row of F), each held to err_gpu <= STEP_BAR['fp32'] = 12 x max(err_f32, 2^-24), err_f32
the larger error of the two float32 CPU forms of the reference (batched matmul | per-key loop in the kernel's order).

Frames: q, k, v sit in NaN-filled buffers (pad columns, the fourth column block and the rows before and after are NaN), out and
lse between sentinel rows, the gradients NaN-prefilled in a [B, F, ldg] buffer whose other columns and frame hold a bit pattern.
After the calls every input and every frame is bitwise unchanged, the gradient blocks hold no NaN (the backward overwrites).

MI355X, err_gpu / max(err_f32, 2^-24), the largest figure over the cases of each group (one DT_PRECISION_LOG run), max_rel /
row_rel, bar 12.  Largest of all: grad_q 3.58 (row_rel, B11-F3-D10-H2), out 2.13, lse 2.13, grad_v 2.08, grad_k 1.49.
  group              out          lse          grad_q       grad_k       grad_v
  widths             1.27 / 1.20  2.13 / 1.97  1.88 / 3.29  1.49 / 0.82  2.08 / 1.49
  layouts            1.34 / 1.23  1.62 / 1.75  1.00 / 2.18  1.07 / 0.99  1.09 / 1.37
  grid               1.60 / 1.12  1.32 / 1.88  0.96 / 3.58  0.99 / 0.54  1.00 / 1.28
  dropout            1.14 / 1.30  1.35 / 1.68  0.85 / 0.67  1.09 / 1.42  1.44 / 1.20
  hard:signed        1.13 / 1.35  1.84 / 1.84  1.29 / 1.19  1.25 / 1.22  1.27 / 1.30
  hard:logits30      1.09 / 1.09  0.99 / 1.00  0.93 / 1.00  0.97 / 1.00  1.03 / 0.95
  hard:q1000         1.00 / 2.13  0.76 / 0.83  1.01 / 1.00  1.01 / 1.00  1.00 / 1.00
  hard:q0            0.96 / 1.35  0.74 / 0.74  0.73 / 1.09  0.00 / 0.00  1.00 / 1.00
  hard:fields        1.09 / 1.33  1.00 / 1.00  1.00 / 1.00  1.00 / 1.00  1.00 / 1.00
  layer core (ops)   1.00 / 0.94               0.80 / 0.54  1.25 / 1.13  1.51 / 1.03
  through ops: out 1.00 / 1.20, grad_x 1.16 / 0.53, grad_W 0.66 / 0.56, grad_b 0.91 / 0.91
On the hard inputs the float32 yardstick itself is 2 .. 1,300 x 2^-24 in max_rel, and in row_rel beyond any bound on the rows
of grad_q / grad_k that a saturated softmax leaves at 1e-60 of their terms: there the figure holds only because the kernels,
like the reference's softmax, give such a row the weight 1.0f exactly and its gradient an exact zero.

What these cases found in the kernels as they were (same cases, same bar, MI355X), and what was changed in csrc/mha.hip:
  1 the backward rebuilt p = exp(s - lse) from lse = m + log l held in ONE float: rounded at the size of the scores, and s - lse
    contracted into an fma on the unrounded product.  hard:fields (scores to 1e6) at D = 12: grad_v 176,385 x (1.4 % of its
    largest entry), grad_k 76,962 x; hard:q1000: grad_v 21.7 x.  Now the forward saves (m, 1 / l) and p = exp(s - m) * (1 / l).
  2 delta_i = dO_i . O_i from the stored output does not cancel against dP_ij the way sum_j p_ij dP_ij does when a row is
    nearly one-hot: hard:logits30 at D = 8: grad_k row_rel 16.5 x.  The backward is now two launches, the first sums delta.
  3 dot * scale - m was contracted into one fma, so the row maximum was not one of the scores the exponentials saw: a
    saturated row's weight came out 1 +- 2^-24 instead of 1, its l below 1, and 2^-24 |dP| |q| leaked into gradients that
    are exactly zero (hard:fields at D = 12: grad_k 16,974 x after 1 and 2).  The scaled score is now a float of its own.
"""
import ctypes

import pytest
import torch

from tests import mha_support as S
from tests import precision as P

pytestmark = pytest.mark.gpu

F64, F32, I32 = torch.float64, torch.float32, torch.int32
G = 64                                      # floats of frame before and after every buffer: a multiple of four (16 bytes)
NAN_BITS, SENTINEL, PATTERN = 0x7FC00000, 0x4B3C2D1E, 0x4A1B2C3D


class Frame:
    """rows x width floats, rows `ld` apart, inside a flat buffer filled with one bit pattern: G + offset floats of frame in
    front, G behind.  offset = 1 puts the first row one float past a 16-byte boundary."""

    def __init__(self, dev, rows, width, ld, bits, offset=0):
        self.flat = torch.full((G + offset + max(rows, 1) * ld + G,), bits, dtype=I32, device=dev)
        self.lo, self.hi, self.rows, self.width, self.ld, self.bits = G + offset, G + offset + rows * ld, rows, width, ld, bits
        self.body = self.flat.view(F32)[self.lo:self.lo + max(rows, 1) * ld].view(max(rows, 1), ld)[:rows]
        assert self.flat.data_ptr() % 16 == 0

    def cols(self, a, b):
        return self.body[:, a:b]

    def put(self, a, values):
        self.body[:, a:a + values.shape[-1]] = values.reshape(self.rows, -1).to(self.flat.device, F32)

    def snapshot(self):
        self.saved = self.flat.clone()

    def unchanged(self):
        return torch.equal(self.flat, self.saved)

    def frame_intact(self, written):
        """everything outside the column ranges `written` [(a, b)] still holds the fill pattern"""
        mask = torch.ones_like(self.flat, dtype=torch.bool)
        body = mask[self.lo:self.lo + self.rows * self.ld].view(self.rows, self.ld)
        for a, b in written:
            body[:, a:b] = False
        return bool((self.flat[mask] == (self.bits if self.bits < 2 ** 31 else self.bits - 2 ** 32)).all())


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _lib():
    from deeptables_amd import _lib
    return _lib.lib()


def run_core(c, dev, offset=0, lse=True, backward=True):
    """one forward (and backward) of a case through the C entry points on framed buffers -> ({name: CPU tensor}, (rc_fwd,
    rc_bwd)); asserts the frames.  offset: every buffer starts that many floats past a 16-byte boundary"""
    lib = _lib()
    ref = S.references(c)
    B, F, D, H = c.B, c.F, c.D, c.H
    ld, ldg = S.strides(c)
    n = B * F
    if c.layout == 'prod':
        src = Frame(dev, n, 4 * D, ld, NAN_BITS, offset)
        ins, views = [src], [src.cols(i * D, (i + 1) * D) for i in range(3)]
        for i, t in enumerate((ref.q, ref.k, ref.v)):
            src.put(i * D, t)
    else:
        ins = [Frame(dev, n, D, ld, NAN_BITS, offset) for _ in range(3)]
        views = [f.cols(0, D) for f in ins]
        for f, t in zip(ins, (ref.q, ref.k, ref.v)):
            f.put(0, t)
    out, lse_f = Frame(dev, n, D, D, SENTINEL, offset), Frame(dev, B * H, F, F, SENTINEL, offset)
    stats = Frame(dev, B * H, 2 * F, 2 * F, SENTINEL, offset)       # (m, 1 / l) of every score row: what the backward takes
    for f in ins:
        f.snapshot()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    seed = int(c.seed) & 0xFFFFFFFF
    rc_f = lib.dt_mha_core_fwd(_ptr(views[0]), _ptr(views[1]), _ptr(views[2]), B, F, D, H, ld, float(c.rate), seed,
                               _ptr(out.body), _ptr(lse_f.body) if lse else None, _ptr(stats.body) if lse else None, stream)
    torch.cuda.synchronize()
    assert all(f.unchanged() for f in ins), 'the forward wrote to an input or its frame'
    assert out.frame_intact([(0, D)] if rc_f == 0 else []) and lse_f.frame_intact([(0, F)] if rc_f == 0 and lse else [])
    assert stats.frame_intact([(0, 2 * F)] if rc_f == 0 and lse else [])
    got = {}
    if rc_f == 0:
        got['out'] = out.body.reshape(B, F, D).cpu()
        if lse:
            got['lse'] = lse_f.body.reshape(B, H, F).cpu()
            got['stats'] = stats.body.reshape(B, H, F, 2).cpu()
    rc_b = None
    if backward:
        assert lse
        gout = Frame(dev, n, D, D, NAN_BITS, offset)
        gout.put(0, ref.up)
        grads = Frame(dev, n, 3 * D, ldg, PATTERN, offset)
        grads.body[:, :3 * D] = float('nan')
        ws = Frame(dev, B * H, F, F, PATTERN, offset)              # delta of every row, between the backward's two launches
        for f in ins + [stats, gout]:
            f.snapshot()
        rc_b = lib.dt_mha_core_bwd(_ptr(views[0]), _ptr(views[1]), _ptr(views[2]), _ptr(stats.body), _ptr(gout.body),
                                   B, F, D, H, ld, ldg, float(c.rate), seed, _ptr(grads.cols(0, D)),
                                   _ptr(grads.cols(D, 2 * D)), _ptr(grads.cols(2 * D, 3 * D)), _ptr(ws.body), stream)
        torch.cuda.synchronize()
        assert all(f.unchanged() for f in ins + [stats, gout]), 'the backward wrote to an input, a saved tensor or a frame'
        assert grads.frame_intact([(0, 3 * D)]), 'the backward wrote outside the three gradient blocks'
        assert ws.frame_intact([(0, F)] if rc_b == 0 else []), 'the backward wrote outside its workspace'
        if rc_b == 0:
            for i, name in enumerate(('grad_q', 'grad_k', 'grad_v')):
                got[name] = grads.cols(i * D, (i + 1) * D).reshape(B, F, D).cpu()
                assert not bool(torch.isnan(got[name]).any()), f'{name}: a NaN of the prefill is left'
        else:
            assert bool(torch.isnan(grads.body[:, :3 * D]).all()), 'a refused backward wrote a gradient'
    return got, (rc_f, rc_b)


def _bits_equal(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[n].view(I32), b[n].view(I32)) for n in a)


def _check_case(test, c, dev):
    has_bwd = S.plan(c)['bwd'] is not None
    got, rc = run_core(c, dev, lse=True, backward=True)
    assert rc == (S.DT_OK, S.DT_OK if has_bwd else S.DT_ERR_UNSUPPORTED), (rc, _lib().dt_last_error())
    st = got.pop('stats').double()
    assert set(got) == set(S.NAMES if has_bwd else S.NAMES[:2])
    S.check(f'{test}[{c.id}]', got, S.references(c), tuple(got))
    # the saved pair (m, 1 / l): m - log(1 / l) is the log-sum-exp; m is one of the row's scores, so its own term of l is
    # exactly 1 and 1 <= l <= F
    S.check(f'{test}:stats[{c.id}]', {'lse': st[..., 0] - torch.log(st[..., 1])}, S.references(c), ('lse',))
    assert bool((st[..., 1] <= 1.0).all()) and bool((st[..., 1] >= (1.0 - 1e-6) / c.F).all()), '1 / l lies in [1 / F, 1]'
    return got


# ---- every path ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', S.params_of(S.WIDTH_CASES))
def test_head_widths(dev, c):
    """every head width of the table: both directions up to 32, out and lse beyond (the backward refuses, nothing is written)"""
    _check_case('widths', c, dev)


@pytest.mark.parametrize('c', S.params_of([c for c in S.LAYOUT_CASES if c.lse]))
def test_layouts(dev, c):
    """q, k, v as column blocks of one [B, F, 4 D] buffer with the gradients in a [B, F, 4 D] buffer (what the layer does), and
    rows one float longer than D (3 D + 1 for the gradients), which only the one-float kernels can take"""
    _check_case('layouts', c, dev)


@pytest.mark.parametrize('c', S.params_of([c for c in S.LAYOUT_CASES if not c.lse]))
def test_forward_without_lse(dev, c):
    """lse == NULL and stats == NULL (inference): the same out, bit for bit, and nothing written where they would go"""
    with_lse = _check_case('no_lse', c, dev)
    got, rc = run_core(c, dev, lse=False, backward=False)
    assert rc[0] == S.DT_OK and set(got) == {'out'} and torch.equal(got['out'].view(I32), with_lse['out'].view(I32))


@pytest.mark.parametrize('c', S.params_of(S.GRID_CASES))
def test_grid_edges(dev, c):
    """B H F = 255 | 256 | 257 | three blocks with a ragged tail, F = 1, a wave that spans ten (b, h) pairs, F = 65 | 70"""
    _check_case('grid', c, dev)


def test_empty_batch_touches_nothing(dev):
    lib = _lib()
    B, F, D, H = S.EMPTY_BATCH
    bufs = [Frame(dev, 4, D, D, SENTINEL) for _ in range(9)]
    p = [_ptr(f.body) for f in bufs]
    assert lib.dt_mha_core_fwd(p[0], p[1], p[2], B, F, D, H, D, 0.0, 0, p[3], p[4], p[5], None) == S.DT_OK
    assert lib.dt_mha_core_bwd(p[0], p[1], p[2], p[5], p[3], B, F, D, H, D, 3 * D, 0.0, 0, p[6], p[7], p[8], p[4], None) == S.DT_OK
    assert lib.dt_mha_core_fwd(None, None, None, B, F, D, H, D, 0.0, 0, None, None, None, None) == S.DT_OK
    torch.cuda.synchronize()
    assert all(f.frame_intact([]) for f in bufs)


# ---- dropout -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', S.params_of(S.DROP_CASES))
def test_dropout(dev, c):
    """the kernel's keep mask is the restatement's (hash, float32 threshold, float32 keep scale; h * 4096 + i * 64 + j unique up
    to F = 64) in the forward and in both roles of the backward: the float64 reference multiplies the softmax by that mask, and
    one flipped weight, a transposed mask or a mask without the head term is over the bar a hundred times
    (test_mha_paths_host.py)"""
    _check_case('dropout', c, dev)


# ---- hard inputs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', S.params_of(S.HARD_CASES))
def test_hard_inputs(dev, c):
    """signed data, logits x 30, a one-hot softmax (q x 1000: exp overflows without the max), uniform weights (q = 0: grad_k is
    exactly zero), fields scaled 1e-3 .. 1e3"""
    got = _check_case(f'hard:{c.data}', c, dev)
    if c.data == 'q0':
        assert not bool(got['grad_k'].any()), 'grad_k = sum_i dS_ir q_i with q = 0 is exactly zero'


# ---- path independence -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('a,b', [pytest.param(a, b, id=a.id) for a, b in S.PAIRS])
def test_float4_and_one_float_kernels_agree_bit_for_bit(dev, a, b):
    """the same values through k_mha_*<DHMAX, true> (ld = D | 4 D) and k_mha_*<DHMAX, false> (ld = D + 1): the two row movers
    feed the same arithmetic; and a second run of one case repeats the first (no atomics, no order left to the scheduler)"""
    ga, gb = run_core(a, dev)[0], run_core(b, dev)[0]
    assert set(ga) == set(S.NAMES) | {'stats'} and _bits_equal(ga, gb)
    assert _bits_equal(ga, run_core(a, dev)[0]) and _bits_equal(gb, run_core(b, dev)[0])


def test_buffers_one_float_off_alignment_take_the_one_float_kernels(dev):
    """a float4 shape whose every buffer starts one float past a 16-byte boundary (a contiguous gradient view at an odd offset
    reaches the kernel this way): the launchers' float4 predicate asks for the pointers' alignment, the one-float kernels run
    and give the aligned run's bits"""
    c = S.OFFSET_CASE
    assert S.plan(c, offset=1)['fwd'].endswith('s') and S.plan(c, offset=1)['bwd'].endswith('s')
    aligned = _check_case('offset', c, dev)
    shifted, rc = run_core(c, dev, offset=1)
    shifted.pop('stats')
    assert rc == (S.DT_OK, S.DT_OK) and _bits_equal(aligned, shifted)


# ---- the domain ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('F,D,H,rate', list(S.REFUSED))
def test_refused_shapes_launch_nothing(dev, F, D, H, rate):
    """outside dt_mha_core_supported: each direction called directly returns what the restatement says (the forward alone takes
    head widths 33 .. 64), a refused call leaves out, lse and the gradients as they were"""
    c = S.refused_case(F, D, H, rate)
    got, rc = run_core(c, dev)
    assert rc == S.REFUSED[(F, D, H, rate)] and rc[1] == S.DT_ERR_UNSUPPORTED, (rc, _lib().dt_last_error())
    assert set(got) == ({'out', 'lse', 'stats'} if rc[0] == S.DT_OK else set())
    assert not _lib().dt_mha_core_supported(F, D, H, 1 if rate > 0 else 0)


@pytest.mark.parametrize('F,D,H,rate', [k for k in S.REFUSED if k[3] == 0])
def test_layer_core_outside_the_domain(dev, F, D, H, rate):
    """MultiheadAttention's core for the shapes the kernels refuse (the reference's op chain), against float64 in both
    directions at the kernels' own bar; ops.mha_core itself refuses a tensor that needs a gradient, in the forward"""
    from deeptables_amd import ops
    from deeptables_amd._lib import DtHipError
    from deeptables_amd.models import layers
    c = S.refused_case(F, D, H, rate)
    ref = S.references(c)
    layer = layers.MultiheadAttention({'num_heads': H, 'dropout_rate': rate})
    xs = [t.float().to(dev).requires_grad_(True) for t in (ref.q, ref.k, ref.v)]
    out = layer._core_by_ops(*xs, 0.0)
    (out * ref.up.float().to(dev)).sum().backward()
    got = dict(zip(('out', 'grad_q', 'grad_k', 'grad_v'), [out.detach().cpu()] + [t.grad.cpu() for t in xs]))
    S.check(f'layer_core[{c.id}]', got, ref, tuple(got))
    with pytest.raises(DtHipError):
        ops.mha_core(*xs, H)


def test_layer_trains_with_dropout_on_65_fields(dev):
    """(F, D, H, rate) = (65, 8, 2, 0.3): attention dropout past the hash's 64 fields.  The layer trains without raising and is
    deterministic in eval (where the kernels run it: no dropout there)"""
    from deeptables_amd import functional
    from deeptables_amd.models import layers
    functional.set_seed(11)
    g = torch.Generator().manual_seed(65)
    x = torch.randn(6, 65, 8, generator=g).to(dev).requires_grad_(True)
    layer = layers.MultiheadAttention({'num_heads': 2, 'dropout_rate': 0.3, 'use_residual': True})
    layer.build(tuple(x.shape))
    layer.to(dev)
    layer.train()
    y = layer(x)
    y.sum().backward()
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in layer.dense_Q.parameters())
    layer.eval()
    with torch.no_grad():
        a, b = layer(x), layer(x)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())


def test_net_with_head_width_40_fits_a_batch(dev):
    """embeddings_output_dim = 40, num_heads = 1: a head 40 wide, past the backward kernel's 32.  The forward agrees with the
    oracle and one train step runs (it used to raise in loss.backward())"""
    from deeptables_amd import functional
    from deeptables_amd.models import ModelConfig, DeepModel
    from deeptables_amd.models.metainfo import CategoricalColumn, ContinuousColumn
    from oracle import bridge
    functional.set_seed(3)
    F, Nd, D, B = 4, 2, 40, 32
    conf = ModelConfig(nets=['autoint_nets'], fixed_embedding_dim=True, embeddings_output_dim=D, embedding_dropout=0,
                       dense_dropout=0, metrics=['AUC'],
                       autoint_params={'num_attention': 1, 'num_heads': 1, 'dropout_rate': 0, 'use_residual': True})
    cats = [CategoricalColumn(f'C{i}', 20 + i, D) for i in range(F)]
    conts = [ContinuousColumn('input_continuous_all', [f'I{j}' for j in range(Nd)])]
    dm = DeepModel('binary', 2, conf, cats, conts)
    dm.build(dev)
    g = torch.Generator().manual_seed(5)
    idx = torch.stack([torch.randint(0, c.vocabulary_size, (B,), generator=g) for c in cats], 1)
    dense = torch.randn(B, Nd, generator=g)
    y = (torch.rand(B, 1, generator=g) < 0.25).float()
    dm.model.train()
    logit = dm.model([idx.int().to(dev), dense.to(dev)])
    ref_logit, _ = bridge.oracle_forward(dm, idx, dense, training=True)
    assert (logit.detach().double().cpu() - ref_logit).abs().max().item() < 1e-4
    loss, _ = dm.train_step([idx.int().to(dev), dense.to(dev)], y.to(dev))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(torch.as_tensor(float(loss))))


# ---- through ops: the default-config layout ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', S.LAYER_SHAPES, ids=lambda s: 'B{}-F{}-D{}-H{}'.format(*s))
def test_projection_core_residual_through_ops(dev, shape):
    """ops.dense ([D, 4 D], relu) + ops.split_cols + ops.mha_core(grad_cols=4) + residual + relu, what MultiheadAttention.call
    runs for every shape the fused layer kernel does not take (D = 4, H = 1 is the default configuration): ld = ldg = 4 D, the
    gradient buffer completed in place by split_cols' backward.  Against the float64 restatement of layers.py:119-150"""
    from deeptables_amd import ops
    B, F, D, H = shape
    t, r64, yard = S.layer_references(shape)
    x, W, b = (t[n].float().to(dev).requires_grad_(True) for n in ('x', 'W', 'b'))
    assert not ops.autoint_supported(x, H) and ops.mha_supported(F, D, H) and ops.dense_supported(x, W)
    y = ops.dense(x, W, b, 'relu')
    parts = list(ops.split_cols(y, D))
    assert [p.stride(1) for p in parts] == [4 * D] * 4
    out = torch.relu(ops.mha_core(parts[0], parts[1], parts[2], H, grad_cols=4) + parts[3])
    out.backward(t['up'].float().to(dev))
    got = dict(zip(S.LAYER_NAMES, [out.detach().cpu(), x.grad.cpu(), W.grad.cpu(), b.grad.cpu()]))
    P.check_step('layer_through_ops[B{}-F{}-D{}-H{}]'.format(*shape), 'mha', 'float32', S.figures(got, r64, yard, S.LAYER_NAMES))
