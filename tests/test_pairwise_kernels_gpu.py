# -*- coding:utf-8 -*-
"""GPU: the pair kernels of csrc/product.hip (InnerProduct, OuterProduct mat / vec / num) and of csrc/interaction.hip
(BilinearInteraction in its three weight layouts, AFM attention pooling) against the float64 restatement of
oracle/reference_layers.py on the same float32-rounded inputs, at every launch path of their dispatch code and on inputs that
are hard for a pair kernel.  Every case compares the forward, grad_x and every parameter gradient.

Paths (tests/pairwise_support.py holds the table; tests/test_pairwise_paths_host.py proves each id against the launchers'
arithmetic): k_pair_dot_* from one pair in one lane to P > 64 lanes, F D > 64 and the second row of a wave's grid-stride loop
(B > 8192 forward, B > 1024 backward under the 256-block cap); the generic mat / bilinear kernels at B around the 64-row tile,
with acc[1], acc[4] and all 16 weight-gradient accumulators, 2 and 16 batch splits, and D = 16 with F = 37 (forward on MFMA,
backward generic); the D = 16 MFMA kernels at B around the 16-row tile, P = 1, a field change inside a wave's pair range,
F = 36 (149,992 B of LDS) and 8 batch splits of 8 and 9 tiles; AFM at the HMAX edges for both activation instantiations, the
unblocked grad_Wa path (D % 4 != 0, or more than 256 register blocks) over one and two rows of a block, three passes of the
pooled sum, the second row of the forward loop, P > 256 threads, P < 64, and no bias through the backward.

Bars (tests/precision.py, yardstick B, no number of it changed): err_gpu <= STEP_BAR['fp32'] = 12 x max(error of the float32
CPU reference, 2^-24), row_rel for tensors of rank >= 2 and max_rel otherwise.  Where fields span six orders of magnitude or
terms cancel (logspace, cancel) the metric is per element, |e| / (|A| |B| of the same contraction) (precision.elem_cond), the
bar the same 12 x max(the float32 reference's figure in that metric, 2^-24).

The forward and grad_x take no atomics: two runs agree bit for bit (test_repeatable).  The parameter gradients are merged
across blocks and batch splits with float atomics, whose order is the hardware's: they are held to the bar only.

MI355X, the largest err_gpu / max(err_f32, 2^-24) per figure over the cases of each test (bar 12; DT_PRECISION_LOG; out and dx
repeat to the digit, the parameter gradients move with the order of the atomics and show the larger of two runs):
  test                     out    dx     dk / dW / dWa  dba    dpv
  paths: k_pair_dot        2.67   2.29   4.74
  paths: generic           3.45   1.96   2.09
  paths: D = 16 MFMA       5.75   2.57   2.06
  paths: AFM               3.10   2.65   1.96           4.36   4.75
  hard: logspace (cond)    1.13   1.10   1.43
  hard: zero_field         3.20   1.16   4.05
  hard: zero_rows          1.18   1.58   1.67
  hard: cancel (cond)      1.00   1.16   2.47
  hard: AFM                1.40   10.79  7.89           2.33   1.52
  layout                   1.37   1.89   1.68           1.30   1.38
  grad_view                              1.50
  repeatable               2.21   1.57   2.65           1.18   0.39
hard: AFM is led by the x scaled by 30 under tanh (dx 10.79, dWa 7.89; the flat and one-pair softmax stay under 1.4): the
attention units saturate, and the kernel, like autograd, takes tanh' = 1 - y^2 from the rounded output y, so a tanhf that is a few
ulp off 1 is a large relative error of the derivative (read from the code; not measured apart).  No figure reached the bar and nothing in the kernels' arithmetic was
changed.  dt_bilinear_bwd's generic grad_x launch asks for 66,304 B of dynamic LDS at D = 64 and did not opt in past 64 KiB: it now
computes the size, refuses past 150 KiB and calls hipFuncSetAttribute (the D = 63 and D = 64 rows of test_paths)"""
import pytest
import torch

from tests import pairwise_support as S
from tests import precision as P

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32


def _group(c):
    if c.kind == 'afm':
        return 'afm'
    if c.kind in S.PAIR_KINDS:
        return 'pair_dot'
    return 'mfma16' if S.mfma_bwd(c.F, c.D) else 'generic'


# ---- every launch path -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', S.params_of(S.PATH_CASES + S.AFM_CASES))
def test_paths(dev, c):
    got, r64 = S.check_case(f'paths:{_group(c)}', c, dev)
    if c.kind == 'afm' and not c.bias:
        assert got[3] is None and r64[3] is None                          # grad_ba: no bias, no gradient


# ---- hard inputs -----------------------------------------------------------------------------------------------------------
def _run_with_upstream(c, inputs, up, dev):
    xs = [None if t is None else t.float().to(dev).requires_grad_(True) for t in inputs]
    out = S.gpu_fn(c)(*xs)
    out.backward(up.float().to(dev))
    return out.detach(), xs[0].grad


@pytest.mark.parametrize('c', S.params_of(S.HARD_CASES))
def test_hard_inputs(dev, c):
    got, r64 = S.check_case(f'hard:{c.data}', c, dev)
    inputs, up, _, _ = S.references(c)
    if c.data == 'zero_field':
        # every output that pairs with the zero field is exactly 0, and so is the slice of a per-pair kernel gradient
        z, zp = S.ZERO_FIELD, S.pairs_with(c.F, S.ZERO_FIELD)
        assert not bool(got[0][:, zp].any())
        if c.kind in ('outer_vec', 'bil_field_interaction'):
            assert not bool(got[2][zp].any())
        if c.kind == 'outer_mat':
            assert not bool(got[2][:, zp].any())
        # with an upstream gradient on those pairs only, every grad_x entry is a product with the zero field, but the
        # field's own: exactly 0
        only = torch.zeros_like(up)
        only[:, zp] = up[:, zp]
        _, dx = _run_with_upstream(c, inputs, only, dev)
        others = [f for f in range(c.F) if f != z]
        assert not bool(dx[:, others].any()) and bool(dx[:, z].any())
    if c.data == 'zero_rows':
        rows = S.ZERO_ROWS(c.B)
        assert not bool(got[1][rows].any()) and bool(got[1].any())
    if c.data == 'afm_flat':
        assert not bool(got[2].any()) and not bool(got[3].any())         # grad_Wa, grad_ba: every term has a factor pv = 0


# ---- refusals --------------------------------------------------------------------------------------------------------------
def _dev_inputs(c, dev):
    inputs, up = S.build_inputs(c)
    return [None if t is None else t.float().to(dev).requires_grad_(True) for t in inputs], up.float().to(dev)


def _refused_in_backward(c, dev, match):
    """the forward succeeds, backward() raises and leaves no gradient behind"""
    from deeptables_amd._lib import DtHipError
    xs, up = _dev_inputs(c, dev)
    out = S.gpu_fn(c)(*xs)
    torch.cuda.synchronize()
    assert out.shape == tuple(S.out_shape(c)) and bool(torch.isfinite(out).all())
    with pytest.raises(DtHipError, match=match):
        out.backward(up)
    torch.cuda.synchronize()
    assert all(t is None or t.grad is None for t in xs)


def test_refusal_afm_attention_factor_65(dev):
    from deeptables_amd._lib import DtHipError
    xs, _ = _dev_inputs(S.case('H65', 'afm', 3, 4, 8, 65, 'relu'), dev)
    with pytest.raises(DtHipError, match=r'dt_afm_fwd: attention factor 65 > 64'):
        S.gpu_fn(S.case('H65', 'afm', 3, 4, 8, 65, 'relu'))(*xs)


@pytest.mark.parametrize('kind,match', [('outer_mat', r'dt_outer_product_bwd\(mat\): D=65 too large'),
                                        ('bil_field_all', r'dt_bilinear_bwd: D=65 > 64')])
def test_refusal_d65_forward_runs_backward_refuses(dev, kind, match):
    """the generic forward fits its LDS tile up to D = 78; the weight-gradient kernels hold 16 accumulators per thread,
    D * D <= 4096 (DESIGN.md names the limit)"""
    _refused_in_backward(S.case('D65', kind, 3, 3, 65), dev, match)


def test_refusal_outer_vec_backward_lds(dev):
    """(F, D) = (26, 40): the forward needs 18,372 B, the backward's rows + kernel gradient 73,840 B > 64 KiB"""
    _refused_in_backward(S.case('F26-D40', 'outer_vec', 2, 26, 40), dev,
                         r'dt_outer_product_bwd\(vec\): F=26 D=40 needs 73840 B of LDS')


def test_refusal_afm_backward_lds(dev):
    """(F, D, H) = (40, 64, 64): P = 780 pairs of datt, bi and dbi rows, 646,496 B against the 150 KiB bound; the forward
    keeps one row and one score per pair and runs"""
    assert S.afm_lds_bwd(40, 64, 64) == 646496
    _refused_in_backward(S.case('F40-D64-H64', 'afm', 2, 40, 64, 64, 'tanh'), dev,
                         r'dt_afm_bwd: F=40 D=64 H=64 needs 646496 B of LDS')


# ---- layout ----------------------------------------------------------------------------------------------------------------
LAYOUT = S.params_of([S.BY_ID[i] for i in S.LAYOUT_IDS])


@pytest.mark.parametrize('view', ['every_other_field', 'permuted_FBD'])
@pytest.mark.parametrize('c', LAYOUT)
def test_noncontiguous_x(dev, c, view):
    inputs, up, refs, scales = S.references(c)
    x = inputs[0].float().to(dev)
    if view == 'every_other_field':
        base = torch.full((c.B, 2 * c.F, c.D), 1e6, device=dev)
        base[:, ::2] = x
        base.requires_grad_(True)
        xv = base[:, ::2]
    else:
        base = x.permute(1, 0, 2).contiguous().requires_grad_(True)      # [F, B, D]
        xv = base.permute(1, 0, 2)
    assert not xv.is_contiguous() and xv.shape == x.shape
    ps = [None if t is None else t.float().to(dev).requires_grad_(True) for t in inputs[1:]]
    out = S.gpu_fn(c)(xv, *ps)
    out.backward(up.float().to(dev))
    if view == 'every_other_field':
        assert not bool(base.grad[:, 1::2].any())
        dx = base.grad[:, ::2]
    else:
        dx = base.grad.permute(1, 0, 2)
    got = [out.detach(), dx] + [None if t is None else t.grad for t in ps]
    P.check_step(f'layout:{view}[{c.id}]', S.KERNEL_OF[c.kind], 'float32', S.figures(c, got, refs[F64], refs[F32], scales))


@pytest.mark.parametrize('c', LAYOUT)
def test_stride0_upstream_gradient(dev, c):
    """out.sum().backward(): the gradient arrives as the expansion of one element, every stride 0"""
    inputs, _ = S.build_inputs(c)
    ones = torch.ones(S.out_shape(c), dtype=F64)
    r64, r32 = (S.run_reference(c, inputs, ones, dt) for dt in (F64, F32))
    xs = [None if t is None else t.float().to(dev).requires_grad_(True) for t in inputs]
    out = S.gpu_fn(c)(*xs)
    out.sum().backward()
    got = [out.detach()] + [None if t is None else t.grad for t in xs]
    P.check_step(f'layout:stride0[{c.id}]', S.KERNEL_OF[c.kind], 'float32', S.figures(c, got, r64, r32))


GRAD_VIEW = S.params_of([S.BY_ID[i] for i in S.LAYOUT_IDS if S.BY_ID[i].kind.startswith(('outer', 'bil'))])


@pytest.mark.parametrize('c', GRAD_VIEW)
def test_parameter_gradient_lands_in_its_flat_view(dev, c):
    """a parameter of a model whose dense weights were flattened (training.flatten_dense_parameters) carries _dt_grad_view, a
    view into the model's one flat gradient buffer, as its .grad: the kernel adds on top of what is there, .grad stays the
    view, and the buffer's neighbours are not touched"""
    inputs, up, refs, _ = S.references(c)
    x = inputs[0].float().to(dev).requires_grad_(True)
    w = inputs[1].float().to(dev).requires_grad_(True)
    g = torch.Generator().manual_seed(5)
    before = S.rnd(g, tuple(w.shape))
    pad = 8
    flat = torch.full((w.numel() + 2 * pad,), -7.0, device=dev)
    view = flat[pad:pad + w.numel()].view(w.shape)
    view.copy_(before.float())
    w.grad = view
    w._dt_grad_view = view
    out = S.gpu_fn(c)(x, w)
    out.backward(up.float().to(dev))
    assert w.grad is not None and w.grad.data_ptr() == view.data_ptr() and w.grad.shape == view.shape
    assert torch.equal(flat[:pad], torch.full((pad,), -7.0, device=dev))
    assert torch.equal(flat[-pad:], torch.full((pad,), -7.0, device=dev))
    want64, want32 = refs[F64][2] + before, refs[F32][2] + before.float()
    m = P.row_rel
    P.check_step(f'grad_view[{c.id}]', S.KERNEL_OF[c.kind], 'float32',
                 {S.figure_names(c)[2]: ('bwd', m(view, want64), m(want32, want64))})


# ---- repeatability ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', S.params_of([S.BY_ID[i] for i in S.REPEAT_IDS]))
def test_repeatable(dev, c):
    """no atomic feeds the forward or grad_x: two runs agree bit for bit.  The parameter gradients meet through float atomics
    (LDS and global, across blocks and batch splits) in the order the hardware serves them, so they are held to the bar and
    not to each other."""
    a, _ = S.check_case('repeatable', c, dev)
    b, _ = S.check_case('repeatable', c, dev)
    assert torch.equal(a[0], b[0]), 'forward'
    assert torch.equal(a[1], b[1]), 'grad_x'
