# -*- coding:utf-8 -*-
"""GPU: the SENET helpers of csrc/interaction.hip (k_field_pool_fwd / _bwd, k_field_scale, k_field_scale_bwd_a) against
float64 torch (mean(-1), max(-1).values, x * a[..., None]), held to the fp32 class (tests/precision.py, yardstick B).

Launch edges: k_field_pool_fwd and k_field_scale_bwd_a run one thread per field in blocks of 256 (B * F = 255, 256, 257);
k_field_pool_bwd and k_field_scale stride over a grid capped at 4096 blocks of 256 threads (2521 x 26 x 16 = 1,048,736
elements: a second trip for 160 of them).  max pooling sends the whole gradient of a field to the FIRST of its maxima
(`p[d] > m` is strict), where torch splits it among ties: the comparison with torch draws inputs without ties, and
test_max_pool_ties pins the kernel's own rule.

MI355X, the largest err_gpu / max(err_f32, 2^-24) per figure (bar 12; DT_PRECISION_LOG): field_pool z 5.13 (mean, summed in
order where torch sums pairwise), dx 0.95; field_scale out 0.99, dx 0.99, da 1.86; strided x and gradient: 1.32 / 0.65 and
0.90 / 0.91 / 1.39."""
import pytest
import torch

from tests.test_precision_gpu import _layer_vs_float32, _rnd

pytestmark = pytest.mark.gpu

EDGES = [pytest.param(51, 5, id='BF255-one_block_one_thread_idle'), pytest.param(32, 8, id='BF256-one_full_block'),
         pytest.param(257, 1, id='BF257-second_block_one_thread')]
BIG = pytest.param(2521, 26, 16, id='1048736_elements-second_grid_stride_trip')
SHAPES = [pytest.param(*p.values, D, id=f'{p.id}-D{D}') for p in EDGES for D in (1, 3, 16, 33)] + [BIG]


def _untied(g, shape):
    """randn in float32-exact float64 whose fields (last axis) have one maximum each, and say so"""
    x = _rnd(g, shape)
    if shape[-1] > 1:
        top = x.topk(2, dim=-1).values
        assert bool((top[..., 0] > top[..., 1]).all()), 'a tie among the maxima: draw again with another seed'
    return x


def _refs(op):
    return (lambda t: t.mean(-1)) if op == 'mean' else (lambda t: t.max(-1).values)


@pytest.mark.parametrize('op', ['mean', 'max'])
@pytest.mark.parametrize('B,F,D', SHAPES)
def test_field_pool(dev, B, F, D, op):
    from deeptables_amd import ops
    g = torch.Generator().manual_seed(B + 3 * F + 7 * D)
    x = _untied(g, (B, F, D))
    _layer_vs_float32(f'field_pool[{op},{B},{F},{D}]', 'field_pool', lambda t: ops.field_pool(t, op), _refs(op), [x],
                      _rnd(g, (B, F)), dev)


@pytest.mark.parametrize('a_rank', [3, 2])
@pytest.mark.parametrize('B,F,D', SHAPES)
def test_field_scale(dev, B, F, D, a_rank):
    """a as [B, F, 1] (what the SENET excitation hands over) and as [B, F]; its gradient comes back in the same shape"""
    from deeptables_amd import ops
    g = torch.Generator().manual_seed(2 * B + F + 5 * D)
    x, a = _rnd(g, (B, F, D)), _rnd(g, (B, F, 1) if a_rank == 3 else (B, F))
    ref = (lambda t, s: t * s) if a_rank == 3 else (lambda t, s: t * s[..., None])
    _layer_vs_float32(f'field_scale[{a_rank},{B},{F},{D}]', 'field_scale', ops.field_scale, ref, [x, a],
                      _rnd(g, (B, F, D)), dev)


def _strided(fn, seen):
    """fn on an x that is every second element of a wider tensor, its result handed on through a slice of a stack so that
    the upstream gradient arrives as a strided view too (asserted in `seen`)"""
    def run(t, *rest):
        wide = torch.stack([t, torch.full_like(t, 1e6)], -1).flatten(-2)
        xs = wide[..., ::2]
        assert not xs.is_contiguous()
        out = fn(xs, *rest)
        out.register_hook(lambda gr: seen.append(gr.is_contiguous()))
        return torch.stack([out, torch.full_like(out, 1e6).detach()], -1)[..., 0]
    return run


@pytest.mark.parametrize('B,F,D', [(51, 5, 3), (32, 8, 16)])
def test_noncontiguous_x_and_upstream_gradient(dev, B, F, D):
    from deeptables_amd import ops
    g = torch.Generator().manual_seed(B + F + D)
    x, a = _untied(g, (B, F, D)), _rnd(g, (B, F, 1))
    for op in ('mean', 'max'):
        seen = []
        _layer_vs_float32(f'field_pool_strided[{op},{B},{F},{D}]', 'field_pool', _strided(lambda t: ops.field_pool(t, op), seen),
                          _refs(op), [x], _rnd(g, (B, F)), dev)
        assert seen == [False]
    seen = []
    _layer_vs_float32(f'field_scale_strided[{B},{F},{D}]', 'field_scale', _strided(ops.field_scale, seen),
                      lambda t, s: t * s, [x, a], _rnd(g, (B, F, D)), dev)
    assert seen == [False]


def test_max_pool_ties(dev):
    """what k_field_pool_fwd documents for ties: the value is the maximum, the whole gradient of the field lands on one
    element that holds it, the first such one, and the field's gradient sums to gz"""
    from deeptables_amd import ops
    x = torch.tensor([[[1.0, 3.0, -2.0, 3.0, 0.5],        # two equal maxima: index 1 wins over 3
                       [0.0, 0.0, 0.0, 0.0, 0.0],         # an all-zero field, as an out-of-range id produces: index 0
                       [-1.0, -1.0, -4.0, -1.0, -1.0],    # negative maxima, four of them
                       [2.0, 2.0, 2.0, 2.0, 7.0]],        # ties below the maximum do not matter: index 4
                      [[5.0, 5.0, 5.0, 5.0, 5.0],
                       [-0.0, 0.0, -0.0, 0.0, -0.0],      # -0 == 0: still the first
                       [0.0, 1.0, 1.0, 0.0, 1.0],
                       [9.0, -9.0, 9.0, -9.0, 9.0]]])
    first = torch.tensor([[1, 0, 0, 4], [0, 0, 1, 0]])
    gz = torch.tensor([[1.5, -2.0, 0.25, 3.0], [-1.0, 4.0, 0.5, -8.0]])
    xd = x.to(dev).requires_grad_(True)
    z = ops.field_pool(xd, 'max')
    z.backward(gz.to(dev))
    gx = xd.grad.cpu()
    assert torch.equal(z.detach().cpu(), x.max(-1).values)
    expect = torch.zeros_like(x).scatter_(-1, first[..., None], gz[..., None])
    assert torch.equal(gx, expect)
    assert torch.equal((gx != 0).sum(-1), torch.ones(2, 4, dtype=torch.long))
    assert bool((x.gather(-1, gx.abs().argmax(-1, keepdim=True))[..., 0] == x.max(-1).values).all())
    assert torch.equal(gx.sum(-1), gz)
    # D = 1: every field is its own maximum
    x1 = torch.tensor([[[2.0], [0.0], [-3.0]]])
    x1d = x1.to(dev).requires_grad_(True)
    z1 = ops.field_pool(x1d, 'max')
    z1.backward(torch.tensor([[1.0, 2.0, 3.0]], device=dev))
    assert torch.equal(z1.detach().cpu(), x1[..., 0]) and torch.equal(x1d.grad.cpu(), torch.tensor([[[1.0], [2.0], [3.0]]]))


def test_empty_batch(dev):
    from deeptables_amd import ops
    F, D = 5, 16
    for op in ('mean', 'max'):
        x = torch.empty((0, F, D), device=dev, requires_grad=True)
        z = ops.field_pool(x, op)
        assert z.shape == (0, F) and z.dtype == torch.float32
        z.sum().backward()
        assert x.grad.shape == (0, F, D)
    for a_shape in ((0, F, 1), (0, F)):
        x = torch.empty((0, F, D), device=dev, requires_grad=True)
        a = torch.empty(a_shape, device=dev, requires_grad=True)
        out = ops.field_scale(x, a)
        assert out.shape == (0, F, D)
        out.sum().backward()
        assert x.grad.shape == (0, F, D) and a.grad.shape == a_shape
    torch.cuda.synchronize()


@pytest.mark.parametrize('B,F,D', [(257, 1, 33), (2521, 26, 16)])
def test_deterministic(dev, B, F, D):
    from deeptables_amd import ops
    g = torch.Generator().manual_seed(B)
    x, a, up, upz = (torch.randn(s, generator=g).to(dev) for s in ((B, F, D), (B, F, 1), (B, F, D), (B, F)))
    runs = []
    for _ in range(2):
        res = []
        for op in ('mean', 'max'):
            xd = x.clone().requires_grad_(True)
            z = ops.field_pool(xd, op)
            z.backward(upz)
            res += [z.detach(), xd.grad]
        xd, ad = x.clone().requires_grad_(True), a.clone().requires_grad_(True)
        out = ops.field_scale(xd, ad)
        out.backward(up)
        runs.append(res + [out.detach(), xd.grad, ad.grad])
    assert all(torch.equal(p, q) for p, q in zip(*runs))
