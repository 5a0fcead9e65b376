# -*- coding:utf-8 -*-
"""GPU: the FGCNN convolution + activation + max-pooling kernels (csrc/fgcnn_train.hip) against
oracle.reference_layers.fgcnn in float64, held to the fp32 class of tests/precision.py in both directions.

  single product (activation linear, pool 1): cond_rms of z, grad_x, grad_kernel, grad_bias against |A| |B| within
      COND_BAR['fp32'] (yardstick A);
  composed kernel (tanh / relu / sigmoid with pooling): the error against float64 within STEP_BAR['fp32'] x the float32 CPU
      oracle's own error in the same metric (gpu_errors), floored at FLOOR (yardstick B); relu units masked with
      kink_mask(.., 'fp32').

Near ties: a window whose two largest float64 pre-activations lie closer than 2^-18 |A| |B| (4 x KINK_TOL['fp32']) may
legitimately select either field, so every reference asserts — on the oracle alone, before the GPU is touched — that its
inputs contain no such window (|A| |B| taken as the largest of the window: the stricter reading).  The seeds below were
picked on the CPU so that this holds; it is a condition of the test, not a measurement.

Shapes (F, D, C, filters, h, pool): the smallest at which each path can go wrong, see SHAPES."""
import functools
import os

import pytest
import torch

from tests import precision as P

pytestmark = pytest.mark.gpu

TIE_TOL = 4 * P.KINK_TOL['fp32']                # 2^-18
B0 = 40
SHAPES = {
    (1, 1, 1, 1, 1, 1): 1,                      # the degenerate shape
    (5, 6, 2, 4, 3, 2): 1,                      # D no power of two, an odd F with a trailing pool pad
    (9, 4, 1, 3, 4, 3): 1,                      # even h: asymmetric convolution padding
    (7, 4, 3, 5, 7, 3): 1,                      # h = F: every tap window leaves the map; qb = 1: window 0 starts before it
    (2, 4, 2, 3, 3, 3): 1,                      # pool > F: one window
    (3, 4, 16, 16, 16, 8): 1,                   # every limit at once
    (26, 16, 1, 14, 7, 2): 1,                   # benchmark block 1
    (13, 16, 14, 16, 7, 2): 1,                  # benchmark block 2
}                                               # value: the seed (no near tie, checked by the reference itself)
SMALL = (3, 4, 1, 2, 3, 2)                      # the smallest map: the batch edges run on it
SMALL_SEEDS = {1: 1, 23: 1, 33: 1, 11265: 1, 16385: 1}             # batch size -> seed; another batch size (_small_batches) finds its own
ACTS = ['tanh', 'relu', 'sigmoid']


def _rnd(g, shape, scale=1.0):
    """float64 values that float32 holds exactly: the kernels and the reference see the same inputs"""
    return (torch.randn(shape, generator=g, dtype=torch.float64) * scale).float().double()


def _oracle_pooled(x, k, b, pool, act):
    """oracle.reference_layers.fgcnn up to its pooled map (the recombination Dense gets a zero weight, one new filter)"""
    from oracle import reference_layers as R
    B, F, D, _ = x.shape
    K = -(-F // pool) * D * k.shape[3]
    return R.fgcnn(x, k, b, torch.zeros(K, F * D, dtype=x.dtype), torch.zeros(F * D, dtype=x.dtype), pool, 1, act)[0]


def _windows(t, F, pool, fill):
    """[B,F,D,O] -> [B,Fp,pool,D,O] with Keras' 'same' pooling pads set to `fill`"""
    Fp = -(-F // pool)
    total = Fp * pool - F
    qb, qa = total // 2, total - total // 2
    t = torch.nn.functional.pad(t, (0, 0, 0, 0, qb, qa), value=fill)
    return t.reshape(t.shape[0], Fp, pool, t.shape[2], t.shape[3])


@functools.lru_cache(maxsize=None)
def reference(shape, B, act, pool, seed):
    """inputs, the float64 oracle forward / backward, the float32 oracle's own error and the |A| |B| scales; computed once
    per case and shared (read-only) by the tests that need it"""
    F, D, C, filters, h, _ = shape
    g = torch.Generator().manual_seed(seed)
    x, k = _rnd(g, (B, F, D, C)), _rnd(g, (h, 1, C, filters), (h * C) ** -0.5)
    b = _rnd(g, (filters,), 0.3)
    lin = lambda x_, k_, b_: _oracle_pooled(x_, k_, b_, 1, None)
    z = lin(x, k, b)
    s_z = P.abs_forward(lin, (x, k, b))
    Fp = -(-F // pool)
    # the condition of the test: no window whose two largest pre-activations are a near tie
    zw, sw = _windows(z, F, pool, float('-inf')), _windows(s_z, F, pool, 0.0).amax(2)
    if pool > 1:
        top = zw.topk(2, dim=2).values
        near = (top[:, :, 0] - top[:, :, 1]) < TIE_TOL * sw
        assert not bool(near.any()), f'{shape} B={B} seed={seed}: {int(near.sum())} near-tie windows, pick another seed'
    pre = zw.amax(2)                                                    # [B,Fp,D,O]: the pooled pre-activation
    up = P.kink_mask(pre, sw, _rnd(g, (B, Fp, D, filters)), act, 'fp32')
    out = {}
    for name, dt in (('f64', torch.float64), ('f32', torch.float32)):
        xr, kr, br = (t.to(dt).clone().requires_grad_(True) for t in (x, k, b))
        y = _oracle_pooled(xr, kr, br, pool, act)
        (y * up.to(dt)).sum().backward()
        out[name] = dict(y=y.detach().double(), dx=xr.grad.double(), dk=kr.grad.double(), db=br.grad.double())
    r = dict(x=x, k=k, b=b, up=up, s_z=s_z, **out['f64'])
    # |A| |B| of the three backward contractions: the float64 gradient at z — `up` act'(y) at the one field every window
    # selects (unique: no near tie), zero elsewhere — sent through the convolution's backward on absolute values
    y = r['y']
    slope = {None: torch.ones_like(y), 'linear': torch.ones_like(y), 'relu': (pre > 0).double(), 'sigmoid': y * (1 - y),
             'tanh': 1 - y * y}[act]
    dzw = torch.zeros_like(zw).scatter_(2, zw.argmax(2, keepdim=True), (up * slope).unsqueeze(2))
    qb = (Fp * pool - F) // 2
    dz = dzw.reshape(B, Fp * pool, D, filters)[:, qb:qb + F]
    xr, kr, br = (t.clone().requires_grad_(True) for t in (x, k, b))
    (lin(xr, kr, br) * dz).sum().backward()                             # the derivation above, checked against the oracle
    for got, want in ((xr.grad, r['dx']), (kr.grad, r['dk']), (br.grad, r['db'])):
        assert (got - want).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item())
    _, (r['s_x'], r['s_k'], r['s_b']) = P.abs_scale(lin, (x, k, b), dz)
    r['f32'] = {'y': P.l2_rel(out['f32']['y'], r['y']), **{n: P.cond_rms(out['f32'][n], r[n], r[s_])
                                                         for n, s_ in (('dx', 's_x'), ('dk', 's_k'), ('db', 's_b'))}}
    return r


def gpu_errors(got, r):
    """the metrics of yardstick B here: l2_rel for the pooled map (an activation's output, nothing cancels); for the three
    gradients the root mean square of |e| / (|A| |B|) — a gradient with few elements (the degenerate shape's kernel
    gradient is ONE number, a sum of 40 terms that cancel to 1 / 66 of their absolute sum) has no relative error two fp32
    evaluations agree on, while its error in units of |A| |B| is what the fp32 class bounds"""
    return {'y': P.l2_rel(got['y'], r['y']), 'dx': P.cond_rms(got['dx'], r['dx'], r['s_x']),
            'dk': P.cond_rms(got['dk'], r['dk'], r['s_k']), 'db': P.cond_rms(got['db'], r['db'], r['s_b'])}


def run_gpu(dev, r, act, pool, need_x=True):
    from deeptables_amd import ops
    xg = r['x'].float().to(dev).requires_grad_(need_x)
    kg, bg = r['k'].float().to(dev).requires_grad_(True), r['b'].float().to(dev).requires_grad_(True)
    assert ops.fgcnn_conv_pool_supported(xg, kg, act, pool)
    y = ops.fgcnn_conv_pool(xg, kg, bg, act, pool)
    (y * r['up'].float().to(dev)).sum().backward()
    torch.cuda.synchronize()
    return dict(y=y.detach(), dx=xg.grad, dk=kg.grad, db=bg.grad)


def check_composed(dev, name, shape, B, act, seed):
    pool = shape[5]
    r = reference(shape, B, act, pool, seed)
    got = run_gpu(dev, r, act, pool)
    err = gpu_errors(got, r)
    figs = {n: ('fwd' if n == 'y' else 'bwd', err[n], r['f32'][n]) for n in ('y', 'dx', 'dk', 'db')}
    ratios = {n: g_ / max(f_, P.FLOOR) for n, (_, g_, f_) in figs.items()}
    print(f'{name}: err_gpu / max(err_f32, 2^-24):', {n: round(v, 3) for n, v in ratios.items()},
          ' err_gpu:', {n: f'{g_:.2e}' for n, (_, g_, _) in figs.items()})
    P.record(name, **ratios)
    bad = {n: (ratios[n], figs[n][1], figs[n][2]) for n in ratios if not ratios[n] <= P.STEP_BAR['fp32']}
    assert not bad, f'{name}: err_gpu / max(err_f32, 2^-24) over {P.STEP_BAR["fp32"]} (ratio, err_gpu, err_f32): {bad}'


@pytest.mark.parametrize('shape', list(SHAPES))
def test_single_product_is_fp32_class(dev, shape):
    """activation linear, pool 1: pooled is z itself, every output one contraction"""
    r = reference(shape, B0, 'linear', 1, SHAPES[shape])
    got = run_gpu(dev, r, 'linear', 1)
    figs = {'z': P.cond_rms(got['y'], r['y'], r['s_z']), 'grad_x': P.cond_rms(got['dx'], r['dx'], r['s_x']),
            'grad_kernel': P.cond_rms(got['dk'], r['dk'], r['s_k']), 'grad_bias': P.cond_rms(got['db'], r['db'], r['s_b'])}
    print(f'fgcnn_conv{list(shape)} cond_rms / 2^-24:', {n: round(v / P.U, 3) for n, v in figs.items()})
    P.record(f'fgcnn_conv_single{list(shape)}', **{n: v / P.U for n, v in figs.items()})
    bad = {n: v / P.U for n, v in figs.items() if not v <= P.COND_BAR['fp32']}
    assert not bad, f'cond_rms in units of 2^-24 over {P.COND_BAR["fp32"] / P.U}: {bad}'


@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('shape', list(SHAPES))
def test_composed_kernel_is_fp32_class(dev, shape, act):
    check_composed(dev, f'fgcnn_conv_pool{list(shape)}[{act}]', shape, B0, act, SHAPES[shape])


def _launch_geometry(backward):
    """(tile rows, grid cap) of the forward or the backward launch on the smallest map, from dt_fg_conv_pool_geometry; the
    backward's are cross-checked against the workspace query (one partial per block: its size over a partial's is the grid)"""
    import ctypes
    from deeptables_amd._lib import lib
    F, D, C, filters, h, pool = SMALL
    rows, cap = ctypes.c_int(0), ctypes.c_int(0)
    assert lib().dt_fg_conv_pool_geometry(F, D, C, filters, h, pool, int(backward), ctypes.byref(rows), ctypes.byref(cap)) == 0
    rows, cap = rows.value, cap.value
    assert 1 <= rows <= 64 and 1 < cap <= 4096
    if backward:
        per_block = 4 * (h * C * filters + filters)
        blocks = lambda B: lib().dt_fg_conv_pool_workspace_bytes(B, F, D, C, filters, h, pool) // per_block
        assert blocks(rows) == 1 and blocks(rows + 1) == 2 and blocks(rows * cap) == cap and blocks(rows * cap + 1) == cap
    return rows, cap


def _small_batches():
    """the batch edges of BOTH launches: their tiles differ (the forward has no dz in LDS), so each has its own
    'one row more than a tile' and its own 'more tiles than blocks' — where a block runs its grid-stride loop a second
    time"""
    (fr, fc), (br, bc) = _launch_geometry(False), _launch_geometry(True)
    return {'one': 1, 'bwd_tile_plus_one': br + 1, 'fwd_tile_plus_one': fr + 1, 'bwd_more_tiles_than_blocks': br * bc + 1,
            'fwd_more_tiles_than_blocks': fr * fc + 1}


def _small_seed(B):
    """the first seed whose inputs have no near-tie window at this batch size (the reference asserts it)"""
    if B not in SMALL_SEEDS:
        for seed in range(1, 40):
            try:
                reference(SMALL, B, 'tanh', SMALL[5], seed)
            except AssertionError:
                continue
            SMALL_SEEDS[B] = seed
            break
    return SMALL_SEEDS[B]


@pytest.mark.parametrize('edge', ['one', 'bwd_tile_plus_one', 'fwd_tile_plus_one', 'bwd_more_tiles_than_blocks',
                                  'fwd_more_tiles_than_blocks'])
def test_batch_edges(dev, edge):
    B = _small_batches()[edge]
    check_composed(dev, f'fgcnn_conv_pool{list(SMALL)}[tanh,B={edge}]', SMALL, B, 'tanh', _small_seed(B))


# ---------------------------------------------------------------------------------------------
# the C ABI directly: the tie rule, the pointer variants, determinism
# ---------------------------------------------------------------------------------------------
def _fwd(dev, x, k, b, shape, act, want_sel=True):
    from deeptables_amd import _lib
    from deeptables_amd._lib import check, ptr, stream_ptr
    F, D, C, filters, h, pool = shape
    B, Fp = x.shape[0], -(-F // pool)
    pooled = torch.full((B, Fp, D, filters), float('nan'), dtype=torch.float32, device=dev)
    sel = torch.full((B, Fp, D, filters), 255, dtype=torch.uint8, device=dev) if want_sel else None
    check(_lib.lib().dt_fg_conv_pool_fwd(ptr(x), ptr(k), ptr(b), B, F, D, C, filters, h, pool, _lib.ACT_CODES[act],
                                            ptr(pooled), ptr(sel), stream_ptr()), 'dt_fg_conv_pool_fwd')
    torch.cuda.synchronize()
    return pooled, sel


def _bwd(dev, x, k, pooled, sel, gp, shape, act, want_x=True, want_b=True):
    from deeptables_amd import _lib
    from deeptables_amd._lib import check, ptr, stream_ptr
    F, D, C, filters, h, pool = shape
    B = x.shape[0]
    nan = float('nan')
    gx = torch.full(x.shape, nan, dtype=torch.float32, device=dev) if want_x else None
    gk = torch.full(k.shape, nan, dtype=torch.float32, device=dev)
    gb = torch.full((filters,), nan, dtype=torch.float32, device=dev) if want_b else None
    nbytes = _lib.lib().dt_fg_conv_pool_workspace_bytes(B, F, D, C, filters, h, pool)
    assert nbytes > 0
    ws = torch.full((nbytes // 4,), nan, dtype=torch.float32, device=dev)
    check(_lib.lib().dt_fg_conv_pool_bwd(ptr(x), ptr(k), ptr(pooled), ptr(sel), ptr(gp), B, F, D, C, filters, h, pool,
                                            _lib.ACT_CODES[act], ptr(gx), ptr(gk), ptr(gb), ptr(ws), stream_ptr()),
          'dt_fg_conv_pool_bwd')
    torch.cuda.synchronize()
    return gx, gk, gb


def test_ties_go_to_the_first_field_closed_form(dev):
    """a zero kernel and a nonzero bias: every z of a window ties.  sel, pooled and all three gradients in closed form."""
    shape = F, D, C, filters, h, pool = (7, 4, 3, 5, 7, 3)              # qb = 1: window 0 is fields {0, 1} at offsets {1, 2}
    B, Fp, qb, pb = 6, 3, 1, 3
    g = torch.Generator().manual_seed(11)
    x, b, gp = _rnd(g, (B, F, D, C)), _rnd(g, (filters,), 0.5), _rnd(g, (B, Fp, D, filters))
    assert bool((b != 0).all())
    xg, kg = x.float().to(dev), torch.zeros(h, 1, C, filters, device=dev)
    pooled, sel = _fwd(dev, xg, kg, b.float().to(dev), shape, 'tanh')
    want_sel = torch.zeros(B, Fp, D, filters, dtype=torch.uint8)
    want_sel[:, 0] = qb                                                 # the first in-map offset of the window before the map
    assert torch.equal(sel.cpu(), want_sel)
    y = torch.tanh(b.float()).expand(B, Fp, D, filters)
    assert (pooled.cpu().double() - y.double()).abs().max().item() <= 4 * P.U
    gx, gk, gb = _bwd(dev, xg, kg, pooled, sel, gp.float().to(dev), shape, 'tanh')
    assert torch.equal(gx.cpu(), torch.zeros(B, F, D, C))               # a zero kernel sends nothing back
    dz = gp * (1 - pooled.cpu().double() ** 2)                          # at field i pool - qb + sel of window i
    field = [i * pool - qb + int(want_sel[0, i, 0, 0]) for i in range(Fp)]
    assert field == [0, 2, 5]
    want_k, scale_k = torch.zeros(h, C, filters, dtype=torch.float64), torch.zeros(h, C, filters, dtype=torch.float64)
    for i, f in enumerate(field):
        for t in range(h):
            ff = f + t - pb
            if 0 <= ff < F:
                want_k[t] += torch.einsum('bdc,bdo->co', x[:, ff], dz[:, i])
                scale_k[t] += torch.einsum('bdc,bdo->co', x[:, ff].abs(), dz[:, i].abs())
    assert P.cond_rms(gk.reshape(h, C, filters), want_k, scale_k) <= P.COND_BAR['fp32']
    assert P.cond_rms(gb, dz.sum((0, 1, 2)), dz.abs().sum((0, 1, 2))) <= P.COND_BAR['fp32']


def test_a_nan_pre_activation_makes_the_window_nan(dev):
    """as torch.amax in the unfold path: a NaN in the map reaches every window one of whose fields has it among its taps,
    whichever position of the window that field has — and no other window"""
    from oracle import reference_layers as R
    shape = F, D, C, filters, h, pool = (9, 4, 1, 3, 3, 3)
    g = torch.Generator().manual_seed(5)
    x, k, b = _rnd(g, (4, F, D, C)), _rnd(g, (h, 1, C, filters), 0.5), _rnd(g, (filters,), 0.3)
    x[0, 0, 0, 0] = x[1, 4, 1, 0] = x[2, 8, 2, 0] = x[3, 5, 3, 0] = float('nan')
    want = torch.isnan(_oracle_pooled(x, k, b, pool, 'tanh'))
    assert bool(want.any()) and not bool(want.all())
    pooled, _ = _fwd(dev, x.float().to(dev), k.float().to(dev), b.float().to(dev), shape, 'tanh')
    assert torch.equal(torch.isnan(pooled).cpu(), want)


def test_pointer_variants_and_determinism(dev):
    """sel == NULL gives the same pooled; grad_x == NULL and grad_bias == NULL leave the other outputs unchanged; two
    backward calls are bit-identical — at a batch with more tiles than blocks in the forward AND the backward launch"""
    edges = _small_batches()
    B = max(edges['fwd_more_tiles_than_blocks'], edges['bwd_more_tiles_than_blocks'])     # both launches loop
    r = reference(SMALL, B, 'tanh', SMALL[5], _small_seed(B))
    x, k, b, gp = (r[n].float().to(dev) for n in ('x', 'k', 'b', 'up'))
    pooled, sel = _fwd(dev, x, k, b, SMALL, 'tanh')
    pooled2, _ = _fwd(dev, x, k, b, SMALL, 'tanh', want_sel=False)
    assert torch.equal(pooled, pooled2)
    gx, gk, gb = _bwd(dev, x, k, pooled, sel, gp, SMALL, 'tanh')
    for t in (gx, gk, gb):
        assert bool(torch.isfinite(t).all())                            # every output overwritten
    gx2, gk2, gb2 = _bwd(dev, x, k, pooled, sel, gp, SMALL, 'tanh')
    assert torch.equal(gk, gk2) and torch.equal(gb, gb2) and torch.equal(gx, gx2)
    _, gk3, gb3 = _bwd(dev, x, k, pooled, sel, gp, SMALL, 'tanh', want_x=False)
    assert torch.equal(gk, gk3) and torch.equal(gb, gb3)
    gx4, gk4, _ = _bwd(dev, x, k, pooled, sel, gp, SMALL, 'tanh', want_b=False)
    assert torch.equal(gk, gk4) and torch.equal(gx, gx4)


# ---------------------------------------------------------------------------------------------
# the layer and a model
# ---------------------------------------------------------------------------------------------
def _run_layer(dev, F, D, C, filters, h, pool, nf, B, switch):
    from deeptables_amd import functional
    from deeptables_amd.models import layers
    functional.set_seed(8)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(B, F, D, C, generator=g)
    layer = layers.FGCNN(filters=filters, kernel_height=h, new_filters=nf, pool_height=pool)
    layer.build((None, F, D, C))
    layer.to(dev)
    with torch.no_grad():
        layer.conv_bias.add_(torch.randn(filters, generator=g).to(dev) * 0.1)
    xg = x.to(dev).requires_grad_(True)
    old = os.environ.get('DT_AMD_FGCNN_CONV')
    os.environ['DT_AMD_FGCNN_CONV'] = switch
    try:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        pooled, newf = layer(xg)
        gp = torch.randn(pooled.shape, generator=g)
        gn = torch.randn(newf.shape, generator=g)
        (pooled * gp.to(dev)).sum().add((newf * gn.to(dev)).sum()).backward()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
    finally:
        if old is None:
            del os.environ['DT_AMD_FGCNN_CONV']
        else:
            os.environ['DT_AMD_FGCNN_CONV'] = old
    return dict(layer=layer, x=x, gp=gp, gn=gn, pooled=pooled.detach(), newf=newf.detach(), dx=xg.grad,
                dk=layer.conv_kernel.grad, db=layer.conv_bias.grad, dW=layer.dense_output.kernel.grad, peak=peak)


def _rel(a, b):
    b = b.double().cpu()
    return (a.detach().double().cpu() - b).abs().max().item() / max(b.abs().max().item(), 1e-12)


def _maxerr(a, b):
    return (a.detach().double().cpu() - b.double().cpu()).abs().max().item()


def test_layer_matches_the_unfold_path_and_the_oracle(dev, monkeypatch):
    from deeptables_amd import ops
    from oracle import reference_layers as R
    F, D, C, filters, h, pool, nf, B = 13, 8, 14, 16, 7, 2, 2, 32
    calls = []
    real = ops.fgcnn_conv_pool
    monkeypatch.setattr(ops, 'fgcnn_conv_pool', lambda *a: calls.append(1) or real(*a))
    new = _run_layer(dev, F, D, C, filters, h, pool, nf, B, '1')
    assert calls == [1]
    old = _run_layer(dev, F, D, C, filters, h, pool, nf, B, '0')
    assert calls == [1]                                                 # the switch keeps the unfold + Dense + amax path
    xd = new['x'].double().requires_grad_(True)
    L = new['layer']
    ws = [t.detach().cpu().double().requires_grad_(True) for t in
          (L.conv_kernel, L.conv_bias, L.dense_output.kernel, L.dense_output.bias)]
    rp, rn = R.fgcnn(xd, ws[0], ws[1], ws[2], ws[3], pool, nf)
    ((rp * new['gp'].double()).sum() + (rn * new['gn'].double()).sum()).backward()
    ref = dict(pooled=rp, newf=rn, dx=xd.grad, dk=ws[0].grad, db=ws[1].grad, dW=ws[2].grad)
    for name, run, other in (('kernels vs oracle', new, ref), ('unfold vs oracle', old, ref), ('kernels vs unfold', new, old)):
        figs = {'pooled': _maxerr(run['pooled'], other['pooled']), 'newf': _maxerr(run['newf'], other['newf']),
                **{n: _rel(run[n], other[n]) for n in ('dx', 'dk', 'db', 'dW')}}
        print(f'FGCNN layer, {name}:', {n: f'{v:.2e}' for n, v in figs.items()})
        assert figs['pooled'] < 1e-4 and figs['newf'] < 1e-4, (name, figs)
        assert all(figs[n] < 2e-4 for n in ('dx', 'dk', 'db', 'dW')), (name, figs)


def test_no_taps_matrix_is_allocated(dev):
    """block 2 of the benchmark preset, B = 256: the peak of forward + backward is lower than with the unfold path"""
    F, D, C, filters, h, pool, nf, B = 13, 16, 14, 16, 7, 2, 2, 256
    new = _run_layer(dev, F, D, C, filters, h, pool, nf, B, '1')
    old = _run_layer(dev, F, D, C, filters, h, pool, nf, B, '0')
    taps = B * F * D * h * C * 4
    print(f'peak bytes over the baseline: kernels {new["peak"]:,}, unfold path {old["peak"]:,}; one taps matrix is {taps:,}')
    assert new['peak'] < old['peak']


class _CallRecorder:
    """ops.lib() stand-in that forwards everything and notes (name, args) of every library call"""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        fn = getattr(self.real, name)

        def call(*args):
            self.calls.append((name, args))
            return fn(*args)
        return call


def test_fgcnn_dnn_model_trains_on_the_kernels(dev, monkeypatch):
    from deeptables_amd import functional, ops
    from deeptables_amd._lib import lib
    from deeptables_amd.models import ModelConfig, DeepModel
    from deeptables_amd.models.metainfo import CategoricalColumn, ContinuousColumn
    from oracle import bridge, reference_layers as R
    from tests.test_models_gpu import batch
    monkeypatch.delenv('DT_AMD_FGCNN_CONV', raising=False)
    F, D, Nd, B = 6, 8, 3, 32
    functional.set_seed(3)
    conf = ModelConfig(nets=['fgcnn_dnn_nets'], fixed_embedding_dim=True, embeddings_output_dim=D, embedding_dropout=0,
                       dense_dropout=0, metrics=['AUC'])
    cats = [CategoricalColumn(f'C{i}', 20 + i, D) for i in range(F)]
    conts = [ContinuousColumn('input_continuous_all', [f'I{j}' for j in range(Nd)])]
    dm = DeepModel('binary', 2, conf, cats, conts)
    dm.build()
    blocks = [l for l in dm.model.layers if l.__class__.__name__ == 'FGCNN']
    assert len(blocks) >= 1
    idx, dense, y = batch(cats, Nd, B, dev)
    w = bridge.oracle_weights(dm, requires_grad=True)
    ref_logit, _ = bridge.oracle_forward(dm, idx, dense, training=True, weights=w)
    R.binary_crossentropy_from_logits(ref_logit, y.double()).backward()
    rec = _CallRecorder(lib())
    monkeypatch.setattr(ops, 'lib', lambda: rec)
    dm.model.train()
    dm.optimizer.zero_grad()
    logit = dm.model([idx.int().to(dev), dense.to(dev)])
    dm._loss(logit, y.to(dev)).backward()
    torch.cuda.synchronize()
    names = [n for n, _ in rec.calls]
    assert names.count('dt_fg_conv_pool_fwd') == len(blocks) and names.count('dt_fg_conv_pool_bwd') == len(blocks)
    # the taps GEMM had B F D rows (F the block's own field count): no Dense launch of that height is left
    taps_rows, Fk = set(), F
    for l in blocks:
        taps_rows.add(B * Fk * D)
        Fk = -(-Fk // l.pool_height)
    # N follows act: (x, W, bias, act, N, ..) forward, (x, W, y, grad_y, act, N, ..) backward
    dense_rows = [(n, a[5] if n.endswith('_bwd') else a[4]) for n, a in rec.calls
                  if n in ('dt_dense_fwd', 'dt_dense_bwd', 'dt_dense_tiled_fwd', 'dt_dense_tiled_bwd')]
    assert {B} <= {d[1] for d in dense_rows if d[0].endswith('_fwd')} and {B} <= {d[1] for d in dense_rows
                                                                                   if d[0].endswith('_bwd')}
    assert dense_rows and not [d for d in dense_rows if d[1] in taps_rows], dense_rows

    def rel(a, b):
        b = torch.as_tensor(b).double()
        return (a.detach().double().cpu().reshape(b.shape) - b).abs().max().item() / max(b.abs().max().item(), 1e-12)

    err = (logit.detach().double().cpu() - ref_logit.detach()).abs().max().item()
    figures = {'logit': err}
    for i, (p, wt) in enumerate(bridge.param_pairs(dm, w)):
        assert p.grad is not None and wt.grad is not None, f'pair {i} of shape {tuple(p.shape)} got no gradient'
        figures[f'grad[{i}]{tuple(p.shape)}'] = rel(p.grad, wt.grad)
    table = dm.model.layers_by_name['emb_categorical_vars_all'].tables[f'd{D}']
    assert table.grad is not None
    figures['grad[table]'] = rel(table.grad, torch.cat([t.grad for t in w['emb_categorical_vars_all']], 0))
    print('fgcnn_dnn_nets: ' + ', '.join(f'{k} {v:.2e}' for k, v in figures.items()))
    assert err < 1e-4, f'logit error {err}'
    bad = {k: v for k, v in figures.items() if k != 'logit' and not v < 2e-4}
    assert not bad, f'gradient max-rel over 2e-4: {bad}'
