# -*- coding:utf-8 -*-
"""GPU: every kernel family held to the precision class it claims (tests/precision.py: CLAIMS), not to a blanket 1e-4.

Single products (dense, cross, CIN in its three modes) are measured in units of |A| |B| of their own contraction (yardstick
A); composed kernels (the fused DeepFM / DCN step in its three tower modes, the pipelined step's weight-gradient GEMMs, the
AutoInt layer in its three modes) against the error the same float64 oracle makes when it is evaluated in float32 on the CPU
(yardstick B).  A kernel that loses bits — a dropped product group, a truncated operand — fails here even where it stays
inside the 1e-4 bars of the other files."""
import numpy as np
import pytest
import torch

from tests import precision as P

pytestmark = pytest.mark.gpu


def _rnd(g, shape, scale=1.0):
    """float64 values that float32 holds exactly: the kernel and the reference see the same inputs"""
    return (torch.randn(shape, generator=g, dtype=torch.float64) * scale).float().double()


# ---- yardstick A: one GEMM-shaped product ---------------------------------------------------------------------------------
@pytest.mark.parametrize('N,K,M,act,bias', [(33, 429, 128, 'relu', True), (37, 128, 64, 'relu', True), (513, 64, 1, None, False),
                                            (64, 39, 1, None, True), (129, 493, 40, 'relu', False), (5, 3, 2, None, True)])
def test_dense_is_fp32_class(dev, N, K, M, act, bias):
    from deeptables_amd import ops
    g = torch.Generator().manual_seed(7 * N + K + M)
    x, W = _rnd(g, (N, K)), _rnd(g, (K, M), 1.0 / np.sqrt(K))
    b = _rnd(g, (M,), 0.3) if bias else None
    lin = lambda x_, W_, b_: x_ @ W_ + (b_ if b_ is not None else 0)
    pre = lin(x, W, b)
    up = P.kink_mask(pre, P.abs_forward(lin, (x, W, b)), _rnd(g, (N, M)), act, 'fp32')
    xr, Wr = x.clone().requires_grad_(True), W.clone().requires_grad_(True)
    br = b.clone().requires_grad_(True) if bias else None
    ref = xr @ Wr + (br if bias else 0)
    ref = torch.relu(ref) if act == 'relu' else ref
    (ref * up).sum().backward()
    upl = up * (pre > 0) if act == 'relu' else up
    s_out, (s_x, s_W, s_b) = P.abs_scale(lin, (x, W, b), upl)
    xd, Wd = x.float().to(dev).requires_grad_(True), W.float().to(dev).requires_grad_(True)
    bd = b.float().to(dev).requires_grad_(True) if bias else None
    out = ops.dense(xd, Wd, bd, act)
    (out * up.float().to(dev)).sum().backward()
    figs = {'y': ('fwd', P.cond_rms(out, ref, s_out)), 'dx': ('bwd', P.cond_rms(xd.grad, xr.grad, s_x)),
            'dW': ('bwd', P.cond_rms(Wd.grad, Wr.grad, s_W))}
    if bias:
        figs['db'] = ('bwd', P.cond_rms(bd.grad, br.grad, s_b))
    P.check_cond(f'dense[{N},{K},{M},{act},{bias}]', 'dense', 'float32', figs)


@pytest.mark.parametrize('B,C,L', [(33, 429, 1), (37, 64, 1), (513, 130, 3), (5, 7, 2)])
def test_cross_is_fp32_class(dev, B, C, L):
    from deeptables_amd import ops
    from oracle import reference_layers as R
    g = torch.Generator().manual_seed(B + 3 * C + L)
    x, w, b = _rnd(g, (B, C), 0.5), _rnd(g, (L, C), 1.0 / np.sqrt(C)), _rnd(g, (L, C), 0.1)
    up = _rnd(g, (B, C))
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
    layers = lambda x_, w_, b_: R.cross(x_, [w_[i].unsqueeze(1) for i in range(L)], [b_[i].unsqueeze(1) for i in range(L)])
    ref = layers(xr, wr, br)
    (ref * up).sum().backward()
    s_out, (s_x, s_w, s_b) = P.abs_scale(layers, (x, w, b), up)
    xd, wd, bd = (t.float().to(dev).requires_grad_(True) for t in (x, w, b))
    out = ops.cross(xd, wd, bd)
    (out * up.float().to(dev)).sum().backward()
    P.check_cond(f'cross[{B},{C},{L}]', 'cross', 'float32',
                 {'y': ('fwd', P.cond_rms(out, ref, s_out)), 'dx': ('bwd', P.cond_rms(xd.grad, xr.grad, s_x)),
                  'dw': ('bwd', P.cond_rms(wd.grad, wr.grad, s_w)), 'db': ('bwd', P.cond_rms(bd.grad, br.grad, s_b))})


CIN_SHAPES = [(5, 4, 4, 6, 3, False, 'relu'), (33, 26, 26, 128, 16, False, 'relu'), (37, 26, 64, 128, 16, True, 'relu'),
              (9, 5, 7, 33, 8, True, 'linear'), (20, 6, 100, 200, 4, False, 'relu'),
              # B D >= 32768: the eight-wave forward / dgrad blocks and the wide wgrad blocks (Hk <= 32 and Hk <= 64 forms)
              (2100, 26, 64, 128, 16, False, 'relu'), (2060, 26, 26, 128, 16, True, 'relu')]


@pytest.mark.parametrize('mode', ['float32', 'bf16x3', 'bf16'])
@pytest.mark.parametrize('B,F0,Hk,L,D,bias,act', CIN_SHAPES)
def test_cin_layer_holds_its_class(dev, mode, B, F0, Hk, L, D, bias, act):
    """CIN.call (layers.py:689-710): y = act(sum_ij x0_i xk_j W_ij + b), contraction length F0 Hk (16 .. 1664)"""
    from deeptables_amd import ops
    g = torch.Generator().manual_seed(B + F0 + Hk + L)
    x0, xk = _rnd(g, (B, F0, D), 0.5), _rnd(g, (B, Hk, D), 0.5)
    W = _rnd(g, (F0 * Hk, L), 1.0 / np.sqrt(F0 * Hk))
    bv = _rnd(g, (L,), 0.1) if bias else None
    lin = lambda a, c, w_, b_: (torch.einsum('bid,bjd,ijl->bld', a, c, w_.reshape(F0, Hk, L)) +
                                (b_[None, :, None] if b_ is not None else 0))
    pre = lin(x0, xk, W, bv)
    up = P.kink_mask(pre, P.abs_forward(lin, (x0, xk, W, bv)), _rnd(g, (B, L, D)), act, P.CLAIMS[('cin', mode)][0])
    x0r, xkr, Wr = (t.clone().requires_grad_(True) for t in (x0, xk, W))
    bvr = bv.clone().requires_grad_(True) if bias else None
    ref = lin(x0r, xkr, Wr, bvr)
    ref = torch.relu(ref) if act == 'relu' else ref
    (ref * up).sum().backward()
    s_out, (s_x0, s_xk, s_W, s_b) = P.abs_scale(lin, (x0, xk, W, bv), up * (pre > 0) if act == 'relu' else up)
    x0d, xkd, Wd = (t.float().to(dev).requires_grad_(True) for t in (x0, xk, W))
    bd = bv.float().to(dev).requires_grad_(True) if bias else None
    out = ops.cin_layer(x0d, xkd, Wd, bd, act, mode)
    (out * up.float().to(dev)).sum().backward()
    figs = {'y': ('fwd', P.cond_rms(out, ref, s_out)), 'dx0': ('bwd', P.cond_rms(x0d.grad, x0r.grad, s_x0)),
            'dxk': ('bwd', P.cond_rms(xkd.grad, xkr.grad, s_xk)), 'dW': ('bwd', P.cond_rms(Wd.grad, Wr.grad, s_W))}
    if bias:
        figs['db'] = ('bwd', P.cond_rms(bd.grad, bvr.grad, s_b))
    P.check_cond(f'cin[{mode},{B},{F0},{Hk},{L},{D}]', 'cin', mode, figs)


# ---- yardstick B: composed kernels against the float32 evaluation of the same oracle ---------------------------------------
def _oracle(dm, idx, dense, y, dtype, loss='bce'):
    from oracle import bridge, reference_layers as R
    w = bridge.oracle_weights(dm, dtype=dtype, requires_grad=True)
    probe, near = [], []
    R.RELU_PROBE, R.RELU_NEAR = probe, near
    try:
        logit, _ = bridge.oracle_forward(dm, idx, dense, dtype=dtype, training=True, weights=w)
    finally:
        R.RELU_PROBE, R.RELU_NEAR = None, None
    if loss == 'bce':
        lv = R.binary_crossentropy_from_logits(logit, y.to(dtype))
    else:
        lv = ((logit - y.to(dtype)) ** 2).mean()
    lv.backward()
    return logit.detach(), float(lv), w, int(sum(near))


def _step_figures(dm, idx, dense, y, ins, yd, cls, loss='bce'):
    """one fused step on the GPU against the float64 and float32 oracles -> {name: (direction, err_gpu, err_f32)}"""
    from oracle import headline
    r64 = _oracle(dm, idx, dense, y, torch.float64, loss)
    if r64[3]:                     # a tower relu input within float32 rounding of zero: move the kinks once, as headline does
        headline.shift_tower_biases(dm)
        r64 = _oracle(dm, idx, dense, y, torch.float64, loss)
    r32 = _oracle(dm, idx, dense, y, torch.float32, loss)
    dm.model.train()
    got_loss, logit = dm.forward_backward(ins, yd)
    torch.cuda.synchronize()
    metric = P.l2_rel if cls == 'bf16' else None
    pick = lambda t: metric or (P.row_rel if t.dim() >= 2 else P.max_rel)
    figs = {'logit': ('fwd', pick(logit)(logit, r64[0]), pick(logit)(r32[0], r64[0])),
            'loss': ('fwd', abs(float(got_loss) - r64[1]), abs(r32[1] - r64[1]))}
    if cls == 'bf16':
        # relu decisions taken on 8-bit inputs flip units that no bias shift clears, and each flip moves a weight gradient
        # by a whole sample's term: only the forward is held to the class (the gradients keep the kink-aware L2 rule of
        # tests/test_x3_gpu.py::test_bf16_tower_headline_config_holds_the_bf16_bar)
        return figs
    g64 = headline.oracle_dense_grads(dm, r64[2])
    g32 = dict((id(p), g) for p, g in headline.oracle_dense_grads(dm, r32[2]))
    names = {id(p): n for n, p in dm.model.named_parameters()}
    assert len(g64) >= 10
    for p, g in g64:
        got = p.grad.reshape(g.shape)
        figs[names[id(p)]] = ('bwd', pick(g)(got, g), pick(g)(g32[id(p)].reshape(g.shape), g))
    emb = dm.model.layers_by_name['emb_categorical_vars_all']
    (key, table), = emb.tables.items()
    t64 = torch.cat([t.grad for t in r64[2]['emb_categorical_vars_all']], 0)
    t32 = torch.cat([t.grad for t in r32[2]['emb_categorical_vars_all']], 0)
    tg = table.grad.to_dense() if table.grad.is_sparse else table.grad
    tmetric = metric or P.row_rel
    figs['table'] = ('bwd', tmetric(tg, t64), tmetric(t32, t64))
    return figs


TOWER_MODES = ['bf16x3', 'f32', 'bf16']


@pytest.mark.parametrize('mode', TOWER_MODES)
@pytest.mark.parametrize('net,B,F,Nd,D,extra', [
    ('DeepFM', 33, 26, 13, 16, None), ('DeepFM', 513, 15, 2, 32, None), ('DeepFM', 256, 26, 13, 16, None),
    ('DeepFM', 37, 26, 13, 16, ((100, 0, False), (40, 0, False))),          # a narrow tower: zero-padded slabs
    ('DCN', 37, 5, 3, 8, 2), ('DCN', 513, 16, 2, 16, 3)])
def test_fused_step_holds_its_class(dev, monkeypatch, mode, net, B, F, Nd, D, extra):
    """logits, loss, every dense gradient and the table gradient (row by row) of the fused step in each tower mode"""
    import tests.test_fused_gpu as T
    from deeptables_amd import fused
    from deeptables_amd.models import deepnets
    monkeypatch.setenv('DT_AMD_TOWER_DTYPE', mode)
    kw = {}
    if net == 'DCN':
        kw = dict(nets=deepnets.DCN, cross_params={'num_cross_layer': extra},
                  dnn_params={'hidden_units': ((128, 0, False), (64, 0, False)), 'activation': 'relu'})
    elif extra:
        kw = dict(dnn_params={'hidden_units': extra, 'activation': 'relu'})
    dm, cats = T.build(F, Nd, D, vocab=30, **kw)
    if net == 'DCN':
        g = torch.Generator().manual_seed(11)
        with torch.no_grad():
            cr = dm.model.layers_by_name['dcn_cross_layer']
            cr.bias_stack.add_(torch.randn(cr.bias_stack.shape, generator=g).to(cr.bias_stack.device) * 0.05)
    plan = dm.fused_plan()
    assert plan is not None and plan.tower_flag == fused._tower_mfma_flag({'mfma_dtype': mode})
    idx, dense, y = T.batch(cats, Nd, B)
    ins = [idx.int().to(dev)] + ([dense.to(dev)] if Nd else [])
    cls = P.CLAIMS[('tower', mode)][0]
    figs = _step_figures(dm, idx, dense, y, ins, y.to(dev), cls)
    P.check_step(f'step[{mode},{net},{B},{F},{Nd},{D},{extra}]', 'tower', mode, figs)


@pytest.mark.parametrize('mode', ['bf16x3', 'f32'])
def test_timed_step_adam_slots_hold_their_class(dev, monkeypatch, mode):
    """the step as bench.py times it — B = 8192 on the benchmarked DeepFM, `_forward_backward(apply_rows=True)` and the
    Keras-Adam update inside the step's launches (dt_deepfm_train_step_adam) — read back through the optimizer's slots:
    after one step on a fresh model m = (1 - beta_1) g, so m / (1 - beta_1) of every dense parameter is the gradient of
    k_wgrad_rows' weight-gradient GEMMs (wgrad_heavy_bf16 with the split tower, wgrad_heavy with the exact one) and that of
    every table row the row gradient merged by the in-step dedupe"""
    import bench
    from oracle import headline
    from deeptables_amd.models import deepnets
    monkeypatch.setenv('DT_AMD_TOWER_DTYPE', mode)
    dm = bench.build_model(deepnets.DeepFM, dev, None, bench.D, {})
    bench.N_BATCHES, keep = 1, bench.N_BATCHES
    try:
        idx, dense, y = bench.make_batches(8192, dev, seed=1234, dist_kind='uniform')[0]
    finally:
        bench.N_BATCHES = keep
    r64 = headline.oracle_train_step(dm, idx, dense, y)
    if r64['relu_units_near_kink']:
        headline.shift_tower_biases(dm)
        r64 = headline.oracle_train_step(dm, idx, dense, y, tables_cpu=r64['tables_cpu'])
    r32 = headline.oracle_train_step(dm, idx, dense, y, dtype=torch.float32, tables_cpu=r64['tables_cpu'])
    opt = dm.optimizer
    dm.model.train()
    loss, logit = dm._forward_backward([idx, dense], y, apply_rows=True)
    assert getattr(opt, '_applied_in_step', False), 'the step did not take the in-step Adam path'
    opt.step()
    torch.cuda.synchronize()
    figs = {'logit': ('fwd', P.max_rel(logit, r64['logit']), P.max_rel(r32['logit'], r64['logit']))}
    g32 = dict((id(p), g) for p, g in headline.oracle_dense_grads(dm, r32['weights']))
    names = {id(p): n for n, p in dm.model.named_parameters()}
    for p, g in headline.oracle_dense_grads(dm, r64['weights']):
        m = P.row_rel if g.dim() >= 2 else P.max_rel
        got = opt._st(p)['m'].reshape(g.shape) / (1.0 - opt.b1)
        figs['m:' + names[id(p)]] = ('bwd', m(got, g), m(g32[id(p)].reshape(g.shape), g))
    u, rg64 = headline.merge_rows(r64['rows'], r64['row_grads'].double())
    u32, rg32 = headline.merge_rows(r32['rows'], r32['row_grads'].double())
    assert torch.equal(u, u32)
    table = dm.model.layers_by_name['emb_categorical_vars_all'].tables[f'd{bench.D}']
    got_rows = opt._st(table, rows=True)['m'][u.to(dev)] / (1.0 - opt.b1)
    figs['m:rows'] = ('bwd', P.row_rel(got_rows, rg64), P.row_rel(rg32, rg64))
    P.check_step(f'timed[{mode}]', 'tower', mode, figs)


# ---- exact-fp32 interaction kernels: the same restatement in float32 on the CPU is the class ---------------------------------
def _layer_vs_float32(test, kernel, gpu_fn, ref_fn, inputs, up, dev):
    refs = {}
    for dt in (torch.float64, torch.float32):
        xs = [t.detach().to(dt).clone().requires_grad_(True) for t in inputs]
        out = ref_fn(*xs)
        (out * up.to(dt)).sum().backward()
        refs[dt] = [out.detach()] + [t.grad for t in xs]
    xs = [t.detach().float().to(dev).requires_grad_(True) for t in inputs]
    out = gpu_fn(*xs)
    (out * up.float().to(dev)).sum().backward()
    got = [out] + [t.grad for t in xs]
    figs = {}
    for i, (a, r64, r32) in enumerate(zip(got, refs[torch.float64], refs[torch.float32])):
        m = P.row_rel if r64.dim() >= 2 else P.max_rel
        figs['out' if i == 0 else f'd_in{i - 1}'] = ('fwd' if i == 0 else 'bwd', m(a, r64), m(r32, r64))
    P.check_step(test, kernel, 'float32', figs)


@pytest.mark.parametrize('B,F,D', [(33, 26, 16), (37, 39, 8), (513, 5, 32), (3, 2, 4)])
def test_fm_inner_product_bilinear_afm_are_fp32_class(dev, B, F, D):
    from deeptables_amd import ops
    from oracle import reference_layers as R
    g = torch.Generator().manual_seed(B * 3 + F + D)
    x = _rnd(g, (B, F, D))
    Pn = F * (F - 1) // 2
    _layer_vs_float32(f'fm[{B},{F},{D}]', 'fm', ops.fm, R.fm, [x], _rnd(g, (B, 1)), dev)
    _layer_vs_float32(f'inner[{B},{F},{D}]', 'inner', ops.inner_product,
                      lambda t: R.inner_product([t[:, i:i + 1] for i in range(F)]), [x], _rnd(g, (B, Pn)), dev)
    for bt, nW in (('field_interaction', Pn), ('field_each', F - 1), ('field_all', 1)):
        W = _rnd(g, (nW, D, D), 1.0 / np.sqrt(D))
        _layer_vs_float32(f'bilinear[{bt},{B},{F},{D}]', 'bilinear', lambda t, w: ops.bilinear_interaction(t, w, bt),
                          lambda t, w: R.bilinear_interaction(t, list(w), bt), [x, W], _rnd(g, (B, Pn, D)), dev)
    H = 8
    Wa, ba, pv = _rnd(g, (D, H), 1.0 / np.sqrt(D)), _rnd(g, (H,), 0.1), _rnd(g, (H, 1), 0.5)
    eye = torch.eye(D, dtype=torch.float64)
    _layer_vs_float32(f'afm[{B},{F},{D}]', 'afm', lambda t, a, b_, p_: ops.afm_pool(t, a, b_, p_, 'relu'),
                      lambda t, a, b_, p_: R.afm([t[:, i:i + 1] for i in range(F)], a, b_, p_, eye.to(t.dtype), 'relu'),
                      [x, Wa, ba, pv], _rnd(g, (B, D)), dev)


@pytest.mark.parametrize('kt', ['mat', 'vec', 'num'])
@pytest.mark.parametrize('B,F,D', [(33, 26, 16), (513, 7, 16), (5, 4, 3)])
def test_outer_product_is_fp32_class(dev, B, F, D, kt):
    from deeptables_amd import ops
    from oracle import reference_layers as R
    g = torch.Generator().manual_seed(B + F + D)
    Pn = F * (F - 1) // 2
    x = _rnd(g, (B, F, D))
    k = _rnd(g, {'mat': (D, Pn, D), 'vec': (Pn, D), 'num': (Pn, 1)}[kt], 0.3)
    _layer_vs_float32(f'outer[{kt},{B},{F},{D}]', 'outer', lambda t, w: ops.outer_product(t, w, kt),
                      lambda t, w: R.outer_product([t[:, i:i + 1] for i in range(F)], w, kt), [x, k], _rnd(g, (B, Pn)), dev)


@pytest.mark.parametrize('N,C', [(33, 429), (8192, 429), (513, 32), (3, 5)])
def test_batchnorm_train_is_fp32_class(dev, N, C):
    from deeptables_amd import ops
    from oracle import reference_layers as R
    g = torch.Generator().manual_seed(N + C)
    x = (_rnd(g, (N, C)) * 2.0 + 3.0).float().double()           # a non-zero mean: the shifted-variance path
    gamma, beta = _rnd(g, (C,)), _rnd(g, (C,))

    def gpu(t, ga, be):
        return ops.batchnorm_train(t, ga, be, torch.zeros(C, device=t.device), torch.ones(C, device=t.device), 1e-3, 0.99)

    def ref(t, ga, be):
        return R.keras_batchnorm(t, ga, be, torch.zeros(C, dtype=t.dtype), torch.ones(C, dtype=t.dtype), training=True)[0]
    _layer_vs_float32(f'bn[{N},{C}]', 'bn', gpu, ref, [x, gamma, beta], _rnd(g, (N, C)), dev)


@pytest.mark.parametrize('B,F,D,Nd', [(33, 26, 16, 13), (513, 5, 8, 0)])
def test_fused_embed_fm_linear_is_fp32_class(dev, B, F, D, Nd):
    """the FM output, the field sums and the packed table gradient of the fused embedding + FM + linear kernel"""
    from deeptables_amd import ops
    from oracle import reference_layers as R
    import tests.test_kernels_gpu as K
    g = torch.Generator().manual_seed(B * 7 + F)
    vocabs = [int(v) for v in torch.randint(3, 40, (F,), generator=g)]
    tables, packed, offs, voc = K.packed_tables(vocabs, D, g)
    idx = torch.stack([torch.randint(0, v, (B,), generator=g) for v in vocabs], 1)
    dense = _rnd(g, (B, Nd)).float() if Nd else None
    u3, u4 = _rnd(g, (B, F)), _rnd(g, (B, 1))
    refs = {}
    for dt in (torch.float64, torch.float32):
        tref = [t.clone().to(dt).requires_grad_(True) for t in tables]
        E = torch.cat(R.multi_column_embedding(idx.float(), tref), dim=1)
        fsum, fmo = E.sum(-1), R.fm(E)
        ((fsum * u3.to(dt)).sum() + (fmo * u4.to(dt)).sum()).backward()
        refs[dt] = (fsum.detach(), fmo.detach(), torch.cat([t.grad for t in tref], 0))
    p = packed.to(dev).requires_grad_(True)
    _, _, fsum, fmo, _ = ops.embed_fm_linear(idx.int().to(dev), p, offs.to(dev), voc.to(dev),
                                             None if dense is None else dense.to(dev), dense_grad=True)
    ((fsum * u3.float().to(dev)).sum() + (fmo * u4.float().to(dev)).sum()).backward()
    r64, r32 = refs[torch.float64], refs[torch.float32]
    P.check_step(f'embed_fm_linear[{B},{F},{D},{Nd}]', 'embed_fm_linear', 'float32',
                 {'fsum': ('fwd', P.row_rel(fsum, r64[0]), P.row_rel(r32[0], r64[0])),
                  'fm': ('fwd', P.max_rel(fmo, r64[1]), P.max_rel(r32[1], r64[1])),
                  'table': ('bwd', P.row_rel(p.grad, r64[2]), P.row_rel(r32[2], r64[2]))})


@pytest.mark.parametrize('mode,B,F,D,H,res', [
    ('float32', 33, 26, 32, 4, True), ('float32', 37, 1, 16, 1, True), ('float32', 64, 32, 16, 2, False),
    ('float32', 513, 13, 16, 2, True),
    ('bf16x2', 33, 26, 32, 4, True), ('bf16x2', 37, 1, 32, 2, True), ('bf16x2', 64, 32, 32, 2, False),
    ('bf16x2', 513, 26, 32, 4, True),
    ('bf16', 33, 26, 32, 4, True), ('bf16', 64, 32, 32, 2, False), ('bf16', 513, 26, 32, 4, True)])
def test_autoint_layer_holds_its_class(dev, mode, B, F, D, H, res):
    """the fused interacting layer (projections, attention, residual, relu) against layers.py:119-150 in float64; the
    float32 evaluation of the same restatement is the fp32 class"""
    from deeptables_amd import ops
    from tests.test_autoint_gpu import reference
    g = torch.Generator().manual_seed(B * 131 + F + D)
    NP = 4 if res else 3
    x = torch.randn(B, F, D, generator=g) * 0.7
    W = torch.randn(D, NP * D, generator=g) * (1.5 / D ** 0.5)
    b = torch.randn(NP * D, generator=g) * 0.2
    go = torch.randn(B, F, D, generator=g)
    xd = x.to(dev).requires_grad_(True)
    Ws = [W[:, i * D:(i + 1) * D].contiguous().to(dev).requires_grad_(True) for i in range(NP)]
    bs = [b[i * D:(i + 1) * D].contiguous().to(dev).requires_grad_(True) for i in range(NP)]
    out = ops.autoint_layer(xd, Ws, bs, H, 0.0, 0, mfma_dtype=mode)
    out.backward(go.to(dev))
    refs = {}
    for dt in (torch.float64, torch.float32):
        xr, Wr, br = (t.to(dt).requires_grad_(True) for t in (x, W, b))
        ar = reference(xr, Wr, br, H, res)
        ar.backward(go.to(dt))
        refs[dt] = (ar.detach(), xr.grad, Wr.grad, br.grad)
    got = (out, xd.grad, torch.cat([w.grad for w in Ws], 1), torch.cat([v.grad for v in bs], 0))
    cls = P.CLAIMS[('autoint', mode)][1]
    names = ('out', 'dx', 'dW', 'db')
    figs = {}
    for i, n in enumerate(names):
        m = P.l2_rel if cls == 'bf16' else (P.row_rel if refs[torch.float64][i].dim() >= 2 else P.max_rel)
        figs[n] = ('fwd' if i == 0 else 'bwd', m(got[i], refs[torch.float64][i]), m(refs[torch.float32][i], refs[torch.float64][i]))
    P.check_step(f'autoint[{mode},{B},{F},{D},{H},{res}]', 'autoint', mode, figs)
