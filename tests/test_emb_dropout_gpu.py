# -*- coding:utf-8 -*-
"""GPU: the embedding gather with the layer's dropout inside the launch (csrc/emb_dropout.hip, dt_embedding_drop_fwd / _bwd;
ops.embedding_lookup(dropout=...), MultiColumnEmbedding, VarLenColumnEmbedding).

The mask is the cell hash: for a fixed seed word the kernel's keep-scale is ops.cell_dropout_keep(seed, salt, B, C, rate) — the
CPU mirror — read at column col_base[f] + d, so the forward and the sparse backward are checked bit for bit, the dense
backward against a float64 scatter within the bound of an fp32 sum in any order, and whole models against the oracle run
with the same mask."""
import math

import pytest
import torch

from tests import precision as P

pytestmark = pytest.mark.gpu

SEED = 0x1234567            # the seed word of the kernel-level tests
SALT = 0xC0FFEE11           # above 2^31: the salt is an unsigned word
RATE = 0.3
LEAD = 3                    # col_base[f] = LEAD + f D: the table is one group of a wider layer, not the layer's first column


def _seed(dev, word=SEED):
    return torch.tensor([word], dtype=torch.int32, device=dev)


class Case:
    """ids [B, F] over vocabularies 5 + f with one id out of range, a packed table, col_base and the mirror's keep-scale
    gathered to [B, F, D]"""

    def __init__(self, B, F, D, kind='i32', rate=RATE, seed=1, vocab=None):
        g = torch.Generator().manual_seed(seed + 1000 * B + 10 * F + D)
        self.B, self.F, self.D, self.rate = B, F, D, rate
        vocab = vocab or [5 + f for f in range(F)]
        self.vocab = torch.tensor(vocab, dtype=torch.int32)
        self.row_offset = torch.cumsum(torch.tensor([0] + vocab[:-1]), 0).to(torch.int64)
        self.idx = torch.stack([torch.randint(0, v, (B,), generator=g) for v in vocab], 1)
        self.idx[B // 2, F - 1] = vocab[F - 1] + 3                       # out of range: a zero row, row -1
        self.ids = self.idx.float() if kind == 'f32' else self.idx.int()
        self.table = torch.randn(sum(vocab), D, generator=g)
        self.col_base = (LEAD + torch.arange(F) * D).to(torch.int32)
        self.C = LEAD + F * D
        self.g = torch.randn(B, F, D, generator=g)

    def keep(self):
        from deeptables_amd import ops
        k = ops.cell_dropout_keep(SEED, SALT, self.B, self.C, self.rate)
        cols = self.col_base.long()[:, None] + torch.arange(self.D)[None, :]          # [F, D]
        return k[:, cols.reshape(-1)].reshape(self.B, self.F, self.D)

    def rows(self):
        ok = (self.idx >= 0) & (self.idx < self.vocab.long()[None, :])
        return torch.where(ok, self.row_offset[None, :] + self.idx, torch.full_like(self.idx, -1))

    def lookup(self, dev, table=None, **kw):
        from deeptables_amd import ops
        table = self.table.to(dev) if table is None else table
        return ops.embedding_lookup(self.ids.to(dev), table, self.row_offset.to(dev), self.vocab.to(dev),
                                    dropout=(self.rate, _seed(dev), SALT, self.col_base.to(dev)), **kw)


def _check_forward(dev, c):
    from deeptables_amd import ops
    oob, oob_plain = (torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(2))
    out, rows = c.lookup(dev, oob=oob)
    plain, rows_plain = ops.embedding_lookup(c.ids.to(dev), c.table.to(dev), c.row_offset.to(dev), c.vocab.to(dev), oob=oob_plain)
    want_rows = c.rows()
    assert torch.equal(rows.cpu(), want_rows) and torch.equal(rows_plain.cpu(), want_rows)
    assert int(oob.item()) == int(oob_plain.item()) == 1
    gathered = torch.where((want_rows >= 0)[..., None], c.table[want_rows.clamp(min=0)], torch.zeros(()))
    assert torch.equal(plain.cpu(), gathered)
    keep = c.keep()
    assert 0 < int((keep == 0).sum()) < keep.numel() or keep.numel() < 8
    assert torch.equal(out.cpu(), gathered * keep)


@pytest.mark.parametrize('kind', ['i32', 'f32'])
@pytest.mark.parametrize('D', [4, 12, 16, 10])            # one 16-byte lane | three lanes | the common case | the float path
@pytest.mark.parametrize('F', [1, 3])
@pytest.mark.parametrize('B', [1, 5, 64])
def test_forward_is_the_gather_times_the_mirror_s_mask(dev, B, F, D, kind):
    _check_forward(dev, Case(B, F, D, kind))


def test_forward_past_one_grid_pass(dev):
    """lookups x lanes above the launch's block cap: the grid-stride loop wraps"""
    from deeptables_amd._lib import lib
    B, F, D = 8192, 33, 16
    assert B * F * (D // 4) > lib().dt_embedding_drop_pass_units()
    _check_forward(dev, Case(B, F, D))


@pytest.mark.parametrize('D', [4, 12, 16, 10])
def test_sparse_backward_is_the_gradient_times_the_mask(dev, D):
    c = Case(64, 3, D)

    class Holder:
        grads = []

        def add_sparse_grad(self, grad):
            self.grads.append(grad)
    holder = Holder()
    table = c.table.to(dev).requires_grad_(True)
    out, rows = c.lookup(dev, table=table, holder=holder, dense_grad=False)
    out.backward(c.g.to(dev))
    assert table.grad is None and len(holder.grads) == 1
    got = holder.grads[0]
    assert torch.equal(got.rows.cpu(), c.rows().reshape(-1))
    assert torch.equal(got.values.cpu(), (c.g * c.keep()).reshape(-1, D))


def _scatter(rows, terms, V):
    """float64 scatter-add of the fp32 `terms` [n, D] into [V, D] -> (sum, n 2^-24 sum |terms| per element, n per row)"""
    t = terms.double()
    ref = torch.zeros(V, t.shape[1], dtype=torch.float64).index_add_(0, rows, t)
    mag = torch.zeros(V, t.shape[1], dtype=torch.float64).index_add_(0, rows, t.abs())
    n = torch.zeros(V, dtype=torch.float64).index_add_(0, rows, torch.ones(rows.numel(), dtype=torch.float64))
    return ref, n[:, None] * 2.0 ** -24 * mag, n


@pytest.mark.parametrize('D', [16, 10])
def test_dense_backward_within_the_bound_of_an_fp32_sum(dev, D):
    """grad_table against a float64 scatter of the fp32 products g * keep: per element within n 2^-24 sum |terms|, n the
    lookups of that row — the bound of an fp32 sum of n terms in any order; rows never looked up stay exactly 0"""
    B, F = 200, 3
    c = Case(B, F, D, vocab=[6, 9, 400])
    c.idx[:100, 0] = 0                                    # one row looked up >= 64 times
    c.ids = c.idx.int()
    rows = c.rows()
    assert int((rows == 0).sum()) >= 64 and int((rows < 0).sum()) == 1
    table = c.table.to(dev).requires_grad_(True)
    out, _ = c.lookup(dev, table=table, dense_grad=True)
    out.backward(c.g.to(dev))
    got = table.grad.cpu()
    terms = (c.g * c.keep()).reshape(-1, D)               # fp32 products: the kernel's bits
    flat = rows.reshape(-1)
    live = flat >= 0
    V = c.table.shape[0]
    ref, bound, n = _scatter(flat[live], terms[live], V)
    err = (got.double() - ref).abs()
    print('dense_bwd', D, 'max err / bound', float((err / bound.clamp(min=1e-300)).max()), 'max n', int(n.max()))
    assert bool((err <= bound).all())
    assert int((n == 0).sum()) > 100 and bool((got[n == 0] == 0).all())


def test_drop_fraction(dev):
    """B C = 2^16 elements: the dropped share within 4 sigma of the rate, sigma = sqrt(rate (1 - rate) / (B C)); the fixed seed
    word was checked with the mirror on the CPU"""
    from deeptables_amd import ops
    B, F, D = 256, 16, 16
    c = Case(B, F, D, vocab=[40] * F)
    c.col_base = (torch.arange(F) * D).to(torch.int32)
    c.C = F * D
    c.idx[B // 2, F - 1] = 0
    c.ids = c.idx.int()
    c.table = torch.ones_like(c.table)                    # out == 0 exactly where the element was dropped
    assert B * c.C >= 2 ** 16
    sigma = math.sqrt(RATE * (1 - RATE) / (B * c.C))
    mirror = float((ops.cell_dropout_keep(SEED, SALT, B, c.C, RATE) == 0).double().mean())
    out, _ = c.lookup(dev)
    share = float((out == 0).double().mean())
    print('drop share', share, 'mirror', mirror, 'sigma', sigma)
    assert share == mirror and abs(share - RATE) <= 4 * sigma


# ---- the layers -------------------------------------------------------------------------------------------------------------
def _fixed_seed(monkeypatch, word=SEED):
    from deeptables_amd import ops
    monkeypatch.setattr(ops, 'draw_cell_seed', lambda device: torch.tensor([word], dtype=torch.int32, device=device))


def test_mixed_width_layer_uses_the_slices_of_one_mask(dev, monkeypatch):
    """output_dims = [4, 8, 4]: two packed tables, two launches, and the concatenated outputs are the concatenated rows times
    ONE [B, 16] mask of the layer's salt"""
    from deeptables_amd import ops
    from deeptables_amd.models import layers
    _fixed_seed(monkeypatch)
    B, vocab, dims = 37, [5, 6, 7], [4, 8, 4]
    layer = layers.MultiColumnEmbedding(vocab, dims, dropout_rate=RATE, name='emb_mixed')
    layer.build((None, 3))
    layer.to(dev).train()
    g = torch.Generator().manual_seed(4)
    idx = torch.stack([torch.randint(0, v, (B,), generator=g) for v in vocab], 1)
    calls = []
    launch = ops.embedding_drop_fwd_launch
    monkeypatch.setattr(ops, 'embedding_drop_fwd_launch', lambda *a: (calls.append(a), launch(*a))[1])
    outs = layer(idx.int().to(dev))
    assert len(calls) == 2 and [tuple(o.shape) for o in outs] == [(B, 1, d) for d in dims]
    assert not any(hasattr(o, '_dt_pack') for o in outs)              # two blocks: no single packed one to hand on
    rows = torch.cat([e.detach().cpu()[idx[:, i]] for i, e in enumerate(layer.embeddings)], 1)        # [B, 16]
    keep = ops.cell_dropout_keep(SEED, ops.cell_salt('emb_mixed'), B, sum(dims), RATE)
    assert torch.equal(torch.cat([o.detach().cpu().reshape(B, -1) for o in outs], 1), rows * keep)


def test_var_len_layer(dev, monkeypatch):
    """L = 3 positions of one table: [B, 1, L D] = the rows times the [B, L D] mask, one launch each way, dense table gradient"""
    from deeptables_amd import ops
    from deeptables_amd.models import layers
    _fixed_seed(monkeypatch)
    B, V, D, L = 21, 9, 4, 3
    layer = layers.VarLenColumnEmbedding(V, D, dropout_rate=RATE, name='var_len_x')
    layer.build((None, L))
    layer.to(dev).train()
    n = {'fwd': 0, 'bwd': 0}
    fwd, bwd = ops.embedding_drop_fwd_launch, ops.embedding_drop_bwd_launch
    monkeypatch.setattr(ops, 'embedding_drop_fwd_launch', lambda *a, **k: (n.__setitem__('fwd', n['fwd'] + 1), fwd(*a, **k))[1])
    monkeypatch.setattr(ops, 'embedding_drop_bwd_launch', lambda *a, **k: (n.__setitem__('bwd', n['bwd'] + 1), bwd(*a, **k))[1])
    monkeypatch.setattr(torch.nn.functional, 'dropout', _no_torch_dropout)
    g = torch.Generator().manual_seed(6)
    idx = torch.randint(0, V, (B, L), generator=g)
    up = torch.randn(B, 1, L * D, generator=g)
    out = layer(idx.int().to(dev))
    out.backward(up.to(dev))
    assert n == {'fwd': 1, 'bwd': 1} and tuple(out.shape) == (B, 1, L * D)
    keep = ops.cell_dropout_keep(SEED, ops.cell_salt('var_len_x'), B, L * D, RATE)
    table = layer.embeddings.detach().cpu()
    assert torch.equal(out.detach().cpu().reshape(B, -1), table[idx].reshape(B, -1) * keep)
    ref, bound, _ = _scatter(idx.reshape(-1), (up.reshape(B, -1) * keep).reshape(-1, D), V)
    assert bool(((layer.embeddings.grad.cpu().double() - ref).abs() <= bound).all())
    layer.eval()
    assert torch.equal(layer(idx.int().to(dev)).detach().cpu().reshape(B, -1), table[idx].reshape(B, -1)) and n['fwd'] == 1


def _no_torch_dropout(*a, **k):
    raise AssertionError('torch.nn.functional.dropout on the fused embedding-dropout path')


F_, ND, D_, B_ = 5, 3, 8, 64


def _model(nets, **extra):
    import tests.test_fused_gpu as T
    return T.build(F_, ND, D_, vocab=30, nets=nets, embedding_dropout=RATE, dense_dropout=0, **extra)


def test_one_launch_each_way_per_table(dev, monkeypatch):
    """a built ['dnn_nets'] model: a training forward + backward makes one launch of each kernel and no torch dropout, the
    Concatenate over the embedding outputs returns the dropped block itself; eval() makes none; DT_AMD_EMB_DROPOUT=0 restores
    the per-column torch chain"""
    import tests.test_fused_gpu as T
    from deeptables_amd import functional, ops
    dm, cats = _model(['dnn_nets'], optimizer='sgd')
    assert dm.fused_plan() is None
    idx, dense, y = T.batch(cats, ND, B_)
    ins = [idx.int().to(dev), dense.to(dev)]
    n, blocks, torch_drops = {'fwd': 0, 'bwd': 0}, [], []
    torch_dropout = torch.nn.functional.dropout
    fwd, bwd = ops.embedding_drop_fwd_launch, ops.embedding_drop_bwd_launch

    def count_fwd(*a, **k):
        n['fwd'] += 1
        blocks.append(a[8])                               # `out`: the dropped block
        return fwd(*a, **k)

    def count_bwd(*a, **k):
        n['bwd'] += 1
        return bwd(*a, **k)
    monkeypatch.setattr(ops, 'embedding_drop_fwd_launch', count_fwd)
    monkeypatch.setattr(ops, 'embedding_drop_bwd_launch', count_bwd)
    monkeypatch.setattr(torch.nn.functional, 'dropout', _no_torch_dropout)
    concats = []
    hooks = [l.register_forward_hook(lambda mod, args, out: concats.append((args[0], out)))
             for l in dm.model.layers_by_name.values() if isinstance(l, functional.Concatenate)]
    dm.model.train()
    dm.model(ins).sum().backward()
    assert n == {'fwd': 1, 'bwd': 1}
    over_emb = [(a, o) for a, o in concats if isinstance(a, (list, tuple)) and len(a) == F_ and hasattr(a[0], '_dt_pack')]
    assert over_emb, 'no Concatenate saw the packed embedding views'
    for a, o in over_emb:
        assert o.data_ptr() == blocks[0].data_ptr() and o.numel() == blocks[0].numel()
    dm.model.eval()
    with torch.no_grad():
        dm.model(ins)
    assert n == {'fwd': 1, 'bwd': 1}
    for h in hooks:
        h.remove()
    # the switch, read at every call
    dm.model.train()
    monkeypatch.setattr(torch.nn.functional, 'dropout',
                        lambda x, p, training, **k: (torch_drops.append(p), torch_dropout(x, p, training, **k))[1])
    monkeypatch.setenv('DT_AMD_EMB_DROPOUT', '0')
    dm.model(ins).sum().backward()
    assert n == {'fwd': 1, 'bwd': 1} and len(torch_drops) == F_
    monkeypatch.setenv('DT_AMD_EMB_DROPOUT', '1')
    dm.model(ins)
    assert n['fwd'] == 2 and len(torch_drops) == F_


# ---- through the model, against the oracle with the same mask ----------------------------------------------------------------
def _masked_oracle(dm, idx, dense, y, keep, dtype):
    """test_fused_gpu's `Masked` table wrapper: tables[f][ids] -> the looked-up rows times this field's keep-scale"""
    from oracle import bridge, reference_layers as R
    B = idx.shape[0]

    class Masked:
        def __init__(self, t, f):
            self.t, self.f = t, f

        def __getitem__(self, ids):
            return self.t[ids] * keep[:, self.f].reshape(B, 1, -1).to(dtype)
    w = bridge.oracle_weights(dm, dtype=dtype, requires_grad=True)
    tabs = w['emb_categorical_vars_all']
    w['emb_categorical_vars_all'] = [Masked(t, f) for f, t in enumerate(tabs)]
    probe, near = [], []
    R.RELU_PROBE, R.RELU_NEAR = probe, near
    try:
        logit, _ = bridge.oracle_forward(dm, idx, dense, dtype=dtype, training=True, weights=w)
    finally:
        R.RELU_PROBE, R.RELU_NEAR = None, None
    loss = R.binary_crossentropy_from_logits(logit, y.to(dtype))
    loss.backward()
    first = [k for k in ('dnn', 'cross_dnn') if k in w][0]
    return {'logit': logit.detach(), 'loss': float(loss.detach()), 'table': torch.cat([t.grad for t in tabs], 0),
            'tower': w[first][0][0].grad, 'near': int(sum(near))}


@pytest.mark.parametrize('net', ['dnn_nets', 'xDeepFM'])
def test_layer_path_step_matches_the_oracle_with_the_same_mask(dev, monkeypatch, net):
    """forward_backward on the layer path (no fused plan) with embedding_dropout = 0.3 and a fixed seed word: logits, loss, table
    gradient and the first tower kernel's gradient within yardstick B, class fp32, of the float64 oracle under the mirror's
    mask — the float32 CPU oracle with that mask is the measure"""
    import tests.test_fused_gpu as T
    from deeptables_amd import ops
    from deeptables_amd.models import deepnets
    from oracle import headline
    monkeypatch.setenv('DT_AMD_CIN_DTYPE', 'float32')                 # every product of the graph in its exact fp32 mode
    _fixed_seed(monkeypatch)
    dm, cats = _model(['dnn_nets'], optimizer='sgd') if net == 'dnn_nets' else _model(deepnets.xDeepFM)
    assert dm.fused_plan() is None
    idx, dense, y = T.batch(cats, ND, B_)
    emb = dm.model.layers_by_name['emb_categorical_vars_all']
    keep = ops.cell_dropout_keep(SEED, ops.cell_salt(emb.name), B_, F_ * D_, RATE).reshape(B_, F_, D_)
    r64 = _masked_oracle(dm, idx, dense, y, keep, torch.float64)
    if r64['near']:                 # a tower relu input within float32 rounding of zero: move the kinks once
        headline.shift_tower_biases(dm)
        r64 = _masked_oracle(dm, idx, dense, y, keep, torch.float64)
    r32 = _masked_oracle(dm, idx, dense, y, keep, torch.float32)
    dm.model.train()
    n = []
    fwd = ops.embedding_drop_fwd_launch
    monkeypatch.setattr(ops, 'embedding_drop_fwd_launch', lambda *a, **k: (n.append(1), fwd(*a, **k))[1])
    loss, logit = dm.forward_backward([idx.int().to(dev), dense.to(dev)], y.to(dev))
    torch.cuda.synchronize()
    assert len(n) == 1
    L = dm.model.layers_by_name
    table = emb.tables[f'd{D_}']
    tg = table.grad.to_dense() if table.grad.is_sparse else table.grad
    got = {'logit': logit, 'table': tg, 'tower': L['dnn_dense_1'].kernel.grad}
    figs = {k: (P.row_rel(got[k], r64[k]), P.row_rel(r32[k], r64[k])) for k in got}
    figs['loss'] = (abs(float(loss) - r64['loss']), abs(r32['loss'] - r64['loss']))
    ratios = {k: g / max(f, P.FLOOR) for k, (g, f) in figs.items()}
    P.record(f'emb_dropout_step[{net}]', **ratios)
    print('emb_dropout_step', net, {k: (round(ratios[k], 2), figs[k]) for k in figs})
    bad = {k: (ratios[k], figs[k]) for k in figs if not (math.isfinite(ratios[k]) and ratios[k] <= P.STEP_BAR['fp32'])}
    assert not bad, bad


def test_replayed_steps_draw_fresh_masks(dev, monkeypatch):
    """fit(steps_per_execution=2) on a resident feed: the gather launches of the two captured steps read two different seed
    words, and the next replay of the SAME graph different ones again — the word is drawn inside the graph and read from
    device memory by the kernel, not frozen into it"""
    import tests.test_fused_gpu as T
    from deeptables_amd import ops
    from deeptables_amd.training import TableBatches
    dm, cats = _model(['dnn_nets'], optimizer='sgd')
    drawn, used = [], []
    draw, fwd = ops.draw_cell_seed, ops.embedding_drop_fwd_launch
    monkeypatch.setattr(ops, 'draw_cell_seed', lambda device: (drawn.append(draw(device)), drawn[-1])[1])
    monkeypatch.setattr(ops, 'embedding_drop_fwd_launch', lambda *a, **k: (used.append(a[5]), fwd(*a, **k))[1])
    idx, dense, y = T.batch(cats, ND, B_ * 4)
    feed = TableBatches.from_device([idx.int().to(dev), dense.to(dev)], ['cat', 'cont'], y.to(dev), y_ndim=2)
    torch.manual_seed(77)
    dm.fit(feed, batch_size=B_, epochs=1, verbose=0, steps_per_execution=2)
    assert dm.compiled_loop is not None and dm.compiled_loop.graph is not None
    torch.cuda.synchronize()
    count = len(used)
    assert count >= 2 and len(drawn) == count                     # the embedding layer is the model's only mask
    assert all(u.data_ptr() == d.data_ptr() for u, d in zip(used, drawn))        # the kernel reads the drawn word's memory
    first = [int(w.item()) for w in used[-2:]]                    # the captured graph's two words, as its last replay left them
    dm.fit(feed, batch_size=B_, epochs=1, verbose=0, steps_per_execution=2)
    torch.cuda.synchronize()
    assert len(used) == count                                     # replays only: no Python ran
    second = [int(w.item()) for w in used[-2:]]
    assert len(set(first + second)) == 4, (first, second)
