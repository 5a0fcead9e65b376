# -*- coding:utf-8 -*-
"""What the fused inference plans' tests share: the stand-in library of the host tests (test_infer*_host.py) and the
train / run / oracle helpers of the GPU tests (test_infer*_gpu.py).  A plain module: no fixtures, no pytest settings."""
import torch


class Recorder:
    """stand-in for fused.lib(): the launches named in `entries` are recorded as (name, args) and return 0; every other call
    (the predicates, the workspace size) goes to the real library"""

    def __init__(self, real, entries):
        self.real, self.entries, self.calls = real, frozenset(entries), []

    def __getattr__(self, name):
        if name in self.entries:
            return lambda *args: self.calls.append((name, args)) or 0
        return getattr(self.real, name)

    def names(self):
        return [n for n, _ in self.calls]


def install_recorder(monkeypatch, entries, env_keys):
    """a Recorder in place of fused.lib(), no stream, and the environment switches in `env_keys` unset"""
    from deeptables_amd import _lib, fused
    r = Recorder(_lib.lib(), entries)
    monkeypatch.setattr(fused, 'lib', lambda: r)
    monkeypatch.setattr(fused, 'stream_ptr', lambda: None)
    for k in env_keys:
        monkeypatch.delenv(k, raising=False)
    return r


def _ins(idx, dense, dev, kind='int32'):
    ids = idx.to(torch.int32 if kind == 'int32' else torch.float32).to(dev)
    return [ids] + ([dense.to(dev)] if dense is not None else [])


def _train_and_perturb(dm, cats, Nd, dev, steps=3, seed=21):
    """a few train steps (the weights and moving statistics leave their initial values), then the moving statistics are
    moved away from (0, 1) so that the inference BN is not the identity"""
    import tests.test_fused_gpu as T
    for s in range(steps):
        idx, dense, y = T.batch(cats, Nd, 64, seed=seed + s)
        dm.train_step(_ins(idx, dense, dev), y.to(dev))
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, layer in dm.model.layers_by_name.items():
            if hasattr(layer, 'moving_mean') and layer.moving_mean is not None:
                mm, mv = layer.moving_mean, layer.moving_variance
                mm.add_((torch.randn(mm.shape, generator=g) * 0.2).to(mm.device))
                mv.mul_((torch.rand(mv.shape, generator=g) + 0.5).to(mv.device))


def run_plan(dm, idx, dense, dev, plan_type, kind='int32'):
    """-> (logit [B,1], out [B,1]) of one prepare + one infer of the model's plan, which must be a `plan_type` (None: any)"""
    plan = dm.inference_plan()
    assert plan is not None
    if plan_type is not None:
        assert type(plan) is plan_type
    B = idx.shape[0]
    ins = _ins(idx, dense, dev, kind)
    logit = torch.empty((B, 1), dtype=torch.float32, device=dev)
    out = torch.empty_like(logit)
    plan.prepare()
    plan.infer(ins[0], ins[1] if len(ins) > 1 else None, logit, out)
    torch.cuda.synchronize()
    return logit, out


def _oracle(dm, ids, dense, dtype, weights=None):
    from oracle import bridge
    with torch.no_grad():
        return bridge.oracle_forward(dm, ids, dense, dtype=dtype, training=False, weights=weights)[0]


def _frame(cats, Nd, n, seed):
    import pandas as pd
    import tests.test_fused_gpu as T
    idx, dense, y = T.batch(cats, Nd, n, seed=seed)
    df = pd.DataFrame({c.name: idx[:, i].numpy() for i, c in enumerate(cats)})
    for j in range(Nd):
        df[f'I{j}'] = dense[:, j].numpy()
    return df, y.reshape(-1).numpy()
