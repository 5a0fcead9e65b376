# -*- coding:utf-8 -*-
"""Times the convolution + activation + max pooling of an FGCNN block on its two paths, in one process: the HIP kernels of
csrc/fgcnn_train.hip (ops.fgcnn_conv_pool) and the pad / unfold / Dense / amax glue layers.FGCNN.call keeps for what the
kernels do not take (restated below, op for op).  Forward alone (no gradient kept) and forward + backward, at the two block
shapes of the benchmark preset — (F, C, filters, h, pool) = (26, 1, 14, 7, 2) and (13, 14, 16, 7, 2), D = 16 — and
B = 8192.  Device events around each call, warm-up calls first, the median of the repeats with min / max.  Next to each
time: the bytes the path cannot avoid moving, computed from the shapes (BYTES below), and the peak memory of one
forward + backward.  The two paths are compared on the same tensors before anything is timed.

    python tools/fgcnn_conv_bench.py [--batch 8192] [--repeats 5] [--warmup 3] [--out profiles/fgcnn_conv_products.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

BLOCKS = {'block1': (26, 16, 1, 14, 7, 2), 'block2': (13, 16, 14, 16, 7, 2)}        # F, D, C, filters, h, pool


def same_pad(size, k, stride):
    out = -(-size // stride)
    total = max((out - 1) * stride + k - size, 0)
    return out, total // 2, total - total // 2


def unfold_path(x, kernel, bias, pool):
    """layers.FGCNN.call's glue up to the pooled map (activation tanh)"""
    from deeptables_amd import ops
    B, F, D, C = x.shape
    h, filters = kernel.shape[0], kernel.shape[3]
    _, pb, pa = same_pad(F, h, 1)
    xp = torch.nn.functional.pad(x, (0, 0, 0, 0, pb, pa))
    taps = xp.unfold(1, h, 1).permute(0, 1, 2, 4, 3).reshape(B * F * D, h * C)
    out = torch.tanh(ops.dense(taps, kernel.reshape(h * C, filters), bias, None)).reshape(B, F, D, filters)
    Fp, qb, qa = same_pad(F, pool, pool)
    if qb or qa:
        out = torch.nn.functional.pad(out, (0, 0, 0, 0, qb, qa), value=float('-inf'))
    return out.reshape(B, Fp, pool, D, filters).amax(dim=2)


def kernel_path(x, kernel, bias, pool):
    from deeptables_amd import ops
    return ops.fgcnn_conv_pool(x, kernel, bias, 'tanh', pool)


def bytes_moved(B, F, D, C, filters, h, pool):
    """fp32 bytes each path reads + writes at the least, forward + backward, from the shapes alone.  kernels: the map is
    read by both launches and its gradient written; pooled is written, read back with its gradient, sel (1 byte) written
    and read.  unfold path: on top of the same map / pooled traffic the padded map, the taps matrix (written by the
    gather, read by the GEMM, read again by the weight-gradient GEMM), its gradient (written by the GEMM, read by
    unfold's backward), and the full-height conv output: written, read and rewritten by tanh, read by the pooling, and the
    same again backward."""
    Fp = -(-F // pool)
    xmap, pooled, taps, conv = 4 * B * F * D * C, 4 * B * Fp * D * filters, 4 * B * F * D * h * C, 4 * B * F * D * filters
    kernels = 2 * xmap + xmap + pooled + 2 * pooled + 2 * (pooled // 4)
    unfold = 3 * xmap + 3 * pooled + 2 * (4 * B * (F + h - 1) * D * C) + 3 * taps + 2 * taps + 8 * conv
    return {'kernels': kernels, 'unfold': unfold, 'taps_matrix': taps, 'map': xmap}


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {'median_ms': statistics.median(ms), 'min_ms': min(ms), 'max_ms': max(ms)}


def bench_block(name, B, warmup, repeats, dev):
    F, D, C, filters, h, pool = BLOCKS[name]
    g = torch.Generator().manual_seed(F + C)
    x = torch.randn((B, F, D, C), generator=g).to(dev).requires_grad_(True)
    kernel = (torch.randn((h, 1, C, filters), generator=g) / (h * C) ** 0.5).to(dev).requires_grad_(True)
    bias = (torch.randn((filters,), generator=g) * 0.1).to(dev).requires_grad_(True)
    gp = torch.randn((B, -(-F // pool), D, filters), generator=g).to(dev)
    paths = {'kernels': kernel_path, 'unfold': unfold_path}

    def step(fn):
        for t in (x, kernel, bias):
            t.grad = None
        fn(x, kernel, bias, pool).backward(gp)

    def forward(fn):
        with torch.no_grad():
            fn(x, kernel, bias, pool)

    # faster and different is not faster: the same tensors through both paths first
    got = {}
    for p, fn in paths.items():
        step(fn)
        got[p] = [fn(x, kernel, bias, pool).detach(), x.grad.clone(), kernel.grad.clone(), bias.grad.clone()]
    rel = [((a - b).abs().max() / b.abs().max()).item() for a, b in zip(got['kernels'], got['unfold'])]
    assert max(rel) < 2e-4, f'{name}: the two paths disagree (pooled, grad_x, grad_kernel, grad_bias): {rel}'
    out = {'shape': dict(B=B, F=F, D=D, C=C, filters=filters, h=h, pool=pool), 'bytes': bytes_moved(B, F, D, C, filters, h, pool),
           'paths_max_rel_diff': dict(zip(('pooled', 'grad_x', 'grad_kernel', 'grad_bias'), rel))}
    for p, fn in paths.items():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        step(fn)
        torch.cuda.synchronize()
        out[p] = {'fwd': timed(lambda: forward(fn), warmup, repeats), 'fwd_bwd': timed(lambda: step(fn), warmup, repeats),
                  'peak_bytes_fwd_bwd': torch.cuda.max_memory_allocated() - base}
    for k in ('fwd', 'fwd_bwd'):
        out[f'unfold_over_kernels_{k}'] = out['unfold'][k]['median_ms'] / out['kernels'][k]['median_ms']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8192)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fgcnn_conv_products.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    import __graft_entry__ as entry
    dev = torch.device('cuda', 0)
    res = {'source_hash': entry.source_hash(), 'device': torch.cuda.get_device_name(0), 'repeats': args.repeats,
           'blocks': {name: bench_block(name, args.batch, args.warmup, args.repeats, dev) for name in BLOCKS}}
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
