# -*- coding:utf-8 -*-
"""Times the three products of the tiled Dense (csrc/dense_tiled.hip: forward, grad_x, grad_W + grad_b) against torch's
matmul (the vendor GEMM) on the same tensors, at the widest Dense shapes of the FiBiNet and FGCNN presets at the
benchmark batch: 8192 x 10413 x 128, 8192 x 2912 x 832 and 8192 x 2093 x 128.  For orientation only: the gate is the
presets' step time (bench.py --model FiBiNet / FGCNN).  Device events around each call, warm-up calls first, the median
of the repeats reported with min / max.  Prints one JSON line: {"shapes": {"NxKxM": {...}}}.
--mode bf16x3,bf16 times the same products of csrc/dense_tiled_x3.hip in those modes as well, on the same tensors in the
same process: per product one more entry per mode beside 'tiled' and 'torch', and its ratio to the fp32 tiled kernel.

    python tools/dense_tiled_bench.py [--shapes 8192x10413x128,8192x2912x832,8192x2093x128] [--repeats R] [--warmup W]
                                      [--mode bf16x3[,bf16]]
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


def bench_shape(N, K, M, warmup, repeats, dev, modes=()):
    from deeptables_amd import _lib
    from deeptables_amd._lib import check, lib, ptr, stream_ptr
    h = lib()
    g = torch.Generator().manual_seed(N + K + M)
    x = torch.randn((N, K), generator=g).to(dev)
    W = (torch.randn((K, M), generator=g) / K ** 0.5).to(dev)
    b = torch.randn((M,), generator=g).to(dev)
    gy = torch.randn((N, M), generator=g).to(dev)
    y, gx = torch.empty((N, M), device=dev), torch.empty((N, K), device=dev)
    gW, gb = torch.zeros((K, M), device=dev), torch.zeros((M,), device=dev)
    relu = _lib.DT_ACT_RELU
    check(h.dt_dense_tiled_fwd(ptr(x), ptr(W), ptr(b), relu, N, K, M, ptr(y), stream_ptr()), 'dt_dense_tiled_fwd')
    G = gy * (y > 0)
    flops = 2.0 * N * K * M

    def ours_bwd(want_x):
        check(h.dt_dense_tiled_bwd(ptr(x), ptr(W), ptr(y), ptr(gy), relu, N, K, M, ptr(gx) if want_x else None, ptr(gW),
                                   ptr(gb), None, stream_ptr()), 'dt_dense_tiled_bwd')

    runs = {
        'fwd': (lambda: check(h.dt_dense_tiled_fwd(ptr(x), ptr(W), ptr(b), relu, N, K, M, ptr(y), stream_ptr()), 'fwd'),
                lambda: torch.relu_(torch.addmm(b, x, W))),
        'grad_W': (lambda: ours_bwd(False), lambda: (torch.addmm(gW, x.t(), G), G.sum(0))),
        # ours: both backward products in one call; the grad_x figure is the difference to the grad_W call
        'grad_x+grad_W': (lambda: ours_bwd(True), lambda: (G @ W.t(), torch.addmm(gW, x.t(), G), G.sum(0))),
    }
    out = {}
    for name, (ours, vendor) in runs.items():
        o, v = timed(ours, warmup, repeats), timed(vendor, warmup, repeats)
        out[name] = {'tiled': o, 'torch': v, 'tiled_over_torch': o['median_ms'] / v['median_ms']}
    for mode in modes:
        code = {'bf16x3': _lib.DT_DENSE_X3, 'bf16': _lib.DT_DENSE_BF16}[mode]

        def x3_fwd():
            check(h.dt_dense_x3_fwd(ptr(x), ptr(W), ptr(b), relu, N, K, M, ptr(y), code, None, stream_ptr()), 'dt_dense_x3_fwd')

        def x3_bwd(want_x):
            check(h.dt_dense_x3_bwd(ptr(x), ptr(W), ptr(y), ptr(gy), relu, N, K, M, ptr(gx) if want_x else None, ptr(gW),
                                    ptr(gb), code, None, stream_ptr()), 'dt_dense_x3_bwd')

        for name, fn in (('fwd', x3_fwd), ('grad_W', lambda: x3_bwd(False)), ('grad_x+grad_W', lambda: x3_bwd(True))):
            t = timed(fn, warmup, repeats)
            out[name][mode] = t
            out[name][mode + '_over_tiled'] = t['median_ms'] / out[name]['tiled']['median_ms']
            out[name][mode + '_over_torch'] = t['median_ms'] / out[name]['torch']['median_ms']
    for name, products in (('fwd', 1), ('grad_W', 1), ('grad_x+grad_W', 2)):
        out[name]['tiled_tflops'] = products * flops / out[name]['tiled']['median_ms'] * 1e-9
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='8192x10413x128,8192x2912x832,8192x2093x128')
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--mode', default='', help="comma list of dense_tiled_x3 modes to time as well: bf16x3, bf16")
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    dev = torch.device('cuda', 0)
    res = {}
    for spec in args.shapes.split(','):
        N, K, M = (int(v) for v in spec.split('x'))
        res[spec] = bench_shape(N, K, M, args.warmup, args.repeats, dev, [m for m in args.mode.split(',') if m])
    print(json.dumps({'shapes': res}))


if __name__ == '__main__':
    main()
