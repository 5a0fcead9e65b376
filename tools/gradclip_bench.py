"""The clip stage alone (training._GradClip.clip_gradients, csrc/gradclip.hip) at the benchmark's shape, with device events:
212,992 lookups into 26 fields x 1 M rows (D = 16, fresh uniform ids every call) plus one 1.7 M-element flat dense gradient,
for clipvalue / clipnorm / global_clipnorm.  The stage is host-enqueued launch by launch, so the figure is the larger of the
device time and the enqueue time; --graph replays a captured stage instead (device time alone).

    python tools/gradclip_bench.py [--graph] [--rounds 20] [--out profiles/gradclip_stage.jsonl]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from deeptables_amd import training  # noqa: E402
from deeptables_amd.ops import SparseRowGrad  # noqa: E402

B, F, D, V, DENSE = 8192, 26, 16, 1_000_000, 1_700_000


class Emb:
    def __init__(self, table):
        self.tables = {'d16': table}
        self.groups = [(D, list(range(F)))]
        self.input_dims = [V] * F
        self.sparse_grads = {}
        self.row_offset_d16 = torch.arange(F, dtype=torch.int64, device=table.device) * V


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--graph', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda')
    table = torch.nn.Parameter(torch.empty(F * V, D, device=dev))          # never read: the stage looks at its shape alone
    dense = torch.nn.Parameter(torch.zeros(DENSE, device=dev))
    emb = Emb(table)
    g = torch.Generator(device=dev).manual_seed(0)
    rows = torch.empty(B * F, dtype=torch.int64, device=dev)
    vals = torch.empty(B * F, D, device=dev)
    grad = torch.empty(DENSE, device=dev)
    results = []
    for key in training.CLIP_KEYS:
        opt = training.Adagrad([dense, table], [emb], **{key: 1.0})

        def fill():
            rows.copy_((torch.randint(0, V, (B, F), generator=g, device=dev) + emb.row_offset_d16[None, :]).reshape(-1))
            vals.normal_(generator=g)
            grad.normal_(generator=g)

        def stage():
            dense.grad = grad
            emb.sparse_grads['d16'] = [SparseRowGrad(rows, vals)]
            opt.clip_gradients()
        graph = None
        times = []
        for it in range(args.warmup + args.rounds):
            fill()
            if args.graph and graph is None and it == args.warmup - 1:
                stage()                                     # (buffers exist: nothing is allocated inside the capture)
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    stage()
                fill()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            graph.replay() if graph is not None else stage()
            e1.record()
            torch.cuda.synchronize()
            if it >= args.warmup:
                times.append(e0.elapsed_time(e1) * 1e3)
        distinct = int((emb.sparse_grads['d16'][0].rows >= 0).sum())
        res = {'mode': key, 'graph': bool(args.graph), 'lookups': B * F, 'distinct_rows': distinct, 'D': D, 'fields': F,
               'dense_elems': DENSE, 'rounds': args.rounds, 'median_us': round(statistics.median(times), 1),
               'min_us': round(min(times), 1), 'max_us': round(max(times), 1)}
        print(json.dumps(res))
        results.append(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            for res in results:
                f.write(json.dumps(res) + '\n')


if __name__ == '__main__':
    main()
