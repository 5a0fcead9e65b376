"""What `KerasAdam(exact_rows=True)` costs (csrc/adam_exact.hip): the layer-path train step of the benchmark's
DeepFM (26 fields x 1 M rows, D = 16, B = 8192; bench.py's model), lazy rows against exact rows, on fresh ids every step —
uniform, and Zipf(1.05) through a per-field permutation as bench.py draws them.  Both models take the same steps; after
`--settle` steps (the gaps between two lookups of a row need a few hundred steps to reach their steady distribution) blocks of
`--steps` steps are timed alternately, host clock around work that ends in a device synchronise.  Also reported for the exact
model, from one batch at the end: the mean gap (idle steps owed per lookup) and the mean trip count of the catch-up loop per
element (tests/adam_exact_reference.py's mirror on a sample of the looked-up rows), and the device time of the catch-up
launch alone on fresh batches (device events).

    DT_AMD_FUSED=0 python tools/adam_exact_bench.py [--steps 100] [--settle 400] [--repeats 3] [--out profiles/adam_exact.jsonl]
(the tool sets DT_AMD_FUSED=0 itself: the lazy model is timed on the layer path too)"""
import argparse
import json
import os
import statistics
import sys
import time

os.environ['DT_AMD_FUSED'] = '0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from tests import adam_exact_reference as R  # noqa: E402

F, VOCAB, ND, D = bench.F, bench.VOCAB, bench.ND, bench.D


class Ids:
    """fresh [B, F] int32 ids per step on the device: bench.make_batches' two distributions"""

    def __init__(self, kind, batch, device):
        self.kind, self.batch, self.device = kind, batch, device
        self.g = torch.Generator(device=device).manual_seed(7)
        if kind == 'zipf':
            gp = torch.Generator(device='cpu').manual_seed(1234)
            self.perms = torch.stack([torch.randperm(VOCAB, generator=gp) for _ in range(F)], 1).to(device)    # [VOCAB, F]

    def __call__(self):
        if self.kind == 'uniform':
            return torch.randint(0, VOCAB, (self.batch, F), generator=self.g, device=self.device, dtype=torch.int32)
        alpha = 1.05
        u = torch.rand(self.batch, F, generator=self.g, device=self.device, dtype=torch.float64)
        rank = ((u * (float(VOCAB) ** (1.0 - alpha) - 1.0) + 1.0) ** (1.0 / (1.0 - alpha)) - 1.0)
        return torch.gather(self.perms, 0, rank.clamp(0, VOCAB - 1).to(torch.int64)).to(torch.int32)


def steps(dm, batches):
    dm.model.train()
    for idx, dense, y in batches:
        dm.train_step([idx, dense], y)


def timed(dm, batches):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    steps(dm, batches)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / len(batches) * 1e6


def gaps_and_trips(dm, idx, sample=4096):
    """of the exact model, for the lookups of `idx` as they stand before their catch-up"""
    emb = dm.model.layers_by_name['emb_categorical_vars_all']
    table = emb.tables[f'd{D}']
    opt = dm.optimizer
    st = opt._st(table, rows=True)
    rows = (idx.long() + emb.row_offset_d16[None, :]).reshape(-1)
    done = opt.t
    gap = (done - st['stamp'][rows].long())
    pick = rows[torch.randperm(rows.numel(), device=rows.device)[:sample]]
    p, m, v = (t[pick].cpu().numpy() for t in (table.detach(), st['m'], st['v']))
    s = st['stamp'][pick].cpu().numpy()[:, None]
    trips = R.idle_steps_f32(p, m, v, s, done - s, opt.lr, opt.b1, opt.b2, opt.eps)[3]
    return {'steps_done': int(done), 'mean_gap': round(float(gap.float().mean()), 1), 'max_gap': int(gap.max()),
            'mean_trips_per_element': round(float(trips.mean()), 1), 'max_trips': int(trips.max())}


def catchup_us(dm, batches):
    """median device time of the catch-up launch alone, each on a fresh batch whose rows are pending (device events)"""
    emb = dm.model.layers_by_name['emb_categorical_vars_all']
    out = []
    for idx in batches:
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        emb.pre_lookup(f'd{D}', idx)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return round(statistics.median(out), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--settle', type=int, default=400)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--batch', type=int, default=8192)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda')
    from deeptables_amd.models import deepnets
    models = {'lazy': bench.build_model(deepnets.DeepFM, dev),
              'exact': bench.build_model(deepnets.DeepFM, dev,
                                         extra={'optimizer': {'class_name': 'Adam', 'config': {'exact_rows': True}}})}
    assert models['exact'].optimizer.exact_rows and not models['lazy'].optimizer.exact_rows
    assert all(dm.fused_plan() is None for dm in models.values())
    results = []
    for kind in ('uniform', 'zipf'):
        ids = Ids(kind, args.batch, dev)
        g = torch.Generator(device=dev).manual_seed(3)

        def draw(n):
            return [(ids(), torch.randn(args.batch, ND, generator=g, device=dev),
                     (torch.rand(args.batch, 1, generator=g, device=dev) < 0.25).float()) for _ in range(n)]
        done = 0
        while done < args.settle:                       # both models take the same steps
            chunk = draw(min(50, args.settle - done))
            for dm in models.values():
                steps(dm, chunk)
            done += len(chunk)
        times = {'lazy': [], 'exact': []}
        for _ in range(args.repeats):
            chunk = draw(args.steps)
            for name, dm in models.items():
                times[name].append(timed(dm, chunk))
        probe = gaps_and_trips(models['exact'], ids())
        probe['catchup_launch_us'] = catchup_us(models['exact'], [ids() for _ in range(5)])
        for name in ('lazy', 'exact'):
            res = {'what': f'layer_path_step_{name}_rows', 'ids': kind, 'batch': args.batch, 'fields': F, 'rows_per_field': VOCAB,
                   'D': D, 'steps_per_block': args.steps, 'settle_steps': args.settle,
                   'median_us_per_step': round(statistics.median(times[name]), 1),
                   'min_us_per_step': round(min(times[name]), 1), 'max_us_per_step': round(max(times[name]), 1)}
            if name == 'exact':
                res.update(probe)
            print(json.dumps(res), flush=True)
            results.append(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            for res in results:
                f.write(json.dumps(res) + '\n')


if __name__ == '__main__':
    main()
