"""The weight-decay / moving-average stages of a row-sparse table (training._StepStages, csrc/optim_stages.hip) at the
benchmark's row shape, with device events around captured graphs (device time alone): 212,992 lookups into 26 fields x 1 M rows
(D = 16, fresh uniform ids every round).  Timed one by one: the added dt_rows_coalesce, the launch ahead of the update (catch-up
of the average + decay; every looked-up row has sat out 100 steps, as nearly all do at this shape), the launch behind it
(average + stamp), and — for scale — plain Adam's row step (KerasAdam.step on the same lookups) and the whole staged step.

    python tools/decay_ema_bench.py [--rounds 30] [--out profiles/decay_ema_stage.jsonl]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from deeptables_amd import training  # noqa: E402
from deeptables_amd._lib import check, lib, ptr, stream_ptr  # noqa: E402
from deeptables_amd.ops import SparseRowGrad  # noqa: E402

B, F, D, V = 8192, 26, 16, 1_000_000
WD, MOM = 0.004, 0.99


class Emb:
    def __init__(self, table):
        self.tables = {'d16': table}
        self.groups = [(D, list(range(F)))]
        self.input_dims = [V] * F
        self.sparse_grads = {}
        self.row_offset_d16 = torch.arange(F, dtype=torch.int64, device=table.device) * V


def timed(body, fill, rounds, warmup=3):
    """median / min / max device microseconds of a captured `body`, `fill` run before every replay outside the timing"""
    for _ in range(warmup):
        fill()
        body()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    times = []
    for _ in range(rounds):
        fill()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        graph.replay()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    return {'median_us': round(statistics.median(times), 1), 'min_us': round(min(times), 1), 'max_us': round(max(times), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=30)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda')
    h = lib()
    table = torch.nn.Parameter(torch.zeros(F * V, D, device=dev))
    emb = Emb(table)
    g = torch.Generator(device=dev).manual_seed(0)
    rows = torch.empty(B * F, dtype=torch.int64, device=dev)
    vals = torch.empty(B * F, D, device=dev)
    staged = training.KerasAdam([table], [emb], weight_decay=WD, use_ema=True, ema_momentum=MOM)
    plain = training.KerasAdam([table], [emb])
    avg, stamp = staged._average_of(table), staged._row_stamps(table)
    state = staged._stage_state(dev)
    staged.stage_t = 100
    offs = emb.row_offset_d16

    def fill():
        rows.copy_((torch.randint(0, V, (B, F), generator=g, device=dev) + offs[None, :]).reshape(-1))
        vals.normal_(generator=g).mul_(1e-3)
        stamp.zero_()

    out = {}

    def coalesce():
        out['rows'], out['vals'], _, out['n'] = staged._coalesce(table, [SparseRowGrad(rows, vals)])

    def pre():
        check(h.dt_rows_stage_pre(ptr(table.data), ptr(avg), ptr(stamp), ptr(out['rows']), out['n'], D, F * V, ptr(offs), None, F,
                                  1, WD, 1e-3, MOM, ptr(state), stream_ptr()), 'dt_rows_stage_pre')

    def post():
        check(h.dt_rows_stage_post(ptr(table.data), ptr(avg), ptr(stamp), ptr(out['rows']), out['n'], D, F * V, MOM, ptr(state),
                                   stream_ptr()), 'dt_rows_stage_post')

    def adam():
        emb.sparse_grads['d16'] = [SparseRowGrad(rows, vals)]
        plain.step()

    def whole():
        emb.sparse_grads['d16'] = [SparseRowGrad(rows, vals)]
        staged.step()

    def fill_coalesced():
        fill()
        coalesce()

    results = []
    for name, body, filler in (('coalesce', coalesce, fill), ('rows_stage_pre', pre, fill_coalesced),
                               ('rows_stage_post', post, fill_coalesced), ('adam_rows_step', adam, fill),
                               ('staged_adam_step', whole, fill)):
        res = dict({'what': name, 'lookups': B * F, 'D': D, 'fields': F, 'rounds': args.rounds},
                   **timed(body, filler, args.rounds))
        if 'rows' in out:
            res['distinct_rows'] = int((out['rows'] >= 0).sum())
        print(json.dumps(res), flush=True)
        results.append(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            for res in results:
                f.write(json.dumps(res) + '\n')


if __name__ == '__main__':
    main()
