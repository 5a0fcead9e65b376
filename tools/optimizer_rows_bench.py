"""Row and dense steps of the slot optimizers (csrc/optim_slots.hip), one build of the library against another:
python tools/optimizer_rows_bench.py [--lib PATH] [--tag NAME] [--out FILE.jsonl]

The method of profiles/optimizers2_rows.jsonl: 26 fields x 1 M rows, batch 8192, fresh uniform ids every round; HIP events
around ONE call (global-hash merge + owner launch); the optimizers alternated inside every round; median of 20 rounds after
5 warm-ups; D = 16 and D = 32; the seven kinds and Adam, which no change to the slot optimizers touches, as the control.
Then the dense step, timed the same way on one 16-byte aligned flat buffer of 2 M floats.  One JSON line per D and one for
the dense step.  --lib: another build of libdt_hip.so with the same C ABI; compare legs of ONE job only (parent, this, this,
parent), and only if Adam's figures agree between them."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

F, V, B = 26, 1_000_000, 8192
ROUNDS, WARMUP = 20, 5
DENSE_N = 2 * 1024 * 1024
LR = 1e-3
FTRL = (0.0, 0.0, 0.0)            # l1, l2, l2_shrinkage
# kind -> (entry-point stem, hyperparameters, slots)
KINDS = {
    'adagrad': ('adagrad', (LR, 1e-7), 1),
    'rmsprop': ('rmsprop', (LR, 0.9, 1e-7), 1),
    'sgdm': ('sgdm', (LR, 0.9, 0), 1),
    'sgdm_nesterov': ('sgdm', (LR, 0.9, 1), 1),
    'adamax': ('adamax', (LR, 0.9, 0.999, 1e-7), 2),
    'ftrl_sqrt': ('ftrl', (LR, -0.5) + FTRL, 2),
    'ftrl_pow': ('ftrl', (LR, -0.3) + FTRL, 2),
}


def timed(calls, each_round=None, each_call=None):
    """{name: median / min / max us}: every round runs each call once, in turn, between two events of its own"""
    us = {k: [] for k in calls}
    for r in range(WARMUP + ROUNDS):
        if each_round is not None:
            each_round()
        for k, call in calls.items():
            if each_call is not None:
                each_call()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            if r >= WARMUP:
                us[k].append(e0.elapsed_time(e1) * 1e3)
    return {k: {'median_us': round(statistics.median(v), 2), 'min_us': round(min(v), 2), 'max_us': round(max(v), 2)}
            for k, v in us.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--lib', default=None)
    ap.add_argument('--tag', default='this')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from deeptables_amd import _lib
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    from deeptables_amd._lib import lib, ptr, stream_ptr, check
    h = lib()
    dev = torch.device('cuda', 0)
    head = {'tag': a.tag, 'device': torch.cuda.get_device_name(0), 'source_hash': h.dt_source_hash().decode(),
            'method': f'HIP events around one call, optimizers alternated inside every round, median of {ROUNDS} rounds after '
                      f'{WARMUP} warm-ups'}
    state = torch.zeros(272 // 4, dtype=torch.int32, device=dev)
    check(h.dt_adam_state_init(ptr(state), LR, 0.9, 0.999, 0, stream_ptr()), 'dt_adam_state_init')
    gen = torch.Generator(device=dev).manual_seed(0)
    lines = []
    n = B * F
    n_slots = h.dt_adam_rows_slots(n)
    hslots = torch.zeros(n_slots, dtype=torch.int64, device=dev)
    mark = torch.empty(n, dtype=torch.int32, device=dev)
    off = (torch.arange(F, device=dev) * V)[None, :]
    for D in (16, 32):
        table = torch.zeros(F * V, D, device=dev)
        one = torch.full((F * V, D), 0.1, device=dev)                 # the one-slot kinds' slot
        rec = torch.full((F * V, 2, D), 0.1, device=dev)              # two slots of a row side by side
        stamp = torch.zeros(F * V, dtype=torch.int32, device=dev)
        vals0 = torch.randn(n, D, device=dev, generator=gen)
        vals, rows = torch.empty_like(vals0), torch.empty(n, dtype=torch.int64, device=dev)

        def fresh():
            rows.copy_((torch.randint(0, V, (B, F), device=dev, generator=gen) + off).reshape(-1))

        def row_call(kind):
            stem, hp, ns = KINDS[kind]
            f = getattr(h, f'dt_{stem}_rows_step')
            slots = [ptr(one)] if ns == 1 else [ptr(rec[:, 0, :]), ptr(rec[:, 1, :])]
            extra, trail = ([ptr(stamp)], [1]) if stem == 'rmsprop' else ([], [])
            args = [ptr(table)] + slots + extra + [ptr(rows), ptr(vals), n, D, 0, ptr(hslots), n_slots, ptr(mark), *hp,
                                                   ptr(state), None, None] + [None] * ns + [0, 1, D * ns] + trail

            def call():
                check(f(*args, stream_ptr()), kind)
            return call

        def adam():
            check(h.dt_adam_rows_step(ptr(table), ptr(rec[:, 0, :]), ptr(rec[:, 1, :]), ptr(rows), ptr(vals), n, D, 0,
                                      ptr(hslots), n_slots, ptr(mark), 0.0, 0.9, 0.999, 1e-7, ptr(state), None, None, None,
                                      None, 0, 1, LR, stream_ptr()), 'adam')
        calls = {k: row_call(k) for k in KINDS}
        calls['adam'] = adam
        # the merge adds a row's duplicates into its first occurrence: every call starts from the same gradient rows
        lines.append(dict(head, what='rows', shape={'fields': F, 'rows_per_field': V, 'D': D, 'batch': B, 'lookups': n},
                          **timed(calls, each_round=fresh, each_call=lambda: vals.copy_(vals0))))
        del table, one, rec, stamp
    p, g = torch.randn(DENSE_N, device=dev), 1e-3 * torch.randn(DENSE_N, device=dev)
    s0, s1 = torch.full_like(p, 0.1), torch.full_like(p, 0.1)

    def dense_call(kind):
        stem, hp, ns = KINDS[kind]
        f = getattr(h, f'dt_{stem}_dense_step')
        args = [ptr(p), ptr(g), ptr(s0)] + ([ptr(s1)] if ns == 2 else []) + [DENSE_N, *hp, ptr(state), 1]
        return lambda: check(f(*args, stream_ptr()), kind)
    calls = {k: dense_call(k) for k in KINDS}
    calls['adam'] = lambda: check(h.dt_adam_dense_step(ptr(p), ptr(g), ptr(s0), ptr(s1), DENSE_N, 0.0, 0.9, 0.999, 1e-7,
                                                       ptr(state), 1, LR, stream_ptr()), 'adam')
    lines.append(dict(head, what='dense', shape={'n': DENSE_N}, **timed(calls)))
    for ln in lines:
        print(json.dumps(ln))
    if a.out:
        with open(a.out, 'a') as f:
            f.writelines(json.dumps(ln) + '\n' for ln in lines)


if __name__ == '__main__':
    main()
