"""Cost of the opt-in averaged generator (--G_ema): unconditional TGANv2 64x64x1, B frames, recipe weights, Adam,
RSGAN + GP 0.5 (bench.py's workload), the whole iteration graph-replayed —
  * median ms per iteration without and with `GenAverage(gen, 0.999)`, the two alternated block by block;
  * the update on its own (tick + t2v_ema_multi over the average's job list, back-to-back launches) and its GB/s at 12 B per
    live element, next to `t2v_adam_multi` over the same tensors (28 B per element) timed the same way in the same run.
Back-to-back launches over a working set near the 256 MB Infinity Cache flatter a streaming kernel; the in-iteration overhead is
the figure that counts.
  python tools/ema_bench.py [--batch 32] [--iters 20] [--rounds 5] [--out result.json]"""
import argparse
import json
import os
import random
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from txt2vid_amd.util.misc import limit_host_threads  # noqa: E402
from steps_bench import make, events_ms  # noqa: E402

DEV = 'cuda:0'


def adam_items(opt):
    """The (p, g, exp_avg, exp_avg_sq) list `optim.Adam.step` hands to t2v_adam_multi (live taps only)."""
    from txt2vid_amd import functional as TF
    items = []
    for group in opt.param_groups:
        for p in group['params']:
            st = opt.state[p]
            g = p.grad
            if g is None or g.stride() != p.stride():        # (timing only: any tensor laid out like p reads the same bytes)
                g = torch.zeros_like(st['exp_avg'])
            ts = (p, g, st['exp_avg'], st['exp_avg_sq'])
            live = getattr(p, '_t2v_live_taps', None)
            if live is not None and not p.is_contiguous() and TF.is_tap_major(p):
                rows = [TF.tap_rows(t) for t in ts]
                items.extend(tuple(r[t] for r in rows) for t in live)
            else:
                items.append(ts)
    return items


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--decay', type=float, default=0.999)
    ap.add_argument('--out')
    a = ap.parse_args()
    limit_host_threads()
    from txt2vid_amd import functional as TF
    from txt2vid_amd.gan.ema import GenAverage
    from txt2vid_amd.gan.trainer import GraphedTrainStep
    random.seed(0)
    np.random.seed(0)
    torch.manual_seed(0)
    B = a.batch
    g = torch.Generator()
    g.manual_seed(1)
    x = (torch.rand(B, 1, 16, 64, 64, generator=g) * 2 - 1).to(DEV)
    runs, parts = {}, {}
    for name in ('off', 'on'):
        gan, optD, optG, losses, prm = make(1, 1, 'rsgan', 0.5)
        if name == 'on':
            gan.gen_ema = GenAverage(gan.gen, a.decay)
        gs = GraphedTrainStep(gan, optD, optG, losses, prm, DEV, (B, 1, 16, 64, 64), warmup=3)
        for _ in range(5):                                  # 3 eager + capture + replays: every shape warm
            gs.step(x)
        torch.cuda.synchronize()
        runs[name], parts[name] = gs, (gan, optG)
    res = {n: [] for n in runs}
    for _ in range(a.rounds):                               # alternate: same machine state for both
        for n, gs in runs.items():
            res[n].append(events_ms(lambda: gs.step(x), a.iters))
    gan, optG = parts['on']
    ema = gan.gen_ema
    items = adam_items(optG)
    n_adam = sum(int(t[0].numel()) for t in items)
    grp = optG.param_groups[0]

    def adam_alone():          # lr = 0: the weights the graphs read stay what they are
        TF.adam_step_multi(items, 0.0, grp['betas'][0], grp['betas'][1], grp['eps'], 10, 1.0, None)
    for fn in (ema.update, adam_alone):
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    upd, adam = [], []
    for _ in range(a.rounds):
        upd.append(events_ms(ema.update, 200))
        adam.append(events_ms(adam_alone, 200))
    med = {n: float(np.median(v)) for n, v in res.items()}
    upd_ms, adam_ms = float(np.median(upd)), float(np.median(adam))
    out = {'workload': 'unconditional TGANv2 64x64x1, B=%d, Adam, RSGAN + GP 0.5; the whole iteration graph-replayed' % B,
           'gpu': torch.cuda.get_device_name(0), 'iters_per_round': a.iters, 'rounds': a.rounds, 'decay': a.decay,
           'graph_replayed': all(gs.graphs is not None for gs in runs.values()),
           'iter_ms': {n: {'median': med[n], 'min': float(min(v)), 'max': float(max(v))} for n, v in res.items()},
           'ema_overhead_ms': med['on'] - med['off'], 'ema_overhead_pct': 100.0 * (med['on'] - med['off']) / med['off'],
           'update': {'jobs': ema.n_jobs, 'launches': 1 + len(ema._update_calls), 'live_elements': ema.live_elements,
                      'bytes': 12 * ema.live_elements, 'ms': upd_ms, 'min_ms': float(min(upd)), 'max_ms': float(max(upd)),
                      'GBps': 12e-6 * ema.live_elements / upd_ms, 'timing': 'tick + update, 200 back-to-back calls per round'},
           'adam_multi': {'jobs': len(items), 'elements': n_adam, 'bytes': 28 * n_adam, 'ms': adam_ms,
                          'GBps': 28e-6 * n_adam / adam_ms, 'timing': '200 back-to-back calls per round'},
           'updates_seen': ema.updates}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
