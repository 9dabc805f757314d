"""Cost of the learning-rate decay inside the replayed graph (--lr_decay): unconditional TGANv2 64x64x1, B frames,
recipe weights, Adam, RSGAN + GP 0.5 (bench.py's workload), the whole iteration graph-replayed —
  * median ms per iteration without a schedule, with `--lr_decay linear --lr_decay_iters 100000` (one tick per optimiser step,
    the scheduled forms of the multi-tensor launches), and without a schedule again, the three alternated block by block: the
    cost is the difference against the first variant, to be read against the difference between the two identical variants;
  * the calls of the optimiser's entry points during the captured pass (= the launches a replayed iteration makes for them).
There is no time threshold; the expectation is a cost of the order of the one-thread launch --D_ada adds per D step
(profiles/ada_bench.json), twice: one tick for D, one for G.
  python tools/lr_bench.py [--batch 32] [--iters 20] [--rounds 5] [--out profiles/lr_sched_bench.json]"""
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
NAMES = ('t2v_lr_tick', 't2v_adam_multi_sched', 't2v_adam_multi', 't2v_adam_tick')


class Counter(object):
    """Counting wrappers around the entry points of the loaded library (the way the tests count them)."""

    def __init__(self):
        from txt2vid_amd import functional as TF
        self.lib = TF.lib()
        self.orig = {n: getattr(self.lib, n) for n in NAMES}
        self.calls = {n: 0 for n in NAMES}
        for n in NAMES:
            setattr(self.lib, n, self._wrap(n))

    def _wrap(self, n):
        def f(*a):
            self.calls[n] += 1
            return self.orig[n](*a)
        return f

    def take(self):
        out, self.calls = self.calls, {n: 0 for n in NAMES}
        return out

    def close(self):
        for n in NAMES:
            setattr(self.lib, n, self.orig[n])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--kind', default='linear', choices=('linear', 'cosine'))
    ap.add_argument('--decay_iters', type=int, default=100000)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'lr_sched_bench.json'))
    a = ap.parse_args()
    limit_host_threads()
    from txt2vid_amd.gan.trainer import GraphedTrainStep
    from txt2vid_amd.gan.lr_sched import LrSchedule
    random.seed(0)
    np.random.seed(0)
    torch.manual_seed(0)
    B = a.batch
    g = torch.Generator()
    g.manual_seed(1)
    x = (torch.rand(B, 1, 16, 64, 64, generator=g) * 2 - 1).to(DEV)
    counter = Counter()
    runs, captured, scheds = {}, {}, {}
    try:
        for name, on in (('off', False), ('lr_decay', True), ('off_again', False)):
            gan, optD, optG, losses, prm = make(1, 1, 'rsgan', 0.5)
            if on:                                          # the TGANv2 recipe: linear to zero
                scheds[name] = LrSchedule(a.kind, a.decay_iters, 0, 0.0, 1, 1, DEV).attach(optD, optG)
            gs = GraphedTrainStep(gan, optD, optG, losses, prm, DEV, (B, 1, 16, 64, 64), warmup=3)
            for i in range(5):                              # 3 eager + capture + replays: every shape warm
                counter.take()
                gs.step(x)
                if i == 3:
                    captured[name] = counter.take()         # the Python pass that was captured
            torch.cuda.synchronize()
            assert not any(counter.take().values())         # a replay makes no call through the library handle
            runs[name] = gs
    finally:
        counter.close()
    res = {n: [] for n in runs}
    for _ in range(a.rounds):                               # alternate: same machine state for all
        for n, gs in runs.items():
            res[n].append(events_ms(lambda: gs.step(x), a.iters))
    med = {n: float(np.median(v)) for n, v in res.items()}
    sched = scheds['lr_decay']
    out = {'workload': 'unconditional TGANv2 64x64x1, B=%d, Adam, RSGAN + GP 0.5; the whole iteration graph-replayed' % B,
           'gpu': torch.cuda.get_device_name(0), 'iters_per_round': a.iters, 'rounds': a.rounds,
           'lr_decay': dict(sched.config(), counters_end=sched.counters(),
                            factor_end=[float(sched.state[w][1]) for w in ('D', 'G')]),
           'graph_replayed': all(gs.graphs is not None and gs.n_graphs == 1 for gs in runs.values()),
           'iter_ms': {n: {'median': med[n], 'min': float(min(v)), 'max': float(max(v))} for n, v in res.items()},
           'overhead_ms': med['lr_decay'] - med['off'], 'overhead_pct': 100.0 * (med['lr_decay'] - med['off']) / med['off'],
           'off_vs_off_again_ms': med['off_again'] - med['off'],
           'calls_in_captured_pass': captured}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
