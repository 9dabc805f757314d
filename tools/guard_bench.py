"""Cost of the gradient guard inside the replayed graph (--grad_guard / --D_clip / --G_clip): unconditional TGANv2
64x64x1, B frames, recipe weights, Adam, RSGAN + GP 0.5 (bench.py's workload), the whole iteration graph-replayed —
  * median ms per iteration with the flags off, with `--grad_guard`, with `--D_clip 1 --G_clip 1`, and with the flags off again,
    the four alternated block by block: the cost is the difference against the first variant, to be read against the difference
    between the two identical variants;
  * the calls of the optimiser's entry points during the captured pass, and the launches the feature adds per replayed
    iteration: per optimiser step ceil(jobs / 64) sumsq launches, the decision, and nothing else (the guarded tick and updates
    replace the unguarded ones launch for launch).
There is no time threshold; the expectation is one more read of every gradient plus these small launches.
  python tools/guard_bench.py [--batch 32] [--iters 20] [--rounds 5] [--out profiles/guard_bench.json]"""
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
NAMES = ('t2v_grad_sumsq_multi', 't2v_grad_guard', 't2v_adam_tick_guard', 't2v_adam_multi_guard', 't2v_adam_multi', 't2v_adam_tick')
JOBS = ('t2v_grad_sumsq_multi',)


class Counter(object):
    """Counting wrappers around the entry points of the loaded library (the way the tests count them)."""

    def __init__(self):
        from txt2vid_amd import functional as TF
        self.lib = TF.lib()
        self.orig = {n: getattr(self.lib, n) for n in NAMES}
        self.calls = {n: 0 for n in NAMES}
        self.sumsq_launches = 0
        for n in NAMES:
            setattr(self.lib, n, self._wrap(n))

    def _wrap(self, n):
        def f(*a):
            self.calls[n] += 1
            if n in JOBS:
                self.sumsq_launches += (int(a[1]) + 63) // 64
            return self.orig[n](*a)
        return f

    def take(self):
        out, self.calls = dict(self.calls, sumsq_launches=self.sumsq_launches), {n: 0 for n in NAMES}
        self.sumsq_launches = 0
        return out

    def close(self):
        for n in NAMES:
            setattr(self.lib, n, self.orig[n])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--clip', type=float, default=1.0)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'guard_bench.json'))
    a = ap.parse_args()
    limit_host_threads()
    from txt2vid_amd.gan.trainer import GraphedTrainStep
    from txt2vid_amd.gan.grad_guard import GradGuard
    random.seed(0)
    np.random.seed(0)
    torch.manual_seed(0)
    B = a.batch
    g = torch.Generator()
    g.manual_seed(1)
    x = (torch.rand(B, 1, 16, 64, 64, generator=g) * 2 - 1).to(DEV)
    counter = Counter()
    runs, captured, guards = {}, {}, {}
    try:
        for name, clips in (('off', None), ('grad_guard', (None, None)), ('clip', (a.clip, a.clip)), ('off_again', None)):
            gan, optD, optG, losses, prm = make(1, 1, 'rsgan', 0.5)
            if clips is not None:
                guards[name] = GradGuard(clips[0], clips[1], DEV).attach(optD, optG)
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
    added = {n: captured[n]['sumsq_launches'] + captured[n]['t2v_grad_guard'] for n in guards}
    out = {'workload': 'unconditional TGANv2 64x64x1, B=%d, Adam, RSGAN + GP 0.5; the whole iteration graph-replayed' % B,
           'gpu': torch.cuda.get_device_name(0), 'iters_per_round': a.iters, 'rounds': a.rounds,
           'guard': {n: dict(g.config(), state_end=g.read()) for n, g in guards.items()},
           'graph_replayed': all(gs.graphs is not None and gs.n_graphs == 1 for gs in runs.values()),
           'iter_ms': {n: {'median': med[n], 'min': float(min(v)), 'max': float(max(v))} for n, v in res.items()},
           'overhead_ms': {n: med[n] - med['off'] for n in guards},
           'overhead_pct': {n: 100.0 * (med[n] - med['off']) / med['off'] for n in guards},
           'off_vs_off_again_ms': med['off_again'] - med['off'],
           'calls_in_captured_pass': captured, 'launches_added_per_replayed_iteration': added}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
