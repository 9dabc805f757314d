"""Cost of the opt-in differentiable augmentation of the discriminator's inputs (--D_aug): unconditional TGANv2
64x64x1, B frames, recipe weights, Adam, RSGAN + GP 0.5 (bench.py's workload), the whole iteration graph-replayed —
  * median ms per iteration with the flag off and with the full policy (color,translation,cutout), the two alternated block by
    block, plus a second flag-off instance: the difference between the two flag-off instances is the spread a difference between
    off and on has to be read against;
  * the calls of the two new entry points during the captured pass (= the launches the policy adds to a replayed iteration) and
    their member counts.
  python tools/diffaug_bench.py [--batch 32] [--iters 20] [--rounds 5] [--out result.json]"""
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
FULL = 'color,translation,cutout'
NAMES = ('t2v_diffaug_fwd', 't2v_diffaug_bwd')


class Counter(object):
    """Counting wrappers around the two entry points of the loaded library (the way the tests count them)."""

    def __init__(self):
        from txt2vid_amd import functional as TF
        self.lib = TF.lib()
        self.orig = {n: getattr(self.lib, n) for n in NAMES}
        self.calls = {n: [] for n in NAMES}
        for n in NAMES:
            setattr(self.lib, n, self._wrap(n))

    def _wrap(self, n):
        def f(*a):
            self.calls[n].append(int(a[1]))
            return self.orig[n](*a)
        return f

    def take(self):
        out, self.calls = self.calls, {n: [] for n in NAMES}
        return out

    def close(self):
        for n in NAMES:
            setattr(self.lib, n, self.orig[n])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out')
    a = ap.parse_args()
    limit_host_threads()
    from txt2vid_amd.gan.trainer import GraphedTrainStep
    random.seed(0)
    np.random.seed(0)
    torch.manual_seed(0)
    B = a.batch
    g = torch.Generator()
    g.manual_seed(1)
    x = (torch.rand(B, 1, 16, 64, 64, generator=g) * 2 - 1).to(DEV)
    counter = Counter()
    runs, captured = {}, {}
    try:
        for name, policy in (('off', ''), ('on', FULL), ('off_again', '')):
            gan, optD, optG, losses, prm = make(1, 1, 'rsgan', 0.5)
            prm.D_aug = policy
            gs = GraphedTrainStep(gan, optD, optG, losses, prm, DEV, (B, 1, 16, 64, 64), warmup=3)
            for i in range(5):                              # 3 eager + capture + replays: every shape warm
                counter.take()
                gs.step(x)
                if i == 3:
                    captured[name] = counter.take()         # the Python pass that was captured
            torch.cuda.synchronize()
            replay_calls = counter.take()
            assert not any(replay_calls.values())           # a replay makes no call through the library handle
            runs[name] = gs
    finally:
        counter.close()
    res = {n: [] for n in runs}
    for _ in range(a.rounds):                               # alternate: same machine state for all
        for n, gs in runs.items():
            res[n].append(events_ms(lambda: gs.step(x), a.iters))
    med = {n: float(np.median(v)) for n, v in res.items()}
    out = {'workload': 'unconditional TGANv2 64x64x1, B=%d, Adam, RSGAN + GP 0.5; the whole iteration graph-replayed' % B,
           'gpu': torch.cuda.get_device_name(0), 'iters_per_round': a.iters, 'rounds': a.rounds, 'policy': FULL,
           'graph_replayed': all(gs.graphs is not None for gs in runs.values()),
           'iter_ms': {n: {'median': med[n], 'min': float(min(v)), 'max': float(max(v))} for n, v in res.items()},
           'overhead_ms': med['on'] - med['off'], 'overhead_pct': 100.0 * (med['on'] - med['off']) / med['off'],
           'off_vs_off_again_ms': med['off_again'] - med['off'],
           'added_launches_per_iteration': {n: {'launches': len(captured['on'][n]), 'members': captured['on'][n]} for n in NAMES},
           'added_launches_flag_off': sum(len(v) for v in captured['off'].values())}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
