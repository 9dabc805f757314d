"""Cost of the geometric names of --D_aug (flip, scale, rotate) over the colour / translation / cutout policy:
unconditional TGANv2 64x64x1, B frames, recipe weights, Adam, RSGAN + GP 0.5 (bench.py's workload), the whole iteration
graph-replayed —
  * median ms per iteration with `--D_aug color,translation,cutout`, with the six-name policy (one more block of draws per site,
    one resampling launch in front of every augmentation launch), and with the three-name policy again, the three alternated
    block by block: the cost is the difference against the first variant, to be read against the difference between the two
    identical variants;
  * the calls of the augmentation entry points during the captured pass (= the launches the names add to a replayed iteration).
There is no time threshold; the condition that stands in for one is the launch budget (tests/test_geoaug_gpu.py).
  python tools/geoaug_bench.py [--batch 32] [--iters 20] [--rounds 5] [--out profiles/geoaug_bench.json]"""
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
SIX = FULL + ',flip,scale,rotate'
NAMES = ('t2v_diffaug_fwd', 't2v_diffaug_bwd', 't2v_geoaug_fwd', 't2v_geoaug_bwd')


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
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'geoaug_bench.json'))
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
        for name, policy in (('aug', FULL), ('aug_geo', SIX), ('aug_again', FULL)):
            gan, optD, optG, losses, prm = make(1, 1, 'rsgan', 0.5)
            prm.D_aug = policy
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
    out = {'workload': 'unconditional TGANv2 64x64x1, B=%d, Adam, RSGAN + GP 0.5; the whole iteration graph-replayed' % B,
           'gpu': torch.cuda.get_device_name(0), 'iters_per_round': a.iters, 'rounds': a.rounds,
           'policies': {'aug': FULL, 'aug_geo': SIX, 'aug_again': FULL},
           'graph_replayed': all(gs.graphs is not None and gs.n_graphs == 1 for gs in runs.values()),
           'iter_ms': {n: {'median': med[n], 'min': float(min(v)), 'max': float(max(v))} for n, v in res.items()},
           'overhead_ms': med['aug_geo'] - med['aug'], 'overhead_pct': 100.0 * (med['aug_geo'] - med['aug']) / med['aug'],
           'aug_vs_aug_again_ms': med['aug_again'] - med['aug'],
           'calls_in_captured_pass': captured}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
