"""Cost of the --discrim_steps N / --gen_steps M schedule: median ms per graph-replayed training iteration (GraphedTrainStep, the
whole unrolled iteration as one HIP graph), unconditional TGANv2 64x64x1, B frames, recipe weights, Adam, for
  1:1  RSGAN + GP 0.5 (the canonical schedule, bench.py's workload)
  2:2  RSGAN + GP 0.5
  5:1  WassersteinGanLoss + GP 10, Adam betas (0, 0.9) — the WGAN-GP recipe of the reference's scripts/run_tgan.sh
the schedules alternated block by block so that all of them see the same machine state.
  python tools/steps_bench.py [--batch 32] [--iters 20] [--rounds 3] [--out result.json]"""
import argparse
import json
import os
import random
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import tganv2_oracle as O  # noqa: E402
from txt2vid_amd.util.misc import limit_host_threads  # noqa: E402

DEV = 'cuda:0'
SCHEDULES = {'1:1': (1, 1, 'rsgan', 0.5), '2:2': (2, 2, 'rsgan', 0.5), '5:1': (5, 1, 'wasserstein', 10.0)}


def make(N, M, loss, gp):
    from txt2vid_amd.models.tganv2.gen import MultiScaleGen
    from txt2vid_amd.models.tganv2.discrim import MultiScaleDiscrim
    from txt2vid_amd.gan.cond_gan import CondGan
    from txt2vid_amd.gan.losses import MixedGanLoss, RSGANLoss, WassersteinGanLoss
    from txt2vid_amd.optim import Adam
    gen = MultiScaleGen(width=64, height=64, num_channels=1)
    dis = MultiScaleDiscrim(num_channels=1)
    for m in (gen, dis):
        m.load_state_dict({k: O.recipe_tensor(k, v.shape) for k, v in m.state_dict().items()})
        m.to(DEV).train()
    gan = CondGan(gen=gen, discrims=[dis], discrim_names=['video'])
    betas = (0.5, 0.999) if loss == 'rsgan' else (0.0, 0.9)
    optD = Adam([{'params': dis.parameters()}], lr=2e-4, betas=betas)
    optG = Adam([{'params': gen.parameters()}], lr=2e-4, betas=betas)
    lc = RSGANLoss if loss == 'rsgan' else WassersteinGanLoss

    class Prm(object):
        frame_sizes = [8, 16, 32, 64]
        subsample_input = True
        discrim_steps, gen_steps, gp_lambda = N, M, gp
        no_mean_discrim_loss = no_mean_gen_loss = True
    return gan, optD, optG, MixedGanLoss(g_loss=lc(), d_loss=lc()), Prm()


def events_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=3)
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
    runs = {}
    for name, (N, M, loss, gp) in SCHEDULES.items():
        gan, optD, optG, losses, prm = make(N, M, loss, gp)
        gs = GraphedTrainStep(gan, optD, optG, losses, prm, DEV, (B, 1, 16, 64, 64), warmup=3)
        for _ in range(5):                                  # 3 eager + capture + replays: every shape warm
            gs.step(x)
        torch.cuda.synchronize()
        runs[name] = gs
    res = {n: [] for n in runs}
    for _ in range(a.rounds):                               # alternate the schedules: same machine state for all
        for n, gs in runs.items():
            res[n].append(events_ms(lambda: gs.step(x), a.iters))
    out = {'workload': 'unconditional TGANv2 64x64x1, B=%d, Adam; the whole N:M iteration graph-replayed' % B,
           'gpu': torch.cuda.get_device_name(0), 'iters_per_round': a.iters, 'rounds': a.rounds}
    for n, v in res.items():
        N, M, loss, gp = SCHEDULES[n]
        out[n] = {'discrim_steps': N, 'gen_steps': M, 'loss': loss, 'gp_lambda': gp, 'graph_replayed': runs[n].graphs is not None,
                  'iter_ms': {'median': float(np.median(v)), 'min': float(min(v)), 'max': float(max(v))}}
    base = out['1:1']['iter_ms']['median']
    out['extra_d_step_ms_5to1'] = (out['5:1']['iter_ms']['median'] - base) / 4.0
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
