"""Cost of the contrastive clip-caption matching term (MultiScaleDiscrim(match=True) with --D_match 1 --G_match 1):
median ms per graph-replayed training iteration (GraphedTrainStep, the whole iteration as one HIP graph) of the text-conditioned
TGANv2 64x64x1, B clips, recipe weights, RSGAN + GP 0.5, Adam, fp32. The sentence codes are a fixed random [B, 256] buffer: the
sentence encoder runs outside the iteration's graph and is the same in every variant. Three variants, off / on / off, alternated
block by block in one session: the two `off` variants are the same program built twice, so their difference is the noise floor
the added time has to be read against.
  python tools/match_bench.py [--batch 32] [--iters 20] [--rounds 5] [--tau 0.1] [--only off|on] [--out profiles/match_bench.json]
`--only` runs one setting — for a kernel trace of the replayed iterations (collect it in a run of its own)."""
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


class Prm(object):
    frame_sizes = [8, 16, 32, 64]
    subsample_input = True
    discrim_steps = gen_steps = 1
    gp_lambda = 0.5
    no_mean_discrim_loss = no_mean_gen_loss = True


def make(match, tau):
    from txt2vid_amd.models.tganv2_cond.gen import MultiScaleGen
    from txt2vid_amd.models.tganv2_cond.discrim import MultiScaleDiscrim
    from txt2vid_amd.gan.cond_gan import CondGan
    from txt2vid_amd.gan.losses import MixedGanLoss, RSGANLoss
    from txt2vid_amd.gan.match import MatchState
    from txt2vid_amd.optim import Adam
    gen = MultiScaleGen(width=64, height=64, num_channels=1, cond_dim=256)
    dis = MultiScaleDiscrim(num_channels=1, cond_dim=256, match=match)
    for m in (gen, dis):
        m.load_state_dict({k: O.recipe_tensor(k, v.shape) for k, v in m.state_dict().items()})
        m.to(DEV).train()
    gan = CondGan(gen=gen, discrims=[dis], discrim_names=['video'])
    if match:
        gan.match = MatchState(1.0, 1.0, tau, DEV)
    optD = Adam([{'params': dis.parameters()}], lr=2e-4, betas=(0.5, 0.999))
    optG = Adam([{'params': gen.parameters()}], lr=2e-4, betas=(0.5, 0.999))
    return gan, optD, optG, MixedGanLoss(g_loss=RSGANLoss(), d_loss=RSGANLoss())


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
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--tau', type=float, default=0.1)
    ap.add_argument('--only', choices=['off', 'on'])
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
    cond = (0.5 * torch.randn(B, 256, generator=g)).to(DEV)
    names = [a.only] if a.only else ['off_a', 'on', 'off_b']
    runs = {}
    for name in names:
        gan, optD, optG, losses = make(name == 'on', a.tau)
        gs = GraphedTrainStep(gan, optD, optG, losses, Prm(), DEV, (B, 1, 16, 64, 64), warmup=3, cond_dim=256)
        for _ in range(5):                                  # 3 eager + capture + replays: every shape warm
            gs.step(x, cond)
        torch.cuda.synchronize()
        runs[name] = gs
    res = {k: [] for k in runs}
    for _ in range(a.rounds):                               # alternate the variants: same machine state for all
        for k, gs in runs.items():
            res[k].append(events_ms(lambda: gs.step(x, cond), a.iters))
    out = {'workload': 'text-conditioned TGANv2 64x64x1, B=%d, RSGAN + GP 0.5, Adam, fp32, fixed sentence codes; the whole '
                       'iteration graph-replayed; matching term (D and G step, weight 1, tau %g) off / on / off alternated' % (B, a.tau),
           'gpu': torch.cuda.get_device_name(0), 'iters_per_round': a.iters, 'rounds': a.rounds}
    for k, v in res.items():
        out['match_%s' % k] = {'iter_ms': {'median': float(np.median(v)), 'min': float(min(v)), 'max': float(max(v))},
                               'graph_replayed': runs[k].graphs is not None}
    if 'on' in runs:
        out['stats_d'], out['stats_g'] = runs['on'].ts.gan.match.stats_d.tolist(), runs['on'].ts.gan.match.stats_g.tolist()
    if not a.only:
        med = {k: out['match_%s' % k]['iter_ms']['median'] for k in res}
        out['off_spread_ms'] = abs(med['off_a'] - med['off_b'])
        out['match_cost_ms'] = med['on'] - 0.5 * (med['off_a'] + med['off_b'])
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
