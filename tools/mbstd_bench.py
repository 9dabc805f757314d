"""Cost of the discriminator's minibatch standard deviation head (MultiScaleDiscrim(mbstd=G)): median ms per
graph-replayed training iteration (GraphedTrainStep, the whole iteration as one HIP graph) of the TGANv2 64x64x1, B clips, recipe
weights and a non-zero w, RSGAN + GP 0.5, Adam, fp32 — text-conditioned (fixed random sentence codes [B, 256]: the sentence
encoder runs outside the iteration's graph and is the same in every variant) or, with --uncond, unconditional. Three variants,
mbstd off / on / off, alternated block by block: the two `off` variants are the same program built twice, so their difference is
the spread the added time has to be read against.
  python tools/mbstd_bench.py [--batch 32] [--group 4] [--uncond] [--iters 20] [--rounds 5] [--only off|on] [--out profiles/mbstd_bench.json]
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
W = (40.0, -60.0)                                   # (w_u, w_c): the term next to the recipe logits in size (tests/mbstd_cases.py)


class Prm(object):
    frame_sizes = [8, 16, 32, 64]
    subsample_input = True
    discrim_steps = gen_steps = 1
    gp_lambda = 0.5
    no_mean_discrim_loss = no_mean_gen_loss = True


def make(group, cond):
    from txt2vid_amd.gan.cond_gan import CondGan
    from txt2vid_amd.gan.losses import MixedGanLoss, RSGANLoss
    from txt2vid_amd.optim import Adam
    if cond:
        from txt2vid_amd.models.tganv2_cond.gen import MultiScaleGen
        from txt2vid_amd.models.tganv2_cond.discrim import MultiScaleDiscrim
        gen = MultiScaleGen(width=64, height=64, num_channels=1, cond_dim=256)
        dis = MultiScaleDiscrim(num_channels=1, cond_dim=256, mbstd=group)
    else:
        from txt2vid_amd.models.tganv2.gen import MultiScaleGen
        from txt2vid_amd.models.tganv2.discrim import MultiScaleDiscrim
        gen = MultiScaleGen(width=64, height=64, num_channels=1)
        dis = MultiScaleDiscrim(num_channels=1, mbstd=group)
    for m in (gen, dis):
        sd = {k: O.recipe_tensor(k, v.shape) for k, v in m.state_dict().items()}
        for k in sd:
            if k.endswith('mbstd.weight'):
                sd[k] = torch.tensor(W[:sd[k].numel()])
        m.load_state_dict(sd)
        m.to(DEV).train()
    gan = CondGan(gen=gen, discrims=[dis], discrim_names=['video'])
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
    ap.add_argument('--group', type=int, default=4)
    ap.add_argument('--uncond', action='store_true')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--only', choices=['off', 'on'])
    ap.add_argument('--out')
    a = ap.parse_args()
    limit_host_threads()
    from txt2vid_amd.gan.trainer import GraphedTrainStep
    random.seed(0)
    np.random.seed(0)
    torch.manual_seed(0)
    B, cond_dim = a.batch, 0 if a.uncond else 256
    g = torch.Generator()
    g.manual_seed(1)
    x = (torch.rand(B, 1, 16, 64, 64, generator=g) * 2 - 1).to(DEV)
    cond = (0.5 * torch.randn(B, 256, generator=g)).to(DEV) if cond_dim else None
    names = [a.only] if a.only else ['off_a', 'on', 'off_b']
    runs = {}
    for name in names:
        gan, optD, optG, losses = make(a.group if name == 'on' else 0, bool(cond_dim))
        gs = GraphedTrainStep(gan, optD, optG, losses, Prm(), DEV, (B, 1, 16, 64, 64), warmup=3, cond_dim=cond_dim)
        for _ in range(5):                                  # 3 eager + capture + replays: every shape warm
            gs.step(x, cond)
        torch.cuda.synchronize()
        runs[name] = gs
    res = {k: [] for k in runs}
    for _ in range(a.rounds):                               # alternate the variants: same machine state for all
        for k, gs in runs.items():
            res[k].append(events_ms(lambda: gs.step(x, cond), a.iters))
    out = {'workload': '%s TGANv2 64x64x1, B=%d, RSGAN + GP 0.5, Adam, fp32%s; the whole iteration graph-replayed; mbstd off / on '
                       '(G=%d) / off alternated' % ('text-conditioned' if cond_dim else 'unconditional', B,
                                                    ', fixed sentence codes' if cond_dim else '', a.group),
           'gpu': torch.cuda.get_device_name(0), 'iters_per_round': a.iters, 'rounds': a.rounds, 'group': a.group}
    for k, v in res.items():
        out['mbstd_%s' % k] = {'iter_ms': {'median': float(np.median(v)), 'min': float(min(v)), 'max': float(max(v))},
                               'graph_replayed': runs[k].graphs is not None}
    if not a.only:
        med = {k: out['mbstd_%s' % k]['iter_ms']['median'] for k in res}
        out['off_spread_ms'] = abs(med['off_a'] - med['off_b'])
        out['mbstd_cost_ms'] = med['on'] - 0.5 * (med['off_a'] + med['off_b'])
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
