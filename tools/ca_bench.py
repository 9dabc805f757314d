"""Cost of the generator's conditioning augmentation (MultiScaleGen(ca_dim=D)): median ms per graph-replayed
training iteration (GraphedTrainStep, the whole iteration as one HIP graph) of the text-conditioned TGANv2 64x64x1, B clips,
recipe weights, RSGAN + GP 0.5, Adam, with CA off and on, in fp32 and in bf16-compute mode. The sentence codes are a fixed
random [B, 256] buffer: the sentence encoder runs outside the iteration's graph and is the same in every variant. The variants
are alternated block by block so that all of them see the same machine state.
  python tools/ca_bench.py [--batch 32] [--ca_dim 128] [--iters 20] [--rounds 3] [--only off|on] [--out result.json]
`--only` runs one CA setting (fp32 and bf16) — for a kernel trace of the replayed iterations."""
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


def make(ca_dim):
    from txt2vid_amd.models.tganv2_cond.gen import MultiScaleGen
    from txt2vid_amd.models.tganv2_cond.discrim import MultiScaleDiscrim
    from txt2vid_amd.gan.cond_gan import CondGan
    from txt2vid_amd.gan.losses import MixedGanLoss, RSGANLoss
    from txt2vid_amd.optim import Adam
    gen = MultiScaleGen(width=64, height=64, num_channels=1, cond_dim=256, ca_dim=ca_dim)
    dis = MultiScaleDiscrim(num_channels=1, cond_dim=256)
    for m in (gen, dis):
        m.load_state_dict({k: O.recipe_tensor(k, v.shape) for k, v in m.state_dict().items()})
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
    ap.add_argument('--ca_dim', type=int, default=128)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--only', choices=['off', 'on'])
    ap.add_argument('--out')
    a = ap.parse_args()
    limit_host_threads()
    from txt2vid_amd import functional as TF
    from txt2vid_amd.gan.trainer import GraphedTrainStep
    random.seed(0)
    np.random.seed(0)
    torch.manual_seed(0)
    B = a.batch
    g = torch.Generator()
    g.manual_seed(1)
    x = (torch.rand(B, 1, 16, 64, 64, generator=g) * 2 - 1).to(DEV)
    cond = (0.5 * torch.randn(B, 256, generator=g)).to(DEV)
    names = [(ca, prec) for ca in ([a.only] if a.only else ['off', 'on']) for prec in ('fp32', 'bf16')]
    runs = {}
    for ca, prec in names:
        old = TF.set_conv_precision(prec)             # the precision is baked into the captured graph
        try:
            gan, optD, optG, losses = make(a.ca_dim if ca == 'on' else 0)
            gs = GraphedTrainStep(gan, optD, optG, losses, Prm(), DEV, (B, 1, 16, 64, 64), warmup=3, cond_dim=256)
            for _ in range(5):                              # 3 eager + capture + replays: every shape warm
                gs.step(x, cond)
            torch.cuda.synchronize()
        finally:
            TF.set_conv_precision(old)
        runs[(ca, prec)] = gs
    res = {k: [] for k in runs}
    for _ in range(a.rounds):                               # alternate the variants: same machine state for all
        for k, gs in runs.items():
            res[k].append(events_ms(lambda: gs.step(x, cond), a.iters))
    out = {'workload': 'text-conditioned TGANv2 64x64x1, B=%d, RSGAN + GP 0.5, Adam, fixed sentence codes; the whole iteration '
                       'graph-replayed; CA width %d' % (B, a.ca_dim),
           'gpu': torch.cuda.get_device_name(0), 'iters_per_round': a.iters, 'rounds': a.rounds}
    for (ca, prec), v in res.items():
        out['ca_%s_%s' % (ca, prec)] = {'iter_ms': {'median': float(np.median(v)), 'min': float(min(v)), 'max': float(max(v))},
                                        'graph_replayed': runs[(ca, prec)].graphs is not None}
    if not a.only:
        for prec in ('fp32', 'bf16'):
            out['ca_cost_ms_%s' % prec] = out['ca_on_%s' % prec]['iter_ms']['median'] - out['ca_off_%s' % prec]['iter_ms']['median']
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
