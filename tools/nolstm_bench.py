"""MultiScaleGen(no_lstm=True) — TGAN-v1's frame-seed generator — against the default ConvLSTM generator, unconditional,
B frames of 64x64x1, recipe weights, RSGAN + GP 0.5, Adam:
  * ms per training iteration, graph-replayed (GraphedTrainStep, one HIP graph per iteration), the two models alternated
    block by block so that both see the same machine state;
  * ms of the generator's forward + backward alone (eager; a fixed random projection of the pyramid as the loss).
  python tools/nolstm_bench.py [--batch 32] [--iters 30] [--rounds 3] [--only nolstm|lstm] [--out result.json]
`--only` runs one model (the profiler run of DESIGN §12 traces `--only nolstm`)."""
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


def make(no_lstm):
    from txt2vid_amd.models.tganv2.gen import MultiScaleGen
    from txt2vid_amd.models.tganv2.discrim import MultiScaleDiscrim
    from txt2vid_amd.gan.cond_gan import CondGan
    from txt2vid_amd.gan.losses import MixedGanLoss, RSGANLoss
    from txt2vid_amd.optim import Adam
    gen = MultiScaleGen(width=64, height=64, num_channels=1, no_lstm=no_lstm)
    dis = MultiScaleDiscrim(num_channels=1)
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


def gen_fwd_bwd(gen, B, TF):
    """One forward + backward of the generator on a fixed z, loss = a fixed random projection of the pyramid. Outside the
    training step: no gradient sink, and the gradients are returned instead of accumulated into the parameters' .grad
    (which the captured iteration owns)."""
    z = torch.randn(B, 256, device=DEV)
    params = list(gen.parameters())
    projs = []

    def run():
        old = TF.set_grad_sink(None)
        try:
            fake = gen(z)
            if not projs:
                projs.extend(torch.randn(f.shape, device=DEV) for f in fake)
            torch.autograd.grad(sum((f * p).sum() for f, p in zip(fake, projs)), params)
        finally:
            TF.set_grad_sink(old)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--only', choices=['nolstm', 'lstm'])
    ap.add_argument('--out')
    a = ap.parse_args()
    limit_host_threads()
    from txt2vid_amd import functional as TF
    from txt2vid_amd.gan.trainer import GraphedTrainStep
    random.seed(0)
    np.random.seed(0)
    torch.manual_seed(0)
    B = a.batch
    names = [a.only] if a.only else ['nolstm', 'lstm']
    g = torch.Generator()
    g.manual_seed(1)
    x = (torch.rand(B, 1, 16, 64, 64, generator=g) * 2 - 1).to(DEV)
    runs = {}
    for n in names:
        gan, optD, optG, losses = make(n == 'nolstm')
        gs = GraphedTrainStep(gan, optD, optG, losses, Prm(), DEV, (B, 1, 16, 64, 64), warmup=3)
        for _ in range(5):                                  # 3 eager + capture + replays: every shape warm
            gs.step(x)
        torch.cuda.synchronize()
        g_fwd_bwd = gen_fwd_bwd(gan.gen, B, TF)
        for _ in range(3):
            g_fwd_bwd()
        torch.cuda.synchronize()
        runs[n] = (gs, g_fwd_bwd)
    res = {n: {'iter_ms': [], 'g_fwd_bwd_ms': []} for n in names}
    for _ in range(a.rounds):                               # alternate the models: same machine state for both
        for n in names:
            gs, fb = runs[n]
            res[n]['iter_ms'].append(events_ms(lambda: gs.step(x), a.iters))
            res[n]['g_fwd_bwd_ms'].append(events_ms(fb, a.iters))
    out = {'workload': 'unconditional TGANv2 64x64x1, B=%d, RSGAN + GP 0.5, Adam; iteration graph-replayed, G fwd+bwd eager' % B,
           'gpu': torch.cuda.get_device_name(0), 'iters_per_round': a.iters}
    for n in names:
        out[n] = {k: {'median': float(np.median(v)), 'min': float(min(v)), 'max': float(max(v))} for k, v in res[n].items()}
        out[n]['graph_replayed'] = runs[n][0].graphs is not None
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
