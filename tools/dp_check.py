"""Two-rank rehearsal of the data-parallel path on ONE GPU (gloo instead of RCCL, both ranks on device 0):
the graph-replayed iteration with the gradient sink + the per-step arena all-reduce must leave every rank with the
same weights, and those must differ from what a rank would have learnt alone (the exchange is live).

    T2V_DIST_BACKEND=gloo T2V_SINGLE_DEVICE=1 python -m torch.distributed.run --nproc-per-node 2 \\
        --master-addr 127.0.0.1 --master-port 29531 tools/dp_check.py [--discrim_steps N] [--gen_steps M] [--cond [--ca_dim D]] [--D_sn]

With a schedule other than 1:1 the line also reports the graphs and the exchanges ('D' / 'G') of one replayed iteration.
--cond: the text-conditioned models (a randomly initialised Bi-LSTM sentence encoder, 8-token captions per rank); --ca_dim D > 0
puts the generator's conditioning augmentation in front of its fc (built here: bench.build_models has no such argument).
--D_sn: spectral normalisation of the discriminator; its master weights, u, v and sigma join the compared state.
"""
import argparse
import os
import random
import sys

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench                                                                    # noqa: E402
from txt2vid_amd import dist as tdist, functional as TF                         # noqa: E402
from txt2vid_amd.gan.trainer import GraphedTrainStep                            # noqa: E402

rank, world = tdist.init_from_env('nccl')
assert world == 2
dev = torch.device('cuda', tdist.local_device_index())
torch.cuda.set_device(dev)
B = 4
ap = argparse.ArgumentParser()
ap.add_argument('--discrim_steps', type=int, default=1)
ap.add_argument('--gen_steps', type=int, default=1)
ap.add_argument('--cond', action='store_true')
ap.add_argument('--ca_dim', type=int, default=0)
ap.add_argument('--D_sn', action='store_true')
args = ap.parse_args()
if args.ca_dim and not args.cond:
    ap.error('--ca_dim needs --cond')


class Params(bench.Params):
    discrim_steps = args.discrim_steps
    gen_steps = args.gen_steps


def build_cond(seed=100):
    """bench.build_models(cond=True) with the generator's conditioning augmentation, plus the sentence encoder."""
    from txt2vid_amd.models.tganv2_cond.gen import MultiScaleGen
    from txt2vid_amd.models.tganv2_cond.discrim import MultiScaleDiscrim
    from txt2vid_amd.models.txt.basic import Seq2Seq
    from txt2vid_amd.data import Vocab
    from txt2vid_amd.gan.cond_gan import CondGan
    from txt2vid_amd.gan.losses import MixedGanLoss, RSGANLoss
    from txt2vid_amd.optim import Adam
    from txt2vid_amd.util.torch.init import init
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    gen = MultiScaleGen(width=64, height=64, num_channels=1, cond_dim=256, ca_dim=args.ca_dim)
    dis = MultiScaleDiscrim(num_channels=1, cond_dim=256)
    txt = Seq2Seq(vocab_size=len(Vocab()))
    for m in (gen, dis, txt):
        init(m, 'xavier')
        m.to(dev)
    gen.train()
    dis.train()
    optD = Adam([{'params': dis.parameters()}], lr=2e-4, betas=(0.5, 0.999))
    optG = Adam([{'params': gen.parameters()}], lr=2e-4, betas=(0.5, 0.999))
    return gen, dis, optD, optG, MixedGanLoss(g_loss=RSGANLoss(), d_loss=RSGANLoss()), CondGan, txt


def run(sync):
    txt = None
    if args.cond:
        gen, dis, optD, optG, losses, CondGan, txt = build_cond()
    else:
        gen, dis, optD, optG, losses, CondGan = bench.build_models(dev)         # same seed -> identical replicas
    gan = CondGan(gen=gen, discrims=[dis], cond_encoder=txt, discrim_names=['video'], gp_scale=float(world if sync else 1))
    if args.D_sn:
        from txt2vid_amd.gan.spectral import SpectralNorm, attach
        attach(gan, optD, SpectralNorm([dis], seed=100))                        # same seed on every rank, like the weights
    gs = None
    if sync:
        arenas = {'D': tdist.model_arena(dis, TF.copy_into), 'G': tdist.model_arena(gen, TF.copy_into)}
        gs = tdist.make_grad_sync(arenas, {'D': optD, 'G': optG}, world)
    pool = bench.synthetic_batches(B, 2, 100 + rank, dev)                       # different data per rank
    random.seed(100 + rank)
    np.random.seed(100 + rank)
    torch.manual_seed(100 + rank)
    codes = None
    if txt is not None:                                                         # different captions per rank
        tg = torch.Generator()
        tg.manual_seed(200 + rank)
        tokens = torch.randint(4, txt.encoder.embed.num_embeddings, (B, 8), generator=tg).to(dev)
        with torch.no_grad():
            codes = txt.encode(tokens, [8] * B)[2].detach()
    step = GraphedTrainStep(gan, optD, optG, losses, Params(), dev, tuple(pool[0].shape), grad_sync=gs, warmup=2,
                            cond_dim=256 if txt is not None else 0)
    seen = []
    if gs is not None:
        exchange = gs.exchange

        def counted(which):
            seen.append(which)
            exchange(which)
        gs.exchange = counted
    for i in range(5):                                                          # 2 eager, capture, 2 replays
        del seen[:]
        lD, lG = step.step(pool[i % 2], codes)
    torch.cuda.synchronize()
    state = list(dis.parameters()) + list(gen.parameters())
    if args.D_sn:
        sn = gan.discrim_sn
        state += sn.orig + sn.u + sn.v + sn.sigma
    chk = torch.stack([p.detach().double().sum() for p in state] + [p.detach().double().abs().sum() for p in state])
    return chk, float(lD), float(lG), (step.n_graphs, ''.join(seen))


chk, lD, lG, (n_graphs, exchanges) = run(True)
both = [torch.empty_like(chk) for _ in range(world)]
dist.all_gather(both, chk.cpu().to(dev))
same = bool(torch.equal(both[0], both[1]))
solo, _, _, _ = run(False)
moved = float((solo - chk).abs().max())
if rank == 0:
    sched = ''
    if (args.discrim_steps, args.gen_steps) != (1, 1):
        sched = '; schedule %d:%d, %d graphs and exchanges %s per replayed iteration' % (args.discrim_steps, args.gen_steps,
                                                                                         n_graphs, exchanges)
    if args.cond:
        sched += '; text-conditioned, ca_dim %d' % args.ca_dim
    if args.D_sn:
        sched += '; spectral norm (W, u, v, sigma compared too)'
    print('DP_CHECK replicas identical after 5 iterations: %s; differs from a solo run by %.3e; lossD %.5f lossG %.5f%s' %
          (same, moved, lD, lG, sched))
    assert same and moved > 1e-6
dist.barrier()
dist.destroy_process_group()
