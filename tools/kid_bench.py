"""Cost of the KID evaluation (`--eval_period`), three measurements in one process and one session:
  1. median ms per graph-replayed training iteration (unconditional TGANv2 64x64x1, B clips, recipe weights, RSGAN + GP 0.5, Adam,
     fp32) with the flag off / on / off, alternated block by block. `on` is what train() runs on an iteration that is not an
     evaluation iteration with a full real bank: the bank check in front of the step, the period check behind it. The two `off`
     variants are the same program built twice, so their difference is the spread the added time has to be read against.
  2. one evaluation at M clips in blocks of S: its wall time, and the same work timed in its three parts (generator forwards in
     eval mode, feature forwards of the generated clips, `t2v_kid_sums`).
  3. `t2v_kid_sums` alone at (n, d, s) = (M, 1024, S): ms, the nominal FLOP rate (3 Grams x 2 s^2 d per block, the symmetric halves
     counted although they are not computed) over the fp64 matrix peak, and as the yardstick the same sums in torch on the same
     tensors: `X.double() @ X.double().T` and so on plus the elementwise epilogue.
  python tools/kid_bench.py [--batch 32] [--clips 2048] [--block 1024] [--iters 20] [--rounds 5] [--out profiles/kid_bench.json]"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import tganv2_oracle as O  # noqa: E402
from txt2vid_amd.util.misc import limit_host_threads  # noqa: E402

DEV = 'cuda:0'
FP64_MATRIX_PEAK_TFLOPS = 78.6                      # MI355X data sheet: FP64 matrix


class Prm(object):
    frame_sizes = [8, 16, 32, 64]
    subsample_input = True
    discrim_steps = gen_steps = 1
    gp_lambda = 0.5
    no_mean_discrim_loss = no_mean_gen_loss = True


def make():
    from txt2vid_amd.gan.cond_gan import CondGan
    from txt2vid_amd.gan.losses import MixedGanLoss, RSGANLoss
    from txt2vid_amd.models.tganv2.gen import MultiScaleGen
    from txt2vid_amd.models.tganv2.discrim import MultiScaleDiscrim
    from txt2vid_amd.optim import Adam
    gen, dis = MultiScaleGen(width=64, height=64, num_channels=1), MultiScaleDiscrim(num_channels=1)
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


def stats(v):
    return {'median': float(np.median(v)), 'min': float(min(v)), 'max': float(max(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--clips', type=int, default=2048)
    ap.add_argument('--block', type=int, default=1024)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out')
    a = ap.parse_args()
    limit_host_threads()
    from txt2vid_amd import functional as TF
    from txt2vid_amd.functional_kid import kid_sums_raw
    from txt2vid_amd.gan.kid import KidEvaluator
    from txt2vid_amd.gan.trainer import GraphedTrainStep
    random.seed(0)
    np.random.seed(0)
    torch.manual_seed(0)
    B, M, S = a.batch, a.clips, a.block
    g = torch.Generator()
    g.manual_seed(1)
    x = (torch.rand(B, 1, 16, 64, 64, generator=g) * 2 - 1).to(DEV)
    out = {'workload': 'unconditional TGANv2 64x64x1, B=%d, RSGAN + GP 0.5, Adam, fp32; the whole iteration graph-replayed; KID with '
                       '%d clips in blocks of %d on the random-init feature network' % (B, M, S),
           'gpu': torch.cuda.get_device_name(0), 'iters_per_round': a.iters, 'rounds': a.rounds, 'clips': M, 'block': S}

    # ---- 1. the iteration, flag off / on / off ---------------------------------------------------------------------------------
    runs = {}
    for name in ('off_a', 'on', 'off_b'):
        gan, optD, optG, losses = make()
        kid = None
        if name == 'on':
            kid = gan.kid = KidEvaluator(gan, DEV, clips=M, block=S, num_channels=1, period=10 ** 9, sample_batch=B)
            t0 = time.perf_counter()
            while not kid.full:                              # distinct clips: a new draw per batch
                kid.observe((torch.rand(B, 1, 16, 64, 64, generator=g) * 2 - 1).to(DEV))
            torch.cuda.synchronize()
            out['fill_real_bank_s'] = time.perf_counter() - t0
        gs = GraphedTrainStep(gan, optD, optG, losses, Prm(), DEV, (B, 1, 16, 64, 64), warmup=3, cond_dim=0)
        for _ in range(5):                                   # 3 eager + capture + replays: every shape warm
            gs.step(x, None)
        torch.cuda.synchronize()
        runs[name] = (gs, kid)

    def body(gs, kid):
        def f():
            if kid is not None and not kid.full:
                kid.observe(x, None)
            gs.step(x, None)
            if kid is not None:
                kid.step(1)
        return f
    res = {k: [] for k in runs}
    for _ in range(a.rounds):                                # alternate the variants: same machine state for all
        for k, (gs, kid) in runs.items():
            res[k].append(events_ms(body(gs, kid), a.iters))
    for k, v in res.items():
        out['iter_%s' % k] = {'iter_ms': stats(v), 'graph_replayed': runs[k][0].graphs is not None}
    med = {k: out['iter_%s' % k]['iter_ms']['median'] for k in res}
    out['off_spread_ms'] = abs(med['off_a'] - med['off_b'])
    out['flag_cost_ms'] = med['on'] - 0.5 * (med['off_a'] + med['off_b'])

    # ---- 2. one evaluation ------------------------------------------------------------------------------------------------------
    gs, kid = runs['on']
    gan = kid.gan
    kid.evaluate(0)                                          # warm: every shape of the eval-mode forwards
    torch.cuda.synchronize()
    walls = []
    for _ in range(3):
        t0 = time.perf_counter()
        rec = kid.evaluate(0)
        walls.append((time.perf_counter() - t0) * 1e3)
    out['evaluation'] = {'wall_ms': stats(walls), 'kid': rec['kid'], 'stderr': rec['stderr'], 'alpha': rec['alpha']}
    gan.gen.eval()
    with torch.no_grad():
        fakes = [gan(kid.z[o:o + B])[-1] for o in range(0, min(M, 4 * B), B)]
        gen_ms = events_ms(lambda: gan(kid.z[:B])[-1], 10) * (M // B)
        feat_ms = events_ms(lambda: kid.features(fakes[0]), 10) * (M // B)
    gan.gen.train()
    sums_ms = [events_ms(lambda: kid_sums_raw(kid.real_bank, kid.fake_bank, S, kid.alpha, out=kid.sums, ws=kid.ws), 10) for _ in range(a.rounds)]
    out['evaluation'].update({'generator_forwards_ms': gen_ms, 'feature_forwards_ms': feat_ms, 'kid_sums_ms': float(np.median(sums_ms)),
                              'forwards': M // B, 'note': 'parts: 10 forwards of one batch timed by events, times the number of batches'})

    # ---- 3. t2v_kid_sums alone against torch ------------------------------------------------------------------------------------
    X, Y, alpha = kid.real_bank, kid.fake_bank, kid.alpha
    n, d = X.shape

    def torch_sums():
        Xd, Yd = X.double(), Y.double()
        rows = []
        for b in range(n // S):
            xb, yb = Xd[b * S:(b + 1) * S], Yd[b * S:(b + 1) * S]
            kxx, kyy, kxy = (alpha * (xb @ xb.T) + 1) ** 3, (alpha * (yb @ yb.T) + 1) ** 3, (alpha * (xb @ yb.T) + 1) ** 3
            rows.append(torch.stack([kxx.sum() - kxx.diagonal().sum(), kyy.sum() - kyy.diagonal().sum(), kxy.sum()]))
        return torch.stack(rows)
    ref = torch_sums()
    got = kid_sums_raw(X, Y, S, alpha)
    torch.cuda.synchronize()
    rel = float(((got - ref).abs() / ref.abs()).max())
    torch_ms = [events_ms(torch_sums, 10) for _ in range(a.rounds)]
    flop = 3 * (n // S) * 2.0 * S * S * d
    ms = float(np.median(sums_ms))
    out['kid_sums'] = {'n': n, 'd': d, 's': S, 'ms': stats(sums_ms), 'nominal_gflop': flop / 1e9, 'nominal_tflops': flop / (ms * 1e-3) / 1e12,
                       'fraction_of_fp64_matrix_peak': flop / (ms * 1e-3) / 1e12 / FP64_MATRIX_PEAK_TFLOPS,
                       'fp64_matrix_peak_tflops': FP64_MATRIX_PEAK_TFLOPS, 'torch_fp64_ms': stats(torch_ms),
                       'kernel_over_torch': ms / float(np.median(torch_ms)), 'max_rel_diff_to_torch': rel}
    TF.set_grad_sink(None)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
