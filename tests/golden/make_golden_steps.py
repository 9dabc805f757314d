"""Golden vectors of the --discrim_steps N / --gen_steps M schedule (txt2vid/gan/trainer.py:221-263) — recorded by running the
REAL reference, from the repository root with a checkout of the reference first on the module path:

    PYTHONPATH=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_steps.py

Same runtime shims (imported with make_golden, which applies them), weight recipe and conventions as make_golden.py; the
unconditional `gen_step` is restated with `ff[0]` exactly as make_golden.golden_steps does (SURVEY §8(a) defect 1). Three
iterations of the loop body per case, uncond / cond TGANv2 64x64x1, B=4, recipe weights, Adam 2e-4 (0.5, 0.999):
  a  unconditional RSGAN + GP 0.5, N=2, M=2, --no_mean_discrim_loss --no_mean_gen_loss (each step's loss divided by N / M)
  b  unconditional WassersteinGanLoss (D and G) + GP 10, N=3, M=1, default means (no division)
  c  text-conditioned RSGAN + GP 0.5, N=2, M=1
Recorded per case: the logged losses (the per-iteration totals), the per-parameter gradient norms of the last D backward and
the last G backward of iterations 0 (`_gn0`) and 2 (`_gn`), the per-parameter norms of (parameter after iteration 2 - recipe
value), the Adam step counts and the generator's BatchNorm `num_batches_tracked` after iteration 2.
"""
import os
import random
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import (GenU, GenC, DisU, DisC, Seq2Seq, CondGan, MixedGanLoss, RSGANLoss, Subsample,   # noqa: E402
                         recipe_tensor, pour, grad_norms, save, pack_norms)
from txt2vid.gan.losses import WassersteinGanLoss                                                       # noqa: E402

CASES = {
    'a': dict(cond=False, loss='rsgan', gp=0.5, N=2, M=2, mean_d=True, mean_g=True),
    'b': dict(cond=False, loss='wasserstein', gp=10.0, N=3, M=1, mean_d=False, mean_g=False),
    'c': dict(cond=True, loss='rsgan', gp=0.5, N=2, M=1, mean_d=False, mean_g=False),
}


def _gen_step(gan, fake, real_pred, conds, losses):
    if conds is not None:
        return gan.gen_step(fake=fake, real_pred=real_pred, cond=conds, loss=losses.gen_loss)
    gan.gen.zero_grad()                                  # cond_gan.py:95 with `ff[0]` (make_golden.golden_steps)
    fc = gan.discrims[0](x=fake, cond=None, xbar=None)
    return torch.stack([losses.gen_loss(fake=ff[0], real=rr) for ff, rr in zip(fc, real_pred[0])]).mean()


def golden_case(tag, cond, loss, gp, N, M, mean_d, mean_g, out):
    B, V = 4, 21
    if cond:
        g = pour(GenC(width=64, height=64, num_channels=1, cond_dim=256))
        d = pour(DisC(num_channels=1, cond_dim=256))
        txt = Seq2Seq(vocab_size=V)
        txt.load_state_dict({k: recipe_tensor('encoder.' + k.split('.', 1)[1], v.shape) for k, v in txt.state_dict().items()})
    else:
        g = pour(GenU(width=64, height=64, num_channels=1))
        d = pour(DisU(num_channels=1))
        txt = None
    init = {m: {k: v.detach().clone() for k, v in mod.named_parameters()} for m, mod in (('G', g), ('D', d))}
    g.train()
    d.train()
    seed = 100
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    gan = CondGan(gen=g, discrims=[d], cond_encoder=txt, discrim_names=['video'])
    lc = RSGANLoss if loss == 'rsgan' else WassersteinGanLoss
    losses = MixedGanLoss(g_loss=lc(), d_loss=lc())
    optD = torch.optim.Adam([{'params': d.parameters()}], lr=2e-4, betas=(0.5, 0.999))
    optG = torch.optim.Adam([{'params': g.parameters()}], lr=2e-4, betas=(0.5, 0.999))
    ss = Subsample()
    fs = [8, 16, 32, 64]
    tokens = None
    if cond:
        tg = torch.Generator()
        tg.manual_seed(1234)
        tokens = torch.randint(4, V, (B, 8), generator=tg)
        tokens[:, 0], tokens[:, -1] = 1, 2
        out[tag + '_tokens'] = tokens.numpy()
    lD_all, lG_all = [], []
    for it in range(3):
        x = (torch.rand(B, 16, 1, 64, 64) * 2 - 1).permute(0, 2, 1, 3, 4)
        c = None
        if cond:
            _, _, c = gan.cond_encoder.encode(tokens, [8] * B)
            c = c.detach()
        xs, conds = [], ([] if cond else None)
        for i in range(4):                               # multiscale_data (trainer.py:131-165)
            xs.append(F.interpolate(x, size=(x.size(2), fs[i], fs[i])) if i != 3 else x)
            x, _ = ss(x)
            if cond:
                conds.append(c)
                c = c[::2]
        z = torch.randn(B, g.latent_size)
        fake = gan(z, cond=conds[0] if cond else None)
        total_d = 0.0
        for j in range(N):                               # trainer.py:228-243
            l = gan.discrim_step(real=xs, fake=[f.detach() for f in fake], cond=conds, loss=losses.discrim_loss, gp_lambda=gp)
            if mean_d:
                l /= N
            l.backward(retain_graph=j != N - 1)
            if it in (0, 2) and j == N - 1:
                pack_norms(tag + ('_D_gn' if it else '_D_gn0'), grad_norms(d), out)
            optD.step()
            total_d += float(l)
        _, _, real_pred = gan.all_discrim_forward(real=xs, cond=conds, fake=None, loss=None)
        total_g = 0.0
        for j in range(M):                               # trainer.py:249-263
            if j != 0:
                fake = gan(z, cond=conds[0] if cond else None)
            l = _gen_step(gan, fake, real_pred, conds, losses)
            if mean_g:
                l /= M
            l.backward(retain_graph=j != M - 1)
            if it in (0, 2) and j == M - 1:
                pack_norms(tag + ('_G_gn' if it else '_G_gn0'), grad_norms(g), out)
            optG.step()
            total_g += float(l)
        lD_all.append(total_d)
        lG_all.append(total_g)
        print('case', tag, 'it', it, total_d, total_g)
    out[tag + '_lossD'] = np.array(lD_all, dtype=np.float64)
    out[tag + '_lossG'] = np.array(lG_all, dtype=np.float64)
    for m, mod in (('G', g), ('D', d)):
        pack_norms(tag + '_%s_dp' % m, {k: float((p.detach() - init[m][k]).norm()) for k, p in mod.named_parameters()}, out)
    out[tag + '_steps'] = np.array([int(next(iter(optD.state.values()))['step']), int(next(iter(optG.state.values()))['step'])])
    out[tag + '_nbt'] = np.array([int(v) for k, v in g.state_dict().items() if k.endswith('num_batches_tracked')])


def golden_steps_schedule():
    out = {}
    for tag, kw in CASES.items():
        golden_case(tag, out=out, **kw)
    save('steps_schedule', **out)


if __name__ == '__main__':
    golden_steps_schedule()
