"""CPU restatement of the generator's conditioning augmentation (CA; StackGAN++, not in the reference) composed with the oracle's
functional pieces (oracle/tganv2_oracle.py) — shared by test_ca_cpu.py and test_ca_gpu.py. No reference exists to record a fixture
from, so these compositions are the yardstick:

    h = Linear(s; ca.fc) [B, 4D];  x = h[:, :2D] * sigmoid(h[:, 2D:]);  mu, logvar = x[:, :D], x[:, D:]
    c = mu + eps * exp(logvar / 2);  KL = mean(-0.5 * (1 + logvar - mu^2 - exp(logvar)))
    G input cat(z, c); each G step's loss: adversarial + kl_coeff * KL

Draw order on the host generator: z, then per generator forward eps [B, D] first and that forward's Subsample phases after it."""
import numpy as np
import torch
import torch.nn.functional as F

import schedule_cases as S
from oracle import tganv2_oracle as O


def ca_ref(h, eps):
    D = h.shape[1] // 4
    x = h[:, :2 * D] * torch.sigmoid(h[:, 2 * D:])
    mu, lv = x[:, :D], x[:, D:]
    c = mu + eps * torch.exp(0.5 * lv)
    kl = (-0.5 * (1 + lv - mu * mu - torch.exp(lv))).mean()
    return c, kl


def gen_state(D, cond_dim=256, num_channels=1, width=64, height=64):
    """Recipe weights of MultiScaleGen(cond_dim, ca_dim=D): the oracle's generator keys with fc.weight [fm, latent + D], plus
    ca.fc.* (the same values `recipe_tensor` gives the module's keys)."""
    PG = O.recipe_state(O.gen_shapes(num_channels=num_channels, width=width, height=height, cond_dim=D, cond_variant=True))
    PG['ca.fc.weight'] = O.recipe_tensor('ca.fc.weight', (4 * D, cond_dim))
    PG['ca.fc.bias'] = O.recipe_tensor('ca.fc.bias', (4 * D,))
    return PG


def gen_ca(PG, z, s, training=True, eps=None, bts=None):
    """CA + `oracle.multiscale_gen`. eps is drawn here (before the generator's phases) unless given. Returns (rendered, KL)."""
    h = F.linear(s, PG['ca.fc.weight'], PG['ca.fc.bias'])
    if eps is None:
        eps = torch.randn(s.size(0), h.size(1) // 4)
    c, kl = ca_ref(h, eps)
    return O.multiscale_gen(PG, z, c, training=training, bts=bts), kl


def oracle_loop(N, M, D, tokens, iters=3, seed=100, kl_coeff=2.0):
    """The text-conditioned N:M loop of schedule_cases.oracle_loop (RSGAN, GP 0.5, no loss means) with CA on the generator input.
    Returns the per-iteration totals of lossD, lossG (with kl_coeff * KL) and KL."""
    import random
    _, PD, PT, pre = S.oracle_states(dict(cond=True))
    PG = gen_state(D)
    g_keys = [k for k, v in PG.items() if v.dtype.is_floating_point and 'running_' not in k]
    d_keys = [k for k, v in PD.items() if v.dtype.is_floating_point]
    for k in g_keys:
        PG[k].requires_grad_(True)
    for k in d_keys:
        PD[k].requires_grad_(True)
    optG = torch.optim.Adam([PG[k] for k in g_keys], lr=2e-4, betas=(0.5, 0.999))
    optD = torch.optim.Adam([PD[k] for k in d_keys], lr=2e-4, betas=(0.5, 0.999))
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    B = S.B
    res = {'lossD': [], 'lossG': [], 'KL': []}
    for it in range(iters):
        x = S.batch()
        with torch.no_grad():
            c = O.text_encode(PT, tokens, [8] * B)
        xs, conds, _ = O.multiscale_data(x, c, S.FS)
        z = torch.randn(B, 256)
        fake, kl = gen_ca(PG, z, conds[0])
        tD = 0.0
        for j in range(N):
            for k in d_keys:
                PD[k].grad = None
            fc0 = conds[0][O.gen_perm(B)]
            fake_conds = [fc0[0:cc.size(0)] for cc in conds]
            l = O.discrim_loss(PD, pre, xs, [f.detach() for f in fake], conds, fake_conds, 0.5)
            l.backward()
            optD.step()
            tD += float(l.detach())
        with torch.no_grad():
            O.gen_perm(B)                               # all_discrim_forward draws a permutation it never uses
            real_pred = O.multiscale_discrim(PD, xs, conds, pre)
        tG = tK = 0.0
        for j in range(M):
            if j:
                fake, kl = gen_ca(PG, z, conds[0])
            for k in g_keys:
                PG[k].grad = None
            l = O.gen_loss(PD, pre, fake, real_pred, conds) + kl_coeff * kl
            l.backward()
            optG.step()
            tG += float(l.detach())
            tK += float(kl.detach())
        res['lossD'].append(tD)
        res['lossG'].append(tG)
        res['KL'].append(tK)
    return res


def host_draw_sequence(B, L, D, n_levels, n_gen, N, M, n_perms):
    """Every host draw of one CA iteration in the documented order (torch: level phases, z, eps 0, G phases 0, the GP alphas of the
    N D steps, then eps j and G phases j per later G forward; numpy: the caption permutations)."""
    from txt2vid_amd.util.misc import gen_perm
    bs = [B]
    for _ in range(n_levels - 1):
        bs.append((bs[-1] + 1) // 2)
    t0s, t0, st = [], 0, 1
    for _ in range(n_levels):
        t0s.append(t0)
        bt = int(torch.randint(2, (1,)))
        t0, st = t0 + bt * st, st * 2
    z = torch.randn(B, L)
    eps = [torch.randn(B, D)]
    phases = [int(torch.randint(2, (1,))) for _ in range(n_gen)]
    alphas = [torch.rand(b, 1, 1, 1, 1).reshape(b) for _ in range(N) for b in bs]
    for _ in range(M - 1):
        eps.append(torch.randn(B, D))
        phases += [int(torch.randint(2, (1,))) for _ in range(n_gen)]
    perms = [gen_perm(B) for _ in range(n_perms)]
    return dict(bs=bs, t0s=t0s, z=z, eps=eps, phases=phases, alphas=alphas, perms=perms)
