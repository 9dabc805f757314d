"""The --discrim_steps N / --gen_steps M cases of tests/golden/steps_schedule.npz (make_golden_steps.py) and their N:M loop
composed from the oracle's functional pieces (oracle/tganv2_oracle.py) on the CPU — shared by test_schedule_cpu.py (the
composition reproduces the fixture) and test_schedule_gpu.py (the HIP loop against both)."""
import numpy as np
import torch

from oracle import tganv2_oracle as O

# mean_d / mean_g: the loss of every step divided by N / M (the reference's --no_mean_*_loss flag PASSED: store_false -> False)
CASES = {
    'a': dict(cond=False, loss='rsgan', gp=0.5, N=2, M=2, mean_d=True, mean_g=True),
    'b': dict(cond=False, loss='wasserstein', gp=10.0, N=3, M=1, mean_d=False, mean_g=False),
    'c': dict(cond=True, loss='rsgan', gp=0.5, N=2, M=1, mean_d=False, mean_g=False),
}
B, V, FS = 4, 21, [8, 16, 32, 64]


def params_for(case):
    class Prm(object):
        frame_sizes = list(FS)
        subsample_input = True
        discrim_steps = case['N']
        gen_steps = case['M']
        gp_lambda = case['gp']
        no_mean_discrim_loss = not case['mean_d']
        no_mean_gen_loss = not case['mean_g']
    return Prm()


def batch():
    """One iteration's real clips [B,C,T,H,W], drawn from the global CPU generator like the fixture."""
    return (torch.rand(B, 16, 1, 64, 64) * 2 - 1).permute(0, 2, 1, 3, 4).contiguous()


def _d_loss(case, PD, pre, xs, fake, conds, fake_conds):
    if case['loss'] == 'rsgan':
        return O.discrim_loss(PD, pre, xs, fake, conds, fake_conds, case['gp'])
    # Wasserstein (unconditional): the zoo loss per level, mean over levels, + gp_lambda * sum of the per-level GPs
    rp = [r[0] for r in O.multiscale_discrim(PD, xs, None, pre)]
    fp = [f[0] for f in O.multiscale_discrim(PD, fake, None, pre)]
    l = torch.stack([O.zoo_loss('wasserstein', 0, f, r) for f, r in zip(fp, rp)]).mean()
    return l + case['gp'] * torch.stack([O.gp_level(PD, pre, xs[i], fake[i]) for i in range(len(xs))]).sum()


def _g_loss(case, PD, pre, fake, real_pred, conds):
    if case['loss'] == 'rsgan':
        return O.gen_loss(PD, pre, fake, real_pred, conds)
    fk = O.multiscale_discrim(PD, fake, None, pre)
    return torch.stack([O.zoo_loss('wasserstein', 1, ff[0], rr) for ff, rr in zip(fk, real_pred)]).mean()


def oracle_states(case):
    cond = case['cond']
    PG = O.recipe_state(O.gen_shapes(num_channels=1, cond_dim=256 if cond else 0, cond_variant=cond))
    pre = 'single_discrim.module.' if cond else 'single_discrim.'
    PD = O.recipe_state(O.resnet3d_shapes(pre, 1, 64, 256 if cond else 0))
    PT = O.recipe_state(O.text_encoder_shapes(V)) if cond else None
    return PG, PD, PT, pre


def oracle_loop(case, tokens=None, iters=3, seed=100):
    """The reference's loop body (trainer.py:221-263) for `iters` iterations, seeded like the fixture. Returns the per-iteration
    totals, the gradient norms of the last D and last G backward of the first and the last iteration, the norms of (parameter - initial value)
    and the Adam step counts."""
    import random
    PG, PD, PT, pre = oracle_states(case)
    g_keys = [k for k, v in PG.items() if v.dtype.is_floating_point and 'running_' not in k]
    d_keys = [k for k, v in PD.items() if v.dtype.is_floating_point]
    init = {k: v.detach().clone() for k, v in list(PG.items()) + list(PD.items())}
    for k in g_keys:
        PG[k].requires_grad_(True)
    for k in d_keys:
        PD[k].requires_grad_(True)
    optG = torch.optim.Adam([PG[k] for k in g_keys], lr=2e-4, betas=(0.5, 0.999))
    optD = torch.optim.Adam([PD[k] for k in d_keys], lr=2e-4, betas=(0.5, 0.999))
    N, M = case['N'], case['M']
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    res = {'lossD': [], 'lossG': []}
    for it in range(iters):
        x = batch()
        c = None
        if case['cond']:
            with torch.no_grad():
                c = O.text_encode(PT, tokens, [8] * B)
        xs, conds, _ = O.multiscale_data(x, c, FS)
        z = torch.randn(B, 256)
        fake = O.multiscale_gen(PG, z, conds[0] if conds else None, training=True)
        tD = 0.0
        for j in range(N):
            for k in d_keys:
                PD[k].grad = None
            fake_conds = None
            if conds is not None:
                fc0 = conds[0][O.gen_perm(B)]
                fake_conds = [fc0[0:cc.size(0)] for cc in conds]
            l = _d_loss(case, PD, pre, xs, [f.detach() for f in fake], conds, fake_conds)
            if case['mean_d']:
                l = l / N
            l.backward()
            if it in (0, iters - 1) and j == N - 1:
                res['D_gn' if it else 'D_gn0'] = {k: float(PD[k].grad.norm()) for k in d_keys if PD[k].grad is not None}
            optD.step()
            tD += float(l.detach())
        with torch.no_grad():
            if conds is not None:
                O.gen_perm(B)                          # all_discrim_forward draws a permutation it never uses
                real_pred = O.multiscale_discrim(PD, xs, conds, pre)
            else:
                real_pred = [r[0] for r in O.multiscale_discrim(PD, xs, None, pre)]
        tG = 0.0
        for j in range(M):
            if j:
                fake = O.multiscale_gen(PG, z, conds[0] if conds else None, training=True)
            for k in g_keys:
                PG[k].grad = None
            l = _g_loss(case, PD, pre, fake, real_pred, conds)
            if case['mean_g']:
                l = l / M
            l.backward()
            if it in (0, iters - 1) and j == M - 1:
                res['G_gn' if it else 'G_gn0'] = {k: float(PG[k].grad.norm()) for k in g_keys if PG[k].grad is not None}
            optG.step()
            tG += float(l.detach())
        res['lossD'].append(tD)
        res['lossG'].append(tG)
    res['G_dp'] = {k: float((PG[k].detach() - init[k]).norm()) for k in g_keys}
    res['D_dp'] = {k: float((PD[k].detach() - init[k]).norm()) for k in d_keys}
    res['steps'] = (int(optD.state[PD[d_keys[0]]]['step']), int(optG.state[PG[g_keys[0]]]['step']))
    return res


def fixture_norms(g, key):
    return dict(zip([str(k) for k in g[key + '_keys']], [float(v) for v in g[key + '_vals']]))
