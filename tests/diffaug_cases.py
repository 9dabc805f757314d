"""CPU restatement of the differentiable augmentation of the discriminator's inputs (--D_aug; DiffAugment, not in the reference)
in plain torch — index arithmetic and masks, any float dtype, autograd for the adjoint — and the oracle loop of schedule_cases
with that restatement at the call sites and draw positions of the trainer. Shared by test_diffaug_cpu.py and test_diffaug_gpu.py.
No reference exists to record a fixture from, so this composition is the yardstick (as with conditioning augmentation).

The definition is the one in txt2vid_amd/functional_aug.py; its integer parameters come from `aug_params` (one definition), the
transformation itself is restated here step by step, literally: brightness, then saturation, then contrast with the clip mean
taken AFTER the first two, then the shift, then the cutout.

Draw order on the host generator per iteration: ... z, G forward 0's draws; per D step a real block, a generated block, then
that step's GP alphas; at G part 0 a real and a generated block; per later G step that forward's draws, then a generated block."""
import numpy as np
import torch

import schedule_cases as S
from oracle import tganv2_oracle as O
from txt2vid_amd import functional_aug as A

FULL = 'color,translation,cutout'
SUBSETS = ['color', 'translation', 'cutout', 'color,translation', 'color,cutout', 'translation,cutout', FULL]


def augment(x, u, policy, stride=1):
    """T(x) for clips x [N, C, T, S, S] (float32 or float64); clip j uses row j * stride of the block u [B, K] (fp32)."""
    bits = A.parse_policy(policy) if isinstance(policy, str) else int(policy)
    N, C, T, Sd, W = x.shape
    assert Sd == W and (N - 1) * stride < u.shape[0]
    P = A.aug_params(u, Sd)
    rows = torch.arange(N) * stride
    y = x
    if bits & A.COLOR:
        def col(k):
            return P[k][rows].to(x.dtype).view(N, 1, 1, 1, 1)
        y = y + col('b')
        m = y.mean(dim=1, keepdim=True)
        y = (y - m) * col('s') + m
        mu = y.mean(dim=(1, 2, 3, 4), keepdim=True)
        y = (y - mu) * col('c') + mu
    if bits & (A.TRANSLATION | A.CUTOUT):
        idx = torch.arange(Sd)
        out = []
        for j in range(N):
            r = int(rows[j])
            yj = y[j]
            if bits & A.TRANSLATION:
                tx, ty = int(P['tx'][r]), int(P['ty'][r])
                sh, sw = idx - ty, idx - tx                                  # out(h, w) reads (h - ty, w - tx)
                ok = ((sh >= 0) & (sh < Sd))[:, None] & ((sw >= 0) & (sw < Sd))[None, :]
                yj = yj[:, :, sh.clamp(0, Sd - 1)][:, :, :, sw.clamp(0, Sd - 1)]
                yj = torch.where(ok, yj, torch.zeros((), dtype=x.dtype))
            if bits & A.CUTOUT:
                x0, y0, size = int(P['x0'][r]), int(P['y0'][r]), P['size']
                cut = ((idx >= y0) & (idx < y0 + size))[:, None] & ((idx >= x0) & (idx < x0 + size))[None, :]
                yj = torch.where(cut, torch.zeros((), dtype=x.dtype), yj)
            out.append(yj)
        y = torch.stack(out)
    return y


def augment_pyramid(xs, u, policy, subsample_input=True):
    return [augment(x, u, policy, 2 ** l if subsample_input else 1) for l, x in enumerate(xs)]


def oracle_loop(cond, N, M, policy=FULL, tokens=None, iters=3, seed=100):
    """schedule_cases.oracle_loop (RSGAN, GP 0.5, no loss means) with the augmentation where the trainer applies it. Returns the
    per-iteration totals of lossD and lossG."""
    import random
    case = dict(cond=cond, loss='rsgan', gp=0.5, N=N, M=M, mean_d=False, mean_g=False)
    PG, PD, PT, pre = S.oracle_states(case)
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
    res = {'lossD': [], 'lossG': []}
    for it in range(iters):
        x = S.batch()
        c = None
        if cond:
            with torch.no_grad():
                c = O.text_encode(PT, tokens, [8] * B)
        xs, conds, _ = O.multiscale_data(x, c, S.FS)
        z = torch.randn(B, 256)
        fake = O.multiscale_gen(PG, z, conds[0] if conds else None, training=True)
        tD = 0.0
        for j in range(N):
            for k in d_keys:
                PD[k].grad = None
            xs_a = augment_pyramid(xs, torch.rand(B, A.K), policy)
            fk_a = augment_pyramid([f.detach() for f in fake], torch.rand(B, A.K), policy)
            fake_conds = None
            if conds is not None:
                fc0 = conds[0][O.gen_perm(B)]
                fake_conds = [fc0[0:cc.size(0)] for cc in conds]
            l = O.discrim_loss(PD, pre, xs_a, fk_a, conds, fake_conds, 0.5)          # draws this step's alphas
            l.backward()
            optD.step()
            tD += float(l.detach())
        xs_g = augment_pyramid(xs, torch.rand(B, A.K), policy)
        u_f = torch.rand(B, A.K)
        with torch.no_grad():
            if conds is not None:
                O.gen_perm(B)                          # all_discrim_forward draws a permutation it never uses
                real_pred = O.multiscale_discrim(PD, xs_g, conds, pre)
            else:
                real_pred = [r[0] for r in O.multiscale_discrim(PD, xs_g, None, pre)]
        tG = 0.0
        for j in range(M):
            if j:
                fake = O.multiscale_gen(PG, z, conds[0] if conds else None, training=True)
                u_f = torch.rand(B, A.K)
            for k in g_keys:
                PG[k].grad = None
            l = O.gen_loss(PD, pre, augment_pyramid(fake, u_f, policy), real_pred, conds)
            l.backward()
            optG.step()
            tG += float(l.detach())
        res['lossD'].append(tD)
        res['lossG'].append(tG)
    return res


def consume(draws, B, L, n_levels, n_gen, N, M, gp, ca_dim, n_perms, aug):
    """Call the draw methods in the order one eager iteration consumes them and return every value (host tensors / ints)."""
    bs = [B]
    for _ in range(n_levels - 1):
        bs.append((bs[-1] + 1) // 2)
    out = []

    def val(t):
        out.append(t.clone() if torch.is_tensor(t) else t)

    def phase():
        host, dev = draws.phase()
        val(int(dev) if dev is not None else host)

    def t0s():
        for host, dev in draws.multiscale_t0(n_levels):
            val(int(dev) if dev is not None else host)
    t0s()
    val(draws.z(B, L, 'cpu'))
    if ca_dim:
        val(draws.ca_eps(B, ca_dim, 'cpu'))
    for _ in range(n_gen):
        phase()
    for _ in range(N):
        if aug:
            val(draws.aug(B, 'cpu'))
            val(draws.aug(B, 'cpu'))
        if gp:
            for b in bs:
                val(draws.alpha(b, 5, 'cpu'))
    if aug:
        val(draws.aug(B, 'cpu'))
        val(draws.aug(B, 'cpu'))
    for _ in range(1, M):
        if ca_dim:
            val(draws.ca_eps(B, ca_dim, 'cpu'))
        for _ in range(n_gen):
            phase()
        if aug:
            val(draws.aug(B, 'cpu'))
    return out
