"""CPU restatement of the adaptive strength of the discriminator's augmentation (--D_aug_p / --D_ada; ADA, Karras et al. 2020, not
in the reference) in plain torch / numpy, and the oracle loop of diffaug_cases with that restatement at the call sites
and draw positions of the trainer. Shared by test_ada_cpu.py and test_ada_gpu.py. No reference exists to record a fixture from,
so this composition is the yardstick (as with --D_aug itself).

The definition is the one in txt2vid_amd/functional_aug.py, restated:

  Gating. Every parameter block u [B, 8] is followed by a gate block g [B, 8] of uniforms in [0, 1) from the same generator.
  Clip j of a member reads gate row j * stride (the row of its parameters). Columns 0, 1, 2 gate color, translation, cutout:
  effective policy = policy & (1 [g0 < p] | 2 [g1 < p] | 4 [g2 < p]), a strict fp32 <. The clip then goes through
  diffaug_cases.augment with that policy; policy 0 is the clip itself.

  Statistic. r_t = mean over levels l and pairs j of sgn(u_r[l][j] - u_f[l][j]), sgn(0) = 0, on the unconditional logits.

  Controller. ada float32[8] = {p, sum of signs, pairs, D steps, 0...}. Per D step: add the step's sign sum and pair count,
  increment ada[3]; when ada[3] >= interval: p <- clamp(p + sgn(ada[1] / ada[2] - target) * step, 0, 1) in float32 (one add, two
  clamps), ada[1..3] <- 0. step = B * interval / (1000 * kclips) in double, rounded once to float32.

Draw order per iteration: diffaug_cases' with every block u followed at once by its gate block g."""
import numpy as np
import torch

import diffaug_cases as DA
import schedule_cases as S
from oracle import tganv2_oracle as O
from txt2vid_amd import functional_aug as A

F32 = np.float32


def effective_policies(g, p, policy, n, stride=1):
    """The effective policy bits of clips 0..n-1 of a member: clip j reads row j * stride of the gate block g [B, K] (fp32)."""
    bits = A.parse_policy(policy) if isinstance(policy, str) else int(policy)
    gn = g.detach().cpu().numpy().astype(F32)
    pv = F32(p)
    out = []
    for j in range(n):
        row = gn[j * stride]
        mask = (1 if row[0] < pv else 0) | (2 if row[1] < pv else 0) | (4 if row[2] < pv else 0)
        out.append(bits & mask)
    return out


def augment(x, u, g, p, policy, stride=1):
    """The gated T(x) for clips x [N, C, T, S, S]: clip j through diffaug_cases.augment with its own effective policy (row
    j * stride of u and of g); an effective policy of 0 returns the clip itself."""
    N = x.shape[0]
    assert (N - 1) * stride < u.shape[0] and g.shape == u.shape
    out = []
    for j, bits in enumerate(effective_policies(g, p, policy, N, stride)):
        xj = x[j:j + 1]
        out.append(xj if bits == 0 else DA.augment(xj, u[j * stride:j * stride + 1], bits, 1))
    return torch.cat(out)


def augment_pyramid(xs, u, g, p, policy, subsample_input=True):
    return [augment(x, u, g, p, policy, 2 ** l if subsample_input else 1) for l, x in enumerate(xs)]


def sign_sum(u_r, u_f):
    """(sum of sgn(u_r - u_f), number of pairs) over the levels; a tie counts 0."""
    s = n = 0
    for r, f in zip(u_r, u_f):
        r, f = np.asarray(r, dtype=F32).reshape(-1), np.asarray(f, dtype=F32).reshape(-1)
        assert r.shape == f.shape
        s += int((r > f).sum()) - int((r < f).sum())
        n += r.size
    return s, n


def step_size(batch, interval, kclips):
    """B * interval / (1000 * kclips) in double, then one rounding to float32."""
    return F32(float(batch) * float(interval) / (1000.0 * float(kclips)))


def controller_init(p0):
    ada = np.zeros(8, dtype=F32)
    ada[0] = F32(p0)
    return ada


def controller_step(ada, s, n, target, step, interval):
    """One D step's sign sum `s` over `n` pairs into the state `ada` (float32[8], changed in place and returned). Every operation
    in numpy float32, in the order of the definition."""
    assert ada.dtype == F32
    target, step = F32(target), F32(step)
    ada[1] = F32(ada[1] + F32(s))
    ada[2] = F32(ada[2] + F32(n))
    ada[3] = F32(ada[3] + F32(1))
    if ada[3] >= F32(interval):
        rt = F32(ada[1] / ada[2])
        sgn = F32(1) if rt > target else (F32(-1) if rt < target else F32(0))
        p = F32(ada[0] + F32(sgn * step))
        p = F32(0) if p < F32(0) else p
        p = F32(1) if p > F32(1) else p
        ada[0] = p
        ada[1:4] = F32(0)
    return ada


def oracle_loop(cond, N, M, policy=DA.FULL, tokens=None, iters=3, seed=100, p0=0.5, target=0.6, interval=1, kclips=0.016):
    """diffaug_cases.oracle_loop (RSGAN, GP 0.5, no loss means) with gated augmentation and the controller where the trainer has
    them. Returns the per-iteration totals of lossD and lossG, 'p': p after every D step (N per iteration), 'ada': the state's
    first four entries after every D step, 'rt': the statistic r_t of every update (None where the window was not full),
    and 'steps': per D step (min |u_r - u_f| over its pairs, max |logit| over the same) for the test's precondition."""
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
    step = step_size(B, interval, kclips)
    ada = controller_init(p0)
    res = {'lossD': [], 'lossG': [], 'p': [], 'ada': [], 'rt': [], 'steps': []}

    def blocks():
        u = torch.rand(B, A.K)
        return u, torch.rand(B, A.K)                   # the gate block right behind its parameter block
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
            p = float(ada[0])
            u, g = blocks()
            xs_a = augment_pyramid(xs, u, g, p, policy)
            u, g = blocks()
            fk_a = augment_pyramid([f.detach() for f in fake], u, g, p, policy)
            fake_conds = None
            if conds is not None:
                fc0 = conds[0][O.gen_perm(B)]
                fake_conds = [fc0[0:cc.size(0)] for cc in conds]
            l = O.discrim_loss(PD, pre, xs_a, fk_a, conds, fake_conds, 0.5)          # draws this step's alphas
            with torch.no_grad():                      # the unconditional logits of the lu term (the same forward, recomputed)
                u_r = [r[0].numpy() for r in O.multiscale_discrim(PD, xs_a, conds, pre)]
                u_f = [f[0].numpy() for f in O.multiscale_discrim(PD, fk_a, conds, pre)]
            res['steps'].append((min(float(np.abs(r.astype(np.float64) - f.astype(np.float64)).min()) for r, f in zip(u_r, u_f)),
                                 max(float(np.abs(t).max()) for t in u_r + u_f)))
            s, n = sign_sum(u_r, u_f)
            full = ada[3] + 1 >= interval
            res['rt'].append((float(ada[1]) + s) / (float(ada[2]) + n) if full else None)
            controller_step(ada, s, n, target, step, interval)
            res['p'].append(float(ada[0]))
            res['ada'].append(ada[:4].copy())
            l.backward()
            optD.step()
            tD += float(l.detach())
        p = float(ada[0])
        u, g = blocks()
        xs_g = augment_pyramid(xs, u, g, p, policy)
        u_f, g_f = blocks()
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
                u_f, g_f = blocks()
            for k in g_keys:
                PG[k].grad = None
            l = O.gen_loss(PD, pre, augment_pyramid(fake, u_f, g_f, p, policy), real_pred, conds)
            l.backward()
            optG.step()
            tG += float(l.detach())
        res['lossD'].append(tD)
        res['lossG'].append(tG)
    return res


def consume(draws, B, L, n_levels, n_gen, N, M, gp, ca_dim, gated):
    """diffaug_cases.consume with augmentation on: the draw methods in the order one eager iteration calls them; a gated draw
    contributes u and then g."""
    bs = [B]
    for _ in range(n_levels - 1):
        bs.append((bs[-1] + 1) // 2)
    out = []

    def val(t):
        out.append(t.clone() if torch.is_tensor(t) else t)

    def phase():
        host, dev = draws.phase()
        val(int(dev) if dev is not None else host)

    def aug():
        if gated:
            u, g = draws.aug(B, 'cpu', gated=True)
            val(u)
            val(g)
        else:
            val(draws.aug(B, 'cpu'))
    for host, dev in draws.multiscale_t0(n_levels):
        val(int(dev) if dev is not None else host)
    val(draws.z(B, L, 'cpu'))
    if ca_dim:
        val(draws.ca_eps(B, ca_dim, 'cpu'))
    for _ in range(n_gen):
        phase()
    for _ in range(N):
        aug()
        aug()
        if gp:
            for b in bs:
                val(draws.alpha(b, 5, 'cpu'))
    aug()
    aug()
    for _ in range(1, M):
        if ca_dim:
            val(draws.ca_eps(B, ca_dim, 'cpu'))
        for _ in range(n_gen):
            phase()
        aug()
    return out
