"""CPU restatement of the LeCam regularisation of the discriminator (--D_lecam; Tseng et al. 2021, not in the reference; DESIGN
§23) in float64 numpy, and the oracle loop of diffaug_cases with the term at the trainer's call site. Shared by test_lecam_cpu.py
and test_lecam_gpu.py. No reference exists to record a fixture from, so this composition is the yardstick (as with --D_ada).

The definition is the one in txt2vid_amd/gan/lecam.py, restated:

  State. lecam float32[20] = {n, R_last, gate_last, L, alpha_R[0..7], alpha_F[0..7]}.

  One D step on the unconditional logits u_r[l], u_f[l] (one vector per pyramid level l < L), with n and the anchors as they
  stood before the step:
    1. gate = 1 if n >= max(start, 1) else 0
    2. R = 1/L sum_l [ mean_i (u_r[l][i] - alpha_F[l])^2 + mean_i (u_f[l][i] - alpha_R[l])^2 ]
    3. the D loss gains lambda * gate * R; R_last = R (ungated), gate_last = gate
    4. the anchors are constants: dR/du_r[l][i] = gate * g * 2 (u_r[l][i] - alpha_F[l]) / (L * b_l), u_f likewise against alpha_R
    5. alpha_R[l] = mean u_r[l], alpha_F[l] = mean u_f[l] if n == 0, else alpha <- decay * alpha + (1 - decay) * mean; n <- n + 1
  `decay` is the float32 the launch receives."""
import numpy as np
import torch

import diffaug_cases as DA
import schedule_cases as S
from oracle import tganv2_oracle as O
from txt2vid_amd import functional_aug as A

F32, F64 = np.float32, np.float64
N_STATE, A_R, A_F = 20, 4, 12


def init_state():
    return np.zeros(N_STATE, dtype=F32)


def _flat(ts):
    return [np.asarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t, dtype=F64).reshape(-1) for t in ts]


def step(state, u_r, u_f, decay, start):
    """Steps 1-5 in float64 from the float32 state `state` (left unchanged) and one D step's logits. Returns (gate * R, the new
    state as float64[20], unrounded)."""
    assert state.dtype == F32 and state.shape == (N_STATE,)
    u_r, u_f = _flat(u_r), _flat(u_f)
    L = len(u_r)
    assert L == len(u_f) and 1 <= L <= 8 and all(r.size == f.size >= 1 for r, f in zip(u_r, u_f))
    s = state.astype(F64)
    n, d = s[0], F64(F32(decay))
    gate = 1.0 if n >= max(int(start), 1) else 0.0
    R = sum(np.mean((r - s[A_F + l]) ** 2) + np.mean((f - s[A_R + l]) ** 2) for l, (r, f) in enumerate(zip(u_r, u_f))) / L
    new = s.copy()
    for l, (r, f) in enumerate(zip(u_r, u_f)):
        mr, mf = np.mean(r), np.mean(f)
        new[A_R + l] = mr if n == 0 else d * s[A_R + l] + (1.0 - d) * mr
        new[A_F + l] = mf if n == 0 else d * s[A_F + l] + (1.0 - d) * mf
    new[0], new[1], new[2], new[3] = n + 1, R, gate, L
    return gate * R, new


def grads(state, u_r, u_f, start, g=1.0):
    """Step 4 in float64 with the anchors of the float32 state `state` as it stood BEFORE the step: ([dR/du_r[l]], [dR/du_f[l]])."""
    u_r, u_f = _flat(u_r), _flat(u_f)
    L = len(u_r)
    s = state.astype(F64)
    gate = 1.0 if s[0] >= max(int(start), 1) else 0.0
    return ([gate * g * 2.0 * (r - s[A_F + l]) / (L * r.size) for l, r in enumerate(u_r)],
            [gate * g * 2.0 * (f - s[A_R + l]) / (L * f.size) for l, f in enumerate(u_f)])


def oracle_loop(cond, N, M, policy=DA.FULL, tokens=None, iters=3, seed=100, lam=0.3, decay=0.5, start=0, dtype=torch.float32):
    """diffaug_cases.oracle_loop (RSGAN, GP 0.5, no loss means, the full augmentation policy of test_diffaug_gpu.make) with
    lam * gate * R added to every D loss. R is formed in torch from a with-grad `O.multiscale_discrim` forward on the step's
    inputs, the anchors entering as constants; the state is kept in float32 and moved by `step`. Returns the per-iteration totals
    of lossD and lossG, 'state': the float32 state after every D step (N per iteration), 'scale': max |logit| of every D step, and
    'share': lam * gate * R / |that step's D loss| of every D step. `dtype=torch.float64` runs the same loop in double on the same
    float32 weights and draws (the oracle's own rounding error is the gap between the two runs)."""
    import random
    case = dict(cond=cond, loss='rsgan', gp=0.5, N=N, M=M, mean_d=False, mean_g=False)
    PG, PD, PT, pre = S.oracle_states(case)
    for P in (PG, PD):                                 # (the text encoder stays float32: its sentence code is an input here)
        for k in list(P):
            if P[k].dtype.is_floating_point:
                P[k] = P[k].to(dtype)
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
    state = init_state()
    res = {'lossD': [], 'lossG': [], 'state': [], 'scale': [], 'share': []}
    for it in range(iters):
        x = S.batch().to(dtype)
        c = None
        if cond:
            with torch.no_grad():
                c = O.text_encode(PT, tokens, [8] * B).to(dtype)
        xs, conds, _ = O.multiscale_data(x, c, S.FS)
        z = torch.randn(B, 256).to(dtype)
        fake = O.multiscale_gen(PG, z, conds[0] if conds else None, training=True)
        tD = 0.0
        for j in range(N):
            for k in d_keys:
                PD[k].grad = None
            xs_a = DA.augment_pyramid(xs, torch.rand(B, A.K).to(dtype), policy)
            fk_a = DA.augment_pyramid([f.detach() for f in fake], torch.rand(B, A.K).to(dtype), policy)
            fake_conds = None
            if conds is not None:
                fc0 = conds[0][O.gen_perm(B)]
                fake_conds = [fc0[0:cc.size(0)] for cc in conds]
            l = O.discrim_loss(PD, pre, xs_a, fk_a, conds, fake_conds, 0.5)          # draws this step's alphas
            # the unconditional logits of the lu term, with their graph (the same forward, recomputed; it draws nothing)
            u_r = [r[0] for r in O.multiscale_discrim(PD, xs_a, conds, pre)]
            u_f = [f[0] for f in O.multiscale_discrim(PD, fk_a, conds, pre)]
            L = len(u_r)
            gate = 1.0 if state[0] >= max(int(start), 1) else 0.0
            R = sum(((r - float(state[A_F + i])) ** 2).mean() + ((f - float(state[A_R + i])) ** 2).mean()
                    for i, (r, f) in enumerate(zip(u_r, u_f))) / L
            _, new = step(state, u_r, u_f, decay, start)
            res['scale'].append(max(float(t.detach().abs().max()) for t in u_r + u_f))
            res['share'].append(lam * gate * float(R.detach()) / abs(float(l.detach()) + lam * gate * float(R.detach())))
            l = l + lam * gate * R
            state = new.astype(F32)
            res['state'].append(state.copy())
            l.backward()
            optD.step()
            tD += float(l.detach())
        xs_g = DA.augment_pyramid(xs, torch.rand(B, A.K).to(dtype), policy)
        u_fk = torch.rand(B, A.K).to(dtype)
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
                u_fk = torch.rand(B, A.K).to(dtype)
            for k in g_keys:
                PG[k].grad = None
            l = O.gen_loss(PD, pre, DA.augment_pyramid(fake, u_fk, policy), real_pred, conds)
            l.backward()
            optG.step()
            tG += float(l.detach())
        res['lossD'].append(tD)
        res['lossG'].append(tG)
    return res
