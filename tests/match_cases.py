"""CPU restatement of the contrastive clip-caption matching term (`Resnet3D(match=True)`, `--D_match` / `--G_match`; DESIGN §32;
XMC-GAN, Zhang et al. 2021; not in the reference) in plain torch, alone (the op cases) and composed with the oracle's functional
pieces (oracle/tganv2_oracle.py) — shared by test_match_cpu.py and test_match_gpu.py. No reference exists to record a fixture
from, so these compositions are the yardstick. With W = match.weight [K, J], per member f [b, K], s [b, J]:

    e = f W;  ê, ŝ = rows over max(norm, 1e-12);  S = ê ŝᵀ / τ;  M_ij = (i == j) or (row s_i and row s_j differ in a bit)
    term = (1/2b) Σ_i [ (max_i − S_ii) + log Σ_j M_ij exp(S_ij − max_i)  +  the same down column i ]        mean over members

A row of e with norm <= 1e-12 gets no gradient (`torch.where`; `F.normalize` would hand it a Jacobian of 10¹²·I).

Op fields, per case (members share W; per-member tensors are compared concatenated, C flattened): term; stats = (clip→caption
top-1 accuracy, caption→clip top-1 accuracy, entries M_ij = 0) of member 0, compared for EQUALITY; C = (P^r + P^c − 2I) / (2bτ);
gE, gf, gW = the gradients of G_UP · term with respect to e, f and W. Metric of tests/norm_cases.py (`ratio`), TOL for every
field. The restatement in fp32 against itself in float64, torch on the CPU, over every op case below, worst error / bound:
term 0.0010 (`pyramid` τ 0.01 scaled), C 0.0071 (`real` τ 0.01), gE 0.0035, gf 0.0024 (both `odd` τ 0.1), gW 0.0028 (`odd` τ 0.01):
TOL = 1e-4 sits 35x or more above the restatement's own rounding (test_match_cpu prints the ratios and asserts a factor of 4).
Measured on an MI355X over the op cases, the autograd surface and the raw ABI on guarded buffers, worst error / bound: term
0.0007 (`odd` τ 0.1 dup), C 0.0074 and gE 0.0032 (`real` τ 0.01 zero, raw ABI), gf 0.0017 (`cap` τ 0.01), gW 0.0009 (`odd` τ 0.01).

The counts are exact because the inputs plant structure: f = (a_i ŝ_t(i) + NOISE · n_i) W⁺ with t(i) = i except for a few rows
planted on another caption, so every row's and column's top-1 margin in S of member 0 (the member the counts are taken from) is
wide; test_match_cpu asserts that every such float64 margin exceeds 100 x the S-error bound `s_bound(tau)` of the case. The one
exception is stated there: a zero-norm row or column is an exact tie of zeros in every precision, and a tie is a miss."""
import functools

import torch

import norm_cases as NC
import schedule_cases as S
import proj_cases as PJ
import mbstd_cases as MB
from oracle import tganv2_oracle as O

EPS = 1e-12
TOL = 1e-4
G_UP = 0.7                              # dL/dterm handed to the backward: not 1, so that a dropped g shows
NOISE = 0.35
WRONG = 0.6                             # a row planted wrong points at the other caption less firmly than that caption's own row
FIELDS = ('term', 'C', 'gE', 'gf', 'gW')

# name -> (rows per member, K, J)
CASES = {
    'one': ([1], 1, 1),
    'pair': ([2], 8, 3),
    'odd': ([3], 70, 37),                           # K and J away from any tile or wave multiple
    'pyramid': ([4, 2, 1, 1], 128, 5),              # the ceil-halved pyramid of B = 4, 1-row members, J below a wave
    'real': ([33], 1024, 256),                      # the real widths, a row count that straddles a register tile
    'cap': ([128], 64, 300),                        # the row limit; J neither a wave multiple nor a chunk multiple
    'eight': ([5, 5, 3, 3, 2, 2, 1, 1], 192, 64),   # T2V_MAX_GROUPS members
}
# (case, tau, variant): every case at XMC-GAN's temperature; 1.0 and 0.01 (needs the maximum subtraction) where rows compete;
# features scaled by 10^3; two equal captions; all captions equal; a zero caption row and a zero feature row
VARIANTS = [(c, 0.1, 'plain') for c in CASES] + \
           [(c, t, 'plain') for c in ('pair', 'odd', 'pyramid', 'real', 'cap') for t in (1.0, 0.01)] + \
           [('real', 0.1, 'scaled'), ('pyramid', 0.01, 'scaled'), ('odd', 0.1, 'dup'), ('real', 0.1, 'dup'), ('eight', 0.1, 'dup'),
            ('odd', 0.1, 'same'), ('pyramid', 0.1, 'same'), ('odd', 0.1, 'zero'), ('real', 0.01, 'zero')]
IDS = ['%s-tau%g-%s' % v for v in VARIANTS]


def s_bound(tau):
    """The error in S the metric allows at this temperature: TOL (max(1, |S|max) + |S|) with |S| <= 1/tau."""
    return TOL * (max(1.0, 1.0 / tau) + 1.0 / tau)


def mask_of(s):
    """M [b, b] (bool) from the fp32 sentence codes: the diagonal, and every pair of rows that differ in a bit pattern."""
    bits = s.detach().to(torch.float32).contiguous().view(torch.int32)
    differ = (bits[:, None, :] != bits[None, :, :]).any(2)
    return differ | torch.eye(s.shape[0], dtype=torch.bool)


def unit_rows(x, grad=True):
    """x_i / max(‖x_i‖, 1e-12); a row at or below 1e-12 is a constant of differentiation."""
    n = x.norm(dim=1, keepdim=True)
    live = n > EPS
    safe = torch.where(live, n, torch.ones_like(n))
    return torch.where(live, x / safe, (x / EPS).detach()) if grad else x / n.clamp_min(EPS)


def scores(e, s, tau):
    return unit_rows(e) @ unit_rows(s.detach(), grad=False).t() / tau


def parts(e, s, tau, M=None):
    """(term 0-d, stats tuple, C [b, b], S) of one member, in the dtype of its arguments."""
    b = e.shape[0]
    M = mask_of(s) if M is None else M
    Sm = scores(e, s, tau)
    Sd = Sm.detach()
    diag = Sm.diagonal()
    eye = torch.eye(b, dtype=torch.bool)
    ninf = torch.full_like(Sd, float('-inf'))
    rmax, cmax = torch.where(M, Sd, ninf).max(1).values, torch.where(M, Sd, ninf).max(0).values
    zero = torch.zeros_like(Sm)
    er = torch.exp(torch.where(M, Sm - rmax[:, None], zero)) * M
    ec = torch.exp(torch.where(M, Sm - cmax[None, :], zero)) * M
    L = (rmax - diag) + torch.log(er.sum(1))
    Lc = (cmax - diag) + torch.log(ec.sum(0))
    term = (L.sum() + Lc.sum()) / (2 * b)
    off = torch.where(M & ~eye, Sd, ninf)
    hits_r, hits_c = (Sd.diagonal() > off.max(1).values), (Sd.diagonal() > off.max(0).values)
    stats = (float(hits_r.sum()) / b, float(hits_c.sum()) / b, float((~M).sum()))
    Pr, Pc = (er / er.sum(1, keepdim=True)).detach(), (ec / ec.sum(0, keepdim=True)).detach()
    C = (Pr + Pc - 2 * eye.to(Sd.dtype)) / (2 * b * tau)
    return term, stats, C, Sd


def margins(Sd, M):
    """Per row and per column of one member: S_ii minus the best unmasked competitor (+inf without one)."""
    eye = torch.eye(Sd.shape[0], dtype=torch.bool)
    off = torch.where(M & ~eye, Sd, torch.full_like(Sd, float('-inf')))
    return Sd.diagonal() - off.max(1).values, Sd.diagonal() - off.max(0).values


@functools.lru_cache(maxsize=None)
def inputs(case, variant='plain'):
    """fp32 CPU tensors of one case (seeded; shared by every test, never modified): W ~ N(0, 1/K); per member s ~ N(0, 1) and
    f = (a_i ŝ_t(i) + NOISE n_i) W⁺ (the pseudo-inverse: e = f W is that target, projected onto W's rows when K < J), t(i) = i
    and a_i = 1, except t(i) = i + 1 (mod b) and a_i = WRONG for the rows planted wrong (row 1 when b >= 3, and row b/2 when
    b >= 8)."""
    bs, K, J = CASES[case]
    g = torch.Generator()
    g.manual_seed(5200 + 29 * list(CASES).index(case))
    W = torch.randn(K, J, generator=g) * (1.0 / K) ** 0.5
    out = {'W': W, 'f': [], 's': [], 'M': []}
    for b in bs:
        s = torch.randn(b, J, generator=g)
        if variant == 'dup' and b >= 2:
            s[b - 1] = s[0]
        if variant == 'same':
            s[:] = s[0].clone()
        target = list(range(b))
        for w in ([1] if b >= 3 else []) + ([b // 2] if b >= 8 else []):
            target[w] = (w + 1) % b
        sh = s / s.norm(dim=1, keepdim=True)
        lead = torch.tensor([1.0 if target[i] == i else WRONG for i in range(b)]).view(b, 1)
        want = lead * sh[target] + NOISE * torch.randn(b, J, generator=g) / J ** 0.5
        f = (want.double() @ torch.linalg.pinv(W.double())).float()
        if variant == 'scaled':
            f = f * 1e3
        if variant == 'zero':
            s[b - 1] = 0.0
            f[b - 1] = 0.0
        out['f'].append(f.contiguous())
        out['s'].append(s.contiguous())
        out['M'].append(mask_of(s))
    return out


def reference(case, tau, variant='plain', dtype=torch.float64):
    """Every op field in `dtype` on the CPU, plus `stats` and the per-member S (`S`)."""
    inp = inputs(case, variant)
    W = inp['W'].to(dtype).clone().requires_grad_(True)
    fs = [t.to(dtype).clone().requires_grad_(True) for t in inp['f']]
    es = [f @ W for f in fs]
    for e in es:
        e.retain_grad()
    res = [parts(e, s.to(dtype), tau, M) for e, s, M in zip(es, inp['s'], inp['M'])]
    term = torch.stack([r[0] for r in res]).mean()
    (G_UP * term).backward()
    return {'term': term.detach(), 'stats': res[0][1], 'C': torch.cat([r[2].reshape(-1) for r in res]),
            'gE': torch.cat([e.grad for e in es], 0), 'gf': torch.cat([f.grad for f in fs], 0), 'gW': W.grad.detach(),
            'S': [r[3] for r in res]}


@functools.lru_cache(maxsize=None)
def case_reference(case, tau, variant='plain'):
    return reference(case, tau, variant)


def check(tag, got, ref, fields=FIELDS):
    """Prints every field's ratio to its bound (`match-ratio <tag> <field> <ratio>`), then asserts all of them."""
    rs = {f: NC.ratio(got[f], ref[f], TOL) for f in fields}
    for f in fields:
        print('match-ratio %s %s %.4g' % (tag, f, rs[f]))
    bad = {f: r for f, r in rs.items() if not r <= 1.0}
    assert not bad, '%s: error / bound %s' % (tag, bad)
    return rs


# ------------------------------------------------------------------------------------------------ composed with the oracle

PRE = PJ.PRE
_plain_multiscale_discrim = O.multiscale_discrim


def term_levels(feats, conds, W, tau):
    """The mean over the pyramid levels of the term of (feats[l] @ W, conds[l])."""
    return torch.stack([parts(f @ W, c, tau)[0] for f, c in zip(feats, conds)]).mean()


def patch(mp, box):
    """From here to the end of the monkeypatch (context), every call of `oracle.multiscale_discrim` — `discrim_loss` and
    `gen_loss` look the name up at call time — appends its result to `box`, so that the features the losses were computed from
    feed the matching term without a second trunk pass."""
    def recording(P, xs, conds=None, prefix='single_discrim.'):
        res = _plain_multiscale_discrim(P, xs, conds, prefix)
        box.append(res)
        return res
    mp.setattr(O, 'multiscale_discrim', recording)


def discrim_loss(box, PD, xs, fake, conds, fake_conds, gp, lam, tau):
    """`oracle.discrim_loss` + lam · the term of the real clips' features (the first trunk pass of the loss) with their captions."""
    del box[:]
    l = O.discrim_loss(PD, PRE, xs, fake, conds, fake_conds, gp)
    if lam is None:
        return l
    return l + lam * term_levels([r[2] for r in box[0]], conds, PD[PRE + 'match.weight'], tau)


def gen_loss(box, PD, fake, real_pred, conds, lam, tau):
    """`oracle.gen_loss` + lam · the term of the generated clips' features with their captions."""
    del box[:]
    l = O.gen_loss(PD, PRE, fake, real_pred, conds)
    if lam is None:
        return l
    return l + lam * term_levels([r[2] for r in box[0]], conds, PD[PRE + 'match.weight'], tau)


def discrim_state(proj=False, mbstd=False):
    """Recipe weights of the text-conditioned MultiScaleDiscrim(num_channels=1, cond_dim=256, match=True[, proj, mbstd]): the
    oracle's keys, then proj.weight, mbstd.weight, and match.weight = the recipe tensor, last."""
    if mbstd:
        PD, PT = MB.discrim_state(cond=True, proj=proj)
    elif proj:
        PD, PT = PJ.discrim_state()
    else:
        _, PD, PT, _ = S.oracle_states(dict(cond=True))
    PD[PRE + 'match.weight'] = O.recipe_tensor(PRE + 'match.weight', (1024, 256))
    return PD, PT


def oracle_loop(monkeypatch, tokens, iters=3, N=1, lam_d=1.0, lam_g=1.0, tau=0.1, proj=False, mbstd=False, seed=100):
    """The text-conditioned N:1 loop of schedule_cases.oracle_loop (RSGAN, GP 0.5, no loss means) with the matching term in
    both steps. Returns the per-iteration losses, the per-key D gradient norms of the first D step, and W after each D step."""
    import random
    import numpy as np
    PG, _, _, _ = S.oracle_states(dict(cond=True))
    PD, PT = discrim_state(proj, mbstd)
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
    res = {'lossD': [], 'lossG': [], 'W': []}
    box = []
    with monkeypatch.context() as mp:
        if mbstd:
            MB.patch(mp, MB.GROUP, proj)
        elif proj:
            PJ.patch(mp)
        patch(mp, box)
        for it in range(iters):
            x = S.batch()
            with torch.no_grad():
                c = O.text_encode(PT, tokens, [8] * B)
            xs, conds, _ = O.multiscale_data(x, c, S.FS)
            z = torch.randn(B, 256)
            fake = O.multiscale_gen(PG, z, conds[0], training=True)
            tD = 0.0
            for j in range(N):
                for k in d_keys:
                    PD[k].grad = None
                fc0 = conds[0][O.gen_perm(B)]
                l = discrim_loss(box, PD, xs, [f.detach() for f in fake], conds, [fc0[0:cc.size(0)] for cc in conds], 0.5, lam_d, tau)
                l.backward()
                if it == 0 and j == 0:
                    res['D_gn0'] = {k: float(PD[k].grad.norm()) for k in d_keys}
                optD.step()
                tD += float(l.detach())
                res['W'].append(PD[PRE + 'match.weight'].detach().clone())
            res['lossD'].append(tD)
            with torch.no_grad():
                O.gen_perm(B)                               # all_discrim_forward draws a permutation it never uses
                real_pred = O.multiscale_discrim(PD, xs, conds, PRE)
            for k in g_keys:
                PG[k].grad = None
            l = gen_loss(box, PD, fake, real_pred, conds, lam_g, tau)
            l.backward()
            optG.step()
            res['lossG'].append(float(l.detach()))
    return res
