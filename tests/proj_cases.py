"""CPU restatement of the discriminator's projection head (`Resnet3D(proj=True)`; DESIGN "Projection head"; Miyato & Koyama 2018;
not in the reference) in plain torch, alone (the op cases) and composed with the oracle's functional pieces
(oracle/tganv2_oracle.py) — shared by test_proj_cpu.py and test_proj_gpu.py. No reference exists to record a fixture from, so
these compositions are the yardstick:

    c = F.linear(cat(feat, s), fc.weight, fc.bias) + ((feat @ V) * s).sum(1, keepdim=True)         V = proj.weight [in_ch, cond_dim]

`oracle.multiscale_discrim` / `gp_level` look `resnet3d` up at call time: `patch` swaps that name (pytest monkeypatch) for
`resnet3d_proj`, which adds the term to the conditional logit of the unedited `oracle.resnet3d`; `discrim_loss`, `gen_loss` and
`OracleTrainer` then run with the projection.

Op fields, per case (members share V; per-member tensors are compared concatenated along the rows), with r a fixed weight per
row:  y;  gf, gs, gV, gbase = the gradients of Σ y·r;  df = ∂(Σy)/∂f (create_graph);  hf, hs, hV, hbase = the gradients of
Σ y·r + ½‖df‖². Metric of tests/norm_cases.py (`ratio`), tol 1e-4 for every field. The restatement in fp32 against itself in
float64, torch on the CPU, over every op case below, worst error / bound: y 0.0034 (`pyramid`), gf 0.0026, gs 0.0070, gV 0.0020,
df 0.0039, hf 0.0026, hs 0.0062, hV 0.0018 (all `real`), gbase and hbase 0 (they are r itself) — the bound sits 4x or more above
the restatement's own rounding (test_proj_cpu asserts it). Measured on an MI355X over the op cases, the raw ABI included: every
field below 0.003 of the bound (worst: y and gV on `real`, y on `eight`)."""
import functools

import torch
import torch.nn.functional as F

import norm_cases as NC
import schedule_cases as S
from oracle import tganv2_oracle as O

# name -> (rows per member, K, J)
CASES = {
    'one': ([1], 1, 1),
    'odd': ([3], 70, 37),                           # K and J away from any tile or wave multiple
    'pyramid': ([4, 2, 1, 1], 128, 5),              # the ceil-halved pyramid of B = 4, 1-row members, J below a wave
    'real': ([33], 1024, 256),                      # the real widths, a row count that straddles a wave
    'eight': ([5, 5, 3, 3, 2, 2, 1, 1], 192, 64),   # T2V_MAX_GROUPS members
}
TOL = 1e-4
FIRST = ('y', 'gf', 'gs', 'gV', 'gbase')
SECOND = ('df', 'hf', 'hs', 'hV', 'hbase')
FIELDS = FIRST + SECOND


def term(f, s, V):
    """Σ_kj f[b,k] V[k,j] s[b,j] as [b, 1], in the dtype of its arguments."""
    return ((f @ V) * s).sum(1, keepdim=True)


def head(feat, s, fc_w, fc_b, V=None):
    """The conditional head: the reference's (V None) or the projection discriminator's."""
    c = F.linear(torch.cat((feat, s), 1), fc_w, fc_b)
    return c if V is None else c + term(feat, s, V)


@functools.lru_cache(maxsize=None)
def inputs(case):
    """fp32 CPU tensors of one case (seeded; shared by every test, never modified): per member f ~ 2 N(0,1), s ~ U(-1,1),
    base ~ N(0,1), r ~ N(0,1); V ~ N(0, 2/(K+J))."""
    bs, K, J = CASES[case]
    g = torch.Generator()
    g.manual_seed(4000 + 13 * list(CASES).index(case))
    V = torch.randn(K, J, generator=g) * (2.0 / (K + J)) ** 0.5
    out = {'V': V, 'f': [], 's': [], 'base': [], 'r': []}
    for b in bs:
        out['f'].append(2 * torch.randn(b, K, generator=g))
        out['s'].append(2 * torch.rand(b, J, generator=g) - 1)
        out['base'].append(torch.randn(b, 1, generator=g))
        out['r'].append(torch.randn(b, 1, generator=g))
    return out


def fields_of(ys, fs, ss, V, bases, rs, second=True):
    """Every op field from the per-member outputs `ys` of any implementation (autograd does the rest)."""
    cat = lambda ts: torch.cat([t.detach() for t in ts], 0)
    out = {'y': cat(ys)}
    l1 = sum((y * r).sum() for y, r in zip(ys, rs))
    n = len(fs)
    g = torch.autograd.grad(l1, list(fs) + list(ss) + [V] + list(bases), retain_graph=second)
    out['gf'], out['gs'], out['gV'], out['gbase'] = cat(g[:n]), cat(g[n:2 * n]), g[2 * n].detach(), cat(g[2 * n + 1:])
    if second:
        dfs = torch.autograd.grad(sum(y.sum() for y in ys), list(fs), create_graph=True)
        out['df'] = cat(dfs)
        l2 = l1 + 0.5 * sum((d * d).sum() for d in dfs)
        h = torch.autograd.grad(l2, list(fs) + list(ss) + [V] + list(bases))
        out['hf'], out['hs'], out['hV'], out['hbase'] = cat(h[:n]), cat(h[n:2 * n]), h[2 * n].detach(), cat(h[2 * n + 1:])
    return out


def reference(case, dtype=torch.float64, V=None):
    """The op in `dtype` on the CPU. `V`: another weight in place of the case's (zeros)."""
    inp = inputs(case)
    leaf = lambda t: t.to(dtype).requires_grad_(True)
    fs, ss, bases = [leaf(t) for t in inp['f']], [leaf(t) for t in inp['s']], [leaf(t) for t in inp['base']]
    Vd = leaf(inp['V'] if V is None else V)
    ys = [b + term(f, s, Vd) for f, s, b in zip(fs, ss, bases)]
    return fields_of(ys, fs, ss, Vd, bases, [r.to(dtype) for r in inp['r']])


@functools.lru_cache(maxsize=None)
def case_reference(case):
    return reference(case)


def check(tag, got, ref, fields):
    """Prints every field's ratio to its bound (`proj-ratio <tag> <field> <ratio>`), then asserts all of them."""
    rs = {f: NC.ratio(got[f], ref[f], TOL) for f in fields}
    for f in fields:
        print('proj-ratio %s %s %.4g' % (tag, f, rs[f]))
    bad = {f: r for f, r in rs.items() if not r <= 1.0}
    assert not bad, '%s: error / bound %s' % (tag, bad)
    return rs


# ------------------------------------------------------------------------------------------------ composed with the oracle

_plain_resnet3d = O.resnet3d
PRE = 'single_discrim.module.'


def resnet3d_proj(P, x, cond=None, prefix='', **kw):
    """`oracle.resnet3d` with the projection term on the conditional logit: (u, c + term, feat)."""
    u, c, feat = _plain_resnet3d(P, x, cond, prefix=prefix, **kw)
    if c is not None:
        c = c + term(feat, cond, P[prefix + 'proj.weight'])
    return u, c, feat


def patch(mp):
    """From here to the end of the monkeypatch (context), every oracle function that calls `resnet3d` runs with the projection."""
    mp.setattr(O, 'resnet3d', resnet3d_proj)


V_SCALE = 1.0


def discrim_state(zero=False):
    """Recipe weights of the text-conditioned MultiScaleDiscrim(num_channels=1, cond_dim=256, proj=True): the oracle's keys and
    proj.weight — the recipe tensor (xavier scale) times V_SCALE, or zeros. On the recipe trunk (features of mean size 0.09 to
    0.37 per level, sentence codes of 0.03) V_SCALE = 1 gives a term of mean size 0.14 to 0.49 next to an existing head of 0.07
    to 0.47 (CPU, oracle): the module tests assert on their own features that the two are of comparable size."""
    _, PD, PT, pre = S.oracle_states(dict(cond=True))
    assert pre == PRE
    V = O.recipe_tensor(PRE + 'proj.weight', (1024, 256)) * V_SCALE
    PD[PRE + 'proj.weight'] = torch.zeros_like(V) if zero else V
    return PD, PT


def oracle_loop(monkeypatch, tokens, iters=3, seed=100, zero=False):
    """The text-conditioned 1:1 loop of schedule_cases.oracle_loop (RSGAN, GP 0.5, no loss means) with the projection head in the
    discriminator. Returns the per-iteration losses, the per-key D gradient norms of the first D step, and V after each D step."""
    import random
    import numpy as np
    PG, _, _, _ = S.oracle_states(dict(cond=True))
    PD, PT = discrim_state(zero)
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
    res = {'lossD': [], 'lossG': [], 'V': []}
    with monkeypatch.context() as mp:
        patch(mp)
        for it in range(iters):
            x = S.batch()
            with torch.no_grad():
                c = O.text_encode(PT, tokens, [8] * B)
            xs, conds, _ = O.multiscale_data(x, c, S.FS)
            z = torch.randn(B, 256)
            fake = O.multiscale_gen(PG, z, conds[0], training=True)
            for k in d_keys:
                PD[k].grad = None
            fc0 = conds[0][O.gen_perm(B)]
            l = O.discrim_loss(PD, PRE, xs, [f.detach() for f in fake], conds, [fc0[0:cc.size(0)] for cc in conds], 0.5)
            l.backward()
            if it == 0:
                res['D_gn0'] = {k: float(PD[k].grad.norm()) for k in d_keys}
            optD.step()
            res['lossD'].append(float(l.detach()))
            res['V'].append(PD[PRE + 'proj.weight'].detach().clone())
            with torch.no_grad():
                O.gen_perm(B)                               # all_discrim_forward draws a permutation it never uses
                real_pred = O.multiscale_discrim(PD, xs, conds, PRE)
            for k in g_keys:
                PG[k].grad = None
            l = O.gen_loss(PD, PRE, fake, real_pred, conds)
            l.backward()
            optG.step()
            res['lossG'].append(float(l.detach()))
    return res
