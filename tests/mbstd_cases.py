"""CPU restatement of the discriminator's minibatch standard deviation head (`Resnet3D(mbstd=G)`; DESIGN "Minibatch standard
deviation"; Karras et al. 2018; not in the reference) in plain torch, alone (the op cases) and composed with the oracle's
functional pieces (oracle/tganv2_oracle.py) — shared by test_mbstd_cpu.py and test_mbstd_gpu.py. No reference exists to record a
fixture from, so these compositions are the yardstick.

One definition. f [b, K] with a segment length seg (b % seg == 0, seg = b unless stated): rows [i·seg, (i+1)·seg) form a segment,
consecutive runs of G rows inside a segment a group; the last group of a segment holds the remainder (possibly one row); groups
never cross a segment boundary. Per group q of n rows:

    μ_k = (1/n) Σ_b f_bk      v_k = (1/n) Σ_b (f_bk − μ_k)²      σ_k = sqrt(v_k + 1e-8)      s_q = (1/K) Σ_k σ_k
    u[b] = fc_uncond(feat)[b] + w_u · s_q(b)         c[b] = (the conditional head, with proj if on)[b] + w_c · s_q(b)

`oracle.multiscale_discrim` / `gp_level` look `resnet3d` up at call time: `patch` swaps that name (pytest monkeypatch) for a
wrapper that adds the term to both logits of the unedited `oracle.resnet3d` (or of `proj_cases.resnet3d_proj`); the oracle calls
the trunk once per batch, so each call is one segment.

Op fields, per case (members share w [H]; per-member tensors are compared concatenated along the rows; y, base, r are [b, H]):
y;  gf, gw, gbase = the gradients of Σ y·r;  df = ∂(Σ y)/∂f (create_graph);  hf, hw = the gradients of Σ y·r + K·Σ df·t — a
Hessian-vector product, because Σ_b‖df_b‖² of this op does not depend on f (up to eps) and a ½‖df‖² probe would be degenerate.
Metric: per field max|got − ref| ≤ 1e-4 · max|ref|, and exact zeros wherever the reference is exactly zero (single-row groups,
a zero w). The restatement in fp32 against itself in float64 (torch on the CPU) stays below 0.25 of that bound on every case
and field (test_mbstd_cpu asserts it; worst measured: hf 0.086 on `eight`, every other field below 0.01). Worst error / bound
measured on an MI355X over the op cases, the raw ABI included: y 0.0009 (`real`), gf 0.0021 (`odd`), gw 0.0030 (`pyramid`), gbase
0, df 0.0037 (`whole`), hf 0.068 (`eight`; 0.032 on `halves`), hw 0.0041 (`whole`)."""
import functools

import torch

import proj_cases as PJ
import schedule_cases as S
from oracle import tganv2_oracle as O

EPS = 1e-8
# name -> (rows per member, segment length per member (None: the member's rows), K, G, H)
CASES = {
    'one': ([1], None, 1, 4, 1),
    'odd': ([7], None, 70, 4, 2),                                # groups of 4 and 3
    'pyramid': ([4, 2, 1, 1], None, 128, 4, 2),
    'real': ([33], None, 1024, 4, 2),                            # eight full groups and a single row
    'eight': ([5, 5, 3, 3, 2, 2, 1, 1], None, 192, 2, 2),        # T2V_MAX_GROUPS members, groups of 2 and 1
    'whole': ([32, 16], None, 1024, 16, 1),                      # the register-heaviest path
    'halves': ([6, 4], (3, 2), 96, 2, 2),                        # real‖fake members: groups restart at row 3 / row 2
}
# Groups of 2 have a zero Hessian away from coincidence (the statistic is |f_1 − f_2|/2 per channel) and a spike of the order of
# 1/sqrt(eps) at it, so `hf` of a G = 2 case is either that spike or pure cancellation noise of ANY fp32 evaluation (the terms that
# cancel are of size Γ/σ). `eight` has a near-coincident pair by its size; the seed of `halves` is the first after 2702 at which
# it has one too, judged by the restatement's own fp32-against-float64 error alone (test_mbstd_cpu asserts the 0.25 condition).
SEEDS = {name: 2600 + 17 * i for i, name in enumerate(CASES)}
SEEDS['halves'] = 2703         # (2702: no such pair — the restatement's own fp32 `hf` is 11 times the bound off its float64)
TOL = 1e-4
FIRST = ('y', 'gf', 'gw', 'gbase')
SECOND = ('df', 'hf', 'hw')
FIELDS = FIRST + SECOND


def segs_of(case):
    bs, segs = CASES[case][0], CASES[case][1]
    return list(bs) if segs is None else list(segs)


def groups(b, G, seg=None):
    """[(first row, rows)] of every group of a member of b rows."""
    seg = b if seg is None else seg
    assert seg >= 1 and b % seg == 0
    return [(r0, min(G, s0 + seg - r0)) for s0 in range(0, b, seg) for r0 in range(s0, s0 + seg, G)]


def stat(f, G, seg=None):
    """s_q(b) of every row as [b, 1], in the dtype of f: per-segment, per-group slicing."""
    out = []
    for r0, n in groups(f.shape[0], G, seg):
        grp = f[r0:r0 + n]
        mu = grp.mean(0, keepdim=True)
        v = ((grp - mu) ** 2).mean(0)
        out.append(torch.sqrt(v + EPS).mean().expand(n))
    return torch.cat(out).view(-1, 1)


def head(base, f, w, G, seg=None):
    """base [b, H] + w [H] · s: every head's logit with the term."""
    return base + stat(f, G, seg) * w.view(1, -1)


@functools.lru_cache(maxsize=None)
def inputs(case):
    """fp32 CPU tensors of one case (seeded; shared by every test, never modified): per member f ~ 2 N(0,1) [b, K], base ~ N(0,1)
    [b, H], r ~ N(0,1) [b, H], t ~ N(0,1) [b, K]; w ~ N(0,1) [H]."""
    bs, _, K, G, H = CASES[case]
    g = torch.Generator()
    g.manual_seed(SEEDS[case])
    out = {'w': torch.randn(H, generator=g), 'f': [], 'base': [], 'r': [], 't': []}
    for b in bs:
        out['f'].append(2 * torch.randn(b, K, generator=g))
        out['base'].append(torch.randn(b, H, generator=g))
        out['r'].append(torch.randn(b, H, generator=g))
        out['t'].append(torch.randn(b, K, generator=g))
    return out


def fields_of(ys, fs, w, bases, rs, ts, second=True):
    """Every op field from the per-member outputs `ys` [b, H] of any implementation (autograd does the rest)."""
    cat = lambda xs: torch.cat([x.detach() for x in xs], 0)
    out = {'y': cat(ys)}
    l1 = sum((y * r).sum() for y, r in zip(ys, rs))
    n, K = len(fs), fs[0].shape[1]
    g = torch.autograd.grad(l1, list(fs) + [w] + list(bases), retain_graph=second)
    out['gf'], out['gw'], out['gbase'] = cat(g[:n]), g[n].detach(), cat(g[n + 1:])
    if second:
        dfs = torch.autograd.grad(sum(y.sum() for y in ys), list(fs), create_graph=True)
        out['df'] = cat(dfs)
        l2 = l1 + K * sum((d * t).sum() for d, t in zip(dfs, ts))
        h = torch.autograd.grad(l2, list(fs) + [w])
        out['hf'], out['hw'] = cat(h[:n]), h[n].detach()
    return out


def reference(case, dtype=torch.float64, w=None):
    """The op in `dtype` on the CPU. `w`: another weight in place of the case's (zeros)."""
    inp = inputs(case)
    G = CASES[case][3]
    leaf = lambda t: t.detach().clone().to(dtype).requires_grad_(True)          # (never the cached input itself)
    fs, bases = [leaf(t) for t in inp['f']], [leaf(t) for t in inp['base']]
    wd = leaf(inp['w'] if w is None else w)
    ys = [head(b, f, wd, G, seg) for f, b, seg in zip(fs, bases, segs_of(case))]
    return fields_of(ys, fs, wd, bases, [r.to(dtype) for r in inp['r']], [t.to(dtype) for t in inp['t']])


@functools.lru_cache(maxsize=None)
def case_reference(case):
    return reference(case)


def ratio(got, ref):
    """max|got − ref| / (TOL · max|ref|); where the reference is exactly zero `got` must be exactly zero (else inf)."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if bool((got[ref == 0] != 0).any()) or not bool(torch.isfinite(got).all()):
        return float('inf')
    top = float(ref.abs().max())
    return 0.0 if top == 0 else float((got - ref).abs().max()) / (TOL * top)


def check(tag, got, ref, fields):
    """Prints every field's ratio to its bound (`mbstd-ratio <tag> <field> <ratio>`), then asserts all of them."""
    rs = {f: ratio(got[f], ref[f]) for f in fields}
    for f in fields:
        print('mbstd-ratio %s %s %.4g' % (tag, f, rs[f]))
    bad = {f: r for f, r in rs.items() if not r <= 1.0}
    assert not bad, '%s: error / bound %s' % (tag, bad)
    return rs


# ------------------------------------------------------------------------------------------------ composed with the oracle

_plain_resnet3d = O.resnet3d
GROUP = 3                      # on the ceil-halved pyramid of B = 4 (4, 2, 1, 1 rows): a group of 3 and a single row, a group of 2, single rows
W_RECIPE = (40.0, -60.0)        # (w_u, w_c) of the module tests: see `discrim_state`


def wrapped(G, inner=None):
    """`oracle.resnet3d` (or `inner`) with the term on both logits: (u + w_u·s, c + w_c·s, feat), each call one segment."""
    inner = inner or _plain_resnet3d

    def resnet3d_mbstd(P, x, cond=None, prefix='', **kw):
        u, c, feat = inner(P, x, cond, prefix=prefix, **kw)
        w = P[prefix + 'mbstd.weight']
        s = stat(feat, G)
        u = u + w[0] * s
        if c is not None:
            c = c + w[1] * s
        return u, c, feat
    return resnet3d_mbstd


def patch(mp, G=GROUP, proj=False):
    """From here to the end of the monkeypatch (context), every oracle function that calls `resnet3d` runs with the head (and
    with the projection term under it when `proj`)."""
    mp.setattr(O, 'resnet3d', wrapped(G, PJ.resnet3d_proj if proj else None))


def prefix(cond):
    return 'single_discrim.module.' if cond else 'single_discrim.'


def discrim_state(cond=True, proj=False, zero=False):
    """Recipe weights of MultiScaleDiscrim(num_channels=1, mbstd=GROUP) — text-conditioned (cond_dim 256, optionally with proj) or
    unconditional: the oracle's keys, proj.weight, and mbstd.weight = W_RECIPE (its first entry alone without a sentence code), or
    zeros. On the recipe trunk the statistic of the two levels with more than one row is 0.0010 to 0.0023 (CPU, oracle) next to
    logits of mean size 0.05 to 0.34 there: W_RECIPE gives a term of 0.04 to 0.10, which the module tests assert on their own
    features to be of the size of the existing logits. (A single-row level's statistic is sqrt(eps) = 1e-4, with no gradient.)"""
    _, PD, PT, pre = S.oracle_states(dict(cond=cond))
    assert pre == prefix(cond)
    if proj:
        PD[pre + 'proj.weight'] = O.recipe_tensor(pre + 'proj.weight', (1024, 256))
    w = torch.tensor(W_RECIPE[:2 if cond else 1])
    PD[pre + 'mbstd.weight'] = torch.zeros_like(w) if zero else w
    return PD, PT


def oracle_loop(monkeypatch, cond, tokens=None, iters=3, seed=100, proj=False, zero=False):
    """The 1:1 loop of schedule_cases.oracle_loop (RSGAN, GP 0.5, no loss means) with the head in the discriminator. Returns the
    per-iteration losses, the per-key D gradient norms of the first D step, and w after each D step."""
    import random
    import numpy as np
    PG, _, _, pre = S.oracle_states(dict(cond=cond))
    PD, PT = discrim_state(cond, proj, zero)
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
    res = {'lossD': [], 'lossG': [], 'w': []}
    with monkeypatch.context() as mp:
        patch(mp, GROUP, proj)
        for it in range(iters):
            x = S.batch()
            c = None
            if cond:
                with torch.no_grad():
                    c = O.text_encode(PT, tokens, [8] * B)
            xs, conds, _ = O.multiscale_data(x, c, S.FS)
            z = torch.randn(B, 256)
            fake = O.multiscale_gen(PG, z, conds[0] if cond else None, training=True)
            for k in d_keys:
                PD[k].grad = None
            fake_conds = None
            if cond:
                fc0 = conds[0][O.gen_perm(B)]
                fake_conds = [fc0[0:cc.size(0)] for cc in conds]
            l = O.discrim_loss(PD, pre, xs, [f.detach() for f in fake], conds if cond else None, fake_conds, 0.5)
            l.backward()
            if it == 0:
                res['D_gn0'] = {k: float(PD[k].grad.norm()) for k in d_keys}
            optD.step()
            res['lossD'].append(float(l.detach()))
            res['w'].append(PD[pre + 'mbstd.weight'].detach().clone())
            with torch.no_grad():
                if cond:
                    O.gen_perm(B)                               # all_discrim_forward draws a permutation it never uses
                    real_pred = O.multiscale_discrim(PD, xs, conds, pre)
                else:
                    real_pred = [r[0] for r in O.multiscale_discrim(PD, xs, None, pre)]
            for k in g_keys:
                PG[k].grad = None
            l = O.gen_loss(PD, pre, fake, real_pred, conds if cond else None)
            l.backward()
            optG.step()
            res['lossG'].append(float(l.detach()))
    return res
