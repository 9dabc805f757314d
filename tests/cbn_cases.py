"""CPU restatement of the generator's conditional BatchNorm (`MultiScaleGen(cond_bn=True)`; DESIGN "Conditional BatchNorm"; not in
the reference) in plain torch, alone (the op cases) and composed with the oracle's functional pieces (oracle/tganv2_oracle.py) —
shared by test_cbn_cpu.py and test_cbn_gpu.py. No reference exists to record a fixture from, so these compositions are the
yardstick:

    tab = cond · Wᵀ + b [B, 2·ΣC];  site k owns columns o_k .. o_k + 2·C_k = [Δγ | Δβ]
    row n of a site at level ℓ belongs to level sample j = n // T_ℓ = base sample j·s  (s = 2^ℓ training, 1 eval)
    x̂ = batch_norm(x) without affine (running stats, counter as BatchNorm2d);  y = x̂ · (γ + Δγ[j·s]) + (β + Δβ[j·s])

`oracle.up_block` / `render_block` look `batchnorm_train` up at call time: `gen_cbn` swaps that name (pytest monkeypatch) for
`site_batchnorm`, which derives the site from the key prefix, T_ℓ and s from the level, and its rows from tab[::s].

Op tolerances: the metric and bounds of tests/norm_cases.py (1e-4 for y / dx / statistics, 2e-4 for dγ / dβ / the table gradient).
The restatement in fp32 against itself in float64, torch on the CPU, over every op case below, worst error / bound: y 0.09 and
dx 0.013 (of 1e-4), dγ 0.17 and the table gradient 0.09 (of 2e-4) — the bounds sit 4x or more above the restatement's own rounding
(test_cbn_cpu asserts it). Measured on an MI355X, worst error / bound over relu x up x fork x (alone, wide) and the raw ABI: y 0.10
(`tiny` / `offset`), dx 0.04 (`tiny` / `offset`), dγ 0.63 (`cap64` / `offset`), dβ 0.004, the table gradient 0.13 (`cap64` / `offset`),
running statistics 1.3e-3, (mean, 1/std) 2.3e-3."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import norm_cases as NC
import schedule_cases as S
from oracle import tganv2_oracle as O

# name -> ((rows, C, H, W), T, s, table rows)
CASES = {
    'tiny': ((6, 6, 5, 5), 2, 1, 3),
    'strided': ((12, 8, 3, 3), 4, 2, 5),           # table rows 0, 2, 4 used; rows 1, 3 must come back exactly zero
    'one_pixel': ((4, 5, 1, 1), 2, 1, 2),          # S = 1: `up` writes a 2x2 block per element; one lane per row in the row sums
    'one_sample': ((4, 7, 4, 4), 4, 1, 1),         # degenerates to the plain BatchNorm with gamma + dgamma
    'straddle': ((5, 8, 21, 29), 1, 1, 5),         # statistics slices cut across samples; a whole workgroup per row in the row sums
    'wide_c': ((2, 1030, 3, 3), 1, 1, 2),          # C beyond the statistics passes' workgroup target
    'cap64': ((2, 3, 181, 183), 1, 1, 2),          # the 64-way Chan merge
    'frames': ((24, 16, 8, 8), 8, 4, 9),           # many frames, large stride; a full wave per row in the row sums
}
RECIPES = ('plain', 'offset')
CASE_RECIPES = [(c, r) for c in CASES for r in (RECIPES if c in ('tiny', 'straddle', 'cap64') else ('plain',))]
MOMENTUM, EPS = 0.3, 1e-3
WIDE_PAD = (5, 6)                                   # columns in front of / behind the site in the `wide` table
TOL = dict(NC.TOL, dtab=2e-4)
RELU_BAND = NC.RELU_BAND


def geometry(case, wide):
    """(ld, off) of the table: the site alone, or at a non-zero column offset inside a wider table."""
    Cc = CASES[case][0][1]
    return (2 * Cc + sum(WIDE_PAD), WIDE_PAD[0]) if wide else (2 * Cc, 0)


def cbn(x, rm, rv, gamma, beta, tab, off, s, T, training, momentum, eps, counter=None):
    """The op in the dtype of its arguments. rm / rv are updated in place in training mode, like nn.BatchNorm2d's buffers."""
    N, Cc = x.shape[0], x.shape[1]
    rows = tab[::s][:N // T]
    assert rows.shape[0] * T == N, (tuple(x.shape), T, s, tuple(tab.shape))
    xhat = F.batch_norm(x, rm, rv, None, None, training, momentum, eps)
    if training and counter is not None:
        counter += 1
    dg = rows[:, off:off + Cc].repeat_interleave(T, 0)[:, :, None, None]
    db = rows[:, off + Cc:off + 2 * Cc].repeat_interleave(T, 0)[:, :, None, None]
    return xhat * (gamma[None, :, None, None] + dg) + (beta[None, :, None, None] + db)


@functools.lru_cache(maxsize=None)
def inputs(case, recipe, wide=False):
    """fp32 CPU tensors of one case / recipe (seeded; shared by every test, never modified)."""
    (N, Cc, H, W), T, s, R = CASES[case]
    ld, off = geometry(case, wide)
    g = torch.Generator()
    g.manual_seed(1000 * list(CASES).index(case) + RECIPES.index(recipe) + 29)

    def randn(*sh):
        return torch.randn(*sh, generator=g)
    x = randn(N, Cc, H, W)
    if recipe == 'offset':
        x = 300 + x
    inp = {'x': x, 'gamma': 1 + 0.1 * randn(Cc), 'beta': 0.1 * randn(Cc), 'rm': 0.1 * randn(Cc),
           'rv': 1 + 0.1 * torch.rand(Cc, generator=g), 'gy': randn(N, Cc, H, W), 'gy_up': randn(N, Cc, 2 * H, 2 * W),
           'w2': randn(N, Cc, H, W)}
    tab = 0.3 * randn(R, 2 * Cc)
    full = randn(R, ld)                              # (the columns outside the site hold values nobody may read or depend on)
    full[:, off:off + 2 * Cc] = tab
    inp['tab'] = full
    pre = cbn(x.double(), None, None, inp['gamma'].double(), inp['beta'].double(), full.double(), off, s, T, True, 0.0, EPS)
    near = (pre.abs() < RELU_BAND) & (pre != 0)
    inp['gy_relu'] = inp['gy'].masked_fill(near, 0.0)
    inp['gy_up_relu'] = inp['gy_up'].masked_fill(F.interpolate(near.double(), scale_factor=2) > 0, 0.0)
    assert TOL['y'] * (max(1.0, float(pre.abs().max())) + RELU_BAND) < RELU_BAND     # the band is wider than the y bound inside it
    return inp


def grad_out(inp, relu, up):
    return inp[('gy_up' if up else 'gy') + ('_relu' if relu else '')]


def reference(case, recipe, relu, up, fork='off', wide=False, training=True, dtype=torch.float64, tab=None):
    """The whole op on the CPU in `dtype`: cbn -> [relu] -> [F.interpolate(x2)], autograd for the gradients of (y * gy).sum()
    [+ (x * w2).sum(): the input's second consumer, fork = 'both']. `tab`: another table in place of the case's (zeros)."""
    inp = inputs(case, recipe, wide)
    _, T, s, R = CASES[case]
    ld, off = geometry(case, wide)
    c = lambda t: t.to(dtype, copy=True)              # (a copy in fp32 too: requires_grad_ below must never reach the shared inputs)
    xd = c(inp['x']).requires_grad_(training)
    gd, bd = c(inp['gamma']).requires_grad_(training), c(inp['beta']).requires_grad_(training)
    td = c(inp['tab'] if tab is None else tab).requires_grad_(training)
    rmd, rvd = c(inp['rm']).clone(), c(inp['rv']).clone()
    y = cbn(xd, rmd, rvd, gd, bd, td, off, s, T, training, MOMENTUM, EPS)
    if relu:
        y = F.relu(y)
    if up:
        y = F.interpolate(y, scale_factor=2)
    out = {'y': y.detach(), 'rm': rmd, 'rv': rvd}
    if not training:
        return out
    out['mean'] = c(inp['x']).mean((0, 2, 3))
    out['istd'] = 1.0 / torch.sqrt(c(inp['x']).var((0, 2, 3), unbiased=False) + EPS)
    loss = (y * c(grad_out(inp, relu, up))).sum()
    if fork == 'both':
        loss = loss + (xd * c(inp['w2'])).sum()
    out['dx'], out['dgamma'], out['dbeta'], out['dtab'] = torch.autograd.grad(loss, [xd, gd, bd, td])
    return out


@functools.lru_cache(maxsize=None)
def case_reference(case, recipe, relu, up, fork='off', wide=False, training=True):
    return reference(case, recipe, relu, up, fork, wide, training)


def check(tag, got, ref, fields):
    """Prints every field's ratio to its bound (`cbn-ratio <tag> <field> <ratio>`), then asserts all of them."""
    rs = {f: NC.ratio(got[f], ref[f], TOL[f]) for f in fields}
    for f in fields:
        print('cbn-ratio %s %s %.4g' % (tag, f, rs[f]))
    bad = {f: r for f, r in rs.items() if not r <= 1.0}
    assert not bad, '%s: error / bound %s' % (tag, bad)
    return rs


# ------------------------------------------------------------------------------------------------ composed with the oracle

def site_prefixes(n_add=3):
    """Key prefixes of the generator's BatchNorm sites in module registration order (site k)."""
    qs = ['abstract_blocks.0.up%d.main.inner_module.%d.' % (u, i) for u in range(3) for i in (0, 4)]
    qs += ['abstract_blocks.%d.main.inner_module.%d.' % (b, i) for b in range(1, n_add + 1) for i in (0, 4)]
    return qs + ['render_blocks.%d.bn.' % b for b in range(n_add + 1)]


def site_table(PG, n_add=3):
    """[(k, C_k, o_k)] from the recipe state's BatchNorm shapes."""
    out, o = [], 0
    for k, q in enumerate(site_prefixes(n_add)):
        Cc = PG[q + 'weight'].shape[0]
        out.append((k, Cc, o))
        o += 2 * Cc
    return out


def site_batchnorm(tab, offsets):
    """`oracle.batchnorm_train` with the site's modulation: the site from q, the level from q, s = 2^level in training mode,
    the rows from tab[::s], T from the row count."""
    qs = site_prefixes()

    def bn(P, q, x, training=True):
        k = qs.index(q)
        level = int(q.split('.')[1])
        s = 2 ** level if training else 1
        T = x.shape[0] // tab[::s].shape[0]
        return cbn(x, P[q + 'running_mean'], P[q + 'running_var'], P[q + 'weight'], P[q + 'bias'], tab, offsets[k], s, T, training,
                   0.1, 1e-5, counter=P[q + 'num_batches_tracked'])
    return bn


def gen_state(D=0, cond_dim=256, no_lstm=False, zero_proj=False):
    """Recipe weights of MultiScaleGen(cond_dim, ca_dim=D, cond_bn=True): the oracle's generator keys, ca.fc.* with CA, and
    cond_bn.* — non-zero by recipe (the module creates them as zeros), or zeros."""
    PG = O.recipe_state(O.gen_shapes(num_channels=1, cond_dim=D or cond_dim, cond_variant=True))
    if D:
        PG['ca.fc.weight'] = O.recipe_tensor('ca.fc.weight', (4 * D, cond_dim))
        PG['ca.fc.bias'] = O.recipe_tensor('ca.fc.bias', (4 * D,))
    if no_lstm:
        PG = {k: v for k, v in PG.items() if not k.startswith('clstm.')}
        for k, shp in seed_shapes().items():
            PG[k] = O.recipe_tensor(k, shp)
    total = 2 * sum(c for _, c, _ in site_table(PG))
    PG['cond_bn.weight'] = O.recipe_tensor('cond_bn.weight', (total, D or cond_dim))
    PG['cond_bn.bias'] = O.recipe_tensor('cond_bn.bias', (total,))
    if zero_proj:
        PG['cond_bn.weight'].zero_()
        PG['cond_bn.bias'].zero_()
    return PG


def seed_shapes(fm=1024):
    """Keys of the frame-seed generator (MultiScaleGen(no_lstm=True).frame_seed_gen, models/tgan/temporal_gen.py)."""
    s, chain = {}, (fm, 512, 256, 128, 128, fm)
    for i in range(5):
        s['frame_seed_gen.dc%d.weight' % i] = (chain[i], chain[i + 1], 1 if i == 0 else 4)
        s['frame_seed_gen.dc%d.bias' % i] = (chain[i + 1],)
        if i < 4:
            for name, shp in (('weight', (chain[i + 1],)), ('bias', (chain[i + 1],)), ('running_mean', (chain[i + 1],)),
                              ('running_var', (chain[i + 1],)), ('num_batches_tracked', ())):
                s['frame_seed_gen.bn%d.%s' % (i, name)] = shp
    return s


def seed_frames(P, q, x, steps=16, training=True):
    """In place of `oracle.conv_lstm` for no_lstm: the reference's FrameSeedGenerator.forward (temporal_gen.py:27-33) on the fc
    output, its [B, fm, 16] result reinterpreted as [B, 16, C, h, w] (MultiScaleGen.forward, gen.py:40-43) and cut into frames."""
    f = 'frame_seed_gen.'
    B = x.size(0)
    h = x.reshape(B, -1, 1)
    for i in range(4):
        h = F.conv_transpose1d(h, P[f + 'dc%d.weight' % i], P[f + 'dc%d.bias' % i], stride=1 if i == 0 else 2, padding=0 if i == 0 else 1)
        h = F.relu(F.batch_norm(h, P[f + 'bn%d.running_mean' % i], P[f + 'bn%d.running_var' % i], P[f + 'bn%d.weight' % i],
                                P[f + 'bn%d.bias' % i], training, 0.1, 1e-5))
        if training:
            P[f + 'bn%d.num_batches_tracked' % i] += 1
    z = torch.tanh(F.conv_transpose1d(h, P[f + 'dc4.weight'], P[f + 'dc4.bias'], stride=2, padding=1)).contiguous()
    v = z.view(B, steps, -1, x.size(2), x.size(3))
    return [v[:, t] for t in range(steps)]


def gen_cbn(monkeypatch, PG, z, s, training=True, eps=None, bts=None):
    """[CA +] the projection + `oracle.multiscale_gen` with every BatchNorm a conditional site. Returns (rendered, KL or None).
    With CA, eps is drawn here (before the generator's phases) unless given, and the projection reads c."""
    kl, vec = None, s
    if 'ca.fc.weight' in PG:
        import ca_cases as CA
        h = F.linear(s, PG['ca.fc.weight'], PG['ca.fc.bias'])
        if eps is None:
            eps = torch.randn(s.size(0), h.size(1) // 4)
        vec, kl = CA.ca_ref(h, eps)
    tab = F.linear(vec, PG['cond_bn.weight'], PG['cond_bn.bias'])
    offsets = [o for _, _, o in site_table(PG)]
    with monkeypatch.context() as mp:
        mp.setattr(O, 'batchnorm_train', site_batchnorm(tab, offsets))
        if 'frame_seed_gen.dc0.weight' in PG:
            mp.setattr(O, 'conv_lstm', functools.partial(seed_frames, training=training))
        return O.multiscale_gen(PG, z, vec, training=training, bts=bts), kl


def oracle_loop(monkeypatch, N, M, tokens, iters=3, seed=100):
    """The text-conditioned N:M loop of schedule_cases.oracle_loop (RSGAN, GP 0.5, no loss means) with conditional BatchNorm in
    the generator (recipe projection, non-zero). Returns the per-iteration totals of lossD and lossG."""
    import random
    _, PD, PT, pre = S.oracle_states(dict(cond=True))
    PG = gen_state()
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
        with torch.no_grad():
            c = O.text_encode(PT, tokens, [8] * B)
        xs, conds, _ = O.multiscale_data(x, c, S.FS)
        z = torch.randn(B, 256)
        fake, _ = gen_cbn(monkeypatch, PG, z, conds[0])
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
        tG = 0.0
        for j in range(M):
            if j:
                fake, _ = gen_cbn(monkeypatch, PG, z, conds[0])
            for k in g_keys:
                PG[k].grad = None
            l = O.gen_loss(PD, pre, fake, real_pred, conds)
            l.backward()
            optG.step()
            tG += float(l.detach())
        res['lossD'].append(tD)
        res['lossG'].append(tG)
    return res
