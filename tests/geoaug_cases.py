"""CPU restatement of the geometric augmentation of the discriminator's inputs (the names flip, scale, rotate of --D_aug; ADA's
geometric family, not in the reference) in plain torch — index arithmetic, any float dtype, autograd for the adjoint —
and the oracle loop of diffaug_cases with the extra draw and the geometric step at the call sites of the trainer. Shared by
test_geoaug_cpu.py and test_geoaug_gpu.py. No reference exists to record a fixture from, so this composition is the yardstick (as
with --D_aug itself).

The definition is the one in txt2vid_amd/functional_aug.py; f, s, theta and the fp32-rounded sampling matrix come from
`geo_params` (one definition), the resampling is restated here literally: output pixel (h, w) has xo = w + 0.5 - S/2,
yo = h + 0.5 - S/2, samples at px = (m00 xo + m01 yo) + S/2 - 0.5 (py from the second row), x0 = floor(px), wx = px - x0, and is
the bilinear blend of the four taps, a tap outside the frame contributing zero. Gated: clip j reads row j * stride of the gate
block; effective policy = policy & (8 [g3 < p] | 16 [g4 < p] | 32 [g5 < p]) with a strict fp32 <; 0 returns the clip itself.

Draw order on the host generator: diffaug_cases' (ada_cases' when gated), with every block u (and its g) followed at once by its
geometric block v: u_real, [g_real], v_real, u_fake, [g_fake], v_fake."""
import numpy as np
import torch

import diffaug_cases as DA
import schedule_cases as S
from oracle import tganv2_oracle as O
from txt2vid_amd import functional_aug as A

GEO = 'flip,scale,rotate'
SIX = DA.FULL + ',' + GEO
GEO_SUBSETS = ['flip', 'scale', 'rotate', 'flip,scale', 'flip,rotate', 'scale,rotate', GEO]
F32 = np.float32


def effective_geo(g, p, policy, n, stride=1):
    """The effective geometric bits of clips 0..n-1 of a member: clip j reads row j * stride of the gate block g [B, K] (fp32)."""
    bits = (A.parse_policy(policy) if isinstance(policy, str) else int(policy)) & A.GEO
    if g is None:
        return [bits] * n
    gn = g.detach().cpu().numpy().astype(F32)
    pv = F32(p)
    out = []
    for j in range(n):
        row = gn[j * stride]
        out.append(bits & ((8 if row[3] < pv else 0) | (16 if row[4] < pv else 0) | (32 if row[5] < pv else 0)))
    return out


def augment_geo(x, v, policy, stride=1, gates=None, p=None):
    """R(x) for clips x [N, C, T, S, S] (float32 or float64); clip j uses row j * stride of the block v [B, K] (fp32) and, gated, of
    `gates`. The non-geometric bits of `policy` are ignored."""
    N, C, T, Sd, W = x.shape
    assert Sd == W and (N - 1) * stride < v.shape[0] and (gates is None) == (p is None)
    eff = effective_geo(gates, p, policy, N, stride)
    rows = torch.arange(N) * stride
    M = A.geo_params(v.detach().cpu()[rows], torch.tensor(eff))['M'].to(x.dtype)       # the fp32-rounded matrix, exactly
    c = torch.arange(Sd, dtype=x.dtype) + 0.5 - Sd / 2
    xo, yo = c.view(1, Sd), c.view(Sd, 1)
    zero = torch.zeros((), dtype=x.dtype)
    out = []
    for j in range(N):
        if eff[j] == 0:
            out.append(x[j])
            continue
        m = M[j]
        px = (m[0, 0] * xo + m[0, 1] * yo) + Sd / 2 - 0.5
        py = (m[1, 0] * xo + m[1, 1] * yo) + Sd / 2 - 0.5
        x0, y0 = torch.floor(px), torch.floor(py)
        wx, wy = px - x0, py - y0
        val = None
        for dy in (0, 1):
            for dx in (0, 1):
                yy, xx = (y0 + dy).long(), (x0 + dx).long()
                ok = (yy >= 0) & (yy < Sd) & (xx >= 0) & (xx < Sd)
                wgt = (wy if dy else 1 - wy) * (wx if dx else 1 - wx)
                term = torch.where(ok, wgt, zero) * x[j][:, :, yy.clamp(0, Sd - 1), xx.clamp(0, Sd - 1)]
                val = term if val is None else val + term
        out.append(val)
    return torch.stack(out)


def augment_pyramid(xs, u, v, policy, subsample_input=True):
    """Geometry first, then diffaug_cases' colour / translation / cutout, with the same row rule."""
    bits = A.parse_policy(policy) if isinstance(policy, str) else int(policy)
    out = []
    for l, x in enumerate(xs):
        st = 2 ** l if subsample_input else 1
        y = augment_geo(x, v, bits, st) if bits & A.GEO else x
        out.append(DA.augment(y, u, bits & 7, st) if bits & 7 else y)
    return out


def oracle_loop(cond, N, M, policy=SIX, tokens=None, iters=3, seed=100):
    """diffaug_cases.oracle_loop with the geometric block v drawn behind every u and the geometric step in front of the
    colour / translation / cutout step. Returns the per-iteration totals of lossD and lossG."""
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

    def blocks():
        u = torch.rand(B, A.K)
        return u, torch.rand(B, A.K)                   # the geometric block right behind its parameter block
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
            u, v = blocks()
            xs_a = augment_pyramid(xs, u, v, policy)
            u, v = blocks()
            fk_a = augment_pyramid([f.detach() for f in fake], u, v, policy)
            fake_conds = None
            if conds is not None:
                fc0 = conds[0][O.gen_perm(B)]
                fake_conds = [fc0[0:cc.size(0)] for cc in conds]
            l = O.discrim_loss(PD, pre, xs_a, fk_a, conds, fake_conds, 0.5)          # draws this step's alphas
            l.backward()
            optD.step()
            tD += float(l.detach())
        u, v = blocks()
        xs_g = augment_pyramid(xs, u, v, policy)
        u_f, v_f = blocks()
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
                u_f, v_f = blocks()
            for k in g_keys:
                PG[k].grad = None
            l = O.gen_loss(PD, pre, augment_pyramid(fake, u_f, v_f, policy), real_pred, conds)
            l.backward()
            optG.step()
            tG += float(l.detach())
        res['lossD'].append(tD)
        res['lossG'].append(tG)
    return res


def consume(draws, B, L, n_levels, n_gen, N, M, gp, ca_dim, gated, geo):
    """ada_cases.consume with the geometric block: the draw methods in the order one eager iteration calls them; a site
    contributes u, then g when gated, then v when `geo`."""
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
        if geo:
            got = draws.aug(B, 'cpu', gated=gated, geo=True)
            assert len(got) == (3 if gated else 2)
        elif gated:
            got = draws.aug(B, 'cpu', gated=True)
        else:
            got = (draws.aug(B, 'cpu'),)
        for t in got:
            val(t)
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
