"""GPU: the discriminator's opt-in projection head (Resnet3D(proj=True); DESIGN "Projection head") on the HIP path, against the
float64 / plain-torch restatement of tests/proj_cases.py, alone and composed with the oracle: the four `t2v_proj_*` roles through
their autograd surface up to the double backward (metric of tests/norm_cases.py, 1e-4), the raw ABI on guarded buffers, the
module, the D and G step losses, three training iterations, graph replay, --end2end, the launch budget and the command line."""
import ctypes as C
import glob
import json
import os
import random
import subprocess
import sys
from collections import Counter

import numpy as np
import pytest
import torch

import proj_cases as PJ
import schedule_cases as S
from oracle import tganv2_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, B = S.V, S.B
PRE = PJ.PRE


def seed(s):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


def _trace(monkeypatch, fn):
    """Names of the C entry points `fn` calls, in order."""
    from txt2vid_amd import _lib
    L, calls = _lib.lib(), []

    def wrap(name, orig):
        def f(*a):
            calls.append(name)
            return orig(*a)
        return f
    with monkeypatch.context() as mp:
        for name in _lib.SIGNATURES:
            mp.setattr(L, name, wrap(name, getattr(L, name)))
        fn()
    torch.cuda.synchronize()
    return calls


def _proj_calls(calls):
    return dict(Counter(c for c in calls if c.startswith('t2v_proj_')))


# ------------------------------------------------------------------------------------------------ op level: the autograd surface

def leaves(case, V_=None):
    inp = PJ.inputs(case)
    dev = lambda t: t.to(DEV).requires_grad_(True)
    Vd = torch.nn.Parameter((inp['V'] if V_ is None else V_).to(DEV))
    return [dev(t) for t in inp['f']], [dev(t) for t in inp['s']], Vd, [dev(t) for t in inp['base']], [t.to(DEV) for t in inp['r']]


def run_op(case, V_=None, second=True):
    """The rows role on fresh device copies of the case's inputs, and every op field behind it through autograd."""
    from txt2vid_amd import functional as TF
    fs, ss, Vd, bases, rs = leaves(case, V_)
    ys = TF.proj_rows_group(Vd, fs, ss, bases)
    return PJ.fields_of(ys, fs, ss, Vd, bases, rs, second)


@pytest.mark.parametrize('case', list(PJ.CASES))
def test_forward_first_order_and_double_backward(case):
    got = run_op(case)
    PJ.check(case, got, PJ.case_reference(case), PJ.FIELDS)


@pytest.mark.parametrize('case', list(PJ.CASES))
def test_zero_v_returns_base_and_still_gets_its_gradient(case):
    inp = PJ.inputs(case)
    zero = torch.zeros_like(inp['V'])
    got = run_op(case, zero, second=False)
    ref = PJ.reference(case, V=zero)
    assert torch.equal(got['y'].cpu(), torch.cat(inp['base'], 0))
    assert not got['gf'].any() and not got['gs'].any()              # exact zeros
    PJ.check(case + '/zeroV', got, ref, PJ.FIRST)
    assert float(ref['gV'].abs().max()) > 0


def test_a_member_without_gradient_is_left_out(monkeypatch):
    """Members 1 and 3 of the pyramid case take no part in the loss: their inputs get no gradient, the launches run over two
    members, the others' gradients are bitwise those of the full run, and dL/dV is the sum over the two."""
    from txt2vid_amd import functional as TF
    full = run_op('pyramid', second=False)
    fs, ss, Vd, bases, rs = leaves('pyramid')
    ys = TF.proj_rows_group(Vd, fs, ss, bases)
    loss = sum((ys[i] * rs[i]).sum() for i in (0, 2))
    box = {}
    calls = _trace(monkeypatch, lambda: box.update(g=torch.autograd.grad(loss, fs + ss + [Vd] + bases, allow_unused=True)))
    g = box['g']
    assert _proj_calls(calls) == {'t2v_proj_feat': 1, 't2v_proj_cond': 1, 't2v_proj_weight': 1}
    n, bs = 4, PJ.CASES['pyramid'][0]
    rows = np.cumsum([0] + bs)
    for i in range(n):
        for grads, field in ((g[:n], 'gf'), (g[n:2 * n], 'gs'), (g[2 * n + 1:], 'gbase')):
            if i in (1, 3):
                assert grads[i] is None
            else:
                assert torch.equal(grads[i], full[field][rows[i]:rows[i + 1]]), (i, field)
    inp = PJ.inputs('pyramid')
    want = sum((inp['r'][i].double() * inp['f'][i].double()).t() @ inp['s'][i].double() for i in (0, 2))
    assert PJ.NC.ratio(g[2 * n], want, PJ.TOL) <= 1.0


def test_frozen_v_and_input_grads_only_issue_no_weight_call(monkeypatch):
    from txt2vid_amd import functional as TF
    fs, ss, Vd, bases, rs = leaves('eight')

    def sweep():
        ys = TF.proj_rows_group(Vd, fs, ss, bases)
        with TF.input_grads_only():
            torch.autograd.grad(sum(y.sum() for y in ys), fs)
    assert _proj_calls(_trace(monkeypatch, sweep)) == {'t2v_proj_rows': 1, 't2v_proj_feat': 1, 't2v_proj_cond': 1}
    Vd.requires_grad_(False)
    ss = [s.detach() for s in ss]                                   # and without --end2end the sentence code carries no gradient

    def frozen():
        ys = TF.proj_rows_group(Vd, fs, ss, bases)
        sum((y * r).sum() for y, r in zip(ys, rs)).backward()
    assert _proj_calls(_trace(monkeypatch, frozen)) == {'t2v_proj_rows': 1, 't2v_proj_feat': 1}
    assert Vd.grad is None and all(f.grad is not None for f in fs)


@pytest.mark.parametrize('case', ['real', 'eight'])
def test_two_runs_give_the_same_bits(case):
    a, b = run_op(case), run_op(case)
    for f in PJ.FIELDS:
        assert torch.equal(a[f], b[f]), f


# ------------------------------------------------------------------------------------------------ op level: the raw ABI, guarded

SENTINEL = -7777.25
GUARD = 256


class Guarded(object):
    """`n` elements carved out of a larger allocation, GUARD sentinel elements on each side; the inside starts as NaN (or `init`),
    so an element the kernel never wrote fails the comparison."""

    def __init__(self, n, init=None):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), SENTINEL, device=DEV, dtype=torch.float32)
        self.t = self.buf[GUARD:GUARD + n]
        if init is None:
            self.t.fill_(float('nan'))
        else:
            self.t.copy_(init.reshape(-1))
        self.p = self.t.data_ptr()

    def intact(self):
        return bool((self.buf[:GUARD] == SENTINEL).all()) and bool((self.buf[GUARD + self.n:] == SENTINEL).all())


@pytest.mark.parametrize('case', ['one', 'odd', 'pyramid', 'eight'])
def test_raw_abi_on_guarded_buffers(case):
    """The four entry points with no Python caller: the restatement's values with g = r, the weight role written and then
    accumulated onto, nothing written outside any buffer."""
    from txt2vid_amd._lib import lib, ProjMember
    from txt2vid_amd._ops import _stream
    L, st = lib(), _stream()
    inp = PJ.inputs(case)
    bs, K, J = PJ.CASES[case]
    n = len(bs)
    keep = {k: [t.to(DEV).contiguous() for t in inp[k]] for k in ('f', 's', 'base', 'r')}
    Vd = inp['V'].to(DEV).contiguous()
    guards = []

    def out(k, init=None):
        guards.append(Guarded(k, init))
        return guards[-1]

    def table(outs=None, base=True):
        arr = (ProjMember * n)()
        for i, a in enumerate(arr):
            a.g, a.f, a.s, a.b = keep['r'][i].data_ptr(), keep['f'][i].data_ptr(), keep['s'][i].data_ptr(), bs[i]
            a.base = keep['base'][i].data_ptr() if base else None
            a.out = outs[i].p if outs is not None else None
        return arr
    ys, y0 = [out(b) for b in bs], [out(b) for b in bs]
    Fs, Cs = [out(b * K) for b in bs], [out(b * J) for b in bs]
    prior = torch.full((K, J), 0.5, device=DEV)
    W, W2 = out(K * J), out(K * J, prior)
    assert L.t2v_proj_rows(table(ys), n, C.c_void_p(Vd.data_ptr()), K, J, st) == 0
    assert L.t2v_proj_rows(table(y0, base=False), n, C.c_void_p(Vd.data_ptr()), K, J, st) == 0
    assert L.t2v_proj_feat(table(Fs), n, C.c_void_p(Vd.data_ptr()), K, J, st) == 0
    assert L.t2v_proj_cond(table(Cs), n, C.c_void_p(Vd.data_ptr()), K, J, st) == 0
    assert L.t2v_proj_weight(table(), n, C.c_void_p(W.p), K, J, 0, st) == 0
    assert L.t2v_proj_weight(table(), n, C.c_void_p(W2.p), K, J, 1, st) == 0
    torch.cuda.synchronize()
    assert all(g.intact() for g in guards), [i for i, g in enumerate(guards) if not g.intact()]
    ref = PJ.case_reference(case)
    base = torch.cat(inp['base'], 0).double()
    got = {'y': torch.cat([g.t for g in ys]).view(-1, 1), 'y0': torch.cat([g.t for g in y0]).view(-1, 1),
           'gf': torch.cat([g.t.view(b, K) for g, b in zip(Fs, bs)], 0), 'gs': torch.cat([g.t.view(b, J) for g, b in zip(Cs, bs)], 0),
           'gV': W.t.view(K, J), 'gV2': W2.t.view(K, J)}
    want = dict(ref, y0=ref['y'] - base, gV2=ref['gV'] + 0.5)
    PJ.check(case + '/abi', got, want, ['y', 'y0', 'gf', 'gs', 'gV', 'gV2'])


def test_entry_points_refuse_bad_arguments_and_launch_nothing():
    """Real device pointers, bad arguments: T2V_EINVAL (a launch would return 0 or a HIP status) and the buffers keep their
    sentinel pattern."""
    from txt2vid_amd._lib import lib, ProjMember, MAX_GROUPS
    L = lib()
    buf = torch.full((4096,), 3.5, device=DEV)
    p = buf.data_ptr()

    def members(n=1, b=2, **null):
        arr = (ProjMember * max(n, 1))()
        for a in arr:
            a.g, a.f, a.s, a.base, a.out, a.b = p, p, p, p, p, b
            for k in null:
                setattr(a, k, None)
        return arr
    Vp = C.c_void_p(p)
    roles = {'rows': L.t2v_proj_rows, 'feat': L.t2v_proj_feat, 'cond': L.t2v_proj_cond,
             'weight': lambda m, n, v, K, J, st: L.t2v_proj_weight(m, n, v, K, J, 0, st)}
    for name, fn in roles.items():
        assert fn(None, 1, Vp, 4, 4, None) == -1 and fn(members(), 1, None, 4, 4, None) == -1, name
        assert fn(members(), 0, Vp, 4, 4, None) == -1 and fn(members(MAX_GROUPS + 1), MAX_GROUPS + 1, Vp, 4, 4, None) == -1, name
        assert fn(members(), 1, Vp, 0, 4, None) == -1 and fn(members(), 1, Vp, 4, 0, None) == -1 and fn(members(), 1, Vp, -1, 4, None) == -1, name
        assert fn(members(b=0), 1, Vp, 4, 4, None) == -1 and fn(members(2, b=-3), 2, Vp, 4, 4, None) == -1, name
    for name, reads in (('rows', ('f', 's', 'out')), ('feat', ('g', 's', 'out')), ('cond', ('g', 'f', 'out')), ('weight', ('g', 'f', 's'))):
        for k in reads:
            assert roles[name](members(**{k: None}), 1, Vp, 4, 4, None) == -1, (name, k)
    torch.cuda.synchronize()
    assert bool((buf == 3.5).all())


def test_symbols_are_exported_and_declared():
    from txt2vid_amd import _lib
    names = ['t2v_proj_rows', 't2v_proj_feat', 't2v_proj_cond', 't2v_proj_weight']
    header = open(os.path.join(ROOT, 'include', 't2v_hip.h')).read()
    for name in names:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name) and ('int %s(' % name) in header


# ------------------------------------------------------------------------------------------------ module level

def pour(module, PD=None):
    sd = {k: O.recipe_tensor(k, v.shape) for k, v in module.state_dict().items()}
    if PD is not None and PRE + 'proj.weight' in sd:
        sd[PRE + 'proj.weight'] = PD[PRE + 'proj.weight'].detach().clone()
    module.load_state_dict(sd)
    return module.to(DEV)


def _discrim(**kw):
    from txt2vid_amd.models.tganv2_cond.discrim import MultiScaleDiscrim
    return MultiScaleDiscrim(num_channels=1, cond_dim=256, **kw)


def tokens_for(batch, s=77):
    tg = torch.Generator()
    tg.manual_seed(s)
    t = torch.randint(4, V, (batch, 8), generator=tg)
    t[:, 0], t[:, -1] = 1, 2
    return t


def pyramid(s=3):
    """Clips and sentence codes of the ceil-halved pyramid of B = 4 at 64x64, C = 1 (CPU)."""
    g = torch.Generator()
    g.manual_seed(s)
    x = (torch.rand(B, 16, 1, 64, 64, generator=g) * 2 - 1).permute(0, 2, 1, 3, 4).contiguous()
    c = 0.1 * torch.randn(B, 256, generator=g)
    xs, conds, _ = O.multiscale_data(x, c, S.FS)
    return [t.contiguous() for t in xs], [t.contiguous() for t in conds]


def test_fresh_proj_discriminator_is_the_plain_one():
    """V = 0: on the same weights and inputs (u, c, feat) are those of the proj=False discriminator — bitwise, c as `base + 0` —
    through the grouped pass and through the single-tensor forward."""
    off, on = pour(_discrim()).train(), pour(_discrim(proj=True), PJ.discrim_state(zero=True)[0]).train()
    assert not on.single_discrim.module.proj.weight.any()
    xs, conds = pyramid()
    xs, conds = [t.to(DEV) for t in xs], [t.to(DEV) for t in conds]
    with torch.no_grad():
        a, b = off(x=xs, cond=conds), on(x=xs, cond=conds)
        a1, b1 = off.sub_discrims[0](xs[1], cond=conds[1]), on.sub_discrims[0](xs[1], cond=conds[1])
    for (u0, c0, f0), (u1, c1, f1) in list(zip(a, b)) + [(a1, b1)]:
        assert torch.equal(u0, u1) and torch.equal(c0, c1) and torch.equal(f0, f1)


def _oracle_params(PD):
    keys = [k for k, v in PD.items() if v.dtype.is_floating_point]
    for k in keys:
        PD[k].requires_grad_(True)
    return keys


def _norms_close(grads, PD, keys, tag, rtol=3e-3):
    """`grads`: key -> dL/dparameter on the device, against the oracle state's .grad."""
    got = np.array([float(grads[k].double().norm()) for k in keys])
    want = np.array([float(PD[k].grad.double().norm()) for k in keys])
    rel = float(np.linalg.norm(got - want) / np.linalg.norm(want))
    print('proj %s: gradient-norm vector rel %.3g; |dV| %.6g (%.6g)' % (tag, rel, got[-1], want[-1]))
    assert rel < rtol, rel
    assert keys[-1].endswith('proj.weight') and want[-1] > 0 and abs(got[-1] - want[-1]) < rtol * want[-1]
    a, b = grads[keys[-1]].cpu().double(), PD[keys[-1]].grad.double()
    assert float((a - b).norm() / b.norm()) < rtol               # element by element too


def test_forward_levels_vs_wrapped_oracle(monkeypatch):
    """One grouped pass over the pyramid with the recipe V: logits and features, the gradients of a fixed weighted sum of the
    logits with respect to every parameter and to the clips, against `oracle.multiscale_discrim` with the wrapped head. Bounds
    of the cBN / CA module tests: rtol 2e-3, atol 5e-4 x scale on the outputs; 3e-3 on the gradient norms. The per-member
    fallback computes the same conditional logits."""
    PD, _ = PJ.discrim_state()
    dis = pour(_discrim(proj=True), PD).train()
    keys = _oracle_params(PD)
    assert [k for k, _ in dis.named_parameters()] == keys
    xs, conds = pyramid()
    g = torch.Generator()
    g.manual_seed(9)
    wu, wc = [torch.randn(x.shape[0], 1, generator=g) for x in xs], [torch.randn(x.shape[0], 1, generator=g) for x in xs]
    xd = [t.to(DEV).requires_grad_(True) for t in xs]
    res = dis(x=xd, cond=[t.to(DEV) for t in conds])
    loss = sum((u * a.to(DEV)).sum() + (c * b.to(DEV)).sum() for (u, c, _), a, b in zip(res, wu, wc))
    loss.backward()
    xo = [t.clone().requires_grad_(True) for t in xs]
    with monkeypatch.context() as mp:
        PJ.patch(mp)
        ro = O.multiscale_discrim(PD, xo, conds, PRE)
    lo = sum((u * a).sum() + (c * b).sum() for (u, c, _), a, b in zip(ro, wu, wc))
    lo.backward()
    terms, heads = [], []
    for (u, c, f), (uo, co, fo), s in zip(res, ro, conds):
        for a, b in ((u, uo), (c, co), (f, fo)):
            scale = max(1.0, float(b.abs().max()))
            np.testing.assert_allclose(a.detach().cpu().numpy(), b.detach().numpy(), rtol=2e-3, atol=5e-4 * scale)
        t = PJ.term(fo.detach(), s, PD[PRE + 'proj.weight'].detach())
        terms.append(float(t.abs().mean()))
        heads.append(float((co.detach() - t).abs().mean()))
    print('proj term / existing head, mean size per level: %s / %s' % (terms, heads))
    # the term cannot hide below the tolerance: it is of the size of the existing head on every level
    assert all(0.1 < t / h < 10 for t, h in zip(terms, heads)), (terms, heads)
    _norms_close({k: p.grad for k, p in dis.named_parameters()}, PD, keys, 'forward_levels')
    for a, b in zip(xd, xo):
        assert float((a.grad.cpu().double() - b.grad.double()).norm() / b.grad.double().norm()) < 3e-3
    # grouped heads against the per-member fallback (computed_features) on the same features
    trunk = dis.single_discrim.module
    feats, cd = [f.detach() for _, _, f in res], [t.to(DEV) for t in conds]
    with torch.no_grad():
        grouped = trunk.cond_heads(feats, cd)
        single = [trunk(cond=c_, computed_features=f_)[1] for f_, c_ in zip(feats, cd)]
    for a, b, (_, c, _) in zip(grouped, single, res):
        assert torch.equal(a, b) and torch.equal(a, c.detach())


def make(proj=True, zero=False, batch=B):
    from txt2vid_amd.models.tganv2_cond.gen import MultiScaleGen
    from txt2vid_amd.models.txt.basic import Seq2Seq
    from txt2vid_amd.gan.cond_gan import CondGan
    from txt2vid_amd.gan.losses import MixedGanLoss, RSGANLoss
    from txt2vid_amd.optim import Adam
    gen = pour(MultiScaleGen(width=64, height=64, num_channels=1, cond_dim=256)).train()
    dis = pour(_discrim(proj=proj), PJ.discrim_state(zero)[0]).train()
    txt = Seq2Seq(vocab_size=V)
    txt.load_state_dict({k: O.recipe_tensor(k if k.startswith('encoder.') else 'encoder.' + k[len('decoder.'):], v.shape)
                         for k, v in txt.state_dict().items()})
    txt.to(DEV)
    gan = CondGan(gen=gen, discrims=[dis], cond_encoder=txt, discrim_names=['video'])
    optD = Adam([{'params': dis.parameters()}], lr=2e-4, betas=(0.5, 0.999))
    optG = Adam([{'params': gen.parameters()}], lr=2e-4, betas=(0.5, 0.999))
    prm = S.params_for(dict(N=1, M=1, gp=0.5, mean_d=False, mean_g=False))
    return gan, optD, optG, MixedGanLoss(g_loss=RSGANLoss(), d_loss=RSGANLoss()), prm


def test_d_and_g_step_losses_and_gradient_norms_vs_wrapped_oracle(monkeypatch):
    """One D step with the gradient penalty (lambda 0.5: mismatched-caption heads, the sweep and the second backward through the
    projection) and one G step, recipe V, against `oracle.discrim_loss` / `gen_loss` with the wrapped head on the same draws:
    losses within 1e-3 x max(1, |ref|), every gradient-norm vector within 3e-3 (the cBN / CA module bounds), dL/dV element by
    element."""
    from txt2vid_amd import functional as TF
    from txt2vid_amd.gan.trainer import multiscale_data
    gan, optD, optG, losses, prm = make()
    dis, gen = gan.discrims[0], gan.gen
    TF.set_grad_sink(None)
    PG, _, _, _ = S.oracle_states(dict(cond=True))
    PD, PT = PJ.discrim_state()
    d_keys = _oracle_params(PD)
    g_keys = [k for k, v in PG.items() if v.dtype.is_floating_point and 'running_' not in k]
    for k in g_keys:
        PG[k].requires_grad_(True)
    seed(7)
    x = S.batch()
    tokens = tokens_for(B)
    with torch.no_grad():
        cond = gan.cond_encoder.encode(tokens.to(DEV), [8] * B)[2].detach()
    state = (torch.get_rng_state(), np.random.get_state(), random.getstate())
    xs, conds = multiscale_data(x.to(DEV), cond, prm.frame_sizes, True)          # (draws the sub-sampling phases of the pyramid)
    z = torch.randn(B, 256)
    fake = gan(z.to(DEV), cond=conds[0])
    lD = gan.discrim_step(real=xs, fake=[f.detach() for f in fake], cond=conds, loss=losses.discrim_loss, gp_lambda=0.5)
    lD.backward()
    TF.grad_sink_flush()
    with torch.no_grad():
        _, _, real_pred = gan.all_discrim_forward(real=xs, cond=conds, fake=None, loss=None)
    d_named = {k: p for k, p in dis.named_parameters()}
    d_grads = {k: p.grad.detach().clone() for k, p in d_named.items()}
    lG = gan.gen_step(fake=fake, real_pred=real_pred, cond=conds, loss=losses.gen_loss)
    lG.backward()
    TF.grad_sink_flush()
    torch.cuda.synchronize()
    torch.set_rng_state(state[0])
    np.random.set_state(state[1])
    random.setstate(state[2])
    with torch.no_grad():
        co = O.text_encode(PT, tokens, [8] * B)
    xo, cso, _ = O.multiscale_data(x, co, S.FS)
    assert torch.equal(torch.randn(B, 256), z)                                    # the same draws in the same order
    with monkeypatch.context() as mp:
        PJ.patch(mp)
        fo = O.multiscale_gen(PG, z, cso[0], training=True)
        fc0 = cso[0][O.gen_perm(B)]
        lDo = O.discrim_loss(PD, PRE, xo, [f.detach() for f in fo], cso, [fc0[0:cc.size(0)] for cc in cso], 0.5)
        lDo.backward()
        _norms_close(d_grads, PD, d_keys, 'D step')
        with torch.no_grad():
            O.gen_perm(B)
            rp = O.multiscale_discrim(PD, xo, cso, PRE)
        lGo = O.gen_loss(PD, PRE, fo, rp, cso)
        lGo.backward()
    print('proj D step: lossD %.6f (%.6f) lossG %.6f (%.6f)' % (float(lD), float(lDo), float(lG), float(lGo)))
    assert abs(float(lD) - float(lDo)) < 1e-3 * max(1.0, abs(float(lDo)))
    assert abs(float(lG) - float(lGo)) < 1e-3 * max(1.0, abs(float(lGo)))
    g_named = dict(gen.named_parameters())
    got = np.array([float(g_named[k].grad.double().norm()) for k in g_keys])
    want = np.array([float(PG[k].grad.double().norm()) for k in g_keys])
    rel = float(np.linalg.norm(got - want) / np.linalg.norm(want))
    print('proj G step: gradient-norm vector rel %.3g' % rel)
    assert rel < 3e-3, rel


# ------------------------------------------------------------------------------------------------ iteration level

def test_proj_iterations_vs_wrapped_oracle(monkeypatch):
    """Three text-conditioned 1:1 iterations from the recipe V against the oracle loop with the wrapped head: lossD and lossG at
    the bounds of the cBN loop test (1e-3, then 2e-2 in iteration 2: the GAN dynamics are chaotic); the per-key D gradient norms
    of the first D step at its --end2end bound (1e-2 of the norm + 1e-5 of the largest); V after the first D step."""
    from txt2vid_amd.gan.trainer import TrainStep
    tokens = tokens_for(B)
    ref = PJ.oracle_loop(monkeypatch, tokens, iters=3)
    gan, optD, optG, losses, prm = make()
    dis = gan.discrims[0]
    seed(100)
    for it in range(3):
        x = S.batch().to(DEV)
        with torch.no_grad():
            cond = gan.cond_encoder.encode(tokens.to(DEV), [8] * B)[2].detach()
        lD, lG, _, _ = TrainStep(gan, optD, optG, losses, prm, DEV).run(x, cond)
        lD, lG = float(lD), float(lG)
        tol = 1e-3 if it < 2 else 2e-2
        print('proj it %d: lossD %.6f (%.6f) lossG %.6f (%.6f)' % (it, lD, ref['lossD'][it], lG, ref['lossG'][it]))
        assert abs(lD - ref['lossD'][it]) < tol * max(1.0, abs(ref['lossD'][it]))
        assert abs(lG - ref['lossG'][it]) < tol * max(1.0, abs(ref['lossG'][it]))
        if it == 0:
            top = max(ref['D_gn0'].values())
            for k, p in dis.named_parameters():
                got, want = float(p.grad.norm()), ref['D_gn0'][k]
                assert abs(got - want) <= 1e-2 * want + 1e-5 * top, (k, got, want)
            Vg, Vo = dis.single_discrim.module.proj.weight.detach().cpu().double(), ref['V'][0].double()
            assert float((Vg - Vo).norm() / Vo.norm()) < 1e-3


def test_v_leaves_zero_after_the_first_d_step(monkeypatch):
    from txt2vid_amd.gan.trainer import TrainStep
    tokens = tokens_for(B)
    gan, optD, optG, losses, prm = make(zero=True)
    Vp = gan.discrims[0].single_discrim.module.proj.weight
    assert not Vp.any()
    seed(100)
    x = S.batch().to(DEV)
    with torch.no_grad():
        cond = gan.cond_encoder.encode(tokens.to(DEV), [8] * B)[2].detach()
    TrainStep(gan, optD, optG, losses, prm, DEV).run(x, cond)
    assert float(Vp.grad.norm()) > 0 and float(Vp.detach().abs().max()) > 0
    # Adam's first step moves every element with a non-zero gradient by lr
    assert abs(float(Vp.detach().abs().max()) - 2e-4) < 1e-6


def test_proj_graph_replay_matches_eager():
    """GraphedTrainStep with the projection head inside the one captured graph reproduces the eager iterations: 2 eager, then
    capture + replays, at the existing replay tolerance."""
    from txt2vid_amd.gan.trainer import TrainStep, GraphedTrainStep
    tokens = tokens_for(B).to(DEV)

    def batches():
        g = torch.Generator()
        g.manual_seed(12)
        return [(torch.rand(B, 1, 16, 64, 64, generator=g) * 2 - 1).to(DEV) for _ in range(4)]
    gan, optD, optG, losses, prm = make()
    seed(6)
    eager = []
    for x in batches():
        cond = gan.cond_encoder.encode(tokens, [8] * B)[2].detach()
        lD, lG, _, _ = TrainStep(gan, optD, optG, losses, prm, DEV).run(x, cond)
        eager.append((float(lD), float(lG)))
    w_eager = gan.discrims[0].single_discrim.module.proj.weight.detach().clone()
    gan, optD, optG, losses, prm = make()
    w0 = gan.discrims[0].single_discrim.module.proj.weight.detach().clone()
    seed(6)
    gs = GraphedTrainStep(gan, optD, optG, losses, prm, DEV, (B, 1, 16, 64, 64), warmup=2, cond_dim=256)
    for i, x in enumerate(batches()):
        cond = gan.cond_encoder.encode(tokens, [8] * B)[2].detach()
        lD, lG = gs.step(x, cond)
        got = (float(lD), float(lG))
        print('proj step %d (%s): %s vs eager %s' % (i, 'replay' if i >= 2 else 'eager', got, eager[i]))
        tol = 2e-5 if i < 2 else 2e-3
        assert all(abs(a - b) < tol for a, b in zip(got, eager[i])), (i, got, eager[i])
    assert gs.graphs is not None and gs.n_graphs == 1
    w = gan.discrims[0].single_discrim.module.proj.weight.detach()
    moved = float((w_eager - w0).norm())
    assert moved > 0 and float((w - w_eager).norm()) < 2e-2 * moved


def test_proj_end2end_encoder_gradient_vs_wrapped_oracle(monkeypatch):
    """--end2end: the sentence code keeps its graph and reaches the loss through the projection term as well (the cond role and
    the s-adjoints are live). One iteration: both losses and the encoder's gradient norms left by the G step, bounds of the cBN
    --end2end test."""
    from txt2vid_amd.gan.trainer import train_iteration
    from txt2vid_amd.optim import Adam
    gan, _, _, losses, prm = make()
    txt = gan.cond_encoder.differentiable(True)
    dis, gen = gan.discrims[0], gan.gen
    optD = Adam([{'params': dis.parameters()}, {'params': txt.parameters()}], lr=2e-4, betas=(0.5, 0.999))
    optG = Adam([{'params': gen.parameters()}, {'params': txt.parameters()}], lr=2e-4, betas=(0.5, 0.999))
    PG, _, _, _ = S.oracle_states(dict(cond=True))
    PD, PT = PJ.discrim_state()
    tr = O.OracleTrainer(PG, PD, d_prefix=PRE, end2end_txt=PT)
    tokens, lengths = tokens_for(B, 5), [8] * B
    seed(31)
    x = (torch.rand(B, 16, 1, 64, 64) * 2 - 1).permute(0, 2, 1, 3, 4).contiguous()
    state = (torch.get_rng_state(), np.random.get_state(), random.getstate())
    cond = txt.encode(tokens.to(DEV), lengths)[2]
    assert cond.requires_grad
    box = {}
    calls = _trace(monkeypatch, lambda: box.update(r=train_iteration(gan, x.to(DEV), cond, optD, optG, losses, prm, DEV, end2end=True)))
    lD, lG = float(box['r'][0]), float(box['r'][1])
    assert _proj_calls(calls).get('t2v_proj_cond', 0) > 0
    torch.set_rng_state(state[0])
    np.random.set_state(state[1])
    random.setstate(state[2])
    with monkeypatch.context() as mp:
        PJ.patch(mp)
        lDo, lGo = tr.step_end2end(x, tokens, lengths)
    print('proj end2end: HIP lossD %.6f lossG %.6f | oracle %.6f %.6f' % (lD, lG, lDo, lGo))
    assert abs(lD - lDo) < 1e-3 and abs(lG - lGo) < 1e-3
    named = dict(txt.encoder.named_parameters())
    ref_max = max(float(PT[k].grad.norm()) for k in tr.t_params)
    for k in tr.t_params:
        got, want = float(named[k[len('encoder.'):]].grad.norm()), float(PT[k].grad.norm())
        assert abs(got - want) <= 1e-2 * want + 1e-5 * ref_max, (k, got, want)


# ------------------------------------------------------------------------------------------------ launch budget

D_STEP_CALLS = {'t2v_proj_rows': 2, 't2v_proj_feat': 3, 't2v_proj_weight': 3}
G_STEP_CALLS = {'t2v_proj_rows': 1, 't2v_proj_feat': 1}


def test_launch_budget(monkeypatch):
    """What DESIGN states. A D step with the gradient penalty: rows for the 8 members of the lock-step pass and for the 4
    mismatched-caption heads; feat in the penalty's sweep and in the adjoints of the two rows launches; weight in those two
    adjoints and in the sweep's second backward — and nothing else of the family (no cond role without --end2end). A G step:
    one rows, one feat. proj=False: no t2v_proj_* call at all, and every other call count is the same as with proj=True except
    one grouped add (`t2v_multi`) behind the fork of the heads' features per backward through a heads launch: the sweep, the
    real||fake heads and the mismatched-caption heads in a D step (3), the generated half's heads in a G step (1)."""
    from txt2vid_amd import functional as TF
    from txt2vid_amd.gan.trainer import TrainStep
    tokens = tokens_for(B)
    out = {}
    for proj in (True, False):
        gan, optD, optG, losses, prm = make(proj=proj)
        with torch.no_grad():
            cond = gan.cond_encoder.encode(tokens.to(DEV), [8] * B)[2].detach()
        seed(3)
        x = S.batch().to(DEV)
        step = TrainStep(gan, optD, optG, losses, prm, DEV)
        step.run(x, cond)                                           # (first call fills the packed-weight and constant caches)
        seed(4)
        d = _trace(monkeypatch, lambda: step.part(0, x, cond))      # pyramid, G forward, the D step
        g = _trace(monkeypatch, lambda: step.part(1))               # D's update, the (fused) G step
        step.part(2)
        out[proj] = (d, g)
        TF.set_grad_sink(None)
    print('proj launch budget: D step %s | G step %s' % (_proj_calls(out[True][0]), _proj_calls(out[True][1])))
    assert _proj_calls(out[True][0]) == D_STEP_CALLS
    assert _proj_calls(out[True][1]) == G_STEP_CALLS
    assert _proj_calls(out[False][0]) == {} and _proj_calls(out[False][1]) == {}
    for k in (0, 1):
        on = Counter(c for c in out[True][k] if not c.startswith('t2v_proj_'))
        off = Counter(out[False][k])
        extra = on - off
        print('proj launch budget: other calls added in the %s step: %s' % ('DG'[k], dict(extra)))
        assert not (off - on) and dict(extra) == {'t2v_multi': (3, 1)[k]}, dict(extra)


# ------------------------------------------------------------------------------------------------ command line

def _cli(args, tmp, ok=True):
    cfg = os.path.join(str(tmp), 'synth.json')
    with open(os.path.join(ROOT, 'tools', 'cfg', 'synth.json')) as f:
        spec = json.load(f)
    with open(cfg, 'w') as f:
        json.dump(spec, f)
    cmd = ['timeout', '-k', '10', '600', sys.executable, '-m', 'txt2vid_amd.train.gan', '--data', cfg] + args
    p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=700)
    out = p.stdout.decode(errors='replace')
    assert (p.returncode == 0) == ok, out[-3000:]
    return out


def test_proj_cli_train_checkpoint_resume_and_mismatch(tmp_path):
    out_dir, smp = str(tmp_path / 'out'), str(tmp_path / 'samples')
    spec = os.path.join(ROOT, 'tools', 'cfg', 'discrim_cond_proj.json')
    base = ['--num_channels', '1', '--cuda', '--frame_sizes', '8', '16', '32', '64', '--D_names', 'video', '--G_lr', '0.0002',
            '--D_lr', '0.0002', '--D_beta1', '0.5', '--D_beta2', '.999', '--G_beta1', '0.5', '--G_beta2', '.999',
            '--D_loss', 'txt2vid.gan.losses.RSGANLoss', '--init_method', 'xavier', '--seed', '100', '--gp_lambda', '.5',
            '--subsample_input', '--workers', '0', '--log_period', '1',
            '--G', 'txt2vid.models.tganv2_cond.gen.MultiScaleGen', '--D', spec,
            '--sent', 'txt2vid.models.txt.basic.Seq2Seq', '--batch_size', '8', '--epochs', '1', '--out', out_dir]
    log = _cli(base + ['--out_samples', smp, '--max_iters', '3', '--save_model_period', '3', '--save_example_period', '0'], tmp_path)
    assert 'Iter 3, Loss_D' in log
    ck = glob.glob(os.path.join(out_dir, 'iter_3_lossG_*'))
    assert len(ck) == 1
    sd = torch.load(ck[0], map_location='cpu', weights_only=False)
    Vw = sd['video'][PRE + 'proj.weight']
    assert tuple(Vw.shape) == (1024, 256) and list(sd['video'])[-1] == PRE + 'proj.weight'
    assert float(Vw.abs().max()) > 0                                 # zeros at initialisation, moved by the optimiser
    log2 = _cli(base + ['--out_samples', smp, '--max_iters', '2', '--weights', ck[0], '--save_model_period', '1000',
                        '--save_example_period', '0'], tmp_path)
    assert 'Iter 2, Loss_D' in log2
    # the same checkpoint without the spec: refused with a message that names proj
    plain = [a if a != spec else 'txt2vid.models.tganv2_cond.discrim.MultiScaleDiscrim' for a in base]
    log3 = _cli(plain + ['--out_samples', smp, '--max_iters', '1', '--weights', ck[0], '--save_model_period', '1000',
                         '--save_example_period', '0'], tmp_path, ok=False)
    assert 'proj' in log3 and 'projection head' in log3
