"""GPU: the discriminator's opt-in minibatch standard deviation head (Resnet3D(mbstd=G); DESIGN "Minibatch standard deviation") on
the HIP path, against the float64 / plain-torch restatement of tests/mbstd_cases.py, alone and composed with the oracle: the four
`t2v_mbstd_*` roles through their autograd surface up to the second order (metric of mbstd_cases, 1e-4 of the field's size), the
raw ABI on guarded buffers, the module (text-conditioned together with proj, and unconditional), the fused D and G step losses,
three training iterations, graph replay, the launch budget and the command line."""
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

import mbstd_cases as MB
import schedule_cases as S
from oracle import tganv2_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, B = S.V, S.B
KINDS = ['cond_proj', 'uncond']                     # text-conditioned with proj and mbstd together; unconditional


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


def _mb_calls(calls):
    return dict(Counter(c for c in calls if c.startswith('t2v_mbstd_')))


# ------------------------------------------------------------------------------------------------ op level: the autograd surface

def leaves(case, w_=None):
    inp = MB.inputs(case)
    dev = lambda t: t.to(DEV).requires_grad_(True)
    wd = torch.nn.Parameter((inp['w'] if w_ is None else w_).to(DEV))
    return [dev(t) for t in inp['f']], wd, [dev(t) for t in inp['base']], [t.to(DEV) for t in inp['r']], [t.to(DEV) for t in inp['t']]


def apply_op(case, fs, wd, bases):
    """[y [b, H] per member] through ONE forward launch: every head's [b, 1] logits go in, and come out with the term."""
    from txt2vid_amd import functional as TF
    _, _, K, G, H = MB.CASES[case]
    per_head = [[b_[:, h:h + 1] for b_ in bases] for h in range(H)]
    res = TF.mbstd_group(wd, G, fs, per_head, MB.segs_of(case))
    return [torch.cat([res[h][i] for h in range(H)], 1) for i in range(len(fs))]


def run_op(case, w_=None, second=True):
    fs, wd, bases, rs, ts = leaves(case, w_)
    return MB.fields_of(apply_op(case, fs, wd, bases), fs, wd, bases, rs, ts, second)


@pytest.mark.parametrize('case', list(MB.CASES))
def test_forward_first_and_second_order(case):
    MB.check(case, run_op(case), MB.case_reference(case), MB.FIELDS)


@pytest.mark.parametrize('case', list(MB.CASES))
def test_zero_w_returns_base_and_still_gets_its_gradient(case):
    inp = MB.inputs(case)
    zero = torch.zeros_like(inp['w'])
    got = run_op(case, zero, second=False)
    ref = MB.reference(case, w=zero)
    assert torch.equal(got['y'].cpu(), torch.cat(inp['base'], 0))
    assert not got['gf'].any()                                        # exact zeros
    MB.check(case + '/zero-w', got, ref, MB.FIRST)
    assert float(ref['gw'].abs().max()) > 0


def test_a_member_without_gradient_is_left_out(monkeypatch):
    """Members 1 and 3 of the pyramid case take no part in the loss: their inputs get no gradient, the launches run over two
    members, the others' gradients are bitwise those of the full run, and dL/dw is the sum over the two."""
    full = run_op('pyramid', second=False)
    fs, wd, bases, rs, ts = leaves('pyramid')
    ys = apply_op('pyramid', fs, wd, bases)
    loss = sum((ys[i] * rs[i]).sum() for i in (0, 2))
    box = {}
    calls = _trace(monkeypatch, lambda: box.update(g=torch.autograd.grad(loss, fs + [wd] + bases, allow_unused=True)))
    g = box['g']
    assert _mb_calls(calls) == {'t2v_mbstd_feat': 1, 't2v_mbstd_weight': 1}
    n, (bs, _, K, G, H) = 4, MB.CASES['pyramid']
    rows = np.cumsum([0] + bs)
    for i in range(n):
        for grads, field in ((g[:n], 'gf'), (g[n + 1:], 'gbase')):
            if i in (1, 3):
                assert grads[i] is None or not grads[i].any()
            else:
                assert torch.equal(grads[i], full[field][rows[i]:rows[i + 1]]), (i, field)
        if i in (1, 3):
            assert g[i] is None
    inp = MB.inputs('pyramid')
    want = sum((inp['r'][i].double() * MB.stat(inp['f'][i].double(), G)).sum(0) for i in (0, 2))
    assert MB.ratio(g[n], want) <= 1.0


def test_frozen_w_and_input_grads_only_issue_no_weight_call(monkeypatch):
    from txt2vid_amd import functional as TF
    fs, wd, bases, rs, ts = leaves('eight')

    def sweep():
        ys = apply_op('eight', fs, wd, bases)
        with TF.input_grads_only():
            torch.autograd.grad(sum(y.sum() for y in ys), fs)
    assert _mb_calls(_trace(monkeypatch, sweep)) == {'t2v_mbstd_fwd': 1, 't2v_mbstd_feat': 1}
    wd.requires_grad_(False)

    def frozen():
        ys = apply_op('eight', fs, wd, bases)
        sum((y * r).sum() for y, r in zip(ys, rs)).backward()
    assert _mb_calls(_trace(monkeypatch, frozen)) == {'t2v_mbstd_fwd': 1, 't2v_mbstd_feat': 1}
    assert wd.grad is None and all(f.grad is not None for f in fs)


def test_the_second_backward_is_two_launches_and_the_third_order_raises(monkeypatch):
    """What the penalty does: a recorded sweep (feat), then a backward through it (second + the weight role with t). Asking for a
    graph of THAT backward and differentiating it raises: no silent None."""
    from txt2vid_amd import functional as TF
    fs, wd, bases, rs, ts = leaves('odd')
    K = MB.CASES['odd'][2]
    ys = apply_op('odd', fs, wd, bases)
    with TF.input_grads_only():
        dfs = torch.autograd.grad(sum(y.sum() for y in ys), fs, create_graph=True)
    pen = K * sum((d * t).sum() for d, t in zip(dfs, ts))
    calls = _trace(monkeypatch, lambda: pen.backward(retain_graph=True))
    assert _mb_calls(calls) == {'t2v_mbstd_second': 1, 't2v_mbstd_weight': 1}
    (h,) = torch.autograd.grad(pen, fs, create_graph=True)
    assert h.requires_grad
    with pytest.raises(RuntimeError, match='no backward'):
        torch.autograd.grad(h.sum(), fs)


@pytest.mark.parametrize('case', ['real', 'eight', 'whole'])
def test_two_runs_give_the_same_bits(case):
    a, b = run_op(case), run_op(case)
    for f in MB.FIELDS:
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


@pytest.mark.parametrize('case', ['one', 'odd', 'pyramid', 'eight', 'halves'])
def test_raw_abi_on_guarded_buffers(case):
    """The four entry points with no Python caller: fwd, feat and weight with g = r give y, gf and gw (written, then accumulated
    onto 0.5); second with Γ = K·t and g = 1 gives hf − gf, and weight on its t gives hw − gw; nothing written outside any buffer."""
    from txt2vid_amd._lib import lib, MbstdMember
    from txt2vid_amd._ops import _stream
    L, st = lib(), _stream()
    inp = MB.inputs(case)
    bs, _, K, G, H = MB.CASES[case]
    segs = MB.segs_of(case)
    n = len(bs)
    f = [t.to(DEV).contiguous() for t in inp['f']]
    gam = [(K * t).to(DEV).contiguous() for t in inp['t']]
    col = lambda ts: [[t[:, h].to(DEV).contiguous() for t in ts] for h in range(H)]
    r, base = col(inp['r']), col(inp['base'])
    ones = [torch.ones(b, device=DEV) for b in bs]
    wd = inp['w'].to(DEV).contiguous()
    guards = []

    def out(k, init=None):
        guards.append(Guarded(k, init))
        return guards[-1]

    def table(g=None, base_=None, gam_=None, y=None, stat=None, out_=None):
        arr = (MbstdMember * n)()
        for i, a in enumerate(arr):
            a.f, a.b, a.seg = f[i].data_ptr(), bs[i], segs[i]
            for h in range(H):
                a.g[h] = g[h][i].data_ptr() if g is not None else None
                a.base[h] = base_[h][i].data_ptr() if base_ is not None else None
                a.y[h] = y[h][i].p if y is not None else None
            a.gam = gam_[i].data_ptr() if gam_ is not None else None
            a.stat = (stat[i].p if isinstance(stat[i], Guarded) else stat[i].data_ptr()) if stat is not None else None
            a.out = out_[i].p if out_ is not None else None
        return arr
    wp = C.c_void_p(wd.data_ptr())
    ys, y0 = [[out(b) for b in bs] for _ in range(H)], [[out(b) for b in bs] for _ in range(H)]
    s1, t2, yt = [out(b) for b in bs], [out(b) for b in bs], [[out(b) for b in bs] for _ in range(H)]
    Fs, Hs = [out(b * K) for b in bs], [out(b * K) for b in bs]
    W, W2, Wt = out(H), out(H, torch.full((H,), 0.5)), out(H)
    assert L.t2v_mbstd_fwd(table(base_=base, y=ys, stat=s1), n, wp, H, K, G, st) == 0
    assert L.t2v_mbstd_fwd(table(y=y0), n, wp, H, K, G, st) == 0                       # no base, no stat
    assert L.t2v_mbstd_feat(table(g=r, out_=Fs), n, wp, H, K, G, st) == 0
    assert L.t2v_mbstd_weight(table(g=r, stat=s1), n, C.c_void_p(W.p), H, K, G, 0, st) == 0
    assert L.t2v_mbstd_weight(table(g=r, stat=s1), n, C.c_void_p(W2.p), H, K, G, 1, st) == 0
    one_g = [ones] * H
    assert L.t2v_mbstd_second(table(g=one_g, gam_=gam, y=yt, stat=t2, out_=Hs), n, wp, H, K, G, st) == 0
    assert L.t2v_mbstd_weight(table(g=one_g, stat=t2), n, C.c_void_p(Wt.p), H, K, G, 0, st) == 0
    torch.cuda.synchronize()
    assert all(g.intact() for g in guards), [i for i, g in enumerate(guards) if not g.intact()]
    ref = MB.case_reference(case)
    rows = lambda gs: torch.cat([torch.stack([gs[h][i].t for h in range(H)], 1) for i in range(n)], 0)
    s64 = torch.cat([MB.stat(t.double(), G, seg) for t, seg in zip(inp['f'], segs)], 0)
    w64 = inp['w'].double().view(1, -1)
    tq = torch.cat([g.t for g in t2]).view(-1, 1).double().cpu()
    got = {'y': rows(ys), 'y0': rows(y0), 'stat': torch.cat([g.t for g in s1]).view(-1, 1),
           'gf': torch.cat([g.t.view(b, K) for g, b in zip(Fs, bs)], 0), 'gw': W.t, 'gw2': W2.t,
           'hf-gf': torch.cat([g.t.view(b, K) for g, b in zip(Hs, bs)], 0), 'hw-gw': Wt.t, 'w·t': rows(yt)}
    want = dict(ref, y0=s64 * w64, stat=s64, gw2=ref['gw'] + 0.5)
    want['hf-gf'], want['hw-gw'] = ref['hf'] - ref['gf'], ref['hw'] - ref['gw']
    want['w·t'] = tq * w64                                                            # (t itself is pinned by hw − gw)
    MB.check(case + '/abi', got, want, ['y', 'y0', 'stat', 'gf', 'gw', 'gw2', 'hf-gf', 'hw-gw', 'w·t'])


def test_entry_points_refuse_bad_arguments_and_launch_nothing():
    """Real device pointers, bad arguments: T2V_EINVAL (a launch would return 0 or a HIP status) and the buffers keep their
    pattern."""
    from txt2vid_amd._lib import lib, MbstdMember, MAX_GROUPS
    L = lib()
    buf = torch.full((4096,), 3.5, device=DEV)
    p = buf.data_ptr()

    def members(n=1, b=4, seg=4, **null):
        arr = (MbstdMember * max(n, 1))()
        for a in arr:
            a.f, a.gam, a.stat, a.out, a.b, a.seg = p, p, p, p, b, seg
            for h in range(2):
                a.g[h], a.base[h], a.y[h] = p, p, p
            for k in null:
                if k in ('g', 'base', 'y'):
                    getattr(a, k)[0] = getattr(a, k)[1] = None
                else:
                    setattr(a, k, None)
        return arr
    w = C.c_void_p(p)
    roles = {'fwd': L.t2v_mbstd_fwd, 'feat': L.t2v_mbstd_feat, 'second': L.t2v_mbstd_second,
             'weight': lambda m, n, v, H, K, G, st: L.t2v_mbstd_weight(m, n, v, H, K, G, 0, st)}
    for name, fn in roles.items():
        assert fn(None, 1, w, 2, 8, 4, None) == -1 and fn(members(), 1, None, 2, 8, 4, None) == -1, name
        assert fn(members(), 0, w, 2, 8, 4, None) == -1 and fn(members(MAX_GROUPS + 1), MAX_GROUPS + 1, w, 2, 8, 4, None) == -1, name
        assert fn(members(), 1, w, 2, 0, 4, None) == -1 and fn(members(b=0, seg=1), 1, w, 2, 8, 4, None) == -1, name
        assert fn(members(seg=0), 1, w, 2, 8, 4, None) == -1 and fn(members(b=4, seg=3), 1, w, 2, 8, 4, None) == -1, name
        assert all(fn(members(), 1, w, 2, 8, G, None) == -1 for G in (1, 0, 17)), name
        assert all(fn(members(), 1, w, H, 8, 4, None) == -1 for H in (0, 3)), name
    for name, reads in (('fwd', ('f', 'y')), ('feat', ('f', 'g', 'out')), ('second', ('f', 'gam', 'g')), ('weight', ('g', 'stat'))):
        for k in reads:
            assert roles[name](members(**{k: None}), 1, w, 2, 8, 4, None) == -1, (name, k)
    torch.cuda.synchronize()
    assert bool((buf == 3.5).all())


def test_symbols_are_exported_and_declared():
    from txt2vid_amd import _lib
    names = ['t2v_mbstd_fwd', 't2v_mbstd_feat', 't2v_mbstd_second', 't2v_mbstd_weight']
    header = open(os.path.join(ROOT, 'include', 't2v_hip.h')).read()
    assert [k for k in _lib.SIGNATURES if k.startswith('t2v_mbstd_')] == names          # at most four entry points
    for name in names:
        assert hasattr(_lib.lib(), name) and ('int %s(' % name) in header


# ------------------------------------------------------------------------------------------------ module level

def pour(module, PD=None):
    sd = {k: O.recipe_tensor(k, v.shape) for k, v in module.state_dict().items()}
    for k in sd:
        if PD is not None and k.endswith('mbstd.weight'):
            sd[k] = PD[k].detach().clone()
    module.load_state_dict(sd)
    return module.to(DEV)


def _discrim(kind, on=True):
    kw = dict(mbstd=MB.GROUP) if on else {}
    if kind == 'uncond':
        from txt2vid_amd.models.tganv2.discrim import MultiScaleDiscrim
        return MultiScaleDiscrim(num_channels=1, **kw)
    from txt2vid_amd.models.tganv2_cond.discrim import MultiScaleDiscrim
    return MultiScaleDiscrim(num_channels=1, cond_dim=256, proj=True, **kw)


def _state(kind, zero=False):
    """(PD, PT, prefix, cond, proj) of the oracle for one kind. The recipe V of `pour` is the one `discrim_state` holds."""
    cond = kind != 'uncond'
    PD, PT = MB.discrim_state(cond, proj=cond, zero=zero)
    return PD, PT, MB.prefix(cond), cond, cond


def _trunk(dis):
    return getattr(dis.single_discrim, 'module', dis.single_discrim)


def tokens_for(batch, s=77):
    tg = torch.Generator()
    tg.manual_seed(s)
    t = torch.randint(4, V, (batch, 8), generator=tg)
    t[:, 0], t[:, -1] = 1, 2
    return t


def pyramid(s=3):
    """Clips and sentence codes of the ceil-halved pyramid of B = 4 at 64x64, C = 1 (CPU): 4, 2, 1, 1 rows."""
    g = torch.Generator()
    g.manual_seed(s)
    x = (torch.rand(B, 16, 1, 64, 64, generator=g) * 2 - 1).permute(0, 2, 1, 3, 4).contiguous()
    c = 0.1 * torch.randn(B, 256, generator=g)
    xs, conds, _ = O.multiscale_data(x, c, S.FS)
    assert [t.shape[0] for t in xs] == [4, 2, 1, 1] and xs[0].shape[0] % MB.GROUP != 0
    return [t.contiguous() for t in xs], [t.contiguous() for t in conds]


@pytest.mark.parametrize('kind', KINDS)
def test_fresh_mbstd_discriminator_is_the_plain_one(kind):
    """w = 0: on the same weights and inputs (u, c, feat) are those of the mbstd=0 discriminator — bitwise, as `base + 0·s` —
    through the grouped pass and through the single-tensor forward."""
    off, on = pour(_discrim(kind, False)).train(), pour(_discrim(kind), _state(kind, zero=True)[0]).train()
    assert not _trunk(on).mbstd.weight.any() and not hasattr(_trunk(off), 'mbstd')
    xs, conds = pyramid()
    xs = [t.to(DEV) for t in xs]
    conds = [t.to(DEV) for t in conds] if kind != 'uncond' else None
    with torch.no_grad():
        a, b = off(x=xs, cond=conds), on(x=xs, cond=conds)
        c1 = None if conds is None else conds[1]
        a1, b1 = off.sub_discrims[0](xs[1], cond=c1), on.sub_discrims[0](xs[1], cond=c1)
    for (u0, c0, f0), (u1, c1, f1) in list(zip(a, b)) + [(a1, b1)]:
        assert torch.equal(u0, u1) and torch.equal(f0, f1) and (c0 is None and c1 is None or torch.equal(c0, c1))


def _oracle_params(PD):
    keys = [k for k, v in PD.items() if v.dtype.is_floating_point]
    for k in keys:
        PD[k].requires_grad_(True)
    return keys


def _norms_close(grads, PD, keys, tag, rtol=3e-3):
    """`grads`: key -> dL/dparameter on the device, against the oracle state's .grad; dL/dw element by element."""
    got = np.array([float(grads[k].double().norm()) for k in keys])
    want = np.array([float(PD[k].grad.double().norm()) for k in keys])
    rel = float(np.linalg.norm(got - want) / np.linalg.norm(want))
    print('mbstd %s: gradient-norm vector rel %.3g; dw %s (%s)' % (tag, rel, grads[keys[-1]].tolist(), PD[keys[-1]].grad.tolist()))
    assert rel < rtol, rel
    assert keys[-1].endswith('mbstd.weight') and want[-1] > 0
    a, b = grads[keys[-1]].cpu().double(), PD[keys[-1]].grad.double()
    assert float((a - b).norm() / b.norm()) < rtol


@pytest.mark.parametrize('kind', KINDS)
def test_forward_levels_vs_wrapped_oracle(kind, monkeypatch):
    """One grouped pass over the pyramid with the recipe w: logits and features, the gradients of a fixed weighted sum of the
    logits with respect to every parameter and to the clips, against `oracle.multiscale_discrim` with the wrapped trunk. Bounds of
    test_proj_gpu's module test: rtol 2e-3, atol 5e-4 x scale on the outputs; 3e-3 on the gradient norms. The per-member fallback
    computes the same logits."""
    PD, _, pre, cond, proj = _state(kind)
    dis = pour(_discrim(kind), PD).train()
    keys = _oracle_params(PD)
    assert [k for k, _ in dis.named_parameters()] == keys
    xs, conds = pyramid()
    if not cond:
        conds = None
    g = torch.Generator()
    g.manual_seed(9)
    wu, wc = [torch.randn(x.shape[0], 1, generator=g) for x in xs], [torch.randn(x.shape[0], 1, generator=g) for x in xs]
    xd = [t.to(DEV).requires_grad_(True) for t in xs]
    cd = [t.to(DEV) for t in conds] if cond else None
    res = dis(x=xd, cond=cd)
    tot = lambda rs, dev: sum((u * a.to(dev)).sum() + ((c * b.to(dev)).sum() if c is not None else 0) for (u, c, _), a, b in zip(rs, wu, wc))
    tot(res, DEV).backward()
    xo = [t.clone().requires_grad_(True) for t in xs]
    with monkeypatch.context() as mp:
        MB.patch(mp, MB.GROUP, proj)
        ro = O.multiscale_discrim(PD, xo, conds, pre)
    tot(ro, 'cpu').backward()
    w = PD[pre + 'mbstd.weight'].detach()
    for lvl, ((u, c, f), (uo, co, fo)) in enumerate(zip(res, ro)):
        for a, b in ((u, uo), (c, co), (f, fo)):
            if b is None:
                assert a is None
                continue
            scale = max(1.0, float(b.abs().max()))
            np.testing.assert_allclose(a.detach().cpu().numpy(), b.detach().numpy(), rtol=2e-3, atol=5e-4 * scale)
        if fo.shape[0] > 1:
            # the term cannot hide below the tolerance: on the levels with a group of more than one row it is of the size of the
            # logit it is added to (a single-row level's statistic is sqrt(eps), with no gradient)
            s = MB.stat(fo.detach(), MB.GROUP)
            for h, lo in enumerate((uo, co)[:w.numel()]):
                term = float((w[h] * s).abs().mean())
                rest = float((lo.detach() - w[h] * s).abs().mean())
                print('mbstd %s level %d head %d: term %.4g next to %.4g' % (kind, lvl, h, term, rest))
                assert 0.1 < term / rest < 10, (lvl, h, term, rest)
    _norms_close({k: p.grad for k, p in dis.named_parameters()}, PD, keys, 'forward_levels/' + kind)
    for a, b in zip(xd, xo):
        assert float((a.grad.cpu().double() - b.grad.double()).norm() / b.grad.double().norm()) < 3e-3
    # grouped heads against the per-member fallback (computed_features) on the same features
    trunk = _trunk(dis)
    if cond:
        feats = [f.detach() for _, _, f in res]
        with torch.no_grad():
            grouped = trunk.cond_heads(feats, cd)
            single = [trunk(cond=c_, computed_features=f_)[1] for f_, c_ in zip(feats, cd)]
            one = [trunk._cond_head(f_, c_) for f_, c_ in zip(feats, cd)]
        for a, b, o, (_, c, _) in zip(grouped, single, one, res):
            assert torch.equal(a, b) and torch.equal(a, o) and torch.equal(a, c.detach())
    with torch.no_grad():
        for i in (0, 1):
            u1, c1, f1 = trunk(xd[i].detach(), cond=cd[i] if cond else None)        # the single-tensor forward: one segment
            close = lambda a, b: torch.allclose(a, b.detach(), rtol=2e-3, atol=5e-4)
            assert close(u1, res[i][0]) and close(f1, res[i][2]) and (c1 is None and not cond or close(c1, res[i][1]))


def make(kind, on=True, zero=False):
    from txt2vid_amd.gan.cond_gan import CondGan
    from txt2vid_amd.gan.losses import MixedGanLoss, RSGANLoss
    from txt2vid_amd.optim import Adam
    txt = None
    if kind == 'uncond':
        from txt2vid_amd.models.tganv2.gen import MultiScaleGen
        gen = pour(MultiScaleGen(width=64, height=64, num_channels=1)).train()
    else:
        from txt2vid_amd.models.tganv2_cond.gen import MultiScaleGen
        from txt2vid_amd.models.txt.basic import Seq2Seq
        gen = pour(MultiScaleGen(width=64, height=64, num_channels=1, cond_dim=256)).train()
        txt = Seq2Seq(vocab_size=V)
        txt.load_state_dict({k: O.recipe_tensor(k if k.startswith('encoder.') else 'encoder.' + k[len('decoder.'):], v.shape)
                             for k, v in txt.state_dict().items()})
        txt.to(DEV)
    dis = pour(_discrim(kind, on), _state(kind, zero)[0]).train()
    gan = CondGan(gen=gen, discrims=[dis], cond_encoder=txt, discrim_names=['video'])
    optD = Adam([{'params': dis.parameters()}], lr=2e-4, betas=(0.5, 0.999))
    optG = Adam([{'params': gen.parameters()}], lr=2e-4, betas=(0.5, 0.999))
    prm = S.params_for(dict(N=1, M=1, gp=0.5, mean_d=False, mean_g=False))
    return gan, optD, optG, MixedGanLoss(g_loss=RSGANLoss(), d_loss=RSGANLoss()), prm


def code(gan, tokens):
    if gan.cond_encoder is None:
        return None
    with torch.no_grad():
        return gan.cond_encoder.encode(tokens.to(DEV), [8] * B)[2].detach()


@pytest.mark.parametrize('kind', KINDS)
def test_fused_d_and_g_step_losses_and_gradient_norms_vs_wrapped_oracle(kind, monkeypatch):
    """One fused D step with the gradient penalty (lambda 0.5: real‖fake members with seg = b, the mismatched-caption heads on the
    real rows, the sweep and the second backward through the head) and one G step, recipe w, against `oracle.discrim_loss` /
    `gen_loss` with the wrapped trunk — which calls it on the real and on the generated batch apart — on the same draws: losses
    within 1e-3 x max(1, |ref|), every gradient-norm vector within 3e-3, dL/dw element by element (test_proj_gpu's bounds). A
    group that straddled the real‖fake boundary would change the statistic of every level."""
    from txt2vid_amd import functional as TF
    from txt2vid_amd.gan.trainer import multiscale_data
    gan, optD, optG, losses, prm = make(kind)
    dis, gen = gan.discrims[0], gan.gen
    TF.set_grad_sink(None)
    PD, PT, pre, cond, proj = _state(kind)
    PG, _, _, _ = S.oracle_states(dict(cond=cond))
    d_keys = _oracle_params(PD)
    g_keys = [k for k, v in PG.items() if v.dtype.is_floating_point and 'running_' not in k]
    for k in g_keys:
        PG[k].requires_grad_(True)
    seed(7)
    x = S.batch()
    tokens = tokens_for(B)
    cnd = code(gan, tokens)
    state = (torch.get_rng_state(), np.random.get_state(), random.getstate())
    xs, conds = multiscale_data(x.to(DEV), cnd, prm.frame_sizes, True)          # (draws the sub-sampling phases of the pyramid)
    z = torch.randn(B, 256)
    fake = gan(z.to(DEV), cond=conds[0]) if cond else gan(z.to(DEV))
    lD = gan.discrim_step(real=xs, fake=[f.detach() for f in fake], cond=conds if cond else None, loss=losses.discrim_loss, gp_lambda=0.5)
    lD.backward()
    TF.grad_sink_flush()
    with torch.no_grad():
        _, _, real_pred = gan.all_discrim_forward(real=xs, cond=conds if cond else None, fake=None, loss=None)
    d_grads = {k: p.grad.detach().clone() for k, p in dis.named_parameters()}
    lG = gan.gen_step(fake=fake, real_pred=real_pred, cond=conds if cond else None, loss=losses.gen_loss)
    lG.backward()
    TF.grad_sink_flush()
    torch.cuda.synchronize()
    torch.set_rng_state(state[0])
    np.random.set_state(state[1])
    random.setstate(state[2])
    co = None
    if cond:
        with torch.no_grad():
            co = O.text_encode(PT, tokens, [8] * B)
    xo, cso, _ = O.multiscale_data(x, co, S.FS)
    assert torch.equal(torch.randn(B, 256), z)                                    # the same draws in the same order
    with monkeypatch.context() as mp:
        MB.patch(mp, MB.GROUP, proj)
        fo = O.multiscale_gen(PG, z, cso[0] if cond else None, training=True)
        fcs = None
        if cond:
            fc0 = cso[0][O.gen_perm(B)]
            fcs = [fc0[0:cc.size(0)] for cc in cso]
        lDo = O.discrim_loss(PD, pre, xo, [f.detach() for f in fo], cso if cond else None, fcs, 0.5)
        lDo.backward()
        _norms_close(d_grads, PD, d_keys, 'D step/' + kind)
        with torch.no_grad():
            if cond:
                O.gen_perm(B)
                rp = O.multiscale_discrim(PD, xo, cso, pre)
            else:
                rp = [r[0] for r in O.multiscale_discrim(PD, xo, None, pre)]
        lGo = O.gen_loss(PD, pre, fo, rp, cso if cond else None)
        lGo.backward()
    print('mbstd %s: lossD %.6f (%.6f) lossG %.6f (%.6f)' % (kind, float(lD), float(lDo), float(lG), float(lGo)))
    assert abs(float(lD) - float(lDo)) < 1e-3 * max(1.0, abs(float(lDo)))
    assert abs(float(lG) - float(lGo)) < 1e-3 * max(1.0, abs(float(lGo)))
    g_named = dict(gen.named_parameters())
    got = np.array([float(g_named[k].grad.double().norm()) for k in g_keys])
    want = np.array([float(PG[k].grad.double().norm()) for k in g_keys])
    rel = float(np.linalg.norm(got - want) / np.linalg.norm(want))
    print('mbstd %s G step: gradient-norm vector rel %.3g' % (kind, rel))
    assert rel < 3e-3, rel


def test_the_fused_d_step_passes_the_halves_as_segments(monkeypatch):
    """The lock-step pass hands `segs` = b for the real‖fake members (2b rows) and the rows of the interpolates; with mbstd off
    the argument is not passed at all."""
    from txt2vid_amd.gan.trainer import multiscale_data
    seen = {}
    for on in (True, False):
        gan, optD, optG, losses, prm = make('uncond', on)
        dis = gan.discrims[0]
        seed(7)
        xs, _ = multiscale_data(S.batch().to(DEV), None, prm.frame_sizes, True)
        fake = [f.detach() for f in gan(torch.randn(B, 256).to(DEV))]
        orig = type(dis).forward

        def spy(self, *a, **k):
            seen[on] = dict(k)
            return orig(self, *a, **k)
        with monkeypatch.context() as mp:
            mp.setattr(type(dis), 'forward', spy)
            gan.discrim_step(real=xs, fake=fake, cond=None, loss=losses.discrim_loss, gp_lambda=0.5)
    assert seen[True]['segs'] == [4, 2, 1, 1, 4, 2, 1, 1] and [t.shape[0] for t in seen[True]['x']] == [8, 4, 2, 2, 4, 2, 1, 1]
    assert 'segs' not in seen[False]


# ------------------------------------------------------------------------------------------------ iteration level

@pytest.mark.parametrize('kind', KINDS[:1])                  # (the unconditional loop runs through the command line below)
def test_mbstd_iterations_vs_wrapped_oracle(kind, monkeypatch):
    """Three 1:1 iterations from the recipe w against the oracle loop with the wrapped trunk: lossD and lossG at the bounds of
    test_proj_gpu's loop test (1e-3, then 2e-2 in iteration 2: the GAN dynamics are chaotic); the per-key D gradient norms of the
    first D step (1e-2 of the norm + 1e-5 of the largest); w after the first D step."""
    from txt2vid_amd.gan.trainer import TrainStep
    cond = kind != 'uncond'
    tokens = tokens_for(B)
    ref = MB.oracle_loop(monkeypatch, cond, tokens, iters=3, proj=cond)
    gan, optD, optG, losses, prm = make(kind)
    dis = gan.discrims[0]
    seed(100)
    for it in range(3):
        x = S.batch().to(DEV)
        lD, lG, _, _ = TrainStep(gan, optD, optG, losses, prm, DEV).run(x, code(gan, tokens))
        lD, lG = float(lD), float(lG)
        tol = 1e-3 if it < 2 else 2e-2
        print('mbstd %s it %d: lossD %.6f (%.6f) lossG %.6f (%.6f)' % (kind, it, lD, ref['lossD'][it], lG, ref['lossG'][it]))
        assert abs(lD - ref['lossD'][it]) < tol * max(1.0, abs(ref['lossD'][it]))
        assert abs(lG - ref['lossG'][it]) < tol * max(1.0, abs(ref['lossG'][it]))
        if it == 0:
            top = max(ref['D_gn0'].values())
            for k, p in dis.named_parameters():
                got, want = float(p.grad.norm()), ref['D_gn0'][k]
                assert abs(got - want) <= 1e-2 * want + 1e-5 * top, (k, got, want)
            wg, wo = _trunk(dis).mbstd.weight.detach().cpu().double(), ref['w'][0].double()
            assert float((wg - wo).norm() / wo.norm()) < 1e-3


@pytest.mark.parametrize('kind', KINDS)
def test_w_leaves_zero_after_the_first_d_step(kind):
    from txt2vid_amd.gan.trainer import TrainStep
    gan, optD, optG, losses, prm = make(kind, zero=True)
    wp = _trunk(gan.discrims[0]).mbstd.weight
    assert not wp.any()
    seed(100)
    x = S.batch().to(DEV)
    TrainStep(gan, optD, optG, losses, prm, DEV).run(x, code(gan, tokens_for(B)))
    assert float(wp.grad.abs().min()) > 0
    # Adam's first step moves every element with a non-zero gradient by lr
    assert float((wp.detach().abs() - 2e-4).abs().max()) < 1e-6


@pytest.mark.parametrize('kind', KINDS)
def test_mbstd_graph_replay_matches_eager(kind):
    """GraphedTrainStep with the head inside the one captured graph reproduces the eager iterations: 2 eager, then capture +
    replays, at the existing replay tolerance."""
    from txt2vid_amd.gan.trainer import TrainStep, GraphedTrainStep
    tokens = tokens_for(B)

    def batches():
        g = torch.Generator()
        g.manual_seed(12)
        return [(torch.rand(B, 1, 16, 64, 64, generator=g) * 2 - 1).to(DEV) for _ in range(4)]
    gan, optD, optG, losses, prm = make(kind)
    seed(6)
    eager = []
    for x in batches():
        lD, lG, _, _ = TrainStep(gan, optD, optG, losses, prm, DEV).run(x, code(gan, tokens))
        eager.append((float(lD), float(lG)))
    w_eager = _trunk(gan.discrims[0]).mbstd.weight.detach().clone()
    gan, optD, optG, losses, prm = make(kind)
    w0 = _trunk(gan.discrims[0]).mbstd.weight.detach().clone()
    seed(6)
    gs = GraphedTrainStep(gan, optD, optG, losses, prm, DEV, (B, 1, 16, 64, 64), warmup=2, cond_dim=256 if kind != 'uncond' else 0)
    for i, x in enumerate(batches()):
        lD, lG = gs.step(x, code(gan, tokens))
        got = (float(lD), float(lG))
        print('mbstd %s step %d (%s): %s vs eager %s' % (kind, i, 'replay' if i >= 2 else 'eager', got, eager[i]))
        tol = 2e-5 if i < 2 else 2e-3
        assert all(abs(a - b) < tol for a, b in zip(got, eager[i])), (i, got, eager[i])
    assert gs.graphs is not None and gs.n_graphs == 1
    w = _trunk(gan.discrims[0]).mbstd.weight.detach()
    moved = float((w_eager - w0).norm())
    assert moved > 0 and float((w - w_eager).norm()) < 2e-2 * moved


# ------------------------------------------------------------------------------------------------ launch budget

# what DESIGN §26 states, per kind: (D step with the penalty, G step)
BUDGET = {
    'cond_proj': ({'t2v_mbstd_fwd': 2, 't2v_mbstd_feat': 3, 't2v_mbstd_second': 1, 't2v_mbstd_weight': 3},
                  {'t2v_mbstd_fwd': 1, 't2v_mbstd_feat': 1}),
    'uncond': ({'t2v_mbstd_fwd': 1, 't2v_mbstd_feat': 2, 't2v_mbstd_second': 1, 't2v_mbstd_weight': 2},
               {'t2v_mbstd_fwd': 1, 't2v_mbstd_feat': 1}),
}


@pytest.mark.parametrize('kind', KINDS)
def test_launch_budget(kind, monkeypatch):
    """A D step with the gradient penalty: fwd for the 8 members of the lock-step pass (and for the 4 mismatched-caption heads);
    feat in the penalty's sweep and in the adjoint of each fwd; second once, in the sweep's second backward; weight in the
    adjoint of each fwd and behind second. A G step: one fwd, one feat (D is frozen: no weight role). mbstd=0: no t2v_mbstd_*
    call at all."""
    from txt2vid_amd import functional as TF
    from txt2vid_amd.gan.trainer import TrainStep
    tokens = tokens_for(B)
    out = {}
    for on in (True, False):
        gan, optD, optG, losses, prm = make(kind, on)
        cnd = code(gan, tokens)
        seed(3)
        x = S.batch().to(DEV)
        step = TrainStep(gan, optD, optG, losses, prm, DEV)
        step.run(x, cnd)                                            # (first call fills the packed-weight and constant caches)
        seed(4)
        d = _trace(monkeypatch, lambda: step.part(0, x, cnd))       # pyramid, G forward, the D step
        g = _trace(monkeypatch, lambda: step.part(1))               # D's update, the (fused) G step
        step.part(2)
        out[on] = (d, g)
        TF.set_grad_sink(None)
    print('mbstd %s launch budget: D step %s | G step %s' % (kind, _mb_calls(out[True][0]), _mb_calls(out[True][1])))
    assert (_mb_calls(out[True][0]), _mb_calls(out[True][1])) == BUDGET[kind]
    assert _mb_calls(out[False][0]) == {} and _mb_calls(out[False][1]) == {}
    for k in (0, 1):
        on = Counter(c for c in out[True][k] if not c.startswith('t2v_mbstd_'))
        extra, fewer = on - Counter(out[False][k]), Counter(out[False][k]) - on
        print('mbstd %s launch budget: other calls added in the %s step: %s' % (kind, 'DG'[k], dict(extra)))
        assert not fewer and set(extra) <= {'t2v_multi'}, (dict(extra), dict(fewer))          # grouped adds behind the forks only


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


def test_mbstd_cli_train_checkpoint_resume_and_mismatch(tmp_path):
    """The unconditional spec with --dont_use_sent (which proj cannot do): train, checkpoint, resume; the same checkpoint without
    the spec is refused with a message that names mbstd."""
    out_dir, smp = str(tmp_path / 'out'), str(tmp_path / 'samples')
    spec = os.path.join(ROOT, 'tools', 'cfg', 'discrim_mbstd.json')
    base = ['--num_channels', '1', '--cuda', '--frame_sizes', '8', '16', '32', '64', '--D_names', 'video', '--G_lr', '0.0002',
            '--D_lr', '0.0002', '--D_beta1', '0.5', '--D_beta2', '.999', '--G_beta1', '0.5', '--G_beta2', '.999',
            '--D_loss', 'txt2vid.gan.losses.RSGANLoss', '--init_method', 'xavier', '--seed', '100', '--gp_lambda', '.5',
            '--subsample_input', '--workers', '0', '--log_period', '1', '--dont_use_sent',
            '--G', 'txt2vid.models.tganv2.gen.MultiScaleGen', '--D', spec,
            '--batch_size', '8', '--epochs', '1', '--out', out_dir]
    log = _cli(base + ['--out_samples', smp, '--max_iters', '3', '--save_model_period', '3', '--save_example_period', '0'], tmp_path)
    assert 'Iter 3, Loss_D' in log
    ck = glob.glob(os.path.join(out_dir, 'iter_3_lossG_*'))
    assert len(ck) == 1
    sd = torch.load(ck[0], map_location='cpu', weights_only=False)
    key = 'single_discrim.mbstd.weight'
    assert list(sd['video'])[-1] == key and tuple(sd['video'][key].shape) == (1,)
    assert float(sd['video'][key].abs().max()) > 0                   # zeros at initialisation, moved by the optimiser
    log2 = _cli(base + ['--out_samples', smp, '--max_iters', '2', '--weights', ck[0], '--save_model_period', '1000',
                        '--save_example_period', '0'], tmp_path)
    assert 'Iter 2, Loss_D' in log2
    plain = [a if a != spec else 'txt2vid.models.tganv2.discrim.MultiScaleDiscrim' for a in base]
    log3 = _cli(plain + ['--out_samples', smp, '--max_iters', '1', '--weights', ck[0], '--save_model_period', '1000',
                         '--save_example_period', '0'], tmp_path, ok=False)
    assert 'mbstd' in log3 and 'minibatch standard deviation' in log3
