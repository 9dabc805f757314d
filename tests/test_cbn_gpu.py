"""GPU: the generator's opt-in conditional BatchNorm (MultiScaleGen(cond_bn=True); DESIGN "Conditional BatchNorm") on the HIP
path, against the float64 / plain-torch restatement of tests/cbn_cases.py, alone and composed with the oracle: every kernel path
of the `t2v_cbn_*` entry points (metric and bounds of tests/norm_cases.py), the module (bounds of tests/test_ca_gpu.py), three
training iterations (1:1 and 2:1), graph replay, --end2end, the launch budget and the command line."""
import ctypes as C
import glob
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import cbn_cases as CB
import norm_cases as nc
import schedule_cases as S
from oracle import tganv2_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, B = S.V, S.B
FIELDS = ['y', 'dx', 'dgamma', 'dbeta', 'dtab', 'rm', 'rv']
IDS = ['%s-%s' % cr for cr in CB.CASE_RECIPES]


def _tag(*parts):
    return '/'.join(str(p) for p in parts)


def seed(s):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


# ------------------------------------------------------------------------------------------------ op level: the autograd surface

def run_op(case, recipe, relu, up, fork, wide, tab=None, counter=None, training=True, gy=None):
    """One `cond_batch_norm_act` forward (+ backward in training mode) on fresh device copies of the case's inputs. In a wide
    table only the site's columns of dL/dtab are defined (the generator's sites cover every column between them; the raw-ABI
    test checks that the others are left alone): the rest is returned as zeros."""
    from txt2vid_amd.functional_cbn import _Shared, cond_batch_norm_act
    inp = CB.inputs(case, recipe, wide)
    _, T, s, R = CB.CASES[case]
    ld, off = CB.geometry(case, wide)
    x = inp['x'].to(DEV).requires_grad_(training)
    gamma, beta = torch.nn.Parameter(inp['gamma'].to(DEV)), torch.nn.Parameter(inp['beta'].to(DEV))
    t = (inp['tab'] if tab is None else tab).to(DEV).requires_grad_(training)
    rm, rv = inp['rm'].to(DEV).clone(), inp['rv'].to(DEV).clone()          # (updated in place: never the shared inputs)
    res = cond_batch_norm_act(x, gamma, beta, rm, rv, training, (t, _Shared(1), off, s, T), CB.MOMENTUM, CB.EPS, relu, counter, up,
                              fork != 'off')
    y, alias = res if fork != 'off' else (res, None)
    out = {'y': y.detach(), 'rm': rm, 'rv': rv, 'alias': alias}
    if training:
        loss = (y * (CB.grad_out(inp, relu, up) if gy is None else gy).to(DEV)).sum()
        if fork == 'both':
            loss = loss + (alias * inp['w2'].to(DEV)).sum()
        out['dx'], out['dgamma'], out['dbeta'], dtab = torch.autograd.grad(loss, [x, gamma, beta, t])
        site = torch.zeros(R, ld, dtype=torch.bool, device=DEV)
        site[:, off:off + 2 * x.shape[1]] = True
        out['dtab'] = torch.where(site, dtab, torch.zeros_like(dtab))
    return out


@pytest.mark.parametrize('wide', [False, True], ids=['alone', 'wide'])
@pytest.mark.parametrize('fork', ['off', 'both'])
@pytest.mark.parametrize('up', [False, True], ids=['flat', 'up'])
@pytest.mark.parametrize('relu', [False, True], ids=['lin', 'relu'])
@pytest.mark.parametrize('case,recipe', CB.CASE_RECIPES, ids=IDS)
def test_cond_batch_norm_act(case, recipe, relu, up, fork, wide):
    got = run_op(case, recipe, relu, up, fork, wide)
    ref = CB.case_reference(case, recipe, relu, up, fork, wide)
    CB.check(_tag(case, recipe, int(relu), int(up), fork, int(wide)), got, ref, FIELDS)
    # exact zeros where the reference has exact zeros: table rows the level does not hold, columns outside the site
    assert not got['dtab'].cpu()[ref['dtab'] == 0].any()
    if fork != 'off':
        assert torch.equal(got['alias'].detach().cpu(), CB.inputs(case, recipe, wide)['x'])


def test_backward_through_the_alias_only_writes_zero_columns():
    """Only the fork's alias takes part in the loss: dL/dx is the alias's gradient, and the site still writes its columns of
    dL/dtab (zeros) so that the shared buffer holds no unwritten memory."""
    from txt2vid_amd.functional_cbn import _Shared, cond_batch_norm_act
    inp = CB.inputs('strided', 'plain', True)
    (N, Cc, H, W), T, s, R = CB.CASES['strided']
    ld, off = CB.geometry('strided', True)
    x = inp['x'].to(DEV).requires_grad_(True)
    gamma, beta = torch.nn.Parameter(inp['gamma'].to(DEV)), torch.nn.Parameter(inp['beta'].to(DEV))
    t = inp['tab'].to(DEV).requires_grad_(True)
    y, alias = cond_batch_norm_act(x, gamma, beta, inp['rm'].to(DEV).clone(), inp['rv'].to(DEV).clone(), True, (t, _Shared(1), off, s, T),
                                   CB.MOMENTUM, CB.EPS, True, None, False, True)
    dx, dg, db, dtab = torch.autograd.grad((alias * inp['w2'].to(DEV)).sum(), [x, gamma, beta, t], allow_unused=True)
    assert torch.equal(dx.cpu(), inp['w2']) and dg is None and db is None
    assert not dtab[:, off:off + 2 * Cc].any()


@pytest.mark.parametrize('up', [False, True], ids=['flat', 'up'])
@pytest.mark.parametrize('relu', [False, True], ids=['lin', 'relu'])
@pytest.mark.parametrize('case', ['strided', 'straddle', 'frames'])
def test_eval_mode(case, relu, up):
    """Running statistics and the same per-sample affine; the buffers and the counter stay as they are."""
    inp = CB.inputs(case, 'plain', True)
    counter = torch.tensor(7, dtype=torch.int64, device=DEV)
    with torch.no_grad():
        got = run_op(case, 'plain', relu, up, 'off', True, counter=counter, training=False)
    CB.check(_tag(case, 'eval', int(relu), int(up)), got, CB.case_reference(case, 'plain', relu, up, 'off', True, False), ['y'])
    assert torch.equal(got['rm'].cpu(), inp['rm']) and torch.equal(got['rv'].cpu(), inp['rv']) and int(counter) == 7


@pytest.mark.parametrize('up', [False, True], ids=['flat', 'up'])
@pytest.mark.parametrize('case,recipe', [('cap64', 'offset'), ('straddle', 'offset'), ('frames', 'plain'), ('one_pixel', 'plain')])
def test_two_runs_give_the_same_bits(case, recipe, up):
    a = run_op(case, recipe, True, up, 'both', True)
    b = run_op(case, recipe, True, up, 'both', True)
    for f in FIELDS:
        assert torch.equal(a[f], b[f]), f


@pytest.mark.parametrize('up', [False, True], ids=['flat', 'up'])
@pytest.mark.parametrize('relu', [False, True], ids=['lin', 'relu'])
@pytest.mark.parametrize('case,recipe', CB.CASE_RECIPES, ids=IDS)
def test_statistics_are_the_plain_sites_and_a_zero_table_is_the_plain_site(case, recipe, relu, up):
    """The statistics never see the affine: running statistics and counter equal `TF.batch_norm_act`'s on the same x BITWISE (the
    same statistics kernel, the same merge), whatever the table holds. With a zero table y, dx, dgamma and dbeta match the plain
    path at the op bound (not bitwise: the conditional pass multiplies by 1/std and by Gamma one after the other). dL/dy is
    zeroed inside the ReLU band of the zero-table pre-activation as well, for the reason norm_cases gives."""
    import torch.nn.functional as F
    from txt2vid_amd import functional as TF
    inp = CB.inputs(case, recipe, True)
    (N, Cc, H, W), T, s, R = CB.CASES[case]
    ld, off = CB.geometry(case, True)
    pre = F.batch_norm(inp['x'].double(), None, None, inp['gamma'].double(), inp['beta'].double(), True, 0.0, CB.EPS)
    near = (pre.abs() < CB.RELU_BAND) & (pre != 0)
    gy = CB.grad_out(inp, relu, up)
    if relu:
        gy = gy.masked_fill(F.interpolate(near.double(), scale_factor=2) > 0 if up else near, 0.0)
    c0, c1, c2 = (torch.tensor(41, dtype=torch.int64, device=DEV) for _ in range(3))
    got = run_op(case, recipe, relu, up, 'both', True, counter=c0)
    zero = run_op(case, recipe, relu, up, 'both', True, tab=torch.zeros(R, ld), counter=c1, gy=gy)
    x = inp['x'].to(DEV).requires_grad_(True)
    gamma, beta = torch.nn.Parameter(inp['gamma'].to(DEV)), torch.nn.Parameter(inp['beta'].to(DEV))
    rm, rv = inp['rm'].to(DEV).clone(), inp['rv'].to(DEV).clone()
    y, alias = TF.batch_norm_act(x, gamma, beta, rm, rv, True, CB.MOMENTUM, CB.EPS, relu, c2, up, True)
    loss = (y * gy.to(DEV)).sum() + (alias * inp['w2'].to(DEV)).sum()
    dx, dg, db = torch.autograd.grad(loss, [x, gamma, beta])
    for r_ in (got, zero):
        assert torch.equal(r_['rm'], rm) and torch.equal(r_['rv'], rv)
    assert int(c0) == int(c1) == int(c2) == 42
    plain = {'y': y.detach(), 'dx': dx, 'dgamma': dg, 'dbeta': db}
    CB.check(_tag(case, recipe, int(relu), int(up), 'zero-vs-plain'), zero, plain, ['y', 'dx', 'dgamma', 'dbeta'])
    assert not zero['dtab'].isnan().any()


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
        self.p = C.c_void_p(self.t.data_ptr())

    def intact(self):
        return bool((self.buf[:GUARD] == SENTINEL).all()) and bool((self.buf[GUARD + self.n:] == SENTINEL).all())


@pytest.mark.parametrize('up', [False, True], ids=['flat', 'up'])
@pytest.mark.parametrize('relu', [False, True], ids=['lin', 'relu'])
@pytest.mark.parametrize('case,recipe', [('strided', 'plain'), ('straddle', 'offset'), ('cap64', 'plain'), ('frames', 'plain'),
                                         ('wide_c', 'plain')])
def test_raw_abi_on_guarded_buffers(case, recipe, relu, up):
    """t2v_cbn_train_fwd[_up] -> t2v_cbn_train_bwd[_up] and t2v_cbn_train_bwd_add with no Python caller, in a wide table: the
    reference's results, (mean, 1/std) and running statistics bitwise those of t2v_bn_train_fwd, a workspace of exactly
    t2v_cbn_ws_floats, the poisoned columns outside the site untouched, nothing written outside any buffer."""
    from txt2vid_amd._lib import lib
    from txt2vid_amd._ops import _stream
    L, st = lib(), _stream()
    inp = CB.inputs(case, recipe, True)
    (N, Cc, H, W), T, s, R = CB.CASES[case]
    ld, off = CB.geometry(case, True)
    n, ny = N * Cc * H * W, N * Cc * H * W * (4 if up else 1)
    keep = [inp[k].to(DEV).contiguous() for k in ('x', 'gamma', 'beta', 'w2', 'tab')] + [CB.grad_out(inp, relu, up).to(DEV).contiguous()]
    x, gamma, beta, w2, tab, gy = [C.c_void_p(t.data_ptr()) for t in keep]
    guards = []

    def out(k, init=None):
        guards.append(Guarded(k, init))
        return guards[-1]
    nws = int(L.t2v_cbn_ws_floats(N, Cc, H * W))
    stats, rm, rv = out(2 * Cc), out(Cc, inp['rm'].to(DEV)), out(Cc, inp['rv'].to(DEV))
    stats_p, rm_p, rv_p = out(2 * Cc), out(Cc, inp['rm'].to(DEV)), out(Cc, inp['rv'].to(DEV))
    y, y_p, gx, dg, db, gx_a, dg_a, db_a = out(ny), out(ny), out(n), out(Cc), out(Cc), out(n), out(Cc), out(Cc)
    poison = torch.full((R, ld), 12345.5, device=DEV)
    gtab, gtab_a = out(R * ld, poison), out(R * ld, poison)
    ws_f, ws_b, ws_a, ws_p = out(nws), out(nws), out(nws), out(int(L.t2v_bn_ws_floats(N, Cc, H * W)))
    counter = torch.tensor([-9, 2 ** 40 + 1, -9], dtype=torch.int64, device=DEV)
    cp = C.c_void_p(counter[1:].data_ptr())
    fwd, bwd = (L.t2v_cbn_train_fwd_up, L.t2v_cbn_train_bwd_up) if up else (L.t2v_cbn_train_fwd, L.t2v_cbn_train_bwd)
    assert fwd(x, gamma, beta, tab, y.p, stats.p, rm.p, rv.p, ws_f.p, N, Cc, H, W, ld, off, s, T, R, CB.MOMENTUM, CB.EPS, int(relu), cp,
               st) == 0
    assert bwd(gy, x, y.p, stats.p, gamma, tab, gx.p, dg.p, db.p, gtab.p, ws_b.p, N, Cc, H, W, ld, off, s, T, R, int(relu), st) == 0
    assert L.t2v_cbn_train_bwd_add(gy, x, y.p, stats.p, gamma, tab, w2, gx_a.p, dg_a.p, db_a.p, gtab_a.p, ws_a.p, N, Cc, H, W, ld, off, s,
                                   T, R, int(up), int(relu), st) == 0
    if up:
        assert L.t2v_bn_train_fwd_up(x, gamma, beta, y_p.p, stats_p.p, rm_p.p, rv_p.p, ws_p.p, N, Cc, H, W, CB.MOMENTUM, CB.EPS, int(relu),
                                     None, st) == 0
    else:
        assert L.t2v_bn_train_fwd(x, gamma, beta, y_p.p, stats_p.p, rm_p.p, rv_p.p, ws_p.p, N, Cc, H * W, CB.MOMENTUM, CB.EPS, int(relu),
                                  None, st) == 0
    torch.cuda.synchronize()
    assert all(g.intact() for g in guards), [i for i, g in enumerate(guards) if not g.intact()]
    assert counter.tolist() == [-9, 2 ** 40 + 2, -9]
    assert torch.equal(stats.t, stats_p.t) and torch.equal(rm.t, rm_p.t) and torch.equal(rv.t, rv_p.t)      # bitwise
    m = 2 if up else 1
    ref = CB.case_reference(case, recipe, relu, up, 'off', True)
    g2 = gtab.t.reshape(R, ld)
    site = torch.zeros(R, ld, dtype=torch.bool, device=DEV)
    site[:, off:off + 2 * Cc] = True
    assert bool((g2[~site] == 12345.5).all()) and bool((gtab_a.t.reshape(R, ld)[~site] == 12345.5).all())
    got = {'y': y.t.reshape(N, Cc, m * H, m * W), 'dx': gx.t.reshape(N, Cc, H, W), 'dgamma': dg.t, 'dbeta': db.t, 'rm': rm.t,
           'rv': rv.t, 'mean': stats.t[:Cc], 'istd': stats.t[Cc:], 'dtab': torch.where(site, g2, torch.zeros_like(g2))}
    CB.check(_tag(case, recipe, int(relu), int(up), 'abi'), got, ref, FIELDS + ['mean', 'istd'])
    ga = gtab_a.t.reshape(R, ld)
    got_a = {'dx': gx_a.t.reshape(N, Cc, H, W), 'dgamma': dg_a.t, 'dbeta': db_a.t, 'dtab': torch.where(site, ga, torch.zeros_like(ga))}
    CB.check(_tag(case, recipe, int(relu), int(up), 'abi-add'), got_a, CB.case_reference(case, recipe, relu, up, 'both', True),
             ['dx', 'dgamma', 'dbeta', 'dtab'])
    if s > 1:                                                   # table rows the level does not hold: exact zeros in the site's columns
        assert not g2[1::s][:, off:off + 2 * Cc].any()


def test_entry_points_refuse_bad_arguments_and_launch_nothing():
    """Real device pointers, bad extents: T2V_EINVAL (a launch would return 0 or a HIP status) and the outputs keep their poison."""
    from txt2vid_amd._lib import lib
    L = lib()
    buf = torch.full((4096,), 3.5, device=DEV)
    p = C.c_void_p(buf.data_ptr())
    for kw in (dict(T=4), dict(R=2), dict(s=2, R=4), dict(ld=11), dict(off=1), dict(N=0), dict(Cc=0), dict(H=0)):
        a = dict(N=6, Cc=6, H=5, W=5, ld=12, off=0, s=1, T=2, R=3)
        a.update(kw)
        g = (a['N'], a['Cc'], a['H'], a['W'], a['ld'], a['off'], a['s'], a['T'], a['R'])
        assert L.t2v_cbn_train_fwd(p, p, p, p, p, p, p, p, p, *g, 0.1, 1e-5, 0, None, None) == -1, kw
        assert L.t2v_cbn_train_fwd_up(p, p, p, p, p, p, p, p, p, *g, 0.1, 1e-5, 0, None, None) == -1, kw
        assert L.t2v_cbn_train_bwd(p, p, p, p, p, p, p, p, p, p, p, *g, 0, None) == -1, kw
        assert L.t2v_cbn_train_bwd_up(p, p, p, p, p, p, p, p, p, p, p, *g, 0, None) == -1, kw
        assert L.t2v_cbn_train_bwd_add(p, p, p, p, p, p, None, p, p, p, p, p, *g, 0, 0, None) == -1, kw
        assert L.t2v_cbn_eval(p, p, p, p, p, p, p, *g, 1e-5, 0, None) == -1, kw
    assert L.t2v_cbn_train_fwd(p, p, p, None, p, p, p, p, p, 6, 6, 5, 5, 12, 0, 1, 2, 3, 0.1, 1e-5, 0, None, None) == -1
    assert L.t2v_cbn_train_bwd(p, p, None, p, p, p, p, p, p, p, p, 6, 6, 5, 5, 12, 0, 1, 2, 3, 1, None) == -1           # relu needs y
    torch.cuda.synchronize()
    assert bool((buf == 3.5).all())


# ------------------------------------------------------------------------------------------------ module level

def pour(module, zero_proj=False):
    sd = {k: O.recipe_tensor(k, v.shape) for k, v in module.state_dict().items()}
    if zero_proj:
        sd['cond_bn.weight'].zero_()
        sd['cond_bn.bias'].zero_()
    module.load_state_dict(sd)
    return module.to(DEV)


def tokens_for(batch, s=77):
    tg = torch.Generator()
    tg.manual_seed(s)
    t = torch.randint(4, V, (batch, 8), generator=tg)
    t[:, 0], t[:, -1] = 1, 2
    return t


def _gen(**kw):
    from txt2vid_amd.models.tganv2_cond.gen import MultiScaleGen
    return MultiScaleGen(width=64, height=64, num_channels=1, cond_dim=256, **kw)


def _close_levels(fake, fo):
    for a, b in zip(fake, fo):
        assert a.shape == b.shape
        scale = max(1.0, float(b.abs().max()))
        np.testing.assert_allclose(a.detach().cpu().numpy(), b.detach().numpy(), rtol=2e-3, atol=5e-4 * scale)


def _module_vs_composition(monkeypatch, Bn=3, watch=('cond_bn.weight', 'cond_bn.bias', 'fc.weight'), zero_proj=False, **kw):
    """Forward + backward of a cond_bn generator with fixed z / phases against the patched-oracle composition: every rendered
    level, the per-parameter gradient norms (one vector, and the watched keys one by one), dL/dcond as one vector; then eval
    mode's video. Bounds of tests/test_ca_gpu.py: rtol 2e-3, atol 5e-4 x scale; 3e-3 on the norms."""
    D, no_lstm = kw.get('ca_dim', 0), kw.get('no_lstm', False)
    m = pour(_gen(cond_bn=True, **kw), zero_proj).train()
    PG = CB.gen_state(D, no_lstm=no_lstm, zero_proj=zero_proj)
    keys = [k for k, _ in m.named_parameters()]
    assert set(keys) == set(k for k, v in PG.items() if v.dtype.is_floating_point and 'running_' not in k)
    for k in keys:
        PG[k].requires_grad_(True)
    g = torch.Generator()
    g.manual_seed(3)
    z, s = torch.randn(Bn, 256, generator=g), 0.5 * torch.randn(Bn, 256, generator=g)
    seed(5)
    sd = s.to(DEV).requires_grad_(True)
    fake, kl = m(z.to(DEV), cond=sd, return_kl=True)
    assert [f.shape[0] for f in fake] == [3, 2, 1, 1][:len(fake)] or Bn != 3
    weights = [torch.randn(*f.shape, generator=g) for f in fake]
    loss = sum((f * w.to(DEV)).sum() for f, w in zip(fake, weights))
    if D:
        loss = loss + 2.0 * kl
    loss.backward()
    seed(5)
    so = s.clone().requires_grad_(True)
    fo, klo = CB.gen_cbn(monkeypatch, PG, z, so)                  # with CA: eps drawn first, then the 3 phases, the module's order
    lo = sum((f * w).sum() for f, w in zip(fo, weights))
    if D:
        lo = lo + 2.0 * klo
    lo.backward()
    _close_levels(fake, fo)
    named = dict(m.named_parameters())
    got = np.array([float(named[k].grad.norm()) for k in keys])
    want = np.array([float(PG[k].grad.norm()) for k in keys])
    rel = float(np.linalg.norm(got - want) / np.linalg.norm(want))
    print('cbn module %s: gradient-norm vector rel %.3g' % (kw, rel))
    assert rel < 3e-3, rel
    for k in watch:
        gk, wk = float(named[k].grad.norm()), float(PG[k].grad.norm())
        print('cbn module %s: |d %s| %.6g (%.6g)' % (kw, k, gk, wk))
        assert wk > 0 and abs(gk - wk) < 3e-3 * wk, (k, gk, wk)
    # the projection's gradients element by element too (their norm alone would not see a site's columns in another's place)
    for k in ('cond_bn.weight', 'cond_bn.bias'):
        a, b = named[k].grad.cpu().double(), PG[k].grad.double()
        assert float((a - b).norm() / b.norm()) < 3e-3, k
    ds = so.grad.double()
    rel = float((sd.grad.cpu().double() - ds).norm() / ds.norm())
    print('cbn module %s: dL/dcond rel %.3g' % (kw, rel))
    assert rel < 3e-3, rel
    assert all(int(m.state_dict()[q + 'num_batches_tracked']) == 1 for q in CB.site_prefixes())
    m.eval()
    with torch.no_grad():
        seed(6)
        v = m(z[:2].to(DEV), cond=sd[:2].detach())
        seed(6)
        e = CB.gen_cbn(monkeypatch, PG, z[:2], s[:2], training=False)[0]
    assert len(v) == 1
    _close_levels(v, e)
    return m, fake, PG


def test_cond_bn_generator_vs_patched_oracle(monkeypatch):
    _module_vs_composition(monkeypatch)


def test_cond_bn_generator_with_ca_vs_patched_oracle(monkeypatch):
    _module_vs_composition(monkeypatch, watch=('cond_bn.weight', 'cond_bn.bias', 'fc.weight', 'ca.fc.weight'), ca_dim=128)


def test_cond_bn_generator_no_lstm_vs_patched_oracle(monkeypatch):
    _module_vs_composition(monkeypatch, watch=('cond_bn.weight', 'cond_bn.bias'), no_lstm=True)


def test_zero_projection_is_the_plain_generator_and_still_gets_its_gradient(monkeypatch):
    m, fake, PG = _module_vs_composition(monkeypatch, watch=('cond_bn.weight', 'cond_bn.bias'), zero_proj=True)
    plain = pour(_gen()).train()                                  # the same recipe weights, no projection
    g = torch.Generator()
    g.manual_seed(3)
    z, s = torch.randn(3, 256, generator=g), 0.5 * torch.randn(3, 256, generator=g)
    seed(5)
    with torch.no_grad():
        ref = plain(z.to(DEV), cond=s.to(DEV))
    _close_levels(fake, [r.cpu() for r in ref])
    assert float(PG['cond_bn.weight'].grad.norm()) > 0


# ------------------------------------------------------------------------------------------------ launch budget

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


def test_launch_budget(monkeypatch):
    """Per generator forward + backward: 16 conditional forwards (two launches each, as the plain site's), 16 conditional
    backwards (two launches each: at most 2 x 16), no plain t2v_bn_* training call, and beyond that exactly what one Linear
    [B, 256] -> [B, 6592] adds forward and backward (the projection). cond_bn=False: no t2v_cbn_* call."""
    from collections import Counter
    from txt2vid_amd import functional as TF
    g = torch.Generator()
    g.manual_seed(3)
    z, s = torch.randn(3, 256, generator=g).to(DEV), (0.5 * torch.randn(3, 256, generator=g)).to(DEV)

    def step(m):
        def f():
            seed(5)
            fake = m(z, cond=s)
            sum(x.sum() for x in fake).backward()
        return f
    on, off = pour(_gen(cond_bn=True)).train(), pour(_gen()).train()
    lin_w = torch.nn.Parameter(on.cond_bn.weight.detach().clone())
    lin_b = torch.nn.Parameter(on.cond_bn.bias.detach().clone())
    tab_g = torch.ones(3, 6592, device=DEV)
    lin = lambda: TF.linear(s, lin_w, lin_b).backward(tab_g)
    for f in (step(on), step(off), lin):                          # (first calls fill the packed-weight and constant caches)
        f()
    c_on, c_off = Counter(_trace(monkeypatch, step(on))), Counter(_trace(monkeypatch, step(off)))
    c_lin = Counter(_trace(monkeypatch, lin))
    cbn = {k: v for k, v in c_on.items() if k.startswith('t2v_cbn_')}
    fwd = sum(v for k, v in cbn.items() if k in ('t2v_cbn_train_fwd', 't2v_cbn_train_fwd_up'))
    bwd = sum(v for k, v in cbn.items() if k in ('t2v_cbn_train_bwd', 't2v_cbn_train_bwd_up', 't2v_cbn_train_bwd_add'))
    print('cbn launch budget: on %s | projection %s' % (sorted(cbn.items()), sorted(c_lin.items())))
    assert fwd == 16 and bwd == 16 and 2 * bwd <= 2 * 16
    assert cbn.get('t2v_cbn_ws_floats', 0) == 32 and 't2v_cbn_eval' not in cbn
    assert not any(k.startswith('t2v_bn_') for k in c_on)
    assert not any(k.startswith('t2v_cbn_') for k in c_off)
    bn_off = {k: v for k, v in c_off.items() if k.startswith('t2v_bn_')}
    assert sum(v for k, v in bn_off.items() if k.startswith('t2v_bn_train_fwd')) == 16
    rest_on = Counter({k: v for k, v in c_on.items() if not k.startswith('t2v_cbn_')})
    rest_off = Counter({k: v for k, v in c_off.items() if not k.startswith('t2v_bn_')})
    assert rest_on == rest_off + c_lin, (rest_on - rest_off, c_lin)


# ------------------------------------------------------------------------------------------------ iteration level

def make(N=1, M=1, batch=B, **kw):
    from txt2vid_amd.models.tganv2_cond.discrim import MultiScaleDiscrim
    from txt2vid_amd.models.txt.basic import Seq2Seq
    from txt2vid_amd.gan.cond_gan import CondGan
    from txt2vid_amd.gan.losses import MixedGanLoss, RSGANLoss
    from txt2vid_amd.optim import Adam
    gen = pour(_gen(cond_bn=True, **kw)).train()
    dis = pour(MultiScaleDiscrim(num_channels=1, cond_dim=256)).train()
    txt = Seq2Seq(vocab_size=V)
    txt.load_state_dict({k: O.recipe_tensor(k if k.startswith('encoder.') else 'encoder.' + k[len('decoder.'):], v.shape)
                         for k, v in txt.state_dict().items()})
    txt.to(DEV)
    gan = CondGan(gen=gen, discrims=[dis], cond_encoder=txt, discrim_names=['video'])
    optD = Adam([{'params': dis.parameters()}], lr=2e-4, betas=(0.5, 0.999))
    optG = Adam([{'params': gen.parameters()}], lr=2e-4, betas=(0.5, 0.999))
    prm = S.params_for(dict(N=N, M=M, gp=0.5, mean_d=False, mean_g=False))
    return gan, optD, optG, MixedGanLoss(g_loss=RSGANLoss(), d_loss=RSGANLoss()), prm


@pytest.mark.parametrize('N,M', [(1, 1), (2, 1)])
def test_cond_bn_iterations_vs_patched_oracle(monkeypatch, N, M):
    """Three text-conditioned iterations against the oracle loop with conditional sites: lossD and lossG at the bounds of the CA
    loop tests (1e-3, then 2e-2 in iteration 2: the GAN dynamics are chaotic)."""
    from txt2vid_amd.gan.trainer import TrainStep
    tokens = tokens_for(B)
    ref = CB.oracle_loop(monkeypatch, N, M, tokens, iters=3)
    gan, optD, optG, losses, prm = make(N, M)
    seed(100)
    for it in range(3):
        x = S.batch().to(DEV)
        with torch.no_grad():
            cond = gan.cond_encoder.encode(tokens.to(DEV), [8] * B)[2].detach()
        lD, lG, _, _ = TrainStep(gan, optD, optG, losses, prm, DEV).run(x, cond)
        lD, lG = float(lD), float(lG)
        tol = 1e-3 if it < 2 else 2e-2
        print('cond_bn %d:%d it %d: lossD %.6f (%.6f) lossG %.6f (%.6f)' % (N, M, it, lD, ref['lossD'][it], lG, ref['lossG'][it]))
        assert abs(lD - ref['lossD'][it]) < tol * max(1.0, abs(ref['lossD'][it]))
        assert abs(lG - ref['lossG'][it]) < tol * max(1.0, abs(ref['lossG'][it]))
    assert float(gan.gen.cond_bn.weight.grad.norm()) > 0


def test_cond_bn_graph_replay_matches_eager():
    """GraphedTrainStep with conditional sites (the projection, the 16 sites and the shared dL/dtab buffer inside the one captured
    graph) reproduces the eager iterations: 2 eager, then capture + replays, at the existing replay tolerance."""
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
    w_eager = gan.gen.cond_bn.weight.detach().clone()
    gan, optD, optG, losses, prm = make()
    seed(6)
    gs = GraphedTrainStep(gan, optD, optG, losses, prm, DEV, (B, 1, 16, 64, 64), warmup=2, cond_dim=256)
    for i, x in enumerate(batches()):
        cond = gan.cond_encoder.encode(tokens, [8] * B)[2].detach()
        lD, lG = gs.step(x, cond)
        got = (float(lD), float(lG))
        print('cond_bn step %d (%s): %s vs eager %s' % (i, 'replay' if i >= 2 else 'eager', got, eager[i]))
        tol = 2e-5 if i < 2 else 2e-3
        assert all(abs(a - b) < tol for a, b in zip(got, eager[i])), (i, got, eager[i])
    assert gs.graphs is not None and gs.n_graphs == 1
    w = gan.gen.cond_bn.weight.detach()
    assert float((w - w_eager).norm() / w_eager.norm()) < 2e-3


def test_cond_bn_end2end_encoder_gradient_vs_patched_oracle(monkeypatch):
    """--end2end: the sentence code keeps its graph and now has two consumers in the generator (fc's input and the projection),
    their gradients summed by the grouped fork. One iteration: both losses and the encoder's gradient norms left by the G step."""
    from txt2vid_amd.gan.trainer import train_iteration
    from txt2vid_amd.optim import Adam
    gan, _, _, losses, prm = make()
    txt = gan.cond_encoder.differentiable(True)
    dis, gen = gan.discrims[0], gan.gen
    optD = Adam([{'params': dis.parameters()}, {'params': txt.parameters()}], lr=2e-4, betas=(0.5, 0.999))
    optG = Adam([{'params': gen.parameters()}, {'params': txt.parameters()}], lr=2e-4, betas=(0.5, 0.999))
    _, PD, PT, pre = S.oracle_states(dict(cond=True))
    PG = CB.gen_state()
    tr = O.OracleTrainer(PG, PD, d_prefix=pre, end2end_txt=PT)
    tokens, lengths = tokens_for(B, 5), [8] * B
    seed(31)
    x = (torch.rand(B, 16, 1, 64, 64) * 2 - 1).permute(0, 2, 1, 3, 4).contiguous()
    state = (torch.get_rng_state(), np.random.get_state(), random.getstate())
    cond = txt.encode(tokens.to(DEV), lengths)[2]
    assert cond.requires_grad
    lD, lG, _, _ = train_iteration(gan, x.to(DEV), cond, optD, optG, losses, prm, DEV, end2end=True)
    lD, lG = float(lD), float(lG)
    torch.set_rng_state(state[0])
    np.random.set_state(state[1])
    random.setstate(state[2])
    # the oracle's step_end2end with conditional sites in the generator
    c = O.text_encode_grad(PT, tokens, lengths)
    xs, conds, _ = O.multiscale_data(x, c, S.FS)
    z = torch.randn(B, 256)
    fake, _ = CB.gen_cbn(monkeypatch, PG, z, conds[0])
    tr.zero(PD, tr.d_params)
    tr.zero(PT, tr.t_params)
    fc0 = conds[0][O.gen_perm(B)]
    lDo = O.discrim_loss(PD, pre, xs, [f.detach() for f in fake], conds, [fc0[0:cc.size(0)] for cc in conds], 0.5)
    lDo.backward(retain_graph=True)
    tr.optD.step()
    O.gen_perm(B)
    real_pred = O.multiscale_discrim(PD, xs, conds, pre)
    tr.zero(PG, tr.g_params)
    tr.zero(PT, tr.t_params)
    lGo = O.gen_loss(PD, pre, fake, real_pred, conds)
    lGo.backward()
    lDo, lGo = float(lDo), float(lGo)
    print('cond_bn end2end: HIP lossD %.6f lossG %.6f | oracle %.6f %.6f' % (lD, lG, lDo, lGo))
    assert abs(lD - lDo) < 1e-3 and abs(lG - lGo) < 1e-3
    named = dict(txt.encoder.named_parameters())
    ref_max = max(float(PT[k].grad.norm()) for k in tr.t_params)
    for k in tr.t_params:
        got, want = float(named[k[len('encoder.'):]].grad.norm()), float(PT[k].grad.norm())
        assert abs(got - want) <= 1e-2 * want + 1e-5 * ref_max, (k, got, want)
    gk, wk = float(gen.cond_bn.weight.grad.norm()), float(PG['cond_bn.weight'].grad.norm())
    assert abs(gk - wk) < 1e-2 * wk, (gk, wk)


# ------------------------------------------------------------------------------------------------ command line

def _cli(args, tmp):
    cfg = os.path.join(str(tmp), 'synth.json')
    with open(cfg, 'w') as f:
        json.dump({'class': 'txt2vid.data.my_dataset', 'args': {'data': 'synthetic', 'num_frames': 16, 'length': 64}}, f)
    cmd = [sys.executable, '-m', 'txt2vid_amd.train.gan', '--data', cfg] + args
    p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = p.stdout.decode(errors='replace')
    assert p.returncode == 0, out[-3000:]
    return out


def test_cond_bn_cli_train_checkpoint_resume_and_sample(tmp_path):
    out_dir, smp = str(tmp_path / 'out'), str(tmp_path / 'samples')
    spec = os.path.join(ROOT, 'tools', 'cfg', 'gen_cond_cbn.json')
    base = ['--num_channels', '1', '--cuda', '--frame_sizes', '8', '16', '32', '64', '--D_names', 'video', '--G_lr', '0.0002',
            '--D_lr', '0.0002', '--D_beta1', '0.5', '--D_beta2', '.999', '--G_beta1', '0.5', '--G_beta2', '.999',
            '--D_loss', 'txt2vid.gan.losses.RSGANLoss', '--init_method', 'xavier', '--seed', '100', '--gp_lambda', '.5',
            '--subsample_input', '--workers', '0', '--log_period', '1',
            '--G', spec, '--D', 'txt2vid.models.tganv2_cond.discrim.MultiScaleDiscrim',
            '--sent', 'txt2vid.models.txt.basic.Seq2Seq', '--batch_size', '8', '--epochs', '1', '--out', out_dir]
    log = _cli(base + ['--out_samples', smp, '--max_iters', '2', '--save_model_period', '2', '--save_example_period', '2'], tmp_path)
    assert 'Iter 2, Loss_D' in log
    ck = glob.glob(os.path.join(out_dir, 'iter_2_lossG_*'))
    assert len(ck) == 1
    sd = torch.load(ck[0], map_location='cpu', weights_only=False)
    assert tuple(sd['gen']['cond_bn.weight'].shape) == (6592, 256) and tuple(sd['gen']['fc.weight'].shape) == (1024, 512)
    # zeros at initialisation, moved by two optimiser steps (the gradient is non-zero although the projection started at zero)
    assert float(sd['gen']['cond_bn.weight'].abs().max()) > 0 and float(sd['gen']['cond_bn.bias'].abs().max()) > 0
    log2 = _cli(base + ['--out_samples', smp, '--max_iters', '2', '--weights', ck[0], '--save_model_period', '1000',
                        '--save_example_period', '0'], tmp_path)
    assert 'Iter 2, Loss_D' in log2
    smp2 = str(tmp_path / 'samples_test')
    _cli(base + ['--out_samples', smp2, '--test', '--weights', ck[0], '--num_samples', '1'], tmp_path)
    assert os.path.exists(os.path.join(smp2, 'real_0.png')) and os.path.exists(os.path.join(smp2, '64x64_0_0.jpg'))
    # a cond_bn checkpoint into the cond_bn-off generator: refused with a message that names cond_bn
    cmd = [sys.executable, '-m', 'txt2vid_amd.train.gan', '--data', os.path.join(str(tmp_path), 'synth.json')] + \
        [a if a != spec else 'txt2vid.models.tganv2_cond.gen.MultiScaleGen' for a in base] + ['--out_samples', smp2, '--test', '--weights', ck[0]]
    p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode != 0 and b'cond_bn' in p.stdout
