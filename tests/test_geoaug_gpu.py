"""GPU: the geometric augmentation of the discriminator's inputs (the names flip, scale, rotate of --D_aug) on the
HIP path, against the CPU restatement composed with the oracle (tests/geoaug_cases.py) —
  (1) the two grouped kernels: the forward against float64 at a derived bound, the bit-exact cases, the adjoint as the exact
      transpose, the autograd surface, the refusals;
  (2) three training iterations against the oracle loop, the gradient through both launches, graph replay against eager, p read at
      run time;
  (3) the launch budget, and off means off;
  (4) the command line: training with --D_ada, checkpoint, resume, sampling."""
import ctypes
import glob
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import diffaug_cases as DA
import geoaug_cases as GC
import schedule_cases as S
import test_ada_gpu as TA                  # (its set-up helper with a controller: make)
import test_diffaug_gpu as TD              # (its set-up helpers: make, batches, seed, tokens_for, the iteration runners)
from txt2vid_amd import functional_aug as A

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -24
B = S.B
TOP = float(np.nextafter(np.float32(1), np.float32(0)))
GEO_FNS = ('t2v_geoaug_fwd', 't2v_geoaug_bwd')
OLD_FNS = ('t2v_diffaug_fwd', 't2v_diffaug_bwd', 't2v_diffaug_gated_fwd', 't2v_diffaug_gated_bwd')
N_ARG = {'t2v_geoaug_fwd': 2, 't2v_geoaug_bwd': 2, 't2v_diffaug_fwd': 1, 't2v_diffaug_bwd': 1, 't2v_diffaug_gated_fwd': 2,
         't2v_diffaug_gated_bwd': 2}

SHAPES = [(3, 1, 2, 8, 8), (2, 3, 4, 16, 16), (2, 1, 1, 9, 9), (1, 3, 3, 32, 32)]       # (9: odd S, a half-integer centre)


def fwd_bound(S_, X):
    """See test_forward_against_float64."""
    return (18 * S_ + 10) * EPS * X


def _inputs(shape, s=0):
    g = torch.Generator()
    g.manual_seed(777 + s + sum(shape))
    x = torch.rand(*shape, generator=g) * 2 - 1
    gy = torch.randn(*shape, generator=g)
    v = torch.rand(2 * shape[0], A.K, generator=g)
    v[0, 0], v[1, 0] = 0.25, 0.75                                   # both sides of the flip among the rows that are read
    gates = torch.rand(2 * shape[0], A.K, generator=g)
    return x, gy, v, gates


def _run(xs, gys, vs, strides, policy, gates=None, p=None, needs=None):
    """Forward + backward through the kernels. Returns (ys, gxs) on the host and the device outputs."""
    needs = [True] * len(xs) if needs is None else needs
    xd = [x.to(DEV).requires_grad_(n) for x, n in zip(xs, needs)]
    vd = [v.to(DEV) for v in vs]
    if gates is None:
        ys = A.geoaug(xd, vd, strides, policy)
    else:
        ys = A.geoaug(xd, vd, strides, policy, [None if g is None else g.to(DEV) for g in gates], p)
    live = [i for i, n in enumerate(needs) if n]
    grads = torch.autograd.grad([ys[i] for i in live], [xd[i] for i in live], [gys[i].to(DEV) for i in live]) if live else ()
    gxs = [None] * len(xs)
    for i, gr in zip(live, grads):
        gxs[i] = gr.cpu()
    return [y.detach().cpu() for y in ys], gxs, ys


def _counted(run, names):
    """Run `run()` with counting wrappers around the entry points of the loaded library; also records the member counts."""
    from txt2vid_amd import functional as TF
    l = TF.lib()
    orig = {n: getattr(l, n) for n in names}
    calls = {n: 0 for n in names}
    members = {n: [] for n in names}

    def wrap(n):
        def f(*a):
            calls[n] += 1
            members[n].append(a[N_ARG[n]])
            return orig[n](*a)
        return f
    try:
        for n in names:
            setattr(l, n, wrap(n))
        out = run()
    finally:
        for n in names:
            setattr(l, n, orig[n])
    return calls, members, out


# ------------------------------------------------------------------------------------------------ 1. op level
@pytest.fixture(scope='module')
def reference():
    """The float64 restatement and its autograd adjoint, once per (shape, policy, stride). Shared and left unchanged."""
    out = {}
    for shape, policy, stride in itertools.product(SHAPES, GC.GEO_SUBSETS, (1, 2)):
        x, gy, v, _ = _inputs(shape)
        xr = x.double().requires_grad_(True)
        y = GC.augment_geo(xr, v, policy, stride)
        gx, = torch.autograd.grad(y, xr, gy.double())
        out[shape, policy, stride] = (y.detach(), gx)
    return out


@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('policy', GC.GEO_SUBSETS)
def test_forward_against_float64(reference, policy, stride):
    """The four shapes in ONE launch per direction, against the float64 restatement on the same fp32-rounded matrix. The bound is
    derived from the operation sequence of geo_src / geo_weight / the blend in csrc/geoaug.hip, with u = 2^-24, X = max |x|,
    |m| <= 2^0.4 < 1.32 for every matrix entry and |cos| + |sin| <= 1.37:

      coordinates. xo, yo (|.| <= S/2) and half are exact. t = m01 * yo rounds once, |t| <= 0.66 S: 0.66 S u. xs = fma(m00, xo, t)
      rounds once, |xs| <= 1.32 * 1.37 * S/2 < 0.91 S: 0.91 S u. xs + half, |.| <= 1.41 S: 1.41 S u. - 0.5: (1.41 S + 0.5) u. So
      |d px| <= (4.39 S + 0.5) u, the same for py; floor and px - floor(px) are exact. The blend is continuous in (px, py), also
      across a floor boundary, with |d/d px| <= |(1 - wy)(b - a) + wy (d - c)| <= 2 X: the coordinates cost at most
      2 * 2 X * (4.39 S + 0.5) u <= (17.6 S + 2) u X, and a disagreement about x0 costs no more than that.
      weights. 1 - wx and 1 - wy round once, the product once: each weight is within 3 u of its value relatively, and the exact
      weights sum to 1: 3 u X (to first order; the slack of 18 against 17.6 covers the higher orders).
      blend. Four fma into one accumulator over terms whose absolute values sum to at most X: 4 u X.

        |dy| <= (17.6 S + 2 + 3 + 4) u X  <=  (18 S + 10) * 2^-24 * max |x|

    Adjoint (the first two shapes): dL/dx[i] sums at most 25 candidates, each weight within the forward's coordinate and weight
    error of the exact one (a bilinear weight has slope <= 1 per axis) and one fma each: the forward's bound with G = max |dL/dy|
    times the candidate count, 25 (18 S + 10) * 2^-24 * G."""
    ins = [_inputs(sh) for sh in SHAPES]
    ys, gxs, _ = _run([i[0] for i in ins], [i[1] for i in ins], [i[2] for i in ins], [stride] * 4, policy)
    for k, shape in enumerate(SHAPES):
        want_y, want_g = reference[shape, policy, stride]
        x, gy = ins[k][0], ins[k][1]
        S_ = shape[-1]
        by, bg = fwd_bound(S_, float(x.abs().max())), 25 * fwd_bound(S_, float(gy.abs().max()))
        ey = float((ys[k].double() - want_y).abs().max())
        eg = float((gxs[k].double() - want_g).abs().max())
        print('%s %s stride %d: forward measured/bound = %.3e / %.3e = %.4f, adjoint %.3e / %.3e = %.4f'
              % (shape, policy, stride, ey, by, ey / by, eg, bg, eg / bg))
        assert ey <= by, (shape, policy, stride, ey, by)
        if k < 2:
            assert eg <= bg, (shape, policy, stride, eg, bg)
        if policy != 'flip':
            assert not torch.equal(ys[k], x)
    ys2, gxs2, _ = _run([i[0] for i in ins], [i[1] for i in ins], [i[2] for i in ins], [stride] * 4, policy)
    assert all(torch.equal(a, b) for a, b in zip(ys, ys2)) and all(torch.equal(a, b) for a, b in zip(gxs, gxs2))


@pytest.mark.parametrize('stride', [1, 2])
def test_bit_exact_cases(stride):
    ins = [_inputs(sh, 1) for sh in SHAPES]
    xs, gys, vs, gs = ([i[k] for i in ins] for k in range(4))
    st = [stride] * 4
    # a pure flip policy: torch.flip where v0 < 0.5, the input elsewhere; the adjoint of a mirror is the mirror
    ys, gxs, _ = _run(xs, gys, vs, st, 'flip')
    for x, gy, v, y, gx in zip(xs, gys, vs, ys, gxs):
        flips = [float(v[j * stride, 0]) < 0.5 for j in range(x.shape[0])]
        assert flips[0] and (len(flips) < 2 or stride == 2 or not flips[1])
        for j, fl in enumerate(flips):
            assert torch.equal(y[j], torch.flip(x[j], dims=[-1]) if fl else x[j])
            assert torch.equal(gx[j], torch.flip(gy[j], dims=[-1]) if fl else gy[j])
    # the identity row copies, through the resampling path (scale and rotate live, s = 1, theta = 0)
    ident = [v.clone() for v in vs]
    for v in ident:
        v[:, 0], v[:, 1], v[:, 2] = 0.75, 0.5, 0.5
    ys, gxs, _ = _run(xs, gys, ident, st, GC.GEO)
    assert all(torch.equal(y, x) for x, y in zip(xs, ys)) and all(torch.equal(g, gy) for gy, g in zip(gys, gxs))
    # p = 0 copies; p = 1 equals the ungated launch; a gate equal to p is dead
    full_y, full_g, _ = _run(xs, gys, vs, st, GC.GEO)
    ys, gxs, _ = _run(xs, gys, vs, st, GC.GEO, gs, torch.zeros(1, device=DEV))
    assert all(torch.equal(y, x) for x, y in zip(xs, ys)) and all(torch.equal(g, gy) for gy, g in zip(gys, gxs))
    ys, gxs, _ = _run(xs, gys, vs, st, GC.GEO, gs, torch.ones(1, device=DEV))
    assert all(torch.equal(a, b) for a, b in zip(ys, full_y)) and all(torch.equal(a, b) for a, b in zip(gxs, full_g))
    dead = [torch.full_like(g, 0.25) for g in gs]
    ys, _, _ = _run(xs, gys, vs, st, GC.GEO, dead, torch.full((1,), 0.25, device=DEV))
    assert all(torch.equal(y, x) for x, y in zip(xs, ys))
    # per clip: the gates' columns 3, 4, 5 select the sub-policy, clip by clip; gates[i] == None leaves a member ungated
    p = 0.5
    ys, gxs, _ = _run(xs, gys, vs, st, GC.GEO, [gs[0], None, gs[2], gs[3]], torch.full((1,), p, device=DEV))
    assert torch.equal(ys[1], full_y[1]) and torch.equal(gxs[1], full_g[1])
    seen = set()
    for k in (0, 2, 3):
        eff = GC.effective_geo(gs[k], p, GC.GEO, xs[k].shape[0], stride)
        seen.update(eff)
        for j, bits in enumerate(eff):
            if bits == 0:
                wy, wg = xs[k][j:j + 1], gys[k][j:j + 1]
            else:
                (wy,), (wg,), _ = _run([xs[k][j:j + 1]], [gys[k][j:j + 1]], [vs[k][j * stride:j * stride + 1]], [1], bits)
            assert torch.equal(ys[k][j:j + 1], wy) and torch.equal(gxs[k][j:j + 1], wg), (k, j, bits)
    assert len(seen) > 1


V1S = [0.0, 0.5, TOP]
V2S = [0.0, 0.25, 0.5, TOP]


@pytest.mark.parametrize('S_', [8, 9])
def test_adjoint_is_the_exact_transpose(S_):
    """The S^2 one-hot frames as clips [S^2, 1, 1, S, S], all rows of v equal: the forward gives the weight matrix W (clip i holds
    column i), the backward on the same one-hot tensors must give W^T BIT FOR BIT — every output pixel that samples an input
    pixel is among that pixel's 5 x 5 candidates and carries the forward's weight. Scale and angle at both ends and in the middle,
    v0 on both sides of 0.5."""
    P = S_ * S_
    hot = torch.eye(P).view(P, 1, 1, S_, S_).contiguous()
    hd = hot.to(DEV).requires_grad_(True)
    for v0, v1, v2 in itertools.product([0.25, 0.75], V1S, V2S):
        v = torch.zeros(P, A.K)
        v[:, 0], v[:, 1], v[:, 2] = v0, v1, v2
        vd = v.to(DEV)
        y, = A.geoaug([hd], [vd], [1], GC.GEO)
        gx, = torch.autograd.grad(y, hd, hd.detach())
        W = y.detach().view(P, P).t().contiguous().cpu()             # W[o, i]: the weight of input pixel i in output pixel o
        WT = gx.view(P, P).cpu()                                     # clip o holds dL/dx for dL/dy = e_o: row o of W
        assert torch.equal(W.view(torch.int32), WT.view(torch.int32)), (S_, v0, v1, v2, int((W != WT).sum()))
        # and W is the restatement's, at the forward's bound with max |x| = 1; no more than four taps per output pixel
        want = GC.augment_geo(hot.double(), v, GC.GEO).view(P, P).t()
        assert float((W.double() - want).abs().max()) <= fwd_bound(S_, 1.0)
        assert int((W != 0).sum(dim=1).max()) <= 4 and float(W.sum()) > 0.3 * P
        if v1 == 0.5 and v2 == 0.5:                                  # identity / mirror: a permutation matrix
            perm = torch.eye(P).view(S_, S_, S_, S_)
            perm = torch.flip(perm, dims=[3]) if v0 < 0.5 else perm
            assert torch.equal(W, perm.reshape(P, P))


def test_member_without_grad_gets_no_backward_work():
    ins = [_inputs(sh, 2) for sh in SHAPES]
    xs, gys, vs = ([i[k] for i in ins] for k in range(3))
    needs = [False, True, False, True]
    calls, members, (ys, gxs, dev_ys) = _counted(lambda: _run(xs, gys, vs, [1] * 4, GC.GEO, needs=needs), GEO_FNS)
    assert calls == {'t2v_geoaug_fwd': 1, 't2v_geoaug_bwd': 1}
    assert members == {'t2v_geoaug_fwd': [4], 't2v_geoaug_bwd': [2]}
    assert [y.requires_grad for y in dev_ys] == needs
    full_y, full_g, _ = _run(xs, gys, vs, [1] * 4, GC.GEO)
    for i in range(4):
        assert torch.equal(ys[i], full_y[i])
        assert torch.equal(gxs[i], full_g[i]) if needs[i] else gxs[i] is None
    # with no live member (the D step's detached clips) there is no backward launch at all
    calls, _, (_, _, dev_ys) = _counted(lambda: _run(xs, gys, vs, [1] * 4, GC.GEO, needs=[False] * 4), GEO_FNS)
    assert calls == {'t2v_geoaug_fwd': 1, 't2v_geoaug_bwd': 0} and not any(y.requires_grad for y in dev_ys)
    # without a geometric bit: no launch, the tensors themselves
    xd = [x.to(DEV) for x in xs]
    calls, _, out = _counted(lambda: A.geoaug(xd, [v.to(DEV) for v in vs], [1] * 4, DA.FULL), GEO_FNS)
    assert calls == {'t2v_geoaug_fwd': 0, 't2v_geoaug_bwd': 0} and all(a is b for a, b in zip(out, xd))


@pytest.mark.parametrize('S_', [9, 16])
def test_parameter_extremes(S_):
    """Rows of v at 0 and at the largest float below 1: the smallest and the largest scale, -30 and +30 degrees, in every
    combination, against the restatement at the derived bounds; every value stays inside the data's range (a convex blend
    with zero fill)."""
    rows = list(itertools.product([0.0, TOP], repeat=3))
    v = torch.zeros(len(rows), A.K)
    for j, r in enumerate(rows):
        v[j, 0], v[j, 1], v[j, 2] = r
    g = torch.Generator()
    g.manual_seed(S_)
    x = torch.rand(len(rows), 2, 3, S_, S_, generator=g) * 2 - 1
    gy = torch.randn(len(rows), 2, 3, S_, S_, generator=g)
    P = A.geo_params(v)
    assert abs(float(P['s'].min()) - 2.0 ** -0.4) < 1e-15 and float(P['theta'].min()) == -A.PI_6 and float(P['theta'].max()) < A.PI_6
    (y,), (gx,), _ = _run([x], [gy], [v], [1], GC.GEO)
    xr = x.double().requires_grad_(True)
    want = GC.augment_geo(xr, v, GC.GEO)
    want_g, = torch.autograd.grad(want, xr, gy.double())
    ey, eg = float((y.double() - want.detach()).abs().max()), float((gx.double() - want_g).abs().max())
    by, bg = fwd_bound(S_, float(x.abs().max())), 25 * fwd_bound(S_, float(gy.abs().max()))
    print('extremes S %d: forward %.3e / %.3e, adjoint %.3e / %.3e' % (S_, ey, by, eg, bg))
    assert ey <= by and eg <= bg
    assert float(y.abs().max()) <= float(x.abs().max()) * (1 + 8 * EPS)
    # the shrunk frame (s = 2^-0.4) shows the zero fill in its corners; the grown one does not
    assert float(y[0, :, :, 0, 0].abs().max()) == 0.0 and float(y[2, :, :, 0, 0].abs().min()) > 0.0


def test_entry_points_refuse_bad_arguments():
    from txt2vid_amd import functional as TF
    from txt2vid_amd._lib import AugMember, MAX_GROUPS
    l, st = TF.lib(), TF._stream()
    x = torch.ones(2, 1, 2, 8, 8, device=DEV)
    y = torch.full_like(x, 7.0)
    v = torch.rand(2, A.K, device=DEV)
    p = torch.ones(1, device=DEV)

    def member(**kw):
        m = dict(x=x.data_ptr(), y=y.data_ptr(), u=v.data_ptr(), N=2, C=1, T=2, S=8, row_stride=1, rows=2, policy=A.GEO)
        m.update(kw)
        return m

    def call(fn, ms, n=None, gates=None, pp=None):
        arr = (AugMember * max(1, len(ms)))()
        for a, m in zip(arr, ms):
            for k, val in m.items():
                setattr(a, k, val)
        return fn(arr, gates, len(ms) if n is None else n, pp, st)
    gates = (ctypes.c_void_p * 1)(v.data_ptr())
    for fn in (l.t2v_geoaug_fwd, l.t2v_geoaug_bwd):
        assert fn(None, None, 1, None, st) < 0
        assert call(fn, [member()], n=0) < 0
        assert call(fn, [member()] * (MAX_GROUPS + 1)) < 0
        for bad in (dict(policy=0), dict(policy=7), dict(policy=9), dict(policy=63), dict(policy=64), dict(policy=-1), dict(x=None),
                    dict(y=None), dict(u=None), dict(y=x.data_ptr()), dict(N=0), dict(C=0), dict(T=0), dict(S=0), dict(row_stride=0),
                    dict(rows=1), dict(row_stride=2)):
            assert call(fn, [member(), member(**bad)]) < 0, bad
        assert call(fn, [member()], gates=gates, pp=None) < 0                      # exactly one of gates / p
        assert call(fn, [member()], gates=None, pp=p.data_ptr()) < 0
    torch.cuda.synchronize()
    assert bool((y == 7).all())                                                   # nothing was launched
    assert call(l.t2v_geoaug_fwd, [member()], gates=gates, pp=p.data_ptr()) == 0
    torch.cuda.synchronize()
    assert not bool((y == 7).any())
    with pytest.raises(ValueError):
        A.geoaug([x] * 9, [v] * 9, [1] * 9, A.GEO)
    with pytest.raises(RuntimeError):
        A.geoaug([x.cpu()], [v], [1], A.GEO)                                      # no CPU fallback
    with pytest.raises(ValueError):
        A.geoaug([x], [v], [1], 'rotation')
    with pytest.raises(ValueError):
        A.geoaug([x], [v], [1], A.GEO, [v], None)
    with pytest.raises(ValueError):
        A.geoaug([x], [v[:, :6]], [1], A.GEO)


# ------------------------------------------------------------------------------------------------ 2. iteration level
def make(cond=False, N=1, M=1, policy=GC.SIX, ada=False):
    if ada:
        parts = TA.make(cond, N, M)
        parts[4].D_aug = policy
        return parts
    return TD.make(cond, N, M, policy)


@pytest.mark.parametrize('cond', [False, True])
@pytest.mark.parametrize('N,M', [(1, 1), (2, 1)])
def test_iterations_vs_oracle_loop(cond, N, M):
    """Three iterations with the six-name policy against the oracle loop with the restatements at the same call sites and draw
    positions: lossD and lossG at the bounds of test_diffaug_gpu.py::test_iterations_vs_oracle_loop (1e-3, then 2e-2 in the third
    iteration)."""
    from txt2vid_amd.gan.trainer import TrainStep
    tokens = TD.tokens_for(B) if cond else None
    ref = GC.oracle_loop(cond, N, M, GC.SIX, tokens=tokens, iters=3)
    gan, optD, optG, losses, prm = make(cond, N, M)
    TD.seed(100)
    for it in range(3):
        x = S.batch().to(DEV)
        c = None
        if cond:
            with torch.no_grad():
                c = gan.cond_encoder.encode(tokens.to(DEV), [8] * B)[2].detach()
        ts = TrainStep(gan, optD, optG, losses, prm, DEV)
        assert ts.aug == 63 and ts.geo == 56
        lD, lG, _, _ = ts.run(x, c)
        lD, lG = float(lD), float(lG)
        tol = 1e-3 if it < 2 else 2e-2
        print('D_aug six %s %d:%d it %d: lossD %.6f (%.6f) lossG %.6f (%.6f)' % ('cond' if cond else 'uncond', N, M, it, lD,
                                                                                ref['lossD'][it], lG, ref['lossG'][it]))
        assert abs(lD - ref['lossD'][it]) < tol * max(1.0, abs(ref['lossD'][it]))
        assert abs(lG - ref['lossG'][it]) < tol * max(1.0, abs(ref['lossG'][it]))


def test_gradient_reaches_the_generator():
    """Through both launches: one backward call of each, a finite gradient that differs from the policy-off one and from the
    colour / translation / cutout one. With flip alone the gradient arriving at every rendered level is exactly the upstream
    gradient, mirrored for the clips whose row says so (level l's clip j reads row j * 2^l)."""
    from txt2vid_amd.models.tganv2.gen import MultiScaleGen
    gen = TD.pour(MultiScaleGen(width=64, height=64, num_channels=1)).train()
    g = torch.Generator()
    g.manual_seed(9)
    z = torch.randn(B, 256, generator=g).to(DEV)
    u = torch.rand(B, A.K, generator=g)
    v = torch.rand(B, A.K, generator=g)
    v[:, 0] = torch.tensor([0.1, 0.9, 0.3, 0.7])
    ws = None
    grads = {}
    for policy in ('', DA.FULL, GC.SIX, 'flip'):
        gen.zero_grad()
        TD.seed(5)
        fake = gen(z)
        if ws is None:
            ws = [torch.randn(*f.shape, generator=g) + 3.0 for f in fake]
        for f in fake:
            f.retain_grad()
        strides = [2 ** l for l in range(len(fake))]

        def run():
            out = A.geoaug(fake, [v.to(DEV)] * len(fake), strides, policy)
            out = A.diffaug(out, [u.to(DEV)] * len(fake), strides, policy)
            sum((o * w.to(DEV)).sum() for o, w in zip(out, ws)).backward()
        calls, _, _ = _counted(run, GEO_FNS + OLD_FNS[:2])
        bits = A.parse_policy(policy)
        assert calls == {'t2v_geoaug_fwd': int(bool(bits & 56)), 't2v_geoaug_bwd': int(bool(bits & 56)),
                         't2v_diffaug_fwd': int(bool(bits & 7)), 't2v_diffaug_bwd': int(bool(bits & 7))}
        grads[policy] = gen.fc.weight.grad.detach().clone()
        assert bool(torch.isfinite(grads[policy]).all())
        if policy == 'flip':
            for l, (f, w) in enumerate(zip(fake, ws)):
                for j in range(f.shape[0]):
                    want = torch.flip(w[j], dims=[-1]) if float(v[j * 2 ** l, 0]) < 0.5 else w[j]
                    assert torch.equal(f.grad[j].cpu(), want), (l, j)
    for a, b in ((GC.SIX, ''), (GC.SIX, DA.FULL), ('flip', '')):
        rel = float((grads[a] - grads[b]).norm() / grads[b].norm())
        print('fc.weight gradient, %r vs %r: relative difference %.3e' % (a, b, rel))
        assert rel > 1e-3


def test_graph_replay_matches_eager():
    """GraphedTrainStep with the six-name policy (the geometric blocks among the device-resident draws, the launches inside the ONE
    captured graph) reproduces the eager iterations: 2 eager, then capture + replays. Tolerances of
    test_diffaug_gpu.test_graph_replay_matches_eager."""
    from txt2vid_amd.gan.trainer import TrainStep, GraphedTrainStep
    gan, optD, optG, losses, prm = make(N=1, M=2)
    TD.seed(6)
    eager = []
    for x in TD.batches():
        lD, lG, _, _ = TrainStep(gan, optD, optG, losses, prm, DEV).run(x, None)
        eager.append((float(lD), float(lG)))
    gan, optD, optG, losses, prm = make(N=1, M=2)
    TD.seed(6)
    gs = GraphedTrainStep(gan, optD, optG, losses, prm, DEV, (B, 1, 16, 64, 64), warmup=2)
    assert gs.draws.n_aug == 2 * 1 + 2 + 1 and gs.draws.n_geo == 2 * 1 + 2 + 1 and not gs.draws.gated
    for i, x in enumerate(TD.batches()):
        lD, lG = gs.step(x)
        got = (float(lD), float(lG))
        print('D_aug six step %d (%s): %s vs eager %s' % (i, 'replay' if i >= 2 else 'eager', got, eager[i]))
        tol = 2e-5 if i < 2 else 2e-3
        assert all(abs(a - b) < tol for a, b in zip(got, eager[i])), (i, got, eager[i])
    assert gs.graphs is not None and gs.n_graphs == 1


def test_p_is_read_at_run_time():
    """One gated forward captured in a graph; replayed with p = 0 and, after p is overwritten ON THE DEVICE, with p = 1: the copy
    becomes the transformation. No re-capture."""
    x, _, v, gates = _inputs(SHAPES[1], 3)
    xd, vd, gd = x.to(DEV), v.to(DEV), gates.to(DEV)
    (full,), _, _ = _run([x], [x], [v], [1], GC.GEO, needs=[False])
    p = torch.zeros(1, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        A.geoaug([xd], [vd], [1], GC.GEO, [gd], p)                  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y, = A.geoaug([xd], [vd], [1], GC.GEO, [gd], p)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y.cpu(), x)
    p.copy_(torch.ones(1, device=DEV))                              # device to device
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y.cpu(), full) and not torch.equal(full, x)
    p.copy_(torch.full((1,), 0.5, device=DEV))
    graph.replay()
    torch.cuda.synchronize()
    want = GC.augment_geo(x.double(), v, GC.GEO, 1, gates, 0.5)
    assert float((y.cpu().double() - want).abs().max()) <= fwd_bound(16, float(x.abs().max()))


# ------------------------------------------------------------------------------------------------ 3. budget; off means off
@pytest.mark.parametrize('ada', [False, True])
@pytest.mark.parametrize('N,M', [(1, 1), (2, 2)])
def test_launch_budget(N, M, ada):
    """Six-name policy, 4 levels: N + M more forward launches and M more backward launches per iteration, one per existing
    augmentation launch, over the same members (real + generated pyramid = 8; a later G step augments the generated pyramid only;
    the backward covers the 4 generated members). The old launches keep their counts: the ungated pair without --D_ada, the gated
    pair with it. Counted over the 2 eager + 1 captured pass of a graphed run (the replay itself makes no call)."""
    calls, members, _ = _counted(lambda: TD._three_graphed_iterations(make(N=N, M=M, ada=ada)), GEO_FNS + OLD_FNS)
    old = ('t2v_diffaug_gated_fwd', 't2v_diffaug_gated_bwd') if ada else ('t2v_diffaug_fwd', 't2v_diffaug_bwd')
    want = dict.fromkeys(GEO_FNS + OLD_FNS, 0)
    want.update({'t2v_geoaug_fwd': 3 * (N + M), 't2v_geoaug_bwd': 3 * M, old[0]: 3 * (N + M), old[1]: 3 * M})
    assert calls == want
    assert members['t2v_geoaug_fwd'] == members[old[0]] == ([8] * (N + 1) + [4] * (M - 1)) * 3
    assert members['t2v_geoaug_bwd'] == members[old[1]] == [4] * (3 * M)


def _parent_augment(self, real, fake):
    """TrainStep._augment as it stood before the geometric names existed, word for word: the unchanged code path."""
    from txt2vid_amd import functional as TF
    if not self.aug:
        return real, fake
    from txt2vid_amd.functional_aug import diffaug
    xs, us, gs, strides = [], [], [], []
    for clips in (real, fake):
        if clips is None:
            continue
        if self.gated:
            u, g = TF.draws.aug(self._batch, self.device, gated=True)
        else:
            u, g = TF.draws.aug(self._batch, self.device), None
        for l, t in enumerate(clips):
            xs.append(t)
            us.append(u)
            gs.append(g)
            strides.append(2 ** l if self.params.subsample_input else 1)
    out = diffaug(xs, us, strides, self.aug, gs, self._p) if self.gated else diffaug(xs, us, strides, self.aug)
    n = len(real) if real is not None else 0
    return (out[:n] if real is not None else None), (out[n:] if fake is not None else None)


def _three_eager_iterations(parts):
    from txt2vid_amd.gan.trainer import TrainStep
    gan, optD, optG, losses, prm = parts
    TD.seed(100)
    out = []
    for x in TD.batches(3):
        lD, lG, _, _ = TrainStep(gan, optD, optG, losses, prm, DEV).run(x, None)
        out.append((float(lD), float(lG)))
    return out


@pytest.mark.parametrize('policy', [DA.FULL, TD.NO_ATTR])
def test_off_means_off(policy, monkeypatch):
    """With --D_aug color,translation,cutout, and with no --D_aug, the new entry points are never called, eagerly or while
    capturing, n_geo == 0, and the losses of three iterations equal bit for bit those of the same run made through the unchanged
    code path (the parent's _augment, which knows neither the geometric block nor the new launch)."""
    from txt2vid_amd.gan.trainer import GraphedTrainStep, TrainStep
    TD._one_eager_iteration(TD.make(policy=policy))                                  # burn-in
    calls, _, here = _counted(lambda: _three_eager_iterations(TD.make(policy=policy)), GEO_FNS)
    assert calls == dict.fromkeys(GEO_FNS, 0)
    calls, _, graphed = _counted(lambda: TD._three_graphed_iterations(TD.make(policy=policy)), GEO_FNS)
    assert calls == dict.fromkeys(GEO_FNS, 0)
    gs = GraphedTrainStep(*TD.make(policy=policy), DEV, (B, 1, 16, 64, 64), warmup=2)
    assert gs.draws.n_geo == 0 and not gs.draws.geo and gs.ts.geo == 0
    assert gs.draws.n_aug == (4 if policy is not TD.NO_ATTR else 0)
    monkeypatch.setattr(TrainStep, '_augment', _parent_augment)
    parent = _three_eager_iterations(TD.make(policy=policy))
    print('policy %r: %r | parent path %r' % (policy if policy is not TD.NO_ATTR else None, here, parent))
    assert here == parent and all(np.isfinite(v) for pair in here for v in pair)
    monkeypatch.undo()
    if policy is DA.FULL:                      # on: the six-name policy calls them and changes the iteration
        calls, _, on = _counted(lambda: _three_eager_iterations(TD.make(policy=GC.SIX)), GEO_FNS)
        assert calls == {'t2v_geoaug_fwd': 6, 't2v_geoaug_bwd': 3} and on != here


# ------------------------------------------------------------------------------------------------ 4. command line
def _cli(args, ok=True):
    p = subprocess.run([sys.executable, '-m', 'txt2vid_amd.train.gan'] + TA.BASE + args, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=600)
    out = p.stdout.decode(errors='replace')
    assert (p.returncode == 0) == ok, out[-3000:]
    return out


def test_cli_train_checkpoint_resume_and_sample(tmp_path):
    flags = ['--D_aug', GC.SIX, '--D_ada', '0.6']
    out = ['--out', str(tmp_path / 'a'), '--out_samples', str(tmp_path / 'a_s')]
    log = _cli(out + flags + ['--D_aug_p', '0.5', '--max_iters', '3', '--save_model_period', '3'])
    assert 'HIP-graph replay' in log and 'Iter 3, Loss_D' in log
    m = re.search(r'Iter 3, Loss_D: ([-0-9.naninf]+) Loss_G: ([-0-9.naninf]+)', log)
    assert m and all(np.isfinite(float(t)) for t in m.groups()), log[-1500:]
    ck, = glob.glob(os.path.join(str(tmp_path / 'a'), 'iter_3_lossG_*'))
    sd = torch.load(ck, map_location='cpu', weights_only=False)
    # no new keys: the checkpoint of a run with --D_aug color,translation,cutout --D_ada has the same ones
    out_b = ['--out', str(tmp_path / 'b'), '--out_samples', str(tmp_path / 'b_s')]
    _cli(out_b + ['--D_aug', DA.FULL, '--D_ada', '0.6', '--D_aug_p', '0.5', '--max_iters', '3', '--save_model_period', '3'])
    ck_b, = glob.glob(os.path.join(str(tmp_path / 'b'), 'iter_3_lossG_*'))
    sd_b = torch.load(ck_b, map_location='cpu', weights_only=False)
    assert sorted(sd.keys()) == sorted(sd_b.keys()) and sorted(sd['ada'].keys()) == sorted(sd_b['ada'].keys())
    assert not torch.equal(sd['gen']['fc.weight'], sd_b['gen']['fc.weight'])      # the names did change the training
    # resume with the flags, eagerly this time
    out_c = ['--out', str(tmp_path / 'c'), '--out_samples', str(tmp_path / 'c_s')]
    log = _cli(out_c + flags + ['--weights', ck, '--max_iters', '2', '--save_model_period', '1000', '--no_graph'])
    assert 'Iter 2, Loss_D' in log and 'HIP-graph replay' not in log
    # sampling never augments: the same files with and without the flag
    files = {}
    for name, extra in (('t_on', ['--D_aug', GC.SIX]), ('t_off', [])):
        smp = str(tmp_path / name)
        _cli(['--out', str(tmp_path / 'c'), '--out_samples', smp, '--test', '--weights', ck, '--num_samples', '1', '--max_iters', '1']
             + extra)
        files[name] = {os.path.basename(f): open(f, 'rb').read() for f in sorted(glob.glob(os.path.join(smp, '*')))}
        assert 'real_0.png' in files[name] and '64x64_0_0.jpg' in files[name]
    assert files['t_on'] == files['t_off']
    log = _cli(['--D_aug', 'flip,rotation', '--max_iters', '1'], ok=False)
    assert '--D_aug' in log
